// kernels.h — launch wrappers for the gfx950 kernels of the VAMP hot path
// (internal to libvampomi; the public boundary is include/vampomi.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

namespace vk {

constexpr int kMaxRhs = 4;     // right-hand sides sharing one pass over X
constexpr int kMaxL = 64;      // mixture components (VAMPOMI_MAX_L)
constexpr int kMaxTerms = 12;  // dot-product terms per reduction launch
constexpr int kRedBlocks = 1024;  // max partial blocks of a reduction

struct CPtrs { const double* p[kMaxRhs]; };
// optional HIP events recorded by a launch's own dispatch (hipExtLaunchKernelGGL)
struct Timing { hipEvent_t start = nullptr, stop = nullptr; };
// Destination of a fused two-stage reduction (see red_finish in kdev.h):
// per-block partials in part, the final sums in out[0..nq) (device memory or
// mapped host memory), ticket a zeroed device counter the kernel re-arms;
// flag (may be null): the last block stores seq there (system scope, after out);
// gate (may be null): the launch does nothing while *gate == 0;
// out2 (may be null): results q >= split go to out2[q - split] instead (one
// launch serving two slot ranges, DotBatch::add_many)
struct RedOut {
    double* part;
    double* out;
    unsigned* ticket;
    unsigned long long* flag = nullptr;
    unsigned long long seq = 0;
    const int* gate = nullptr;
    double* out2 = nullptr;
    int split = 0;
};
struct Ptrs { double* p[kMaxRhs]; };

// The device-resident marker shard: M columns (markers) of N samples, column
// stride ld >= N elements (ld % 16 == 0, pad rows zero), plus marker stats.
// The elements are doubles, floats with f32 set (VAMPOMI_STORE_F32), or 16-bit
// fixed point with u16 set (VAMPOMI_STORE_U16: uint16_t k, value k * 2^-16):
// every kernel that reads X has an entry point per element type (the narrow
// ones with an _f32 / _u16 suffix) over one body; a lane owns the same rows in
// every case and widens what it loads (exactly), so all storages sum in the
// same order.
// The element kind where a plain int names it (kernel names, occupancy,
// gen_markers, stream_read): kXF64, kXF32, kXU16.
enum { kXF64 = 0, kXF32 = 1, kXU16 = 2 };
inline const char* xe_suffix(int ek) { return ek == kXU16 ? "_u16" : ek == kXF32 ? "_f32" : ""; }
struct Shard {
    const void* X;
    int64_t ld, N, M;
    const double* mave;
    const double* msig;
    int f32 = 0;
    int u16 = 0;
    const double* x64() const { return static_cast<const double*>(X); }
    const float* x32() const { return static_cast<const float*>(X); }
    const uint16_t* x16() const { return static_cast<const uint16_t*>(X); }
    int ek() const { return u16 ? kXU16 : f32 ? kXF32 : kXF64; }
};

// ---- A.x : two-stage, deterministic --------------------------------------
// Stage 1 (ax_partial): the (row tile, marker) segments are split into equal
// shares, one per workgroup (two per CU): a fixed fraction of one or two
// tiles in every marker band (band plan), or a contiguous tile-major stripe;
// each tile a workgroup touches gets its own partial slot, written to
// part[slot][k][ld].  Stage 2 (ax_reduce): sums every tile's slots in order.
struct AxPlan {
    int variant;      // row/unroll variant (tuning table in kernels.hip)
    int64_t rows;     // rows per tile
    int64_t tiles;    // ceil(N / rows)
    int64_t total;    // tiles * M segments
    int64_t span;     // stripe plan: segments per workgroup
    int64_t nband;    // band plan: marker bands (0: stripe plan)
    int64_t sa, sb;   // tile t's first slot-owning workgroup is t*sa/sb
    int groups;       // workgroups (grid)
    int nslots;       // partial slots of the busiest tile (part holds nslots x kMaxRhs x ld)
    // team plan (variant kAxTeam, ax_team_kernel): T workgroups per team split
    // the rows (TR each, S loads per lane per column), every team a full
    // N-vector slot over its interleaved columns; one tile of N rows (sa =
    // nslots teams, sb = 1).  T = 0: the tile plans above
    int T = 0, TR = 0, S = 0;
};
// partial slots tile t uses: the workgroups whose share meets it
inline int64_t ax_slots(const AxPlan& p, int64_t t) { return ((t + 1) * p.sa - 1) / p.sb - (t * p.sa) / p.sb + 1; }
// Kernel variants (tuning tables in kernels.hip) are per-context launch
// settings: the defaults are the measured winners, other values are
// development hooks (tools/kbench.py, vampomi_dev_set_variant).
// kAxDefault: the team plan where it has teams of >= kAxTeamMinT (N above
// ~16k rows: C3/C4/C5; 3.7-3.8 % faster than the best tile plan there,
// profiles/r05s_lockstep_ab.txt), else variant 0 (C2 keeps its bits)
constexpr int kAxDefault = -1, kAxTeam = 7, kAxTeamMinT = 8, kAtxDefault = -1 /* per-K choice */, kLooDefault = 16;
AxPlan ax_plan(int64_t N, int64_t M, int variant = kAxDefault);
AxPlan ax_plan_for(int64_t N, int64_t M, int cus, int variant);  // (ax_plan on `cus` compute units)
int ax_variant_count();
bool ax_variant_ok(int v);
int atx_variant_count();
bool atx_variant_ok(int v);
// Optional fusion into the A.x pass (the CG direction update of the previous
// step): with z set, the pass multiplies x_k = z_k + beta[k]*p_k, where
// p_k is the `x` argument (every consumer of the new direction forms it the
// same way; cg_update stores it).  gate (may be null): no work while *gate == 0.
struct AxFuse {
    CPtrs z{};
    const double* beta = nullptr;  // device
    const int* gate = nullptr;
};
hipError_t ax_partial(const Shard& s, const AxPlan& pl, int K, CPtrs x, double* part, hipStream_t st,
                      const Timing& tm = Timing{}, const AxFuse& fu = AxFuse{});
// A pure read stream of x[0, n) (the read ceiling, vampomi_dev_read_ceiling):
// kind 0 lockstep 8-wave workgroups (cus of them), kind 1 a 1 MiB chunk per
// wave; returns the bytes read in *bytes (whole units of 1024 / 2^17
// elements).  ek (kXF64 / kXF32 / kXU16) is x's element kind: floats are read
// with the 8-byte loads of the fp32 kernels; 16-bit elements with 16-byte loads
// over the resident bytes (a pure read is tied to no summation order, so it
// need not keep the operators' rows per lane; n a multiple of 8 elements).
// Either way the ceiling of the bytes actually resident
hipError_t stream_read(const void* x, int ek, int64_t n, int kind, int cus, hipStream_t st, const Timing& tm,
                       double* sink, double* bytes);
// the team plan (atax_team.hip): false if N has none (rows per member past 4
// loads per lane of 1024-row steps at every team size)
bool ax_team_plan(int64_t N, int64_t M, int cus, AxPlan* out);
hipError_t ax_team(const Shard& s, const AxPlan& pl, int K, CPtrs x, double* part, hipStream_t st, const Timing& tm,
                   const AxFuse& fu);
std::string ax_kernel_name(int K, bool fused, const AxPlan& pl, int ek = 0);  // as rocprofv3 prints it
// out_k[j] = sum_c part[c][k][j]; if div > 0 then out_k[j] /= div
hipError_t ax_reduce(const AxPlan& pl, int K, int64_t N, int64_t ld, const double* part, Ptrs out,
                     double div, hipStream_t st, const int* gate = nullptr);
// out_k[j] /= div (after the cross-rank all-reduce)
// v_k / div into dst_k (dst null: in place)
hipError_t vec_div(int K, int64_t n, int64_t ld, Ptrs v, double div, hipStream_t st, const Ptrs* dst = nullptr);

// ---- A^T.u : one wave per group of markers --------------------------------
// mode 0: out_k[i] = (msig_i * dot_k(i)) * scale
// mode 1 (lmmse_mult): out_k[i] = ((msig_i*dot)*scale)*tau + gam2*p_k[i]
// (<out_k, p_k> is a separate fixed-geometry reduction); gate as in AxFuse
int atx_blocks(int64_t M, int K, int variant);
std::string kernel_name(int which, int K, int mode, int variant, int ek = 0);  // as rocprofv3 prints it
// zf/beta (mode 1, may be null): the epilogue's p_k is zf_k + beta[k]*p_k;
// sraw (mode 1, may be null): also stores the raw product (msig_i*dot)*scale
hipError_t atx(const Shard& s, int K, CPtrs u, Ptrs out, double scale, int mode, double tau,
               double gam2, CPtrs p, hipStream_t st, int variant = kAtxDefault, const Timing& tm = Timing{},
               const int* gate = nullptr, CPtrs zf = CPtrs{}, const double* beta = nullptr, Ptrs sraw = Ptrs{});

// ---- one-pass CG operator: A^T q and A d from ONE read of X ----------------
// A CG step needs d = tau*A^T(A p) + gam2*p.  With q = A p carried as an
// N-vector recurrence (q = A r/diag + beta*q_old, A r -= alpha*A d), the pass
// over X computes, per marker i, t_i = (msig_i*sum_j (X_ij - mave_i) q_j)/sqrt(N)
// and d_i = tau*t_i + gam2*p_i, and while the column is still in registers
// accumulates (A d)_j += (X_ij - mave_i)*(msig_i*d_i): A^T and A in one read.
// Two kernels:
//  * T = 0 (atax_kernel, kernels.hip): one workgroup per CU owns whole
//    columns, q in LDS, so K*N <= 20,000;
//  * T >= 1 (atax_team_kernel, atax_team.hip): teams of T workgroups split
//    the rows of each column and hand the column dots over inside the launch
//    (T = 1: no hand-off), for N up to 32 x 8 x 896 rows.
constexpr int kOpMaxK = 2;
// A team launch on a 3-system plan (team_sys3_plan) carries kOpMaxK CG systems
// and, in a third slot, the alternate system of OpAlt (diag = tau = 1,
// gam2 = 0, no fused direction update, no <d,p>): K = kOpSys.  Its d is
// OpAlt.d and its A d partials are slot kOpMaxK of each team.
constexpr int kOpSys = kOpMaxK + 1;
// the head-start launch (pcg.cpp): one operator system plus kOpPlain plain
// right-hand sides A x_kp from the same read of X (stats: K = 1 + kOpPlain)
constexpr int kOpPlain = 3;
struct OpPlan {
    int grid;       // workgroups (at most one per CU)
    int S;          // 16-byte loads per lane per column
    int64_t nslots; // partial A d slots (nslots x kMaxRhs x ld): workgroups (T = 0) or teams
    int T = 0;      // team size (0: the whole-column kernel)
    int TR = 0;     // rows per team member (T >= 1)
    int cfg = 0;    // team kernel configuration (prefetch, lag, polls in flight)
};
// variant: -1 the default choice for N; 0 the whole-column kernel; T*10 + cfg (cfg < 10) or 1000 + T*100 + cfg
// a team plan (development hook, tools/kbench.py)
constexpr int kOpDefault = -1;
bool op_plan(int64_t N, int64_t M, int cus, int variant, OpPlan* out);
bool op_supported(int64_t N, int K);
bool team_plan(int64_t N, int64_t M, int cus, int T, int cfg, OpPlan* out);
// the team kernel's dynamic LDS for plan pl with K operator systems (the one
// layout its launches and team_plan use, atax_team.hip tm_lds), in doubles:
// out[0] head words, [1] q offset, [2] q stride, [3] partials offset,
// [4] totals offset, [5] total words; false: pl is not a team plan
bool team_lds_layout(const OpPlan& pl, int64_t N, int K, int64_t out[6]);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device):
// bit d of done is device d; a failure is returned, never left pending
hipError_t lds_allow(const void* kern, std::atomic<unsigned long long>& done, int bytes);
struct CgState;
struct CgMirror;
// Several ranks (pcg.cpp): the previous CG step's decision (cg_decide on its
// all-reduced sums red) formed by the operator launch that needs its beta,
// instead of by a launch of its own between the all-reduce and this one: every
// workgroup decides from src (the same arithmetic, the same bits), workgroup 0
// stores the new state to dst (a second state: src is still being read) and
// publishes it (mirror / flag, as cg_decide); the launch then runs on the new
// beta, gated on its "any".  on = 0: a.beta and the gate as given
struct OpFold {
    const CgState* src = nullptr;
    CgState* dst = nullptr;
    const double* red = nullptr;
    int on = 0, it = 0, mask = 0xf, pack = 0;
    CgMirror* mirror = nullptr;
    unsigned long long* flag = nullptr;
    unsigned long long seq = 0;
};
// The pre-step (pcg.cpp; one rank): an operator slot whose own system has
// stopped carries the products T1 = A^T A b and A T1 of the NEXT Onsager
// solve's right-hand side b instead of a discarded step.  Offered with cs set:
// the launch's slot k = the lowest k < K with cs->active[k] == 0, if there is
// one and *done != token (no pre-step made in this solve yet), runs with
// ar_k = ar, p_k = p, d_k = d (= sraw_k), diag = tau = 1, gam2 = 0 and its
// fuse bit cleared; its <d,p> means nothing.  Every workgroup reads the same
// state (only cg_update's last block, after the launch, writes cs and done)
struct OpAlt {
    const CgState* cs = nullptr;
    const unsigned long long* done = nullptr;
    unsigned long long token = 0;
    const double* ar = nullptr;  // A b (N-space, replicated)
    const double* p = nullptr;   // any finite M-vector (b)
    double* d = nullptr;         // T1 (M)
    // filled by the launch (atax_team): slot k's pointers and scalars as the
    // kernel reads them, k < K from OpArgs, entry kOpMaxK the alternate's (one
    // indexed read per value instead of two candidates held in registers)
    struct Slot {
        const double* ar;
        const double* p;
        double* d;
        double* sraw;
        double diag, tau, gam2;
    };
    Slot tab[2 + 1];  // kOpMaxK + 1
};
struct OpArgs {
    CPtrs ar, qo;       // q_k = ar_k/diag [+ beta_k*qo_k when fuse] (N-space, replicated)
    CPtrs p, z;         // p_k [= z_k + beta_k*p_k when fuse] (M-space)
    const double* beta; // device (CgState.beta)
    int fuse;           // bit k: system k's direction update p = z + beta p is fused into this launch
    double diag, scale, tau, gam2;
    Ptrs d, sraw;       // d_k (M); sraw_k = t_k (may be null)
    CPtrs px;           // head-start launch only: the kOpPlain plain right-hand sides (M), A x_kp into
                        // partial slots 1 .. kOpPlain
    double* part;       // nslots x kMaxRhs x ld partial A d (before the sum over slots)
    RedOut ro;          // <d_k, p_k> summed over the shard (K values)
    // team kernel with T > 1: hand-off granules ((M + grid) x kOpMaxK x T x 2
    // words, then 2 x kOpMaxK dummy words per workgroup, then one XCD word per
    // workgroup; kOpSys in place of kOpMaxK for a launch with K = kOpSys, which
    // lays the same block out for three systems: every 8-byte word of the block
    // carries its launch's tag in its high half under either layout; zeroed once), this launch's
    // tag (never 0, new every launch) and a mapped host word set when a
    // hand-off timed out
    unsigned long long* xg;
    unsigned tag;
    unsigned* err;
    unsigned long long* ts;  // experiment builds (TM_TS=1) only: per workgroup {start, end, XCC id, HW id}
    int dbg;  // timing experiments only (VAMPOMI_OP_DBG; results are wrong when set, except bit 5):
              // bit 0 no poll waits, 1 no publishes, 2 no butterfly, 3 no A d accumulation,
              // 5 write-through hand-off even when the team shares an XCD, 11 no LDS q reads,
              // 12 no hand-off work (the hand-off wave only keeps the step barriers)
    OpFold fold;  // team kernels only (atax_team.hip)
    OpAlt alt;    // team kernels only, never with fold.on or plain right-hand sides; K = kOpSys: the third
                  // slot's system (ar, p, d), cs null
};
static_assert(sizeof(OpAlt::tab) / sizeof(OpAlt::Slot) == kOpMaxK + 1, "one entry per system and the alternate's");
std::string op_kernel_name(int K, const OpPlan& pl, int ek = 0);
std::string team_kernel_name(int K, const OpPlan& pl, int ek = 0);
// workgroups of the team kernel of plan pl (T >= 1) with K right-hand sides one
// CU holds at once (0: it cannot run); a plan needs grid <= this x CUs, since
// a team launch needs all its workgroups resident together (ek: of that
// element kind's entry point)
int team_occupancy(const OpPlan& pl, int K, int ek = 0);
hipError_t atax(const Shard& s, const OpPlan& pl, int K, const OpArgs& a, hipStream_t st, const Timing& tm = Timing{},
                const int* gate = nullptr);
hipError_t atax_team(const Shard& s, const OpPlan& pl, int K, const OpArgs& a, hipStream_t st, const Timing& tm,
                     const int* gate);
// the head-start launch: the team kernel with K = 1 and the kOpPlain plain
// right-hand sides a.px (plan from team_plain_plan)
hipError_t atax_team_plain(const Shard& s, const OpPlan& pl, const OpArgs& a, hipStream_t st, const Timing& tm,
                           const int* gate);
// a team plan for the head-start kernel (the main plan's team size if its rows
// fit, else larger teams); false: none (the solve starts without a head start)
bool team_plain_plan(int64_t N, int64_t M, int cus, const OpPlan& main, OpPlan* out);
// a team plan for launches with K = kOpSys systems: the main plan's team size
// (at least 2, at most 16: the hand-off wave sums three systems in groups of
// 16 lanes) if three accumulator sets fit the registers at its rows per
// member, else larger teams.  A function of (N, M, cus, main) only, so every
// storage of X has the same one.  false: none
bool team_sys3_plan(int64_t N, int64_t M, int cus, const OpPlan& main, OpPlan* out);
// whether pl can launch with K = kOpSys (a plan team_sys3_plan may return)
bool team_sys3_ok(const OpPlan& pl);
// out_k[j] = sum_b part[b][k0 + k][j] (slots in order); if div > 0 then /= div
hipError_t op_reduce(const OpPlan& pl, int K, int64_t N, int64_t ld, const double* part, Ptrs out, double div,
                     hipStream_t st, const int* gate = nullptr, int k0 = 0);

// ---- marker statistics (data::compute_markers_statistics) ----------------
// (of the stored values, accumulated in fp64; s.mave / s.msig are not read)
hipError_t marker_stats(const Shard& s, double nonas, double alpha_scale, double* mave, double* msig,
                        hipStream_t st);

// ---- synthetic data --------------------------------------------------------
// (ek kXF32: X holds floats and receives the generator's value rounded to
// nearest even; kXU16 is not generated in place: the engine quantises staged
// fp64 chunks, convert_cols)
hipError_t gen_markers(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M, void* X, int ek,
                       hipStream_t st);
// ---- ingest and read-back (ingest.hip): the element conversions ---------------
// What convert_cols and na_ingest_cols have seen of the entries they quantised
// since the record was zeroed (device memory, 4 words): every field is an
// integer sum, a minimum or a maximum, so none depends on the order the
// launches' threads ran in.
struct QuantRec {
    unsigned long long rejected;  // entries that are NaN, infinite, < 0 or > 1
    unsigned long long first;     // the smallest index (col0 + c) * nfile + row of a rejected entry (~0: none)
    unsigned long long clamped;   // accepted entries that rounded to 65536 and were stored as 65535
    unsigned long long max_err;   // max |k * 2^-16 - x| over the accepted entries, as the bits of that double
};
// dst[c*ldd + j] = conv(src[c*lds + row(j)]), j < n, c < ncols: a chunk of
// columns of nfile elements (lds >= nfile; a staged chunk's are packed, so a
// column is only as aligned as its element) into columns of stride ldd.
// rows == nullptr: n == nfile and row(j) = j; else row(j) = rows[j], n
// ascending device indices in [0, nfile) (a row subset), and the stored bits
// are those of the conversion of the chunk with the other rows taken out
// beforehand.  src_ek / dst_ek (kXF64 / kXF32 / kXU16; a 16-bit element is a
// uint16_t k, value k * 2^-16) pick conv:
//   double -> float            nearest even
//   float -> double            exact
//   16 bits -> double, float   k * 2^-16, exact
//   double, float -> 16 bits   min(65535, rint(x * 65536)) (ties to even; the
//       product is exact; a float is widened first) for 0 <= x <= 1 (-0.0 is
//       0); any other entry stores 0 and is counted in *rec, its index
//       (col0 + c) * nfile + row(j) (col0: the index of column 0)
//   the kinds agree            a copy
// rec is not read for the other conversions
hipError_t convert_cols(const void* src, int src_ek, int64_t lds, const int32_t* rows, int64_t n, int64_t ncols,
                        void* dst, int dst_ek, int64_t ldd, int64_t nfile, int64_t col0, QuantRec* rec,
                        hipStream_t st);
// ---- missing values (NaN): the column-wise ingest ----------------------------
// What na_ingest_cols has seen since the record was zeroed (first: all ones):
// integer sums and a minimum, so none depends on the order anything ran in.
struct NaRec {
    unsigned long long missing;  // NaN entries among the kept rows
    unsigned long long first;    // the smallest index (col0 + c) * nfile + row of one (~0: none)
    unsigned long long markers;  // columns with at least one
    unsigned long long masked;   // columns stored as zeros (kNaMean)
};
enum { kNaFatal = 1, kNaMean = 2 };  // (VAMPOMI_NA_FATAL / VAMPOMI_NA_MEAN)
// convert_cols' conversions of a staged chunk of doubles or floats (src_ek
// kXF64 / kXF32) with a NaN policy; rows, n and nfile as convert_cols takes
// them.  One workgroup per column, two sweeps:
//   1. the NaNs among the kept rows are counted (cnt[c], and *nrec) and the
//      other kept entries summed in fp64: thread t adds rows t, t + 256, ...
//      in that order, each wave's 64 sums are folded by wave_sum's butterfly,
//      and the four wave sums added in wave order.  The order depends on n and
//      on which rows are NaN, on nothing else.
//   2. kNaMean: each kept entry is stored as conv(x), a NaN as conv(s / n_obs);
//      a column with n_obs == 0 or (double)n_missing > max_frac * (double)n is
//      stored as zeros.  Into kXU16 the observed entries (a masked column's
//      too) go through *qrec as in convert_cols; the fill and the zeros do not.
//      kNaFatal: the same for a column without NaN; a column with one is not
//      stored (the load fails).
// cnt: ncols device counters (the chunk's slice of the shard's)
hipError_t na_ingest_cols(const void* src, int src_ek, int64_t lds, const int32_t* rows, int64_t n, int64_t ncols,
                          void* dst, int dst_ek, int64_t ldd, int64_t nfile, int64_t col0, int mode, double max_frac,
                          int64_t* cnt, NaRec* nrec, QuantRec* qrec, hipStream_t st);
// ---- covariate adjustment: the residual of each column on an orthonormal basis ---
// src: an fp64 work block of ncols packed columns of n rows (what convert_cols
// or na_ingest_cols leaves with dst_ek = kXF64, ldd = n); Q: n x R doubles on
// the device, column-major and packed, orthonormal (R <= kAdjMaxR).  Per column
// c = Q^T x, r = x - Q c in fp64, stored as dst[col*ldd + j] = (XD)r_j (dst_ek
// kXF64 or kXF32: one rounding); a column with ||r||^2 <= 1e-20 ||x||^2 is
// stored as zeros, flags[col] = 1 (else 0) and *absorbed is incremented.  The
// sums run in an order that depends on n and R alone (ingest.hip), so a
// column's stored bits depend on neither the chunk nor the columns beside it.
constexpr int kAdjMaxR = 65;  // VAMPOMI_MAX_C + 1: the intercept and every covariate
hipError_t adjust_cols(const double* src, int64_t n, int64_t ncols, const double* Q, int R, void* dst, int dst_ek,
                       int64_t ldd, uint8_t* flags, unsigned long long* absorbed, hipStream_t st);
// beta_i = gauss(seed) for causal markers (uniform < lam), else 0; the count
// of causal markers in ro.out[0]
hipError_t gen_beta(uint64_t seed, double lam, int64_t S, int64_t M, double* beta, const RedOut& ro, hipStream_t st);
hipError_t scale_vec(int64_t n, double* v, double a, hipStream_t st);
// y_j = y_j + sqrt1mh2 * gauss(seed, noise stream, j)
hipError_t add_noise(uint64_t seed, int64_t N, double sd, double* y, hipStream_t st);

// ---- reductions --------------------------------------------------------------
// PUPD: a . (c + *beta * b) (a CG step's <d, p> with p = z + beta p fused);
// SQPUPD: (c + *beta * b)^2 (a is not used; pass b)
enum DotOp { DOT = 0, DIFF2 = 1, SUM = 2, PUPD = 3, SQPUPD = 4 };
struct DotTerm {
    const double* a;
    const double* b;
    int op;
    const double* c = nullptr;
    const double* beta = nullptr;
};
// gam1 chain (rides in a reduction launch, after the sum a2 = <bern, invQ>): from
// the sum of term `term`, a2: alpha2 = gam2*a2, eta2 = gam2/alpha2, gam1 =
// rho*min(max(eta2 - gam2, 1e-11), 1e11) + (1 - rho)*gam1_prev into out[0] =
// gam1, out[1] = eta2, out[2] = alpha2 (out null: none)
struct G1Chain {
    int term = 0;
    double gam2 = 0.0, rho = 0.0, gam1_prev = 0.0;
    double* out = nullptr;
};
// device copies of chosen results (the results themselves may land in mapped
// host memory, which a later kernel reads at a PCIe round trip's cost)
struct DotCopy {
    int n = 0;
    int term[2] = {0, 0};
    double* dst[2] = {nullptr, nullptr};
};
struct DotArgs {
    DotTerm t[kMaxTerms];
    int nt;
    G1Chain g1;    // formed by the launch's last block from its final sums
    DotCopy copy;  // ... and these copies stored by it
};
int red_blocks(int64_t n);
// ro.out[q] = term q summed over [0, n): per-block partials, then the blocks'
// sums in block order (fixed geometry: depends on n only)
hipError_t dots(const DotArgs& a, int64_t n, const RedOut& ro, hipStream_t st);
// a over [0, na) and b over [0, nb) in ONE launch, each bitwise as its own
// dots launch (its partials at its RedOut's part; one shared ticket; roa
// without a flag, rob's flag after both).  No PUPD / SQPUPD terms; the term
// counts of the pairs instantiated (10, 11) only, else hipErrorInvalidValue
hipError_t dots2(const DotArgs& a, int64_t na, const RedOut& roa, const DotArgs& b, int64_t nb, const RedOut& rob,
                 hipStream_t st);

// ---- denoiser (vamp::g1 / g1d) ---------------------------------------------
struct Mix {
    double probs[kMaxL];
    double vars[kMaxL];
    int L;
};
// The mixture words of the device EM update, kMixWords doubles: [0] L,
// [1, 1 + kMaxL) probs, [1 + kMaxL, 1 + 2 kMaxL) vars, [1 + 2 kMaxL] eta_max
constexpr int kMixWords = 2 + 2 * kMaxL;
// x1 = g1(r1) (then rho*x1 + (1-rho)*x1_prev if damp), x1d = g1d(r1),
// sum of x1d in ro.out[0].  mixw / gam1dev (may be null): the mixture's words
// (kMixWords, device: an EM round's update, em_sums' upd) and gam1 (G1Chain)
// from the device instead of mix and gam1.
// po (may be null, with mixw): the launch's last block also forms the next
// prelude's scalars (PreOut) from the sum of x1d
struct PreOut;
hipError_t denoise(int64_t M, const double* r1, double gam1, const Mix& mix, double* x1,
                   const double* x1_prev, int damp, double rho, double* x1d, const RedOut& ro, hipStream_t st,
                   const double* mixw = nullptr, const double* gam1dev = nullptr, const PreOut* po = nullptr);

// ---- EM prior update (vamp::updatePrior) per-marker sums --------------------
// the round's update of the mixture, formed on the device by the launch that
// finishes the round's sums (em_sums): out non-null
struct EmUpd {
    int64_t Mt = 0;
    int learn_vars = 0;
    double merge_vars_thr = 0.0;
    double* out = nullptr;     // the updated mixture's words (kMixWords, device: denoise's mixw)
    double* mirror = nullptr;  // the same words in mapped host memory, for the host's check
};
struct EmArgs {
    double omegas[kMaxL];
    double vars[kMaxL];
    double v[kMaxL];
    double lambda, noise_var, gam1, max_sigma;
    int L;
    // r1out (may be null): the round also forms r1 = (la*lx - lb*ly)/lc (the
    // lincomb_div of src/vamp.cpp:348-350, bit for bit) and stores it, instead
    // of reading r1: one launch where there were two
    const double* lx;
    const double* ly;
    double la, lb, lc;
    double* r1out;
    // dsc (may be null): gam1 = dsc[0] and la = eta2 = dsc[1] come from the
    // device (G1Chain), and noise_var = 1/gam1, v[j-1] = 1/(1/vars[j] + gam1)
    // are formed here, with the host's expressions (the host fields are unused)
    const double* dsc;
    // upd.out (may be null): the launch's last block also forms this round's
    // update of the mixture (vars and L here; vamp.cpp em_finish with one
    // round and the merging of close variances, src/vamp.cpp:598-642: the
    // host's expressions, bit for bit) into upd.out and upd.mirror
    EmUpd upd;
};
// ro.out[q], Q = 1 + 2(L-1): q=0 sum pin; q=j (1..L-1) sum beta_j pin;
// q=L-1+j sum beta_j (g_j^2 + v_j) pin
hipError_t em_sums(int64_t M, const double* r1, const EmArgs& a, const RedOut& ro, hipStream_t st);

// ---- elementwise VAMP updates -----------------------------------------------
// out = (a*x - b*y) / c        (r2 and r1 updates, src/vamp.cpp:259-261, 348-350)
hipError_t lincomb_div(int64_t n, double a, const double* x, double b, const double* y, double c,
                       double* out, hipStream_t st);
// out = a*x + b*y              (v = gamw*ATx(y) + gam2*r2, src/vamp.cpp:305-306)
hipError_t axpby(int64_t n, double a, const double* x, double b, const double* y, double* out,
                 hipStream_t st);
// bern[i] = (2*bit(seed,it,S+i) - 1) / sqrtMt
hipError_t bernoulli(uint64_t seed, int it, int64_t S, int64_t M, double sqrtMt, double* out,
                     hipStream_t st);
// The linear iteration's elementwise work before its CG solves, one launch
// (the same arithmetic as the separate kernels above, element for element):
//   r2 = (eta1*x1 - gam1*r1) / gam2      (src/vamp.cpp:259-261)
//   v = gamw*atxy + gam2*r2              (:303-306)
//   bern = the probe of iteration it     (:295-296, P2); bern_next: of it + 1 (may be null)
//   zero[z][i] = 0 for the non-null zero[z] (the CG solves' zero starts)
// The next iteration's prelude scalars, formed on the device by the launch
// that finishes its last sum (denoise, one rank), so that the prelude can be
// queued before the host has them: alpha1 = sum_d/Mt, eta1 = gam1/alpha1,
// gam2 = min(max(eta1 - gam1, 1e-11), 1e11), gamw = N/(tn + tc*Mt) (src/vamp.
// cpp:223, 230, 255-256, 521-528) and the CG's diag = gamw*(N-1)/N + gam2
// (:676-677): the host's expressions, bit for bit.  out (device) = {eta1, gam2, gamw, diag,
// gam1}, mirror (mapped host) = its first four, for the host's check.  tn,
// tc: device copies (DotCopy) of earlier launches' results
struct PreOut {
    const double* tn = nullptr;
    const double* tc = nullptr;
    double Mt = 0.0, N = 0.0;
    double* out = nullptr;
    double* mirror = nullptr;
};
// Several ranks: what the one-rank launches' last blocks form from their final
// sums (G1Chain, EmArgs.upd, PreOut), formed by one thread after the sums'
// all-reduce (vamp.cpp's host-free tail; the same expressions, bit for bit).
// mode 0: gam1_chain from src[0] = a2 into g1.out, and the device copies
// cp_dst[i] = *cp_src[i]; 1: one EM round's update of the mixture (L, vars)
// from src (1 + 2(L-1) sums) into upd.out / upd.mirror; 2: the next prelude's
// scalars from src[0] = the sum of x1d and gam1 = gam1dev[0] into po
struct TailPost {
    int mode = 0;
    const double* src = nullptr;
    G1Chain g1;
    const double* cp_src[2] = {nullptr, nullptr};
    double* cp_dst[2] = {nullptr, nullptr};
    int L = 0;
    double vars[kMaxL] = {};
    EmUpd upd;
    PreOut po;
    const double* gam1dev = nullptr;
};
hipError_t tail_post(const TailPost& t, hipStream_t st);
// scal (device, may be null): the prelude's scalars {eta1, gam2, gamw, diag,
// gam1} from PreOut.out instead of the Prelude's own (prelude_cg_init only)
struct PreDev {
    const double* scal = nullptr;
};
struct Prelude {
    double eta1, gam1, gam2, gamw;
    PreDev dev;  // prelude_cg_init only
    const double* x1;
    const double* r1;
    const double* atxy;
    double* r2;
    double* v;
    uint64_t seed;
    int it;
    int64_t S;
    double sqrtMt;
    double* bern;
    double* bern_next;
    double* zero[2];
};
hipError_t prelude(int64_t M, const Prelude& p, hipStream_t st);
// out = x / d
hipError_t div_scalar(int64_t n, const double* x, double d, double* out, hipStream_t st);
// out[0, n) = x / d and out[n, 2n) = r / d in one launch (the iteration writer)
hipError_t div2_scalar(int64_t n, const double* x, const double* r, double d, double* out, hipStream_t st);

// ---- probit model (src/vamp_probit.cpp) -------------------------------------
// z1[i] = g1_bin_class(p1[i], tau1, y[i]); the sum of g1d_bin_class in ro.out[0]
// (src/vamp_probit.cpp:213-233, 469-488; probit_var = 1, m_cov = 0)
hipError_t probit_denoise(int64_t N, const double* p1, const double* y, double tau1, double* z1, const RedOut& ro,
                          hipStream_t st);
// predict_probit(z_k, 0.5) + confusion_matrix against y (src/vamp_probit.cpp:619-651),
// nz <= 2 vectors at z + k*ld; ro.out[4k + {TP, TN, FP, FN}]
hipError_t probit_confusion(int64_t N, int nz, const double* z, int64_t ld, const double* y, const RedOut& ro,
                            hipStream_t st);
// P2 start: p1[i] = gauss(seed ^ salt, 0, i) (replaces simulate(N, {1}, {1}), :53)
hipError_t probit_p1(uint64_t seed, int64_t N, double* p1, hipStream_t st);
// probit_denoise with the covariate offset: c = (p1[i] + m_cov[i]) / sqrt(1 + 1/tau1)
// (g1_bin_class / g1d_bin_class with m_cov, :469-488); the same block sums and RedOut protocol
hipError_t probit_denoise_cov(int64_t N, const double* p1, const double* y, const double* m_cov, double tau1,
                              double* z1, const RedOut& ro, hipStream_t st);

// ---- covariate effects of the probit model (vamp::Newton_method_cov, :490-617) --
// Z: C covariates of N samples, covariate-major with column stride ld.  A
// workgroup owns the tile of kCovTile samples [t*kCovTile, (t+1)*kCovTile) and
// forms every sum over it in row order; cov_finish adds the tiles' partials in
// tile order, one thread per sum.  No sum depends on the grid or the device,
// and the mlogL of cov_mlogl is bitwise that of cov_eval on the same inputs.
constexpr int kCovMaxC = 64;   // VAMPOMI_MAX_C
constexpr int kCovTile = 64;   // samples per workgroup
inline int64_t cov_tiles(int64_t N) { return (N + kCovTile - 1) / kCovTile; }
inline int cov_nq(int C) { return C * (C + 1) / 2 + C + 1; }
// Per sample: g = gg_i + sum_j Z_ij eta_j (j ascending; gg may be null: zeros),
// s = 2 y_i - 1, arg = s g, ratio = (2/sqrt(2 pi)) / erfcx(-arg/sqrt 2),
// lambda = ratio s, w = lambda (lambda + g)  (:536-547).  out (device, C*C + C
// + 1 doubles): H_jk = sum Z_ij Z_ik w (j <= k formed, mirrored), rhs_j = sum
// Z_ij lambda, mlogL = (sum -log(0.5 erfc(-arg/sqrt 2))) / N  (:490-502).
// eta: device, C.  part: device scratch, cov_tiles(N) * cov_nq(C) doubles.
hipError_t cov_eval(int64_t N, int C, const double* Z, int64_t ld, const double* y, const double* gg,
                    const double* eta, double* part, double* out, hipStream_t st);
// mlogL alone into out[0] (the line search's evaluations); part: cov_tiles(N) doubles
hipError_t cov_mlogl(int64_t N, int C, const double* Z, int64_t ld, const double* y, const double* gg,
                     const double* eta, double* part, double* out, hipStream_t st);
// m[i] = sum_j Z_ij eta_j, j ascending (inner_prod(Z[i], cov_eff), :214-216)
hipError_t cov_offset(int64_t N, int C, const double* Z, int64_t ld, const double* eta, double* m, hipStream_t st);

// ---- association tests (src/main_meth.cpp:206-264, src/data.cpp:385-417) -------
// stats[5j + {0..4}] = sum X, sum X^2, sum X*ym, sum ym, sum ym^2 over the
// samples of marker j (RAW X), ym = ymod + X / sqrtN * x1[j]  (data::pvals_loo)
hipError_t loo_sums(const Shard& s, const double* ymod, const double* x1, double sqrtN, double* stats,
                    hipStream_t st, int variant = kLooDefault, const Timing& tm = Timing{});
// The same sums for KT = 2, 3, 4 phenotypes from one pass over the shard:
// ymod: KT ld-padded vectors of stride s.ld, x1: KT vectors of stride
// max(M, 1), stats: KT blocks of 5*M.  Block t holds, bit for bit, what
// loo_sums(s, ymod_t, x1_t, ...) gives under any 8-wave workgroup variant
// (kLooDefault among them).  Markers per workgroup and unroll per KT (they do
// not change the bits; profiles/assoc_multi.md):
constexpr int kLooMultiMax = 4;
constexpr int kLooMultiG2 = 4, kLooMultiUJ2 = 2, kLooMultiG3 = 4, kLooMultiUJ3 = 1, kLooMultiG4 = 2, kLooMultiUJ4 = 2;
hipError_t loo_multi_sums(const Shard& s, int KT, const double* ymod, const double* x1, double sqrtN, double* stats,
                          hipStream_t st, const Timing& tm = Timing{});
std::string loo_multi_kernel_name(int KT, int ek = 0);
std::string loo_kernel_name(int variant, int ek = 0);
// ---- leave-one-chromosome-out test --------------------------
// Each marker has a label in [0, G), G <= kSegMax.  Both passes walk the local
// markers sorted by (label, index), through lists the host cuts (seg_lists):
//   cols       the M sorted column indices
//   chunk_at   nchunks + 1 offsets into cols: chunk k is [chunk_at[k],
//              chunk_at[k + 1]), at most kSegChunk columns of ONE label; a
//              label's run of n columns is cut into ceil(n / kSegChunk) equal
//              shares
//   lab_chunk  G + 1: label c's chunks are [lab_chunk[c], lab_chunk[c + 1])
//   grp_col    ngroups x kLocoG columns of ONE label (-1: none), grp_lab its label
constexpr int kSegMax = 64;      // VAMPOMI_MAX_SEGMENTS
constexpr int kSegChunk = 256;   // columns per chunk at most
constexpr int kSegRows = 512;    // rows per tile of the segmented A.x
constexpr int kLocoG = 4;        // markers per workgroup of the marker pass (kLooDefault's)
struct SegLists {
    std::vector<int32_t> cols, chunk_at, lab_chunk, grp_col, grp_lab;
    int nchunks() const { return (int)chunk_at.size() - 1; }
    int ngroups() const { return (int)grp_lab.size(); }
};
inline int64_t seg_max_chunks(int64_t M) { return (M + kSegChunk - 1) / kSegChunk + kSegMax; }
inline int64_t seg_max_groups(int64_t M) { return (M + kLocoG - 1) / kLocoG + kSegMax; }
// labels: M values in [0, G) (checked by the caller)
void seg_lists(const int32_t* labels, int64_t M, int G, SegLists* out);
// Stage 1: workgroup (chunk, row tile of kSegRows) adds the terms (X_ij -
// mave_i) * (msig_i * x_i), formed as ax_partial forms them, over the chunk's
// columns in list order into part[chunk][j] (nchunks x ld; rows j < N).
// Stage 2 (ax_seg_reduce): z[c][j] = label c's slots added in chunk order
// (zeros for a label without markers), / div if div > 0; z: G x ld, pad rows
// not written.  Every sum has a fixed order: no atomics.
hipError_t ax_seg_partial(const Shard& s, const double* x, const int32_t* cols, const int32_t* chunk_at, int nchunks,
                          double* part, hipStream_t st, const Timing& tm = Timing{});
hipError_t ax_seg_reduce(int G, int64_t N, int64_t ld, const int32_t* lab_chunk, const double* part, double* z,
                         double div, hipStream_t st);
// zc[c][j] = (y[j] - z) + z_c[j] in place, z = z_0 + ... + z_{G-1} in ascending
// c and z_c = zc[c][j] (/ div if div > 0: the all-reduced raw sums)
hipError_t loco_resid(int G, int64_t N, int64_t ld, const double* y, double* zc, double div, hipStream_t st);
// stats[5j + {0..4}] for every marker j of the groups: the five sums of
// loo_sums(s, ys + lab[j] * ldy, x1 = 0) under any 8-wave workgroup variant
// (kLooDefault among them), bit for bit.  ldy = 0: one phenotype for all
hipError_t loco_sums(const Shard& s, const double* ys, int64_t ldy, const int32_t* grp_col, const int32_t* grp_lab,
                     int ngroups, double* stats, hipStream_t st, const Timing& tm = Timing{});
std::string ax_seg_kernel_name(int ek = 0);
std::string loco_kernel_name(int ek = 0);
int loo_variant_count();
bool loo_variant_ok(int v);
// pvals[j] = linear_reg1d_pvals(stats[5j..5j+4], n)  (src/utilities.cpp:269-282)
hipError_t loo_pvals(int64_t M, const double* stats, int n, double* pvals, hipStream_t st);
// pvals[j] = P(N(r1_j, 1/(gam1 N)) <= 0), flipped for r1_j <= 0 (src/main_meth.cpp:231-236)
hipError_t se_pvals(int64_t M, const double* r1, double gam1, int64_t N, double* pvals, hipStream_t st);
// *p = v (one thread; a host value placed in stream order)
hipError_t set_scalar(double* p, double v, hipStream_t st);
// out = x * a
hipError_t mul_scalar(int64_t n, const double* x, double a, double* out, hipStream_t st);

// ---- host completion flag (system-scope store into mapped host memory) -------
hipError_t signal_host(unsigned long long* flag, unsigned long long seq, hipStream_t st);
// the same with a relaxed store (what it announces was written by earlier kernels)
hipError_t post_flag(unsigned long long* flag, unsigned long long seq, hipStream_t st);
// copies a[0..na) -> ha and b[0..nb) -> hb (mapped host memory), then stores seq into flag
hipError_t publish_host(const double* a, int na, double* ha, const double* b, int nb, double* hb,
                        unsigned long long* flag, unsigned long long seq, hipStream_t st);

// ---- PCG (vamp::precondCG_solver), K right-hand sides --------------------------
struct CgVecs {
    double* mu[kMaxRhs];
    double* r[kMaxRhs];
    double* z[kMaxRhs];
    double* p[kMaxRhs];
    const double* d[kMaxRhs];   // lmmse_mult(mu0) for init (nullptr: mu0 == 0), A p in the loop
    const double* v[kMaxRhs];
    const double* atx0[kMaxRhs];  // init only: A^T(A mu0) computed earlier (then d is ignored)
    double tau, gam2;             // init only, with atx0
    // cg_update only (may be null): W += alpha * S alongside mu += alpha * p,
    // S = the step's raw A^T(A p) (atx sraw), so W tracks A^T A mu
    double* W[kMaxRhs];
    const double* S[kMaxRhs];
    // cg_update only (may be null): AW += alpha * AS over nA samples, AS = the
    // step's A p (the replicated N-vector of the A.x pass), so AW tracks A mu
    double* AW[kMaxRhs];
    const double* AS[kMaxRhs];
    int64_t nA;
    // cg_update only, one-pass operator (may be null): over nA samples,
    // q = AR/diag [+ beta*Q when fuse] is stored in Q (the step's A p, as the
    // pass formed it), AW += alpha*q, AR -= AD*alpha (A r tracks r -= d*alpha)
    double* Q[kMaxRhs];
    double* AR[kMaxRhs];
    const double* AD[kMaxRhs];
    // one rank, one-pass operator (may be null): AD is not read; A d of
    // sample i is summed here from the operator's per-slot partials
    // adpart[(t*kMaxRhs + k)*adld + i], t < adslots, in op_reduce's order, and
    // divided by addiv (the separate op_reduce launch folded into this one).
    // Without adpart, addiv > 0: AD holds the all-reduced sums not yet divided,
    // and each is divided here as it is read (the vec_div launch folded in)
    const double* adpart;
    int64_t adld;
    int adslots;
    double addiv;
    // the pre-step (OpAlt; with adpart only, may be null): when the step's
    // operator launch ran slot k on the alternate system (the same rule, from
    // the state and *pre_done this launch reads at its start), that slot's
    // A d partials are summed into pre_u1 (the same order, / addiv) instead,
    // and the last block stores pre_token into *pre_done and sets bit 31 of
    // the packed decision word (kCgPackPre)
    double* pre_u1;
    unsigned long long* pre_done;
    unsigned long long pre_token;
};
// the pre-step's slot for a launch on state s (OpAlt): -1 if none
__host__ __device__ inline int cg_pre_slot(const int* active, int K, bool made) {
    if (made) return -1;
    for (int k = 0; k < K && k < kMaxRhs; ++k)
        if (!active[k]) return k;
    return -1;
}
// r = v - d (or v, or v - (atx0*tau + gam2*mu)), z = r/diag, p = z;
// <r,z>, <v,v> per system in ro.out (2K values)
hipError_t cg_init(int K, int64_t M, const CgVecs& c, double diag, const RedOut& ro, hipStream_t st);
// Device-side CG control.  The scalar recurrences of a CG step (alpha, the
// Onsager and residual stops, beta) run on the device from a CgState, so the
// host can queue the next step before this one's sums are known: every launch
// of a step is gated on `any` (a step queued after the last system stopped
// does nothing).  `mirror` (mapped host memory, two slots) receives
// seq/any/iters of step `it` in slot it & 1, then the step's flag.  Two slots:
// when the host reads step i-1's decision, step i is already queued and may
// have decided too (a gated step decides in microseconds); one shared slot let
// ranks read different steps' decisions and issue different collectives.
// off[k]: steps system k took before step 0 (the head start, pcg.cpp), so its
// count after step `it` is it + 1 + off[k]; a system stops after maxit steps.
struct CgState {
    double rz[kMaxRhs], vv[kMaxRhs], prev_ons[kMaxRhs], beta[kMaxRhs];
    double gam2, tol;
    int active[kMaxRhs], iters[kMaxRhs], onsager[kMaxRhs], off[kMaxRhs];
    int K, any, maxit;
};
// A step's decision in ONE 64-bit word (the one-pass CG: K <= 2 systems,
// iteration counts below 2^15): the step's sequence number in the high half
// (so the word grows with it), any in bit 30, iters[1] in bits 15-29 and
// iters[0] in bits 0-14.  One system-scope store publishes it whole: no
// mirror, no ordering wait.
constexpr int kCgPackMaxIter = (1 << 15) - 2;
__host__ __device__ inline unsigned long long cg_pack(unsigned long long seq, int any, int it0, int it1) {
    return (seq << 32) | ((unsigned long long)(any ? 1 : 0) << 30) | ((unsigned long long)(it1 & 0x7fff) << 15) |
           (unsigned long long)(it0 & 0x7fff);
}
// bit 31 of the packed word: this step's launches made the pre-step (CgVecs.pre_u1)
constexpr unsigned long long kCgPackPre = 1ull << 31;
struct CgMirror {
    unsigned long long seq;  // the step's flag value: the slot holds that step's decision
    int any;
    int iters[kMaxRhs];
};
constexpr int kCgMirrorSlots = 2;
// *dst = init (one thread)
hipError_t cg_start(const CgState& init, CgState* dst, hipStream_t st);
// *dst = init with rz[k], vv[k] = sums[2k], sums[2k+1] (cg_init's sums, in device memory)
// gam2dev (may be null): init.gam2 from the device (a start queued ahead: the
// next prelude's scalars, PreOut.out + 1)
hipError_t cg_start_from(const CgState& init, const double* sums, CgState* dst, hipStream_t st,
                         const double* gam2dev = nullptr);
// prelude() and cg_init() in one launch (cg_init's grid and sums: bitwise the
// two launches), where cg_init's v_k may be the prelude's v or bern (taken from
// registers).  start (may be null): the last block also writes *dst = *start
// with rz[k], vv[k] from the sums (cg_start_from; one rank, the sums final)
hipError_t prelude_cg_init(int K, int64_t M, const Prelude& p, const CgVecs& c, double diag, const RedOut& ro,
                           const CgState* start, CgState* dst, hipStream_t st);
// for active k: [fuse: p = z + beta_k p, stored] alpha_k = rz[k] / dp_dev[k];
// mu += alpha p; r -= d alpha; z = r/diag; <r,z>, <r,r>, <v,mu> in ro.out (3K
// values, k-major; zeros for stopped systems); gated on cs->any.  dc.on (one
// rank: the sums are final): the last block also takes cg_decide's decisions.
struct CgDecide {
    int on = 0, it = 0;
    // pack: *flag receives the decision as ONE word (cg_pack) instead of the
    // mirror slot + sequence number
    int pack = 0;
    int mask = 0xf;  // the systems this step is for (the others keep their state; see cg_update)
    CgMirror* mirror = nullptr;
    unsigned long long* flag = nullptr;
    unsigned long long seq = 0;
};
// pp_dev (may be null): dp_dev holds |A p_k|^2 and pp_dev |p_k|^2, and
// <d,p> = tau*|A p|^2 + gam2*|p|^2 (c.tau, c.gam2).  fuse: bit k set when
// system k's direction update is fused into this step; dc.mask: the systems
// this step updates (the others are left as they are: the head start's step
// of one system, pcg.cpp)
hipError_t cg_update(int K, int64_t M, const CgVecs& c, double diag, CgState* cs, const double* dp_dev,
                     const double* pp_dev, int fuse, const RedOut& ro, const CgDecide& dc, hipStream_t st);
// step `it`'s decisions from red (the 3K sums of cg_update, summed over ranks),
// src/vamp.cpp:700-750, for the systems in mask; then mirror and flag (each
// stored when non-null, even when gated off)
hipError_t cg_decide(CgState* cs, const double* red, int it, CgMirror* mirror, unsigned long long* flag,
                     unsigned long long seq, hipStream_t st, int mask = 0xf, int pack = 0);
// The first CG step's operator products of a zero-start system with
// right-hand side b, composed from T1 = A^T A b, U1 = A T1 and ab = A b (the
// pre-step, OpAlt) with no pass over X.  p = b/diag as cg_init left it:
//   t_i = T1_i/diag, d_i = tau*t_i + gam2*p_i, S_i = t_i (S may be null),
//   AD_j = (tau*U1_j + gam2*ab_j)/diag, <d,p> in ro.out[0]
// (A^T A is linear, so these are the step's d = tau*A^T A p + gam2*p and A d
// up to rounding.)  Gated on ro.gate
struct PreCompose {
    const double* T1;  // M
    const double* U1;  // N
    const double* ab;  // N
    const double* p;   // M
    double* d;         // M
    double* S;         // M, may be null
    double* AD;        // N
    double diag, tau, gam2;
    // (may be null) rz_save[0] = cs->rz[0], <r0,z0> before the composed step's
    // decision replaces it: pre_compose2 forms the step's alpha from it
    const CgState* cs = nullptr;
    double* rz_save = nullptr;
};
hipError_t pre_compose(int64_t M, int64_t N, const PreCompose& a, const RedOut& ro, hipStream_t st);
// The SECOND CG step's operator products of the same system, composed from
// T1, T2 = A^T A T1, U1 = A T1 and U2 = A T2 after the composed first step
// (pre_compose, then its cg_update), with no pass over X.  With alpha0 =
// rz_save[0] / dp0[0] (cg_update's own expression on the same values),
// beta0 = cs->beta[0], p0 = p as stored and p1 = z_i + beta0*p0_i (the
// direction update the step's cg_update stores):
//   w_i  = (tau*T2_i + gam2*T1_i)/diag                     (A^T A d0)
//   S_i  = (T1_i - alpha0*w_i)/diag + beta0*(T1_i/diag)    (A^T A p1)
//   d_i  = tau*S_i + gam2*p1_i
//   q1_j = ar_j/diag + beta0*q_j                           (A p1, as cg_update forms it)
//   AD_j = tau*((U1_j - alpha0*((tau*U2_j + gam2*U1_j)/diag))/diag + beta0*(U1_j/diag)) + gam2*q1_j
// <d,p1> in ro.out[0] (dp0 may be ro.out: every block reads it before the
// last one stores).  Gated on ro.gate; nothing if system 0 has stopped
struct PreCompose2 {
    const double* T1;  // M
    const double* T2;  // M
    const double* U1;  // N
    const double* U2;  // N
    const double* ar;  // N: A r1 (after the composed first step)
    const double* q;   // N: q0 = A p0
    const double* p;   // M: p0
    const double* z;   // M: z1
    double* d;         // M
    double* S;         // M, may be null
    double* AD;        // N
    double diag, tau, gam2;
    const CgState* cs;
    const double* rz_save;
    const double* dp0;
};
hipError_t pre_compose2(int64_t M, int64_t N, const PreCompose2& a, const RedOut& ro, hipStream_t st);

}  // namespace vk
