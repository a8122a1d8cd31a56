// ctx.h — libvampomi internals shared by engine.cpp, ingest.cpp, assoc.cpp, pcg.cpp and vamp.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vampomi.h"
#include "kernels.h"

// ---- errors ---------------------------------------------------------------
vampomi_status fail(vampomi_status s, const std::string& msg);

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(VAMPOMI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

#define NCCLCHK(expr)                                                                                 \
    do {                                                                                              \
        ncclResult_t _r = (expr);                                                                     \
        if (_r != ncclSuccess)                                                                        \
            return fail(VAMPOMI_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_r));        \
    } while (0)

#define STCHK(expr)                                   \
    do {                                              \
        vampomi_status _s = (expr);                   \
        if (_s != VAMPOMI_OK) return _s;              \
    } while (0)

// ---- the context ------------------------------------------------------------
struct vampomi_ctx;
// Marks a COLLECTIVE entry point on this thread: an error raised inside it
// (fail()) aborts the context's communicator first (comm_abort), so that the
// other ranks fail at their next collective instead of waiting for this one.
struct CollScope {
    explicit CollScope(vampomi_ctx* c);
    ~CollScope();
    vampomi_ctx* prev;
};
struct VampRun;
class IterWriter;
struct LoopbackComm;  // engine.cpp: test-only in-process communicator
struct ShmComm;       // shmcomm.cpp: test-only cross-process communicator (VAMPOMI_COMM=shm)
std::shared_ptr<ShmComm> shm_join(const void* id, int P, int rank, double limit_s, std::string* err);
std::string shm_allreduce(ShmComm& s, int rank, double* buf, size_t n, uint64_t seq, const char* site, int line,
                          double limit_s);
void shm_poison(ShmComm& s, const std::string& why);

struct TimedLaunch {
    hipEvent_t a, b;
    int cls;  // 0 ax, 1 atx, 2 loo, 3 one-pass operator, 4 all-reduce
    int K;
    double bytes, flops;
};

// scalar slots in ctx->scal: <d,p> of the fused lmmse epilogue, then the
// synced (summed over ranks) and local halves of a DotBatch
// (SL_CG: the 3K sums of a CG step, decided on the device; SL_CGI: the 2K sums
// of cg_init, read by cg_start_from)
// (SL_CHAIN, device, one rank: [0, 3) gam1, eta2, alpha2 of G1Chain; [3, 8)
// the next prelude's scalars (vk::PreOut); [8] tn, [9] tc (DotCopy))
enum : int { SL_DP = 0, SL_CG = 4, SL_SYNC = 16, SL_NSYNC = 256, SL_LOCAL = SL_SYNC + SL_NSYNC, SL_NLOCAL = 128,
             SL_CGI = SL_LOCAL + SL_NLOCAL, SL_CHECK = SL_CGI + 16, SL_AGREE = SL_CHECK + 8, SL_CHAIN = SL_AGREE + 8, SL_TOTAL = 512, SL_BARRIER = SL_TOTAL - 1 };

struct vampomi_ctx {
    int rank = 0, nranks = 1, device = 0;
    int64_t N = 0, Mt = 0, M = 0, S = 0, Mm = 0, ld = 0;
    double alpha_scale = 1.0;
    double sqrtN = 1.0;
    hipStream_t st = nullptr;  // every launch and collective of the context (one stream: DESIGN.md §6)
    bool mr_tail = true;   // several ranks: the linear iteration's tail without host waits (vamp.cpp), as agreed
    double coll_limit_s = 0.0;  // > 0: the limit of the collective in progress (vampomi_barrier_timeout)
    bool mr_tail_req = true;  // this rank's VAMPOMI_MR_TAIL (0: off), agreed over the ranks by op_agree
    bool cg_fold = true;   // several ranks: each CG decision formed by the next operator launch (pcg.cpp); VAMPOMI_CG_FOLD=0
    bool dp_separate = false;  // several ranks, two-pass CG: <d,p> by its own reduction, the one-rank form (pcg.cpp); VAMPOMI_DP_SEPARATE=1
    bool team_reg = false;           // registered with its device's team gate (engine.cpp)
    hipEvent_t team_ev = nullptr;    // recorded on st when another context must order behind it
    ncclComm_t comm = nullptr;
    bool use_comm = false;  // nranks > 1 (or VAMPOMI_FORCE_RCCL): all-reduces through RCCL
    std::shared_ptr<LoopbackComm> loopback;  // VAMPOMI_COMM=loopback: ranks are threads of one process
    std::shared_ptr<ShmComm> shm;            // VAMPOMI_COMM=shm: ranks are processes of one host
    uint64_t coll_seq = 0;  // collectives issued so far (divergence checks)
    bool aborted = false;   // comm_abort ran: no further collective

    // M columns x ld, marker-major, pad rows zero: doubles, floats with
    // storage == VAMPOMI_STORE_F32, or 16-bit fixed point (uint16_t k, value
    // k * 2^-16) with VAMPOMI_STORE_U16 (fixed once X is allocated; rank-local:
    // the ranks agree on nothing that depends on it)
    void* X = nullptr;
    int storage = VAMPOMI_STORE_F64;
    // U16 storage: what the last load's quantisation saw (vk::convert_cols;
    // zeroed when a load starts) and its host copy (vampomi_get_quant_stats)
    vk::QuantRec* qrec = nullptr;
    int64_t q_clamped = 0;
    double q_max_err = 0.0;
    // missing values (vampomi_set_meth_na; fixed once X is allocated, rank-local):
    // the policy, what the last load's vk::na_ingest_cols saw (na_rec; na_cnt: M
    // per-marker counts) and the host copy (vampomi_get_missing_stats)
    int na_policy = VAMPOMI_NA_PASS;
    double na_max_frac = 1.0;
    vk::NaRec* na_rec = nullptr;
    int64_t* na_cnt = nullptr;
    int64_t na_missing = 0, na_markers = 0, na_masked = 0;
    std::vector<int64_t> na_per_marker;  // empty: all zeros
    // the row subset (vampomi_set_row_subset; N_file == 0: none): the files hold
    // N_file rows of which rows_host (N ascending indices) are loaded; rows_dev:
    // their device copy for vk::convert_cols
    int64_t N_file = 0;
    std::vector<int64_t> rows_host;
    int32_t* rows_dev = nullptr;
    // covariate adjustment (vampomi_set_adjust; adj_R == 0: none; fixed once X is
    // allocated): adj_Q, N x adj_R orthonormal doubles, column-major, the
    // intercept's first; adj_dropped, one flag per column of the table.  The
    // device side exists during a load only (IngestScope, ingest.cpp);
    // adj_flags / adj_absorbed are the host copy of what vk::adjust_cols
    // recorded (vampomi_get_adjust_stats)
    int adj_R = 0, adj_C = 0;
    std::vector<double> adj_Q;
    std::vector<int> adj_dropped;
    std::vector<uint8_t> adj_flags;  // empty: all zeros
    int64_t adj_absorbed = 0;
    double* mave = nullptr;
    double* msig = nullptr;
    double* y = nullptr;     // ld, zero pad
    std::vector<double> y_host;
    bool have_X = false, have_y = false;
    // covariates of the probit model (covariates.cpp): the whole N x C table on
    // every rank, as y.  cov_host: C columns of N; cov_Z: C columns of stride ld
    int cov_C = 0;
    std::vector<double> cov_host;
    double* cov_Z = nullptr;
    double* cov_part = nullptr;  // cov_tiles(N) x cov_nq(C) tile partials
    double* cov_dev = nullptr;   // eta (kCovMaxC), then H, rhs, mlogL of vk::cov_eval
    std::vector<double> cov_eff;  // fitted by the last vampomi_vamp_begin (bin_class)
    bool cov_fitted = false;

    vk::AxPlan axp{};
    int atx_variant = vk::kAtxDefault, loo_variant = vk::kLooDefault;  // per context (dev hooks)
    double* ax_part = nullptr;  // nslots x kMaxRhs x ld partial sums of A.x
    double* red_part = nullptr;  // per-block partials of every reduction
    size_t red_cap = 0;
    double* scal = nullptr;     // device scalars (SL_*)
    double* h_scal = nullptr;   // pinned host mirror, mapped and coherent: one-rank reductions land here directly
    double* d_hscal = nullptr;  // its device-side address
    unsigned* ticket = nullptr; // arrival counter of the fused reductions (zero between launches)
    unsigned long long* h_flag = nullptr;  // mapped host word the stream stores sync sequence numbers into
    unsigned long long* d_flag = nullptr;
    unsigned long long sync_seq = 0;
    vk::CgState* cgs = nullptr;     // device-side CG control (pcg.cpp), two states (the folded decisions alternate)
    vk::CgMirror* h_cgm = nullptr;  // its mapped host mirror, and the mirror's device address
    vk::CgMirror* d_cgm = nullptr;
    // one-pass CG operator (batch_rhs 4; allocated on first use, pcg.cpp)
    vk::OpPlan opp{};
    int op_variant = vk::kOpDefault;  // plan choice (dev hook: vampomi_dev_set_variant(c, 3, v))
    bool op_ready = false;            // opp planned (locally) and its buffers allocated
    bool op_ok_mine = false;          // this rank's plan exists and its grid fits the device
    bool op_ok = false;               // the operator runs: op_ok_mine on one rank; the agreed value on several
    // several ranks: the one-pass / head-start choice is agreed at one fixed
    // collective point every rank reaches (op_agree, at vampomi_vamp_begin);
    // set_variant(3 / 5) requests wait for it (applied at once on one rank)
    bool op_agreed = false;
    int op_variant_req = vk::kOpDefault;
    int cus = 0;                // compute units of the device (the operator's grid)
    double* op_part = nullptr;  // opp.nslots x kMaxRhs x ld partial A d
    int64_t op_part_slots = 0;
    double* op_nvec = nullptr;  // 3 x kMaxRhs x ld + 16: A r, q = A p, A d (+ <d,p> tail)
    unsigned long long* op_xg = nullptr;  // team hand-off granules (M x kOpMaxK x T x 2; x kOpSys on opp3), zeroed once
    size_t op_xg_words = 0;
    unsigned op_tag = 0;        // the last team launch's tag
    // the head-start launch (pcg.cpp): its plan and whether it runs (default
    // on; VAMPOMI_HEADSTART=0 or vampomi_dev_set_variant(c, 5, 0) turns it off)
    vk::OpPlan opp_hs{};
    bool hs_ok_mine = false;  // this rank's head-start plan exists and fits
    bool hs_ok = false;       // the head start runs (hs_on included; agreed on several ranks)
    bool hs_on = true;
    bool hs_on_req = true;
    // launches with a third operator system (kernels.h kOpSys; op_dev with
    // K = 3): their plan, and whether it exists and fits this device
    vk::OpPlan opp3{};
    bool sys3_ok = false;
    // the pre-step (HeadStart below): 0 off, 1 on at any size, 2 auto (one
    // rank, the linear model, the head start on and an X shard of at least
    // kPreMinBytes); 3: mode 1 with two pre-steps per solve in a third
    // operator slot where a 3-system plan exists (else mode 1);
    // VAMPOMI_PRESTEP or vampomi_dev_set_variant(c, 7, v)
    int pre_mode = 2;
    unsigned long long pre_seq = 0;        // the last solve's token (OpAlt.token)
    int64_t pre_made_n = 0, pre_used_n = 0;  // since vampomi_vamp_begin (vampomi_dev_prestep_counts)
    unsigned long long* op_ts = nullptr;  // VAMPOMI_OP_TS=1 (TM_TS builds): the last launch's workgroup times
    double* nbuf = nullptr;     // kMaxRhs * ld scratch N-vectors (API calls)
    double* mbuf = nullptr;     // (2*kMaxRhs) * M scratch M-vectors (API calls)
    // vampomi_assoc_loo_multi's chunk scratch (allocated on first use): am_n,
    // 2 * kLooMultiMax ld-vectors (y_t, then ymod_t); am_m, 8 * kLooMultiMax
    // M-vectors (estimates, x1, p-values, then the 5 sums of each phenotype)
    double* am_n = nullptr;
    double* am_m = nullptr;
    // vampomi_assoc_loco's workspaces (allocated on first use, grown when a
    // call needs more): lc_z, lc_G ld-vectors (z_c, then y_c in place; pad rows
    // zero); lc_part, lc_slots partial slots of the segmented A.x (ld each);
    // lc_idx, the lists of vk::SegLists (lc_idx_cap words)
    double* lc_z = nullptr;
    double* lc_part = nullptr;
    int32_t* lc_idx = nullptr;
    int lc_G = 0;
    int64_t lc_slots = 0, lc_idx_cap = 0;

    bool timing = false;
    int tperiod = 1;            // time 1 in tperiod launches of each (class, K)
    int64_t tcount[5][vk::kMaxRhs] = {};
    std::vector<TimedLaunch> pending;
    std::vector<hipEvent_t> ev_pool;
    vampomi_stats stats{};

    std::unique_ptr<VampRun> run;
    std::unique_ptr<IterWriter> writer;  // per-iteration output (writer.h), created with the context

    bool f32() const { return storage == VAMPOMI_STORE_F32; }
    bool u16() const { return storage == VAMPOMI_STORE_U16; }
    int ek() const { return u16() ? vk::kXU16 : f32() ? vk::kXF32 : vk::kXF64; }  // the element kind (kernels.h)
    int64_t esize() const { return u16() ? 2 : f32() ? 4 : 8; }  // bytes per element of X
    vk::Shard shard() const { return vk::Shard{X, ld, N, M, mave, msig, f32() ? 1 : 0, u16() ? 1 : 0}; }
    vampomi_ctx();   // defined in vamp.cpp, where VampRun is complete
    ~vampomi_ctx();
};

vampomi_status dev_alloc(double** p, size_t n);
void dev_free(double*& p);
vampomi_status host_sync(vampomi_ctx* c);
// spins until word `word` of the context's host flag block reaches seq (stores
// from the stream; word 0 the stream's sync sequence, kCgPackWord.. the CG's
// packed decisions)
vampomi_status wait_flag(vampomi_ctx* c, unsigned long long seq, int word = 0);
// hipStreamSynchronize, except with an RCCL communicator: polls the stream and
// the communicator, and aborts / fails on a broken job or after
// VAMPOMI_COLL_TIMEOUT_S (engine.cpp) instead of blocking forever
vampomi_status sync_stream(vampomi_ctx* c, hipStream_t st);
// SUM all-reduce of n doubles over the ranks (nothing on one rank). COLLECTIVE:
// every rank must make the same calls in the same order; site/line identify
// the call for the divergence checks (loopback always, RCCL with
// VAMPOMI_COLL_CHECK=1)
vampomi_status allreduce_dev(vampomi_ctx* c, double* buf, size_t n, const char* site = __builtin_FUNCTION(),
                             int line = __builtin_LINE());
// *total = local summed over the ranks (one all-reduce; *total = local on one
// rank).  COLLECTIVE: how ranks agree on a decision that started rank-local
vampomi_status sum_over_ranks(vampomi_ctx* c, double local, double* total, const char* site = __builtin_FUNCTION(),
                              int line = __builtin_LINE());
// poisons (loopback) or aborts (RCCL) the communicator after a rank-local error
void comm_abort(vampomi_ctx* c, const std::string& why);
void resolve_timing(vampomi_ctx* c);
// counts a launch of class cls with K right-hand sides (bytes, flops: its
// algorithmic work); returns HIP events for it if it is sampled (else nulls)
TimedLaunch launch_stat(vampomi_ctx* c, int cls, int K, double bytes, double flops);
// algorithmic bytes / flops of one pass over the shard with K right-hand sides
double pass_bytes(const vampomi_ctx* c, int K);
double pass_flops(const vampomi_ctx* c, int K);
// n doubles of a caller's vector (mem: VAMPOMI_MEM_HOST / _DEVICE) into a
// device buffer on the context's stream; stage_out: back, then the stream is
// synchronised (the caller may read dst)
vampomi_status stage_in(vampomi_ctx* c, const double* src, int64_t n, int mem, double* dst);
vampomi_status stage_out(vampomi_ctx* c, const double* src, int64_t n, int mem, double* dst);
// forgets the counts since `before` and the samples queued since pending_mark
// (the gated launches of a CG step queued after the solve had stopped)
void drop_launches(vampomi_ctx* c, size_t pending_mark, const vampomi_stats& before);
void release_ctx_resources(vampomi_ctx* c);
// ---- ingest (ingest.cpp) ------------------------------------------------------
// the rows of a column of the input: the file's with a row subset, else N
int64_t rows_in(const vampomi_ctx* c);
// y <- y - Q (Q^T y) on an adjusted context, long double sums, rounded once
void adjust_phen(const vampomi_ctx* c, std::vector<double>& y);

// ---- operators on device buffers ---------------------------------------------
// out_k = A x_k (K <= 4), outputs at outbase + k*ld (one all-reduce). COLLECTIVE
// fu (may be null): fused direction update and gate (vk::AxFuse).  tail (may
// be null; several ranks only): local M-sums all-reduced in the same call,
// landing at outbase[K*ld + q] (outbase must hold K*ld + tail->nt doubles)
vampomi_status ax_dev(vampomi_ctx* c, int K, const double* const* x, double* outbase,
                      const vk::AxFuse* fu = nullptr, const vk::DotArgs* tail = nullptr);
// out_k = A^T u_k (mode 0) or tau*A^T u_k + gam2*p_k with <out_k,p_k> summed over
// ranks into scal[SL_DP + k] (mode 1).  u_k: ld-padded N-vectors.  gate: as in
// vk::AxFuse; zf/beta (may be null): p_k stands for zf_k + beta[k]*p_k
// dp = false (mode 1): <out_k,p_k> is not formed (the caller has it otherwise)
vampomi_status atx_dev(vampomi_ctx* c, int K, const double* const* u, double* const* out, int mode, double tau,
                       double gam2, const double* const* p, const int* gate = nullptr,
                       const double* const* zf = nullptr, const double* beta = nullptr, bool dp = true,
                       double* const* sraw = nullptr);
// d_k = tau*A^T A v_k + gam2*v_k (lmmse_mult), <d_k,v_k> in scal[SL_DP+k]. COLLECTIVE
vampomi_status lmmse_dev(vampomi_ctx* c, int K, const double* const* v, double* const* d, double tau, double gam2,
                         double* nscratch);

// ---- batched scalar reductions ---------------------------------------------------
// Every inner_prod / l2_norm2 of the reference (src/utilities.cpp:138-162) is a
// fixed-order device reduction into a scalar slot.  A DotBatch queues several
// of them (each with its own sync flag: sync = summed over ranks, the
// reference's inner_prod(..., 1)) and resolves them with ONE all-reduce, ONE
// device-to-host copy and ONE host synchronisation.
class DotBatch {
   public:
    explicit DotBatch(vampomi_ctx* c) : c_(c) {}
    vampomi_status add(std::initializer_list<vk::DotTerm> terms, int64_t n, bool sync, double* out);
    // several groups of terms over the same length n in ONE kernel (<= 8 terms
    // in all): each group's results reach its out at flush(), exactly as its
    // own add() would give them (per-term sums do not depend on the other terms)
    struct Group {
        std::vector<vk::DotTerm> terms;
        bool sync;
        double* out;
    };
    // chain (may be null): its arithmetic rides in the launch, on the sum of
    // the group whose out is chain_of (a one-term group); copies: the result
    // of each one-term group whose out is .first is also stored at .second
    // (device memory) by the launch (at most 2)
    vampomi_status add_many(int64_t n, const std::vector<Group>& groups, const vk::G1Chain* chain = nullptr,
                            const double* chain_of = nullptr,
                            const std::vector<std::pair<const double*, double*>>& copies = {});
    // add_many over [0, na) with ga and over [0, nb) with gb in one launch
    // where vk::dots2 has the pairing (else two launches): the same results
    vampomi_status add_pair(int64_t na, const std::vector<Group>& ga, const vk::G1Chain* chain,
                            const double* chain_of, const std::vector<std::pair<const double*, double*>>& ca,
                            int64_t nb, const std::vector<Group>& gb,
                            const std::vector<std::pair<const double*, double*>>& cb);
    // reserves nq result slots for a fused reduction kernel: *ro says where the
    // kernel writes; the values reach out[0..nq) at flush()
    vampomi_status sink(int nq, bool sync, double* out, vk::RedOut* ro);
    vampomi_status flush();
    bool empty() const { return sinks_.empty(); }
    // one rank: the device address where the result that flush() will copy to
    // out is written (mapped host memory), for a kernel queued before the
    // flush; null if out is not a sink of this batch or with a communicator
    const double* dev_result(const double* out) const;
    // several ranks: all-reduces the synced slots filled since the last call,
    // on the main stream, with no host copy or wait (flush() then publishes
    // them without reducing them again), so that a kernel queued next can read
    // the final sums at dev_slot(); nothing on one rank.  COLLECTIVE
    vampomi_status reduce_now();
    // several ranks: the device address of the slot whose value flush() will
    // copy to out (final after reduce_now() for a synced result); else null
    double* dev_slot(const double* out) const;
    // the stream the batch's launches go to (the context's)
    hipStream_t stream() const;

   private:
    // a launch's DotArgs and RedOut from its groups (sinks registered, flag sequence taken)
    vampomi_status build(const std::vector<Group>& groups, const vk::G1Chain* chain, const double* chain_of,
                         const std::vector<std::pair<const double*, double*>>& copies, vk::DotArgs& a,
                         vk::RedOut& ro);
    struct Sink {
        int slot, count;
        double* out;
    };
    vampomi_ctx* c_;
    int nsync_ = 0, nlocal_ = 0;
    int nred_ = 0;  // synced slots [0, nred_) already all-reduced (reduce_now)
    unsigned long long last_seq_ = 0;  // one rank: flag value the last reduction kernel stores
    std::vector<Sink> sinks_;
};

inline vk::DotTerm T(const double* a, const double* b, int op = vk::DOT) { return vk::DotTerm{a, b, op}; }

// ---- PCG (vamp::precondCG_solver) ----------------------------------------------
struct CgSystem {
    const double* v = nullptr;     // right-hand side (device, M)
    double* mu = nullptr;          // in: start (if mu0_nonzero), out: solution
    bool mu0_nonzero = false;      // false: start from zeros (lmmse_mult short-circuit)
    const double* atx0 = nullptr;  // optional: A^T(A mu0) computed earlier (saves the start's passes)
    // optional recurrence (batch_rhs 2): W (device, M) holds A^T A mu0 on entry
    // (zeros when mu0 = 0) and A^T A mu on return, updated with each step's raw
    // A^T(A p) kept in S (device, M scratch); W may alias atx0
    double* W = nullptr;
    double* S = nullptr;
    // optional (batch_rhs 3): AW (device, ld) holds A mu0 on entry (zeros when
    // mu0 = 0) and A mu on return, updated with each step's A p
    double* AW = nullptr;
    bool onsager = false;          // denoiser == 0 in the reference: extra Onsager stop
    int iters = 0;
    double *r = nullptr, *z = nullptr, *p = nullptr, *d = nullptr;  // work vectors (device, M)
};
// The HEAD START (PcgArgs::hs; onepass, K = 2, extra_x).  System 0 must
// start from zero (r0 = v, e.g. the Onsager solve, whose v is a probe known an
// iteration early).  abern (device ld) holds A v of system 0: then system
// 0's first CG step runs in the pass that would only compute A r0 of system 1
// and A extra_x (one operator launch with plain right-hand sides,
// op_dev_plain), and the two systems step together from there, system 0 one
// step ahead, so the solve takes 1 + max(k1 - 1, k2) passes instead of
// 1 + max(k1, k2).  Every step is the reference's (src/vamp.cpp:697-757).
// xnext (may be null, device M): one more right-hand side of that pass,
// axnext = A xnext (the next solve's abern).  Without abern the first
// A.x pass carries xnext instead.
struct HeadStart {
    double* abern = nullptr;  // (the Onsager solve's A r: updated in place)
    const double* xnext = nullptr;
    double* axnext = nullptr;
    bool used = false;  // out: the head start ran
    // The PRE-STEP (one rank; kernels.h OpAlt, PreCompose).  In a step whose
    // operator launch has a slot whose system has stopped, that slot forms
    // T1 = A^T A xnext and U1 = A T1 (once per solve), the first CG step's
    // products of the NEXT solve's system 0 up to its scalars.  With pre_have,
    // this solve's system 0 takes its step 1 from them with no pass over X
    // (vk::pre_compose), its step 2 rides in the head-start pass, and the
    // solve takes 1 + max(k1 - 2, k2) passes.
    double* T1 = nullptr;                  // M
    double* U1 = nullptr;                  // ld
    unsigned long long* pre_done = nullptr;  // device: the token of the last solve that made a pre-step
    bool pre_have = false;   // in: T1, U1 hold the products of this solve's system 0 (with abern)
    bool pre_offer = false;  // in: make them for the next solve (with xnext / axnext)
    bool pre_made = false;   // out: made (for xnext)
    bool pre_used = false;   // out: consumed
    // Mode 3 (pre3; a 3-system plan exists, kernels.h kOpSys): no slot rule and
    // no token.  Regular steps 0 and 1 of every solve are 3-system launches
    // whose third slot forms T1 = A^T A xnext, U1 = A T1 (step 0) and
    // T2 = A^T A T1, U2 = A T2 (step 1): a step that ran made its pre-step.
    // With n_have = J in {0, 1, 2} this solve's system 0 composes its first J
    // steps (vk::pre_compose, vk::pre_compose2), step J + 1 rides in the
    // head-start pass, and the solve takes 1 + max(k1, k2 - 1 - J) passes (k2:
    // the steps of system 0, the Onsager solve; k1: system 1's).
    bool pre3 = false;
    double* T2 = nullptr;      // M
    double* U2 = nullptr;      // ld
    double* rz_save = nullptr;  // device, 1 double: <r0,z0> of system 0 (PreCompose.rz_save)
    int n_have = 0;  // in: the pre-steps in hand (pre_have: >= 1)
    int n_made = 0;  // out
    int n_used = 0;  // out
};
// how PcgArgs::pre's launch is queued (one rank)
enum class PreMode { normal, ahead, queued };
// pcg_run's arguments beside the systems (tau*A^T A + gam2*I) mu = v
struct PcgArgs {
    double tau = 0.0, gam2 = 0.0;
    int max_iter = 0;    // CG steps per system at most
    double tol = 0.0;    // a system stops when ||r||/||v|| < tol
    double* nscratch = nullptr;     // device scratch, kMaxRhs*ld + kMaxRhs doubles
    int64_t* ref_passes = nullptr;  // (may be null) += the passes over X the reference would have made
    // (may be null) flushed together with the initial residual reductions (one host wait)
    DotBatch* init = nullptr;
    // extra_x (may be null, device M): ex_out (device, ld) = A extra_x, carried as
    // one more right-hand side of the first step's A.x pass (its own pass if no
    // step runs); K <= 2
    const double* extra_x = nullptr;
    double* ex_out = nullptr;
    // (K <= 2) every CG step reads X once (vk::atax; A r0 by one A.x pass per
    // solve, which also carries extra_x); otherwise two passes per step
    bool onepass = false;
    // (may be null; onepass only) ar0[k] (device, ld, may be null) already
    // holds A r0 of system k (its start is zero, so r0 = v), and the first A.x
    // pass covers only the systems without it (no pass if none)
    const double* const* ar0 = nullptr;
    HeadStart* hs = nullptr;  // the head start above (may be null; onepass, K = 2, extra_x, system 0 at zero, no ar0)
    // pre (may be null; init must be null): the caller's prelude launch, fused
    // with the solve's start (vk::prelude_cg_init).  pm (one rank, with pre):
    // ahead: queue only that launch, its scalars from the device (pre->dev; tau
    // and gam2 unused), and return; queued: that launch was queued ahead (the same
    // sys, hs and pre): the solve goes on after it
    const vk::Prelude* pre = nullptr;
    PreMode pm = PreMode::normal;
};
// Solves the systems together: every CG step streams X twice (once with
// onepass) for all still active systems; each keeps its own scalars and
// stopping rule.  The arguments are checked before anything is queued
vampomi_status pcg_run(vampomi_ctx* c, const std::vector<CgSystem*>& sys, const PcgArgs& args);
// plans the one-pass operator on this rank (c->opp, op_ok_mine, hs_ok_mine)
// and allocates its buffers (idempotent until the plan or the head-start
// switch changes); never a collective.  Sets op_ok / hs_ok: this rank's plan
// on one rank; on several the values op_agree agreed (both false before it)
vampomi_status op_prepare(vampomi_ctx* c);
// COLLECTIVE (several ranks; nothing on one): applies pending set_variant(3 /
// 5) requests, plans, and agrees op_ok and hs_ok over the ranks (both change
// the job's collective sequence; each rank planned from its own shard size,
// CU count and VAMPOMI_HEADSTART).  Called unconditionally by
// vampomi_vamp_begin, the one point every rank of a run reaches
vampomi_status op_agree(vampomi_ctx* c);
// whether pcg_run's head start can run on this context (plans the operator;
// the same answer on every rank)
vampomi_status headstart_available(vampomi_ctx* c, bool* yes);
// the smallest X shard at which the auto pre-step turns on (its bytes as stored; never below
// 256 MiB: the pinned default schedules of the small test shapes stay)
constexpr int64_t kPreMinBytes = (int64_t)256 << 20;
// whether the linear model's solves use the pre-step on this context (where
// the head start is available): c->pre_mode resolved
bool prestep_on(const vampomi_ctx* c);
// ... and which rule: 0 off, 1 the slot rule (one pre-step per solve, in a
// slot whose system has stopped), 3 two pre-steps per solve in a third
// operator slot (a 3-system plan exists; op_prepare has run)
int prestep_mode(const vampomi_ctx* c);
// whether auto (2) asks for rule 3 where it turns the pre-step on (C2: 210.9-213.3 against 197.3-199.4
// iterations/s under rule 1 in one job, profiles/prestep2.md)
constexpr bool kPreAutoThird = true;
// the context asks for rule 3 (pre_mode 3, or auto with kPreAutoThird), whether or not a 3-system plan exists
bool prestep_wants3(const vampomi_ctx* c);
// the device word a team launch sets when a hand-off timed out, and its host view
unsigned* op_err_dev(vampomi_ctx* c);
vampomi_status op_check_err(vampomi_ctx* c);
// d_k = tau*A^T q_k + gam2*p_k and A d_k (into op_nvec's A d block, /sqrt(N),
// summed over ranks with <d_k,p_k> at its tail; one rank: <d_k,p_k> in
// scal[SL_DP+k]) from one pass over X.  COLLECTIVE.  reduce = false (one
// rank only): the per-slot A d partials stay in op_part for cg_update to sum
// divide = false (several ranks): A d stays all-reduced but undivided, for a
// consumer that divides as it reads (cg_update's addiv)
vampomi_status op_dev(vampomi_ctx* c, int K, const vk::OpArgs& a, const int* gate, bool reduce = true,
                      bool divide = true);
// the head-start launch (c->opp_hs): op_dev's work for ONE system (a, K = 1),
// and out[kp] = A px[kp] (device ld, /sqrt(N), summed over ranks) for the
// kOpPlain plain right-hand sides, from the same pass over X.  One rank: the
// system's A d partials stay in op_part (opp_hs.nslots slots) for cg_update;
// several: its A d is op_nvec's A d block row 0, <d,p> at A d + (1 + kOpPlain)*ld.
// COLLECTIVE
vampomi_status op_dev_plain(vampomi_ctx* c, const vk::OpArgs& a, const double* const* px, double* const* out,
                            const int* gate);

// ---- covariates of the probit model (covariates.cpp) -----------------------------
// One evaluation of vamp::Newton_method_cov's sums (src/vamp_probit.cpp:536-551)
// at eta (host, C) with gg (device, N, may be null: zeros): H (C*C), rhs (C) and
// mlogL to the host (any may be null).  One host wait.
vampomi_status cov_eval_dev(vampomi_ctx* c, const double* gg, const double* eta, double* H, double* rhs,
                            double* mlogL);
// vamp::Newton_method_cov (:525-617) around the device sums, gg as above; eta
// (host, C) starts at eta0 (null: zeros).  iters: outer iterations run;
// backtracks / rel_err (may be null, >= 501 entries): per outer iteration.
// Rank-local: the N-side is replicated, every rank computes the same bits
vampomi_status cov_newton_dev(vampomi_ctx* c, const double* gg, const double* eta0, double* eta, int* iters,
                              int* backtracks, double* rel_err);
// m (device, N) = Z eta for eta on the host
vampomi_status cov_offset_dev(vampomi_ctx* c, const double* eta, double* m);
