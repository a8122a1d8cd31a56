// assoc.cpp — libvampomi: the association tests' entry points (--run-mode
// association_test): the leave-one-out test for one phenotype and for several,
// the leave-one-chromosome-out test with its label file and the lists its
// passes walk, and the SE p-values.  Nothing here runs during a VAMP
// iteration; the kernels are in assoc.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "hostio.h"

// The marker pass for KT phenotypes (vectors of stride ld in ymod, max(M, 1)
// in x1; KT blocks of 5*M sums into st), booked and launched: raw X once, the
// KT ymod and x1 vectors, the KT blocks of sums; per element 4 operations for
// the quotient and the x-only sums and 7 per phenotype (at KT = 1: 1 div, 2
// mul + 1 add for ym, 5 accumulations, 3 of them products).  KT = 1 runs the
// context's association variant.
// (Every width is booked into the one stats.loo record, which has no per-K
// records: its time is exact at timing period 1 only.  At a longer period it
// is the sampled mean times the launch count over launches of different widths
// and costs, so it is biased)
static vampomi_status loo_pass(vampomi_ctx* c, int KT, const double* ymod, const double* x1, double* st) {
    const double N = (double)c->N, M = (double)c->M, sqrtN = std::sqrt(N);
    TimedLaunch t = launch_stat(c, 2, KT, (double)c->esize() * N * M + 8.0 * N * KT + 8.0 * 6.0 * M * KT,
                                (4.0 + 7.0 * KT) * N * M);
    if (KT == 1)
        HIPCHK(vk::loo_sums(c->shard(), ymod, x1, sqrtN, st, c->st, c->loo_variant, vk::Timing{t.a, t.b}));
    else
        HIPCHK(vk::loo_multi_sums(c->shard(), KT, ymod, x1, sqrtN, st, c->st, vk::Timing{t.a, t.b}));
    c->stats.a_passes_exec++;
    return VAMPOMI_OK;
}

// What every test ends with: the p-values of n markers' sums in st, both
// handed out (where asked for), the stream drained and its samples resolved
static vampomi_status assoc_finish(vampomi_ctx* c, int64_t n, const double* st, double* pv, double* stats,
                                   double* pvals, int mem) {
    HIPCHK(vk::loo_pvals(n, st, (int)c->N, pv, c->st));
    if (stats) STCHK(stage_out(c, st, 5 * n, mem, stats));
    if (pvals) STCHK(stage_out(c, pv, n, mem, pvals));
    STCHK(sync_stream(c, c->st));
    if (c->timing) resolve_timing(c);
    return VAMPOMI_OK;
}

// --run-mode association_test --pval-method loo (src/main_meth.cpp:245-264,
// data::pvals_loo src/data.cpp:385-417).  COLLECTIVE (one A.x).
extern "C" vampomi_status vampomi_assoc_loo(vampomi_ctx* c, const double* est, double* pvals, double* stats,
                                            int mem) {
    CollScope cs_(c);
    if (!c || (!est && c->M > 0)) return fail(VAMPOMI_ERR_ARG, "null argument");
    if (!c->have_X || !c->have_y) return fail(VAMPOMI_ERR_STATE, "load methylation data and phenotype first");
    HIPCHK(hipSetDevice(c->device));
    const int64_t M = c->M, N = c->N, Mx = std::max<int64_t>(M, 1), ld = c->ld;
    double* e = c->mbuf;            // estimate-file values
    double* x1 = c->mbuf + Mx;      // x1_hat * sqrt(N)
    double* pv = c->mbuf + 2 * Mx;  // p-values
    double* st = c->mbuf + 3 * Mx;  // 5 sums per marker (slots 3..7)
    double* z1 = c->nbuf;
    double* ymod = c->nbuf + ld;
    STCHK(stage_in(c, est, M, mem, e));
    HIPCHK(vk::mul_scalar(M, e, std::sqrt((double)N), x1, c->st));  // :254-255
    const double* xs[1] = {x1};
    STCHK(ax_dev(c, 1, xs, z1));                                     // :257
    HIPCHK(vk::axpby(N, 1.0, c->y, -1.0, z1, ymod, c->st));          // y_mod = y - z1 (data.cpp:390-391)
    if (ld > N) HIPCHK(hipMemsetAsync(ymod + N, 0, (size_t)(ld - N) * 8, c->st));
    STCHK(loo_pass(c, 1, ymod, x1, st));                             // :393-416
    return assoc_finish(c, M, st, pv, stats, pvals, mem);
}

// vampomi_assoc_loo for T phenotypes with the shard read once per chunk of up
// to vk::kLooMultiMax of them: per chunk one batched A.x
// (none with est == NULL), ymod_t = y_t - z_t, one vk::loo_multi_sums (a chunk
// of one: vk::loo_sums), the p-values of the chunk's blocks.  Block t is bit
// for bit vampomi_set_phen(Y_t) + vampomi_assoc_loo(est_t) under the default
// association variant.  COLLECTIVE (one A.x per chunk; est is NULL on every
// rank or on none).
extern "C" vampomi_status vampomi_assoc_loo_multi(vampomi_ctx* c, int T, const double* Y, int64_t ldY,
                                                  int standardize, const double* est, double* pvals, double* stats,
                                                  int mem) {
    CollScope cs_(c);
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (T < 1) return fail(VAMPOMI_ERR_ARG, "assoc_loo_multi: T < 1");
    if (!Y) return fail(VAMPOMI_ERR_ARG, "assoc_loo_multi: null Y");
    if (ldY < c->N) return fail(VAMPOMI_ERR_ARG, "assoc_loo_multi: ldY < N");
    if (!c->have_X) return fail(VAMPOMI_ERR_STATE, "load methylation data first");
    HIPCHK(hipSetDevice(c->device));
    const int64_t M = c->M, N = c->N, Mx = std::max<int64_t>(M, 1), ld = c->ld;
    constexpr int KM = vk::kLooMultiMax;
    if (!c->am_n) {
        STCHK(dev_alloc(&c->am_n, (size_t)2 * KM * ld));
        HIPCHK(hipMemsetAsync(c->am_n, 0, (size_t)2 * KM * ld * 8, c->st));  // pad rows stay zero
    }
    if (!c->am_m) STCHK(dev_alloc(&c->am_m, (size_t)8 * KM * Mx));
    double* yd = c->am_n;                  // y_t
    double* ymod = c->am_n + KM * ld;      // y_t - z_t
    double* e = c->am_m;                   // estimate-file values
    double* x1 = c->am_m + KM * Mx;        // x1_hat * sqrt(N)
    double* pv = c->am_m + 2 * KM * Mx;    // p-values
    double* st = c->am_m + 3 * KM * Mx;    // KT blocks of 5 sums per marker
    double* z = c->nbuf;                   // A x1_t
    // every column as vampomi_set_phen prepares it (host; the context's own
    // phenotype is not touched)
    std::vector<double> yh((size_t)T * (size_t)N), col;
    for (int t = 0; t < T; ++t) {
        col.assign(Y + (int64_t)t * ldY, Y + (int64_t)t * ldY + N);
        adjust_phen(c, col);
        if (standardize) vio::standardize_phen(col);
        std::copy(col.begin(), col.end(), yh.begin() + (size_t)t * (size_t)N);
    }
    const double sqrtN = std::sqrt((double)N);
    for (int t0 = 0; t0 < T; t0 += KM) {
        const int KT = std::min(KM, T - t0);
        double* ym = est ? ymod : yd;  // without estimates ymod_t = y_t
        for (int k = 0; k < KT; ++k)
            HIPCHK(hipMemcpyAsync(yd + (int64_t)k * ld, yh.data() + (size_t)(t0 + k) * (size_t)N, (size_t)N * 8,
                                  hipMemcpyHostToDevice, c->st));
        if (est) {
            const double* xs[KM] = {};
            for (int k = 0; k < KT; ++k) {
                STCHK(stage_in(c, est + (int64_t)(t0 + k) * M, M, mem, e + k * Mx));
                HIPCHK(vk::mul_scalar(M, e + k * Mx, sqrtN, x1 + k * Mx, c->st));
                xs[k] = x1 + k * Mx;
            }
            STCHK(ax_dev(c, KT, xs, z));
            for (int k = 0; k < KT; ++k)
                HIPCHK(vk::axpby(N, 1.0, yd + (int64_t)k * ld, -1.0, z + (int64_t)k * ld, ymod + (int64_t)k * ld, c->st));
        } else {
            HIPCHK(hipMemsetAsync(x1, 0, (size_t)KT * Mx * 8, c->st));
        }
        STCHK(loo_pass(c, KT, ym, x1, st));
        STCHK(assoc_finish(c, (int64_t)KT * M, st, pv, stats ? stats + (int64_t)t0 * 5 * M : nullptr,
                           pvals ? pvals + (int64_t)t0 * M : nullptr, mem));
    }
    return VAMPOMI_OK;
}

// ---------------------------------------------------------------------------
// leave-one-chromosome-out test
// ---------------------------------------------------------------------------
namespace vk {

// The lists both passes walk.  A label's markers are not contiguous in an
// array-ordered file, so the local markers are sorted by (label, index) and
// the sorted list is cut twice, never across a label: into chunks of at most
// kSegChunk columns (equal shares of a label's run) for the segmented A.x,
// and into groups of kLocoG columns (a label's last group padded with -1) for
// the marker pass.
void seg_lists(const int32_t* labels, int64_t M, int G, SegLists* out) {
    SegLists& L = *out;
    std::vector<int32_t> count(G + 1, 0);
    for (int64_t i = 0; i < M; ++i) count[labels[i] + 1]++;
    for (int c = 0; c < G; ++c) count[c + 1] += count[c];  // label c's run is [count[c], count[c + 1])
    L.cols.assign((size_t)M, 0);
    {
        std::vector<int32_t> at(count.begin(), count.end() - 1);
        for (int64_t i = 0; i < M; ++i) L.cols[at[labels[i]]++] = (int32_t)i;  // stable: ascending index inside a label
    }
    L.chunk_at.clear();
    L.lab_chunk.assign(1, 0);
    L.grp_col.clear();
    L.grp_lab.clear();
    for (int c = 0; c < G; ++c) {
        const int64_t b = count[c], n = count[c + 1] - b;
        const int64_t nch = (n + kSegChunk - 1) / kSegChunk;
        for (int64_t k = 0; k < nch; ++k) L.chunk_at.push_back((int32_t)(b + k * n / nch));
        L.lab_chunk.push_back((int32_t)L.chunk_at.size());
        for (int64_t i = 0; i < n; i += kLocoG) {
            for (int g = 0; g < kLocoG; ++g) L.grp_col.push_back(i + g < n ? L.cols[b + i + g] : -1);
            L.grp_lab.push_back(c);
        }
    }
    L.chunk_at.push_back((int32_t)M);
}

}  // namespace vk

// The leave-one-chromosome-out test: the segmented A.x over
// the markers sorted by (label, index), z and y_c, the marker pass against the
// phenotype of each marker's label.  COLLECTIVE (one all-reduce of G ld-vectors;
// none with est == NULL, which is NULL on every rank or on none).
extern "C" vampomi_status vampomi_assoc_loco(vampomi_ctx* c, const double* est, const int32_t* labels, int G,
                                             double* pvals, double* stats, double* resid, int mem) {
    CollScope cs_(c);
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (!labels && c->M > 0) return fail(VAMPOMI_ERR_ARG, "assoc_loco: null labels");
    if (G < 1 || G > vk::kSegMax)
        return fail(VAMPOMI_ERR_ARG, "assoc_loco: G = " + std::to_string(G) + " outside [1, " +
                                         std::to_string(vk::kSegMax) + "]");
    for (int64_t i = 0; i < c->M; ++i)
        if (labels[i] < 0 || labels[i] >= G)
            return fail(VAMPOMI_ERR_ARG, "assoc_loco: label " + std::to_string(labels[i]) + " of marker " +
                                             std::to_string(i) + " outside [0, " + std::to_string(G) + ")");
    if (!c->have_X || !c->have_y) return fail(VAMPOMI_ERR_STATE, "load methylation data and phenotype first");
    HIPCHK(hipSetDevice(c->device));
    const int64_t M = c->M, N = c->N, Mx = std::max<int64_t>(M, 1), ld = c->ld;
    vk::SegLists L;
    vk::seg_lists(labels, M, G, &L);
    const int nchunks = L.nchunks(), ngroups = L.ngroups();
    // the lists in one device block: cols, chunk_at, lab_chunk, grp_col, grp_lab
    const int64_t o_chunk = M, o_lab = o_chunk + nchunks + 1, o_gcol = o_lab + G + 1,
                  o_glab = o_gcol + (int64_t)ngroups * vk::kLocoG, words = o_glab + ngroups;
    if (words > c->lc_idx_cap) {
        if (c->lc_idx) (void)hipFree(c->lc_idx);
        c->lc_idx = nullptr;
        c->lc_idx_cap = 0;
        // (what any labelling of this shard needs, so a later call does not grow it)
        const int64_t cap = M + vk::seg_max_chunks(M) + 1 + vk::kSegMax + 1 + vk::seg_max_groups(M) * (vk::kLocoG + 1);
        hipError_t e = hipMalloc((void**)&c->lc_idx, (size_t)cap * sizeof(int32_t));
        if (e != hipSuccess) return fail(VAMPOMI_ERR_OOM, std::string("hipMalloc(label lists): ") + hipGetErrorString(e));
        c->lc_idx_cap = cap;
    }
    std::vector<int32_t> host((size_t)words);
    std::copy(L.cols.begin(), L.cols.end(), host.begin());
    std::copy(L.chunk_at.begin(), L.chunk_at.end(), host.begin() + o_chunk);
    std::copy(L.lab_chunk.begin(), L.lab_chunk.end(), host.begin() + o_lab);
    std::copy(L.grp_col.begin(), L.grp_col.end(), host.begin() + o_gcol);
    std::copy(L.grp_lab.begin(), L.grp_lab.end(), host.begin() + o_glab);
    HIPCHK(hipMemcpyAsync(c->lc_idx, host.data(), (size_t)words * sizeof(int32_t), hipMemcpyHostToDevice, c->st));
    STCHK(sync_stream(c, c->st));  // host is a local: the copy has left it
    double* pv = c->mbuf + 2 * Mx;  // p-values
    double* st = c->mbuf + 3 * Mx;  // 5 sums per marker
    const double* ys = c->y;        // est == NULL: every y_c is y
    int64_t ldy = 0;
    if (est) {
        if (G > c->lc_G) {
            dev_free(c->lc_z);
            c->lc_G = 0;
            STCHK(dev_alloc(&c->lc_z, (size_t)G * ld));
            HIPCHK(hipMemsetAsync(c->lc_z, 0, (size_t)G * ld * 8, c->st));  // pad rows stay zero
            c->lc_G = G;
        }
        if (nchunks > c->lc_slots) {
            dev_free(c->lc_part);
            c->lc_slots = 0;
            STCHK(dev_alloc(&c->lc_part, (size_t)nchunks * ld));
            c->lc_slots = nchunks;
        }
        double* e = c->mbuf;        // estimate-file values
        double* x1 = c->mbuf + Mx;  // x1_hat * sqrt(N)
        STCHK(stage_in(c, est, M, mem, e));
        HIPCHK(vk::mul_scalar(M, e, std::sqrt((double)N), x1, c->st));
        // X once, the lists and x1, one slot per chunk written and read back
        TimedLaunch t = launch_stat(c, 0, 1, pass_bytes(c, 1) + 16.0 * (double)N * nchunks, pass_flops(c, 1));
        HIPCHK(vk::ax_seg_partial(c->shard(), x1, c->lc_idx, c->lc_idx + o_chunk, nchunks, c->lc_part, c->st,
                                  vk::Timing{t.a, t.b}));
        c->stats.a_passes_exec++;
        if (!c->use_comm) {
            HIPCHK(vk::ax_seg_reduce(G, N, ld, c->lc_idx + o_lab, c->lc_part, c->lc_z, c->sqrtN, c->st));
            HIPCHK(vk::loco_resid(G, N, ld, c->y, c->lc_z, 0.0, c->st));
        } else {
            HIPCHK(vk::ax_seg_reduce(G, N, ld, c->lc_idx + o_lab, c->lc_part, c->lc_z, 0.0, c->st));
            STCHK(allreduce_dev(c, c->lc_z, (size_t)G * ld));  // ONE all-reduce for all G vectors
            HIPCHK(vk::loco_resid(G, N, ld, c->y, c->lc_z, c->sqrtN, c->st));
        }
        ys = c->lc_z;
        ldy = ld;
    }
    // raw X once, G phenotypes, the lists, five sums per marker; per element 5
    // accumulations (3 of them products) less the two shared ones of a group
    TimedLaunch t = launch_stat(c, 2, 1,
                                (double)c->esize() * (double)N * (double)M + 8.0 * (double)N * (est ? G : 1) +
                                    8.0 * 6.0 * (double)M,
                                7.0 * (double)N * (double)M);
    HIPCHK(vk::loco_sums(c->shard(), ys, ldy, c->lc_idx + o_gcol, c->lc_idx + o_glab, ngroups, st, c->st,
                         vk::Timing{t.a, t.b}));
    c->stats.a_passes_exec++;
    if (resid)
        for (int g = 0; g < G; ++g)
            HIPCHK(hipMemcpyAsync(resid + (int64_t)g * N, ys + (int64_t)g * ldy, (size_t)N * 8, hipMemcpyDeviceToHost,
                                  c->st));
    return assoc_finish(c, M, st, pv, stats, pvals, mem);
}

extern "C" vampomi_status vampomi_read_labels(const char* path, int64_t Mt, int32_t* labels, int* G, char* names,
                                              size_t names_cap) {
    if (!path || Mt < 0) return fail(VAMPOMI_ERR_ARG, "read_labels: null path or Mt < 0");
    std::vector<int32_t> lab;
    std::vector<std::string> nm;
    std::vector<int64_t> cnt;
    std::string err;
    switch (vio::read_labels(path, Mt, vk::kSegMax, lab, nm, cnt, &err)) {
        case 0: break;
        case -1: return fail(VAMPOMI_ERR_IO, err);
        default: return fail(VAMPOMI_ERR_ARG, err);
    }
    if (labels) std::copy(lab.begin(), lab.end(), labels);
    if (G) *G = (int)nm.size();
    if (names) {
        std::string all;
        for (const std::string& s : nm) all += s + "\n";
        if (all.size() + 1 > names_cap)
            return fail(VAMPOMI_ERR_ARG, "read_labels: names_cap holds " + std::to_string(names_cap) + " bytes, " +
                                             std::to_string(all.size() + 1) + " are needed");
        std::memcpy(names, all.c_str(), all.size() + 1);
    }
    return VAMPOMI_OK;
}

// --pval-method se (src/main_meth.cpp:218-242): rank-local
extern "C" vampomi_status vampomi_assoc_se(vampomi_ctx* c, const double* r1, double gam1, double* pvals, int mem) {
    if (!c || (!r1 && c->M > 0) || (!pvals && c->M > 0)) return fail(VAMPOMI_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t Mx = std::max<int64_t>(c->M, 1);
    STCHK(stage_in(c, r1, c->M, mem, c->mbuf));
    HIPCHK(vk::se_pvals(c->M, c->mbuf, gam1, c->N, c->mbuf + Mx, c->st));
    STCHK(stage_out(c, c->mbuf + Mx, c->M, mem, pvals));
    return VAMPOMI_OK;
}
