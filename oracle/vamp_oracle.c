/*
 * vamp_oracle.c — CPU restatement (C11 + OpenMP) of the gVAMPomi linear VAMP
 * hot path.  TEST INFRASTRUCTURE ONLY (see vamp_oracle.h header): tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg are the only users.
 *
 * Parity pins, by part:
 *  - the OPERATORS (A.x, A^T.u, marker statistics, read_phen) are pinned to
 *    the reference itself: its own src/data.cpp, compiled where it lies
 *    (oracle/Makefile target ref), on the reference-written data_sim.py files
 *    and a generated problem (tests/test_ref_pin.py, tests/golden/ref_data_pin.npz);
 *  - the ITERATION (g1/g1d, EM, PCG, Onsager, noise precision, probit) is
 *    parity unpinned: src/vamp.cpp / vamp_probit.cpp need Boost, absent here,
 *    so no reference-run vector exists; this file restates them function by
 *    function with file:line citations into /root/reference/src.
 * Deviations P1/P2: see vamp_oracle.h.
 *
 * Determinism: every reduction is blocked with a fixed block size and summed
 * in block order, so results do not depend on the OpenMP thread count.
 */
#define _GNU_SOURCE
#include "vamp_oracle.h"

#include <errno.h>
#include <fcntl.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------------- */
/* index-keyed generators                                                    */
/* ------------------------------------------------------------------------- */

uint64_t orc_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* replaces std::bernoulli_distribution(0.5)(std::random_device) of
 * src/vamp.cpp:142,295-296 (P2) */
int orc_bern_bit(uint64_t seed, int it, int64_t gidx) {
    uint64_t k = orc_splitmix64(seed ^ 0xB5AD4ECEDA1CE2A9ULL);
    uint64_t h = orc_splitmix64(k ^ (((uint64_t)(uint32_t)it << 40) ^ (uint64_t)gidx));
    return (int)(h >> 63);
}

/* Synthetic i.i.d. design (stands for simulation/data_sim.py:35, which draws
 * np.random.normal unseeded): Irwin-Hall sum of 12 dyadic 16-bit uniforms,
 * centred and unit-variance, exactly representable. */
double orc_gauss_dyadic(uint64_t seed, int64_t i, int64_t j) {
    uint64_t k = orc_splitmix64(orc_splitmix64(seed ^ 0x4741555353ULL) + (uint64_t)i);
    uint64_t acc = 0;
    for (uint64_t t = 0; t < 3; ++t) {
        uint64_t h = orc_splitmix64(k ^ (((uint64_t)j << 2) | t));
        acc += (h & 0xFFFFULL) + ((h >> 16) & 0xFFFFULL) + ((h >> 32) & 0xFFFFULL) + (h >> 48);
    }
    return (double)(2 * acc + 12) * (1.0 / 131072.0) - 6.0;
}

/* Methylation-like beta value: per-marker mean in
 * [51/1024, 972/1024], sd in [10/1024, 137/1024], clamped to [0,1]. */
double orc_meth_dyadic(uint64_t seed, int64_t i, int64_t j) {
    uint64_t hm = orc_splitmix64(orc_splitmix64(seed ^ 0x6D657468ULL) + (uint64_t)i);
    double mu = (double)(51 + (hm & 1023ULL) % 922ULL) * (1.0 / 1024.0);
    double sd = (double)(10 + ((hm >> 10) & 127ULL)) * (1.0 / 1024.0);
    double v = mu + sd * orc_gauss_dyadic(seed ^ 0x5A5A5A5AULL, i, j);
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

void orc_generate_markers(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M,
                          double* X) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < M; ++i) {
        double* col = X + i * ld;
        for (int64_t j = 0; j < N; ++j)
            col[j] = kind == 1 ? orc_meth_dyadic(seed, S + i, j) : orc_gauss_dyadic(seed, S + i, j);
        for (int64_t j = N; j < ld; ++j) col[j] = 0.0;
    }
}

/* ------------------------------------------------------------------------- */
/* reductions: src/utilities.cpp:138-162 inner_prod / l2_norm2 (deterministic)*/
/* ------------------------------------------------------------------------- */

#define ORC_BLK 2048

double orc_dot(const double* a, const double* b, int64_t n) {
    int64_t nb = (n + ORC_BLK - 1) / ORC_BLK;
    if (nb <= 1) {
        double s = 0.0;
        for (int64_t i = 0; i < n; ++i) s += a[i] * b[i];
        return s;
    }
    double* part = (double*)malloc(sizeof(double) * (size_t)nb);
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < nb; ++k) {
        int64_t lo = k * ORC_BLK, hi = lo + ORC_BLK < n ? lo + ORC_BLK : n;
        double s = 0.0;
        for (int64_t i = lo; i < hi; ++i) s += a[i] * b[i];
        part[k] = s;
    }
    double s = 0.0;
    for (int64_t k = 0; k < nb; ++k) s += part[k];
    free(part);
    return s;
}

typedef struct {
    const orc_problem* pb;
} orc_ctx;

static double allreduce1(const orc_problem* pb, double v) {
    if (pb->allreduce) pb->allreduce(&v, 1, pb->user);
    return v;
}

/* ------------------------------------------------------------------------- */
/* Association modes (sensitivity measurement for the probit parity bar,      */
/* tests/golden/make_c4_spread.py; ORC_ASSOC_DEFAULT otherwise).  The same    */
/* arithmetic, the sums grouped differently:                                   */
/*  - ORC_ASSOC_DEVICE (T, grid): as the MI355X engine groups them at its      */
/*    team plan (vampomi_amd/csrc): a reduction over n elements on nblk blocks */
/*    of 256 threads (thread t of block b takes e = 256 b + t, + 256 nblk, ... */
/*    in order; a block adds its 4 waves' xor-butterfly sums in wave order;    */
/*    the last block's thread t adds the partials of blocks t, t + 256, ...,   */
/*    then the same butterfly and wave order: dots_part / block_put_sums /     */
/*    red_final: vec.hip, kdev.h) with nblk = red_blocks(n) for the dots, the  */
/*    CG's cg_init / cg_update sums and the denoisers' sums, ceil(M/256) for   */
/*    the EM round's (em_kernel); the CG's <d,p> as the one-pass operator      */
/*    forms it (each workgroup over the columns its team member owns, then    */
/*    lanes over workgroups: atax_team.hip, ticket_sum_blocks in kdev.h); the  */
/*    CG's beta from the correctly rounded 1/rz (kdev.h cg_decide_into).       */
/*  - ORC_ASSOC_REFRUN (threads, seed): as ONE rank of the reference sums with */
/*    OMP_NUM_THREADS = threads: inner_prod's `omp parallel for reduction`     */
/*    (src/utilities.cpp:138-158) gives each thread a contiguous static chunk, */
/*    summed in order, and adds the threads' sums in arrival order (here a     */
/*    seeded random order per call); sum_d and the EM sums are the reference's */
/*    sequential loops (src/vamp_probit.cpp:120-124, src/vamp.cpp:576,590-593).*/
/* Only single-rank runs use the non-default modes (the call counter of the    */
/* arrival order is shared).                                                   */
/* ------------------------------------------------------------------------- */
static int g_assoc = ORC_ASSOC_DEFAULT;
static int g_dev_T = 1, g_dev_grid = 256, g_ref_threads = 1;
static uint64_t g_ref_seed = 0, g_ref_calls = 0;

void orc_set_assoc(int mode, int a, int b, uint64_t seed) {
    g_assoc = mode;
    g_dev_T = mode == ORC_ASSOC_DEVICE && a > 0 ? a : 1;
    g_dev_grid = mode == ORC_ASSOC_DEVICE && b > 0 ? b : 256;
    g_ref_threads = mode == ORC_ASSOC_REFRUN && a > 0 ? a : 1;
    g_ref_seed = seed;
    g_ref_calls = 0;
}

/* the xor butterfly over 64 lanes (kdev.h wave_sum): every lane ends with the
 * same value, lane 0's tree: (l, l + o) for o = 32, 16, ..., 1 */
static double wave64(const double* v) {
    double t[64];
    memcpy(t, v, sizeof t);
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) t[l] = t[l] + t[l + o];
    return t[0];
}

/* 256 threads' values: each wave's butterfly, the 4 wave sums in order */
static double block256(const double* th) {
    return ((wave64(th) + wave64(th + 64)) + wave64(th + 128)) + wave64(th + 192);
}

static int dev_red_blocks(int64_t n) { /* vec.hip red_blocks */
    int64_t b = (n + 511) / 512;
    if (b < 1) b = 1;
    if (b > 1024) b = 1024;
    return (int)b;
}

static int dev_cg_blocks(int64_t M) { /* pcg.hip cg_update: mblocks (2 elements per thread) */
    int64_t b = (M + 511) / 512;
    if (b < 1) b = 1;
    if (b > 512) b = 512;
    return (int)b;
}

/* sum over e < n of a[e] * b[e] (b null: a[e]) grouped as a device reduction on nblk blocks */
static double dev_red(const double* a, const double* b, int64_t n, int nblk) {
    const int64_t stride = (int64_t)nblk * 256;
    double* part = (double*)malloc(sizeof(double) * (size_t)nblk);
#pragma omp parallel for schedule(static)
    for (int bk = 0; bk < nblk; ++bk) {
        double th[256];
        for (int t = 0; t < 256; ++t) {
            double acc = 0.0;
            for (int64_t e = (int64_t)bk * 256 + t; e < n; e += stride) acc += b ? a[e] * b[e] : a[e];
            th[t] = acc;
        }
        part[bk] = block256(th);
    }
    double th[256];
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (int bk = t; bk < nblk; bk += 256) acc += part[bk];
        th[t] = acc;
    }
    free(part);
    return block256(th);
}

/* <d, p> as the one-pass team operator forms it (grid workgroups, teams of T,
 * teams of one XCD numbered together: atax_team.hip); each workgroup's sum
 * over the columns its member owns, in column order, then lane l adds
 * workgroups l, l + 64, ... and the butterfly */
static double dev_dp(const double* d, const double* p, int64_t M, int T, int grid) {
    const int nteams = grid / T;
    double* part = (double*)calloc((size_t)grid, sizeof(double));
#pragma omp parallel for schedule(static)
    for (int bk = 0; bk < grid; ++bk) {
        const int g = bk >> 3, member = g % T;
        const int team = g / T + (nteams >> 3) * (bk & 7);
        /* teams of T > 1: interleaved columns (configurations 2-5); T = 1: a
         * contiguous range per workgroup (configurations 0-1) */
        const int ilv = T > 1;
        const int64_t mb = ilv ? team : (int64_t)team * M / nteams;
        const int64_t n = ilv ? (team < M ? (M - team + nteams - 1) / nteams : 0)
                              : (int64_t)(team + 1) * M / nteams - mb;
        const int64_t cs = ilv ? nteams : 1;
        double acc = 0.0;
        for (int64_t m = 0; m < n; ++m)
            if ((m & (T - 1)) == member) {
                const int64_t col = mb + m * cs;
                acc += d[col] * p[col];
            }
        part[bk] = acc;
    }
    double lanes[64];
    for (int l = 0; l < 64; ++l) {
        double acc = 0.0;
        for (int bk = l; bk < grid; bk += 64) acc += part[bk];
        lanes[l] = acc;
    }
    free(part);
    return wave64(lanes);
}

/* inner_prod's local sum in the reference's OpenMP form (REFRUN) */
static double refrun_inner(const double* a, const double* b, int64_t n) {
    const int T = g_ref_threads;
    double part[1024];
    int order[1024];
    const int nt = T < 1024 ? T : 1024;
    const int64_t q = n / nt, r = n % nt;
    int64_t lo = 0;
    for (int t = 0; t < nt; ++t) {
        const int64_t len = q + (t < r ? 1 : 0);
        double acc = 0.0;
        for (int64_t i = lo; i < lo + len; ++i) acc += a[i] * b[i];
        part[t] = acc;
        lo += len;
        order[t] = t;
    }
    uint64_t h = orc_splitmix64(g_ref_seed ^ orc_splitmix64(++g_ref_calls));
    for (int t = nt - 1; t > 0; --t) { /* Fisher-Yates: the arrival order of the threads' sums */
        h = orc_splitmix64(h);
        const int j = (int)(h % (uint64_t)(t + 1));
        const int x = order[t];
        order[t] = order[j];
        order[j] = x;
    }
    double s = 0.0;
    for (int t = 0; t < nt; ++t) s += part[order[t]];
    return s;
}

static double seq_dot(const double* a, const double* b, int64_t n) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += a[i] * b[i];
    return s;
}

/* the kind of sum a call site is (it picks the grouping in the non-default modes) */
enum { SUM_INNER = 0, SUM_CG = 1, SUM_ACC_M = 2, SUM_EM = 3, SUM_ACC_N = 4 };

static double assoc_sum(const double* a, const double* b, int64_t n, int kind) {
    if (g_assoc == ORC_ASSOC_DEVICE) {
        const int nblk = kind == SUM_CG ? dev_cg_blocks(n) : kind == SUM_EM ? (int)((n + 255) / 256) : dev_red_blocks(n);
        return dev_red(a, b, n, nblk > 0 ? nblk : 1);
    }
    if (g_assoc == ORC_ASSOC_REFRUN) return kind == SUM_INNER || kind == SUM_CG ? refrun_inner(a, b, n) : seq_dot(a, b, n);
    return orc_dot(a, b, n);
}

/* one sum of the current association mode (kind: 0 inner_prod, 1 the CG's
 * sums, 2 sum over M (sum_d), 3 the EM round's, 4 sum over N; tests) */
double orc_assoc_dot(const double* a, const double* b, int64_t n, int kind) { return assoc_sum(a, b, n, kind); }
/* the CG's <d, p> as the device's operator forms it at plan (T, grid) (tests) */
double orc_dev_dp(const double* d, const double* p, int64_t M, int T, int grid) { return dev_dp(d, p, M, T, grid); }

/* inner_prod(u, v, sync) — src/utilities.cpp:138-158 */
static double inner_prod_k(const orc_problem* pb, const double* a, const double* b, int64_t n, int sync, int kind) {
    double s = assoc_sum(a, b, n, kind);
    return sync ? allreduce1(pb, s) : s;
}
static double inner_prod(const orc_problem* pb, const double* a, const double* b, int64_t n,
                         int sync) {
    return inner_prod_k(pb, a, b, n, sync, SUM_INNER);
}

/* ------------------------------------------------------------------------- */
/* divide_work — src/utilities.cpp:207-239                                    */
/* ------------------------------------------------------------------------- */
void orc_divide_work(int64_t Mt, int nranks, int rank, int64_t* M, int64_t* S, int64_t* Mm) {
    int64_t modu = Mt % nranks, size = Mt / nranks, cum = 0;
    for (int r = 0; r < nranks; ++r) {
        int64_t len = r < modu ? size + 1 : size;
        if (r == rank) {
            *M = len;
            *S = cum;
        }
        cum += len;
    }
    if (Mm) *Mm = modu != 0 ? size + 1 : size;
}

/* ------------------------------------------------------------------------- */
/* read_phen — src/data.cpp:58-110                                            */
/* ------------------------------------------------------------------------- */
void orc_standardize_phen(double* y, int64_t n) {
    /* src/data.cpp:97-104: avg from the running sum; scale only, no centring */
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) sum += y[i];
    double avg = sum / (double)n;
    double sqn = 0.0;
    for (int64_t i = 0; i < n; ++i)
        if (y[i] != DBL_MAX) sqn += (y[i] - avg) * (y[i] - avg);
    sqn = sqrt((double)(n - 1) / sqn);
    for (int64_t i = 0; i < n; ++i) y[i] *= sqn;
}

int64_t orc_read_phen(const char* path, int standardize, double* y, int64_t cap,
                      double* intercept, double* scale) {
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    char* line = NULL;
    size_t lcap = 0;
    ssize_t len;
    int64_t n = 0;
    double sum = 0.0;
    while ((len = getline(&line, &lcap, f)) != -1) {
        if (len > 0 && line[len - 1] == '\n') line[--len] = '\0';
        /* std::regex("\\s+") token split with -1: leading whitespace yields an
         * empty first token; tokens[2] is the third field counted that way. */
        char* p = line;
        int tok = 0;
        char* t2 = NULL;
        char* start = p;
        for (;;) {
            char* q = start;
            while (*q && !(*q == ' ' || *q == '\t' || *q == '\r' || *q == '\v' || *q == '\f')) ++q;
            if (tok == 2) {
                t2 = start;
                if (*q) *q = '\0';
                break;
            }
            if (!*q) break;
            while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\v' || *q == '\f') ++q;
            start = q;
            ++tok;
            if (!*start) break; /* trailing separator: regex iterator yields no empty suffix */
        }
        if (!t2) continue;
        if (strcmp(t2, "NA") == 0) {
            free(line);
            fclose(f);
            return -2; /* src/data.cpp:73-74 throw "NAN in data!" */
        }
        if (n < cap) y[n] = atof(t2);
        sum += atof(t2);
        ++n;
    }
    free(line);
    fclose(f);
    if (intercept) *intercept = 0.0;
    if (scale) *scale = 1.0;
    if (standardize && n > 1) {
        double avg = sum / (double)n;
        double sqn = 0.0;
        for (int64_t i = 0; i < n && i < cap; ++i)
            if (y[i] != DBL_MAX) sqn += (y[i] - avg) * (y[i] - avg);
        sqn = sqrt((double)(n - 1) / sqn);
        for (int64_t i = 0; i < n && i < cap; ++i) y[i] *= sqn;
        if (intercept) *intercept = avg;
        if (scale) *scale = sqn;
    }
    return n;
}

/* ------------------------------------------------------------------------- */
/* compute_markers_statistics — src/data.cpp:233-283                          */
/* ------------------------------------------------------------------------- */
void orc_marker_stats(const double* X, int64_t N, int64_t ld, int64_t M, int64_t nonas,
                      double alpha_scale, double* mave, double* msig) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < M; ++i) {
        const double* m = X + i * ld;
        double suma = 0.0;
        for (int64_t j = 0; j < N; ++j) suma += m[j];
        mave[i] = suma / (double)nonas;
        double sumsqr = 0.0;
        for (int64_t j = 0; j < N; ++j) {
            double val = m[j] - mave[i];
            sumsqr += val * val;
        }
        if (sumsqr != 0.0) {
            if (alpha_scale == 1.0)
                msig[i] = 1.0 / sqrt(sumsqr / ((double)nonas - 1.0));
            else
                msig[i] = 1.0 / pow(sqrt(sumsqr / ((double)nonas - 1.0)), alpha_scale);
        } else {
            msig[i] = 1.0;
        }
    }
}

/* ------------------------------------------------------------------------- */
/* Ax — src/data.cpp:340-373 (same per-element summation order: markers in    */
/* index order, one running sum per sample)                                   */
/* ------------------------------------------------------------------------- */
#define ORC_ROWBLK 2048
void orc_ax_local(const double* X, int64_t N, int64_t ld, int64_t M, const double* mave,
                  const double* msig, const double* x, double* out) {
    int64_t nb = (N + ORC_ROWBLK - 1) / ORC_ROWBLK;
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < nb; ++b) {
        int64_t lo = b * ORC_ROWBLK, hi = lo + ORC_ROWBLK < N ? lo + ORC_ROWBLK : N;
        double acc[ORC_ROWBLK];
        for (int64_t j = lo; j < hi; ++j) acc[j - lo] = 0.0;
        for (int64_t i = 0; i < M; ++i) {
            const double* m = X + i * ld;
            double ave = mave[i];
            double sig_phen_i = msig[i] * x[i];
            for (int64_t j = lo; j < hi; ++j) acc[j - lo] += (m[j] - ave) * sig_phen_i;
        }
        for (int64_t j = lo; j < hi; ++j) out[j] = acc[j - lo];
    }
}

void orc_ax(const double* X, int64_t N, int64_t ld, int64_t M, const double* mave,
            const double* msig, const double* x, double* out, orc_allreduce_fn ar, void* user) {
    orc_ax_local(X, N, ld, M, mave, msig, x, out);
    if (ar) ar(out, N, user); /* MPI_Allreduce(N) src/data.cpp:367 */
    double sq = sqrt((double)N);
    for (int64_t j = 0; j < N; ++j) out[j] /= sq; /* src/data.cpp:369-370 */
}

/* Sensitivity mode (test infrastructure, off by default): with B > 0 the
 * per-marker sum over samples of orc_atx runs in blocks of B rows whose sums
 * are combined in block order -- the kind of reassociation every parallel
 * A^T.u has (the device splits a column's rows over lanes, waves and team
 * members).  Together with the virtual-shard runs (tests/_data.py, many ranks:
 * the sums over markers split) it measures how far the reference's own result
 * moves under a change of summation order (tests/golden/make_c4_window.py). */
static int g_atx_block = 0;
void orc_set_atx_block(int B) { g_atx_block = B > 0 ? B : 0; }

/* ATx / dot_product — src/data.cpp:294-333 */
void orc_atx(const double* X, int64_t N, int64_t ld, int64_t M, const double* mave,
             const double* msig, const double* u, double* out) {
    const int64_t B = g_atx_block;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < M; ++i) {
        const double* m = X + i * ld;
        double mu = mave[i];
        double dpa = 0.0;
        if (B > 0) {
            for (int64_t lo = 0; lo < N; lo += B) {
                const int64_t hi = lo + B < N ? lo + B : N;
                double b = 0.0;
                for (int64_t j = lo; j < hi; ++j) b += (m[j] - mu) * u[j];
                dpa += b;
            }
        } else {
            for (int64_t j = 0; j < N; ++j) dpa += (m[j] - mu) * u[j];
        }
        out[i] = msig[i] * dpa;
    }
    double scale = 1.0 / sqrt((double)N);
    for (int64_t i = 0; i < M; ++i) out[i] *= scale;
}

/* ------------------------------------------------------------------------- */
/* g1 / g1d — src/vamp.cpp:440-492                                           */
/* ------------------------------------------------------------------------- */
/* std::max / std::min semantics (NaN in the first argument propagates) */
static double smax(double a, double b) { return (a < b) ? b : a; }
static double smin(double a, double b) { return (b < a) ? b : a; }

static double vmax(const double* v, int L) {
    double m = v[0];
    for (int i = 1; i < L; ++i)
        if (v[i] > m) m = v[i];
    return m;
}

double orc_g1(double y, double gam1, const double* probs, const double* vars, int L) {
    double sigma = 1 / gam1;
    double eta_max = vmax(vars, L);
    double pk = 0, pkd = 0;
    if (sigma < 1e-10 && sigma > -1e-10) return y;
    for (int i = 0; i < L; ++i) {
        double expe_sum = -0.5 * (y * y) * (eta_max - vars[i]) / (vars[i] + sigma) / (eta_max + sigma);
        double z = probs[i] / sqrt(vars[i] + sigma) * exp(expe_sum);
        pk = pk + z;
        z = z / (vars[i] + sigma) * y;
        pkd = pkd - z;
    }
    return y + sigma * pkd / pk;
}

double orc_g1d(double y, double gam1, const double* probs, const double* vars, int L) {
    double sigma = 1 / gam1;
    double eta_max = vmax(vars, L);
    double pk = 0, pkd = 0, pkdd = 0;
    if (sigma < 1e-10 && sigma > -1e-10) return 1;
    for (int i = 0; i < L; ++i) {
        double expe_sum = -0.5 * (y * y) * (eta_max - vars[i]) / (vars[i] + sigma) / (eta_max + sigma);
        double z = probs[i] / sqrt(vars[i] + sigma) * exp(expe_sum);
        pk = pk + z;
        z = z / (vars[i] + sigma) * y;
        pkd = pkd - z;
        double z2 = z / (vars[i] + sigma) * y;
        pkdd = pkdd - probs[i] / pow(vars[i] + sigma, 1.5) * exp(expe_sum) + z2;
    }
    double q = pkd / pk;
    return 1 + sigma * (pkdd / pk - q * q);
}

/* ------------------------------------------------------------------------- */
/* output writers                                                            */
/* ------------------------------------------------------------------------- */

/* mpi_store_vec_to_file — src/utilities.cpp:241-249: CREATE|WRONLY, no
 * truncation, M doubles at byte offset S*8 */
int orc_store_vec(const char* path, const double* v, int64_t S, int64_t M) {
    int fd = open(path, O_CREAT | O_WRONLY, 0666);
    if (fd < 0) return -1;
    size_t want = (size_t)M * sizeof(double);
    ssize_t w = pwrite(fd, v, want, (off_t)S * (off_t)sizeof(double));
    close(fd);
    return w == (ssize_t)want ? 0 : -1;
}

/* setup_io (src/vamp.cpp:854-882) + write_ofile_csv_header
 * (src/utilities.cpp:388-401): delete, create exclusively, header at 0 */
int orc_csv_header(const char* path, const char* const* fields, int n) {
    unlink(path);
    int fd = open(path, O_CREAT | O_WRONLY | O_EXCL, 0666);
    if (fd < 0) return -1;
    size_t tot = 2;
    for (int i = 0; i < n; ++i) tot += strlen(fields[i]) + 2;
    char* s = (char*)malloc(tot);
    s[0] = '\0';
    for (int i = 0; i < n; ++i) {
        if (i) strcat(s, ", ");
        strcat(s, fields[i]);
    }
    strcat(s, "\n");
    ssize_t w = pwrite(fd, s, strlen(s), 0);
    close(fd);
    int ok = w == (ssize_t)strlen(s);
    free(s);
    return ok ? 0 : -1;
}

/* write_ofile_csv — src/utilities.cpp:366-385: "%5d" + ", %20.15f"*n + "\n"
 * written at byte offset it * strlen(row) */
int orc_csv_row(const char* path, int it, const double* vals, int n) {
    char buf[50000];
    int cx = snprintf(buf, sizeof buf, "%5d", it);
    for (int i = 0; i < n; ++i) cx += snprintf(buf + cx, sizeof buf - (size_t)cx, ", %20.15f", vals[i]);
    cx += snprintf(buf + cx, sizeof buf - (size_t)cx, "\n");
    int fd = open(path, O_WRONLY);
    if (fd < 0) return -1;
    ssize_t w = pwrite(fd, buf, (size_t)cx, (off_t)it * (off_t)cx);
    close(fd);
    return w == cx ? 0 : -1;
}

/* ------------------------------------------------------------------------- */
/* the VAMP state                                                            */
/* ------------------------------------------------------------------------- */
typedef struct {
    const orc_problem* pb;
    int64_t N, M, Mt;
    int L;
    double probs[ORC_MAX_L], vars[ORC_MAX_L];
    double gam1, gam2, gamw;
    double* r1;
    double* bern_vec;
    double* invQ_bern_vec;
    double* mu_CG_last;
    double* x2_hat;
    int64_t passes;
    int cg_iters_last;
    /* params */
    int CG_max_iter, EM_max_iter, learn_vars, verbosity;
    double CG_err_tol, EM_err_thr, merge_vars_thr;
} orc_vamp;

static void ax(orc_vamp* s, const double* x, double* out) {
    const orc_problem* pb = s->pb;
    orc_ax(pb->X, pb->N, pb->ld, pb->M, pb->mave, pb->msig, x, out, pb->allreduce, pb->user);
    s->passes++;
}

static void atx(orc_vamp* s, const double* u, double* out) {
    const orc_problem* pb = s->pb;
    orc_atx(pb->X, pb->N, pb->ld, pb->M, pb->mave, pb->msig, u, out);
    s->passes++;
}

static int all_zero(const double* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (v[i] != 0.0) return 0;
    return 1;
}

/* lmmse_mult — src/vamp.cpp:645-662: tau*A^T(A v) + gam2*v; local zero check */
static void lmmse_mult(orc_vamp* s, const double* v, double tau, double* res, double* tmpN) {
    int64_t M = s->M;
    if (all_zero(v, M)) {
        memset(res, 0, sizeof(double) * (size_t)M);
        return;
    }
    ax(s, v, tmpN);
    atx(s, tmpN, res);
    for (int64_t i = 0; i < M; ++i) {
        res[i] *= tau;
        res[i] += s->gam2 * v[i];
    }
}

/* precondCG_solver — src/vamp.cpp:664-757 */
static void precondCG(orc_vamp* s, const double* v, const double* mu_start, double tau, int denoiser,
                      double* mu_out) {
    const orc_problem* pb = s->pb;
    int64_t M = s->M, N = s->N;
    double diag = tau * (double)(N - 1) / (double)N + s->gam2; /* :676-677 */
    double* mu = mu_out;
    memcpy(mu, mu_start, sizeof(double) * (size_t)M);
    double* r = (double*)malloc(sizeof(double) * (size_t)M);
    double* z = (double*)malloc(sizeof(double) * (size_t)M);
    double* p = (double*)malloc(sizeof(double) * (size_t)M);
    double* d = (double*)malloc(sizeof(double) * (size_t)M);
    double* tmpN = (double*)malloc(sizeof(double) * (size_t)N);
    lmmse_mult(s, mu, tau, r, tmpN);
    for (int64_t i = 0; i < M; ++i) r[i] = v[i] - r[i];
    for (int64_t i = 0; i < M; ++i) z[i] = r[i] / diag;
    memcpy(p, z, sizeof(double) * (size_t)M);
    double prev_onsager = 0;
    int it_done = 0;
    double norm_v = sqrt(inner_prod_k(pb, v, v, M, 1, SUM_CG));
    for (int i = 0; i < s->CG_max_iter; ++i) {
        it_done = i + 1;
        lmmse_mult(s, p, tau, d, tmpN);
        double rz = inner_prod_k(pb, r, z, M, 1, SUM_CG);
        double dp = g_assoc == ORC_ASSOC_DEVICE ? allreduce1(pb, dev_dp(d, p, M, g_dev_T, g_dev_grid))
                                                : inner_prod_k(pb, d, p, M, 1, SUM_CG);
        double alpha = rz / dp;
        for (int64_t j = 0; j < M; ++j) mu[j] += alpha * p[j];
        if (denoiser == 0) {
            double onsager = s->gam2 * inner_prod_k(pb, v, mu, M, 1, SUM_CG);
            double rel_err = onsager != 0 ? fabs((onsager - prev_onsager) / onsager) : 1;
            if (rel_err < 1e-8) break;
            prev_onsager = onsager;
        }
        double beta = g_assoc == ORC_ASSOC_DEVICE ? 1.0 / rz : pow(rz, -1); /* :731 */
        for (int64_t j = 0; j < M; ++j) r[j] -= d[j] * alpha;
        for (int64_t j = 0; j < M; ++j) z[j] = r[j] / diag;
        beta *= inner_prod_k(pb, r, z, M, 1, SUM_CG);
        for (int64_t j = 0; j < M; ++j) p[j] = z[j] + beta * p[j];
        double rel_err = sqrt(inner_prod_k(pb, r, r, M, 1, SUM_CG)) / norm_v;
        if (s->verbosity >= 2 && pb->rank == 0)
            printf("[CG] it = %d: ||r_it|| / ||RHS|| = %g\n", i, rel_err);
        if (rel_err < s->CG_err_tol) break;
    }
    s->cg_iters_last = it_done;
    if (denoiser == 1) memcpy(s->mu_CG_last, mu, sizeof(double) * (size_t)M);
    free(r);
    free(z);
    free(p);
    free(d);
    free(tmpN);
}

/* updatePrior — src/vamp.cpp:531-643 */
static void update_prior(orc_vamp* s) {
    const orc_problem* pb = s->pb;
    int64_t M = s->M;
    double noise_var = 1 / s->gam1;
    double lambda = 1 - s->probs[0];
    double omegas[ORC_MAX_L];
    for (int j = 0; j < s->L; ++j) omegas[j] = s->probs[j];
    for (int j = 1; j < s->L; ++j) omegas[j] /= lambda;
    const double* r1 = s->r1;
    for (int it = 0; it < s->EM_max_iter; ++it) {
        int L = s->L, Lm = L - 1;
        double max_sigma = vmax(s->vars, L);
        double probs_prev[ORC_MAX_L], vars_prev[ORC_MAX_L];
        memcpy(probs_prev, s->probs, sizeof probs_prev);
        memcpy(vars_prev, s->vars, sizeof vars_prev);
        double* beta = (double*)malloc(sizeof(double) * (size_t)(M * (Lm > 0 ? Lm : 1)));
        double* gammas = (double*)malloc(sizeof(double) * (size_t)(M * (Lm > 0 ? Lm : 1)));
        double* pin = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
        double v[ORC_MAX_L];
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < M; ++i) {
            double* tb = beta + i * Lm;
            double* tg = gammas + i * Lm;
            for (int j = 1; j < L; ++j) {
                double num = lambda * omegas[j] *
                             exp(-(r1[i] * r1[i]) / 2 * (max_sigma - s->vars[j]) / (s->vars[j] + noise_var) /
                                 (max_sigma + noise_var)) /
                             sqrt(s->vars[j] + noise_var) / sqrt(2 * M_PI);
                double num_gammas = s->gam1 * r1[i] / (1 / s->vars[j] + s->gam1);
                tb[j - 1] = num;
                tg[j - 1] = num_gammas;
            }
            double sum_of_elems = 0.0; /* std::accumulate, sequential */
            for (int j = 0; j < Lm; ++j) sum_of_elems += tb[j];
            for (int j = 0; j < Lm; ++j) tb[j] /= sum_of_elems;
            pin[i] = 1 / (1 + (1 - lambda) / sqrt(2 * M_PI * noise_var) *
                                  exp(-(r1[i] * r1[i]) / 2 * max_sigma / noise_var / (noise_var + max_sigma)) /
                                  sum_of_elems);
        }
        for (int j = 1; j < L; ++j) v[j - 1] = 1.0 / (1.0 / s->vars[j] + s->gam1);
        /* lambda = accumulate(pin) then Allreduce / Mt  (:576-579) */
        double ones_dummy = 0.0;
        (void)ones_dummy;
        double lam_local = 0.0;
        {
            /* blocked deterministic sum of pin */
            double* onesv = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
            for (int64_t i = 0; i < M; ++i) onesv[i] = 1.0;
            lam_local = assoc_sum(pin, onesv, M, SUM_EM);
            free(onesv);
        }
        double lambda_total = allreduce1(pb, lam_local);
        lambda = lambda_total / (double)s->Mt;
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < M; ++i)
            for (int j = 0; j < Lm; ++j) {
                double g = gammas[i * Lm + j];
                gammas[i * Lm + j] = beta[i * Lm + j] * (g * g + v[j]);
            }
        double sum_of_pin = lambda_total;
        double* colb = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
        double* colg = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
        for (int j = 0; j < Lm; ++j) {
            for (int64_t i = 0; i < M; ++i) {
                colb[i] = beta[i * Lm + j];
                colg[i] = gammas[i * Lm + j];
            }
            double res = assoc_sum(colb, pin, M, SUM_EM);
            double res_gammas = assoc_sum(colg, pin, M, SUM_EM);
            double res_gammas_total = allreduce1(pb, res_gammas);
            double res_total = allreduce1(pb, res);
            if (s->learn_vars == 1) s->vars[j + 1] = res_gammas_total / res_total;
            omegas[j + 1] = res_total / sum_of_pin;
            s->probs[j + 1] = lambda * omegas[j + 1];
        }
        s->probs[0] = 1 - lambda;
        free(colb);
        free(colg);
        free(beta);
        free(gammas);
        free(pin);
        double distance_probs = 0, norm_probs = 0, distance_vars = 0, norm_vars = 0;
        for (int j = 0; j < L; ++j) {
            distance_probs += (s->probs[j] - probs_prev[j]) * (s->probs[j] - probs_prev[j]);
            norm_probs += s->probs[j] * s->probs[j];
            distance_vars += (s->vars[j] - vars_prev[j]) * (s->vars[j] - vars_prev[j]);
            norm_vars += s->vars[j] * s->vars[j];
        }
        double dist_probs = sqrt(distance_probs / norm_probs);
        double dist_vars = sqrt(distance_vars / norm_vars);
        if (dist_probs < s->EM_err_thr && dist_vars < s->EM_err_thr) break;
    }
    /* merging close variances (:626-642); abs() on double == fabs */
    for (int j = 0; j < s->L; ++j) {
        for (int k = j + 1; k < s->L; ++k) {
            double denom = s->vars[j] != 0 ? smin(s->vars[j], s->vars[k]) : 1e-7;
            if (fabs(s->vars[j] - s->vars[k]) / denom < s->merge_vars_thr) {
                double sum2probs = s->probs[j] + s->probs[k];
                for (int q = k; q + 1 < s->L; ++q) {
                    s->vars[q] = s->vars[q + 1];
                    s->probs[q] = s->probs[q + 1];
                }
                s->L--;
                s->probs[j] = sum2probs;
                k--;
            }
        }
    }
}

/* err_measures — src/vamp.cpp:760-852 (scalars only; Axest given) */
static void err_measures(orc_vamp* s, const double* xhat, const double* ts, const double* Axest,
                         const double* y, int ind, double* metrics) {
    const orc_problem* pb = s->pb;
    int64_t M = s->M, N = s->N;
    double corr = inner_prod(pb, xhat, ts, M, 1) /
                  sqrt(inner_prod(pb, xhat, xhat, M, 1) * inner_prod(pb, ts, ts, M, 1));
    if (ind == 1)
        metrics[1] = corr;
    else
        metrics[3] = corr;
    double* tempN = (double*)malloc(sizeof(double) * (size_t)N);
    for (int64_t i = 0; i < N; ++i) tempN[i] = -Axest[i] + y[i];
    double l2_pred_err = sqrt(inner_prod(pb, tempN, tempN, N, 0) / inner_prod(pb, y, y, N, 0));
    double R2 = 1 - l2_pred_err * l2_pred_err;
    double corr_y = inner_prod(pb, Axest, y, N, 1) /
                    sqrt(inner_prod(pb, Axest, Axest, N, 1) * inner_prod(pb, y, y, N, 1));
    double corr_y_2 = corr_y * corr_y;
    free(tempN);
    if (ind == 1) {
        metrics[0] = R2;
        metrics[4] = corr_y_2;
    } else {
        metrics[2] = R2;
        metrics[5] = corr_y_2;
    }
}

static void join_path(char* dst, size_t cap, const char* dir, const char* name, const char* suffix) {
    snprintf(dst, cap, "%s/%s%s", dir, name, suffix);
}

/* ------------------------------------------------------------------------- */
/* infere_linear — src/vamp.cpp:110-438 (constructor :18-91)                  */
/* ------------------------------------------------------------------------- */
int orc_vamp_infere_linear(const orc_problem* pb, const orc_params* prm, orc_result* res) {
    int64_t N = pb->N, M = pb->M, Mt = pb->Mt;
    orc_vamp s;
    memset(&s, 0, sizeof s);
    s.pb = pb;
    s.N = N;
    s.M = M;
    s.Mt = Mt;
    s.L = prm->L;
    if (s.L < 1 || s.L > ORC_MAX_L) return -1;
    for (int j = 0; j < s.L; ++j) {
        s.probs[j] = prm->probs[j];
        s.vars[j] = prm->vars[j] * (double)N; /* :87-88 */
    }
    s.gam1 = prm->gam1;
    s.gamw = 1.0 / (1.0 - prm->h2);
    s.gam2 = 0;
    s.CG_max_iter = prm->CG_max_iter;
    s.CG_err_tol = prm->CG_err_tol;
    s.EM_max_iter = prm->EM_max_iter;
    s.EM_err_thr = prm->EM_err_thr;
    s.learn_vars = prm->learn_vars;
    s.merge_vars_thr = prm->merge_vars_thr;
    s.verbosity = prm->verbosity;
    int write = prm->out_dir && prm->out_dir[0] && pb->rank >= 0;
    size_t Mb = sizeof(double) * (size_t)(M > 0 ? M : 1), Nb = sizeof(double) * (size_t)N;

    double sqrtN = sqrt((double)N);
    double* x1_hat = (double*)calloc(1, Mb);
    double* x1_hat_prev = (double*)calloc(1, Mb);
    double* x1_hat_d = (double*)calloc(1, Mb);
    double* x1_scaled = (double*)calloc(1, Mb);
    double* r2 = (double*)calloc(1, Mb);
    double* v = (double*)calloc(1, Mb);
    double* z1 = (double*)calloc(1, Nb);
    double* Ax2 = (double*)calloc(1, Nb);
    double* tmpN = (double*)calloc(1, Nb);
    double* tmpM = (double*)calloc(1, Mb);
    double* ts = (double*)calloc(1, Mb);
    s.r1 = (double*)calloc(1, Mb);
    s.bern_vec = (double*)calloc(1, Mb);
    s.invQ_bern_vec = (double*)calloc(1, Mb);
    s.mu_CG_last = (double*)calloc(1, Mb);
    s.x2_hat = (double*)calloc(1, Mb);
    if (pb->true_signal) memcpy(ts, pb->true_signal, sizeof(double) * (size_t)M);
    /* P1: x1_hat and r1 sized M, then :71-72, :78-79 */
    for (int64_t i = 0; i < M; ++i) {
        double init = pb->x1hat_init ? pb->x1hat_init[i] : 0.0;
        x1_hat[i] = init / sqrt((double)N);
        s.r1[i] = init / sqrt((double)N);
    }
    const double* y = pb->y;

    char p_params[4096], p_metrics[4096], p_prior[4096], pbuf[4096];
    if (write) {
        join_path(p_metrics, sizeof p_metrics, prm->out_dir, prm->out_name, "_metrics.csv");
        join_path(p_params, sizeof p_params, prm->out_dir, prm->out_name, "_params.csv");
        join_path(p_prior, sizeof p_prior, prm->out_dir, prm->out_name, "_prior.csv");
        if (pb->rank == 0) {
            static const char* mh[] = {"iteration",          "R2 denoising",         "x1 correlation denoising",
                                       "R2 LMMSE",           "x2 correlation LMMSE", "z1 correlation denoising",
                                       "z2 correlation LMMSE"};
            static const char* ph[] = {"iteration", "alpha1", "gam1", "alpha2", "gam2", "gamw"};
            char names[2 + 2 * ORC_MAX_L][16];
            const char* prh[2 + 2 * ORC_MAX_L];
            prh[0] = "iteration";
            prh[1] = "number of components";
            int np = 2;
            for (int i = 0; i < s.L; ++i) {
                snprintf(names[np], 16, "prob%d", i);
                prh[np] = names[np];
                ++np;
            }
            for (int i = 0; i < s.L; ++i) {
                snprintf(names[np], 16, "var%d", i);
                prh[np] = names[np];
                ++np;
            }
            orc_csv_header(p_metrics, mh, 7);
            orc_csv_header(p_params, ph, 6);
            orc_csv_header(p_prior, prh, np);
        }
    }

    double metrics[6] = {0, 0, 0, 0, 0, 0}, params[5] = {0, 0, 0, 0, 0};
    double alpha1 = 0, alpha2 = 0, eta1 = 0, eta2 = 0;
    int it;
    int iters_run = 0;
    if (res) res->wall_start = omp_get_wtime();
    for (it = 1; it <= prm->max_iter; ++it) {
        iters_run = it;
        if (it > prm->learn_prior_delay) update_prior(&s); /* :186-187 */
        if (res && res->L_hist) res->L_hist[it - 1] = s.L;

        memcpy(x1_hat_prev, x1_hat, Mb); /* :203 */
        for (int64_t i = 0; i < M; ++i) x1_hat[i] = orc_g1(s.r1[i], s.gam1, s.probs, s.vars, s.L);
        if (it > 1)
            for (int64_t i = 0; i < M; ++i) x1_hat[i] = prm->rho * x1_hat[i] + (1 - prm->rho) * x1_hat_prev[i];
        for (int64_t i = 0; i < M; ++i) x1_hat_d[i] = orc_g1d(s.r1[i], s.gam1, s.probs, s.vars, s.L);
        {
            double* onesv = tmpM;
            for (int64_t i = 0; i < M; ++i) onesv[i] = 1.0;
            double sum_d = assoc_sum(x1_hat_d, onesv, M, SUM_ACC_M);
            alpha1 = allreduce1(pb, sum_d) / (double)Mt; /* :221-223 */
        }
        eta1 = s.gam1 / alpha1;
        ax(&s, x1_hat, z1); /* :232 */

        for (int64_t i = 0; i < M; ++i) x1_scaled[i] = x1_hat[i] / sqrtN;
        if (res && res->x1_hist) memcpy(res->x1_hist + (int64_t)(it - 1) * M, x1_scaled, Mb);
        if (res && res->r1_hist)
            for (int64_t i = 0; i < M; ++i) res->r1_hist[(int64_t)(it - 1) * M + i] = s.r1[i] / sqrtN;
        if (write) {
            char suf[64];
            snprintf(suf, sizeof suf, "_it_%d.bin", it);
            join_path(pbuf, sizeof pbuf, prm->out_dir, prm->out_name, suf);
            orc_store_vec(pbuf, x1_scaled, pb->S, M);
            for (int64_t i = 0; i < M; ++i) tmpM[i] = s.r1[i] / sqrtN;
            snprintf(suf, sizeof suf, "_r1_it_%d.bin", it);
            join_path(pbuf, sizeof pbuf, prm->out_dir, prm->out_name, suf);
            orc_store_vec(pbuf, tmpM, pb->S, M);
        }

        s.gam2 = eta1 - s.gam1; /* :255-256 */
        s.gam2 = smin(smax(s.gam2, 1e-11), 1e11);
        for (int64_t i = 0; i < M; ++i) r2[i] = (eta1 * x1_hat[i] - s.gam1 * s.r1[i]) / s.gam2;

        err_measures(&s, x1_hat, ts, z1, y, 1, metrics); /* :272 */
        params[0] = alpha1;
        params[1] = s.gam1;

        /* LMMSE */
        for (int64_t i = 0; i < M; ++i) /* :295-296 with P2 */
            s.bern_vec[i] = (2 * orc_bern_bit(prm->seed, it, pb->S + i) - 1) / sqrt((double)Mt);
        atx(&s, y, v); /* :303 */
        for (int64_t i = 0; i < M; ++i) v[i] = s.gamw * v[i] + s.gam2 * r2[i];
        if (it == 1)
            memset(tmpM, 0, Mb);
        else
            memcpy(tmpM, s.mu_CG_last, Mb);
        precondCG(&s, v, tmpM, s.gamw, 1, s.x2_hat); /* :308-311 */
        if (res && res->cg_iters) res->cg_iters[it - 1] = s.cg_iters_last;

        /* g2d_onsager :494-501 */
        memset(tmpM, 0, Mb);
        precondCG(&s, s.bern_vec, tmpM, s.gamw, 0, s.invQ_bern_vec);
        if (res && res->ons_iters) res->ons_iters[it - 1] = s.cg_iters_last;
        alpha2 = s.gam2 * inner_prod(pb, s.bern_vec, s.invQ_bern_vec, M, 1);

        eta2 = s.gam2 / alpha2; /* :341-346 */
        double gam1_prev = s.gam1;
        s.gam1 = eta2 - s.gam2;
        s.gam1 = smin(smax(s.gam1, 1e-11), 1e11);
        s.gam1 = prm->rho * s.gam1 + (1 - prm->rho) * gam1_prev;
        for (int64_t i = 0; i < M; ++i) s.r1[i] = (eta2 * s.x2_hat[i] - s.gam2 * r2[i]) / s.gam1;

        /* updateNoisePrec :504-529 */
        ax(&s, s.x2_hat, Ax2);
        for (int64_t i = 0; i < N; ++i) tmpN[i] = Ax2[i] - y[i];
        double temp_norm2 = inner_prod(pb, tmpN, tmpN, N, 0);
        ax(&s, s.invQ_bern_vec, tmpN);
        atx(&s, tmpN, tmpM);
        double trace_corr = inner_prod(pb, s.bern_vec, tmpM, M, 1) * (double)Mt;
        s.gamw = (double)N / (temp_norm2 + trace_corr);

        /* err_measures(2): Ax(x2_hat) recomputed at :826 — same operator, same
         * input; counted as a pass, value identical to Ax2 */
        s.passes++;
        err_measures(&s, s.x2_hat, ts, Ax2, y, 2, metrics);
        params[2] = alpha2;
        params[3] = s.gam2;
        params[4] = s.gamw;
        if (res && res->params) memcpy(res->params + (int64_t)(it - 1) * 5, params, sizeof params);
        if (res && res->metrics) memcpy(res->metrics + (int64_t)(it - 1) * 6, metrics, sizeof metrics);
        if (write && pb->rank == 0) {
            orc_csv_row(p_params, it, params, 5);
            orc_csv_row(p_metrics, it, metrics, 6);
        }
        if (prm->verbosity >= 1 && pb->rank == 0)
            printf("it %d: alpha1 %.6g gam1 %.6g alpha2 %.6g gam2 %.6g gamw %.6g L %d cg %d\n", it, alpha1,
                   s.gam1, alpha2, s.gam2, s.gamw, s.L, s.cg_iters_last);

        /* stopping criteria :409-423 */
        for (int64_t i = 0; i < M; ++i) tmpM[i] = x1_hat_prev[i] - x1_hat[i];
        double NMSE = sqrt(inner_prod(pb, tmpM, tmpM, M, 1) / inner_prod(pb, x1_hat_prev, x1_hat_prev, M, 1));
        if (res && res->it_wall) res->it_wall[it - 1] = omp_get_wtime(); /* bench.py's CPU leg */
        if (it > 1 && NMSE < prm->stop_criteria_thr) break;
    }
    if (res) {
        res->iterations_run = iters_run;
        if (res->x1_final) memcpy(res->x1_final, x1_scaled, sizeof(double) * (size_t)M);
        res->L_final = s.L;
        if (res->probs_final)
            for (int j = 0; j < s.L; ++j) res->probs_final[j] = s.probs[j];
        if (res->vars_final)
            for (int j = 0; j < s.L; ++j) res->vars_final[j] = s.vars[j] / (double)N;
        res->a_passes = s.passes;
    }
    free(x1_hat);
    free(x1_hat_prev);
    free(x1_hat_d);
    free(x1_scaled);
    free(r2);
    free(v);
    free(z1);
    free(Ax2);
    free(tmpN);
    free(tmpM);
    free(ts);
    free(s.r1);
    free(s.bern_vec);
    free(s.invQ_bern_vec);
    free(s.mu_CG_last);
    free(s.x2_hat);
    return 0;
}

/* ------------------------------------------------------------------------- */
/* probit model — src/vamp_probit.cpp                                        */
/* ------------------------------------------------------------------------- */

int orc_csv_create(const char* path) {
    unlink(path);
    int fd = open(path, O_CREAT | O_WRONLY | O_EXCL, 0666);
    if (fd < 0) return -1;
    close(fd);
    return 0;
}

/* P2 for the Gaussian start p1 = simulate(N, {1}, {1}) (src/vamp_probit.cpp:53):
 * one N(0,1)-like dyadic draw per sample, keyed on (seed, i) */
double orc_probit_p1(uint64_t seed, int64_t i) {
    return orc_gauss_dyadic(seed ^ 0x50524F4249545031ULL, 0, i);
}

/* erfcx — src/utilities.cpp:293-363.  The reference embeds N. Juffa's
 * published scaled-complementary-error-function approximation: map
 * a = |x| to q = (a-4)/(a+4), evaluate a degree-23 polynomial in q with fma
 * (Horner), divide by (1+2a) with one Newton correction, reflect for x < 0.
 * Outside [-10, 10] the reference returns +inf (x < -10) and
 * std::numeric_limits<double>::lowest() (x > 10) — reproduced as is. */
static const double ORC_ERFCX_POLY[24] = {
    0x1.edcad78fc8044p-31,  0x1.b1548f14735d1p-30,  -0x1.a1ad2e6c4a7a8p-27, -0x1.1985b48f08574p-26,
    0x1.c6a8093ac4f83p-24,  0x1.31c2b2b44b731p-24,  -0x1.b87373facb29fp-21, 0x1.3fef1358803b7p-22,
    0x1.7eec072bb0be3p-18,  -0x1.78a680a741c4ap-17, -0x1.9951f39295cf4p-16, 0x1.3be1255ce180bp-13,
    -0x1.a1df71176b791p-13, -0x1.8d4aaa0099bc8p-11, 0x1.49c673066c831p-8,   -0x1.0962386ea02b7p-6,
    0x1.3079edf465cc3p-5,   -0x1.0fb06dfedc4ccp-4,  0x1.7fee004e266dfp-4,   -0x1.9ddb23c3e14d2p-4,
    0x1.16ecefcfa4865p-4,   0x1.f7f5df66fc349p-7,   -0x1.1df1ad154a27fp-3,  0x1.dd2c8b74febf6p-3};

double orc_erfcx(double x) {
    if (x < -10.0) return INFINITY;
    if (x > 10.0) return -DBL_MAX;
    const double a = fmax(x, 0.0 - x);
    /* q = (a-4)/(a+4), refined */
    const double inv = 1.0 / (a + 4.0);
    double q = (a - 4.0) * inv;
    const double t0 = fma(q + 1.0, -4.0, a);
    q = fma(inv, fma(q, -a, t0), q);
    double p = ORC_ERFCX_POLY[0];
    for (int k = 1; k < 24; ++k) p = fma(p, q, ORC_ERFCX_POLY[k]);
    /* (1 + p) / (1 + 2a) with a residual correction */
    const double h = (1.0 / (a + 0.5)) * 0.5;
    const double q1 = fma(p, h, h);
    const double res = (p - q1) + fma(q1 + q1, -a, 1.0);
    double r = fma(res, h, q1);
    if (a > DBL_MAX) r = 0.0;
    if (x < 0.0) { /* erfcx(x) = 2 exp(x^2) - erfcx(|x|) */
        const double s = x * x;
        const double lo = fma(x, x, -s);
        const double e = exp(s);
        r = fma(e, lo + lo, e - r) + e;
        if (e > DBL_MAX) r = e;
    }
    return r;
}

/* g1_bin_class / g1d_bin_class — src/vamp_probit.cpp:469-488 with
 * probit_var = 1 and m_cov = 0 (main_meth reads no covariates) */
#define ORC_PROBIT_VAR 1.0
double orc_g1_bin(double p, double tau1, double y) {
    const double c = (p + 0.0) / sqrt(ORC_PROBIT_VAR + 1.0 / tau1);
    const double ratio = 2.0 / sqrt(2 * M_PI) / orc_erfcx(-(2 * y - 1) * c / sqrt(2));
    return p + (2 * y - 1) * ratio / tau1 / sqrt(ORC_PROBIT_VAR + 1.0 / tau1);
}

double orc_g1d_bin(double p, double tau1, double y) {
    const double c = (p + 0.0) / sqrt(ORC_PROBIT_VAR + 1.0 / tau1);
    const double ratio = 2.0 / sqrt(2 * M_PI) / orc_erfcx(-(2 * y - 1) * c / sqrt(2));
    return 1 - ratio / (1 + tau1 * ORC_PROBIT_VAR) * ((2 * y - 1) * c + ratio);
}

/* predict_probit(z, 0.5) + confusion_matrix + accuracy —
 * src/vamp_probit.cpp:619-663, normal_cdf src/utilities.cpp:284-287.
 * out: TP, TN, FP, FN, acc */
static void probit_confusion(const double* z, const double* y, int64_t N, double* out) {
    int64_t TP = 0, TN = 0, FP = 0, FN = 0;
    for (int64_t i = 0; i < N; ++i) {
        const double yh = (0.5 * erfc(-z[i] * M_SQRT1_2) >= 0.5) ? 1.0 : 0.0;
        if (y[i] == 1 && yh == 1)
            TP++;
        else if (y[i] == 0 && yh == 0)
            TN++;
        else if (y[i] == 1 && yh == 0)
            FN++;
        else if (y[i] == 0 && yh == 1)
            FP++;
    }
    out[0] = (double)TP;
    out[1] = (double)TN;
    out[2] = (double)FP;
    out[3] = (double)FN;
    out[4] = (double)(TP + TN) / (double)(TP + TN + FP + FN);
}

/* infere_bin_class — src/vamp_probit.cpp:19-467 */
int orc_vamp_infere_probit(const orc_problem* pb, const orc_params* prm, orc_result* res) {
    int64_t N = pb->N, M = pb->M, Mt = pb->Mt;
    orc_vamp s;
    memset(&s, 0, sizeof s);
    s.pb = pb;
    s.N = N;
    s.M = M;
    s.Mt = Mt;
    s.L = prm->L;
    if (s.L < 1 || s.L > ORC_MAX_L) return -1;
    for (int j = 0; j < s.L; ++j) {
        s.probs[j] = prm->probs[j];
        s.vars[j] = prm->vars[j] * (double)N; /* src/vamp.cpp:87-88 */
    }
    s.gam1 = prm->gam1;
    s.gam2 = 0;
    s.CG_max_iter = prm->CG_max_iter;
    s.CG_err_tol = prm->CG_err_tol;
    s.EM_max_iter = prm->EM_max_iter;
    s.EM_err_thr = prm->EM_err_thr;
    s.learn_vars = prm->learn_vars;
    s.merge_vars_thr = prm->merge_vars_thr;
    s.verbosity = prm->verbosity;
    const double gmin = 1e-11, gmax = 1e11; /* src/vamp.hpp:33-34 */
    int write = prm->out_dir && prm->out_dir[0];
    size_t Mb = sizeof(double) * (size_t)(M > 0 ? M : 1), Nb = sizeof(double) * (size_t)N;
    const double sqrtN = sqrt((double)N);

    double* x1_hat = (double*)calloc(1, Mb);
    double* x1_hat_prev = (double*)calloc(1, Mb);
    double* x1_scaled = (double*)calloc(1, Mb);
    double* x2_s = (double*)calloc(1, Mb);
    double* r2 = (double*)calloc(1, Mb);
    double* v = (double*)calloc(1, Mb);
    double* tmpM = (double*)calloc(1, Mb);
    double* tss = (double*)calloc(1, Mb);
    double* p1 = (double*)calloc(1, Nb);
    double* p2 = (double*)calloc(1, Nb);
    double* z1_hat = (double*)calloc(1, Nb);
    double* z2_hat = (double*)calloc(1, Nb);
    double* zacc = (double*)calloc(1, Nb);
    s.r1 = (double*)calloc(1, Mb);
    s.bern_vec = (double*)calloc(1, Mb);
    s.invQ_bern_vec = (double*)calloc(1, Mb);
    s.mu_CG_last = (double*)calloc(1, Mb);
    s.x2_hat = (double*)calloc(1, Mb);
    /* constructor: x1_hat = x1hat_init / sqrt(N) (P1, src/vamp.cpp:71-72) */
    for (int64_t i = 0; i < M; ++i) x1_hat[i] = (pb->x1hat_init ? pb->x1hat_init[i] : 0.0) / sqrtN;
    /* :41-44 true_signal_scaled; true_g = Ax(.) (:46) is never read again:
     * counted as a pass, not computed */
    for (int64_t i = 0; i < M; ++i) tss[i] = (pb->true_signal ? pb->true_signal[i] : 0.0) * sqrtN;
    s.passes++;
    for (int64_t i = 0; i < N; ++i) p1[i] = orc_probit_p1(prm->seed, i); /* :53 (P2) */
    double tau1 = s.gam1, tau2 = 0;                                        /* :35 */
    double alpha1 = 0, alpha2 = 0, eta1 = 0, beta1 = 0, beta2 = 0;
    const double* y = pb->y;

    char p_params[4096], p_metrics[4096], p_prior[4096], pbuf[4096];
    if (write) {
        join_path(p_metrics, sizeof p_metrics, prm->out_dir, prm->out_name, "_metrics.csv");
        join_path(p_params, sizeof p_params, prm->out_dir, prm->out_name, "_params.csv");
        join_path(p_prior, sizeof p_prior, prm->out_dir, prm->out_name, "_prior.csv");
        if (pb->rank == 0) {
            orc_csv_create(p_metrics);
            orc_csv_create(p_params);
            orc_csv_create(p_prior);
        }
    }
    double metrics[12] = {0}, params[8] = {0}, prior_row[1 + 2 * ORC_MAX_L];
    int iters_run = 0;
    if (res) res->wall_start = omp_get_wtime();
    for (int it = 1; it <= prm->max_iter; ++it) {
        iters_run = it;
        /* ---- denoising x (:104-198) ---- */
        memcpy(x1_hat_prev, x1_hat, Mb);
        const double alpha1_prev = alpha1;
        for (int64_t i = 0; i < M; ++i) x1_hat[i] = orc_g1(s.r1[i], s.gam1, s.probs, s.vars, s.L);
        for (int64_t i = 0; i < M; ++i) tmpM[i] = orc_g1d(s.r1[i], s.gam1, s.probs, s.vars, s.L);
        {
            double* onesv = v;
            for (int64_t i = 0; i < M; ++i) onesv[i] = 1.0;
            alpha1 = allreduce1(pb, assoc_sum(tmpM, onesv, M, SUM_ACC_M)) / (double)Mt; /* :120-129 */
        }
        eta1 = s.gam1 / alpha1;          /* :130 */
        if (it > 1) update_prior(&s);    /* :139 (after g1 / g1d) */
        if (res && res->L_hist) res->L_hist[it - 1] = s.L;
        if (it > 1) {                    /* :160-165 */
            for (int64_t i = 0; i < M; ++i) x1_hat[i] = prm->rho * x1_hat[i] + (1 - prm->rho) * x1_hat_prev[i];
            alpha1 = prm->rho * alpha1 + (1 - prm->rho) * alpha1_prev;
        }
        for (int64_t i = 0; i < M; ++i) x1_scaled[i] = x1_hat[i] / sqrtN; /* :168-172 */
        if (res && res->x1_hist) memcpy(res->x1_hist + (int64_t)(it - 1) * M, x1_scaled, Mb);
        if (res && res->r1_hist)
            for (int64_t i = 0; i < M; ++i) res->r1_hist[(int64_t)(it - 1) * M + i] = s.r1[i] / sqrtN;
        if (write) {
            char suf[64];
            snprintf(suf, sizeof suf, "_it_%d.bin", it);
            join_path(pbuf, sizeof pbuf, prm->out_dir, prm->out_name, suf);
            orc_store_vec(pbuf, x1_scaled, pb->S, M);
            for (int64_t i = 0; i < M; ++i) tmpM[i] = s.r1[i] / sqrtN;
            snprintf(suf, sizeof suf, "_r1_it_%d.bin", it);
            join_path(pbuf, sizeof pbuf, prm->out_dir, prm->out_name, suf);
            orc_store_vec(pbuf, tmpM, pb->S, M);
        }
        const double x1_corr = inner_prod(pb, x1_hat, tss, M, 1) /
                               sqrt(inner_prod(pb, x1_hat, x1_hat, M, 1) * inner_prod(pb, tss, tss, M, 1)); /* :189 */
        s.gam2 = smin(smax(eta1 - s.gam1, gmin), gmax); /* :194 */
        for (int64_t i = 0; i < M; ++i) r2[i] = (eta1 * x1_hat[i] - s.gam1 * s.r1[i]) / s.gam2;

        /* ---- denoising z (:202-253) ---- */
        for (int64_t i = 0; i < N; ++i) z1_hat[i] = orc_g1_bin(p1[i], tau1, y[i]);
        {
            for (int64_t i = 0; i < N; ++i) zacc[i] = orc_g1d_bin(p1[i], tau1, y[i]);
            double* onesv = p2;
            for (int64_t i = 0; i < N; ++i) onesv[i] = 1.0;
            beta1 = assoc_sum(zacc, onesv, N, SUM_ACC_N); /* local: y and p1 are replicated */
        }
        if (beta1 >= N) beta1 = N - 1.0;
        beta1 /= N;
        for (int64_t i = 0; i < N; ++i) p2[i] = (z1_hat[i] - beta1 * p1[i]) / (1 - beta1);
        tau2 = tau1 * (1 - beta1) / beta1;
        params[0] = alpha1;
        params[1] = beta1;
        params[2] = s.gam1;
        params[3] = tau1;
        ax(&s, x1_scaled, zacc); /* :271-282 */
        probit_confusion(zacc, y, N, metrics);
        metrics[5] = x1_corr;

        /* ---- LMMSE (:297-385) ---- */
        for (int64_t i = 0; i < M; ++i)
            s.bern_vec[i] = (2 * orc_bern_bit(prm->seed, it, pb->S + i) - 1) / sqrt((double)Mt);
        atx(&s, p2, v); /* :300-303 */
        for (int64_t i = 0; i < M; ++i) v[i] = tau2 * v[i] + s.gam2 * r2[i];
        memset(tmpM, 0, Mb);
        precondCG(&s, v, tmpM, tau2, 1, s.x2_hat); /* :307 (zero start) */
        if (res && res->cg_iters) res->cg_iters[it - 1] = s.cg_iters_last;
        memset(tmpM, 0, Mb);
        precondCG(&s, s.bern_vec, tmpM, tau2, 0, s.invQ_bern_vec); /* g2d_onsager(gam2, tau2) :311 */
        if (res && res->ons_iters) res->ons_iters[it - 1] = s.cg_iters_last;
        alpha2 = s.gam2 * inner_prod(pb, s.bern_vec, s.invQ_bern_vec, M, 1);
        for (int64_t i = 0; i < M; ++i) x2_s[i] = s.x2_hat[i] / sqrt((double)N); /* :318-320 */
        const double x2_corr = inner_prod(pb, s.x2_hat, tss, M, 1) /
                               sqrt(inner_prod(pb, s.x2_hat, s.x2_hat, M, 1) * inner_prod(pb, tss, tss, M, 1));
        for (int64_t i = 0; i < M; ++i) s.r1[i] = (s.x2_hat[i] - alpha2 * r2[i]) / (1 - alpha2); /* :337-338 */
        s.gam1 = smin(smax(s.gam2 * (1 - alpha2) / alpha2, gmin), gmax);                    /* :345-346 */
        ax(&s, s.x2_hat, z2_hat);                                                                /* :352 */
        beta2 = (double)Mt / N * (1 - alpha2);                                                   /* :354 */
        for (int64_t i = 0; i < N; ++i) p1[i] = (z2_hat[i] - beta2 * p2[i]) / (1 - beta2);      /* :367-368 */
        tau1 = smin(smax(tau2 * (1 - beta2) / beta2, gmin), gmax);                               /* :375-376 */
        params[4] = alpha2;
        params[5] = beta2;
        params[6] = s.gam2;
        params[7] = tau2;
        ax(&s, x2_s, zacc); /* :403-415 */
        probit_confusion(zacc, y, N, metrics + 6);
        metrics[11] = x2_corr;
        /* prior row (:423-428): L, probs, vars (still multiplied by N) */
        int np = 0;
        prior_row[np++] = (double)s.L;
        for (int j = 0; j < s.L; ++j) prior_row[np++] = s.probs[j];
        for (int j = 0; j < s.L; ++j) prior_row[np++] = s.vars[j];
        if (res && res->params) memcpy(res->params + (int64_t)(it - 1) * 8, params, sizeof params);
        if (res && res->metrics) memcpy(res->metrics + (int64_t)(it - 1) * 12, metrics, sizeof metrics);
        if (res && res->prior_hist) {
            double* dst = res->prior_hist + (int64_t)(it - 1) * (1 + 2 * ORC_MAX_L);
            memset(dst, 0, sizeof(double) * (1 + 2 * ORC_MAX_L));
            memcpy(dst, prior_row, sizeof(double) * (size_t)np);
        }
        if (write && pb->rank == 0) { /* :430-435 */
            orc_csv_row(p_params, it, params, 8);
            orc_csv_row(p_metrics, it, metrics, 12);
            orc_csv_row(p_prior, it, prior_row, np);
        }
        if (prm->verbosity >= 1 && pb->rank == 0)
            printf("it %d: alpha1 %.6g beta1 %.6g gam1 %.6g tau1 %.6g alpha2 %.6g beta2 %.6g L %d\n", it, alpha1,
                   beta1, s.gam1, tau1, alpha2, beta2, s.L);
        /* stopping criteria (:444-458) */
        for (int64_t i = 0; i < M; ++i) tmpM[i] = x1_hat_prev[i] - x1_hat[i];
        double NMSE = sqrt(inner_prod(pb, tmpM, tmpM, M, 1) / inner_prod(pb, x1_hat_prev, x1_hat_prev, M, 1));
        if (res && res->it_wall) res->it_wall[it - 1] = omp_get_wtime(); /* bench.py's CPU leg */
        if (it > 1 && NMSE < prm->stop_criteria_thr) break;
    }
    if (res) {
        res->iterations_run = iters_run;
        if (res->x1_final) memcpy(res->x1_final, x1_hat, sizeof(double) * (size_t)M); /* :465 */
        res->L_final = s.L;
        if (res->probs_final)
            for (int j = 0; j < s.L; ++j) res->probs_final[j] = s.probs[j];
        if (res->vars_final)
            for (int j = 0; j < s.L; ++j) res->vars_final[j] = s.vars[j] / (double)N;
        res->a_passes = s.passes;
    }
    free(x1_hat);
    free(x1_hat_prev);
    free(x1_scaled);
    free(x2_s);
    free(r2);
    free(v);
    free(tmpM);
    free(tss);
    free(p1);
    free(p2);
    free(z1_hat);
    free(z2_hat);
    free(zacc);
    free(s.r1);
    free(s.bern_vec);
    free(s.invQ_bern_vec);
    free(s.mu_CG_last);
    free(s.x2_hat);
    return 0;
}

/* ------------------------------------------------------------------------- */
/* association tests — src/main_meth.cpp:206-264, src/data.cpp:385-417,      */
/* src/utilities.cpp:269-282                                                 */
/* ------------------------------------------------------------------------- */

/* ln B(a, 1/2).  For a >= 30: ln sqrt(pi) - [lnG(a+1/2) - lnG(a)] with the
 * asymptotic series of the lgamma difference (error < 2e-16 there); below,
 * lgamma directly (values small, absolute error ~1e-15). */
double orc_lnbeta_half(double a) {
    if (a >= 30.0) {
        const double i1 = 1.0 / a, i2 = i1 * i1;
        const double d = 0.5 * log(a) - i1 * (1.0 / 8.0) + i1 * i2 * (1.0 / 192.0) - i1 * i2 * i2 * (1.0 / 640.0) +
                         i1 * i2 * i2 * i2 * (17.0 / 14336.0);
        return 0.57236494292470008707 - d; /* ln sqrt(pi) */
    }
    return lgamma(a) + lgamma(0.5) - lgamma(a + 0.5);
}

/* continued fraction of the regularized incomplete beta I_x(a, b)
 * (modified Lentz, the classic even/odd term pair per step) */
static double ibeta_cf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 4e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 20000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return h;
}

/* P(T > t) for Student's t with df degrees of freedom, t >= 0:
 * 0.5 * I_x(df/2, 1/2), x = df / (df + t^2).  Stands for
 * boost::math::cdf(complement(students_t(df), t)) (Boost is absent here:
 * pinned against scipy.stats.t.sf in tests/test_oracle_assoc.py). */
double orc_t_sf(double t, double df) {
    if (isnan(t) || isnan(df)) return NAN;
    if (t <= 0.0) return t == 0.0 ? 0.5 : 1.0 - orc_t_sf(-t, df);
    const double a = 0.5 * df, b = 0.5, tt = t * t;
    /* t = inf, or a finite t whose square overflows: x = df / (df + inf) = 0
     * and I_0 = 0, which is what Boost returns (below, tt / (df + tt) would
     * be inf / inf).  Every t with a finite square takes the path it took. */
    if (!isfinite(tt)) return 0.0;
    const double lx = -log1p(tt / df);     /* ln x */
    const double l1x = log(tt / (df + tt)); /* ln (1 - x) */
    const double x = df / (df + tt);
    const double front = exp(a * lx + b * l1x - orc_lnbeta_half(a));
    /* the direct fraction in x for the tail (t >= 3), the fraction of the
     * complement in 1 - x below: either is accurate to ~2e-12 relative
     * (worst near t = 3 at large df; mpmath check in DESIGN.md §3) */
    if (t >= 3.0 && x < (a + 1.0) / (a + b + 2.0)) return 0.5 * (front * ibeta_cf(a, b, x) / a);
    return 0.5 * (1.0 - front * ibeta_cf(b, a, tt / (df + tt)) / b);
}

/* linear_reg1d_pvals — src/utilities.cpp:269-282 */
double orc_reg1d_pval(double sumx, double sumsqx, double sumxy, double sumy, double sumsqy, int n) {
    const double s2y = (sumsqy - sumy * sumy / n) / (n - 1);
    const double s2x = (sumsqx - sumx * sumx / n) / (n - 1);
    const double sxy = (sumxy - sumx * sumy / n) / (n - 1);
    const double rxy = sxy / sqrt(s2x * s2y);
    const double t = rxy * sqrt((n - 2) / (1 - rxy * rxy));
    return 2.0 * orc_t_sf(t > 0 ? t : (0 - t), (double)(n - 2));
}

/* --pval-method loo — src/main_meth.cpp:245-264 + data::pvals_loo
 * src/data.cpp:385-417.  est = the --estimate-file slice as stored
 * (x1_hat / sqrt(N)); X is the RAW marker data (the leave-one-out add-back
 * uses meth_data, not the standardised column). */
void orc_assoc_loo(const orc_problem* pb, const double* est, double* pvals, double* stats) {
    const int64_t N = pb->N, M = pb->M, ld = pb->ld;
    double* x1 = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
    double* z1 = (double*)malloc(sizeof(double) * (size_t)N);
    double* ymod = (double*)malloc(sizeof(double) * (size_t)N);
    for (int64_t i = 0; i < M; ++i) x1[i] = est[i] * sqrt((double)N); /* :254-255 */
    orc_ax(pb->X, N, ld, M, pb->mave, pb->msig, x1, z1, pb->allreduce, pb->user); /* :257 */
    for (int64_t i = 0; i < N; ++i) ymod[i] = pb->y[i] - z1[i];                    /* data.cpp:390-391 */
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t j = 0; j < M; ++j) {
        const double* meth = pb->X + j * ld;
        double sumx = 0.0, sumsqx = 0.0, sumxy = 0.0, sumy = 0.0, sumsqy = 0.0;
        for (int64_t i = 0; i < N; ++i) {
            const double ym = ymod[i] + meth[i] / sqrt((double)N) * x1[j]; /* :403-404 */
            sumx += meth[i];
            sumsqx += meth[i] * meth[i];
            sumxy += meth[i] * ym;
            sumy += ym;
            sumsqy += ym * ym;
        }
        if (stats) {
            double* s = stats + 5 * j;
            s[0] = sumx;
            s[1] = sumsqx;
            s[2] = sumxy;
            s[3] = sumy;
            s[4] = sumsqy;
        }
        pvals[j] = orc_reg1d_pval(sumx, sumsqx, sumxy, sumy, sumsqy, (int)N);
    }
    free(x1);
    free(z1);
    free(ymod);
}

/* --pval-method se — src/main_meth.cpp:218-242: P(N(r1_j, 1/(gam1 N)) <= 0),
 * flipped for r1_j <= 0.  boost::math::cdf(normal(m, s), x) is
 * erfc(-((x - m) / s) / sqrt(2)) / 2. */
void orc_assoc_se(const double* r1, int64_t M, double gam1, int64_t N, double* pvals) {
    const double sd = sqrt(1.0 / (gam1 * (double)N));
    for (int64_t j = 0; j < M; ++j) {
        const double diff = (0.0 - r1[j]) / sd;
        double p = erfc(-diff / M_SQRT2) / 2;
        if (r1[j] <= 0.0) p = 1 - p;
        pvals[j] = p;
    }
}

/* ------------------------------------------------------------------------- */
/* --run-mode test — src/main_meth.cpp:112-205, calc_stdev                   */
/* src/utilities.cpp:183-205                                                  */
/* ------------------------------------------------------------------------- */
/* one estimate file's row of _test.csv: est = this shard's slice as stored
 * (x1_hat/sqrt(N)); pb describes the TEST data set (N = N_test).
 * out[0] = R2 test, out[1] = squared correlation of A.x with y. */
void orc_test_metrics(const orc_problem* pb, const double* est, double* out) {
    const int64_t N = pb->N, M = pb->M;
    double* x = (double*)malloc(sizeof(double) * (size_t)(M > 0 ? M : 1));
    double* z = (double*)malloc(sizeof(double) * (size_t)N);
    double* d = (double*)malloc(sizeof(double) * (size_t)N);
    for (int64_t i = 0; i < M; ++i) x[i] = est[i] * sqrt((double)N); /* :172-174 */
    orc_ax(pb->X, N, pb->ld, M, pb->mave, pb->msig, x, z, pb->allreduce, pb->user); /* :177 */
    const double* y = pb->y;
    for (int64_t i = 0; i < N; ++i) d[i] = y[i] - z[i];
    const double l2 = orc_dot(d, d, N); /* :180-183 */
    /* calc_stdev(y_test) (sync = 0) */
    for (int64_t i = 0; i < N; ++i) d[i] = 1.0;
    const double sum = orc_dot(y, d, N), sq_sum = orc_dot(y, y, N);
    const double mean = sum / (double)N;
    const double stdev = sqrt((sq_sum - (double)N * mean * mean) / (double)(N - 1));
    out[0] = 1 - l2 / (stdev * stdev * (double)N); /* :187 */
    /* inner_prod(., 1) multiplies each replicated sum by the rank count, which
     * cancels in the ratio: computed unsynced */
    const double corr = orc_dot(z, y, N) / sqrt(orc_dot(z, z, N) * orc_dot(y, y, N)); /* :190 */
    out[1] = corr * corr;
    free(x);
    free(z);
    free(d);
}

/* updatePrior alone (src/vamp.cpp:531-643), for tests: r1 (M local values),
 * gam1, the mixture (*L, probs, vars multiplied by N) updated in place */
int orc_update_prior(const orc_problem* pb, const double* r1, double gam1, const orc_params* prm, int* L,
                     double* probs, double* vars) {
    orc_vamp s;
    memset(&s, 0, sizeof s);
    s.pb = pb;
    s.N = pb->N;
    s.M = pb->M;
    s.Mt = pb->Mt;
    s.L = *L;
    if (s.L < 1 || s.L > ORC_MAX_L) return -1;
    for (int j = 0; j < s.L; ++j) {
        s.probs[j] = probs[j];
        s.vars[j] = vars[j];
    }
    s.gam1 = gam1;
    s.r1 = (double*)r1;
    s.EM_max_iter = prm->EM_max_iter;
    s.EM_err_thr = prm->EM_err_thr;
    s.learn_vars = prm->learn_vars;
    s.merge_vars_thr = prm->merge_vars_thr;
    update_prior(&s);
    *L = s.L;
    for (int j = 0; j < s.L; ++j) {
        probs[j] = s.probs[j];
        vars[j] = s.vars[j];
    }
    return 0;
}
