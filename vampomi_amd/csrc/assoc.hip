// assoc.hip — gfx950 kernels of the association tests: the marker pass of the
// leave-one-out test for one phenotype (loo_kernel, loo_wg_kernel) and for
// several (loo_multi_kernel), the two passes of the leave-one-chromosome-out
// test (ax_seg_kernel, loco_kernel), the Student-t tail and the p-values.
// Nothing here is launched by a VAMP iteration; assoc.cpp holds the entry
// points, and the association section of kernels.h is the interface between
// the two.
#include "kernels.h"
#include "kdev.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace vk {

// ---------------------------------------------------------------------------
// association tests: data::pvals_loo (src/data.cpp:385-417) and the SE
// p-values (src/main_meth.cpp:218-242)
// ---------------------------------------------------------------------------
// One pass over the RAW shard: a wave owns G markers, lanes stride the
// samples (16-B nontemporal loads, 1 KiB per wave per load), every ymod
// value serves G markers.  Per element exactly the reference's
// ym = ymod + (X / sqrt(N)) * x1_j, then the five sums of linear_reg1d_pvals.
// Pad rows are zero in X and ymod and add exact zeros.
//
// X / sqrt(N) is the correctly rounded quotient either way: FASTDIV computes
// q0 = X*r (r = RN(1/sqrt(N))), the exact residual e = fma(-q0, sqrt(N), X)
// and q = fma(e, r, q0), which is RN(X/sqrt(N)) whenever r is the rounded
// reciprocal and q0 is within one ulp (Markstein's theorem; checked
// bit for bit against IEEE division in tests/test_hostio.py and on the
// device in tests/test_gpu_assoc.py) — 3 instructions instead of the ~10 of
// the IEEE division sequence, which made the pass ALU-bound.  Only the sign
// of a zero quotient can differ, which no sum can see.  Every lane adds its
// samples in increasing order whatever G / UJ are, so all variants give
// bitwise identical sums.
// (the body of loo_kernel, loo_kernel_f32 and loo_kernel_u16: XE is X's element type)
template <int G, int UJ, bool FASTDIV, class XE>
__device__ __forceinline__ void loo_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                         const double* __restrict__ ymod, const double* __restrict__ x1,
                                         double sqrtN, double* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * G;
    const double rinv = 1.0 / sqrtN;
    double acc[G][5];
    double xj[G];
    const XE* col[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t m = (m0 + g < M) ? m0 + g : M - 1;  // clamp: in-bounds, discarded
        xj[g] = x1[m];
        col[g] = X + m * ld;
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[g][q] = 0.0;
    }
    auto add = [&](int g, double m, double y) {
        double q;
        if (FASTDIV) {
            const double q0 = m * rinv;
            q = __builtin_fma(__builtin_fma(-q0, sqrtN, m), rinv, q0);
        } else {
            q = m / sqrtN;
        }
        const double ym = y + q * xj[g];
        acc[g][0] += m;
        acc[g][1] += m * m;
        acc[g][2] += m * ym;
        acc[g][3] += ym;
        acc[g][4] += ym * ym;
    };
    int64_t j = 2 * lane;
    for (; j + 128 * (UJ - 1) < N; j += 128 * UJ) {
        v2d yy[UJ];
        xpair_t<XE> xx[UJ][G];
#pragma unroll
        for (int t = 0; t < UJ; ++t)
#pragma unroll
            for (int g = 0; g < G; ++g) xx[t][g] = ldx<true>(col[g] + j + 128 * t);
#pragma unroll
        for (int t = 0; t < UJ; ++t) yy[t] = ld2(ymod + j + 128 * t);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int t = 0; t < UJ; ++t) {
                add(g, widen(xx[t][g]).x, yy[t].x);
                add(g, widen(xx[t][g]).y, yy[t].y);
            }
    }
    for (; j < N; j += 128) {
        xpair_t<XE> xx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) xx[g] = ldx<true>(col[g] + j);
        const v2d yy = ld2(ymod + j);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            add(g, widen(xx[g]).x, yy.x);
            add(g, widen(xx[g]).y, yy.y);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double s = wave_sum(acc[g][q]);
            if (lane == 0 && m0 + g < M) stats[5 * (m0 + g) + q] = s;
        }
}

template <int G, int UJ, bool FASTDIV>
__global__ __launch_bounds__(kBlock) void loo_kernel(const double* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                                     const double* __restrict__ ymod, const double* __restrict__ x1,
                                                     double sqrtN, double* __restrict__ stats) {
    loo_body<G, UJ, FASTDIV>(X, ld, N, M, ymod, x1, sqrtN, stats);
}

template <int G, int UJ, bool FASTDIV>
__global__ __launch_bounds__(kBlock) void loo_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                         int64_t M, const double* __restrict__ ymod,
                                                         const double* __restrict__ x1, double sqrtN,
                                                         double* __restrict__ stats) {
    loo_body<G, UJ, FASTDIV>(X, ld, N, M, ymod, x1, sqrtN, stats);
}

template <int G, int UJ, bool FASTDIV>
__global__ __launch_bounds__(kBlock) void loo_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                         int64_t M, const double* __restrict__ ymod,
                                                         const double* __restrict__ x1, double sqrtN,
                                                         double* __restrict__ stats) {
    loo_body<G, UJ, FASTDIV>(X, ld, N, M, ymod, x1, sqrtN, stats);
}

// The same sums with W waves of a workgroup sharing its G markers, for KT
// phenotypes from ONE pass over the shard: wave w, lane l
// takes rows 2l + 128 (w + W t), so one load round of the workgroup reads
// W KiB contiguous of each column (the wave-per-marker form above reads 1 KiB
// per wave from columns all over the shard); the W wave sums meet in LDS and
// are added in wave order.  The x-only work of an element (the fma-corrected
// quotient q of loo_kernel, sum X, sum X^2) is done once and the three
// phenotype sums KT times; rows, per-lane order, wave_sum and the wave-order
// LDS sum do not depend on KT, G or UJ, and the per-phenotype expressions are
// the same for every t, so block t of stats is bit for bit what KT = 1 gives
// for (ymod_t, x1_t) at the same W.
// KT = 1 is the body of loo_wg_kernel, loo_wg_kernel_f32 and loo_wg_kernel_u16
// (ldy = Mx = 0: one vector each, five accumulators per marker in the order of
// stats); KT = 2, 3, 4 that of the loo_multi kernels, at W = 8.
// acc[g][0..1]: sum X, sum X^2 (written into every block); acc[g][2 + 3t ..]:
// sum X*ym_t, sum ym_t, sum ym_t^2.
// ymod: KT vectors of stride ldy; x1: KT vectors of stride Mx; stats: KT
// blocks of 5*M.
template <int KT, int G, int UJ, int W, class XE>
__device__ __forceinline__ void loo_multi_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                               const double* __restrict__ ymod, int64_t ldy,
                                               const double* __restrict__ x1, int64_t Mx, double sqrtN,
                                               double* __restrict__ stats) {
    constexpr int NA = 2 + 3 * KT;  // accumulators per marker
    __shared__ double part[W][NA * G];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * G;
    const double rinv = 1.0 / sqrtN;
    double acc[G][NA];
    double xj[G][KT];
    const XE* col[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t m = (m0 + g < M) ? m0 + g : M - 1;  // clamp: in-bounds, discarded
#pragma unroll
        for (int t = 0; t < KT; ++t) xj[g][t] = x1[(int64_t)t * Mx + m];
        col[g] = X + m * ld;
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[g][q] = 0.0;
    }
    auto add = [&](int g, double m, const double (&y)[KT]) {
        const double q0 = m * rinv;
        const double q = __builtin_fma(__builtin_fma(-q0, sqrtN, m), rinv, q0);
        acc[g][0] += m;
        acc[g][1] += m * m;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const double ym = y[t] + q * xj[g][t];
            acc[g][2 + 3 * t] += m * ym;
            acc[g][3 + 3 * t] += ym;
            acc[g][4 + 3 * t] += ym * ym;
        }
    };
    constexpr int64_t RS = 128 * W;  // rows per load round of the workgroup
    int64_t j = 2 * lane + 128 * wave;
    for (; j + RS * (UJ - 1) < N; j += RS * UJ) {
        xpair_t<XE> xx[UJ][G];
#pragma unroll
        for (int u = 0; u < UJ; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) xx[u][g] = ldx<true>(col[g] + j + RS * u);
        double ya[UJ][KT], yb[UJ][KT];
        auto ldy_round = [&](int u) {
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const v2d yy = ld2(ymod + (int64_t)t * ldy + j + RS * u);
                ya[u][t] = yy.x;
                yb[u][t] = yy.y;
            }
        };
        // Where the ymod loads stand and which loop is the outer one decide
        // registers only: an accumulator gets its addends in increasing row
        // order either way.  One phenotype: every ymod load of the round before
        // the arithmetic, markers outermost; several: a load round's ymod
        // values loaded when that round is summed (all of them up front cost
        // loo_multi_kernel<2, 4, 2, 8> and <3, 4, 1, 8> a wave per SIMD, the
        // other way round loo_wg_kernel<4, 2, 2> one; profiles/assoc_refactor.md)
        if constexpr (KT == 1) {
#pragma unroll
            for (int u = 0; u < UJ; ++u) ldy_round(u);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int u = 0; u < UJ; ++u) {
                    add(g, widen(xx[u][g]).x, ya[u]);
                    add(g, widen(xx[u][g]).y, yb[u]);
                }
        } else {
#pragma unroll
            for (int u = 0; u < UJ; ++u) {
                ldy_round(u);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    add(g, widen(xx[u][g]).x, ya[u]);
                    add(g, widen(xx[u][g]).y, yb[u]);
                }
            }
        }
    }
    for (; j < N; j += RS) {  // (N even or the pad row: ld-padded columns, zero pads)
        xpair_t<XE> xx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) xx[g] = ldx<true>(col[g] + j);
        double ya[KT], yb[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const v2d yy = ld2(ymod + (int64_t)t * ldy + j);
            ya[t] = yy.x;
            yb[t] = yy.y;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            add(g, widen(xx[g]).x, ya);
            add(g, widen(xx[g]).y, yb);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const double s = wave_sum(acc[g][q]);
            if (lane == 0) part[wave][NA * g + q] = s;
        }
    __syncthreads();
    // thread i < 5*KT*G: phenotype t, marker g, sum q of block t
    const int i = (int)threadIdx.x;
    if (i < 5 * KT * G) {
        const int t = i / (5 * G), g = (i % (5 * G)) / 5, q = i % 5;
        if (m0 + g < M) {
            const int src = NA * g + (q < 2 ? q : q + 3 * t);
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) s += part[w][src];
            stats[(int64_t)t * 5 * M + 5 * (m0 + g) + q] = s;
        }
    }
}

template <int KT, int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_multi_kernel(const double* __restrict__ X, int64_t ld, int64_t N,
                                                           int64_t M, const double* __restrict__ ymod, int64_t ldy,
                                                           const double* __restrict__ x1, int64_t Mx, double sqrtN,
                                                           double* __restrict__ stats) {
    loo_multi_body<KT, G, UJ, W>(X, ld, N, M, ymod, ldy, x1, Mx, sqrtN, stats);
}

template <int KT, int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_multi_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                               int64_t M, const double* __restrict__ ymod,
                                                               int64_t ldy, const double* __restrict__ x1, int64_t Mx,
                                                               double sqrtN, double* __restrict__ stats) {
    loo_multi_body<KT, G, UJ, W>(X, ld, N, M, ymod, ldy, x1, Mx, sqrtN, stats);
}

template <int KT, int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_multi_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                               int64_t M, const double* __restrict__ ymod,
                                                               int64_t ldy, const double* __restrict__ x1, int64_t Mx,
                                                               double sqrtN, double* __restrict__ stats) {
    loo_multi_body<KT, G, UJ, W>(X, ld, N, M, ymod, ldy, x1, Mx, sqrtN, stats);
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_wg_kernel(const double* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                                        const double* __restrict__ ymod, const double* __restrict__ x1,
                                                        double sqrtN, double* __restrict__ stats) {
    loo_multi_body<1, G, UJ, W>(X, ld, N, M, ymod, 0, x1, 0, sqrtN, stats);
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_wg_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                            int64_t M, const double* __restrict__ ymod,
                                                            const double* __restrict__ x1, double sqrtN,
                                                            double* __restrict__ stats) {
    loo_multi_body<1, G, UJ, W>(X, ld, N, M, ymod, 0, x1, 0, sqrtN, stats);
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loo_wg_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                            int64_t M, const double* __restrict__ ymod,
                                                            const double* __restrict__ x1, double sqrtN,
                                                            double* __restrict__ stats) {
    loo_multi_body<1, G, UJ, W>(X, ld, N, M, ymod, 0, x1, 0, sqrtN, stats);
}

struct LooVariant { int G, UJ; bool FD; int W = 0; };  // W > 0: loo_wg_kernel
static constexpr LooVariant kLooVariants[] = {
    {4, 2, true}, {4, 2, false}, {2, 2, true}, {8, 1, true}, {4, 1, true}, {4, 4, true}, {2, 4, true}, {8, 2, true},
    {1, 2, true, 8}, {2, 2, true, 8}, {1, 4, true, 8}, {2, 4, true, 8}, {2, 2, true, 4}, {4, 2, true, 4},
    {4, 1, true, 4}, {8, 1, true, 4}, {4, 2, true, 8}, {4, 2, true, 2}, {8, 2, true, 2}, {4, 4, true, 2},
};
static constexpr int kNumLooVariants = sizeof(kLooVariants) / sizeof(kLooVariants[0]);
// default (round 3): 16, loo_wg_kernel<4, 2, 8>: 7.00 TB/s at the c5 shard (N=100,000 x 62,500) on
// MI355X against 6.81 TB/s for the round-1 default 2 (loo_kernel<2, 2, true>, fma-corrected division,
// itself 6.80 against 5.63 TB/s with the IEEE division sequence); tools/kbench.py,
// profiles/r03l_kbench_loo.txt, profiles/r01_kbench_loo.json
int loo_variant_count() { return kNumLooVariants; }
bool loo_variant_ok(int v) { return v >= 0 && v < kNumLooVariants; }

std::string loo_kernel_name(int variant, int ek) {
    const LooVariant& v = kLooVariants[loo_variant_ok(variant) ? variant : kLooDefault];
    const char* sfx = xe_suffix(ek);
    char b[64];
    if (v.W > 0)
        std::snprintf(b, sizeof b, "loo_wg_kernel%s<%d, %d, %d>", sfx, v.G, v.UJ, v.W);
    else
        std::snprintf(b, sizeof b, "loo_kernel%s<%d, %d, %s>", sfx, v.G, v.UJ, v.FD ? "true" : "false");
    return b;
}

template <int G, int UJ, bool FD>
static void launch_loo(const Shard& s, const double* ymod, const double* x1, double sqrtN, double* stats,
                       hipStream_t st, const Timing& tm) {
    // two waves per workgroup, as A^T.u (C5 shape: 7339 vs 7477 us with four);
    // VAMPOMI_LOO_WPB: tuning experiments
    static const int wpb = std::getenv("VAMPOMI_LOO_WPB") ? std::max(1, std::min(4, std::atoi(std::getenv("VAMPOMI_LOO_WPB")))) : 2;
    launch_xe(s, loo_kernel<G, UJ, FD>, loo_kernel_f32<G, UJ, FD>, loo_kernel_u16<G, UJ, FD>,
              dim3((unsigned)cdiv(s.M, wpb * G)), dim3(64 * wpb), st, tm, s.N, s.M, ymod, x1, sqrtN, stats);
}

template <int G, int UJ, int W>
static void launch_loo_wg(const Shard& s, const double* ymod, const double* x1, double sqrtN, double* stats,
                          hipStream_t st, const Timing& tm) {
    launch_xe(s, loo_wg_kernel<G, UJ, W>, loo_wg_kernel_f32<G, UJ, W>, loo_wg_kernel_u16<G, UJ, W>,
              dim3((unsigned)cdiv(s.M, G)), dim3(64 * W), st, tm, s.N, s.M, ymod, x1, sqrtN, stats);
}

hipError_t loo_sums(const Shard& s, const double* ymod, const double* x1, double sqrtN, double* stats,
                    hipStream_t st, int variant, const Timing& tm) {
    if (s.M <= 0) return hipSuccess;
    switch (variant) {
        case 8: launch_loo_wg<1, 2, 8>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 9: launch_loo_wg<2, 2, 8>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 10: launch_loo_wg<1, 4, 8>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 11: launch_loo_wg<2, 4, 8>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 12: launch_loo_wg<2, 2, 4>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 13: launch_loo_wg<4, 2, 4>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 14: launch_loo_wg<4, 1, 4>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 15: launch_loo_wg<8, 1, 4>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 16: launch_loo_wg<4, 2, 8>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 17: launch_loo_wg<4, 2, 2>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 18: launch_loo_wg<8, 2, 2>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 19: launch_loo_wg<4, 4, 2>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 0: launch_loo<4, 2, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 1: launch_loo<4, 2, false>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 2: launch_loo<2, 2, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 3: launch_loo<8, 1, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 4: launch_loo<4, 1, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 5: launch_loo<4, 4, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 6: launch_loo<2, 4, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 7: launch_loo<8, 2, true>(s, ymod, x1, sqrtN, stats, st, tm); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int KT, int G, int UJ>
static void launch_loo_multi(const Shard& s, const double* ymod, const double* x1, double sqrtN, double* stats,
                             hipStream_t st, const Timing& tm) {
    const int64_t Mx = s.M > 1 ? s.M : 1;
    launch_xe(s, loo_multi_kernel<KT, G, UJ, 8>, loo_multi_kernel_f32<KT, G, UJ, 8>, loo_multi_kernel_u16<KT, G, UJ, 8>,
              dim3((unsigned)cdiv(s.M, G)), dim3(64 * 8), st, tm, s.N, s.M, ymod, s.ld, x1, Mx, sqrtN, stats);
}

std::string loo_multi_kernel_name(int KT, int ek) {
    const int G = KT == 2 ? kLooMultiG2 : KT == 3 ? kLooMultiG3 : kLooMultiG4;
    const int UJ = KT == 2 ? kLooMultiUJ2 : KT == 3 ? kLooMultiUJ3 : kLooMultiUJ4;
    char b[64];
    std::snprintf(b, sizeof b, "loo_multi_kernel%s<%d, %d, %d, 8>", xe_suffix(ek), KT, G, UJ);
    return b;
}

// G and UJ per KT (kernels.h): the fastest of the scratch-free choices timed
// at the C5 shard on MI355X, <2: 4, 2>, <3: 4, 1>, <4: 2, 2> against
// <2: 2, 4 | 4, 1>, <3: 2, 2 | 4, 2>, <4: 4, 1 | 4, 2> (profiles/assoc_multi.md);
// they do not change the bits
hipError_t loo_multi_sums(const Shard& s, int KT, const double* ymod, const double* x1, double sqrtN, double* stats,
                          hipStream_t st, const Timing& tm) {
    if (s.M <= 0) return hipSuccess;
    switch (KT) {
        case 2: launch_loo_multi<2, kLooMultiG2, kLooMultiUJ2>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 3: launch_loo_multi<3, kLooMultiG3, kLooMultiUJ3>(s, ymod, x1, sqrtN, stats, st, tm); break;
        case 4: launch_loo_multi<4, kLooMultiG4, kLooMultiUJ4>(s, ymod, x1, sqrtN, stats, st, tm); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// leave-one-chromosome-out test
// ---------------------------------------------------------------------------
// Segmented A.x, stage 1: workgroup (chunk ch, row tile t) streams the
// kSegRows rows of tile t of the chunk's columns, in list order, and stores
// partial slot ch.  Rows per lane as ax_partial's R = 2 tiles (wave w the slab
// of 128 rows, lane l rows 2l and 2l + 1: one row pair per column), U columns
// loaded before any arithmetic, the term (x - mave_i) * (msig_i * x_i) as
// ax_piece forms it.  The tile is the fast index of the grid, so workgroups
// resident together read neighbouring pieces of the same columns.
template <int U, class XE>
__device__ __forceinline__ void ax_seg_body(const XE* __restrict__ X, int64_t ld, int64_t N,
                                            const double* __restrict__ mave, const double* __restrict__ msig,
                                            const double* __restrict__ x, const int32_t* __restrict__ cols,
                                            const int32_t* __restrict__ chunk_at, int64_t tiles,
                                            double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ch = (int64_t)blockIdx.x / tiles, t = (int64_t)blockIdx.x - ch * tiles;
    const int64_t j0 = t * kSegRows + (int64_t)wave * 128 + 2 * lane;
    if (j0 >= N) return;  // (no barrier below)
    const int i1 = chunk_at[ch + 1];
    int i = chunk_at[ch];
    const XE* base = X + j0;
    double a0 = 0.0, a1 = 0.0;
    for (; i + (U - 1) < i1; i += U) {
        int64_t c[U];
        xpair_t<XE> xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c[u] = cols[i + u];
            xv[u] = ldx<true>(base + c[u] * ld);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double ave = mave[c[u]];
            const double w = msig[c[u]] * x[c[u]];
            a0 += (widen(xv[u]).x - ave) * w;
            a1 += (widen(xv[u]).y - ave) * w;
        }
    }
    for (; i < i1; ++i) {
        const int64_t c = cols[i];
        const v2d xv = widen(ldx<true>(base + c * ld));
        const double ave = mave[c];
        const double w = msig[c] * x[c];
        a0 += (xv.x - ave) * w;
        a1 += (xv.y - ave) * w;
    }
    double* dst = part + ch * ld + j0;
    dst[0] = a0;
    if (j0 + 1 < N) dst[1] = a1;
}

template <int U>
__global__ __launch_bounds__(kBlock) void ax_seg_kernel(const double* __restrict__ X, int64_t ld, int64_t N,
                                                        const double* __restrict__ mave,
                                                        const double* __restrict__ msig, const double* __restrict__ x,
                                                        const int32_t* __restrict__ cols,
                                                        const int32_t* __restrict__ chunk_at, int64_t tiles,
                                                        double* __restrict__ part) {
    ax_seg_body<U>(X, ld, N, mave, msig, x, cols, chunk_at, tiles, part);
}

template <int U>
__global__ __launch_bounds__(kBlock) void ax_seg_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                            const double* __restrict__ mave,
                                                            const double* __restrict__ msig,
                                                            const double* __restrict__ x,
                                                            const int32_t* __restrict__ cols,
                                                            const int32_t* __restrict__ chunk_at, int64_t tiles,
                                                            double* __restrict__ part) {
    ax_seg_body<U>(X, ld, N, mave, msig, x, cols, chunk_at, tiles, part);
}

template <int U>
__global__ __launch_bounds__(kBlock) void ax_seg_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                            const double* __restrict__ mave,
                                                            const double* __restrict__ msig,
                                                            const double* __restrict__ x,
                                                            const int32_t* __restrict__ cols,
                                                            const int32_t* __restrict__ chunk_at, int64_t tiles,
                                                            double* __restrict__ part) {
    ax_seg_body<U>(X, ld, N, mave, msig, x, cols, chunk_at, tiles, part);
}

constexpr int kSegU = 8;  // columns in flight (ax_partial's default variant)

std::string ax_seg_kernel_name(int ek) {
    char b[48];
    std::snprintf(b, sizeof b, "ax_seg_kernel%s<%d>", xe_suffix(ek), kSegU);
    return b;
}

hipError_t ax_seg_partial(const Shard& s, const double* x, const int32_t* cols, const int32_t* chunk_at, int nchunks,
                          double* part, hipStream_t st, const Timing& tm) {
    if (nchunks <= 0 || s.N <= 0) return hipSuccess;
    const int64_t tiles = cdiv(s.N, kSegRows);
    if (tiles * nchunks > 0x7fffffffLL) return hipErrorInvalidValue;
    launch_xe(s, ax_seg_kernel<kSegU>, ax_seg_kernel_f32<kSegU>, ax_seg_kernel_u16<kSegU>,
              dim3((unsigned)(tiles * nchunks)), dim3(kBlock), st, tm, s.N, s.mave, s.msig, x, cols, chunk_at, tiles, part);
    return hipGetLastError();
}

// Stage 2: z[c][j] = the slots of label c's chunks added in chunk order
// (zero for a label without chunks); if div > 0 then / div.  Pad rows are not
// written.  grid: (N / kBlock, G)
__global__ __launch_bounds__(kBlock) void ax_seg_reduce_kernel(int64_t N, int64_t ld,
                                                               const int32_t* __restrict__ lab_chunk,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ z, double div) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= N) return;
    const int c = blockIdx.y;
    const int k1 = lab_chunk[c + 1];
    int k = lab_chunk[c];
    const double* p = part + j;
    double s = 0.0;
    for (; k + 4 <= k1; k += 4) {
        const double q0 = p[(int64_t)(k + 0) * ld], q1 = p[(int64_t)(k + 1) * ld];
        const double q2 = p[(int64_t)(k + 2) * ld], q3 = p[(int64_t)(k + 3) * ld];
        s += q0;
        s += q1;
        s += q2;
        s += q3;
    }
    for (; k < k1; ++k) s += p[(int64_t)k * ld];
    if (div > 0.0) s /= div;
    z[(int64_t)c * ld + j] = s;
}

hipError_t ax_seg_reduce(int G, int64_t N, int64_t ld, const int32_t* lab_chunk, const double* part, double* z,
                         double div, hipStream_t st) {
    if (G <= 0 || N <= 0) return hipSuccess;
    hipLaunchKernelGGL(ax_seg_reduce_kernel, dim3((unsigned)cdiv(N, kBlock), (unsigned)G), dim3(kBlock), 0, st, N, ld,
                       lab_chunk, part, z, div);
    return hipGetLastError();
}

// z = z_0 + z_1 + ... + z_{G-1} (ascending c), then zc[c][j] = (y[j] - z) +
// z_c[j] in place: y with the fitted effect of every marker outside label c
// taken out.  div > 0: z_c stands for zc[c] / div (the all-reduced raw sums)
__global__ __launch_bounds__(kBlock) void loco_resid_kernel(int G, int64_t N, int64_t ld,
                                                            const double* __restrict__ y, double* zc, double div) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= N) return;
    auto zof = [&](int c) {
        const double v = zc[(int64_t)c * ld + j];
        return div > 0.0 ? v / div : v;
    };
    double z = zof(0);
    for (int c = 1; c < G; ++c) z += zof(c);
    const double ym = y[j] - z;
    for (int c = 0; c < G; ++c) zc[(int64_t)c * ld + j] = ym + zof(c);
}

hipError_t loco_resid(int G, int64_t N, int64_t ld, const double* y, double* zc, double div, hipStream_t st) {
    if (G <= 0 || N <= 0) return hipSuccess;
    hipLaunchKernelGGL(loco_resid_kernel, dim3((unsigned)cdiv(N, kBlock)), dim3(kBlock), 0, st, G, N, ld, y, zc, div);
    return hipGetLastError();
}

// The marker pass: loo_multi_body<1, kLocoG, UJ, 8> over a group of the list
// instead of G neighbouring columns, with x1 = 0 and the phenotype of the
// group's label.  ym = y + q * 0 is y, so the quotient is not formed; rows,
// per-lane order, wave_sum and the wave-order LDS sum are that body's, so a marker's
// five sums are bit for bit those of loo_wg_kernel<*, *, 8> on (y_c, 0).  The
// markers of a group share y, and with it sum y and sum y^2 operation for
// operation: those two are accumulated once per group (acc[3 G], acc[3 G + 1])
// and stored for each of its markers.
template <int G, int UJ, int W, class XE>
__device__ __forceinline__ void loco_body(const XE* __restrict__ X, int64_t ld, int64_t N,
                                          const double* __restrict__ ys, int64_t ldy,
                                          const int32_t* __restrict__ grp_col, const int32_t* __restrict__ grp_lab,
                                          double* __restrict__ stats) {
    constexpr int NA = 3 * G + 2;
    __shared__ double part[W][NA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* gc = grp_col + (int64_t)blockIdx.x * G;
    const double* __restrict__ y = ys + (int64_t)grp_lab[blockIdx.x] * ldy;
    double acc[NA];
    const XE* col[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int32_t m = gc[g] >= 0 ? gc[g] : gc[0];  // a pad entry reads the group's first column: discarded
        col[g] = X + (int64_t)m * ld;
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[q] = 0.0;
    auto addx = [&](int g, double m, double ym) {
        acc[3 * g] += m;
        acc[3 * g + 1] += m * m;
        acc[3 * g + 2] += m * ym;
    };
    auto addy = [&](double ym) {
        acc[3 * G] += ym;
        acc[3 * G + 1] += ym * ym;
    };
    constexpr int64_t RS = 128 * W;  // rows per load round of the workgroup
    int64_t j = 2 * lane + 128 * wave;
    for (; j + RS * (UJ - 1) < N; j += RS * UJ) {
        v2d yy[UJ];
        xpair_t<XE> xx[UJ][G];
#pragma unroll
        for (int t = 0; t < UJ; ++t)
#pragma unroll
            for (int g = 0; g < G; ++g) xx[t][g] = ldx<true>(col[g] + j + RS * t);
#pragma unroll
        for (int t = 0; t < UJ; ++t) yy[t] = ld2(y + j + RS * t);
#pragma unroll
        for (int t = 0; t < UJ; ++t) {
            addy(yy[t].x);
            addy(yy[t].y);
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int t = 0; t < UJ; ++t) {
                addx(g, widen(xx[t][g]).x, yy[t].x);
                addx(g, widen(xx[t][g]).y, yy[t].y);
            }
    }
    for (; j < N; j += RS) {  // (N even or the pad row: ld-padded columns, zero pads)
        xpair_t<XE> xx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) xx[g] = ldx<true>(col[g] + j);
        const v2d yy = ld2(y + j);
        addy(yy.x);
        addy(yy.y);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            addx(g, widen(xx[g]).x, yy.x);
            addx(g, widen(xx[g]).y, yy.y);
        }
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) part[wave][q] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < 5 * G) {
        const int g = threadIdx.x / 5, q = threadIdx.x % 5;
        const int32_t m = gc[g];
        if (m >= 0) {
            const int src = q < 3 ? 3 * g + q : 3 * G + (q - 3);
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) s += part[w][src];
            stats[5 * (int64_t)m + q] = s;  // the marker's own index
        }
    }
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loco_kernel(const double* __restrict__ X, int64_t ld, int64_t N,
                                                      const double* __restrict__ ys, int64_t ldy,
                                                      const int32_t* __restrict__ grp_col,
                                                      const int32_t* __restrict__ grp_lab,
                                                      double* __restrict__ stats) {
    loco_body<G, UJ, W>(X, ld, N, ys, ldy, grp_col, grp_lab, stats);
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loco_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                          const double* __restrict__ ys, int64_t ldy,
                                                          const int32_t* __restrict__ grp_col,
                                                          const int32_t* __restrict__ grp_lab,
                                                          double* __restrict__ stats) {
    loco_body<G, UJ, W>(X, ld, N, ys, ldy, grp_col, grp_lab, stats);
}

template <int G, int UJ, int W>
__global__ __launch_bounds__(64 * W) void loco_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                          const double* __restrict__ ys, int64_t ldy,
                                                          const int32_t* __restrict__ grp_col,
                                                          const int32_t* __restrict__ grp_lab,
                                                          double* __restrict__ stats) {
    loco_body<G, UJ, W>(X, ld, N, ys, ldy, grp_col, grp_lab, stats);
}

constexpr int kLocoUJ = 2;  // (kLooDefault's: loo_wg_kernel<4, 2, 8>)

std::string loco_kernel_name(int ek) {
    char b[48];
    std::snprintf(b, sizeof b, "loco_kernel%s<%d, %d, 8>", xe_suffix(ek), kLocoG, kLocoUJ);
    return b;
}

hipError_t loco_sums(const Shard& s, const double* ys, int64_t ldy, const int32_t* grp_col, const int32_t* grp_lab,
                     int ngroups, double* stats, hipStream_t st, const Timing& tm) {
    if (ngroups <= 0) return hipSuccess;
    launch_xe(s, loco_kernel<kLocoG, kLocoUJ, 8>, loco_kernel_f32<kLocoG, kLocoUJ, 8>,
              loco_kernel_u16<kLocoG, kLocoUJ, 8>, dim3((unsigned)ngroups), dim3(64 * 8), st, tm, s.N, ys, ldy, grp_col,
              grp_lab, stats);
    return hipGetLastError();
}

// ln B(a, 1/2) and the Student-t upper tail: the same operations as the
// oracle's orc_lnbeta_half / ibeta_cf / orc_t_sf (oracle/vamp_oracle.c),
// standing for Boost's complemented students_t cdf (src/utilities.cpp:278-279)
__device__ double lnbeta_half(double a) {
    if (a >= 30.0) {
        const double i1 = 1.0 / a, i2 = i1 * i1;
        const double d = 0.5 * log(a) - i1 * (1.0 / 8.0) + i1 * i2 * (1.0 / 192.0) - i1 * i2 * i2 * (1.0 / 640.0) +
                         i1 * i2 * i2 * i2 * (17.0 / 14336.0);
        return 0.57236494292470008707 - d;
    }
    return lgamma(a) + lgamma(0.5) - lgamma(a + 0.5);
}

__device__ double ibeta_cf(double a, double b, double x) {
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

__device__ double t_sf_pos(double t, double df) {  // t > 0
    const double a = 0.5 * df, b = 0.5, tt = t * t;
    if (!isfinite(tt)) return 0.0;  // t = inf or t * t overflows: x = 0, I_0 = 0 (as orc_t_sf)
    const double lx = -log1p(tt / df);
    const double l1x = log(tt / (df + tt));
    const double x = df / (df + tt);
    const double front = exp(a * lx + b * l1x - lnbeta_half(a));
    if (t >= 3.0 && x < (a + 1.0) / (a + b + 2.0)) return 0.5 * (front * ibeta_cf(a, b, x) / a);
    return 0.5 * (1.0 - front * ibeta_cf(b, a, tt / (df + tt)) / b);
}

__device__ double t_sf(double t, double df) {
    if (isnan(t) || isnan(df)) return __builtin_nan("");
    if (t == 0.0) return 0.5;
    return t > 0.0 ? t_sf_pos(t, df) : 1.0 - t_sf_pos(-t, df);
}

__global__ void loo_pval_kernel(int64_t M, const double* __restrict__ stats, int n, double* __restrict__ pvals) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= M) return;
    const double* s = stats + 5 * j;
    const double sumx = s[0], sumsqx = s[1], sumxy = s[2], sumy = s[3], sumsqy = s[4];
    const double s2y = (sumsqy - sumy * sumy / n) / (n - 1);
    const double s2x = (sumsqx - sumx * sumx / n) / (n - 1);
    const double sxy = (sumxy - sumx * sumy / n) / (n - 1);
    const double rxy = sxy / sqrt(s2x * s2y);
    const double t = rxy * sqrt((n - 2) / (1 - rxy * rxy));
    pvals[j] = 2.0 * t_sf(t > 0 ? t : (0 - t), (double)(n - 2));
}

hipError_t loo_pvals(int64_t M, const double* stats, int n, double* pvals, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(loo_pval_kernel, dim3((unsigned)cdiv(M, kBlock)), dim3(kBlock), 0, st, M, stats, n, pvals);
    return hipGetLastError();
}

__global__ void se_pval_kernel(int64_t M, const double* __restrict__ r1, double sd, double* __restrict__ pvals) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= M) return;
    const double diff = (0.0 - r1[j]) / sd;  // boost normal cdf at 0: erfc(-diff / sqrt(2)) / 2
    double p = erfc(-diff / M_SQRT2) / 2;
    if (r1[j] <= 0.0) p = 1 - p;
    pvals[j] = p;
}

hipError_t se_pvals(int64_t M, const double* r1, double gam1, int64_t N, double* pvals, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    const double sd = sqrt(1.0 / (gam1 * (double)N));
    hipLaunchKernelGGL(se_pval_kernel, dim3((unsigned)cdiv(M, kBlock)), dim3(kBlock), 0, st, M, r1, sd, pvals);
    return hipGetLastError();
}

}  // namespace vk
