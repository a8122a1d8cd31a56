// kernels.hip — the gfx950 (CDNA4) kernels of the gVAMPomi VAMP hot path that
// stream X: A.x (the tile variants, their plans and ax_reduce), A^T.u, the
// whole-column one-pass operator (op_plan, lds_allow, op_reduce; the team
// operator is atax_team.hip), the marker statistics, the pure read stream and
// the synthetic-data generators, with the tuning tables behind kernel_name()
// and op_kernel_name().  The vector side lives in vec.hip, the PCG vector
// steps in pcg.hip, the probit model in probit.hip; kernels.h is the one
// interface of them all.
//
// The design matrix X is fp64, marker-major (each marker = one column of N
// samples, contiguous, README.md:15 / src/data.cpp:127-142), resident in HBM
// with a 128-byte aligned column stride ld.  A.x and A^T.u are HBM-bound
// GEMVs (0.375 flop/B); they stream X with 16-byte-per-lane nontemporal loads
// and never use MFMA.  All reductions are two-stage with fixed block counts
// and fixed summation order, so every result is bitwise reproducible run to
// run and independent of the rank count's effect on scheduling.
#include "kernels.h"
#include "kdev.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace vk {

// ---------------------------------------------------------------------------
// A.x   (data::Ax, src/data.cpp:340-373)
// ---------------------------------------------------------------------------
// Work split.  The rows are cut into tiles of 256*R, and the (tile, marker)
// segments, tiles*M of them, into G equal shares, one per workgroup, with
// G = two workgroups per CU: one resident round in which every CU carries the
// same load (a tile x chunk grid leaves some CUs a third workgroup whenever
// tiles*chunks is not a multiple of the CU count, and those set the kernel's
// time).  Two layouts of the shares:
//  * band plan (tiles <= G): the markers are cut into bands of about 64 MiB
//    of columns, and workgroup g owns the same fraction [g*tiles, (g+1)*tiles)
//    / G of the tile-major (tile, marker-in-band) space of every band: one or
//    two tiles, a run of each band's columns per tile.  All workgroups walk
//    the bands together, so the reads in flight stay inside one band (page
//    translation and DRAM locality: equal contiguous stripes spread over a
//    50 GB matrix ran 4% slower).  A band's column boundaries are dithered
//    per band so floor rounding does not favour the same workgroups.
//  * stripe plan (tiles > G): workgroup g owns the contiguous stripe
//    [g*span, (g+1)*span) of the tile-major space (whole tiles, in order).
// Either way the piece of tile t that workgroup g streams lands in partial
// slot g - lo(t) of that tile, lo(t) = t*sa/sb ((sa, sb) = (G, tiles) for
// bands, (M, span) for stripes).  The plan does not depend on the batch width
// K, so batched and solo passes sum identically.
//
// Within a piece, wave w owns the contiguous slab of 64*R rows
// [tile0 + 64*R*w, ...); lane l owns rows 2l + 128q (q < R/2), i.e. each
// 16-byte load instruction reads 1 KiB contiguous, and the workgroup streams
// 2*R KiB of every marker column.  U markers are loaded before any
// arithmetic (U*R/2 16-byte loads in flight per lane).  Per-sample summation
// order within a slot is the reference's: markers in index order,
// acc += (x - mave_i) * (msig_i * x_i).
// x_k[i] of the pass: p_k[i], or with fusion (FU) z_k[i] + beta_k*p_k[i]
// (the CG direction update, src/vamp.cpp:738-739, as every consumer of the new
// direction forms it).  The kernel stores nothing but its partials, so the
// compiler keeps the per-marker loads scalar.
template <int K, int R, int U, bool NT, bool FU, class XE>
__device__ __forceinline__ void ax_piece(const XE* __restrict__ X, int64_t ld, int64_t N,
                                         const double* __restrict__ mave, const double* __restrict__ msig,
                                         const CPtrs& xs, const AxFuse& fu, const double (&bk)[K], int64_t j0,
                                         int64_t i0, int64_t i1, double (&acc)[K][R]) {
    constexpr int P = R / 2;  // 16-byte pieces per lane per marker
    int64_t off[P];  // invalid pieces read row 0 of the column (in bounds) and are discarded at the store
#pragma unroll
    for (int q = 0; q < P; ++q) off[q] = (j0 + 128 * q < N) ? 128 * q : -j0;
    const XE* col = X + i0 * ld + j0;
    int64_t i = i0;
    for (; i + (U - 1) < i1; i += U) {
        xpair_t<XE> xv[U][P];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < P; ++q)
                xv[u][q] = ldx<NT>(col + (int64_t)u * ld + off[q]);
        double xk[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k)
                xk[u][k] = FU ? fu.z.p[k][i + u] + bk[k] * xs.p[k][i + u] : xs.p[k][i + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double ave = mave[i + u];
            const double sg = msig[i + u];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double w = sg * xk[u][k];
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    acc[k][2 * q] += (widen(xv[u][q]).x - ave) * w;
                    acc[k][2 * q + 1] += (widen(xv[u][q]).y - ave) * w;
                }
            }
        }
        col += (int64_t)U * ld;
    }
    for (; i < i1; ++i) {
        xpair_t<XE> xv[P];
#pragma unroll
        for (int q = 0; q < P; ++q) xv[q] = ldx<NT>(col + off[q]);
        double xk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) xk[k] = FU ? fu.z.p[k][i] + bk[k] * xs.p[k][i] : xs.p[k][i];
        const double ave = mave[i];
        const double sg = msig[i];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double w = sg * xk[k];
#pragma unroll
            for (int q = 0; q < P; ++q) {
                acc[k][2 * q] += (widen(xv[q]).x - ave) * w;
                acc[k][2 * q + 1] += (widen(xv[q]).y - ave) * w;
            }
        }
        col += ld;
    }
}

template <int K, int R>
__device__ __forceinline__ void ax_store(double* __restrict__ part, int64_t slot, int64_t ld, int64_t N, int64_t j0,
                                         const double (&acc)[K][R]) {
    double* dst = part + slot * K * ld + j0;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int q = 0; q < R / 2; ++q) {
            if (j0 + 128 * q < N) {
                dst[(int64_t)k * ld + 128 * q] = acc[k][2 * q];
                if (j0 + 128 * q + 1 < N) dst[(int64_t)k * ld + 128 * q + 1] = acc[k][2 * q + 1];
            }
        }
}

template <int K, int R>
__device__ __forceinline__ void ax_zero(double (&acc)[K][R]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[k][r] = 0.0;
}

// (the body of ax_partial_kernel, ax_partial_kernel_f32 and ax_partial_kernel_u16: XE is X's element type)
template <int K, int R, int U, bool NT, bool FU, class XE>
__device__ __forceinline__ void ax_partial_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                                const double* __restrict__ mave,
                                                const double* __restrict__ msig, const CPtrs& xs, int64_t tiles,
                                                int64_t span, int64_t nband, double* __restrict__ part,
                                                const AxFuse& fu) {
    if (fu.gate && !*fu.gate) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = blockIdx.x, G = gridDim.x;
    double bk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) bk[k] = FU ? fu.beta[k] : 0.0;
    const int64_t slab = (int64_t)wave * (64 * R) + 2 * lane;  // row offset inside a tile
    double acc[K][R];
    if (nband > 0) {
        // band plan: u-space [g*tiles, (g+1)*tiles) over tiles of G units each
        const int64_t ulo = g * tiles, uhi = ulo + tiles;
        const int64_t tA = ulo / G;
        const int64_t xa0 = ulo - tA * G, xa1 = ((uhi < (tA + 1) * G) ? uhi : (tA + 1) * G) - tA * G;
        const bool hasB = uhi > (tA + 1) * G;
        const int64_t xb1 = uhi - (tA + 1) * G;
        const int64_t jA = tA * (kBlock * R) + slab, jB = jA + kBlock * R;
        double accB[K][R];
        ax_zero<K, R>(acc);
        ax_zero<K, R>(accB);
        // boundaries in whole groups of U markers (full-width load trips); the
        // last group boundary stands for M (the M % U leftover markers)
        const int64_t Mu = M / U;
        for (int64_t p = 0; p < nband; ++p) {
            const int64_t c = p * Mu / nband, w = (p + 1) * Mu / nband - c;
            const int64_t phi = (int64_t)(((uint64_t)p * 0x9E3779B97F4A7C15ULL) >> 40) % G;  // dither in [0, G)
            if (jA < N) {
                const int64_t u0 = c + (xa0 * w + phi) / G, u1 = c + (xa1 * w + phi) / G;
                ax_piece<K, R, U, NT, FU>(X, ld, N, mave, msig, xs, fu, bk, jA, u0 == Mu ? M : u0 * U,
                                      u1 == Mu ? M : u1 * U, acc);
            }
            if (hasB && jB < N) {
                const int64_t u1 = c + (xb1 * w + phi) / G;
                ax_piece<K, R, U, NT, FU>(X, ld, N, mave, msig, xs, fu, bk, jB, c * U, u1 == Mu ? M : u1 * U,
                                      accB);
            }
        }
        if (jA < N) ax_store<K, R>(part, g - (tA * G) / tiles, ld, N, jA, acc);
        if (hasB && jB < N) ax_store<K, R>(part, g - ((tA + 1) * G) / tiles, ld, N, jB, accB);
        return;
    }
    // stripe plan
    const int64_t total = tiles * M;
    int64_t pos = g * span;
    const int64_t end = (pos + span < total) ? pos + span : total;
    while (pos < end) {
        const int64_t t = pos / M;
        const int64_t i0 = pos - t * M;
        const int64_t i1 = (i0 + (end - pos) < M) ? i0 + (end - pos) : M;
        pos += i1 - i0;
        const int64_t j0 = t * (kBlock * R) + slab;
        if (j0 >= N) continue;
        ax_zero<K, R>(acc);
        ax_piece<K, R, U, NT, FU>(X, ld, N, mave, msig, xs, fu, bk, j0, i0, i1, acc);
        ax_store<K, R>(part, g - (t * M) / span, ld, N, j0, acc);
    }
}

template <int K, int R, int U, bool NT, bool FU>
__global__ __launch_bounds__(kBlock) void ax_partial_kernel(const double* __restrict__ X, int64_t ld,
                                                            int64_t N, int64_t M,
                                                            const double* __restrict__ mave,
                                                            const double* __restrict__ msig, CPtrs xs,
                                                            int64_t tiles, int64_t span, int64_t nband,
                                                            double* __restrict__ part, AxFuse fu) {
    ax_partial_body<K, R, U, NT, FU>(X, ld, N, M, mave, msig, xs, tiles, span, nband, part, fu);
}

template <int K, int R, int U, bool NT, bool FU>
__global__ __launch_bounds__(kBlock) void ax_partial_kernel_f32(const float* __restrict__ X, int64_t ld,
                                                                int64_t N, int64_t M,
                                                                const double* __restrict__ mave,
                                                                const double* __restrict__ msig, CPtrs xs,
                                                                int64_t tiles, int64_t span, int64_t nband,
                                                                double* __restrict__ part, AxFuse fu) {
    ax_partial_body<K, R, U, NT, FU>(X, ld, N, M, mave, msig, xs, tiles, span, nband, part, fu);
}

template <int K, int R, int U, bool NT, bool FU>
__global__ __launch_bounds__(kBlock) void ax_partial_kernel_u16(const uint16_t* __restrict__ X, int64_t ld,
                                                                int64_t N, int64_t M,
                                                                const double* __restrict__ mave,
                                                                const double* __restrict__ msig, CPtrs xs,
                                                                int64_t tiles, int64_t span, int64_t nband,
                                                                double* __restrict__ part, AxFuse fu) {
    ax_partial_body<K, R, U, NT, FU>(X, ld, N, M, mave, msig, xs, tiles, span, nband, part, fu);
}

// tuning table (rows per lane R, markers in flight U, nontemporal loads)
struct AxVariant { int R, U; bool NT; };
static constexpr AxVariant kAxVariants[] = {
    {2, 8, true}, {2, 8, false}, {4, 4, true}, {4, 8, true}, {8, 4, true}, {2, 4, true}, {2, 12, true},
};
static constexpr int kNumAxVariants = sizeof(kAxVariants) / sizeof(kAxVariants[0]);
// default 0: R=2, U=8, nontemporal (tools/kbench.py)

int ax_variant_count() { return kNumAxVariants + 1; }  // + kAxTeam
bool ax_variant_ok(int v) { return v == kAxDefault || (v >= 0 && v < kNumAxVariants) || v == kAxTeam; }
static_assert(kAxTeam == kNumAxVariants, "the team plan numbers after the tile variants");

static int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 256;
    return cus;
}

AxPlan ax_plan(int64_t N, int64_t M, int variant) { return ax_plan_for(N, M, device_cus(), variant); }

AxPlan ax_plan_for(int64_t N, int64_t M, int cus, int variant) {
    AxPlan p;
    if (variant == kAxDefault || variant == kAxTeam) {
        if (ax_team_plan(N, M, cus, &p) && (variant == kAxTeam || p.T >= kAxTeamMinT)) return p;
        p = AxPlan{};
    }
    p.variant = variant >= 0 && variant < kNumAxVariants ? variant : 0;
    p.rows = (int64_t)kBlock * kAxVariants[p.variant].R;
    p.tiles = cdiv(N, p.rows);
    p.total = p.tiles * M;
    // tuning experiments: VAMPOMI_AX_WPC workgroups per CU, VAMPOMI_AX_BANDSEG
    // segments per workgroup per band (0: stripe plan)
    int64_t wpc = 2, bandseg = 32;
    if (const char* f = std::getenv("VAMPOMI_AX_WPC")) wpc = std::max(1, std::atoi(f));
    if (const char* f = std::getenv("VAMPOMI_AX_BANDSEG")) bandseg = std::max(0, std::atoi(f));
    int64_t G = std::min<int64_t>(wpc * cus, cdiv(p.total, 64));  // >= 64 segments per workgroup
    if (G < 1) G = 1;
    p.span = cdiv(p.total, G);
    if (p.tiles <= G && bandseg > 0 && M >= (int64_t)kAxVariants[p.variant].U) {
        p.groups = (int)G;
        p.nband = std::max<int64_t>(1, std::min<int64_t>(M / kAxVariants[p.variant].U, p.total / (bandseg * G)));
        p.sa = G;
        p.sb = p.tiles;
    } else {
        p.groups = (int)cdiv(p.total, p.span);
        p.nband = 0;
        p.sa = M;
        p.sb = p.span;
    }
    int64_t ns = 1;
    for (int64_t t = 0; t < p.tiles; ++t) ns = std::max(ns, ax_slots(p, t));
    p.nslots = (int)ns;
    return p;
}

// launches go through hipExtLaunchKernelGGL: the optional start / stop events
// are written by the kernel's own dispatch (no extra marker packets around it)
template <int K, int R, int U, bool NT>
static void launch_ax(const Shard& s, const AxPlan& pl, CPtrs x, double* part, hipStream_t st, const Timing& tm,
                      const AxFuse& fu) {
    if (fu.z.p[0])
        launch_xe(s, ax_partial_kernel<K, R, U, NT, true>, ax_partial_kernel_f32<K, R, U, NT, true>,
                  ax_partial_kernel_u16<K, R, U, NT, true>, dim3(pl.groups), dim3(kBlock), st, tm, s.N, s.M, s.mave,
                  s.msig, x, pl.tiles, pl.span, pl.nband, part, fu);
    else
        launch_xe(s, ax_partial_kernel<K, R, U, NT, false>, ax_partial_kernel_f32<K, R, U, NT, false>,
                  ax_partial_kernel_u16<K, R, U, NT, false>, dim3(pl.groups), dim3(kBlock), st, tm, s.N, s.M, s.mave,
                  s.msig, x, pl.tiles, pl.span, pl.nband, part, fu);
}

template <int K>
static bool launch_ax_v(int v, const Shard& s, const AxPlan& pl, CPtrs x, double* part, hipStream_t st,
                        const Timing& tm, const AxFuse& fu) {
    switch (v) {
        case 0: launch_ax<K, 2, 8, true>(s, pl, x, part, st, tm, fu); return true;
        case 1: launch_ax<K, 2, 8, false>(s, pl, x, part, st, tm, fu); return true;
        case 2: launch_ax<K, 4, 4, true>(s, pl, x, part, st, tm, fu); return true;
        case 3: launch_ax<K, 4, 8, true>(s, pl, x, part, st, tm, fu); return true;
        case 4: launch_ax<K, 8, 4, true>(s, pl, x, part, st, tm, fu); return true;
        case 5: launch_ax<K, 2, 4, true>(s, pl, x, part, st, tm, fu); return true;
        case 6: launch_ax<K, 2, 12, true>(s, pl, x, part, st, tm, fu); return true;
        default: return false;
    }
}

hipError_t ax_partial(const Shard& s, const AxPlan& pl, int K, CPtrs x, double* part, hipStream_t st,
                      const Timing& tm, const AxFuse& fu) {
    if (pl.T > 0) return ax_team(s, pl, K, x, part, st, tm, fu);
    if (pl.rows != (int64_t)kBlock * kAxVariants[pl.variant].R || pl.total != pl.tiles * s.M ||
        pl.tiles * pl.rows < s.N)
        return hipErrorInvalidValue;  // plan made for another shape
    bool ok = false;
    switch (K) {
        case 1: ok = launch_ax_v<1>(pl.variant, s, pl, x, part, st, tm, fu); break;
        case 2: ok = launch_ax_v<2>(pl.variant, s, pl, x, part, st, tm, fu); break;
        case 3: ok = launch_ax_v<3>(pl.variant, s, pl, x, part, st, tm, fu); break;
        case 4: ok = launch_ax_v<4>(pl.variant, s, pl, x, part, st, tm, fu); break;
        default: break;
    }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}

// Stage 2: out_k[j] = sum over tile(j)'s slots of part[s][k][j].  A 512-thread
// block covers 64 consecutive samples (one wave per slot group, coalesced
// across lanes); group q sums its contiguous slot range in index order, then
// the 8 group sums are added in group order: a fixed tree, short dependent
// chains.
constexpr int kRedGroups = 8;
__global__ __launch_bounds__(64 * kRedGroups) void ax_reduce_kernel(int K, int64_t N, int64_t ld, int64_t sa,
                                                                    int64_t rows, int64_t sb,
                                                                    const double* __restrict__ part, Ptrs out,
                                                                    double div, const int* gate) {
    if (gate && !*gate) return;
    __shared__ double lds[kRedGroups][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = e < (int64_t)K * N;
    const int k = valid ? (int)(e / N) : 0;
    const int64_t j = valid ? e - (int64_t)k * N : 0;
    const int64_t t = j / rows;
    const int nslots = (int)(((t + 1) * sa - 1) / sb - (t * sa) / sb + 1);
    const int per = (nslots + kRedGroups - 1) / kRedGroups;
    const int c0 = g * per, c1 = (c0 + per < nslots) ? c0 + per : nslots;
    const int64_t stride = (int64_t)K * ld;
    const double* p = part + (int64_t)k * ld + j;
    double s = 0.0;
    if (valid) {
        int c = c0;
        for (; c + 4 <= c1; c += 4) {
            const double q0 = p[(int64_t)(c + 0) * stride], q1 = p[(int64_t)(c + 1) * stride];
            const double q2 = p[(int64_t)(c + 2) * stride], q3 = p[(int64_t)(c + 3) * stride];
            s += q0;
            s += q1;
            s += q2;
            s += q3;
        }
        for (; c < c1; ++c) s += p[(int64_t)c * stride];
    }
    lds[g][lane] = s;
    __syncthreads();
    if (g == 0 && valid) {
        double t2 = lds[0][lane];
#pragma unroll
        for (int q = 1; q < kRedGroups; ++q) t2 += lds[q][lane];
        if (div > 0.0) t2 /= div;  // src/data.cpp:369-370: Ax_total[i] /= sqrt(N)
        out.p[k][j] = t2;
    }
}

hipError_t ax_reduce(const AxPlan& pl, int K, int64_t N, int64_t ld, const double* part, Ptrs out, double div,
                     hipStream_t st, const int* gate) {
    const int64_t n = (int64_t)K * N;
    hipLaunchKernelGGL(ax_reduce_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64 * kRedGroups), 0, st, K, N, ld,
                       pl.sa, pl.rows, pl.sb, part, out, div, gate);
    return hipGetLastError();
}

// A pure read stream (the read ceiling of vampomi_dev_read_ceiling; the same
// shapes as tools/hbm_ceiling's lock and chunk variants).  The sums feed a
// store that never happens (the comparison with the NaN `never`), so no load
// is dead.
template <class XE>
__device__ __forceinline__ void stream_lock_body(const XE* __restrict__ x, int64_t units, double never,
                                                 double* __restrict__ sink) {
    constexpr int U = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = units * blockIdx.x / gridDim.x * 1024, e = units * (blockIdx.x + 1) / gridDim.x * 1024;
    double a0 = 0.0, a1 = 0.0;
    int64_t j = b + 128 * wave + 2 * lane;
    for (; j + 1024 * (U - 1) < e; j += 1024 * U) {
        xpair_t<XE> v[U];
#pragma unroll
        for (int t = 0; t < U; ++t) v[t] = ldx<true>(x + j + 1024 * t);
#pragma unroll
        for (int t = 0; t < U; ++t) {
            a0 += widen(v[t]).x;
            a1 += widen(v[t]).y;
        }
        __syncthreads();
    }
    for (; j < e; j += 1024) {
        const v2d v = widen(ldx<true>(x + j));
        a0 += v.x;
        a1 += v.y;
    }
    if (a0 + a1 == never) sink[0] = a0;
}

__global__ __launch_bounds__(512) void stream_lock_kernel(const double* __restrict__ x, int64_t units,
                                                          double never, double* __restrict__ sink) {
    stream_lock_body(x, units, never, sink);
}

__global__ __launch_bounds__(512) void stream_lock_kernel_f32(const float* __restrict__ x, int64_t units,
                                                              double never, double* __restrict__ sink) {
    stream_lock_body(x, units, never, sink);
}

// 16-bit elements: the resident bytes as 16-byte loads (units of 8 KiB, the
// double kernel's).  A pure read is tied to no summation order, so it does not
// keep the operators' two rows per lane; the words are summed as the bit
// patterns they are, which nothing ever reads.
__global__ __launch_bounds__(512) void stream_lock_kernel_u16(const uint16_t* __restrict__ x, int64_t units,
                                                              double never, double* __restrict__ sink) {
    stream_lock_body(reinterpret_cast<const double*>(x), units, never, sink);
}

template <class XE>
__device__ __forceinline__ void stream_chunk_body(const XE* __restrict__ x, int64_t nchunks, double never,
                                                  double* __restrict__ sink) {
    constexpr int U = 8;
    constexpr int64_t CW = 1 << 17;  // elements per wave (1 MiB of doubles, 512 KiB of floats)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nchunks) return;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t j = w * CW + 2 * lane; j < (w + 1) * CW; j += 128 * U) {
        xpair_t<XE> v[U];
#pragma unroll
        for (int t = 0; t < U; ++t) v[t] = ldx<true>(x + j + 128 * t);
#pragma unroll
        for (int t = 0; t < U; ++t) {
            a0 += widen(v[t]).x;
            a1 += widen(v[t]).y;
        }
    }
    if (a0 + a1 == never) sink[0] = a0;
}

__global__ __launch_bounds__(256) void stream_chunk_kernel(const double* __restrict__ x, int64_t nchunks,
                                                           double never, double* __restrict__ sink) {
    stream_chunk_body(x, nchunks, never, sink);
}

__global__ __launch_bounds__(256) void stream_chunk_kernel_f32(const float* __restrict__ x, int64_t nchunks,
                                                               double never, double* __restrict__ sink) {
    stream_chunk_body(x, nchunks, never, sink);
}

// (16-byte loads, 1 MiB per wave: see stream_lock_kernel_u16)
__global__ __launch_bounds__(256) void stream_chunk_kernel_u16(const uint16_t* __restrict__ x, int64_t nchunks,
                                                               double never, double* __restrict__ sink) {
    stream_chunk_body(reinterpret_cast<const double*>(x), nchunks, never, sink);
}

hipError_t stream_read(const void* x, int ek, int64_t n, int kind, int cus, hipStream_t st, const Timing& tm,
                       double* sink, double* bytes) {
    const double never = __builtin_nan("");
    if (ek == kXU16) {  // n 16-bit elements are n / 4 eight-byte words, read as the double kernels read them
        const int64_t nw = n / 4;
        if (kind == 0) {
            const int64_t units = nw / 1024;
            if (units < cus) return hipErrorInvalidValue;
            *bytes = 8.0 * (double)(units * 1024);
            hipExtLaunchKernelGGL(stream_lock_kernel_u16, dim3(cus), dim3(512), 0, st, tm.start, tm.stop, 0,
                                  static_cast<const uint16_t*>(x), units, never, sink);
        } else {
            const int64_t nch = nw / (1 << 17);
            if (nch < 1) return hipErrorInvalidValue;
            *bytes = 8.0 * (double)(nch << 17);
            hipExtLaunchKernelGGL(stream_chunk_kernel_u16, dim3((unsigned)((nch + 3) / 4)), dim3(256), 0, st,
                                  tm.start, tm.stop, 0, static_cast<const uint16_t*>(x), nch, never, sink);
        }
        return hipGetLastError();
    }
    const bool f32 = ek == kXF32;
    const double esize = f32 ? 4.0 : 8.0;
    if (kind == 0) {
        const int64_t units = n / 1024;
        if (units < cus) return hipErrorInvalidValue;
        *bytes = esize * (double)(units * 1024);
        if (f32)
            hipExtLaunchKernelGGL(stream_lock_kernel_f32, dim3(cus), dim3(512), 0, st, tm.start, tm.stop, 0,
                                  static_cast<const float*>(x), units, never, sink);
        else
            hipExtLaunchKernelGGL(stream_lock_kernel, dim3(cus), dim3(512), 0, st, tm.start, tm.stop, 0,
                                  static_cast<const double*>(x), units, never, sink);
    } else {
        const int64_t nch = n / (1 << 17);
        if (nch < 1) return hipErrorInvalidValue;
        *bytes = esize * (double)(nch << 17);
        if (f32)
            hipExtLaunchKernelGGL(stream_chunk_kernel_f32, dim3((unsigned)((nch + 3) / 4)), dim3(256), 0, st,
                                  tm.start, tm.stop, 0, static_cast<const float*>(x), nch, never, sink);
        else
            hipExtLaunchKernelGGL(stream_chunk_kernel, dim3((unsigned)((nch + 3) / 4)), dim3(256), 0, st, tm.start,
                                  tm.stop, 0, static_cast<const double*>(x), nch, never, sink);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// A^T.u  (data::ATx + data::dot_product, src/data.cpp:294-333)
// ---------------------------------------------------------------------------
// A wave owns G consecutive markers (workgroups of two waves, dispatched in
// order: the dispatcher balances the CUs); lanes stride the samples two at a time,
// so each load instruction reads 1 KiB of one column, UJ such 128-row steps
// per loop trip.  Every u value loaded serves G markers.  The wave's partial
// dots are reduced with an xor butterfly; mode 1 fuses the lmmse_mult
// epilogue (src/vamp.cpp:656-659).
// (the body of atx_kernel, atx_kernel_f32 and atx_kernel_u16: XE is X's element type)
template <int G, int K, int MODE, int UJ, bool NT, class XE>
__device__ __forceinline__ void atx_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                         const double* __restrict__ mave, const double* __restrict__ msig,
                                         const CPtrs& u, const Ptrs& out, double scale, double tau, double gam2,
                                         const CPtrs& pv, const int* __restrict__ gate, const CPtrs& zf,
                                         const double* __restrict__ beta, const Ptrs& sraw) {
    if (gate && !*gate) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * G;
    double acc[G][K];
    double mu[G];
    const XE* col[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t m = (m0 + g < M) ? m0 + g : M - 1;  // clamp: in-bounds, discarded
        mu[g] = mave[m];
        col[g] = X + m * ld;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[g][k] = 0.0;
    }
    int64_t j = 2 * lane;
    for (; j + 128 * (UJ - 1) < N; j += 128 * UJ) {
        v2d uu[UJ][K];
        xpair_t<XE> xx[UJ][G];
#pragma unroll
        for (int t = 0; t < UJ; ++t)
#pragma unroll
            for (int g = 0; g < G; ++g) xx[t][g] = ldx<NT>(col[g] + j + 128 * t);
#pragma unroll
        for (int t = 0; t < UJ; ++t)
#pragma unroll
            for (int k = 0; k < K; ++k) uu[t][k] = ld2(u.p[k] + j + 128 * t);
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int t = 0; t < UJ; ++t) {
                const double d0 = widen(xx[t][g]).x - mu[g], d1 = widen(xx[t][g]).y - mu[g];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    acc[g][k] += d0 * uu[t][k].x;
                    acc[g][k] += d1 * uu[t][k].y;
                }
            }
        }
    }
    for (; j < N; j += 128) {  // tail; j+1 may be the zero pad row (u pad is zero too)
        v2d uu[K];
        xpair_t<XE> xx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) xx[g] = ldx<NT>(col[g] + j);
#pragma unroll
        for (int k = 0; k < K; ++k) uu[k] = ld2(u.p[k] + j);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double d0 = widen(xx[g]).x - mu[g], d1 = widen(xx[g]).y - mu[g];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[g][k] += d0 * uu[k].x;
                acc[g][k] += d1 * uu[k].y;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double dot = wave_sum(acc[g][k]);
            const int64_t m = m0 + g;
            if (m < M && lane == 0) {
                double val = msig[m] * dot;  // sigma_inv * dpa
                val *= scale;                // ATx[mloc] *= 1/sqrt(N)
                if (MODE == 1 && sraw.p[0]) sraw.p[k][m] = val;  // A^T(A p) itself (CG recurrences)
                if (MODE == 1) {
                    const double pk = zf.p[0] ? zf.p[k][m] + beta[k] * pv.p[k][m] : pv.p[k][m];
                    val *= tau;        // res[i] *= tau
                    val += gam2 * pk;  // res[i] += gam2 * v[i]
                }
                out.p[k][m] = val;
            }
        }
    }
}

template <int G, int K, int MODE, int UJ, bool NT>
__global__ __launch_bounds__(kBlock) void atx_kernel(const double* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                                     const double* __restrict__ mave,
                                                     const double* __restrict__ msig, CPtrs u, Ptrs out,
                                                     double scale, double tau, double gam2, CPtrs pv,
                                                     const int* __restrict__ gate, CPtrs zf,
                                                     const double* __restrict__ beta, Ptrs sraw) {
    atx_body<G, K, MODE, UJ, NT>(X, ld, N, M, mave, msig, u, out, scale, tau, gam2, pv, gate, zf, beta, sraw);
}

template <int G, int K, int MODE, int UJ, bool NT>
__global__ __launch_bounds__(kBlock) void atx_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                         int64_t M, const double* __restrict__ mave,
                                                         const double* __restrict__ msig, CPtrs u, Ptrs out,
                                                         double scale, double tau, double gam2, CPtrs pv,
                                                         const int* __restrict__ gate, CPtrs zf,
                                                         const double* __restrict__ beta, Ptrs sraw) {
    atx_body<G, K, MODE, UJ, NT>(X, ld, N, M, mave, msig, u, out, scale, tau, gam2, pv, gate, zf, beta, sraw);
}

template <int G, int K, int MODE, int UJ, bool NT>
__global__ __launch_bounds__(kBlock) void atx_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                         int64_t M, const double* __restrict__ mave,
                                                         const double* __restrict__ msig, CPtrs u, Ptrs out,
                                                         double scale, double tau, double gam2, CPtrs pv,
                                                         const int* __restrict__ gate, CPtrs zf,
                                                         const double* __restrict__ beta, Ptrs sraw) {
    atx_body<G, K, MODE, UJ, NT>(X, ld, N, M, mave, msig, u, out, scale, tau, gam2, pv, gate, zf, beta, sraw);
}

// tuning table (markers per wave G, 128-row steps per trip UJ, nontemporal)
struct AtxVariant { int G, UJ; bool NT; };
static constexpr AtxVariant kAtxVariants[] = {
    {4, 2, true}, {4, 2, false}, {2, 2, true}, {8, 2, true}, {4, 4, true}, {4, 1, true}, {8, 1, true}, {2, 4, true},
};
static constexpr int kNumAtxVariants = sizeof(kAtxVariants) / sizeof(kAtxVariants[0]);
// -1 (the default): per-K choice measured on MI355X at C2 (tools/kbench.py,
// profiles/r01_kbench.json): K=1 -> G=2,UJ=2 (6.86 TB/s); K>=2 -> G=4,UJ=4 (6.70 TB/s at K=2)
static int atx_variant_for(int variant, int K) { return variant >= 0 ? variant : (K == 1 ? 2 : 4); }

int atx_variant_count() { return kNumAtxVariants; }
bool atx_variant_ok(int v) { return v >= -1 && v < kNumAtxVariants; }

// rocprofv3 kernel name of the launch that ax_partial / atx would make now
std::string kernel_name(int which, int K, int mode, int variant, int ek) {
    char b[160];
    const char* sfx = xe_suffix(ek);
    if (which == 0) {
        const AxVariant& v = kAxVariants[variant >= 0 && variant < kNumAxVariants ? variant : 0];
        std::snprintf(b, sizeof b, "ax_partial_kernel%s<%d, %d, %d, %s, %s>", sfx, K, v.R, v.U,
                      v.NT ? "true" : "false", mode == 1 ? "true" : "false");
    } else {
        const AtxVariant& v = kAtxVariants[atx_variant_for(variant, K)];
        std::snprintf(b, sizeof b, "atx_kernel%s<%d, %d, %d, %d, %s>", sfx, v.G, K, mode, v.UJ,
                      v.NT ? "true" : "false");
    }
    return b;
}

int atx_blocks(int64_t M, int K, int variant) { return (int)cdiv(M, 4 * kAtxVariants[atx_variant_for(variant, K)].G); }

template <int G, int K, int MODE, int UJ, bool NT>
static void launch_atx(const Shard& s, CPtrs u, Ptrs out, double scale, double tau, double gam2, CPtrs p,
                       const int* gate, CPtrs zf, const double* beta, Ptrs sraw, hipStream_t st, const Timing& tm) {
    // two waves per workgroup: a finer dispatch grain than four (C2: -2..4%,
    // profiles/r01_kbench_ax_swap.txt); VAMPOMI_ATX_WPB: tuning experiments
    static const int wpb = std::getenv("VAMPOMI_ATX_WPB") ? std::max(1, std::min(4, std::atoi(std::getenv("VAMPOMI_ATX_WPB")))) : 2;
    launch_xe(s, atx_kernel<G, K, MODE, UJ, NT>, atx_kernel_f32<G, K, MODE, UJ, NT>, atx_kernel_u16<G, K, MODE, UJ, NT>,
              dim3((unsigned)cdiv(s.M, wpb * G)), dim3(64 * wpb), st, tm, s.N, s.M, s.mave, s.msig, u, out, scale, tau,
              gam2, p, gate, zf, beta, sraw);
}

template <int K, int MODE>
static bool launch_atx_v(int v, const Shard& s, CPtrs u, Ptrs out, double scale, double tau, double gam2, CPtrs p,
                         const int* gate, CPtrs zf, const double* beta, Ptrs sraw, hipStream_t st, const Timing& tm) {
    switch (v) {
        case 0: launch_atx<4, K, MODE, 2, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 1: launch_atx<4, K, MODE, 2, false>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 2: launch_atx<2, K, MODE, 2, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 3: launch_atx<8, K, MODE, 2, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 4: launch_atx<4, K, MODE, 4, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 5: launch_atx<4, K, MODE, 1, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 6: launch_atx<8, K, MODE, 1, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        case 7: launch_atx<2, K, MODE, 4, true>(s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); return true;
        default: return false;
    }
}

hipError_t atx(const Shard& s, int K, CPtrs u, Ptrs out, double scale, int mode, double tau, double gam2, CPtrs p,
               hipStream_t st, int variant, const Timing& tm, const int* gate, CPtrs zf, const double* beta,
               Ptrs sraw) {
    if (!atx_variant_ok(variant)) return hipErrorInvalidValue;
    const int v = atx_variant_for(variant, K);
    bool ok = false;
    if (mode == 0) {
        switch (K) {
            case 1: ok = launch_atx_v<1, 0>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            case 2: ok = launch_atx_v<2, 0>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            case 3: ok = launch_atx_v<3, 0>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            default: break;
        }
    } else {
        switch (K) {
            case 1: ok = launch_atx_v<1, 1>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            case 2: ok = launch_atx_v<2, 1>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            case 3: ok = launch_atx_v<3, 1>(v, s, u, out, scale, tau, gam2, p, gate, zf, beta, sraw, st, tm); break;
            default: break;
        }
    }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One-pass CG operator (kernels.h: atax).  A^T q (data::ATx,
// src/data.cpp:294-333, with the lmmse_mult epilogue src/vamp.cpp:656-659)
// and A d (data::Ax, src/data.cpp:340-373) from one read of X.
// ---------------------------------------------------------------------------
// One workgroup per CU (kOpWaves waves) owns whole columns: markers
// [b*M/grid, (b+1)*M/grid).  Wave w, lane l owns rows 1024*s + 128*w + 2l
// (+1), s < S = ceil(N/1024): every load instruction reads 1 KiB contiguous
// of one column.  Per marker i (a column of X in registers, the next one
// loading):
//   t_i = msig_i * sum_j (X_ij - mave_i) q_j * scale   (the wave partials
//         meet in LDS, one barrier; every wave sums them in wave order)
//   d_i = t_i*tau + gam2*p_i,  c_i = msig_i*d_i
//   acc_j += (X_ij - mave_i) * c_i                      (registers)
// q = A r/diag [+ beta*q_old] is formed once per launch into LDS (K*N
// doubles, each thread only ever reads its own rows: no barrier), so
// K*N <= kOpLdsDoubles.  The column is read from HBM once for both products;
// the workgroup's A d partial (K*N) goes to its slot, op_reduce sums the
// slots in order.  Summation orders are fixed, results bitwise reproducible.
static constexpr int kOpWaves = 8;               // 2 per SIMD: <= 256 VGPRs
static constexpr int kOpThreads = 64 * kOpWaves;
static constexpr int kOpRows = 128 * kOpWaves;   // rows per load step of the workgroup
static constexpr int kOpMaxS = 10;               // rows per workgroup <= kOpRows*kOpMaxS = 10,240
static constexpr int64_t kOpLdsDoubles = 20480 - 2 - 2 * kOpWaves * 2;  // the CU's 160 KiB of LDS

static bool whole_column_ok(int64_t N) {
    return N >= 1 && kOpMaxK * (N + 2) <= kOpLdsDoubles && (N + kOpRows - 1) / kOpRows <= kOpMaxS;
}

// The default: whole columns per workgroup (team size 1, the team kernel
// without a hand-off: 585 us against 646 us for atax_kernel at C2, K = 2,
// profiles/r02c_op_sweep.txt) while the rows fit one workgroup, else the
// smallest team whose members' rows fit the registers (configuration 7:
// 4 columns prefetched, a lag of 5 steps, polls 2 steps ahead, measured best
// at N = 50,000 and 100,000, profiles/r02c_op_sweep.txt; with the teams'
// columns interleaved, team t taking columns t, t + nteams, ..., so that all
// teams stream neighbouring columns instead of 8-16 ranges gigabytes apart:
// 10-13 % faster at the C3 shard, config 4 whole and 240 GB,
// profiles/r02i_op_interleave.txt).
bool op_plan(int64_t N, int64_t M, int cus, int variant, OpPlan* out) {
    if (N < 1 || cus < 1) return false;
    if (variant == kOpDefault) {
        // one workgroup per column range (team size 1): two columns prefetched
        // where they fit the registers (S <= 8), else one, up to S = 9; at
        // S = 10 (252-256 VGPRs) a team of 4 is faster (C2, N = 10,000, K = 2:
        // 585-588 against 597 us; N = 9,216, S = 9: 543 against 560 us for the
        // team; profiles/r02g_op_plans_by_N.txt)
        OpPlan p{};
        if ((team_plan(N, M, cus, 1, 1, &p) || team_plan(N, M, cus, 1, 0, &p)) && p.S <= 9) {
            *out = p;
            return true;
        }
    }
    if (variant == kOpDefault) {
        // just past one workgroup's rows (9,216 < N <= 10,752, C2 among them): a
        // team of 2 with six loads per lane (configuration 5, round 3's 12: F = 2, L = 3,
        // 253 VGPRs) beats the team of 4 (C2: 589.7-590.2 against 594.5-595.8 us
        // per launch in VAMP, 192.0-192.3 against 191.0-191.3 it/s, three rounds
        // on one box, profiles/r03pl_c2_plans.txt)
        OpPlan p{};
        if (team_plan(N, M, cus, 2, 5, &p)) {
            *out = p;
            return true;
        }
    }
    if (variant == 0) {
        if (!whole_column_ok(N)) return false;
        OpPlan p{};
        p.S = (int)std::max<int64_t>(1, (N + kOpRows - 1) / kOpRows);
        p.grid = (int)std::max<int64_t>(1, std::min<int64_t>(cus, M));
        p.nslots = p.grid;
        p.T = 0;
        *out = p;
        return true;
    }
    if (variant >= 1000) return team_plan(N, M, cus, (variant - 1000) / 100, variant % 100, out);  // 1000 + T*100 + cfg
    if (variant > 0) return team_plan(N, M, cus, variant / 10, variant % 10, out);
    for (int cfg : {2, 4}) {  // then fewer columns in flight for one more load per lane (S <= 5)
        for (int T = 2; T <= 32; T *= 2) {
            OpPlan p{};
            if (!team_plan(N, M, cus, T, cfg, &p)) continue;
            *out = p;
            return true;
        }
    }
    return false;  // N beyond 32 x 5 x 896 rows: the CG step keeps two passes (pcg.cpp)
}

bool op_supported(int64_t N, int K) {
    OpPlan p{};
    return K >= 1 && K <= kOpMaxK && op_plan(N, 1 << 20, 256, kOpDefault, &p);
}

// one column in registers: its X rows and the marker's mean
template <int K, int S, class XE = double>
struct OpCol {
    xpair_t<XE> x[S];  // as loaded (widened where it is used)
    double mu;
};

// (the body of atax_kernel, atax_kernel_f32 and atax_kernel_u16: XE is X's element type)
template <int K, int S, class XE>
__device__ __forceinline__ void atax_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                          const double* __restrict__ mave, const double* __restrict__ msig,
                                          const OpArgs& a, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    // LDS: q (K x NL; each thread only ever touches its own rows), a zero
    // pair, then 2 x kOpWaves x K dot partials
    extern __shared__ double q_lds[];
    const int NL = (int)N + 1 + ((int)N & 1);  // even stride; q[N] = 0 (the odd-N pad row)
    const int zslot = K * NL;
    double* s_part = q_lds + zslot + 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t mb = (int64_t)blockIdx.x * M / gridDim.x, me = (int64_t)(blockIdx.x + 1) * M / gridDim.x;
    // row of this thread in step s: jb + kOpRows*s (recomputed, not kept in registers)
    const int jb = 128 * wave + 2 * lane;
    const int n32 = (int)N;
#define OP_J(s) (jb + kOpRows * (s))
#define OP_OK(s) (OP_J(s) < n32)
    if (threadIdx.x == 0) {  // rows past N meet q = 0: the zero pair, and q[N] for odd N
        q_lds[zslot] = 0.0;
        q_lds[zslot + 1] = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) q_lds[k * NL + n32] = 0.0;
    }
    v2d acc[K][S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc[k][s] = v2d{0.0, 0.0};
            if (!OP_OK(s)) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int jj = OP_J(s) + h;
                if (jj < N) {
                    double q = a.ar.p[k][jj] / a.diag;              // A z = A r / diag
                    if ((a.fuse >> k) & 1) q = q + a.beta[k] * a.qo.p[k][jj];  // A p = A z + beta A p
                    q_lds[k * NL + jj] = q;
                }
            }
        }
    }
    __syncthreads();  // the zero pair and q[N] (thread 0) are read by other threads
    double bk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) bk[k] = ((a.fuse >> k) & 1) ? a.beta[k] : 0.0;
    double dpacc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dpacc[k] = 0.0;
    // columns in registers: three where they fit beside acc, else two
    constexpr int NB = K * S <= 16 ? 3 : 2;
    OpCol<K, S, XE> cb[NB];
    auto load = [&](OpCol<K, S, XE>& c, int64_t m) {
        const char* col = reinterpret_cast<const char*>(X + m * ld);
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (OP_OK(s))
                c.x[s] = ldx<true>(reinterpret_cast<const XE*>(col + (unsigned)(OP_J(s) * (int)sizeof(XE))));
        c.mu = mave[m];
    };
    // dot partials of column c -> s_part[par][wave][k]
    auto dots = [&](const OpCol<K, S, XE>& c, int par) {
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (!OP_OK(s)) continue;
            const double dx = widen(c.x[s]).x - c.mu, dy = widen(c.x[s]).y - c.mu;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const v2d q = *reinterpret_cast<const v2d*>(q_lds + k * NL + OP_J(s));  // q[N] = 0 for odd N
                v[k] += dx * q.x;
                v[k] += dy * q.y;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // the K butterflies interleaved: their exchanges fly together
            double t[K];
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] = __shfl_xor(v[k], o, 64);
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] += t[k];
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) s_part[(par * kOpWaves + wave) * K + k] = v[k];
        }
    };
    // the column's d (all waves, identically) and acc += (x - mave)*msig*d
    auto finish = [&](const OpCol<K, S, XE>& c, int64_t m, int par) {
        const double sg = msig[m];
        double cc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double dot = 0.0;
#pragma unroll
            for (int w = 0; w < kOpWaves; ++w) dot += s_part[(par * kOpWaves + w) * K + k];
            double t = sg * dot;  // sigma_inv * dpa
            t *= a.scale;         // ATx[mloc] *= 1/sqrt(N)
            double pk = a.p.p[k][m];
            if ((a.fuse >> k) & 1) pk = a.z.p[k][m] + bk[k] * pk;  // p = z + beta p
            double val = t * a.tau;  // res[i] *= tau
            val += a.gam2 * pk;      // res[i] += gam2 * v[i]
            if (threadIdx.x == 0) {
                if (a.sraw.p[0]) a.sraw.p[k][m] = t;
                a.d.p[k][m] = val;
            }
            dpacc[k] += val * pk;
            cc[k] = sg * val;  // Ax: (x - mave) * (msig * x_i)
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (!OP_OK(s)) continue;
            const double dx = widen(c.x[s]).x - c.mu, dy = widen(c.x[s]).y - c.mu;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[k][s].x += dx * cc[k];
                acc[k][s].y += dy * cc[k];
            }
        }
    };
    // NB columns in registers: m is finished while m+1 .. m+NB-1 load; the
    // buffer m frees takes m+NB.  Dot partials alternate between two LDS slots.
    auto step = [&](OpCol<K, S, XE>& cur, OpCol<K, S, XE>& nxt, int64_t m, int par) {
        finish(cur, m, par);
        if (m + NB < me) load(cur, m + NB);
        if (m + 1 < me) {
            dots(nxt, par ^ 1);
            __syncthreads();
        }
    };
    if (mb < me) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (mb + b < me) load(cb[b], mb + b);
        dots(cb[0], 0);
        __syncthreads();
        int par = 0;
        for (int64_t m = mb; m < me; m += NB) {
            step(cb[0], cb[1], m, par);
            par ^= 1;
            if constexpr (NB == 2) {
                if (m + 1 < me) {
                    step(cb[1], cb[0], m + 1, par);
                    par ^= 1;
                }
            } else {
                if (m + 1 < me) {
                    step(cb[1], cb[2 % NB], m + 1, par);
                    par ^= 1;
                }
                if (m + 2 < me) {
                    step(cb[2 % NB], cb[0], m + 2, par);
                    par ^= 1;
                }
            }
        }
    }
    // this workgroup's partial A d
    double* dst = a.part + (int64_t)blockIdx.x * kMaxRhs * ld;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (!OP_OK(s)) continue;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            dst[(int64_t)k * ld + OP_J(s)] = acc[k][s].x;
            if (OP_J(s) + 1 < n32) dst[(int64_t)k * ld + OP_J(s) + 1] = acc[k][s].y;
        }
    }
#undef OP_J
#undef OP_OK
    // <d_k, p_k>: this workgroup's sums over its markers in order (every
    // thread holds them), then the last workgroup adds them in block order
    const RedOut& ro = a.ro;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red_put(ro, (int64_t)blockIdx.x * K + k, dpacc[k]);
    }
    if (wave == 0) ticket_sum_blocks<K>(ro);
}

template <int K, int S>
__global__ __launch_bounds__(kOpThreads) void atax_kernel(const double* __restrict__ X, int64_t ld, int64_t N,
                                                          int64_t M, const double* __restrict__ mave,
                                                          const double* __restrict__ msig, OpArgs a,
                                                          const int* __restrict__ gate) {
    atax_body<K, S>(X, ld, N, M, mave, msig, a, gate);
}

template <int K, int S>
__global__ __launch_bounds__(kOpThreads) void atax_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                              int64_t M, const double* __restrict__ mave,
                                                              const double* __restrict__ msig, OpArgs a,
                                                              const int* __restrict__ gate) {
    atax_body<K, S>(X, ld, N, M, mave, msig, a, gate);
}

template <int K, int S>
__global__ __launch_bounds__(kOpThreads) void atax_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                              int64_t M, const double* __restrict__ mave,
                                                              const double* __restrict__ msig, OpArgs a,
                                                              const int* __restrict__ gate) {
    atax_body<K, S>(X, ld, N, M, mave, msig, a, gate);
}

std::string op_kernel_name(int K, const OpPlan& pl, int ek) {
    if (pl.T > 0) return team_kernel_name(K, pl, ek);
    char b[96];
    std::snprintf(b, sizeof b, "atax_kernel%s<%d, %d>", xe_suffix(ek), K, pl.S);
    return b;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize, bytes) for `kern` on the
// current device, once per (kernel, device): bit d of `done` is device d.  A
// failure is returned (and not left behind as the thread's last error, which
// the next launch's hipGetLastError would report as its own).
hipError_t lds_allow(const void* kern, std::atomic<unsigned long long>& done, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e;
    }
    done.fetch_or(bit, std::memory_order_acq_rel);
    return hipSuccess;
}

template <int K, int S>
static hipError_t launch_op(const Shard& s, const OpPlan& pl, const OpArgs& a, hipStream_t st, const Timing& tm,
                            const int* gate) {
    const size_t lds = ((size_t)K * (s.N + 1 + (s.N & 1)) + 2 + 2 * kOpWaves * K) * sizeof(double);
    static std::atomic<unsigned long long> allowed{0};  // more than 64 KiB of dynamic LDS must be allowed explicitly
    if (s.u16) {
        static std::atomic<unsigned long long> allowed16{0};
        if (const hipError_t e =
                lds_allow(reinterpret_cast<const void*>(&atax_kernel_u16<K, S>), allowed16, 160 * 1024))
            return e;
        hipExtLaunchKernelGGL((atax_kernel_u16<K, S>), dim3(pl.grid), dim3(kOpThreads), lds, st, tm.start, tm.stop, 0,
                              s.x16(), s.ld, s.N, s.M, s.mave, s.msig, a, gate);
        return hipSuccess;
    }
    if (s.f32) {
        static std::atomic<unsigned long long> allowed32{0};
        if (const hipError_t e =
                lds_allow(reinterpret_cast<const void*>(&atax_kernel_f32<K, S>), allowed32, 160 * 1024))
            return e;
        hipExtLaunchKernelGGL((atax_kernel_f32<K, S>), dim3(pl.grid), dim3(kOpThreads), lds, st, tm.start, tm.stop, 0,
                              s.x32(), s.ld, s.N, s.M, s.mave, s.msig, a, gate);
        return hipSuccess;
    }
    if (const hipError_t e = lds_allow(reinterpret_cast<const void*>(&atax_kernel<K, S>), allowed, 160 * 1024))
        return e;
    hipExtLaunchKernelGGL((atax_kernel<K, S>), dim3(pl.grid), dim3(kOpThreads), lds, st, tm.start, tm.stop, 0,
                          s.x64(), s.ld, s.N, s.M, s.mave, s.msig, a, gate);
    return hipSuccess;
}

template <int K>
static hipError_t launch_op_s(int S, const Shard& s, const OpPlan& pl, const OpArgs& a, hipStream_t st,
                              const Timing& tm, const int* gate) {
    switch (S) {
        case 1: return launch_op<K, 1>(s, pl, a, st, tm, gate);
        case 2: return launch_op<K, 2>(s, pl, a, st, tm, gate);
        case 3: return launch_op<K, 3>(s, pl, a, st, tm, gate);
        case 4: return launch_op<K, 4>(s, pl, a, st, tm, gate);
        case 5: return launch_op<K, 5>(s, pl, a, st, tm, gate);
        case 6: return launch_op<K, 6>(s, pl, a, st, tm, gate);
        case 7: return launch_op<K, 7>(s, pl, a, st, tm, gate);
        case 8: return launch_op<K, 8>(s, pl, a, st, tm, gate);
        case 9: return launch_op<K, 9>(s, pl, a, st, tm, gate);
        case 10: return launch_op<K, 10>(s, pl, a, st, tm, gate);
        default: return hipErrorInvalidValue;
    }
}

hipError_t atax(const Shard& s, const OpPlan& pl, int K, const OpArgs& a, hipStream_t st, const Timing& tm,
                const int* gate) {
    if (pl.T > 0) return atax_team(s, pl, K, a, st, tm, gate);
    if (K < 1 || K > kOpMaxK || !whole_column_ok(s.N) ||
        pl.S != (int)std::max<int64_t>(1, (s.N + kOpRows - 1) / kOpRows))
        return hipErrorInvalidValue;
    if (s.M <= 0) return hipSuccess;
    hipError_t e = hipErrorInvalidValue;
    switch (K) {
        case 1: e = launch_op_s<1>(pl.S, s, pl, a, st, tm, gate); break;
        case 2: e = launch_op_s<2>(pl.S, s, pl, a, st, tm, gate); break;
        default: break;
    }
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void op_reduce_kernel(int64_t N, int64_t ld, int nslots,
                                                        const double* __restrict__ part, Ptrs out, double div,
                                                        const int* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ v2d wsum[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tpk = (N + 127) / 128;
    const int k = (int)(blockIdx.x / tpk);
    const int64_t i = (blockIdx.x - k * tpk) * 128 + 2 * lane;  // < ld (a multiple of 16)
    const bool ok = i < N;
    wsum[w][lane] = ok ? slot_sum(part + (int64_t)k * ld + i, (int64_t)kMaxRhs * ld, w * nslots / 4,
                                  (w + 1) * nslots / 4)
                       : v2d{0.0, 0.0};
    __syncthreads();
    if (w != 0 || !ok) return;
    v2d r = ((wsum[0][lane] + wsum[1][lane]) + wsum[2][lane]) + wsum[3][lane];
    if (div > 0) r /= div;
    out.p[k][i] = r.x;
    if (i + 1 < N) out.p[k][i + 1] = r.y;
}

hipError_t op_reduce(const OpPlan& pl, int K, int64_t N, int64_t ld, const double* part, Ptrs out, double div,
                     hipStream_t st, const int* gate, int k0) {
    const int64_t n = (int64_t)K * N;
    if (n <= 0) return hipSuccess;
    if (k0 < 0 || k0 + K > kMaxRhs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(op_reduce_kernel, dim3((unsigned)(K * cdiv(N, 128))), dim3(256), 0, st, N, ld, (int)pl.nslots,
                       part + (int64_t)k0 * ld, out, div, gate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// marker statistics (src/data.cpp:233-283): one wave per marker, two passes
// ---------------------------------------------------------------------------
// (the body of stats_kernel, stats_kernel_f32 and stats_kernel_u16: the statistics of the stored
// values, widened, summed in fp64)
template <class XE>
__device__ __forceinline__ void stats_body(const XE* __restrict__ X, int64_t ld, int64_t N, int64_t M, double nonas,
                                           double alpha_scale, double* __restrict__ mave,
                                           double* __restrict__ msig) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * 4 + wave;
    if (m >= M) return;
    const XE* col = X + m * ld;
    double s = 0.0;
    for (int64_t j = 2 * lane; j < N; j += 128) {
        const v2d x = widen(ldx<false>(col + j));
        s += x.x;
        if (j + 1 < N) s += x.y;
    }
    s = wave_sum(s);
    const double mean = s / nonas;
    double q = 0.0;
    for (int64_t j = 2 * lane; j < N; j += 128) {
        const v2d x = widen(ldx<false>(col + j));
        const double a = x.x - mean;
        q += a * a;
        if (j + 1 < N) {
            const double b = x.y - mean;
            q += b * b;
        }
    }
    q = wave_sum(q);
    if (lane == 0) {
        mave[m] = mean;
        double sg;
        if (q != 0.0) {
            if (alpha_scale == 1.0)
                sg = 1.0 / sqrt(q / (nonas - 1.0));
            else
                sg = 1.0 / pow(sqrt(q / (nonas - 1.0)), alpha_scale);
        } else {
            sg = 1.0;
        }
        msig[m] = sg;
    }
}

__global__ __launch_bounds__(kBlock) void stats_kernel(const double* __restrict__ X, int64_t ld, int64_t N, int64_t M,
                                                       double nonas, double alpha_scale, double* __restrict__ mave,
                                                       double* __restrict__ msig) {
    stats_body(X, ld, N, M, nonas, alpha_scale, mave, msig);
}

__global__ __launch_bounds__(kBlock) void stats_kernel_f32(const float* __restrict__ X, int64_t ld, int64_t N,
                                                           int64_t M, double nonas, double alpha_scale,
                                                           double* __restrict__ mave, double* __restrict__ msig) {
    stats_body(X, ld, N, M, nonas, alpha_scale, mave, msig);
}

__global__ __launch_bounds__(kBlock) void stats_kernel_u16(const uint16_t* __restrict__ X, int64_t ld, int64_t N,
                                                           int64_t M, double nonas, double alpha_scale,
                                                           double* __restrict__ mave, double* __restrict__ msig) {
    stats_body(X, ld, N, M, nonas, alpha_scale, mave, msig);
}

hipError_t marker_stats(const Shard& s, double nonas, double alpha_scale, double* mave, double* msig,
                        hipStream_t st) {
    if (s.M <= 0) return hipSuccess;
    launch_xe(s, stats_kernel, stats_kernel_f32, stats_kernel_u16, dim3((unsigned)cdiv(s.M, 4)), dim3(kBlock), st,
              Timing{}, s.N, s.M, nonas, alpha_scale, mave, msig);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// synthetic data
// ---------------------------------------------------------------------------
__device__ __forceinline__ double meth_dyadic(uint64_t seed, int64_t i, int64_t j) {
    const uint64_t hm = splitmix64(splitmix64(seed ^ 0x6D657468ULL) + (uint64_t)i);
    const double mu = (double)(51 + (hm & 1023ULL) % 922ULL) * (1.0 / 1024.0);
    const double sd = (double)(10 + ((hm >> 10) & 127ULL)) * (1.0 / 1024.0);
    const double v = mu + sd * gauss_dyadic(seed ^ 0x5A5A5A5AULL, i, j);
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

// (XE = float: the generator's value rounded to nearest even, as an ingest of
// the fp64 matrix would store it)
template <class XE>
__device__ __forceinline__ void gen_body(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M,
                                         XE* X) {
    const int64_t total = M * ld;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / ld, j = e - i * ld;
        double v = 0.0;
        if (j < N) v = kind == 1 ? meth_dyadic(seed, S + i, j) : gauss_dyadic(seed, S + i, j);
        X[e] = (XE)v;
    }
}

__global__ void gen_kernel(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M, double* X) {
    gen_body(seed, kind, N, ld, S, M, X);
}

__global__ void gen_kernel_f32(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M, float* X) {
    gen_body(seed, kind, N, ld, S, M, X);
}

hipError_t gen_markers(uint64_t seed, int kind, int64_t N, int64_t ld, int64_t S, int64_t M, void* X, int ek,
                       hipStream_t st) {
    int64_t blocks = cdiv(M * ld, kBlock);
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) return hipSuccess;
    if (ek == kXU16) return hipErrorInvalidValue;  // quantised from staged fp64 chunks by the engine
    if (ek == kXF32)
        hipLaunchKernelGGL(gen_kernel_f32, dim3((unsigned)blocks), dim3(kBlock), 0, st, seed, kind, N, ld, S, M,
                           static_cast<float*>(X));
    else
        hipLaunchKernelGGL(gen_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, seed, kind, N, ld, S, M,
                           static_cast<double*>(X));
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void gen_beta_kernel(uint64_t seed, double lam, int64_t S, int64_t M,
                                                          double* beta, RedOut ro) {
    __shared__ double lds[4];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double c = 0.0;
    if (i < M) {
        const uint64_t h = splitmix64(splitmix64(seed ^ 0x63617573ULL) + (uint64_t)(S + i));
        const double uni = (double)(h >> 11) * (1.0 / 9007199254740992.0);
        const bool causal = uni < lam;
        beta[i] = causal ? gauss_dyadic(seed ^ 0x62657461ULL, S + i, 0) : 0.0;
        c = causal ? 1.0 : 0.0;
    }
    c = block_sum(c, lds);
    if (threadIdx.x == 0) red_put(ro, blockIdx.x, c);
    red_finish(ro, 1, lds);
}

hipError_t gen_beta(uint64_t seed, double lam, int64_t S, int64_t M, double* beta, const RedOut& ro, hipStream_t st) {
    const int nblk = (int)std::max<int64_t>(1, cdiv(M, kBlock));
    hipLaunchKernelGGL(gen_beta_kernel, dim3(nblk), dim3(kBlock), 0, st, seed, lam, S, M, beta, ro);
    return hipGetLastError();
}

__global__ void noise_kernel(uint64_t seed, int64_t N, double sd, double* y) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < N) y[j] = y[j] + sd * gauss_dyadic(seed ^ 0x6E6F697365ULL, -1, j);
}

hipError_t add_noise(uint64_t seed, int64_t N, double sd, double* y, hipStream_t st) {
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)cdiv(N, kBlock)), dim3(kBlock), 0, st, seed, N, sd, y);
    return hipGetLastError();
}

}  // namespace vk
