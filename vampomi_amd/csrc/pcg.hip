// pcg.hip — gfx950 kernels of the PCG vector steps: the start of a solve
// (cg_init_kernel; prelude_cg_init_kernel with the iteration's prelude in the
// same launch), the device-side CgState (cg_start_kernel,
// cg_start_from_kernel), the step's decision on its own (cg_decide_kernel),
// the step itself (cg_update_kernel) and the pre-step composed without a pass
// (pre_compose_kernel).  None of them reads X.  Launched only by pcg.cpp; the
// CG section of kernels.h (CgVecs, CgState, CgDecide, PreCompose) is the
// interface between the two.
#include "kernels.h"
#include "kdev.h"

#include <algorithm>
#include <cstdlib>

namespace vk {

// ---------------------------------------------------------------------------
// PCG vector steps (src/vamp.cpp:671-757), K right-hand sides per launch
// ---------------------------------------------------------------------------
// System k's start at marker i (cg_init_kernel, prelude_cg_init_kernel):
// r = v - lmmse_mult(mu0) in the form the system has (c.atx0[k]: from the
// precomputed A^T(A mu0), res *= tau; res += gam2 * mu0; else c.d[k]: from the
// start's own pass; else a zero start), z = r / diag, p = z, and the terms of
// <r,z> and <v,v>.  vi, atx0, mu, d: the loaded values (those of another form
// are not read); tau, gam2, diag: c's and the launch's, or the device's.
__device__ __forceinline__ void cg_start_at(const CgVecs& c, int k, int64_t i, double vi, double atx0, double mu,
                                            double d, double tau, double gam2, double diag, double& rz, double& vv) {
    double r;
    if (c.atx0[k]) {
        double dv = atx0;
        dv *= tau;
        dv += gam2 * mu;
        r = vi - dv;
    } else {
        r = c.d[k] ? vi - d : vi - 0.0;
    }
    const double z = r / diag;
    c.r[k][i] = r;
    c.z[k][i] = z;
    c.p[k][i] = z;
    rz += r * z;
    vv += vi * vi;
}

__global__ __launch_bounds__(kBlock) void cg_init_kernel(int K, int64_t M, CgVecs c, double diag, RedOut ro) {
    __shared__ double lds[4];
    double acc[2 * kMaxRhs];
#pragma unroll
    for (int q = 0; q < 2 * kMaxRhs; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int k = 0; k < kMaxRhs; ++k) {
            if (k < K) {
                const double vi = c.v[k][i];
                const double a0 = c.atx0[k] ? c.atx0[k][i] : 0.0;
                const double mu = c.atx0[k] ? c.mu[k][i] : 0.0;
                const double d = !c.atx0[k] && c.d[k] ? c.d[k][i] : 0.0;
                cg_start_at(c, k, i, vi, a0, mu, d, c.tau, c.gam2, diag, acc[2 * k], acc[2 * k + 1]);
            }
        }
    }
    block_put_sums<2 * kMaxRhs>(acc, 2 * K, ro, (int64_t)blockIdx.x * 2 * K);
    red_finish(ro, 2 * K, lds);
}

// prelude_kernel's and cg_init_kernel's work in one launch, on cg_init's grid
// (prelude_at and cg_start_at, the bodies of both: the same sums, in the same
// order); v_k that the prelude forms (v, bern) is used from registers.  Two elements per round (i, i + stride), all of both
// elements' loads issued before either is used; the sums still run over i,
// i + stride, ... in order.  start: the last block builds the CgState
// (cg_start_from)
__global__ __launch_bounds__(kBlock) void prelude_cg_init_kernel(int K, int64_t M, Prelude p, CgVecs c, double diag,
                                                                 RedOut ro, CgState start, CgState* dst) {
    __shared__ double lds[4];
    __shared__ double fin[2 * kMaxRhs];
    double eta1 = p.eta1, gam1 = p.gam1, gam2 = p.gam2, gamw = p.gamw, tau = c.tau, cgam2 = c.gam2;
    if (p.dev.scal) {  // the scalars from the device (kernels.h PreDev, formed by the denoiser's launch)
        const double* q = p.dev.scal;
        eta1 = q[0];
        gam2 = cgam2 = q[1];
        gamw = tau = q[2];
        diag = q[3];
        gam1 = q[4];
    }
    double acc[2 * kMaxRhs];
#pragma unroll
    for (int q = 0; q < 2 * kMaxRhs; ++q) acc[q] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < M; i0 += 2 * stride) {
        const bool two = i0 + stride < M;
        double x1v[2], r1v[2], ayv[2], vo[2][kMaxRhs], a0[2][kMaxRhs], muv[2][kMaxRhs], dd[2][kMaxRhs];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t i = i0 + h * stride;
            if (h == 1 && !two) break;
            x1v[h] = p.x1[i];
            r1v[h] = p.r1[i];
            ayv[h] = p.atxy[i];
#pragma unroll
            for (int k = 0; k < kMaxRhs; ++k) {
                if (k >= K) continue;
                vo[h][k] = c.v[k] == p.v || c.v[k] == p.bern ? 0.0 : c.v[k][i];
                a0[h][k] = c.atx0[k] ? c.atx0[k][i] : 0.0;
                muv[h][k] = c.atx0[k] ? c.mu[k][i] : 0.0;
                dd[h][k] = !c.atx0[k] && c.d[k] ? c.d[k][i] : 0.0;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t i = i0 + h * stride;
            if (h == 1 && !two) break;
            double vv, bn;
            prelude_at(p, i, x1v[h], r1v[h], ayv[h], eta1, gam1, gam2, gamw, vv, bn);
#pragma unroll
            for (int k = 0; k < kMaxRhs; ++k) {
                if (k >= K) continue;
                const double vi = c.v[k] == p.v ? vv : c.v[k] == p.bern ? bn : vo[h][k];
                cg_start_at(c, k, i, vi, a0[h][k], muv[h][k], dd[h][k], tau, cgam2, diag, acc[2 * k], acc[2 * k + 1]);
            }
        }
    }
    block_put_sums<2 * kMaxRhs>(acc, 2 * K, ro, (int64_t)blockIdx.x * 2 * K);
    if (red_finish(ro, 2 * K, lds, fin) && dst && threadIdx.x == 0) {
        *dst = start;  // then its sums (indexed in place: no stack copy of the state)
        dst->gam2 = cgam2;
        for (int k = 0; k < K; ++k) {
            dst->rz[k] = fin[2 * k];
            dst->vv[k] = fin[2 * k + 1];
        }
    }
}

hipError_t prelude_cg_init(int K, int64_t M, const Prelude& p, const CgVecs& c, double diag, const RedOut& ro,
                           const CgState* start, CgState* dst, hipStream_t st) {
    hipLaunchKernelGGL(prelude_cg_init_kernel, dim3(red_blocks(M)), dim3(kBlock), 0, st, K, M, p, c, diag, ro,
                       start ? *start : CgState{}, start ? dst : nullptr);
    return hipGetLastError();
}

hipError_t cg_init(int K, int64_t M, const CgVecs& c, double diag, const RedOut& ro, hipStream_t st) {
    hipLaunchKernelGGL(cg_init_kernel, dim3(red_blocks(M)), dim3(kBlock), 0, st, K, M, c, diag, ro);
    return hipGetLastError();
}

__global__ void cg_start_kernel(CgState init, CgState* dst) {
    if (threadIdx.x == 0) *dst = init;
}

hipError_t cg_start(const CgState& init, CgState* dst, hipStream_t st) {
    hipLaunchKernelGGL(cg_start_kernel, dim3(1), dim3(64), 0, st, init, dst);
    return hipGetLastError();
}

__global__ void cg_start_from_kernel(CgState init, const double* __restrict__ sums, CgState* dst,
                                     const double* __restrict__ gam2dev) {
    if (threadIdx.x != 0) return;
    for (int k = 0; k < init.K; ++k) {
        init.rz[k] = sums[2 * k];
        init.vv[k] = sums[2 * k + 1];
    }
    if (gam2dev) init.gam2 = gam2dev[0];
    *dst = init;
}

hipError_t cg_start_from(const CgState& init, const double* sums, CgState* dst, hipStream_t st,
                         const double* gam2dev) {
    hipLaunchKernelGGL(cg_start_from_kernel, dim3(1), dim3(64), 0, st, init, sums, dst, gam2dev);
    return hipGetLastError();
}

__global__ void cg_decide_kernel(CgState* cs, const double* __restrict__ red, int it, CgMirror* mirror,
                                 unsigned long long* flag, unsigned long long seq, int mask, int pack) {
    if (threadIdx.x == 0) cg_decide_body(cs, red, it, mirror, flag, seq, mask, pack);
}

// Latency, not bytes, sets this kernel's time at C2 (~25 MB in ~16 us): a
// chain of dependent memory round trips.  So every scalar comes in one burst
// (the whole CgState: the deciding block needs no further state load), both
// M-elements of a thread and a tile's N-vectors are loaded before the
// dependent work, and the decision takes its sums from LDS.  One
// instantiation per system count K: the unrolled per-system loops then carry
// K systems, not kMaxRhs (at K = 2: a quarter of the live registers, no
// spills, and only the K systems' vector pointers loaded from the arguments);
// every per-element operation and every sum is the same, in the same order.
// CGU_ABL (experiment builds only, results wrong; tools/cgu_ablation.sh):
// 1 = no slot sums / N-side updates, 2 = no M-side loads / stores, 4 = no
// decision, 8 = no last-block sums (nor decision), 16 = no partials and no
// ticket, 32 = a constant state instead of *cs and <d,p>
#ifndef CGU_ABL
#define CGU_ABL 0
#endif
template <int K, int W>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(int64_t M, CgVecs c, double diag,
                                                           CgState* cs, const double* __restrict__ dp_dev,
                                                           const double* __restrict__ pp_dev, int fuse, RedOut ro,
                                                           CgDecide dc, int mblocks) {
#if CGU_ABL & 32
    CgState st{};
    st.K = K;
    st.any = 1;
    for (int k = 0; k < K; ++k) {
        st.active[k] = 1;
        st.rz[k] = st.vv[k] = 1.0;
    }
    double dpv[K], ppv[K];
    for (int k = 0; k < K; ++k) dpv[k] = 1.0, ppv[k] = 0.0;
#else
    const CgState st = *cs;
    double dpv[K], ppv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        dpv[k] = dp_dev[k];
        ppv[k] = pp_dev ? pp_dev[k] : 0.0;
    }
#endif
    if (!st.any) return;
    // the pre-step (kernels.h OpAlt): the slot the step's operator launch ran on
    // the alternate system, by the same rule from the same state (-1: none)
    const int pre = c.pre_u1 ? cg_pre_slot(st.active, K, *c.pre_done == c.pre_token) : -1;
    __shared__ double fin[3 * kMaxRhs];  // the step's final sums, for the deciding thread
    // blocks [0, mblocks) stream the M-vectors; with c.adpart the blocks past
    // them sum the operator's A d partials and update the N-vectors
    const bool mpart = (int)blockIdx.x < mblocks;
    double alpha[K];
    bool on[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        on[k] = st.active[k] && ((dc.mask >> k) & 1);
        const double dp = pp_dev ? c.tau * dpv[k] + c.gam2 * ppv[k] : dpv[k];  // <d,p>
        alpha[k] = on[k] ? st.rz[k] / dp : 0.0;  // :702
    }
    double acc[3 * K];
#pragma unroll
    for (int q = 0; q < 3 * K; ++q) acc[q] = 0.0;
    double beta[K];
    bool fk[K];  // system k's direction update p = z + beta p rides in this step
#pragma unroll
    for (int k = 0; k < K; ++k) {
        fk[k] = on[k] && ((fuse >> k) & 1);
        beta[k] = fk[k] ? st.beta[k] : 0.0;
    }
    // two elements per round (i, i + stride), both loaded before either is
    // stored (the vectors may alias as far as the compiler knows: loads after
    // a store would wait for it); the sums still run over i, i + stride, ...
    // in order, as one element per round would
    const int64_t mstride = (int64_t)mblocks * kBlock;
    // (W < 32, the large-N plans: one element per round, fewer registers and
    // more workgroups per CU; the same sums in the same order)
    constexpr int H = W >= 32 || K >= 3 ? 2 : 1;  // (K >= 3 keeps two: one would spill to scratch)
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; mpart && !(CGU_ABL & 2) && i0 < M;
         i0 += H * mstride) {
        double pv[H][K], zv[H][K], muv[H][K], rv[H][K], dv[H][K], vv[H][K], wv[H][K], sv[H][K];
        const bool two = H == 2 && i0 + mstride < M;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int64_t i = i0 + h * mstride;
            if (h == 1 && !two) break;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (on[k]) {
                    pv[h][k] = c.p[k][i];
                    zv[h][k] = fk[k] ? c.z[k][i] : 0.0;
                    muv[h][k] = c.mu[k][i];
                    rv[h][k] = c.r[k][i];
                    dv[h][k] = c.d[k][i];
                    vv[h][k] = c.v[k][i];
                    wv[h][k] = c.W[k] ? c.W[k][i] : 0.0;
                    sv[h][k] = c.W[k] ? c.S[k][i] : 0.0;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int64_t i = i0 + h * mstride;
            if (h == 1 && !two) break;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (on[k]) {
                    double pi = pv[h][k];
                    if (fk[k]) {  // p = z + beta p (:738-739)
                        pi = zv[h][k] + beta[k] * pi;
                        c.p[k][i] = pi;
                    }
                    const double mu = muv[h][k] + alpha[k] * pi;  // mu += alpha * p
                    const double r = rv[h][k] - dv[h][k] * alpha[k];  // r -= d * alpha
                    const double z = r / diag;
                    c.mu[k][i] = mu;
                    c.r[k][i] = r;
                    c.z[k][i] = z;
                    if (c.W[k]) c.W[k][i] = wv[h][k] + alpha[k] * sv[h][k];  // A^T A mu, as mu += alpha p
                    acc[3 * k] += r * z;
                    acc[3 * k + 1] += r * r;
                    acc[3 * k + 2] += vv[h][k] * mu;
                }
            }
        }
    }
    // A mu alongside mu (replicated N-vectors, the same on every rank)
    if (c.adpart) {
        // one rank, one-pass operator: A d from the operator's slots, in
        // op_reduce's order (tiles of 128 samples of one system)
        __shared__ v2d wsum[4][64];
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ns = c.adslots;
        const int nb = (int)gridDim.x - mblocks;
        const int64_t tpk = (c.nA + 127) / 128;  // tiles per system
        for (int64_t tile = (int)blockIdx.x - mblocks; !(CGU_ABL & 1) && !mpart && tile < K * tpk; tile += nb) {
            const int k = (int)(tile / tpk);
            const int64_t i = (tile - k * tpk) * 128 + 2 * lane;  // < adld (a multiple of 16)
            const bool ok = i < c.nA;
            bool onk = false, fuk = false;  // on[k], fk[k], alpha[k], beta[k] without indexing registers at run time
            double alk = 0.0, bek = 0.0;
#pragma unroll
            for (int kk = 0; kk < (K < kOpMaxK ? K : kOpMaxK); ++kk)
                if (kk == k) {
                    onk = on[kk];
                    fuk = fk[kk];
                    alk = alpha[kk];
                    bek = beta[kk];
                }
            // wave 0's N-vectors of the tile, loaded before the slot sums (pairs
            // of samples: i + 1 < adld, the pads lie inside the vectors)
            const bool upd = w == 0 && ok && onk;
            v2d arv{0.0, 0.0}, qov{0.0, 0.0}, awv{0.0, 0.0};
            if (upd) {
                arv = *reinterpret_cast<const v2d*>(c.AR[k] + i);
                if (fuk) qov = *reinterpret_cast<const v2d*>(c.Q[k] + i);
                if (c.AW[k]) awv = *reinterpret_cast<const v2d*>(c.AW[k] + i);
            }
            wsum[w][lane] = ok ? slot_sum<W>(c.adpart + (int64_t)k * c.adld + i, (int64_t)kMaxRhs * c.adld,
                                             w * ns / 4, (w + 1) * ns / 4)
                               : v2d{0.0, 0.0};
            __syncthreads();
            if (upd) {
                const v2d ad = (((wsum[0][lane] + wsum[1][lane]) + wsum[2][lane]) + wsum[3][lane]) / c.addiv;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t j = i + e;
                    if (j >= c.nA) break;
                    double q = arv[e] / diag;
                    if (fuk) q = q + bek * qov[e];
                    c.Q[k][j] = q;
                    if (c.AW[k]) c.AW[k][j] = awv[e] + alk * q;
                    c.AR[k][j] = arv[e] - ad[e] * alk;
                }
            } else if (w == 0 && ok && k == pre) {  // the alternate system's A d: the same sum, into U1
                const v2d ad = (((wsum[0][lane] + wsum[1][lane]) + wsum[2][lane]) + wsum[3][lane]) / c.addiv;
                c.pre_u1[i] = ad[0];
                if (i + 1 < c.nA) c.pre_u1[i + 1] = ad[1];
            }
            __syncthreads();
        }
    } else if (c.Q[0]) {  // one-pass operator: q (the step's A p) from A r, then A r -= A d * alpha
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < c.nA; i += (int64_t)gridDim.x * kBlock) {
            double ar[K], qo[K], ad[K], aw[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
                    ar[k] = c.AR[k][i];
                    qo[k] = fk[k] ? c.Q[k][i] : 0.0;
                    ad[k] = c.addiv > 0 ? c.AD[k][i] / c.addiv : c.AD[k][i];  // (vec_div's division)
                    aw[k] = c.AW[k] ? c.AW[k][i] : 0.0;
                }
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
                    double q = ar[k] / diag;  // A z = A r / diag
                    if (fk[k]) q = q + beta[k] * qo[k];  // A p = A z + beta A p
                    c.Q[k][i] = q;
                    if (c.AW[k]) c.AW[k][i] = aw[k] + alpha[k] * q;
                    c.AR[k][i] = ar[k] - ad[k] * alpha[k];
                }
        }
    } else
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < c.nA; i += (int64_t)gridDim.x * kBlock) {
        double aw[K], as[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k] && c.AW[k]) {
                aw[k] = c.AW[k][i];
                as[k] = c.AS[k][i];
            }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k] && c.AW[k]) c.AW[k][i] = aw[k] + alpha[k] * as[k];
    }
    // The M-side blocks publish their sums.  The slot-sum blocks' sums are
    // zero: they publish none, and the last block adds the first mblocks
    // blocks' partials (the same partials in the same order, without the
    // zeros: the same bits).  Every block still takes the ticket, so that the
    // decision below, which rewrites *cs, follows every block's read of the
    // state; a slot-sum block takes it without waiting for its vector stores
    // (the decision reads none of them; the next launch sees them after the
    // kernel boundary).
    bool last = false;
    if (CGU_ABL & 16) {
    } else if (mpart) {
        block_put_sums<3 * K>(acc, 3 * K, ro, (int64_t)blockIdx.x * 3 * K);
        last = red_ticket(ro, (int)gridDim.x);
    } else {
        last = red_ticket_nowait(ro, (int)gridDim.x);
    }
    if (last && !(CGU_ABL & 8)) red_final(ro, 3 * K, mblocks, fin, true);
    // one rank: the last block decides the step itself (its sums are final),
    // from the state read at the start (only this decision writes it)
    if (last && dc.on && threadIdx.x == 0 && !(CGU_ABL & 12)) {
        double r[3 * kMaxRhs];
#pragma unroll
        for (int q = 0; q < 3 * kMaxRhs; ++q) r[q] = q < 3 * K ? fin[q] : 0.0;
        cg_decide_from(st, cs, r, dc.it, dc.mirror, dc.flag, dc.seq, dc.mask, dc.pack, pre >= 0);
    }
    // (every block read the done word before it took the ticket)
    if (last && pre >= 0 && threadIdx.x == 0) *c.pre_done = c.pre_token;
}

// cg_update_kernel<K, W> of the system count's instantiation (wide: W = 32)
template <int K, class... A>
static void launch_cgu(bool wide, int blocks, hipStream_t st, A... args) {
    if (wide)
        hipLaunchKernelGGL((cg_update_kernel<K, 32>), dim3(blocks), dim3(kBlock), 0, st, args...);
    else
        hipLaunchKernelGGL((cg_update_kernel<K, 8>), dim3(blocks), dim3(kBlock), 0, st, args...);
}

constexpr int kCguBlocks = 512;
hipError_t cg_update(int K, int64_t M, const CgVecs& c, double diag, CgState* cs, const double* dp_dev,
                     const double* pp_dev, int fuse, const RedOut& ro, const CgDecide& dc, hipStream_t st) {
    // VAMPOMI_CG_EPT: M elements per thread (tuning experiments; default 2, red_blocks)
    static const int ept = std::getenv("VAMPOMI_CG_EPT") ? std::max(1, std::atoi(std::getenv("VAMPOMI_CG_EPT"))) : 2;
    const int mb = (int)std::min<int64_t>(std::max<int64_t>(cdiv(M, (int64_t)kBlock * ept), 1), kRedBlocks / 2);
    int nb = 0;
    if (c.adpart) {
        if (K > kOpMaxK || c.adslots < 1 || !c.Q[0]) return hipErrorInvalidValue;
        // at most kCguBlocks workgroups in all (two per CU): every one takes the
        // step's ticket, and beyond that their arrivals cost more than the tiles
        // they share (C4 shard, 782 slot-sum workgroups: 164.8 -> 127.4 us of
        // cg_update per iteration at 400, 142.0 at 158; C2's 158 is best at C2,
        // profiles/r06n_cgu_blocks.txt).  Each workgroup takes tiles nb apart,
        // the same tiles summed the same way: bitwise the same for any nb.
        // VAMPOMI_CGU_NB: the count itself (tuning experiments)
        static const int nbset = std::getenv("VAMPOMI_CGU_NB") ? std::atoi(std::getenv("VAMPOMI_CGU_NB")) : 0;
        nb = (int)std::min<int64_t>(K * cdiv(c.nA, 128), nbset > 0 ? nbset : std::max(kCguBlocks - mb, 1));
        nb = std::max(std::min(nb, kRedBlocks - mb), 1);
    }
    // the 32-load slot rounds only where a wave sums >= 32 slots (C2's team of
    // 2); else rounds of <= 8 loads and the registers of more workgroups per CU
    const bool wide = c.adpart && c.adslots >= 4 * 32;
    switch (K) {
        case 1: launch_cgu<1>(wide, mb + nb, st, M, c, diag, cs, dp_dev, pp_dev, fuse, ro, dc, mb); break;
        case 2: launch_cgu<2>(wide, mb + nb, st, M, c, diag, cs, dp_dev, pp_dev, fuse, ro, dc, mb); break;
        case 3: launch_cgu<3>(wide, mb + nb, st, M, c, diag, cs, dp_dev, pp_dev, fuse, ro, dc, mb); break;
        case 4: launch_cgu<4>(wide, mb + nb, st, M, c, diag, cs, dp_dev, pp_dev, fuse, ro, dc, mb); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t cg_decide(CgState* cs, const double* red, int it, CgMirror* mirror, unsigned long long* flag,
                     unsigned long long seq, hipStream_t st, int mask, int pack) {
    hipLaunchKernelGGL(cg_decide_kernel, dim3(1), dim3(64), 0, st, cs, red, it, mirror, flag, seq, mask, pack);
    return hipGetLastError();
}

// The pre-step's first CG step without a pass (kernels.h PreCompose).  The
// expression order (no contraction: the file is built with -ffp-contract=off):
//   t  = T1_i / diag                      (A^T A p, p = b/diag)
//   d  = t * tau;  d += gam2 * p_i        (the lmmse_mult epilogue's two steps)
//   S  = t
//   AD = (tau * U1_j + gam2 * ab_j) / diag
// <d,p>: per-block sums over i, i + stride, ... in order, then the blocks in
// order (red_finish), as every reduction here
__global__ __launch_bounds__(kBlock) void pre_compose_kernel(int64_t M, int64_t N, PreCompose a, RedOut ro) {
    if (ro.gate && !*ro.gate) return;
    __shared__ double lds[4];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += stride) {
        const double t = a.T1[i] / a.diag;
        const double p = a.p[i];
        double d = t * a.tau;
        d += a.gam2 * p;
        a.d[i] = d;
        if (a.S) a.S[i] = t;
        acc[0] += d * p;
    }
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride) {
        double u = a.tau * a.U1[j];
        u += a.gam2 * a.ab[j];
        a.AD[j] = u / a.diag;
    }
    if (a.rz_save && blockIdx.x == 0 && threadIdx.x == 0) a.rz_save[0] = a.cs->rz[0];
    block_put_sums<1>(acc, 1, ro, (int64_t)blockIdx.x);
    red_finish(ro, 1, lds);
}

// The second composed step (kernels.h PreCompose2), every expression in the
// order written there (no contraction).  The sums as pre_compose's
__global__ __launch_bounds__(kBlock) void pre_compose2_kernel(int64_t M, int64_t N, PreCompose2 a, RedOut ro) {
    if (ro.gate && !*ro.gate) return;
    if (!a.cs->active[0]) return;  // the solve stopped inside its composed steps (uniform over the grid)
    __shared__ double lds[4];
    const double alpha0 = a.rz_save[0] / a.dp0[0];
    const double beta0 = a.cs->beta[0];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += stride) {
        const double t1 = a.T1[i];
        double w = a.tau * a.T2[i];
        w += a.gam2 * t1;
        w = w / a.diag;
        double s = (t1 - alpha0 * w) / a.diag;
        s = s + beta0 * (t1 / a.diag);
        const double p1 = a.z[i] + beta0 * a.p[i];
        double d = s * a.tau;
        d += a.gam2 * p1;
        a.d[i] = d;
        if (a.S) a.S[i] = s;
        acc[0] += d * p1;
    }
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride) {
        const double u1 = a.U1[j];
        double w = a.tau * a.U2[j];
        w += a.gam2 * u1;
        w = w / a.diag;
        double s = (u1 - alpha0 * w) / a.diag;
        s = s + beta0 * (u1 / a.diag);
        double q1 = a.ar[j] / a.diag;
        q1 = q1 + beta0 * a.q[j];
        double u = a.tau * s;
        u += a.gam2 * q1;
        a.AD[j] = u;
    }
    block_put_sums<1>(acc, 1, ro, (int64_t)blockIdx.x);
    red_finish(ro, 1, lds);
}

hipError_t pre_compose2(int64_t M, int64_t N, const PreCompose2& a, const RedOut& ro, hipStream_t st) {
    hipLaunchKernelGGL(pre_compose2_kernel, dim3(red_blocks(M)), dim3(kBlock), 0, st, M, N, a, ro);
    return hipGetLastError();
}

hipError_t pre_compose(int64_t M, int64_t N, const PreCompose& a, const RedOut& ro, hipStream_t st) {
    hipLaunchKernelGGL(pre_compose_kernel, dim3(red_blocks(M)), dim3(kBlock), 0, st, M, N, a, ro);
    return hipGetLastError();
}

}  // namespace vk
