// vec.hip — gfx950 kernels of the vector side that every model shares: the
// fused two-stage reductions (dots, dots2, red_blocks) with the gam1 chain on
// their sums, the denoiser (g1 / g1d) and the EM sums with the mixture's
// update, tail_post, the element-wise updates (lincomb_div, axpby, bernoulli,
// prelude, the *_scalar kernels, vec_div, scale_vec) and the host flag kernels
// (signal_host, post_flag, publish_host).  None of them reads X.  Launched by
// engine.cpp (DotBatch and the vector entry points), vamp.cpp, probit.cpp,
// pcg.cpp and assoc.cpp; the reduction, denoiser and element-wise sections of
// kernels.h are the interface.
#include "kernels.h"
#include "kdev.h"

#include <algorithm>

namespace vk {

// ---------------------------------------------------------------------------
// reductions (inner_prod / l2_norm2, src/utilities.cpp:138-162)
// ---------------------------------------------------------------------------
int red_blocks(int64_t n) {
    int64_t b = cdiv(n, 512);  // >= 2 elements per thread; enough blocks to fill 256 CUs at M ~ 1e5
    if (b < 1) b = 1;
    if (b > kRedBlocks) b = kRedBlocks;
    return (int)b;
}

// src/vamp.cpp:341-346, 498 (G1Chain): the host's expressions
__device__ __forceinline__ void gam1_chain(double a2, double gam2, double rho, double gam1_prev, double* out) {
    const double alpha2 = gam2 * a2;    // :498
    const double eta2 = gam2 / alpha2;  // :341
    const double d = eta2 - gam2;
    double g = d < 1e-11 ? 1e-11 : d;  // std::max(d, 1e-11)
    g = 1e11 < g ? 1e11 : g;           // std::min(., 1e11)
    out[0] = rho * g + (1 - rho) * gam1_prev;  // :346
    out[1] = eta2;
    out[2] = alpha2;
}

// every term loads both operands unconditionally (a SUM term's b is its a,
// set on the host) so a thread's loads for all terms are in flight together;
// the op is a per-launch uniform selected per element.  UPD: some term is a
// PUPD / SQPUPD (its c and beta are loaded); a launch without one does not
// keep those pointers (up to 12 terms without scalar-register spills)
// one reduction's blocks [bid of nblk]: the per-block partials of its NT terms
template <int NT, bool UPD>
__device__ __forceinline__ void dots_part(const DotArgs& a, int64_t n, const RedOut& ro, int bid, int nblk) {
    double bt[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) bt[q] = UPD && (a.t[q].op == PUPD || a.t[q].op == SQPUPD) ? *a.t[q].beta : 0.0;
    double acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = 0.0;
    for (int64_t e = (int64_t)bid * kBlock + threadIdx.x; e < n; e += (int64_t)nblk * kBlock) {
        double va[NT], vb[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            va[q] = a.t[q].a[e];
            vb[q] = UPD && (a.t[q].op == PUPD || a.t[q].op == SQPUPD) ? a.t[q].c[e] + bt[q] * a.t[q].b[e]
                                                                     : a.t[q].b[e];
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const double d = va[q] - vb[q];
            const int op = a.t[q].op;
            const double v = (op == DOT || op == PUPD) ? va[q] * vb[q]
                             : op == SQPUPD            ? vb[q] * vb[q]
                             : op == DIFF2             ? d * d
                                                       : va[q];
            acc[q] += v;
        }
    }
    block_put_sums<NT>(acc, NT, ro, (int64_t)bid * NT);
}

// the launch's hooks on its final sums (thread 0 of the last block)
__device__ __forceinline__ void dots_post(const DotArgs& a, const double* fin) {
    if (a.g1.out) gam1_chain(fin[a.g1.term], a.g1.gam2, a.g1.rho, a.g1.gam1_prev, a.g1.out);
    for (int j = 0; j < a.copy.n && j < 2; ++j) a.copy.dst[j][0] = fin[a.copy.term[j]];
}

template <int NT, bool UPD>
__global__ __launch_bounds__(kBlock) void dots_kernel(DotArgs a, int64_t n, RedOut ro) {
    if (ro.gate && !*ro.gate) return;
    __shared__ double lds[4];
    dots_part<NT, UPD>(a, n, ro, (int)blockIdx.x, (int)gridDim.x);
    __shared__ double fin[NT];
    const bool post = a.g1.out || a.copy.n;
    if (red_finish(ro, NT, lds, post ? fin : nullptr) && post && threadIdx.x == 0) dots_post(a, fin);
}

// Two reductions in one launch (dots2): blocks [0, ba) are reduction A's
// (red_blocks(na) of them), the rest B's; each part's partials, final sums and
// hooks are those of its own dots launch, bit for bit.  One ticket counts every
// block; the last one finishes A, then B (B's RedOut carries the flag).
template <int NA, int NB>
__global__ __launch_bounds__(kBlock) void dots2_kernel(DotArgs a, int64_t na, RedOut roa, int ba, DotArgs b,
                                                       int64_t nb, RedOut rob) {
    if ((int)blockIdx.x < ba)
        dots_part<NA, false>(a, na, roa, (int)blockIdx.x, ba);
    else
        dots_part<NB, false>(b, nb, rob, (int)blockIdx.x - ba, (int)gridDim.x - ba);
    if (!red_ticket(roa, (int)gridDim.x)) return;
    __shared__ double fa[NA], fb[NB];
    red_final(roa, NA, ba, fa, false);
    red_final(rob, NB, (int)gridDim.x - ba, fb, true);
    if (threadIdx.x == 0) {
        dots_post(a, fa);
        dots_post(b, fb);
    }
}

hipError_t dots2(const DotArgs& a, int64_t na, const RedOut& roa, const DotArgs& b, int64_t nb, const RedOut& rob,
                 hipStream_t st) {
    const int ba = red_blocks(na), bb = red_blocks(nb);
    if (roa.flag || roa.gate || rob.gate || rob.ticket != roa.ticket) return hipErrorInvalidValue;
    for (const DotArgs* x : {&a, &b})
        for (int q = 0; q < x->nt; ++q)
            if (x->t[q].op == PUPD || x->t[q].op == SQPUPD) return hipErrorInvalidValue;
    const dim3 g(ba + bb), blk(kBlock);
    if (a.nt == 10 && b.nt == 11)
        hipLaunchKernelGGL((dots2_kernel<10, 11>), g, blk, 0, st, a, na, roa, ba, b, nb, rob);
    else
        return hipErrorInvalidValue;  // (the one pairing in use: vamp.cpp's iteration tail)
    return hipGetLastError();
}

template <bool UPD>
static hipError_t dots_launch(const DotArgs& a, int64_t n, const RedOut& ro, hipStream_t st) {
    const dim3 g(red_blocks(n)), b(kBlock);
    switch (a.nt) {
        case 1: hipLaunchKernelGGL((dots_kernel<1, UPD>), g, b, 0, st, a, n, ro); break;
        case 2: hipLaunchKernelGGL((dots_kernel<2, UPD>), g, b, 0, st, a, n, ro); break;
        case 3: hipLaunchKernelGGL((dots_kernel<3, UPD>), g, b, 0, st, a, n, ro); break;
        case 4: hipLaunchKernelGGL((dots_kernel<4, UPD>), g, b, 0, st, a, n, ro); break;
        case 5: hipLaunchKernelGGL((dots_kernel<5, UPD>), g, b, 0, st, a, n, ro); break;
        case 6: hipLaunchKernelGGL((dots_kernel<6, UPD>), g, b, 0, st, a, n, ro); break;
        case 7: hipLaunchKernelGGL((dots_kernel<7, UPD>), g, b, 0, st, a, n, ro); break;
        case 8: hipLaunchKernelGGL((dots_kernel<8, UPD>), g, b, 0, st, a, n, ro); break;
        case 9: if (!UPD) { hipLaunchKernelGGL((dots_kernel<9, false>), g, b, 0, st, a, n, ro); break; } return hipErrorInvalidValue;
        case 10: if (!UPD) { hipLaunchKernelGGL((dots_kernel<10, false>), g, b, 0, st, a, n, ro); break; } return hipErrorInvalidValue;
        case 11: if (!UPD) { hipLaunchKernelGGL((dots_kernel<11, false>), g, b, 0, st, a, n, ro); break; } return hipErrorInvalidValue;
        case 12: if (!UPD) { hipLaunchKernelGGL((dots_kernel<12, false>), g, b, 0, st, a, n, ro); break; } return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (at most 8 terms when one of them is a PUPD / SQPUPD)
hipError_t dots(const DotArgs& a, int64_t n, const RedOut& ro, hipStream_t st) {
    bool upd = false;
    for (int q = 0; q < a.nt && q < kMaxTerms; ++q) upd = upd || a.t[q].op == PUPD || a.t[q].op == SQPUPD;
    return upd ? dots_launch<true>(a, n, ro, st) : dots_launch<false>(a, n, ro, st);
}

constexpr int Q_MAX_EM = 1 + 2 * (kMaxL - 1);  // an EM round's sums

// x^1.5, correctly rounded except in hard midpoint cases (glibc's pow is within
// 0.52 ulp, i.e. the same double in practice).  sqrt is correctly rounded;
// e = x - s^2 and the product's low part are exact through fma, so
// t + (t_lo + x*e/(2s)) is x*sqrt(x) to ~2^-105 before the final rounding.
// g1d's pkdd term needs this: at gam1 = 1e-6 (sigma = 1e6) it feeds a
// cancellation 1 + sigma*(...) ~ 5e-8 that amplifies one ulp ~1e7-fold.
__device__ __forceinline__ double pow_1p5(double x) {
    if (!(x > 0.0) || x == __builtin_huge_val()) return pow(x, 1.5);
    const double s = sqrt(x);
    const double e = __builtin_fma(-s, s, x);
    const double t = x * s;
    const double t_lo = __builtin_fma(x, s, -t);
    return t + (t_lo + x * (e / (2.0 * s)));
}

// ---------------------------------------------------------------------------
// denoiser: vamp::g1 / vamp::g1d (src/vamp.cpp:440-492)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void g1_g1d(double y, double gam1, const double* probs, const double* vars, int L,
                                       double eta_max, double* g, double* gd) {
    const double sigma = 1 / gam1;
    if (sigma < 1e-10 && sigma > -1e-10) {
        *g = y;
        *gd = 1;
        return;
    }
    double pk = 0, pkd = 0, pkdd = 0;
    for (int i = 0; i < L; ++i) {
        const double vs = vars[i] + sigma;
        const double expe_sum = -0.5 * (y * y) * (eta_max - vars[i]) / vs / (eta_max + sigma);
        const double ex = exp(expe_sum);
        double z = probs[i] / sqrt(vs) * ex;
        pk = pk + z;
        z = z / vs * y;
        pkd = pkd - z;
        const double z2 = z / vs * y;
        pkdd = pkdd - probs[i] / pow_1p5(vs) * ex + z2;
    }
    *g = y + sigma * pkd / pk;
    const double q = pkd / pk;
    *gd = 1 + sigma * (pkdd / pk - q * q);
}

// One EM round's update of the mixture (L components, variances vars) from
// the round's sums q (1 + 2(L-1)) and the merging of close variances
// (vamp.cpp em_finish with one round, the host's expressions in the host's
// order: src/vamp.cpp:598-642; every prob is rewritten), by ONE thread, into
// the mixture words w (kMixWords, LDS: [0] L, probs, vars, eta_max)
__device__ void em_update_mix(const double* q, int L, const double* vars, const EmUpd& u, double* w) {
    double* pr = w + 1;
    double* va = w + 1 + kMaxL;
    for (int j = 0; j < L; ++j) va[j] = vars[j];
    const double lambda_total = q[0];
    const double lambda = lambda_total / (double)u.Mt;
    const double sum_of_pin = lambda_total;
    for (int j = 0; j < L - 1; ++j) {
        const double res_total = q[1 + j];
        const double res_gammas_total = q[L + j];
        if (u.learn_vars == 1) va[j + 1] = res_gammas_total / res_total;
        const double omega = res_total / sum_of_pin;
        pr[j + 1] = lambda * omega;
    }
    pr[0] = 1 - lambda;
    for (int j = 0; j < L; ++j) {  // merging close variances (src/vamp.cpp:626-642)
        for (int k = j + 1; k < L; ++k) {
            const double denom = va[j] != 0 ? (va[k] < va[j] ? va[k] : va[j]) : 1e-7;  // std::min
            if (fabs(va[j] - va[k]) / denom < u.merge_vars_thr) {
                const double sum2probs = pr[j] + pr[k];
                for (int r = k; r + 1 < L; ++r) {
                    va[r] = va[r + 1];
                    pr[r] = pr[r + 1];
                }
                L--;
                pr[j] = sum2probs;
                k--;
            }
        }
    }
    double eta_max = va[0];  // (denoise: the host's loop)
    for (int i = 1; i < L; ++i)
        if (va[i] > eta_max) eta_max = va[i];
    w[0] = (double)L;
    w[1 + 2 * kMaxL] = eta_max;
}

// the next prelude's scalars (kernels.h PreOut) from the sum of x1d, gam1 and
// the two updateNoisePrec sums: the host's expressions
__device__ void pre_scalars(double sum_d, double gam1, double tn, double tc, const PreOut& po) {
    const double alpha1 = sum_d / po.Mt;  // :223
    const double eta1 = gam1 / alpha1;    // :230
    const double dg = eta1 - gam1;
    double gam2 = dg < 1e-11 ? 1e-11 : dg;  // std::max(., 1e-11) (:255-256)
    gam2 = 1e11 < gam2 ? 1e11 : gam2;       // std::min(., 1e11)
    const double trace_corr = tc * po.Mt;    // :521
    const double gamw = po.N / (tn + trace_corr);  // :528
    const double diag = gamw * (po.N - 1) / po.N + gam2;  // :676-677 (pcg_run)
    const double v[5] = {eta1, gam2, gamw, diag, gam1};
    for (int q = 0; q < 5; ++q) po.out[q] = v[q];
    for (int q = 0; q < 4; ++q) po.mirror[q] = v[q];
}

// the mixture words w (em_update_mix) into upd.out and upd.mirror
__device__ void em_write(const double* w, const EmUpd& u) {
    const int Ln = (int)w[0];
    for (double* o : {u.out, u.mirror}) {
        o[0] = w[0];
        for (int j = 0; j < Ln; ++j) {
            o[1 + j] = w[1 + j];
            o[1 + kMaxL + j] = w[1 + kMaxL + j];
        }
        o[1 + 2 * kMaxL] = w[1 + 2 * kMaxL];
    }
}

// Dev: the mixture's words (an EM round's update, em_kernel) and gam1
// (G1Chain) from the device, the words staged in LDS; else mix and gam1
template <bool Dev>
__global__ __launch_bounds__(kBlock) void denoise_kernel(int64_t M, const double* __restrict__ r1, double gam1,
                                                         Mix mix, double eta_max, double* __restrict__ x1,
                                                         const double* __restrict__ x1_prev, int damp, double rho,
                                                         double* __restrict__ x1d, RedOut ro,
                                                         const double* __restrict__ mixw,
                                                         const double* __restrict__ gam1dev, PreOut po) {
    __shared__ double lds[4];
    __shared__ double sm[Dev ? kMixWords : 1];
    // po: tn and tc (device copies) are loaded at the start, their latency
    // behind the launch's work; the last block uses them
    double tn = 0.0, tc = 0.0;
    if (Dev && po.out && threadIdx.x == 0) {
        tn = po.tn[0];
        tc = po.tc[0];
    }
    const double* probs = mix.probs;
    const double* vars = mix.vars;
    int L = mix.L;
    if (Dev) {
        for (int q = threadIdx.x; q < kMixWords; q += kBlock) sm[q] = mixw[q];
        gam1 = gam1dev[0];
        __syncthreads();
        L = (int)sm[0];
        probs = sm + 1;
        vars = sm + 1 + kMaxL;
        eta_max = sm[1 + 2 * kMaxL];
    }
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M; i += (int64_t)gridDim.x * kBlock) {
        double g, gd;
        g1_g1d(r1[i], gam1, probs, vars, L, eta_max, &g, &gd);
        if (damp) g = rho * g + (1 - rho) * x1_prev[i];  // src/vamp.cpp:208-211
        x1[i] = g;
        x1d[i] = gd;
        acc += gd;
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) red_put(ro, blockIdx.x, acc);
    __shared__ double fin[1];
    const bool last = red_finish(ro, 1, lds, Dev && po.out ? fin : nullptr);
    if (Dev && po.out && last && threadIdx.x == 0) pre_scalars(fin[0], gam1, tn, tc, po);
}

hipError_t denoise(int64_t M, const double* r1, double gam1, const Mix& mix, double* x1, const double* x1_prev,
                   int damp, double rho, double* x1d, const RedOut& ro, hipStream_t st, const double* mixw,
                   const double* gam1dev, const PreOut* po) {
    double eta_max = mix.vars[0];
    for (int i = 1; i < mix.L; ++i)
        if (mix.vars[i] > eta_max) eta_max = mix.vars[i];
    if (mixw) {
        if (!gam1dev || (po && (!po->out || !po->mirror || !po->tn || !po->tc))) return hipErrorInvalidValue;
        hipLaunchKernelGGL(denoise_kernel<true>, dim3(red_blocks(M)), dim3(kBlock), 0, st, M, r1, gam1, mix, eta_max,
                           x1, x1_prev, damp, rho, x1d, ro, mixw, gam1dev, po ? *po : PreOut{});
    } else {
        if (po) return hipErrorInvalidValue;
        hipLaunchKernelGGL(denoise_kernel<false>, dim3(red_blocks(M)), dim3(kBlock), 0, st, M, r1, gam1, mix,
                           eta_max, x1, x1_prev, damp, rho, x1d, ro, nullptr, nullptr, PreOut{});
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// EM prior update sums (src/vamp.cpp:554-597), one marker per thread
// ---------------------------------------------------------------------------
__device__ __forceinline__ double em_num(const EmArgs& a, double noise_var, double r, int j) {
    return a.lambda * a.omegas[j] *
           exp(-(r * r) / 2 * (a.max_sigma - a.vars[j]) / (a.vars[j] + noise_var) / (a.max_sigma + noise_var)) /
           sqrt(a.vars[j] + noise_var) / sqrt(2 * M_PI);
}

// The Q = 1 + 2(L-1) block sums: each wave reduces every value in registers
// and leaves it in LDS, ONE barrier, then thread q adds the four wave sums in
// wave order: per value the arithmetic of block_sum (bitwise), with one
// barrier instead of 2Q.  a.r1out: r1 is formed here (lincomb_div's
// expression) and stored, not read.
__global__ __launch_bounds__(kBlock) void em_kernel(int64_t M, const double* __restrict__ r1, EmArgs a, RedOut ro) {
    __shared__ double lds[4];
    __shared__ double wl[4][1 + 2 * (kMaxL - 1)];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool valid = i < M;
    // gam1 and eta2 from the device (a.dsc) or the host; the derived scalars
    // with the host's expressions (vamp.cpp em_queue)
    const double gam1 = a.dsc ? a.dsc[0] : a.gam1;
    const double noise_var = a.dsc ? 1 / gam1 : a.noise_var;
    double r = 0.0;
    if (valid) {
        if (a.r1out) {
            const double la = a.dsc ? a.dsc[1] : a.la, lc = a.dsc ? gam1 : a.lc;
            r = (la * a.lx[i] - a.lb * a.ly[i]) / lc;  // lincomb_div_kernel's expression
            a.r1out[i] = r;
        } else {
            r = r1[i];
        }
    }
    const int L = a.L, Q = 1 + 2 * (L - 1);
    // em_num of the first kEmC - 1 slabs is formed once and kept in registers
    // (fixed-bound unrolled loops: no run-time register indexing); the same
    // values, summed in the same order, as forming it twice
    constexpr int kEmC = 12;
    double en[kEmC];
    double sum_of_elems = 0.0;
#pragma unroll
    for (int j = 1; j < kEmC; ++j)
        if (j < L) {
            en[j] = em_num(a, noise_var, r, j);
            sum_of_elems += en[j];
        }
    for (int j = kEmC; j < L; ++j) sum_of_elems += em_num(a, noise_var, r, j);
    const double pin = 1 / (1 + (1 - a.lambda) / sqrt(2 * M_PI * noise_var) *
                                    exp(-(r * r) / 2 * a.max_sigma / noise_var / (noise_var + a.max_sigma)) /
                                    sum_of_elems);
    double s = wave_sum(valid ? pin : 0.0);
    if (lane == 0) wl[w][0] = s;
    auto slab = [&](int j, double num) {
        const double beta = num / sum_of_elems;
        const double g = gam1 * r / (1 / a.vars[j] + gam1);
        const double vj = a.dsc ? 1.0 / (1.0 / a.vars[j] + gam1) : a.v[j - 1];
        const double gam = beta * (g * g + vj);
        const double sb = wave_sum(valid ? beta * pin : 0.0);
        const double sg = wave_sum(valid ? gam * pin : 0.0);
        if (lane == 0) {
            wl[w][j] = sb;
            wl[w][(L - 1) + j] = sg;
        }
    };
#pragma unroll
    for (int j = 1; j < kEmC; ++j)
        if (j < L) slab(j, en[j]);
    for (int j = kEmC; j < L; ++j) slab(j, em_num(a, noise_var, r, j));
    __syncthreads();
    for (int q = threadIdx.x; q < Q; q += kBlock)
        red_put(ro, (int64_t)blockIdx.x * Q + q, ((wl[0][q] + wl[1][q]) + wl[2][q]) + wl[3][q]);
    __shared__ double fin[Q_MAX_EM];
    const bool last = red_finish(ro, Q, lds, a.upd.out ? fin : nullptr);
    if (last && a.upd.out && threadIdx.x == 0) {  // the round's update of the mixture (EmArgs.upd)
        __shared__ double w[kMixWords];
        em_update_mix(fin, L, a.vars, a.upd, w);
        em_write(w, a.upd);
    }
}

// kernels.h TailPost: the one-rank last blocks' work, after the all-reduce
__global__ void tail_post_kernel(TailPost t) {
    if (threadIdx.x != 0) return;
    if (t.mode == 0) {
        gam1_chain(t.src[0], t.g1.gam2, t.g1.rho, t.g1.gam1_prev, t.g1.out);
        for (int i = 0; i < 2; ++i)
            if (t.cp_dst[i]) *t.cp_dst[i] = *t.cp_src[i];
    } else if (t.mode == 1) {
        __shared__ double w[kMixWords];
        em_update_mix(t.src, t.L, t.vars, t.upd, w);
        em_write(w, t.upd);
    } else {
        pre_scalars(t.src[0], t.gam1dev[0], t.po.tn[0], t.po.tc[0], t.po);
    }
}

hipError_t tail_post(const TailPost& t, hipStream_t st) {
    if (!t.src || t.mode < 0 || t.mode > 2 || (t.mode == 0 && !t.g1.out) || (t.mode == 1 && (!t.upd.out || !t.upd.mirror)) ||
        (t.mode == 2 && (!t.gam1dev || !t.po.out || !t.po.mirror || !t.po.tn || !t.po.tc)))
        return hipErrorInvalidValue;
    for (int i = 0; i < 2; ++i)
        if (t.cp_dst[i] && !t.cp_src[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tail_post_kernel, dim3(1), dim3(64), 0, st, t);
    return hipGetLastError();
}

hipError_t em_sums(int64_t M, const double* r1, const EmArgs& a, const RedOut& ro, hipStream_t st) {
    const int nblk = (int)std::max<int64_t>(1, cdiv(M, kBlock));
    hipLaunchKernelGGL(em_kernel, dim3(nblk), dim3(kBlock), 0, st, M, r1, a, ro);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// elementwise
// ---------------------------------------------------------------------------
__global__ void lincomb_div_kernel(int64_t n, double a, const double* __restrict__ x, double b,
                                   const double* __restrict__ y, double c, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (a * x[i] - b * y[i]) / c;
}

hipError_t lincomb_div(int64_t n, double a, const double* x, double b, const double* y, double c, double* out,
                       hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lincomb_div_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, a, x, b, y, c,
                       out);
    return hipGetLastError();
}

__global__ void axpby_kernel(int64_t n, double a, const double* __restrict__ x, double b,
                             const double* __restrict__ y, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = a * x[i] + b * y[i];
}

hipError_t axpby(int64_t n, double a, const double* x, double b, const double* y, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, a, x, b, y, out);
    return hipGetLastError();
}

__global__ void bern_kernel(uint64_t seed, int it, int64_t S, int64_t M, double sqrtMt, double* out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < M) out[i] = (double)(2 * bern_bit(seed, it, S + i) - 1) / sqrtMt;
}

hipError_t bernoulli(uint64_t seed, int it, int64_t S, int64_t M, double sqrtMt, double* out, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(bern_kernel, dim3((unsigned)cdiv(M, kBlock)), dim3(kBlock), 0, st, seed, it, S, M, sqrtMt,
                       out);
    return hipGetLastError();
}

__global__ void prelude_kernel(int64_t M, Prelude p) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    double vv, bn;
    prelude_at(p, i, p.x1[i], p.r1[i], p.atxy[i], p.eta1, p.gam1, p.gam2, p.gamw, vv, bn);
}

hipError_t prelude(int64_t M, const Prelude& p, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(prelude_kernel, dim3((unsigned)cdiv(M, kBlock)), dim3(kBlock), 0, st, M, p);
    return hipGetLastError();
}

__global__ void set_scalar_kernel(double* p, double v) {
    if (threadIdx.x == 0) *p = v;
}

hipError_t set_scalar(double* p, double v, hipStream_t st) {
    hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(64), 0, st, p, v);
    return hipGetLastError();
}

__global__ void div_scalar_kernel(int64_t n, const double* __restrict__ x, double d, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = x[i] / d;
}

hipError_t div_scalar(int64_t n, const double* x, double d, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(div_scalar_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, x, d, out);
    return hipGetLastError();
}

// out[0, n) = x / d, out[n, 2n) = r / d (IEEE division, as the host's x / sqrt(N))
__global__ void div2_scalar_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ r, double d,
                                   double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        out[i] = x[i] / d;
        out[n + i] = r[i] / d;
    }
}

hipError_t div2_scalar(int64_t n, const double* x, const double* r, double d, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(div2_scalar_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, x, r, d, out);
    return hipGetLastError();
}

__global__ void vec_div_kernel(int K, int64_t n, Ptrs v, double div, Ptrs dst) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (int64_t)K * n) return;
    const int k = (int)(e / n);
    const int64_t j = e - (int64_t)k * n;
    dst.p[k][j] = v.p[k][j] / div;
}

hipError_t vec_div(int K, int64_t n, int64_t /*ld*/, Ptrs v, double div, hipStream_t st, const Ptrs* dst) {
    hipLaunchKernelGGL(vec_div_kernel, dim3((unsigned)cdiv((int64_t)K * n, kBlock)), dim3(kBlock), 0, st, K, n, v,
                       div, dst ? *dst : v);
    return hipGetLastError();
}

__global__ void scale_kernel(int64_t n, double* v, double a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) v[i] *= a;
}

hipError_t scale_vec(int64_t n, double* v, double a, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, v, a);
    return hipGetLastError();
}

__global__ void mul_scalar_kernel(int64_t n, const double* __restrict__ x, double a, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = x[i] * a;
}

hipError_t mul_scalar(int64_t n, const double* x, double a, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mul_scalar_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, st, n, x, a, out);
    return hipGetLastError();
}

// completion flag for the host: a system-scope release store of seq into
// mapped host memory, after everything earlier on the stream
__global__ void signal_kernel(unsigned long long* flag, unsigned long long seq) {
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// a sequence number into mapped host memory after everything earlier on the
// stream; the iteration writer's "slot landed" word.  The staging data it
// announces was written by an earlier kernel with plain stores, so the store
// is a system-scope RELEASE: it writes back the L2 (the whole device's, not
// only this kernel's writes) before the word can be seen by the host, which
// does not rely on the packet fence scope or on the staging memory's mapping
// type.  One thread, once per iteration: the writeback costs nothing
__global__ void post_flag_kernel(unsigned long long* flag, unsigned long long seq) {
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t post_flag(unsigned long long* flag, unsigned long long seq, hipStream_t st) {
    hipLaunchKernelGGL(post_flag_kernel, dim3(1), dim3(1), 0, st, flag, seq);
    return hipGetLastError();
}

hipError_t signal_host(unsigned long long* flag, unsigned long long seq, hipStream_t st) {
    hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(1), 0, st, flag, seq);
    return hipGetLastError();
}

// multi-rank DotBatch results: after the all-reduce, copy the synced and the
// local slot ranges into mapped host memory, then raise the host flag
__global__ void publish_kernel(const double* __restrict__ a, int na, double* __restrict__ ha, const double* __restrict__ b,
                               int nb, double* __restrict__ hb, unsigned long long* flag, unsigned long long seq) {
    for (int i = threadIdx.x; i < na; i += blockDim.x) ha[i] = a[i];
    for (int i = threadIdx.x; i < nb; i += blockDim.x) hb[i] = b[i];
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t publish_host(const double* a, int na, double* ha, const double* b, int nb, double* hb,
                        unsigned long long* flag, unsigned long long seq, hipStream_t st) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(256), 0, st, a, na, ha, b, nb, hb, flag, seq);
    return hipGetLastError();
}

}  // namespace vk
