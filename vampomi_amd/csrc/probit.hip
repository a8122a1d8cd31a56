// probit.hip — gfx950 kernels of the probit model: the N-side denoiser with
// and without the covariate offset (probit_denoise_kernel,
// probit_denoise_cov_kernel) over the reference's erfcx, the accuracy counts
// (confusion_kernel), the first p1 (probit_p1_kernel), and the covariate
// effects' Newton fit: the tile sums of H, rhs and mlogL (cov_tile_kernel,
// cov_finish_kernel) and the offset Z eta (cov_offset_kernel).  None of them
// reads X.  Launched by probit.cpp and covariates.cpp (and by the denoiser's
// own C entry point, vampomi_denoise_bin_cov in engine.cpp); the probit and
// covariate sections of kernels.h are the interface.
#include "kernels.h"
#include "kdev.h"

namespace vk {

// exp correctly rounded in practice (the probit denoiser's erfcx; exp_cr.h)
#define EXPCR_FN __device__ __forceinline__
#include "exp_cr.h"

// ---------------------------------------------------------------------------
// probit model: N-side denoiser and accuracy counts (src/vamp_probit.cpp)
// ---------------------------------------------------------------------------
// erfcx as the reference evaluates it (src/utilities.cpp:293-363: N. Juffa's
// published fma approximation, with +inf below -10 and lowest() above 10).
// Same operations in the same order as the oracle's orc_erfcx.  exp() is the
// correctly rounded exp_cr (exp_cr.h), not OCML's ~1-ulp exp: it equals glibc's
// (the oracle's, the reference's) except where glibc misrounds, 0.08 % of the
// arguments (tests/exp_cr_check.c).
__constant__ double kErfcxPoly[24] = {
    0x1.edcad78fc8044p-31,  0x1.b1548f14735d1p-30,  -0x1.a1ad2e6c4a7a8p-27, -0x1.1985b48f08574p-26,
    0x1.c6a8093ac4f83p-24,  0x1.31c2b2b44b731p-24,  -0x1.b87373facb29fp-21, 0x1.3fef1358803b7p-22,
    0x1.7eec072bb0be3p-18,  -0x1.78a680a741c4ap-17, -0x1.9951f39295cf4p-16, 0x1.3be1255ce180bp-13,
    -0x1.a1df71176b791p-13, -0x1.8d4aaa0099bc8p-11, 0x1.49c673066c831p-8,   -0x1.0962386ea02b7p-6,
    0x1.3079edf465cc3p-5,   -0x1.0fb06dfedc4ccp-4,  0x1.7fee004e266dfp-4,   -0x1.9ddb23c3e14d2p-4,
    0x1.16ecefcfa4865p-4,   0x1.f7f5df66fc349p-7,   -0x1.1df1ad154a27fp-3,  0x1.dd2c8b74febf6p-3};

__device__ __forceinline__ double erfcx_ref(double x) {
    if (x < -10.0) return __builtin_inf();
    if (x > 10.0) return -1.7976931348623157e308;
    const double a = fmax(x, 0.0 - x);
    const double inv = 1.0 / (a + 4.0);
    double q = (a - 4.0) * inv;
    const double t0 = __builtin_fma(q + 1.0, -4.0, a);
    q = __builtin_fma(inv, __builtin_fma(q, -a, t0), q);
    double p = kErfcxPoly[0];
#pragma unroll
    for (int k = 1; k < 24; ++k) p = __builtin_fma(p, q, kErfcxPoly[k]);
    const double h = (1.0 / (a + 0.5)) * 0.5;
    const double q1 = __builtin_fma(p, h, h);
    const double res = (p - q1) + __builtin_fma(q1 + q1, -a, 1.0);
    double r = __builtin_fma(res, h, q1);
    if (a > 1.7976931348623157e308) r = 0.0;
    if (x < 0.0) {
        const double s = x * x;
        const double lo = __builtin_fma(x, x, -s);
        const double e = exp_cr(s);
        r = __builtin_fma(e, lo + lo, e - r) + e;
        if (e > 1.7976931348623157e308) r = e;
    }
    return r;
}

// (the body of probit_denoise_kernel and probit_denoise_cov_kernel)  COV: with
// the covariate offset m_cov (g1_bin_class / g1d_bin_class with m_cov,
// src/vamp_probit.cpp:469-488); else the offset is the reference's 0.0
template <bool COV>
__device__ __forceinline__ void probit_denoise_body(int64_t N, const double* __restrict__ p1,
                                                    const double* __restrict__ y,
                                                    const double* __restrict__ m_cov, double tau1,
                                                    double* __restrict__ z1, const RedOut& ro) {
    __shared__ double lds[4];
    const double sq = sqrt(1.0 + 1.0 / tau1);           // sqrt(probit_var + 1/tau1)
    const double k0 = 2.0 / sqrt(2 * M_PI), rt2 = sqrt(2.0);
    const double den = 1 + tau1 * 1.0;                  // 1 + tau1*probit_var
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
        const double p = p1[i], s = 2 * y[i] - 1;
        const double c = (p + (COV ? m_cov[i] : 0.0)) / sq;
        const double ratio = k0 / erfcx_ref(-s * c / rt2);
        z1[i] = p + s * ratio / tau1 / sq;
        acc += 1 - ratio / den * (s * c + ratio);
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) red_put(ro, blockIdx.x, acc);
    red_finish(ro, 1, lds);
}

__global__ __launch_bounds__(kBlock) void probit_denoise_kernel(int64_t N, const double* __restrict__ p1,
                                                                const double* __restrict__ y, double tau1,
                                                                double* __restrict__ z1, RedOut ro) {
    probit_denoise_body<false>(N, p1, y, nullptr, tau1, z1, ro);
}

__global__ __launch_bounds__(kBlock) void probit_denoise_cov_kernel(int64_t N, const double* __restrict__ p1,
                                                                    const double* __restrict__ y,
                                                                    const double* __restrict__ m_cov, double tau1,
                                                                    double* __restrict__ z1, RedOut ro) {
    probit_denoise_body<true>(N, p1, y, m_cov, tau1, z1, ro);
}

hipError_t probit_denoise(int64_t N, const double* p1, const double* y, double tau1, double* z1, const RedOut& ro,
                          hipStream_t st) {
    hipLaunchKernelGGL(probit_denoise_kernel, dim3(red_blocks(N)), dim3(kBlock), 0, st, N, p1, y, tau1, z1, ro);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void confusion_kernel(int64_t N, int nz, const double* __restrict__ z,
                                                           int64_t ld, const double* __restrict__ y,
                                                           RedOut ro) {
    __shared__ double lds[4];
    double cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
        const double yi = y[i];
        for (int k = 0; k < nz; ++k) {
            const double yh = (0.5 * erfc(-z[k * ld + i] * M_SQRT1_2) >= 0.5) ? 1.0 : 0.0;  // normal_cdf >= th
            if (yi == 1 && yh == 1)
                cnt[4 * k + 0] += 1;
            else if (yi == 0 && yh == 0)
                cnt[4 * k + 1] += 1;
            else if (yi == 0 && yh == 1)
                cnt[4 * k + 2] += 1;
            else if (yi == 1 && yh == 0)
                cnt[4 * k + 3] += 1;
        }
    }
    block_put_sums<8>(cnt, 4 * nz, ro, (int64_t)blockIdx.x * 4 * nz);
    red_finish(ro, 4 * nz, lds);
}

hipError_t probit_confusion(int64_t N, int nz, const double* z, int64_t ld, const double* y, const RedOut& ro,
                            hipStream_t st) {
    if (nz < 1 || nz > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(confusion_kernel, dim3(red_blocks(N)), dim3(kBlock), 0, st, N, nz, z, ld, y, ro);
    return hipGetLastError();
}

__global__ void probit_p1_kernel(uint64_t seed, int64_t N, double* p1) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < N) p1[i] = gauss_dyadic(seed ^ 0x50524F4249545031ULL, 0, i);
}

hipError_t probit_p1(uint64_t seed, int64_t N, double* p1, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(probit_p1_kernel, dim3((unsigned)cdiv(N, kBlock)), dim3(kBlock), 0, st, seed, N, p1);
    return hipGetLastError();
}

hipError_t probit_denoise_cov(int64_t N, const double* p1, const double* y, const double* m_cov, double tau1,
                              double* z1, const RedOut& ro, hipStream_t st) {
    hipLaunchKernelGGL(probit_denoise_cov_kernel, dim3(red_blocks(N)), dim3(kBlock), 0, st, N, p1, y, m_cov, tau1, z1,
                       ro);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// probit model: covariate effects (vamp::Newton_method_cov, mlogL_probit,
// src/vamp_probit.cpp:490-617)
// ---------------------------------------------------------------------------
// entry e of the upper triangle, rows in order: (0,0) .. (0,C-1), (1,1) ..
__device__ __forceinline__ void cov_tri(int e, int C, int& j, int& k) {
    j = 0;
    while (e >= C - j) {
        e -= C - j;
        ++j;
    }
    k = j + e;
}

// One tile of kCovTile samples per workgroup.  FULL (256 threads): the tile's
// Z rows are staged in LDS (row stride C | 1: the lanes' (j, k) reads spread
// over the banks), threads 0..nr-1 form g, lambda, w and -log Phi(arg) of their
// row, then thread e forms sum number e over the tile's rows in row order:
// the C(C+1)/2 upper entries of H, the C of rhs, the mlogL sum, written to
// part[tile*nq + e].  !FULL (64 threads): the mlogL sum alone, part[tile], by
// the same operations in the same order.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void cov_tile_kernel(int64_t N, int C, const double* __restrict__ Z, int64_t ld,
                                                          const double* __restrict__ y,
                                                          const double* __restrict__ gg,
                                                          const double* __restrict__ eta,
                                                          double* __restrict__ part) {
    constexpr int T = kCovTile;
    __shared__ double zt[FULL ? T * (kCovMaxC + 1) : 1];
    __shared__ double lam[T], w[T], ml[T], et[kCovMaxC];
    const int CS = C | 1, tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * T;
    const int nr = (int)(N - i0 < T ? N - i0 : T);
    if (tid < C) et[tid] = eta[tid];
    if constexpr (FULL) {
        const int r = tid & (T - 1);
        for (int j = tid / T; j < C; j += kBlock / T) zt[r * CS + j] = r < nr ? Z[(int64_t)j * ld + i0 + r] : 0.0;
    }
    __syncthreads();
    if (tid < nr) {
        const int64_t i = i0 + tid;
        double s = 0.0;  // inner_prod(Z[i], eta)
        for (int j = 0; j < C; ++j) {
            double zij;
            if constexpr (FULL)
                zij = zt[tid * CS + j];
            else
                zij = Z[(int64_t)j * ld + i];
            s += zij * et[j];
        }
        const double g = (gg ? gg[i] : 0.0) + s;
        const double sg = 2 * y[i] - 1;
        const double arg = sg * g;
        if constexpr (FULL) {
            const double ratio = 2.0 / sqrt(2 * M_PI) / erfcx_ref(-arg / sqrt(2.0));
            const double l = ratio * sg;
            lam[tid] = l;
            w[tid] = l * (l + g);
        }
        ml[tid] = -log(0.5 * erfc(-arg * M_SQRT1_2));  // -log(normal_cdf(arg))
    }
    __syncthreads();
    const int nH = C * (C + 1) / 2, nq = FULL ? nH + C + 1 : 1;
    for (int e = tid; e < nq; e += (int)blockDim.x) {
        double acc = 0.0;
        if (e == nq - 1) {
            for (int r = 0; r < nr; ++r) acc += ml[r];
        } else if (e < nH) {
            int j, k;
            cov_tri(e, C, j, k);
            for (int r = 0; r < nr; ++r) acc += zt[r * CS + j] * zt[r * CS + k] * w[r];
        } else {
            const int j = e - nH;
            for (int r = 0; r < nr; ++r) acc += zt[r * CS + j] * lam[r];
        }
        part[(int64_t)blockIdx.x * nq + e] = acc;
    }
}

// sum number q over the tiles in tile order, one thread per sum; full: out =
// H (C*C, mirrored), rhs (C), mlogL/N; else out[0] = mlogL/N
__global__ __launch_bounds__(kBlock) void cov_finish_kernel(int64_t ntiles, int nq, int C, int64_t N,
                                                            const double* __restrict__ part, double* __restrict__ out,
                                                            int full) {
    const int q = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (q >= nq) return;
    double s = 0.0;
    for (int64_t t = 0; t < ntiles; ++t) s += part[t * nq + q];
    if (!full) {
        out[0] = s / (double)N;
        return;
    }
    const int nH = C * (C + 1) / 2;
    if (q == nq - 1) {
        out[C * C + C] = s / (double)N;
    } else if (q >= nH) {
        out[C * C + (q - nH)] = s;
    } else {
        int j, k;
        cov_tri(q, C, j, k);
        out[j * C + k] = s;
        out[k * C + j] = s;
    }
}

static bool cov_args_ok(int64_t N, int C, const double* Z, int64_t ld) {
    return N >= 1 && C >= 1 && C <= kCovMaxC && Z && ld >= N;
}

hipError_t cov_eval(int64_t N, int C, const double* Z, int64_t ld, const double* y, const double* gg,
                    const double* eta, double* part, double* out, hipStream_t st) {
    if (!cov_args_ok(N, C, Z, ld) || !y || !eta || !part || !out) return hipErrorInvalidValue;
    const int64_t nt = cov_tiles(N);
    const int nq = cov_nq(C);
    hipLaunchKernelGGL(cov_tile_kernel<true>, dim3((unsigned)nt), dim3(kBlock), 0, st, N, C, Z, ld, y, gg, eta, part);
    hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)cdiv(nq, kBlock)), dim3(kBlock), 0, st, nt, nq, C, N, part,
                       out, 1);
    return hipGetLastError();
}

hipError_t cov_mlogl(int64_t N, int C, const double* Z, int64_t ld, const double* y, const double* gg,
                     const double* eta, double* part, double* out, hipStream_t st) {
    if (!cov_args_ok(N, C, Z, ld) || !y || !eta || !part || !out) return hipErrorInvalidValue;
    const int64_t nt = cov_tiles(N);
    hipLaunchKernelGGL(cov_tile_kernel<false>, dim3((unsigned)nt), dim3(kCovTile), 0, st, N, C, Z, ld, y, gg, eta,
                       part);
    hipLaunchKernelGGL(cov_finish_kernel, dim3(1), dim3(kBlock), 0, st, nt, 1, C, N, part, out, 0);
    return hipGetLastError();
}

__global__ void cov_offset_kernel(int64_t N, int C, const double* __restrict__ Z, int64_t ld,
                                  const double* __restrict__ eta, double* __restrict__ m) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int j = 0; j < C; ++j) s += Z[(int64_t)j * ld + i] * eta[j];
    m[i] = s;
}

hipError_t cov_offset(int64_t N, int C, const double* Z, int64_t ld, const double* eta, double* m, hipStream_t st) {
    if (!cov_args_ok(N, C, Z, ld) || !eta || !m) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cov_offset_kernel, dim3((unsigned)cdiv(N, kBlock)), dim3(kBlock), 0, st, N, C, Z, ld, eta, m);
    return hipGetLastError();
}

}  // namespace vk
