// ingest.hip — gfx950 kernels of the methylation ingest and read-back: the
// element conversions between a staged chunk and the shard (with the row
// gather and the 16-bit quantisation), the NaN policy and the covariate
// adjustment.  Nothing here is launched by a VAMP iteration or an association
// test.
#include "kdev.h"

#include <algorithm>

namespace vk {

// ---------------------------------------------------------------------------
// 16-bit fixed-point storage: quantisation at ingest
// ---------------------------------------------------------------------------
// dst = min(65535, rint(x * 65536)) for 0 <= x <= 1 (x * 65536 is exact, rint
// rounds ties to even, -0.0 compares equal to 0); anything else (NaN fails both
// comparisons) is rejected: stored as 0 and counted.  Each wave folds what its
// lanes saw (integer sums, a minimum, a maximum of non-negative doubles, which
// order as their bit patterns do) and lane 0 adds it to *rec with ordinary
// atomics, so the record does not depend on the order anything ran in.
struct QuantAcc {
    unsigned long long rejected = 0, clamped = 0, first = ~0ull;
    double err = 0.0;
    // the stored element of x; at: the entry's index for rec->first
    __device__ uint16_t put(double x, unsigned long long at) {
        unsigned k = 0;
        if (x >= 0.0 && x <= 1.0) {
            const double r = __builtin_rint(x * 65536.0);
            if (r > 65535.0) {
                k = 65535u;
                ++clamped;
            } else {
                k = (unsigned)r;
            }
            const double d = fabs((double)k * 0x1p-16 - x);
            err = d > err ? d : err;
        } else {
            ++rejected;
            first = at < first ? at : first;
        }
        return (uint16_t)k;
    }
    // every lane of the wave, once, after its last put
    __device__ void flush(QuantRec* __restrict__ rec) {
        unsigned long long eb = (unsigned long long)__double_as_longlong(err);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            rejected += __shfl_xor(rejected, o, 64);
            clamped += __shfl_xor(clamped, o, 64);
            const unsigned long long f = __shfl_xor(first, o, 64), m = __shfl_xor(eb, o, 64);
            first = f < first ? f : first;
            eb = m > eb ? m : eb;
        }
        if ((threadIdx.x & 63) == 0) {
            if (rejected) {
                atomicAdd(&rec->rejected, rejected);
                atomicMin(&rec->first, first);
            }
            if (clamped) atomicAdd(&rec->clamped, clamped);
            if (eb) atomicMax(&rec->max_err, eb);
        }
    }
};

// ---------------------------------------------------------------------------
// the ingest and read-back conversions, with or without a row gather
// ---------------------------------------------------------------------------
// what a conversion stores for one element where no record is kept: a double
// narrowed to nearest even, a float widened (exact), k * 2^-16 (exact as a
// double, and as a float: 16 significant bits), the identity where the types
// agree
template <class XD, class XS>
__device__ __forceinline__ XD ingest_conv(XS x) {
    return (XD)x;
}
template <>
__device__ __forceinline__ double ingest_conv<double, uint16_t>(uint16_t k) {
    return (double)k * 0x1p-16;
}
template <>
__device__ __forceinline__ float ingest_conv<float, uint16_t>(uint16_t k) {
    return (float)((double)k * 0x1p-16);
}

// dst[c*ldd + j] = conv(src[c*lds + row(j)]), j < n, c < ncols; row(j) is
// rows[j] with GATHER, else j.  A staged chunk's columns are packed, so a
// column starts only as aligned as its element: one element per load.  Doubles
// or floats into 16 bits go through a QuantAcc, the entry's index
// (col0 + c) * nfile + row(j): what a dropped row holds is neither stored,
// rejected nor counted
template <class XS, class XD, bool GATHER>
__global__ __launch_bounds__(kBlock) void convert_kernel(const XS* __restrict__ src, int64_t lds,
                                                         const int32_t* __restrict__ rows, int64_t n, int64_t ncols,
                                                         XD* __restrict__ dst, int64_t ldd, int64_t nfile,
                                                         int64_t col0, QuantRec* __restrict__ rec) {
    constexpr bool kQuant = sizeof(XD) == 2 && sizeof(XS) != 2;
    const int64_t total = n * ncols;
    [[maybe_unused]] QuantAcc acc;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t c = e / n, j = e - c * n;
        const int64_t r = GATHER ? (int64_t)rows[j] : j;
        if constexpr (kQuant)
            dst[c * ldd + j] = acc.put((double)src[c * lds + r], (unsigned long long)((col0 + c) * nfile + r));
        else
            dst[c * ldd + j] = ingest_conv<XD, XS>(src[c * lds + r]);
    }
    if constexpr (kQuant) acc.flush(rec);
}

hipError_t convert_cols(const void* src, int src_ek, int64_t lds, const int32_t* rows, int64_t n, int64_t ncols,
                        void* dst, int dst_ek, int64_t ldd, int64_t nfile, int64_t col0, QuantRec* rec,
                        hipStream_t st) {
    if (n <= 0 || ncols <= 0) return hipSuccess;
    const auto kind = [](int ek) { return ek == kXF64 || ek == kXF32 || ek == kXU16; };
    if (!kind(src_ek) || !kind(dst_ek) || n > nfile || (!rows && n != nfile) || lds < nfile || ldd < n ||
        (dst_ek == kXU16 && src_ek != kXU16 && !rec))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(n * ncols, kBlock), 65536));
    const auto go = [&](auto xs, auto xd) {
        using XS = decltype(xs);
        using XD = decltype(xd);
        if (rows)
            hipLaunchKernelGGL((convert_kernel<XS, XD, true>), grid, dim3(kBlock), 0, st, static_cast<const XS*>(src),
                               lds, rows, n, ncols, static_cast<XD*>(dst), ldd, nfile, col0, rec);
        else
            hipLaunchKernelGGL((convert_kernel<XS, XD, false>), grid, dim3(kBlock), 0, st, static_cast<const XS*>(src),
                               lds, rows, n, ncols, static_cast<XD*>(dst), ldd, nfile, col0, rec);
    };
    const auto from = [&](auto xs) {
        dst_ek == kXF64 ? go(xs, double{}) : dst_ek == kXF32 ? go(xs, float{}) : go(xs, uint16_t{});
    };
    src_ek == kXF64 ? from(double{}) : src_ek == kXF32 ? from(float{}) : from(uint16_t{});
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// missing values (NaN): the ingest conversions, column by column
// ---------------------------------------------------------------------------
// what the ingest stores for the value v where no record is kept: the fill of
// a missing entry (QuantAcc::put's k for a v in [0, 1], uncounted; 0 for any
// other, which only an infinite observed entry can make of a mean)
template <class XD>
__device__ __forceinline__ XD na_store(double v) {
    return (XD)v;
}
template <>
__device__ __forceinline__ uint16_t na_store<uint16_t>(double v) {
    if (!(v >= 0.0 && v <= 1.0)) return 0;
    const double r = __builtin_rint(v * 65536.0);
    return (uint16_t)(r > 65535.0 ? 65535u : (unsigned)r);
}

// the loads a thread issues before it uses the first (a 256 MB chunk of long
// columns is a few hundred workgroups, about one per CU: the memory-level
// parallelism has to come from within the thread).  The values are then used
// in row order, so the depth does not change a sum
static constexpr int kNaDepth = 8;

// One workgroup per column (grid-stride over the chunk's columns), two sweeps
// (kernels.h); the second re-reads what this workgroup has just read, out of
// L2.  The source columns are packed, so a column starts only as aligned as
// its element: one element per load, as in convert_kernel.  GATHER: row j of
// the output is row rows[j] of the input.
template <class XS, class XD, bool GATHER>
__global__ __launch_bounds__(kBlock) void na_ingest_kernel(const XS* __restrict__ src, int64_t lds,
                                                           const int32_t* __restrict__ rows, int64_t n, int64_t ncols,
                                                           XD* __restrict__ dst, int64_t ldd, int64_t nfile,
                                                           int64_t col0, int mode, double max_frac,
                                                           int64_t* __restrict__ cnt, NaRec* __restrict__ nrec,
                                                           QuantRec* __restrict__ qrec) {
    __shared__ double l_sum[4];
    __shared__ unsigned long long l_cnt[4], l_first[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    QuantAcc acc;
    for (int64_t c = blockIdx.x; c < ncols; c += gridDim.x) {
        const XS* __restrict__ col = src + c * lds;
        // sweep 1: this thread's rows in ascending order
        double s = 0.0;
        unsigned long long miss = 0, first = ~0ull;
        const auto see = [&](XS xs, int64_t r) {
            const double x = (double)xs;
            if (__builtin_isnan(x)) {
                ++miss;
                const unsigned long long at = (unsigned long long)((col0 + c) * nfile + r);
                first = at < first ? at : first;
            } else {
                s += x;
            }
        };
        int64_t j = threadIdx.x;
        for (; j + (kNaDepth - 1) * kBlock < n; j += kNaDepth * kBlock) {  // kNaDepth loads in flight, then in order
            XS x[kNaDepth];
            int64_t r[kNaDepth];
#pragma unroll
            for (int u = 0; u < kNaDepth; ++u) {
                r[u] = GATHER ? (int64_t)rows[j + u * kBlock] : j + u * kBlock;
                x[u] = col[r[u]];
            }
#pragma unroll
            for (int u = 0; u < kNaDepth; ++u) see(x[u], r[u]);
        }
        for (; j < n; j += kBlock) {
            const int64_t r = GATHER ? (int64_t)rows[j] : j;
            see(col[r], r);
        }
        s = wave_sum(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            miss += __shfl_xor(miss, o, 64);
            const unsigned long long f = __shfl_xor(first, o, 64);
            first = f < first ? f : first;
        }
        __syncthreads();  // the previous column's totals have been read
        if (lane == 0) {
            l_sum[w] = s;
            l_cnt[w] = miss;
            l_first[w] = first;
        }
        __syncthreads();
        s = ((l_sum[0] + l_sum[1]) + l_sum[2]) + l_sum[3];
        miss = l_cnt[0] + l_cnt[1] + l_cnt[2] + l_cnt[3];
        const bool masked = mode == kNaMean && (miss == (unsigned long long)n || (double)miss > max_frac * (double)n);
        if (threadIdx.x == 0) {
            cnt[c] = (int64_t)miss;
            if (miss) {
                unsigned long long f = l_first[0];
#pragma unroll
                for (int k = 1; k < 4; ++k) f = l_first[k] < f ? l_first[k] : f;
                atomicAdd(&nrec->missing, miss);
                atomicMin(&nrec->first, f);
                atomicAdd(&nrec->markers, 1ull);
                if (masked) atomicAdd(&nrec->masked, 1ull);
            }
        }
        if (mode == kNaFatal && miss) continue;  // (block-uniform) the load fails: nothing to store
        // sweep 2
        const double fill = masked ? 0.0 : s / (double)((unsigned long long)n - miss);
        const XD fill_st = na_store<XD>(fill);
        XD* __restrict__ out = dst + c * ldd;
        const auto put = [&](XS x, int64_t r) -> XD {
            XD v = fill_st;
            if (!__builtin_isnan(x)) {
                if constexpr (sizeof(XD) == 2)
                    v = acc.put((double)x, (unsigned long long)((col0 + c) * nfile + r));
                else
                    v = (XD)x;
                if (masked) v = (XD)0;
            }
            return v;
        };
        for (j = threadIdx.x; j + (kNaDepth - 1) * kBlock < n; j += kNaDepth * kBlock) {
            XS x[kNaDepth];
            int64_t r[kNaDepth];
#pragma unroll
            for (int u = 0; u < kNaDepth; ++u) {
                r[u] = GATHER ? (int64_t)rows[j + u * kBlock] : j + u * kBlock;
                x[u] = col[r[u]];
            }
#pragma unroll
            for (int u = 0; u < kNaDepth; ++u) out[j + u * kBlock] = put(x[u], r[u]);
        }
        for (; j < n; j += kBlock) {
            const int64_t r = GATHER ? (int64_t)rows[j] : j;
            out[j] = put(col[r], r);
        }
    }
    if constexpr (sizeof(XD) == 2) acc.flush(qrec);
}

template <class XS, class XD>
static void na_launch(const void* src, int64_t lds, const int32_t* rows, int64_t n, int64_t ncols, void* dst,
                      int64_t ldd, int64_t nfile, int64_t col0, int mode, double max_frac, int64_t* cnt, NaRec* nrec,
                      QuantRec* qrec, hipStream_t st) {
    const dim3 grid((unsigned)std::min<int64_t>(ncols, 65536));
    if (rows)
        hipLaunchKernelGGL((na_ingest_kernel<XS, XD, true>), grid, dim3(kBlock), 0, st, static_cast<const XS*>(src),
                           lds, rows, n, ncols, static_cast<XD*>(dst), ldd, nfile, col0, mode, max_frac, cnt, nrec,
                           qrec);
    else
        hipLaunchKernelGGL((na_ingest_kernel<XS, XD, false>), grid, dim3(kBlock), 0, st, static_cast<const XS*>(src),
                           lds, rows, n, ncols, static_cast<XD*>(dst), ldd, nfile, col0, mode, max_frac, cnt, nrec,
                           qrec);
}

hipError_t na_ingest_cols(const void* src, int src_ek, int64_t lds, const int32_t* rows, int64_t n, int64_t ncols,
                          void* dst, int dst_ek, int64_t ldd, int64_t nfile, int64_t col0, int mode, double max_frac,
                          int64_t* cnt, NaRec* nrec, QuantRec* qrec, hipStream_t st) {
    if (n <= 0 || ncols <= 0) return hipSuccess;
    if (!cnt || !nrec || n > nfile || (!rows && n != nfile) || lds < nfile || ldd < n ||
        (mode != kNaFatal && mode != kNaMean) || (src_ek != kXF64 && src_ek != kXF32) || (dst_ek == kXU16 && !qrec))
        return hipErrorInvalidValue;
    auto go = [&](auto xs, auto xd) {
        na_launch<decltype(xs), decltype(xd)>(src, lds, rows, n, ncols, dst, ldd, nfile, col0, mode, max_frac, cnt,
                                              nrec, qrec, st);
    };
    const bool d = src_ek == kXF64;
    if (dst_ek == kXF64)
        d ? go(double{}, double{}) : go(float{}, double{});
    else if (dst_ek == kXF32)
        d ? go(double{}, float{}) : go(float{}, float{});
    else if (dst_ek == kXU16)
        d ? go(double{}, uint16_t{}) : go(float{}, uint16_t{});
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// covariate adjustment: r = x - Q (Q^T x), column by column
// ---------------------------------------------------------------------------
// A workgroup takes kAdjB columns at a time (grid-stride over the chunk's
// column blocks), so every element of Q it reads serves kAdjB columns; thread t
// owns rows t, t + 256, ... of all of them.
//   1. c = Q^T x, kAdjKT basis vectors per sweep over the rows (kAdjB * kAdjKT
//      running sums per thread; x is re-read out of L2 for every sweep).
//   2. r = x - sum_k Q_k c_k, k ascending, one fma per term; r is stored as it
//      is formed, ||x||^2 and ||r||^2 summed, and an absorbed column's rows are
//      then overwritten with zeros by the threads that wrote them.
// Every sum: the thread's rows ascending (fma), wave_sum's butterfly, the four
// wave sums in wave order.  A column's sums are its own, so its bits depend on
// n, R, Q and x alone: not on its block-mates (a short last block computes on
// its first column again and stores nothing for it) nor on the chunk.
static constexpr int kAdjB = 4, kAdjKT = 8;

template <class XD>
__global__ __launch_bounds__(kBlock) void adjust_kernel(const double* __restrict__ src, int64_t n, int64_t ncols,
                                                        const double* __restrict__ Q, int R, XD* __restrict__ dst,
                                                        int64_t ldd, uint8_t* __restrict__ flags,
                                                        unsigned long long* __restrict__ absorbed) {
    __shared__ double l_part[4][kAdjB * kAdjKT];
    __shared__ double l_c[kAdjB][kAdjMaxR];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t c0 = (int64_t)blockIdx.x * kAdjB; c0 < ncols; c0 += (int64_t)gridDim.x * kAdjB) {
        const int nb = (int)(ncols - c0 < kAdjB ? ncols - c0 : kAdjB);
        const double* __restrict__ col[kAdjB];
#pragma unroll
        for (int b = 0; b < kAdjB; ++b) col[b] = src + (c0 + (b < nb ? b : 0)) * n;
        // 1. the coefficients
        for (int k0 = 0; k0 < R; k0 += kAdjKT) {
            double acc[kAdjB][kAdjKT];
#pragma unroll
            for (int b = 0; b < kAdjB; ++b)
#pragma unroll
                for (int kk = 0; kk < kAdjKT; ++kk) acc[b][kk] = 0.0;
            for (int64_t j = threadIdx.x; j < n; j += kBlock) {
                double x[kAdjB], q[kAdjKT];
#pragma unroll
                for (int b = 0; b < kAdjB; ++b) x[b] = col[b][j];
#pragma unroll
                for (int kk = 0; kk < kAdjKT; ++kk) q[kk] = k0 + kk < R ? Q[(int64_t)(k0 + kk) * n + j] : 0.0;
#pragma unroll
                for (int b = 0; b < kAdjB; ++b)
#pragma unroll
                    for (int kk = 0; kk < kAdjKT; ++kk) acc[b][kk] = fma(q[kk], x[b], acc[b][kk]);
            }
            __syncthreads();  // the previous sweep's partials have been read
#pragma unroll
            for (int b = 0; b < kAdjB; ++b)
#pragma unroll
                for (int kk = 0; kk < kAdjKT; ++kk) {
                    const double s = wave_sum(acc[b][kk]);
                    if (lane == 0) l_part[w][b * kAdjKT + kk] = s;
                }
            __syncthreads();
            if (threadIdx.x < kAdjB * kAdjKT) {
                const int i = threadIdx.x, k = k0 + i % kAdjKT;
                if (k < R) l_c[i / kAdjKT][k] = ((l_part[0][i] + l_part[1][i]) + l_part[2][i]) + l_part[3][i];
            }
        }
        __syncthreads();  // c is complete
        // 2. the residual, stored as it is formed
        double nx2[kAdjB], nr2[kAdjB];
#pragma unroll
        for (int b = 0; b < kAdjB; ++b) nx2[b] = nr2[b] = 0.0;
        for (int64_t j = threadIdx.x; j < n; j += kBlock) {
            double x[kAdjB], r[kAdjB];
#pragma unroll
            for (int b = 0; b < kAdjB; ++b) r[b] = x[b] = col[b][j];
#pragma unroll 4
            for (int k = 0; k < R; ++k) {
                const double q = Q[(int64_t)k * n + j];
#pragma unroll
                for (int b = 0; b < kAdjB; ++b) r[b] = fma(-q, l_c[b][k], r[b]);
            }
#pragma unroll
            for (int b = 0; b < kAdjB; ++b) {
                nx2[b] = fma(x[b], x[b], nx2[b]);
                nr2[b] = fma(r[b], r[b], nr2[b]);
                if (b < nb) dst[(c0 + b) * ldd + j] = (XD)r[b];
            }
        }
        __syncthreads();  // c and the last sweep's partials have been read
#pragma unroll
        for (int b = 0; b < kAdjB; ++b) {
            const double sx = wave_sum(nx2[b]), sr = wave_sum(nr2[b]);
            if (lane == 0) {
                l_part[w][2 * b] = sx;
                l_part[w][2 * b + 1] = sr;
            }
        }
        __syncthreads();
        // absorbed: ||r||^2 <= (1e-10)^2 ||x||^2 (an all-zero column too; a NaN never)
#pragma unroll
        for (int b = 0; b < kAdjB; ++b) {
            if (b >= nb) break;
            const double sx = ((l_part[0][2 * b] + l_part[1][2 * b]) + l_part[2][2 * b]) + l_part[3][2 * b];
            const double sr =
                ((l_part[0][2 * b + 1] + l_part[1][2 * b + 1]) + l_part[2][2 * b + 1]) + l_part[3][2 * b + 1];
            const bool gone = sr <= 1e-20 * sx;  // (block-uniform)
            if (threadIdx.x == 0) {
                flags[c0 + b] = gone ? 1 : 0;
                if (gone) atomicAdd(absorbed, 1ull);
            }
            if (gone)
                for (int64_t j = threadIdx.x; j < n; j += kBlock) dst[(c0 + b) * ldd + j] = (XD)0;
        }
    }
}

hipError_t adjust_cols(const double* src, int64_t n, int64_t ncols, const double* Q, int R, void* dst, int dst_ek,
                       int64_t ldd, uint8_t* flags, unsigned long long* absorbed, hipStream_t st) {
    if (n <= 0 || ncols <= 0) return hipSuccess;
    if (!src || !Q || !dst || !flags || !absorbed || R < 1 || R > kAdjMaxR || ldd < n ||
        (dst_ek != kXF64 && dst_ek != kXF32))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(ncols, kAdjB), 65536));
    if (dst_ek == kXF64)
        hipLaunchKernelGGL(adjust_kernel<double>, grid, dim3(kBlock), 0, st, src, n, ncols, Q, R,
                           static_cast<double*>(dst), ldd, flags, absorbed);
    else
        hipLaunchKernelGGL(adjust_kernel<float>, grid, dim3(kBlock), 0, st, src, n, ncols, Q, R,
                           static_cast<float*>(dst), ldd, flags, absorbed);
    return hipGetLastError();
}

}  // namespace vk
