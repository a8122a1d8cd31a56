// kdev.h — what the gfx950 kernel files (kernels.hip, atax_team.hip, vec.hip,
// pcg.hip, probit.hip, ingest.hip, assoc.hip) share: the row-pair loads of X
// and launch_xe over its three storages, the block sums and the finish of a
// two-stage reduction, the CG decision, slot_sum, the counter-based
// generators and the prelude's per-element expressions.  Internal to
// libvampomi.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace vk {

constexpr int kBlock = 256;  // 4 waves of 64
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One launch for the three storages of X: k64, k32 and k16 are the same body
// over double, float and 16-bit columns (the family's three __global__
// wrappers); the one of the shard's element type gets (X, ld, args...), with
// the timing events in its dispatch packet (hipExtLaunchKernelGGL: written by
// the kernel's own dispatch, no extra marker packets around it).
template <class K64, class K32, class K16, class... A>
static void launch_xe(const Shard& s, K64 k64, K32 k32, K16 k16, dim3 grid, dim3 block, hipStream_t st,
                      const Timing& tm, A... args) {
    if (s.u16)
        hipExtLaunchKernelGGL(k16, grid, block, 0, st, tm.start, tm.stop, 0, s.x16(), s.ld, args...);
    else if (s.f32)
        hipExtLaunchKernelGGL(k32, grid, block, 0, st, tm.start, tm.stop, 0, s.x32(), s.ld, args...);
    else
        hipExtLaunchKernelGGL(k64, grid, block, 0, st, tm.start, tm.stop, 0, s.x64(), s.ld, args...);
}

typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef uint16_t v2h __attribute__((ext_vector_type(2)));  // (a ushort2: two fixed-point rows in one dword)

// A row pair of a column of X: one 16-byte load of a double column, one
// 8-byte load of a float column, or one 4-byte load of a 16-bit fixed-point
// column (uint16_t k, value k * 2^-16).  The lane owns the same two rows in
// every case, so every sum over a column runs in the same order for all
// storages.  The pair stays as loaded (xpair_t) until it is used and is widened
// there (widen: exact; nothing for doubles; (double)k * 2^-16 is an exact
// product, a power-of-two scaling of an integer below 2^16), so a load issued
// ahead is not waited for by a conversion.  NT: nontemporal (the streaming
// passes)
template <class E>
struct XPair;
template <>
struct XPair<double> {
    typedef v2d type;
};
template <>
struct XPair<float> {
    typedef v2f type;
};
template <>
struct XPair<uint16_t> {
    typedef v2h type;
};
template <class E>
using xpair_t = typename XPair<E>::type;

template <bool NT, class E>
__device__ __forceinline__ xpair_t<E> ldx(const E* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const xpair_t<E>*>(p));
    return *reinterpret_cast<const xpair_t<E>*>(p);
}
// a row pair of an N-vector (16-byte aligned: ld-padded vectors, even rows)
__device__ __forceinline__ v2d ld2(const double* p) { return *reinterpret_cast<const v2d*>(p); }
__device__ __forceinline__ v2d widen(v2d x) { return x; }
__device__ __forceinline__ v2d widen(v2f x) { return v2d{(double)x.x, (double)x.y}; }
__device__ __forceinline__ v2d widen(v2h x) { return v2d{(double)x.x * 0x1p-16, (double)x.y * 0x1p-16}; }
// one stored element widened (the team operator keeps single rows in its ring)
__device__ __forceinline__ double widen1(double x) { return x; }
__device__ __forceinline__ double widen1(float x) { return (double)x; }
__device__ __forceinline__ double widen1(uint16_t x) { return (double)x * 0x1p-16; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;  // butterfly: every lane holds the same value
}

// Fused finish of a two-stage reduction.  Thread 0 of every block publishes
// its per-block partials with red_put (agent-coherent, write-through stores);
// red_finish drains them (s_waitcnt) and takes a ticket; the LAST block to
// arrive sums the partials in block order, exactly as a separate one-block
// sum kernel would (so results are bitwise those of the two-launch form),
// writes out[0..nq) (device memory or mapped host memory) and re-arms the
// ticket.  No __threadfence: an agent-scope fence writes back the XCD's whole
// L2 (every dirty line of the vectors the kernel just updated), which made
// the fused kernels slower than the two launches (MI355X_MICROARCH.md,
// handoff-flag: drained sc1 payload, then the flag).
__device__ __forceinline__ void red_put(const RedOut& ro, int64_t idx, double v) {
    __hip_atomic_store(ro.part + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0 of every block: after thread 0 has red_put this block's K values at
// part[block*K + k], take the ticket; the last block sums the blocks' values
// in block order per k (lanes stride the blocks, then a butterfly) into
// ro.out[0..K) and re-arms the ticket.  Call from wave 0 only.
template <int K>
__device__ __forceinline__ void ticket_sum_blocks(const RedOut& ro) {
    const int lane = threadIdx.x & 63;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(ro.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, 0, 64);
    if (old != gridDim.x - 1) return;
    const int nblk = (int)gridDim.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int b = lane; b < nblk; b += 64)
            t += __hip_atomic_load(ro.part + (int64_t)b * K + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = wave_sum(t);
        if (lane == 0) ro.out[k] = t;
    }
    if (lane == 0) __hip_atomic_store(ro.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread: the host loop of vamp::precondCG_solver after each step's sums
// red[3k..3k+2] = <r,z>, <r,r>, <v,mu> of system k, applied to the state s
// (in place; nothing if the solve had stopped: s.any == 0).  Returns whether
// the step ran (s.any on entry).
__device__ inline bool cg_decide_into(CgState& s, const double* red, int it, int mask) {
    const bool ran = s.any != 0;  // a step queued after the solve stopped decides (and publishes) nothing
    if (ran) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < kMaxRhs; ++k) {
            if (k >= s.K || !s.active[k]) continue;
            if (!((mask >> k) & 1)) {  // not this step's: unchanged, still running
                any = 1;
                continue;
            }
            s.iters[k] = it + 1 + s.off[k];
            const double rz_new = red[3 * k], rr = red[3 * k + 1], vmu = red[3 * k + 2];
            if (s.onsager[k]) {  // :708-726
                const double ons = s.gam2 * vmu;
                const double rel = ons != 0 ? fabs((ons - s.prev_ons[k]) / ons) : 1;
                if (rel < 1e-8) {
                    s.active[k] = 0;
                    continue;
                }
                s.prev_ons[k] = ons;
            }
            // :731 pow(rz, -1): the correctly rounded reciprocal; glibc's pow
            // differs from it by one ulp on ~0.1% of inputs (tests/powm1_check.c)
            double bt = 1.0 / s.rz[k];
            bt *= rz_new;                 // :736
            s.rz[k] = rz_new;
            const double rel_err = sqrt(rr) / sqrt(s.vv[k]);  // :742-744
            if (rel_err < s.tol) {                            // :750
                s.active[k] = 0;
                continue;
            }
            s.beta[k] = bt;
            if (s.iters[k] >= s.maxit) {  // the solver's loop bound (:697)
                s.active[k] = 0;
                continue;
            }
            any = 1;
        }
        s.any = any;
    }
    return ran;
}

// the decided state s to the host: pack: *flag receives the decision as one
// word (cg_pack), no mirror; else the mirror slot (it & 1) then the flag
__device__ inline void cg_publish(const CgState& s, bool ran, int it, CgMirror* mirror, unsigned long long* flag,
                                  unsigned long long seq, int pack, bool pre = false) {
    if (pack) {  // one word, one system-scope store: nothing to order
        if (flag && ran)
            __hip_atomic_store(flag, cg_pack(seq, s.any, s.iters[0], s.iters[1]) | (pre ? kCgPackPre : 0ull),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // the mirror (mapped host memory) written through and drained, then the
    // flag: the host reads the mirror after the flag (no release fence, which
    // would write back this XCD's whole L2 first)
    if (mirror) {
        CgMirror* m = mirror + (it & 1);  // (it >= 0 whenever a mirror is given)
        __hip_atomic_store(&m->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&m->any, s.any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
        for (int k = 0; k < kMaxRhs; ++k)
            __hip_atomic_store(&m->iters[k], s.iters[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (flag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// s: the state as *cs holds it (read by the caller in one burst); it is
// written back once (a chain of dependent device loads and stores otherwise:
// this runs at the end of every CG step), then published
__device__ inline void cg_decide_from(CgState s, CgState* cs, const double* red, int it, CgMirror* mirror,
                                      unsigned long long* flag, unsigned long long seq, int mask, int pack = 0,
                                      bool pre = false) {
    const bool ran = cg_decide_into(s, red, it, mask);
    if (ran) *cs = s;
    cg_publish(s, ran, it, mirror, flag, seq, pack, pre);
}

__device__ inline void cg_decide_body(CgState* cs, const double* red, int it, CgMirror* mirror, unsigned long long* flag,
                                      unsigned long long seq, int mask, int pack = 0) {
    const CgState s = *cs;
    double r[3 * kMaxRhs];
#pragma unroll
    for (int q = 0; q < 3 * kMaxRhs; ++q) r[q] = q < 3 * s.K ? red[q] : 0.0;
    cg_decide_from(s, cs, r, it, mirror, flag, seq, mask, pack);
}

// ---- block sums and the finish of a two-stage reduction (red_put above) ----
// sum over a 256-thread block; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* lds4) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds4[w] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// red_put (above) publishes a block's partials; red_finish (below) takes the
// ticket and sums them in block order (the protocol is described at red_put).

// Block sums of nq <= NQ values at once, published with red_put at
// part[base + q]: every wave reduces all values in registers, ONE barrier,
// then thread q adds the four wave sums in wave order — the additions of nq
// separate block_sum calls, with one barrier instead of 2*nq.
template <int NQ>
__device__ __forceinline__ void block_put_sums(double (&v)[NQ], int nq, const RedOut& ro, int64_t base) {
    __shared__ double lds[4 * NQ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q < nq) v[q] = wave_sum(v[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q < nq) lds[w * NQ + q] = v[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        const int q = threadIdx.x;
        red_put(ro, base + q, ((lds[q] + lds[NQ + q]) + lds[2 * NQ + q]) + lds[3 * NQ + q]);
    }
}

// (red_ticket, red_ticket_nowait, red_final and red_finish are static, not
// inline: the inline hint changes the inliner's choices and with them scalar
// instructions of the callers, profiles/kernel_split.md)
// (red_finish's halves, for a launch that finishes two reductions: dots2)
// every partial store of this block is acknowledged before the ticket moves;
// true in the block that brings it to nblocks (block-uniform)
[[maybe_unused]] static __device__ bool red_ticket(const RedOut& ro, int nblocks) {
    __shared__ int is_last;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __syncthreads();
    if (threadIdx.x == 0)
        is_last = __hip_atomic_fetch_add(ro.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                  (unsigned)nblocks - 1;
    __syncthreads();
    return is_last;
}

// red_ticket for a block that published nothing: no wait for its own stores
// (block-uniform; the barrier: every wave of the block is past its start)
[[maybe_unused]] static __device__ bool red_ticket_nowait(const RedOut& ro, int nblocks) {
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0)
        is_last = __hip_atomic_fetch_add(ro.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                  (unsigned)nblocks - 1;
    __syncthreads();
    return is_last;
}

// the last block's sums of the nblk blocks' partials at ro.part, into ro.out
// (and keep); finish: then re-arm the ticket and store the host flag
[[maybe_unused]] static __device__ void red_final(const RedOut& ro, int nq, int nblk, double* keep, bool finish) {
    __shared__ double lds[4 * 8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int q0 = 0; q0 < nq; q0 += 8) {
        const int nc = nq - q0 < 8 ? nq - q0 : 8;
        double s[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) s[c] = 0.0;
        for (int b = threadIdx.x; b < nblk; b += kBlock) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < nc)
                    s[c] += __hip_atomic_load(ro.part + (int64_t)b * nq + q0 + c, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < nc) s[c] = wave_sum(s[c]);
        __syncthreads();  // lds of the previous round consumed
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < nc) lds[w * 8 + c] = s[c];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int c = 0; c < nc; ++c) {
                const double v = ((lds[c] + lds[8 + c]) + lds[16 + c]) + lds[24 + c];
                const int q = q0 + c;
                double* dst = ro.out2 && q >= ro.split ? ro.out2 + (q - ro.split) : ro.out + q;
                if (ro.flag || !finish)  // mapped host memory: written through, drained before the flag below
                    __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else
                    *dst = v;
                if (keep) keep[q0 + c] = v;
            }
    }
    if (finish && threadIdx.x == 0) {
        __hip_atomic_store(ro.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // host completion flag, after the results above have landed (drained
        // write-through stores: no release fence, which would first write back
        // this XCD's whole L2, MI355X_MICROARCH.md)
        if (ro.flag) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ro.flag, ro.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The last block sums up to 8 results per round: each thread adds its
// blocks' partials of every result (blocks in order), then each result is
// wave-reduced and the four wave sums added in wave order — per result, the
// operations of block_sum, so the sums are bitwise those of one block_sum per
// result, with one barrier round per 8 results instead of one per result.
// Returns true in the last block (after out[] is written; thread 0 wrote it).
// keep (LDS, may be null): thread 0 also leaves the results there (a caller
// that goes on with them in thread 0 then reads no global memory).
[[maybe_unused]] static __device__ bool red_finish(const RedOut& ro, int nq, double* /*lds4*/, double* keep = nullptr) {
    if (!red_ticket(ro, (int)gridDim.x)) return false;
    red_final(ro, nq, (int)gridDim.x, keep, true);
    return true;
}

// The per-slot A d partials summed over the slots: a workgroup takes 128
// samples of one system (two per lane, 16-byte loads); wave w sums the slots
// [w*ns/4, (w+1)*ns/4) in order with up to 32 loads in flight, wave 0 adds
// the four wave sums in order.  cg_update's one-rank form (cg_update_kernel,
// c.adpart) sums in exactly this order, so the two paths agree bit for bit.
// (Every load of a round is issued before the first add: the adds stay in
// slot order, so the round size changes the latency, not the bits.)
// W: the largest round (32: 128 VGPRs of loads in flight; 8 for the few slots
// of the large-N plans, so that cg_update's workgroups are not held to one per
// CU by a round they never run)
template <int W = 32>
__device__ __forceinline__ v2d slot_sum(const double* src, int64_t ss, int t0, int t1) {
    v2d acc = {0.0, 0.0};
    int t = t0;
    for (; W >= 32 && t + 32 <= t1; t += 32) {  // (C2, team of 2: 128 slots, 32 per wave, one round trip)
        v2d x[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) x[u] = *reinterpret_cast<const v2d*>(src + (t + u) * ss);
#pragma unroll
        for (int u = 0; u < 32; ++u) acc += x[u];
    }
    for (; W >= 16 && t + 16 <= t1; t += 16) {
        v2d x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = *reinterpret_cast<const v2d*>(src + (t + u) * ss);
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += x[u];
    }
    for (; t + 8 <= t1; t += 8) {
        v2d x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const v2d*>(src + (t + u) * ss);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; t < t1; ++t) acc += *reinterpret_cast<const v2d*>(src + t * ss);
    return acc;
}

// ---- the counter-based generators (synthetic data, the probes, probit_p1) ----
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// Irwin-Hall(12) dyadic normal draw; same specification as the oracle's
// orc_gauss_dyadic (oracle/vamp_oracle.c), exactly representable.
__device__ __forceinline__ double gauss_dyadic(uint64_t seed, int64_t i, int64_t j) {
    const uint64_t k = splitmix64(splitmix64(seed ^ 0x4741555353ULL) + (uint64_t)i);
    uint64_t acc = 0;
#pragma unroll
    for (uint64_t t = 0; t < 3; ++t) {
        const uint64_t h = splitmix64(k ^ (((uint64_t)j << 2) | t));
        acc += (h & 0xFFFFULL) + ((h >> 16) & 0xFFFFULL) + ((h >> 32) & 0xFFFFULL) + (h >> 48);
    }
    return (double)(2 * acc + 12) * (1.0 / 131072.0) - 6.0;
}

__device__ __forceinline__ int bern_bit(uint64_t seed, int it, int64_t gidx) {
    const uint64_t k = splitmix64(seed ^ 0xB5AD4ECEDA1CE2A9ULL);
    const uint64_t h = splitmix64(k ^ (((uint64_t)(uint32_t)it << 40) ^ (uint64_t)gidx));
    return (int)(h >> 63);
}

// The prelude at marker i (prelude_kernel in vec.hip, prelude_cg_init_kernel
// in pcg.hip): r2, v, the probes bern and bern_next and the zero starts, from
// the loaded x1[i], r1[i], atxy[i] and the scalars (p's, or the device's).
// vv and bn: what went to p.v[i] and p.bern[i].
__device__ __forceinline__ void prelude_at(const Prelude& p, int64_t i, double x1, double r1, double atxy, double eta1,
                                           double gam1, double gam2, double gamw, double& vv, double& bn) {
    const double r2 = (eta1 * x1 - gam1 * r1) / gam2;  // lincomb_div's expression
    p.r2[i] = r2;
    vv = gamw * atxy + gam2 * r2;                      // axpby's
    p.v[i] = vv;
    bn = (double)(2 * bern_bit(p.seed, p.it, p.S + i) - 1) / p.sqrtMt;
    p.bern[i] = bn;
    if (p.bern_next) p.bern_next[i] = (double)(2 * bern_bit(p.seed, p.it + 1, p.S + i) - 1) / p.sqrtMt;
    if (p.zero[0]) p.zero[0][i] = 0.0;
    if (p.zero[1]) p.zero[1][i] = 0.0;
}

}  // namespace vk
