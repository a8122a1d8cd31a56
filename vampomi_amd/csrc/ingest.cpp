// ingest.cpp — libvampomi: how the methylation shard gets into HBM and back
// out.  The settings a load obeys (storage, NaN policy, row subset, covariate
// adjustment), the loaders (host block, file, generator), the conversion of
// each staged chunk (put_cols) and what the last load recorded.  Nothing here
// runs during a VAMP iteration or an association test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "ctx.h"

// ---------------------------------------------------------------------------
// what a load obeys: storage, NaN policy, row subset
// ---------------------------------------------------------------------------
extern "C" vampomi_status vampomi_set_storage(vampomi_ctx* c, int storage) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (storage != VAMPOMI_STORE_F64 && storage != VAMPOMI_STORE_F32 && storage != VAMPOMI_STORE_U16)
        return fail(VAMPOMI_ERR_ARG, "storage must be VAMPOMI_STORE_F64, VAMPOMI_STORE_F32 or VAMPOMI_STORE_U16");
    if (c->X) return fail(VAMPOMI_ERR_STATE, "the storage is fixed once the methylation shard is allocated");
    if (storage == VAMPOMI_STORE_U16 && c->adj_R)
        return fail(VAMPOMI_ERR_ARG, "covariate-adjusted values leave [0, 1]: VAMPOMI_STORE_U16 cannot hold them");
    c->storage = storage;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_get_storage(const vampomi_ctx* c, int* storage) {
    if (!c || !storage) return fail(VAMPOMI_ERR_ARG, "null argument");
    *storage = c->storage;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_set_meth_na(vampomi_ctx* c, int policy, double max_missing_frac) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (policy != VAMPOMI_NA_PASS && policy != VAMPOMI_NA_FATAL && policy != VAMPOMI_NA_MEAN)
        return fail(VAMPOMI_ERR_ARG, "the policy must be VAMPOMI_NA_PASS, VAMPOMI_NA_FATAL or VAMPOMI_NA_MEAN");
    if (!(max_missing_frac >= 0.0 && max_missing_frac <= 1.0))
        return fail(VAMPOMI_ERR_ARG, "max_missing_frac must lie in [0, 1]");
    if (c->X) return fail(VAMPOMI_ERR_STATE, "the NaN policy is fixed once the methylation shard is allocated");
    c->na_policy = policy;
    c->na_max_frac = max_missing_frac;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_get_meth_na(const vampomi_ctx* c, int* policy, double* max_missing_frac) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (policy) *policy = c->na_policy;
    if (max_missing_frac) *max_missing_frac = c->na_max_frac;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_set_row_subset(vampomi_ctx* c, int64_t N_file, const int64_t* rows, int64_t n) {
    if (!c || !rows) return fail(VAMPOMI_ERR_ARG, "null argument");
    if (c->X) return fail(VAMPOMI_ERR_STATE, "the row subset is fixed once the methylation shard is allocated");
    if (c->have_y || c->cov_C > 0)
        return fail(VAMPOMI_ERR_STATE, "set the row subset before the phenotype and the covariates");
    if (c->adj_R) return fail(VAMPOMI_ERR_STATE, "set the row subset before the covariate adjustment");
    if (N_file >= ((int64_t)1 << 31)) return fail(VAMPOMI_ERR_ARG, "row subset: N_file must be below 2^31");
    if (n != c->N)
        return fail(VAMPOMI_ERR_ARG, "row subset: n (" + std::to_string(n) + ") != the context's N (" +
                                         std::to_string(c->N) + "): open the context with N = n");
    if (n < 2 || n > N_file) return fail(VAMPOMI_ERR_ARG, "row subset: 2 <= n <= N_file");
    for (int64_t j = 0; j < n; ++j)
        if (rows[j] < 0 || rows[j] >= N_file || (j > 0 && rows[j] <= rows[j - 1]))
            return fail(VAMPOMI_ERR_ARG, "row subset: rows must be strictly ascending within [0, N_file) (entry " +
                                             std::to_string(j) + " is " + std::to_string(rows[j]) + ")");
    HIPCHK(hipSetDevice(c->device));
    if (!c->rows_dev && hipMalloc((void**)&c->rows_dev, (size_t)n * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        c->rows_dev = nullptr;
        return fail(VAMPOMI_ERR_OOM, "row subset");
    }
    const std::vector<int32_t> r32(rows, rows + n);
    HIPCHK(hipMemcpyAsync(c->rows_dev, r32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->rows_host.assign(rows, rows + n);
    c->N_file = N_file;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_get_row_subset(const vampomi_ctx* c, int64_t* N_file, int64_t* rows) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (N_file) *N_file = c->N_file;
    if (rows && c->N_file) std::memcpy(rows, c->rows_host.data(), c->rows_host.size() * sizeof(int64_t));
    return VAMPOMI_OK;
}

int64_t rows_in(const vampomi_ctx* c) { return c->N_file ? c->N_file : c->N; }

// ---------------------------------------------------------------------------
// covariate adjustment of the linear model: X and y are
// replaced at ingest by their residuals on span{1, Z}
// ---------------------------------------------------------------------------
// Modified Gram-Schmidt over the intercept, then Z's columns in order: each
// vector is orthogonalised twice against the accepted ones, every sum in long
// double, and rounded to double once it is normalised.  A column whose norm is
// 0, or at most 1e-8 of it after the orthogonalisation, is dropped.
extern "C" vampomi_status vampomi_adjust_basis(const double* Z, int64_t n, int C, int64_t ld_in, double* Q, int* R,
                                               int* dropped) {
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    if (n < 1 || !Q || !R || (C > 0 && (!Z || !dropped || ld_in < n))) return fail(VAMPOMI_ERR_ARG, "bad covariate table");
    for (int i = 0; i < C; ++i)
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(Z[(int64_t)i * ld_in + j]))
                return fail(VAMPOMI_ERR_ARG, "covariate " + std::to_string(i) + ", row " + std::to_string(j) +
                                                 " is not finite");
    std::vector<long double> v((size_t)n);
    const auto norm = [&] {
        long double s = 0.0L;
        for (int64_t j = 0; j < n; ++j) s += v[(size_t)j] * v[(size_t)j];
        return std::sqrt(s);
    };
    int r = 0;
    for (int i = -1; i < C; ++i) {  // -1: the intercept
        for (int64_t j = 0; j < n; ++j) v[(size_t)j] = i < 0 ? 1.0L : (long double)Z[(int64_t)i * ld_in + j];
        const long double before = norm();
        bool keep = before > 0.0L;
        if (keep) {
            for (int pass = 0; pass < 2; ++pass)
                for (int k = 0; k < r; ++k) {
                    const double* q = Q + (size_t)k * (size_t)n;
                    long double d = 0.0L;
                    for (int64_t j = 0; j < n; ++j) d += (long double)q[j] * v[(size_t)j];
                    for (int64_t j = 0; j < n; ++j) v[(size_t)j] -= d * (long double)q[j];
                }
            const long double after = norm();
            keep = after > 1e-8L * before;
            if (keep) {
                double* q = Q + (size_t)r * (size_t)n;
                for (int64_t j = 0; j < n; ++j) q[j] = (double)(v[(size_t)j] / after);
                ++r;
            }
        }
        if (i >= 0) dropped[i] = keep ? 0 : 1;
    }
    *R = r;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_set_adjust(vampomi_ctx* c, const double* Z, int C, int64_t ld_in) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    if (C > 0 && (!Z || ld_in < c->N)) return fail(VAMPOMI_ERR_ARG, "bad covariate table");
    if (c->u16())
        return fail(VAMPOMI_ERR_ARG, "covariate-adjusted values leave [0, 1]: VAMPOMI_STORE_U16 cannot hold them");
    if (c->X) return fail(VAMPOMI_ERR_STATE, "the adjustment is fixed once the methylation shard is allocated");
    if (c->have_y) return fail(VAMPOMI_ERR_STATE, "set the adjustment before the phenotype");
    std::vector<double> Q((size_t)(C + 1) * (size_t)c->N);
    std::vector<int> dropped((size_t)C, 0);
    int R = 0;
    STCHK(vampomi_adjust_basis(Z, c->N, C, ld_in, Q.data(), &R, dropped.data()));
    Q.resize((size_t)R * (size_t)c->N);
    c->adj_Q.swap(Q);
    c->adj_dropped.swap(dropped);
    c->adj_R = R;
    c->adj_C = C;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_read_adjust(vampomi_ctx* c, const char* path, int C) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    if (C == 0) return vampomi_set_adjust(c, nullptr, 0, c->N);
    const int64_t Nin = c->N_file ? c->N_file : c->N;
    std::vector<double> raw((size_t)C * (size_t)Nin);
    STCHK(vampomi_parse_covariates(path, Nin, C, 0, raw.data()));
    if (!c->N_file) return vampomi_set_adjust(c, raw.data(), C, c->N);
    std::vector<double> Z((size_t)C * (size_t)c->N);
    for (int j = 0; j < C; ++j)
        for (int64_t i = 0; i < c->N; ++i)
            Z[(size_t)j * c->N + i] = raw[(size_t)j * c->N_file + c->rows_host[(size_t)i]];
    return vampomi_set_adjust(c, Z.data(), C, c->N);
}

extern "C" vampomi_status vampomi_get_adjust(const vampomi_ctx* c, int* R, int* dropped, double* Q) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (R) *R = c->adj_R;
    if (dropped) std::copy(c->adj_dropped.begin(), c->adj_dropped.end(), dropped);
    if (Q && c->adj_R) std::memcpy(Q, c->adj_Q.data(), c->adj_Q.size() * sizeof(double));
    return VAMPOMI_OK;
}

void adjust_phen(const vampomi_ctx* c, std::vector<double>& y) {
    if (!c->adj_R) return;
    const size_t n = (size_t)c->N;
    std::vector<long double> r(y.begin(), y.end());
    for (int k = 0; k < c->adj_R; ++k) {
        const double* q = c->adj_Q.data() + (size_t)k * n;
        long double d = 0.0L;
        for (size_t j = 0; j < n; ++j) d += (long double)q[j] * (long double)y[j];
        for (size_t j = 0; j < n; ++j) r[j] -= d * (long double)q[j];
    }
    for (size_t j = 0; j < n; ++j) y[j] = (double)r[j];
}

// ---------------------------------------------------------------------------
// one load
// ---------------------------------------------------------------------------
// the bytes of one staging chunk of an ingest (256 MB; VAMPOMI_IO_CHUNK_BYTES:
// tuning experiments, and tests of the chunk boundaries at small shapes)
static int64_t io_chunk_bytes() {
    const char* env = std::getenv("VAMPOMI_IO_CHUNK_BYTES");
    const int64_t v = env ? std::atoll(env) : 0;
    return v >= 4096 ? v : (int64_t)256 << 20;
}

namespace {

// a device buffer that a load grows on demand
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
};

// at least `need` bytes in b (what it held is gone); what: the message of a failure
vampomi_status grow(vampomi_ctx* c, DevBuf& b, size_t need, const char* what) {
    if (b.cap >= need) return VAMPOMI_OK;
    HIPCHK(hipStreamSynchronize(c->st));  // the launches that use the old buffer
    if (b.p) (void)hipFree(b.p);
    b = DevBuf{};
    if (hipMalloc(&b.p, need) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(VAMPOMI_ERR_OOM, what);
    }
    b.cap = need;
    return VAMPOMI_OK;
}

// One load of the shard, from input elements of in_es bytes (8: doubles, 4:
// floats, 2: 16-bit fixed point; 0: no input, the generator).  begin() ..
// put_cols() per chunk .. end(); what only the load uses on the device lives
// here and is freed on every way out.
struct IngestScope {
    vampomi_ctx* const c;
    const int in_es;
    // whether the load looks for missing values: a policy other than pass, and
    // an input that can hold a NaN
    const bool look;
    DevBuf stage;  // a chunk as the input holds it (conversions only)
    DevBuf work;   // an adjusted load's fp64 chunk of packed columns, between the conversion and vk::adjust_cols
    // an adjusted load (c->adj_R > 0; else nothing is allocated and nothing
    // launched): Q, and the absorbed flags and counter that vk::adjust_cols fills
    double* adj_Q = nullptr;
    uint8_t* adj_flags = nullptr;
    unsigned long long* adj_cnt = nullptr;

    IngestScope(vampomi_ctx* c_, int in_es_)
        : c(c_), in_es(in_es_), look(c_->na_policy != VAMPOMI_NA_PASS && (in_es_ == 8 || in_es_ == 4)) {}
    IngestScope(const IngestScope&) = delete;
    ~IngestScope() {
        if (!stage.p && !work.p && !adj_Q && !adj_flags && !adj_cnt) return;
        (void)hipStreamSynchronize(c->st);
        for (void* p : {stage.p, work.p, (void*)adj_Q, (void*)adj_flags, (void*)adj_cnt})
            if (p) (void)hipFree(p);
    }
    vampomi_status begin();
    vampomi_status put_cols(int64_t i0, int64_t nc, const void* src, int64_t ld_in);
    vampomi_status end();
};

// X allocated; the last load's records forgotten on the host and, where this
// load will write them, zeroed on the device (qrec, na_rec and na_cnt live as
// long as the context); the adjustment's basis uploaded
vampomi_status IngestScope::begin() {
    if (!c->X) {
        const size_t bytes = (size_t)std::max<int64_t>(c->M, 1) * (size_t)c->ld * (size_t)c->esize();
        const hipError_t e = hipMalloc(&c->X, bytes);
        if (e != hipSuccess)
            return fail(VAMPOMI_ERR_OOM, "hipMalloc(" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    }
    c->q_clamped = 0;
    c->q_max_err = 0.0;
    if (c->u16()) {
        if (!c->qrec && hipMalloc((void**)&c->qrec, sizeof(vk::QuantRec)) != hipSuccess) {
            (void)hipGetLastError();
            c->qrec = nullptr;
            return fail(VAMPOMI_ERR_OOM, "quantisation record");
        }
        HIPCHK(hipMemsetAsync(c->qrec, 0, sizeof(vk::QuantRec), c->st));
        HIPCHK(hipMemsetAsync(&c->qrec->first, 0xff, sizeof(unsigned long long), c->st));
    }
    c->na_missing = c->na_markers = c->na_masked = 0;
    c->na_per_marker.clear();
    if (look) {
        const size_t cb = (size_t)std::max<int64_t>(c->M, 1) * sizeof(int64_t);
        if ((!c->na_rec && hipMalloc((void**)&c->na_rec, sizeof(vk::NaRec)) != hipSuccess) ||
            (!c->na_cnt && hipMalloc((void**)&c->na_cnt, cb) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(VAMPOMI_ERR_OOM, "missing-value counters");
        }
        HIPCHK(hipMemsetAsync(c->na_rec, 0, sizeof(vk::NaRec), c->st));
        HIPCHK(hipMemsetAsync(&c->na_rec->first, 0xff, sizeof(unsigned long long), c->st));
        HIPCHK(hipMemsetAsync(c->na_cnt, 0, cb, c->st));
    }
    c->adj_absorbed = 0;
    c->adj_flags.clear();
    if (c->adj_R) {
        const size_t qb = c->adj_Q.size() * sizeof(double), fb = (size_t)std::max<int64_t>(c->M, 1);
        if (hipMalloc((void**)&adj_Q, qb) != hipSuccess || hipMalloc((void**)&adj_flags, fb) != hipSuccess ||
            hipMalloc((void**)&adj_cnt, sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VAMPOMI_ERR_OOM, "covariate basis on the device");
        }
        HIPCHK(hipMemcpyAsync(adj_Q, c->adj_Q.data(), qb, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(adj_flags, 0, fb, c->st));
        HIPCHK(hipMemsetAsync(adj_cnt, 0, sizeof(unsigned long long), c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return VAMPOMI_OK;
}

// Columns [i0, i0 + nc) of the shard from a host block of nc columns of
// in_es-byte elements, column stride ld_in elements (with a row subset a
// column holds N_file of them).  All on the context's stream, so the caller
// may reuse src once the stream has passed this point.
vampomi_status IngestScope::put_cols(int64_t i0, int64_t nc, const void* src, int64_t ld_in) {
    if (nc <= 0) return VAMPOMI_OK;
    char* const shard = (char*)c->X + (size_t)i0 * (size_t)c->ld * (size_t)c->esize();
    // (a) where the block's values go: into the shard, or, on an adjusted
    // context, into the fp64 work block (the row gather and the NaN fill come
    // first), which vk::adjust_cols then empties into the shard: one rounding
    // into F32
    void* dst = shard;
    int dst_ek = c->ek();
    int64_t ldd = c->ld;
    if (c->adj_R) {
        STCHK(grow(c, work, (size_t)nc * (size_t)c->N * 8, "device work block of the covariate adjustment"));
        dst = work.p;
        dst_ek = vk::kXF64;
        ldd = c->N;
    }
    const int src_ek = in_es == 2 ? vk::kXU16 : in_es == 4 ? vk::kXF32 : vk::kXF64;
    const size_t es = (size_t)in_es;
    if (src_ek == dst_ek && !c->N_file && !look) {
        // (b) the target's element type, every row, no NaN to look for: a strided copy, no staging hop
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldd * es, src, (size_t)ld_in * es, (size_t)c->N * es, (size_t)nc,
                                hipMemcpyHostToDevice, c->st));
    } else {
        // (c) the block staged on the device as it is, and one kernel that
        // converts, keeps the subset's rows and, under a NaN policy, does the
        // policy's work
        const int64_t Nin = rows_in(c);
        const int32_t* rows = c->N_file ? c->rows_dev : nullptr;
        STCHK(grow(c, stage, (size_t)nc * (size_t)Nin * es, "device staging buffer of the storage conversion"));
        HIPCHK(hipMemcpy2DAsync(stage.p, (size_t)Nin * es, src, (size_t)ld_in * es, (size_t)Nin * es, (size_t)nc,
                                hipMemcpyHostToDevice, c->st));
        if (look)
            HIPCHK(vk::na_ingest_cols(stage.p, src_ek, Nin, rows, c->N, nc, dst, dst_ek, ldd, Nin, c->S + i0,
                                      c->na_policy, c->na_max_frac, c->na_cnt + i0, c->na_rec, c->qrec, c->st));
        else
            HIPCHK(vk::convert_cols(stage.p, src_ek, Nin, rows, c->N, nc, dst, dst_ek, ldd, Nin, c->S + i0, c->qrec,
                                    c->st));
    }
    // (d)
    if (c->adj_R)
        HIPCHK(vk::adjust_cols((const double*)work.p, c->N, nc, adj_Q, c->adj_R, shard, c->ek(), c->ld, adj_flags + i0,
                               adj_cnt, c->st));
    return VAMPOMI_OK;
}

// The records read back: missing values first (of a NaN and a value out of
// range the NaN is reported), then the quantisation, then the adjustment.
// Missing entries under VAMPOMI_NA_FATAL (VAMPOMI_ERR_NAN_METH) and entries
// that 16 bits cannot hold (VAMPOMI_ERR_RANGE) fail the load and leave the
// context without X.  Then the pad rows and the marker statistics.
vampomi_status IngestScope::end() {
    const unsigned long long nin = (unsigned long long)rows_in(c);
    const auto where = [&](unsigned long long at) {  // (the file's row)
        return "marker " + std::to_string((long long)(at / nin)) + ", row " + std::to_string((long long)(at % nin));
    };
    if (look) {
        vk::NaRec r{};
        HIPCHK(hipMemcpyAsync(&r, c->na_rec, sizeof r, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (r.missing && c->na_policy == VAMPOMI_NA_FATAL) {
            c->have_X = false;
            return fail(VAMPOMI_ERR_NAN_METH, std::to_string(r.missing) + " missing methylation value(s) (NaN); the "
                                              "first is " + where(r.first));
        }
        if (r.missing) {
            c->na_per_marker.resize((size_t)c->M);
            HIPCHK(hipMemcpyAsync(c->na_per_marker.data(), c->na_cnt, (size_t)c->M * sizeof(int64_t),
                                  hipMemcpyDeviceToHost, c->st));
            HIPCHK(hipStreamSynchronize(c->st));
        }
        c->na_missing = (int64_t)r.missing;
        c->na_markers = (int64_t)r.markers;
        c->na_masked = (int64_t)r.masked;
    }
    if (c->u16()) {
        vk::QuantRec r{};
        HIPCHK(hipMemcpyAsync(&r, c->qrec, sizeof r, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (r.rejected) {
            c->have_X = false;
            return fail(VAMPOMI_ERR_RANGE,
                        std::to_string(r.rejected) + " methylation value(s) cannot be stored as 16-bit fixed point (NaN, "
                        "infinite, below 0 or above 1); the first is " + where(r.first));
        }
        c->q_clamped = (int64_t)r.clamped;
        std::memcpy(&c->q_max_err, &r.max_err, sizeof(double));
    }
    if (c->adj_R) {
        unsigned long long n = 0;
        c->adj_flags.assign((size_t)c->M, 0);
        HIPCHK(hipMemcpyAsync(&n, adj_cnt, sizeof n, hipMemcpyDeviceToHost, c->st));
        if (c->M > 0)
            HIPCHK(hipMemcpyAsync(c->adj_flags.data(), adj_flags, (size_t)c->M, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        c->adj_absorbed = (int64_t)n;
    }
    const size_t es = (size_t)c->esize();
    if (c->ld > c->N && c->M > 0)
        HIPCHK(hipMemset2DAsync((char*)c->X + (size_t)c->N * es, (size_t)c->ld * es, 0, (size_t)(c->ld - c->N) * es,
                                (size_t)c->M, c->st));
    // compute_markers_statistics with nonas = N (read_phen asserts N rows, src/data.cpp:85)
    HIPCHK(vk::marker_stats(c->shard(), (double)c->N, c->alpha_scale, c->mave, c->msig, c->st));
    STCHK(sync_stream(c, c->st));
    c->have_X = true;
    return VAMPOMI_OK;
}

struct FdGuard {
    int fd;
    ~FdGuard() {
        if (fd >= 0) ::close(fd);
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// the loaders
// ---------------------------------------------------------------------------
// a host shard of doubles (in_es 8), floats (4) or 16-bit fixed point (2), in
// chunks of about 256 MB where it has to be converted (put_cols' staging
// buffer)
static vampomi_status load_host(vampomi_ctx* c, const void* X, int64_t ld_in, int in_es) {
    if (!c || (!X && c->M > 0) || ld_in < rows_in(c)) return fail(VAMPOMI_ERR_ARG, "invalid host shard");
    HIPCHK(hipSetDevice(c->device));
    IngestScope load(c, in_es);
    STCHK(load.begin());
    const int64_t chunk = (int64_t)in_es == c->esize() && !c->N_file && !load.look && !c->adj_R
                              ? std::max<int64_t>(c->M, 1)
                              : std::max<int64_t>(1, io_chunk_bytes() / (rows_in(c) * in_es));
    for (int64_t i0 = 0; i0 < c->M; i0 += chunk)
        STCHK(load.put_cols(i0, std::min(chunk, c->M - i0), (const char*)X + (size_t)i0 * (size_t)ld_in * in_es,
                            ld_in));
    return load.end();
}

extern "C" vampomi_status vampomi_load_meth_host(vampomi_ctx* c, const double* X, int64_t ld_in) {
    return load_host(c, X, ld_in, 8);
}

extern "C" vampomi_status vampomi_load_meth_host_u16(vampomi_ctx* c, const uint16_t* X, int64_t ld_in) {
    return load_host(c, X, ld_in, 2);
}

extern "C" vampomi_status vampomi_load_meth_host_f32(vampomi_ctx* c, const float* X, int64_t ld_in) {
    return load_host(c, X, ld_in, 4);
}

// [off, off + want) of fd into dst, split over nt reader threads (page cache
// and NVMe both need several requests in flight to stream at full rate)
static bool pread_parallel(int fd, char* dst, size_t want, off_t off, int nt) {
    if (nt <= 1 || want < ((size_t)8 << 20)) nt = 1;
    const size_t per = ((want + nt - 1) / nt + 4095) & ~(size_t)4095;
    std::atomic<bool> ok{true};
    auto work = [&](size_t lo, size_t hi) {
        size_t got = 0;
        while (lo + got < hi) {
            const ssize_t r = ::pread(fd, dst + lo + got, hi - lo - got, off + (off_t)(lo + got));
            if (r <= 0) {
                ok = false;
                return;
            }
            got += (size_t)r;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) {
        const size_t lo = (size_t)t * per;
        if (lo < want) th.emplace_back(work, lo, std::min(want, lo + per));
    }
    work(0, std::min(want, per));
    for (auto& x : th) x.join();
    return ok;
}

// read_methylation_data (src/data.cpp:116-153): this rank's M*N elements of
// in_es bytes (8: the reference's doubles; 4: floats, 2: little-endian uint16
// k meaning k * 2^-16, in the same marker-major layout) at byte offset
// S*N*in_es (64-bit offsets: the reference's int i*N
// overflows past 2^31 elements), streamed through three pinned 256 MB staging
// buffers: the parallel read of chunk k+1 overlaps the host-to-device copy of
// chunk k, which lands directly in the ld-padded column layout, or, where the
// file's element type is not the storage's, in a device staging buffer that a
// conversion kernel empties into it (put_cols).  Marker statistics follow on
// the device (IngestScope::end).
static vampomi_status load_file(vampomi_ctx* c, const char* path, int in_es) {
    if (!c || !path) return fail(VAMPOMI_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const FdGuard file{::open(path, O_RDONLY)};
    if (file.fd < 0) return fail(VAMPOMI_ERR_IO, std::string("cannot open methylation file ") + path);
    IngestScope load(c, in_es);
    STCHK(load.begin());
    const size_t colb = (size_t)rows_in(c) * (size_t)in_es;
    const size_t chunk_cols = std::max<size_t>(1, (size_t)io_chunk_bytes() / colb);
    const char* env = std::getenv("VAMPOMI_IO_THREADS");
    const int nt = env ? std::max(1, std::atoi(env)) : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    constexpr int NB = 3;
    char* pin[NB] = {};
    hipEvent_t done[NB];
    bool used[NB] = {};
    for (int b = 0; b < NB; ++b) {
        if (hipHostMalloc((void**)&pin[b], chunk_cols * colb, hipHostMallocDefault) != hipSuccess) {
            for (int k = 0; k < b; ++k) (void)hipHostFree(pin[k]);
            return fail(VAMPOMI_ERR_OOM, "pinned staging buffer");
        }
        (void)hipEventCreate(&done[b]);
    }
    vampomi_status st = VAMPOMI_OK;
    int64_t i0 = 0;
    int b = 0;
    while (i0 < c->M && st == VAMPOMI_OK) {
        const int64_t nc = std::min<int64_t>((int64_t)chunk_cols, c->M - i0);
        if (used[b]) (void)hipEventSynchronize(done[b]);
        const size_t want = (size_t)nc * colb;
        const off_t off = (off_t)(c->S + i0) * (off_t)colb;
        if (!pread_parallel(file.fd, pin[b], want, off, nt)) {
            st = fail(VAMPOMI_ERR_IO, std::string("short read from methylation file ") + path);
            break;
        }
        st = load.put_cols(i0, nc, pin[b], rows_in(c));
        if (st != VAMPOMI_OK) break;
        if (hipEventRecord(done[b], c->st) != hipSuccess) {
            st = fail(VAMPOMI_ERR_HIP, "host-to-device copy of the methylation shard");
            break;
        }
        used[b] = true;
        i0 += nc;
        b = (b + 1) % NB;
    }
    (void)hipStreamSynchronize(c->st);
    for (int k = 0; k < NB; ++k) {
        (void)hipHostFree(pin[k]);
        (void)hipEventDestroy(done[k]);
    }
    return st != VAMPOMI_OK ? st : load.end();
}

extern "C" vampomi_status vampomi_load_meth_file(vampomi_ctx* c, const char* path) { return load_file(c, path, 8); }

extern "C" vampomi_status vampomi_load_meth_file_f32(vampomi_ctx* c, const char* path) {
    return load_file(c, path, 4);
}

extern "C" vampomi_status vampomi_load_meth_file_u16(vampomi_ctx* c, const char* path) {
    return load_file(c, path, 2);
}

extern "C" vampomi_status vampomi_generate_meth(vampomi_ctx* c, uint64_t seed, int kind) {
    if (!c || (kind != VAMPOMI_GEN_GAUSS && kind != VAMPOMI_GEN_METH)) return fail(VAMPOMI_ERR_ARG, "bad argument");
    if (c->N_file) return fail(VAMPOMI_ERR_STATE, "a context with a row subset loads its shard from a file or the host");
    if (c->adj_R)
        return fail(VAMPOMI_ERR_STATE, "a covariate-adjusted context loads its shard from a file or the host");
    if (c->u16() && kind == VAMPOMI_GEN_GAUSS)
        return fail(VAMPOMI_ERR_RANGE, "VAMPOMI_GEN_GAUSS values are not in [0, 1]: they cannot be stored as 16-bit "
                                       "fixed point (VAMPOMI_STORE_U16)");
    HIPCHK(hipSetDevice(c->device));
    IngestScope load(c, 0);
    STCHK(load.begin());
    if (!c->u16()) {
        HIPCHK(vk::gen_markers(seed, kind, c->N, c->ld, c->S, c->M, c->X, c->ek(), c->st));
        return load.end();
    }
    // U16: the generator's doubles in chunks of columns (about 256 MB), each
    // quantised into the shard as an ingest of the fp64 matrix would be (the
    // chunk's columns at stride ld, the record's indices by N)
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(c->M, 1),
                                            std::max<int64_t>(1, io_chunk_bytes() / (c->ld * 8)));
    STCHK(grow(c, load.stage, (size_t)chunk * (size_t)c->ld * 8, "device staging buffer of the generator"));
    hipError_t e = hipSuccess;
    for (int64_t i0 = 0; i0 < c->M && e == hipSuccess; i0 += chunk) {
        const int64_t nc = std::min(chunk, c->M - i0);
        e = vk::gen_markers(seed, kind, c->N, c->ld, c->S + i0, nc, load.stage.p, vk::kXF64, c->st);
        if (e == hipSuccess)
            e = vk::convert_cols(load.stage.p, vk::kXF64, c->ld, nullptr, c->N, nc, (uint16_t*)c->X + i0 * c->ld,
                                 vk::kXU16, c->ld, c->N, c->S + i0, c->qrec, c->st);
    }
    if (e != hipSuccess) return fail(VAMPOMI_ERR_HIP, std::string("generate_meth: ") + hipGetErrorString(e));
    return load.end();
}

// ---------------------------------------------------------------------------
// what the last load recorded; the stored values read back
// ---------------------------------------------------------------------------
extern "C" vampomi_status vampomi_get_missing_stats(const vampomi_ctx* c, int64_t* missing,
                                                    int64_t* markers_with_missing, int64_t* markers_masked,
                                                    int64_t* per_marker) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (!c->have_X) return fail(VAMPOMI_ERR_STATE, "no methylation data loaded");
    if (missing) *missing = c->na_missing;
    if (markers_with_missing) *markers_with_missing = c->na_markers;
    if (markers_masked) *markers_masked = c->na_masked;
    if (per_marker && c->na_per_marker.empty()) std::fill(per_marker, per_marker + c->M, (int64_t)0);
    if (per_marker && !c->na_per_marker.empty())
        std::copy(c->na_per_marker.begin(), c->na_per_marker.end(), per_marker);
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_get_quant_stats(const vampomi_ctx* c, int64_t* clamped, double* max_abs_err) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (!c->have_X) return fail(VAMPOMI_ERR_STATE, "no methylation data loaded");
    if (clamped) *clamped = c->q_clamped;
    if (max_abs_err) *max_abs_err = c->q_max_err;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_get_adjust_stats(const vampomi_ctx* c, int64_t* absorbed, uint8_t* per_marker) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (!c->have_X) return fail(VAMPOMI_ERR_STATE, "no methylation data loaded");
    if (absorbed) *absorbed = c->adj_absorbed;
    if (per_marker && c->adj_flags.empty()) std::fill(per_marker, per_marker + c->M, (uint8_t)0);
    if (per_marker && !c->adj_flags.empty()) std::copy(c->adj_flags.begin(), c->adj_flags.end(), per_marker);
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_read_markers(vampomi_ctx* c, int64_t i0, int64_t count, double* out) {
    if (!c || !out || i0 < 0 || count < 0 || i0 + count > c->M) return fail(VAMPOMI_ERR_ARG, "bad marker range");
    if (!c->have_X) return fail(VAMPOMI_ERR_STATE, "no methylation data loaded");
    HIPCHK(hipSetDevice(c->device));
    const bool narrow = c->f32() || c->u16();
    if (count > 0 && !narrow)
        HIPCHK(hipMemcpy2DAsync(out, (size_t)c->N * 8, (const double*)c->X + i0 * c->ld, (size_t)c->ld * 8,
                                (size_t)c->N * 8, (size_t)count, hipMemcpyDeviceToHost, c->st));
    // fp32 / 16-bit storage: the stored values widened on the device (exact),
    // in chunks of about 64 MB through a staging buffer
    void* stage = nullptr;
    if (count > 0 && narrow) {
        const int64_t chunk = std::min<int64_t>(count, std::max<int64_t>(1, ((int64_t)64 << 20) / (c->N * 8)));
        HIPCHK(hipMalloc(&stage, (size_t)chunk * (size_t)c->N * 8));
        for (int64_t k = 0; k < count; k += chunk) {
            const int64_t nc = std::min(chunk, count - k);
            hipError_t e = vk::convert_cols((const char*)c->X + (size_t)((i0 + k) * c->ld * c->esize()), c->ek(), c->ld,
                                            nullptr, c->N, nc, stage, vk::kXF64, c->N, c->N, 0, nullptr, c->st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(out + k * c->N, stage, (size_t)nc * (size_t)c->N * 8, hipMemcpyDeviceToHost, c->st);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(c->st);
                (void)hipFree(stage);
                return fail(VAMPOMI_ERR_HIP, std::string("read_markers: ") + hipGetErrorString(e));
            }
        }
    }
    const vampomi_status st = sync_stream(c, c->st);
    if (stage) (void)hipFree(stage);
    return st;
}
