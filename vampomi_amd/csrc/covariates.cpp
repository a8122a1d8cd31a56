// covariates.cpp — covariates of the probit model: ingest, the Newton fit of
// their effects (vamp::Newton_method_cov, src/vamp_probit.cpp:525-617) around
// the device sums of probit.hip, and the entry points of include/vampomi.h.
//
// The table is N-side data: every rank holds all of it, as it holds y, and
// fits the effects itself from the same bits (no collective).
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "hostio.h"

static_assert(VAMPOMI_MAX_C == vk::kCovMaxC, "VAMPOMI_MAX_C");

namespace {

// boost::numeric::ublas::lu_factorize (partial pivoting: the first entry of
// largest magnitude; the column scaled by the pivot's reciprocal); returns 0,
// or 1 + the first column whose pivot is exactly zero.  A: n x n, row-major
int lu_factorize(std::vector<double>& A, int n, std::vector<int>& pm) {
    int singular = 0;
    for (int i = 0; i < n; ++i) pm[i] = i;
    for (int i = 0; i < n; ++i) {
        int ip = i;
        double t = 0.0;
        for (int r = i; r < n; ++r) {
            const double u = std::fabs(A[r * n + i]);
            if (u > t) {
                ip = r;
                t = u;
            }
        }
        if (A[ip * n + i] != 0.0) {
            if (ip != i) {
                pm[i] = ip;
                for (int k = 0; k < n; ++k) std::swap(A[i * n + k], A[ip * n + k]);
            }
            const double inv = 1.0 / A[i * n + i];
            for (int r = i + 1; r < n; ++r) A[r * n + i] *= inv;
        } else if (singular == 0) {
            singular = i + 1;
        }
        for (int r = i + 1; r < n; ++r)
            for (int k = i + 1; k < n; ++k) A[r * n + k] -= A[r * n + i] * A[i * n + k];
    }
    return singular;
}

// lu_substitute: the row swaps, the unit lower solve, the upper solve
void lu_substitute(const std::vector<double>& A, int n, const std::vector<int>& pm, double* b) {
    for (int i = 0; i < n; ++i)
        if (pm[i] != i) std::swap(b[i], b[pm[i]]);
    for (int i = 0; i < n; ++i) {
        const double t = b[i];
        if (t != 0.0)
            for (int r = i + 1; r < n; ++r) b[r] -= A[r * n + i] * t;
    }
    for (int i = n - 1; i >= 0; --i) {
        const double t = b[i] /= A[i * n + i];
        if (t != 0.0)
            for (int r = 0; r < i; ++r) b[r] -= A[r * n + i] * t;
    }
}

double dot_seq(const double* a, const double* b, int n) {  // inner_prod(a, b, 0), src/utilities.cpp:138-150
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i] * b[i];
    return s;
}

vampomi_status need_cov(vampomi_ctx* c) {
    if (c->cov_C < 1) return fail(VAMPOMI_ERR_STATE, "set the covariates first");
    if (!c->have_y) return fail(VAMPOMI_ERR_STATE, "set the phenotype first");
    return VAMPOMI_OK;
}

// eta to the device; out: where vk::cov_eval / cov_mlogl write
vampomi_status put_eta(vampomi_ctx* c, const double* eta, double** out) {
    HIPCHK(hipMemcpyAsync(c->cov_dev, eta, (size_t)c->cov_C * 8, hipMemcpyHostToDevice, c->st));
    *out = c->cov_dev + vk::kCovMaxC;
    return VAMPOMI_OK;
}

vampomi_status mlogl_dev(vampomi_ctx* c, const double* gg, const double* eta, double* v) {
    double* out = nullptr;
    STCHK(put_eta(c, eta, &out));
    HIPCHK(vk::cov_mlogl(c->N, c->cov_C, c->cov_Z, c->ld, c->y, gg, c->cov_dev, c->cov_part, out, c->st));
    HIPCHK(hipMemcpyAsync(v, out, 8, hipMemcpyDeviceToHost, c->st));
    return sync_stream(c, c->st);
}

// the table in c->cov_host (C columns of N) to the device, with its scratch
vampomi_status upload_cov(vampomi_ctx* c, int C) {
    for (double** p : {&c->cov_Z, &c->cov_part, &c->cov_dev}) dev_free(*p);
    c->cov_C = 0;
    c->cov_fitted = false;
    if (C == 0) {
        c->cov_host.clear();
        return VAMPOMI_OK;
    }
    const size_t ld = (size_t)c->ld, N = (size_t)c->N;
    STCHK(dev_alloc(&c->cov_Z, (size_t)C * ld));
    STCHK(dev_alloc(&c->cov_part, (size_t)vk::cov_tiles(c->N) * (size_t)vk::cov_nq(C)));
    STCHK(dev_alloc(&c->cov_dev, (size_t)vk::kCovMaxC + (size_t)C * C + C + 1));
    HIPCHK(hipMemsetAsync(c->cov_Z, 0, (size_t)C * ld * 8, c->st));
    HIPCHK(hipMemcpy2DAsync(c->cov_Z, ld * 8, c->cov_host.data(), N * 8, N * 8, (size_t)C, hipMemcpyHostToDevice,
                            c->st));
    STCHK(sync_stream(c, c->st));
    c->cov_C = C;
    return VAMPOMI_OK;
}

}  // namespace

vampomi_status cov_eval_dev(vampomi_ctx* c, const double* gg, const double* eta, double* H, double* rhs,
                            double* mlogL) {
    const int C = c->cov_C;
    double* out = nullptr;
    STCHK(put_eta(c, eta, &out));
    HIPCHK(vk::cov_eval(c->N, C, c->cov_Z, c->ld, c->y, gg, c->cov_dev, c->cov_part, out, c->st));
    if (H) HIPCHK(hipMemcpyAsync(H, out, (size_t)C * C * 8, hipMemcpyDeviceToHost, c->st));
    if (rhs) HIPCHK(hipMemcpyAsync(rhs, out + C * C, (size_t)C * 8, hipMemcpyDeviceToHost, c->st));
    if (mlogL) HIPCHK(hipMemcpyAsync(mlogL, out + C * C + C, 8, hipMemcpyDeviceToHost, c->st));
    return sync_stream(c, c->st);
}

vampomi_status cov_offset_dev(vampomi_ctx* c, const double* eta, double* m) {
    double* out = nullptr;
    STCHK(put_eta(c, eta, &out));
    HIPCHK(vk::cov_offset(c->N, c->cov_C, c->cov_Z, c->ld, c->cov_dev, m, c->st));
    return VAMPOMI_OK;
}

// The reference's loop with its oddities kept (:531-615): the step's
// acceptance test is the Armijo one with the factor 1/2 on a Newton step; the
// relative-error stop fires BEFORE eta takes the step (the last step is
// thrown away); the monotonicity stop fires after it.  mlogL at an eta already
// evaluated is not evaluated again (:566, :604, :606 repeat :575's and the
// sums' values: the kernels give the same bits for the same input).  A step
// that is exactly zero (a singular H, :556-559, or rhs = 0) ends the loop at
// once: the reference would repeat the same iteration to the same eta.
vampomi_status cov_newton_dev(vampomi_ctx* c, const double* gg, const double* eta0, double* eta, int* iters,
                              int* backtracks, double* rel_err) {
    const int C = c->cov_C;
    const double N = (double)c->N;
    std::vector<double> e((size_t)C, 0.0), en((size_t)C), H((size_t)C * C), step((size_t)C), grad((size_t)C),
        displ((size_t)C);
    std::vector<int> pm((size_t)C);
    if (eta0) e.assign(eta0, eta0 + C);
    int it = 0;
    for (; it <= 500; ++it) {
        double init_val = 0.0;
        STCHK(cov_eval_dev(c, gg, e.data(), H.data(), step.data(), &init_val));
        for (int j = 0; j < C; ++j) grad[j] = -step[j] / N;  // grad_cov (:504-523), probit_var = 1
        if (lu_factorize(H, C, pm) == 0)
            lu_substitute(H, C, pm, step.data());
        else
            std::fill(step.begin(), step.end(), 0.0);
        bool zero = true;
        for (int j = 0; j < C; ++j) zero = zero && step[j] == 0.0;
        const double norm_eta = std::sqrt(dot_seq(e.data(), e.data(), C));
        if (zero) {
            if (backtracks) backtracks[it] = 0;
            if (rel_err) rel_err[it] = norm_eta == 0 ? 1.0 : 0.0;
            ++it;
            break;
        }
        double scale = 1, curr_val = 0.0;
        int bt = 0;
        for (int i = 1; i < 300; ++i) {  // :568-583
            for (int j = 0; j < C; ++j) displ[j] = scale * step[j];
            for (int j = 0; j < C; ++j) en[j] = e[j] + displ[j];
            STCHK(mlogl_dev(c, gg, en.data(), &curr_val));
            if (curr_val <= init_val + dot_seq(displ.data(), grad.data(), C) / 2) break;
            scale *= 0.9;
            ++bt;
        }
        double d2 = 0.0;
        for (int j = 0; j < C; ++j) d2 += (e[j] - en[j]) * (e[j] - en[j]);
        const double rel = norm_eta == 0 ? 1.0 : std::sqrt(d2) / norm_eta;  // :585-593
        if (backtracks) backtracks[it] = bt;
        if (rel_err) rel_err[it] = rel;
        if (rel < 1e-4) {  // :597-601
            ++it;
            break;
        }
        e = en;                       // :605
        if (curr_val > init_val) {    // :608-614
            ++it;
            break;
        }
    }
    if (it > 501) it = 501;
    if (iters) *iters = it;
    std::memcpy(eta, e.data(), (size_t)C * 8);
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_parse_covariates(const char* path, int64_t N, int C, int standardize, double* out) {
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    if (C == 0) return VAMPOMI_OK;
    if (!path || !out || N < 1) return fail(VAMPOMI_ERR_ARG, "bad argument");
    std::string err;
    if (vio::read_covariates(path, N, C, standardize != 0, out, &err) != 0) return fail(VAMPOMI_ERR_IO, err);
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_read_covariates(vampomi_ctx* c, const char* path, int C) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> Z((size_t)C * (size_t)c->N);
    if (c->N_file && C > 0) {  // the file's N_file rows raw, the subset's kept, then standardised
        std::vector<double> raw((size_t)C * (size_t)c->N_file);
        STCHK(vampomi_parse_covariates(path, c->N_file, C, 0, raw.data()));
        for (int j = 0; j < C; ++j)
            for (int64_t i = 0; i < c->N; ++i)
                Z[(size_t)j * c->N + i] = raw[(size_t)j * c->N_file + c->rows_host[(size_t)i]];
        vio::standardize_covariates(Z.data(), c->N, C, c->N);
    } else {
        STCHK(vampomi_parse_covariates(path, c->N, C, 1, Z.data()));
    }
    c->cov_host.swap(Z);
    return upload_cov(c, C);
}

extern "C" vampomi_status vampomi_set_covariates(vampomi_ctx* c, const double* Z, int C, int64_t ld_in,
                                                 int standardize) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (C < 0 || C > VAMPOMI_MAX_C)
        return fail(VAMPOMI_ERR_ARG, "number of covariates out of range (0.." + std::to_string(VAMPOMI_MAX_C) + ")");
    if (C > 0 && (!Z || ld_in < c->N)) return fail(VAMPOMI_ERR_ARG, "bad covariate table");
    HIPCHK(hipSetDevice(c->device));
    c->cov_host.assign((size_t)C * (size_t)c->N, 0.0);
    for (int j = 0; j < C; ++j)
        std::memcpy(c->cov_host.data() + (size_t)j * c->N, Z + (int64_t)j * ld_in, (size_t)c->N * 8);
    if (standardize) vio::standardize_covariates(c->cov_host.data(), c->N, C, c->N);
    return upload_cov(c, C);
}

extern "C" vampomi_status vampomi_get_covariates(vampomi_ctx* c, double* out) {
    if (!c || (!out && c->cov_C > 0)) return fail(VAMPOMI_ERR_ARG, "null argument");
    if (c->cov_C > 0) std::memcpy(out, c->cov_host.data(), c->cov_host.size() * 8);
    return VAMPOMI_OK;
}

// gg (N, mem) into the context's scratch; *dev: its device address, or null
static vampomi_status stage_gg(vampomi_ctx* c, const double* gg, int mem, const double** dev) {
    *dev = nullptr;
    if (!gg) return VAMPOMI_OK;
    HIPCHK(hipMemcpyAsync(c->nbuf, gg, (size_t)c->N * 8,
                          mem == VAMPOMI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->st));
    *dev = c->nbuf;
    return VAMPOMI_OK;
}

extern "C" vampomi_status vampomi_cov_eval(vampomi_ctx* c, const double* gg, const double* eta, double* H,
                                           double* rhs, double* mlogL, int mem) {
    if (!c || !eta) return fail(VAMPOMI_ERR_ARG, "null argument");
    STCHK(need_cov(c));
    HIPCHK(hipSetDevice(c->device));
    const double* g = nullptr;
    STCHK(stage_gg(c, gg, mem, &g));
    return cov_eval_dev(c, g, eta, H, rhs, mlogL);
}

extern "C" vampomi_status vampomi_newton_cov(vampomi_ctx* c, const double* gg, const double* eta0, double* eta,
                                             int* iters, int* backtracks, double* rel_err, int mem) {
    if (!c || !eta) return fail(VAMPOMI_ERR_ARG, "null argument");
    STCHK(need_cov(c));
    HIPCHK(hipSetDevice(c->device));
    const double* g = nullptr;
    STCHK(stage_gg(c, gg, mem, &g));
    return cov_newton_dev(c, g, eta0, eta, iters, backtracks, rel_err);
}

extern "C" vampomi_status vampomi_get_cov_eff(vampomi_ctx* c, double* out) {
    if (!c) return fail(VAMPOMI_ERR_ARG, "null context");
    if (!c->cov_fitted) return fail(VAMPOMI_ERR_STATE, "no covariate effects fitted: run the bin_class model first");
    if (!c->cov_eff.empty()) {
        if (!out) return fail(VAMPOMI_ERR_ARG, "null argument");
        std::memcpy(out, c->cov_eff.data(), c->cov_eff.size() * 8);
    }
    return VAMPOMI_OK;
}
