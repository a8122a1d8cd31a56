/*
 * vampomi.h — C ABI of the MI355X-native gVAMPomi VAMP engine.
 *
 * Plain C, plain pointers and sizes.  One context per process, driving one
 * gfx950 device and one contiguous marker shard [S, S+M) of the Mt markers
 * (the reference's MPI rank, src/utilities.cpp:207-239).  Contexts of a job
 * are joined by an RCCL communicator over xGMI; every entry point marked
 * COLLECTIVE must be called by all ranks in the same order, exactly like the
 * reference's MPI_Allreduce-bearing calls.
 *
 * Reference seams replaced (paths relative to the reference repository):
 *   data::data / read_methylation_data / compute_markers_statistics
 *        src/data.cpp:24-53, 116-153, 233-283 -> vampomi_open + vampomi_load_meth_*
 *   data::read_phen            src/data.cpp:58-110      -> vampomi_read_phen / vampomi_set_phen
 *   data::Ax                   src/data.cpp:340-373     -> vampomi_ax      (COLLECTIVE)
 *   data::ATx / dot_product    src/data.cpp:294-333     -> vampomi_atx
 *   data::get_mave/get_msig    src/data.hpp:56-57       -> vampomi_get_marker_stats
 *   data::get_phen             src/data.hpp:48          -> vampomi_get_phen
 *   vamp::lmmse_mult           src/vamp.cpp:645-662     -> vampomi_lmmse_mult (COLLECTIVE)
 *   vamp::precondCG_solver     src/vamp.cpp:664-757     -> vampomi_pcg      (COLLECTIVE)
 *   vamp::g1 / vamp::g1d       src/vamp.cpp:440-492     -> vampomi_denoise  (COLLECTIVE: alpha1 sum)
 *   vamp::updatePrior          src/vamp.cpp:531-643     -> vampomi_update_prior (COLLECTIVE)
 *   vamp::g1_bin_class / g1d_bin_class
 *        src/vamp_probit.cpp:469-488                    -> vampomi_denoise_bin / _denoise_bin_cov
 *   data::read_covariates      src/data.cpp:159-227     -> vampomi_read_covariates / vampomi_set_covariates
 *   vamp::Newton_method_cov / grad_cov / mlogL_probit
 *        src/vamp_probit.cpp:490-617                    -> vampomi_newton_cov / vampomi_cov_eval
 *   vamp::vamp + vamp::infere / infere_linear / infere_bin_class
 *        src/vamp.cpp:18-91, 94-107, 110-438,
 *        src/vamp_probit.cpp:19-488                     -> vampomi_infere   (COLLECTIVE)
 *        (or vampomi_vamp_begin / _step / _end, one VAMP iteration per step)
 *   divide_work                src/utilities.cpp:207-239 -> vampomi_divide_work
 *   run mode test              src/main_meth.cpp:112-205 -> vampomi_test_metrics (COLLECTIVE)
 *   association_test loo / se  src/main_meth.cpp:206-264, src/data.cpp:385-417,
 *                              src/utilities.cpp:269-282 -> vampomi_assoc_loo / _se
 *   (not in the reference) covariates regressed out of the linear model's
 *        matrix and phenotype at ingest                 -> vampomi_set_adjust / vampomi_read_adjust
 *
 * Testing aid: with VAMPOMI_COMM=loopback in the environment, the contexts
 * of a multi-rank job are driven by threads of ONE process (any device, the
 * same one allowed) and all-reduces become an in-process rendezvous that sums
 * in rank order; comm_id is then any 128 bytes shared by the ranks.
 *
 * Errors: every call returns a vampomi_status; nothing aborts the process
 * (the reference calls MPI_Abort / exit / throw).  vampomi_last_error() gives
 * a message for the calling thread.
 */
#ifndef VAMPOMI_H
#define VAMPOMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMPOMI_ABI_VERSION 3
#define VAMPOMI_MAX_L 64          /* mixture components */
#define VAMPOMI_MAX_C 64          /* covariates of the probit model */
#define VAMPOMI_MAX_SEGMENTS 64   /* labels of the leave-one-chromosome-out test */
#define VAMPOMI_UNIQUE_ID_BYTES 128

typedef enum {
    VAMPOMI_OK = 0,
    VAMPOMI_ERR_ARG = 1,          /* bad argument / shape */
    VAMPOMI_ERR_HIP = 2,          /* HIP runtime failure */
    VAMPOMI_ERR_RCCL = 3,         /* RCCL failure */
    VAMPOMI_ERR_IO = 4,           /* file could not be opened / read / written */
    VAMPOMI_ERR_NAN_PHEN = 5,     /* "NA" in phenotype file (src/data.cpp:73-74) */
    VAMPOMI_ERR_STATE = 6,        /* call out of order (e.g. Ax before data load) */
    VAMPOMI_ERR_OOM = 7,          /* device or host allocation failed */
    VAMPOMI_ERR_MODEL = 8,        /* unsupported --model (src/vamp.cpp:103-104) */
    VAMPOMI_ERR_RANGE = 9,        /* methylation values a VAMPOMI_STORE_U16 shard cannot hold */
    VAMPOMI_ERR_NAN_METH = 10     /* missing methylation values (NaN) under VAMPOMI_NA_FATAL */
} vampomi_status;

/* where a caller buffer lives */
#define VAMPOMI_MEM_HOST 0
#define VAMPOMI_MEM_DEVICE 1

/* synthetic design kinds for vampomi_generate_meth */
#define VAMPOMI_GEN_GAUSS 0       /* i.i.d. N(0,1)-like (simulation/data_sim.py:35) */
#define VAMPOMI_GEN_METH 1        /* methylation-like beta values in [0,1] */

/* how the methylation shard is held on the device (vampomi_set_storage).  The
 * matrix is the only object whose size matters, and every pass is bound by
 * reading it: as floats it takes half the memory and half the bytes per pass.
 * Only the storage changes: every sum, the CG, the denoiser, EM and p-values
 * stay fp64, and an F32 context computes, bit for bit, what an F64 context
 * computes on the widened copy of the same stored values. */
#define VAMPOMI_STORE_F64 0       /* doubles (the default; the reference's file format) */
#define VAMPOMI_STORE_F32 1       /* floats: fp64 input is rounded to nearest even at ingest */
/* 16-bit fixed point: the stored element is a uint16 k meaning k * 2^-16, a
 * quarter of the doubles' memory and bytes per pass.  Methylation beta values
 * lie in [0, 1]; the grid's absolute error is at most 2^-17 (7.7e-6) everywhere
 * in [0, 1 - 2^-17), below the data's last digit.  An input x (fp64 or fp32) is
 * stored as k = min(65535, rint(x * 65536)), ties to even: 0 <= x <= 1 is
 * accepted (-0.0 is 0; x >= 1 - 2^-17, 1.0 included, is CLAMPED to 65535);
 * NaN, +-inf, x < 0 and x > 1 are REJECTED: the load returns VAMPOMI_ERR_RANGE,
 * vampomi_last_error gives the number of rejected entries and the smallest
 * offending (marker, row) (the global marker index), and the context is left
 * without a shard, as after an I/O error.  The widening (double)k * 2^-16 is
 * exact, so a U16 context computes, bit for bit, what an F64 context computes
 * on the dequantised matrix.  (16, not 2: the value is the element's bits.) */
#define VAMPOMI_STORE_U16 16

typedef struct vampomi_ctx vampomi_ctx;

typedef struct {
    int64_t N;                    /* individuals (--N) */
    int64_t Mt;                   /* total markers (--Mt) */
    int rank, nranks;             /* this process's shard */
    int device;                   /* HIP device ordinal; -1: rank % visible devices */
    const void* comm_id;          /* VAMPOMI_UNIQUE_ID_BYTES from vampomi_comm_unique_id
                                     on rank 0, broadcast by the caller; NULL if nranks==1 */
    double alpha_scale;           /* --alpha-scale (src/data.cpp:261-264) */
} vampomi_shard_desc;

/* ---- job / context ---- */
int vampomi_abi_version(void);
const char* vampomi_last_error(void);
/* src/utilities.cpp:207-239 */
void vampomi_divide_work(int64_t Mt, int nranks, int rank, int64_t* M, int64_t* S, int64_t* Mm);
vampomi_status vampomi_comm_unique_id(void* out /* VAMPOMI_UNIQUE_ID_BYTES */);
vampomi_status vampomi_open(const vampomi_shard_desc* desc, vampomi_ctx** out);
void vampomi_close(vampomi_ctx* ctx);
/* M (local markers), S (first global marker), ld (device leading dimension) */
vampomi_status vampomi_shard_info(const vampomi_ctx* ctx, int64_t* M, int64_t* S, int64_t* ld);
vampomi_status vampomi_sync(vampomi_ctx* ctx);          /* drain the context's stream */
vampomi_status vampomi_barrier(vampomi_ctx* ctx);       /* COLLECTIVE: RCCL barrier + drain */
/* COLLECTIVE: vampomi_barrier with its own wait limit instead of
 * VAMPOMI_COLL_TIMEOUT_S: the barrier after a rank-local phase of uneven
 * length, e.g. the shard load, where the ranks' files come off storage at
 * different rates (there is no MPI_Barrier in the reference's data::data,
 * src/data.cpp:23-46; its first collective simply waits). */
vampomi_status vampomi_barrier_timeout(vampomi_ctx* ctx, double seconds);
/* COLLECTIVE: *all_ok = 1 iff local_ok != 0 on every rank.  How ranks agree on
   a rank-local outcome (a file read) before the next collective; the
   reference's rank-local exits (exit(1), throw) leave the other MPI ranks
   blocked in MPI_Allreduce instead. */
vampomi_status vampomi_all_ok(vampomi_ctx* ctx, int local_ok, int* all_ok);
/* After a rank-local failure: poisons the test-only loopback communicator
   (every rank's pending and later collectives fail at once) or aborts the RCCL
   communicator, so no rank waits for this one.  Every COLLECTIVE entry point
   does this itself when it fails. */
vampomi_status vampomi_comm_abort(vampomi_ctx* ctx);

/* ---- data ingest (data::data) ---- */
/* The storage of the shard, VAMPOMI_STORE_F64 (the default), _F32 or _U16.  Legal
 * only before the shard is allocated, i.e. before any vampomi_load_meth_* or
 * vampomi_generate_meth: VAMPOMI_ERR_STATE afterwards, VAMPOMI_ERR_ARG for
 * any other value.  VAMPOMI_STORAGE=f64|f32|u16 in the environment sets the default
 * at vampomi_open (any other value: vampomi_open fails with VAMPOMI_ERR_ARG).
 * Rank-local: the ranks of a job need not agree on it.  The column stride ld
 * (elements) and every kernel plan are the same for all storages. */
vampomi_status vampomi_set_storage(vampomi_ctx* ctx, int storage);
vampomi_status vampomi_get_storage(const vampomi_ctx* ctx, int* storage);
/* A row subset: the files hold N_file rows (individuals) of which the context
 * analyses the n = N listed in rows, so a phenotype's missing values, a QC list
 * or a train/test split need no second copy of the matrix.  Open the context
 * with N = n.  rows: strictly ascending within [0, N_file), 2 <= n <= N_file,
 * n == the context's N, N_file < 2^31; anything else is VAMPOMI_ERR_ARG.  Legal
 * only before the shard is allocated (as vampomi_set_storage) and before a
 * phenotype or covariates are set: VAMPOMI_ERR_STATE afterwards.  Rank-local:
 * every rank of a job sets the same subset.  From then on
 *   - every vampomi_load_meth_file* reads this shard's bytes [S*N_file*es,
 *     (S+M)*N_file*es) (es: the file's element size; a file too short for
 *     N_file rows is VAMPOMI_ERR_IO), and vampomi_load_meth_host* takes columns
 *     of N_file rows, ld_in >= N_file.  Every chunk is staged on the device as
 *     it is and a gather kernel keeps the listed rows as it converts, also
 *     where the input's element type is the storage's.  A U16 context range-checks
 *     and counts the kept entries only, and VAMPOMI_ERR_RANGE names the
 *     file's row;
 *   - vampomi_read_phen and vampomi_read_covariates expect N_file rows, keep the
 *     listed ones and only then standardise; "NA" is VAMPOMI_ERR_NAN_PHEN in a
 *     kept row and ignored in any other.  vampomi_set_phen and
 *     vampomi_set_covariates keep taking n rows;
 *   - vampomi_generate_meth returns VAMPOMI_ERR_STATE.
 * The context holds, bit for bit, what a context of N = n without a subset
 * holds after loading files from which the other rows were removed, and so
 * computes the same bits in everything that follows.  Without a subset every
 * path and launch is what it is without this call. */
vampomi_status vampomi_set_row_subset(vampomi_ctx* ctx, int64_t N_file, const int64_t* rows, int64_t n);
/* *N_file = the subset's file rows, 0 without a subset; rows (n entries, or
 * NULL) receives the list */
vampomi_status vampomi_get_row_subset(const vampomi_ctx* ctx, int64_t* N_file, int64_t* rows);
/* The rows of a PLINK phenotype file that an analysis keeps; needs no device.
 * The file is split as vampomi_read_phen splits it: per row FID, IID and the
 * value, missing where the value is "NA".  keep_path (or NULL): PLINK --keep
 * style, per non-blank line FID and IID, further fields ignored; a row is kept
 * iff its pair is named there, so the result is ascending in the phenotype
 * file's order whatever the keep file's order or duplicates.  A pair found in
 * no phenotype row is VAMPOMI_ERR_ARG (vampomi_last_error names the pair and
 * its line).  drop_na != 0 also drops the rows whose value is "NA"; with
 * drop_na == 0 an "NA" in a row that would be kept is VAMPOMI_ERR_NAN_PHEN.
 * *N_file = the file's rows, *n = the kept rows (either may be NULL); rows
 * (NULL: count only) receives them, cap < n is VAMPOMI_ERR_ARG.  A file that
 * cannot be opened is VAMPOMI_ERR_IO. */
vampomi_status vampomi_phen_rows(const char* phen_path, const char* keep_path, int drop_na, int64_t* rows,
                                 int64_t cap, int64_t* N_file, int64_t* n);
/* The rows that an analysis of all T phenotype files keeps; needs no device.
 * Every file must have the same number of rows and the same (FID, IID)
 * sequence, else VAMPOMI_ERR_ARG (vampomi_last_error names the first
 * differing file and row).  The keep file is vampomi_phen_rows's.  With
 * drop_na != 0 a row is kept iff it is kept and not "NA" in EVERY file; with
 * drop_na == 0 an "NA" in a kept row of any file is VAMPOMI_ERR_NAN_PHEN
 * (the message names the file).  na_per_file (T entries, may be NULL): the
 * "NA"s among the rows the keep file leaves, per file.  rows, cap, *N_file
 * and *n as vampomi_phen_rows's; for T = 1 the call returns what
 * vampomi_phen_rows returns. */
vampomi_status vampomi_phen_rows_common(const char* const* phen_paths, int T, const char* keep_path, int drop_na,
                                        int64_t* rows, int64_t cap, int64_t* N_file, int64_t* n,
                                        int64_t* na_per_file);
/* marker-major fp64 file (README.md:15): this shard's bytes [S*N*8, (S+M)*N*8).
 * On an F32 or U16 context each chunk is staged on the device as fp64 and
 * rounded (nearest even) or quantised (VAMPOMI_STORE_U16: range-checked,
 * VAMPOMI_ERR_RANGE) there into the column layout. */
vampomi_status vampomi_load_meth_file(vampomi_ctx* ctx, const char* path);
/* the same marker-major layout with 4-byte float elements: this shard's bytes
 * [S*N*4, (S+M)*N*4), through the same read pipeline; widened (exactly) on an
 * F64 context, quantised on a U16 one */
vampomi_status vampomi_load_meth_file_f32(vampomi_ctx* ctx, const char* path);
/* the same layout with 2-byte little-endian uint16 elements k meaning k * 2^-16
 * (VAMPOMI_STORE_U16's own format): this shard's bytes [S*N*2, (S+M)*N*2).
 * Loads into any storage: copied as it is on a U16 context, widened exactly on
 * an F32 or F64 one (k * 2^-16 is exactly a float too) */
vampomi_status vampomi_load_meth_file_u16(vampomi_ctx* ctx, const char* path);
/* host shard: M columns of N samples, column stride ld_in >= N doubles
 * (rounded on the device on an F32 context, quantised there on a U16 one) */
vampomi_status vampomi_load_meth_host(vampomi_ctx* ctx, const double* X, int64_t ld_in);
/* host shard of floats, column stride ld_in >= N floats, for any storage
 * (widened exactly on an F64 context, quantised on a U16 one) */
vampomi_status vampomi_load_meth_host_f32(vampomi_ctx* ctx, const float* X, int64_t ld_in);
/* host shard of uint16 k meaning k * 2^-16, column stride ld_in >= N elements,
 * for any storage (widened exactly on an F32 or F64 context) */
vampomi_status vampomi_load_meth_host_u16(vampomi_ctx* ctx, const uint16_t* X, int64_t ld_in);
/* What the last load or generation of a U16 context did to its input: *clamped
 * = the accepted entries that rounded to 65536 and were stored as 65535,
 * *max_abs_err = the maximum over the shard of |stored value - input| (fp64; a
 * count and a maximum, so neither depends on the order of the device's work).
 * Both are zero on F64 and F32 contexts and after a uint16 input.  Either
 * pointer may be NULL.  VAMPOMI_ERR_STATE before a shard is loaded. */
vampomi_status vampomi_get_quant_stats(const vampomi_ctx* ctx, int64_t* clamped, double* max_abs_err);
/* Missing methylation values.  A MISSING entry is a NaN of the input's element
 * type (fp64 or fp32; any sign, any payload).  An infinity is a value.  uint16
 * input has no missing code, and vampomi_generate_meth makes none: the policy
 * does not touch them and their counts are zero.  With a row subset only the
 * kept rows are looked at.  The policy is rank-local, as the storage is, and
 * adds no collective.
 *   VAMPOMI_NA_PASS (the default): nobody looks; a load does what it did before
 *     the policy existed, launch for launch (a NaN loads silently into an F64 or
 *     F32 shard and is VAMPOMI_ERR_RANGE on a U16 one).
 *   VAMPOMI_NA_FATAL: a load that meets a missing entry fails with
 *     VAMPOMI_ERR_NAN_METH; vampomi_last_error gives their number and the
 *     smallest (global marker, the file's row), and the context is left without
 *     a shard, as after VAMPOMI_ERR_RANGE.  On a U16 context a NaN gives this
 *     error, an out-of-range value still VAMPOMI_ERR_RANGE, and both together
 *     this error.
 *   VAMPOMI_NA_MEAN: each missing entry of a marker is replaced by the mean
 *     s / n_obs of the marker's observed entries, s their fp64 sum in a fixed
 *     order that depends on the kept rows alone, and the mean
 *     is stored as any input value is (as it is, rounded to nearest even, or
 *     quantised).  A marker with no observed entry, or with
 *     (double)n_missing > max_missing_frac * (double)N, is MASKED: every entry
 *     is stored as 0, a constant column (mave 0, msig 1, exactly null).  Filled
 *     and masked entries are not counted by vampomi_get_quant_stats; observed
 *     ones are converted, range-checked and counted as ever.  Nothing after the
 *     ingest knows of missingness: the context holds what vampomi_read_markers
 *     returns and computes, bit for bit, what a plain context of the same
 *     storage computes after loading that matrix.
 * Under FATAL and MEAN every block of a load is staged on the device (also
 * where the input's element type is the storage's) and one workgroup per
 * column sweeps it twice.  max_missing_frac in [0, 1] matters under MEAN only.
 * Legal only before the shard is allocated (VAMPOMI_ERR_STATE afterwards);
 * another policy, or a fraction outside [0, 1] or NaN, is VAMPOMI_ERR_ARG. */
#define VAMPOMI_NA_PASS 0
#define VAMPOMI_NA_FATAL 1
#define VAMPOMI_NA_MEAN 2
vampomi_status vampomi_set_meth_na(vampomi_ctx* ctx, int policy, double max_missing_frac);
vampomi_status vampomi_get_meth_na(const vampomi_ctx* ctx, int* policy, double* max_missing_frac);
/* What the last load saw (this rank's shard): the missing entries, the markers
 * that had any, the markers masked, and per_marker (M entries, host; the true
 * count of a masked marker too).  Any pointer may be NULL.  All zeros under
 * VAMPOMI_NA_PASS.  VAMPOMI_ERR_STATE before a shard is loaded. */
vampomi_status vampomi_get_missing_stats(const vampomi_ctx* ctx, int64_t* missing, int64_t* markers_with_missing,
                                         int64_t* markers_masked, int64_t* per_marker);
/* ---- covariate adjustment of the LINEAR model ----
 * By Frisch-Waugh, y = Z g + X b + e with a flat prior on g is the model
 * P y = P X b + P e, P = I - Q Q^T, Q an orthonormal basis of span{1, Z}.  An
 * adjusted context stores P X and P y at ingest; nothing after the load knows
 * of it (operators, CG, denoiser, EM, association tests, test mode).
 *
 * vampomi_adjust_basis needs no device.  Z: C columns (0 <= C <= VAMPOMI_MAX_C)
 * of n raw values, column stride ld_in >= n; a value that is not finite is
 * VAMPOMI_ERR_ARG.  Q receives n x R doubles, column-major, R <= C + 1 (have
 * room for C + 1 columns): modified Gram-Schmidt over the intercept (always
 * kept, always first: Q's first column is 1/sqrt(n)) and then Z's columns in
 * order, each vector orthogonalised twice against the accepted ones, every sum
 * in long double, the normalised vector rounded to double.  dropped (C flags;
 * may be NULL when C == 0): 1 for a column whose norm is 0 or, after the
 * orthogonalisation, at most 1e-8 of what it was (constant or dependent).
 *
 * vampomi_set_adjust: the table for the context's N rows (C == 0: the
 * intercept only).  Legal only before the shard is allocated and before a
 * phenotype is set, and after vampomi_set_row_subset if there is one (which
 * returns VAMPOMI_ERR_STATE on an adjusted context): VAMPOMI_ERR_STATE
 * otherwise.  Residuals leave [0, 1]: VAMPOMI_ERR_ARG on a VAMPOMI_STORE_U16
 * context, and from vampomi_set_storage(VAMPOMI_STORE_U16) on an adjusted one
 * (uint16 INPUT into F64 / F32 storage is fine: widened, then adjusted).
 * vampomi_read_adjust: the file parsed as vampomi_parse_covariates(..,
 * standardize = 0) with N_file rows of which the subset's are taken.  Rank-local
 * and without a collective: every rank sets the same table and computes the
 * same bits.  From then on
 *   - every vampomi_load_meth_* adjusts each marker after the row gather and the
 *     NaN fill, in fp64: x the column (kept rows, missing entries filled as
 *     VAMPOMI_NA_MEAN defines), c = Q^T x, r = x - Q c, every sum in a fixed
 *     order that depends on N and R alone.  F64 stores r, F32
 *     (float)r: one rounding.  A marker with |r|^2 <= 1e-20 |x|^2 (constant,
 *     inside the covariates' span, all zero, masked) is ABSORBED: stored as
 *     zeros, a constant column (mave 0, msig 1, exactly null), and counted;
 *   - vampomi_read_phen and vampomi_set_phen replace y by y - Q (Q^T y) (host,
 *     long double sums) before their standardize step; vampomi_get_phen returns
 *     the adjusted, then scaled, vector;
 *   - vampomi_generate_meth, and vampomi_vamp_begin / vampomi_infere with
 *     "bin_class" (the probit model has its own covariates), return
 *     VAMPOMI_ERR_STATE.
 * The context holds what vampomi_read_markers and vampomi_get_phen return and
 * computes, bit for bit, what a plain context of the same storage computes
 * after vampomi_load_meth_host of that matrix and vampomi_set_phen(.., 0) of
 * that vector; the stored bits depend on neither the chunk size, file or array
 * input, nor the rank count, and an F32 context holds (float) of what an F64
 * one holds.  The association test's p-values keep N - 2 degrees of freedom, as
 * after an offline adjustment.  Without an adjustment every load is what it is
 * without these calls, launch for launch. */
vampomi_status vampomi_adjust_basis(const double* Z, int64_t n, int C, int64_t ld_in, double* Q, int* R,
                                    int* dropped);
vampomi_status vampomi_set_adjust(vampomi_ctx* ctx, const double* Z, int C, int64_t ld_in);
vampomi_status vampomi_read_adjust(vampomi_ctx* ctx, const char* path, int C);
/* *R = the basis vectors (0: no adjustment), dropped: the table's C flags, Q:
 * N x R doubles.  Every pointer may be NULL. */
vampomi_status vampomi_get_adjust(const vampomi_ctx* ctx, int* R, int* dropped, double* Q);
/* The last load: the absorbed markers of this rank's shard and per_marker (M
 * flags, host).  Either pointer may be NULL.  Zeros without an adjustment.
 * VAMPOMI_ERR_STATE before a shard is loaded. */
vampomi_status vampomi_get_adjust_stats(const vampomi_ctx* ctx, int64_t* absorbed, uint8_t* per_marker);
/* synthetic shard generated on the device (bit-identical to the oracle's; an
 * F32 context stores the generator's value rounded: VAMPOMI_GEN_GAUSS values
 * are exactly floats, VAMPOMI_GEN_METH values are not; a U16 context stores
 * VAMPOMI_GEN_METH values quantised and refuses VAMPOMI_GEN_GAUSS with
 * VAMPOMI_ERR_RANGE before generating anything) */
vampomi_status vampomi_generate_meth(vampomi_ctx* ctx, uint64_t seed, int kind);
/* PLINK phenotype, standardize = scale to unit variance, NOT centred */
vampomi_status vampomi_read_phen(vampomi_ctx* ctx, const char* path, int standardize);
vampomi_status vampomi_set_phen(vampomi_ctx* ctx, const double* y /* N, host */, int standardize);
vampomi_status vampomi_get_phen(vampomi_ctx* ctx, double* y /* N, host */);
/* synthetic phenotype y = sqrt(N)*A*beta + N(0,1-h2) noise, beta spike-and-slab
 * (lam causal fraction, h2 heritability), then read_phen scaling.  beta_out
 * (M local, host, may be NULL) receives beta = the true signal. COLLECTIVE */
vampomi_status vampomi_simulate_phen(vampomi_ctx* ctx, uint64_t seed, double lam, double h2,
                                     double* beta_out);
/* binary phenotype for the probit model: the liability of vampomi_simulate_phen
 * thresholded at 0 (y = 1 if > 0 else 0), stored raw (read_phen(false),
 * src/data.cpp:40-41). COLLECTIVE */
vampomi_status vampomi_simulate_phen_binary(vampomi_ctx* ctx, uint64_t seed, double lam, double h2,
                                            double* beta_out);
/* ---- covariates of the probit model (data::read_covariates, src/data.cpp:159-227) ----
 * An N x C table (age, sex, batch, cell types ...), held whole on every rank as
 * y is.  A context that holds one (C > 0) fits the covariate effects at the
 * start of every bin_class run and offsets the z-side denoiser with them
 * (below); the LINEAR model ignores the table, as the reference's main_meth.exe
 * does (its covariates are regressed out at ingest: vampomi_set_adjust).  Two properties of the reference's fit that are kept: a constant column
 * standardises to zeros and makes the Newton matrix singular, so the fit
 * returns ALL effects zero; and no intercept is fitted unless the table
 * carries a (non-constant) column for one.
 *
 * vampomi_parse_covariates needs no device: the file's first line (a header) is
 * skipped; every further line is split on whitespace runs, its first two fields
 * (the IDs) skipped, and exactly C numeric fields must remain, else the
 * reference's "FATAL: number of covariates = ... does not match ..." line is
 * printed to stdout and the call returns VAMPOMI_ERR_IO (the reference exits);
 * a row count other than N is VAMPOMI_ERR_IO too.  standardize: per column,
 * accumulated in long double, the mean and the POPULATION standard deviation
 * (divided by N); a column with deviation < 1e-8 becomes zeros, any other
 * (v - mean)/deviation.  out: C columns of N doubles (covariate-major).
 * C == 0 does nothing; C > VAMPOMI_MAX_C is VAMPOMI_ERR_ARG. */
vampomi_status vampomi_parse_covariates(const char* path, int64_t N, int C, int standardize, double* out);
/* the file, standardised as the reference always does, into the context (C == 0: none) */
vampomi_status vampomi_read_covariates(vampomi_ctx* ctx, const char* path, int C);
/* host table: C columns of N samples, column stride ld_in >= N (C == 0: none) */
vampomi_status vampomi_set_covariates(vampomi_ctx* ctx, const double* Z, int C, int64_t ld_in, int standardize);
/* the stored columns, C x N doubles, covariate-major (host) */
vampomi_status vampomi_get_covariates(vampomi_ctx* ctx, double* out);
/* One evaluation of the Newton quantities (src/vamp_probit.cpp:536-551, 490-523)
 * at eta (C, host) with the genetic predictor gg (N, `mem`; NULL = zeros): per
 * sample g = gg_i + sum_j Z_ij eta_j, s = 2 y_i - 1, arg = s g, ratio =
 * (2/sqrt(2 pi)) / erfcx(-arg/sqrt 2), lambda = ratio s, w = lambda (lambda + g);
 * H_jk = sum_i Z_ij Z_ik w (C*C, host), rhs_j = sum_i Z_ij lambda (C, host; the
 * gradient of -logL/N is -rhs/N), *mlogL = -(1/N) sum_i log Phi(arg).  Every sum
 * runs in a fixed order that depends on neither the device nor the launch: the
 * results repeat bit for bit.  H, rhs, mlogL may each be NULL.  Rank-local. */
vampomi_status vampomi_cov_eval(vampomi_ctx* ctx, const double* gg, const double* eta, double* H, double* rhs,
                                double* mlogL, int mem);
/* vamp::Newton_method_cov (:525-617): up to 501 Newton steps from eta0 (C, host;
 * NULL = zeros), H factored by LU with partial pivoting (a zero pivot: no step),
 * a backtracking line search (scale 1, x0.9, at most 299 evaluations; accepted
 * when mlogL(eta + d) <= mlogL(eta) + d.grad/2); rel_err = |eta - eta_new|/|eta|
 * (1 when |eta| = 0) below 1e-4 stops BEFORE eta takes the step (the last step
 * is discarded, as in the reference), a rise of mlogL stops after it.  eta (C,
 * host) receives the effects, *iters the outer iterations run; backtracks and
 * rel_err (each NULL or >= 501 entries) one value per outer iteration.
 * Rank-local: the N-side is replicated, every rank computes the same bits. */
vampomi_status vampomi_newton_cov(vampomi_ctx* ctx, const double* gg, const double* eta0, double* eta, int* iters,
                                  int* backtracks, double* rel_err, int mem);
/* the effects fitted by the last vampomi_vamp_begin / vampomi_infere of a
 * bin_class run on this context (C doubles; nothing when it holds no
 * covariates); VAMPOMI_ERR_STATE before that */
vampomi_status vampomi_get_cov_eff(vampomi_ctx* ctx, double* out);
/* (the statistics of the STORED values, rounded or quantised, accumulated in fp64) */
vampomi_status vampomi_get_marker_stats(vampomi_ctx* ctx, double* mave, double* msig);
/* copy local markers [i0, i0+count) back to the host, count x N doubles
 * (data::get_meth_data, src/data.hpp:53); an F32 or U16 context returns the
 * stored values widened (exactly): each a float, or a multiple of 2^-16 */
vampomi_status vampomi_read_markers(vampomi_ctx* ctx, int64_t i0, int64_t count, double* out);

/* ---- operators ---- */
/* out (N) = (sum over all ranks of (X_i - mave_i) * msig_i * x_i) / sqrt(N). COLLECTIVE */
vampomi_status vampomi_ax(vampomi_ctx* ctx, const double* x /* M */, double* out /* N */, int mem);
/* out (M) = msig_i * sum_j (X_ij - mave_i) * u_j * (1/sqrt(N)) */
vampomi_status vampomi_atx(vampomi_ctx* ctx, const double* u /* N */, double* out /* M */, int mem);
/* out = tau * ATx(Ax(v)) + gam2 * v, zero v short-circuits. COLLECTIVE */
vampomi_status vampomi_lmmse_mult(vampomi_ctx* ctx, const double* v, double tau, double gam2,
                                  double* out, int mem);
/* preconditioned CG on (tau*A^T A + gam2*I) mu = v from mu0 (NULL = zeros);
 * onsager != 0 adds the Onsager stop of src/vamp.cpp:708-726. COLLECTIVE */
vampomi_status vampomi_pcg(vampomi_ctx* ctx, const double* v, const double* mu0, double tau,
                           double gam2, int onsager, int max_iter, double tol, double* mu,
                           int* iters, int mem);
/* x1 = g1(r1), x1d = g1d(r1) for the mixture (probs, vars) with vars ALREADY
 * multiplied by N (src/vamp.cpp:87-88); *sum_d = sum over all ranks of x1d.
 * COLLECTIVE */
vampomi_status vampomi_denoise(vampomi_ctx* ctx, const double* r1, double gam1, const double* probs,
                               const double* vars, int L, double* x1, double* x1d, double* sum_d,
                               int mem);

/* vamp::updatePrior (src/vamp.cpp:531-643): EM_max_iter EM passes over r1 (this
 * shard's M values) at noise precision gam1 for the mixture (*L, probs, vars;
 * vars ALREADY multiplied by N), then the merging of variances closer than
 * merge_vars_thr; the mixture is updated in place (*L may shrink). COLLECTIVE */
vampomi_status vampomi_update_prior(vampomi_ctx* ctx, const double* r1, double gam1, int* L, double* probs,
                                    double* vars, int EM_max_iter, double EM_err_thr, int learn_vars,
                                    double merge_vars_thr, int mem);

/* probit z-denoiser: z1[i] = g1_bin_class(p1[i], tau1, y[i]) with the context's
 * phenotype y (raw 0/1), *sum_d = sum_i g1d_bin_class(p1[i], tau1, y[i]) (local:
 * the N-side is replicated on every rank).  probit_var = 1, covariate offset 0
 * (vampomi_denoise_bin_cov with m_cov = NULL).
 * src/vamp_probit.cpp:213-233, 469-488; erfcx src/utilities.cpp:293-363 */
vampomi_status vampomi_denoise_bin(vampomi_ctx* ctx, const double* p1, double tau1, double* z1,
                                   double* sum_d, int mem);
/* the same with the covariate offsets m_cov (N, `mem`; m_cov_i = Z_i.cov_eff,
 * :213-233): g1 / g1d_bin_class(p1[i], tau1, y[i], m_cov[i]), i.e. c = (p1 +
 * m_cov)/sqrt(1 + 1/tau1).  m_cov = NULL: vampomi_denoise_bin, bit for bit */
vampomi_status vampomi_denoise_bin_cov(vampomi_ctx* ctx, const double* p1, double tau1, const double* m_cov,
                                       double* z1, double* sum_d, int mem);

/* ---- the VAMP linear and probit models (vamp::infere) ---- */
typedef struct {
    double gam1, h2;              /* --gam1, --h2 (gamw = 1/(1-h2), src/main_meth.cpp:52) */
    int max_iter, CG_max_iter;    /* --iterations, --CG-max-iter */
    double CG_err_tol;            /* --CG-err-tol */
    int EM_max_iter;              /* --EM-max-iter */
    double EM_err_thr, rho;       /* --EM-err-thr, --rho */
    int learn_vars, learn_prior_delay;
    double stop_criteria_thr, merge_vars_thr;
    int L;                        /* number of mixture components */
    double vars[VAMPOMI_MAX_L];   /* as on the command line (NOT multiplied by N) */
    double probs[VAMPOMI_MAX_L];
    uint64_t seed;                /* index-keyed Bernoulli probe seed */
    const char* out_dir;          /* NULL or "" => write no files */
    const char* out_name;
    int verbosity;
    const double* true_signal;    /* local slice (M) or NULL => zeros (host) */
    const double* x1hat_init;     /* local slice (M) or NULL => zeros (host) */
    int batch_rhs;                /* 4 (default): 3, and each CG step reads X ONCE: A^T q
                                     and A d from the same pass, with q = A p and A r
                                     carried as N-vector recurrences (one A.x pass per
                                     solve for A r0; equal up to rounding);
                                     3: 2, plus A x2 carried through the CG steps
                                     and z1 = A x1 in the first CG pass (no pass over X
                                     outside the CG; equal up to rounding); 2: 1, plus the
                                     linear model's updateNoisePrec products A^T A x2 /
                                     A^T A invQ carried through the CG steps (one pass over
                                     X fewer per iteration; equal up to rounding);
                                     1: share each A/A^T pass between the x2
                                     and Onsager CG solves (every value bitwise that of 0);
                                     0: run them back to back */
    const char* model;            /* "linear" (NULL == "linear") or "bin_class" (probit,
                                     src/vamp_probit.cpp; phenotype must be raw 0/1, i.e. read
                                     with standardize = 0; h2/gamw unused; seed also keys the
                                     Gaussian start p1; the context's covariates, if any, are
                                     fitted at vampomi_vamp_begin and offset the z-side
                                     denoiser; "linear" ignores them) */
} vampomi_params;

typedef struct {
    int iterations_run;
    /* per-iteration arrays, caller allocated (max_iter entries; may be NULL) */
    int* cg_iters;                /* k1 */
    int* ons_iters;               /* k2 */
    int* L_hist;                  /* mixture components after updatePrior */
    double* params;               /* per iteration, 5 (linear): alpha1 gam1 alpha2 gam2 gamw;
                                     8 (bin_class): alpha1 beta1 gam1 tau1 alpha2 beta2 gam2 tau2 */
    double* metrics;              /* per iteration, 6 (linear); 12 (bin_class): TP TN FP FN
                                     acc1 x1_corr TP TN FP FN acc2 x2_corr */
    double* x1_hist;              /* M per iteration: x1_hat/sqrt(N) (== _it_K.bin slice) */
    double* r1_hist;              /* M per iteration: r1/sqrt(N)     (== _r1_it_K.bin slice) */
    double* x1_final;             /* M: what vamp::infere returns: x1_hat_scaled for linear
                                     (src/vamp.cpp:437), x1_hat for bin_class (vamp_probit.cpp:465) */
    double probs_final[VAMPOMI_MAX_L];
    double vars_final[VAMPOMI_MAX_L];   /* divided by N, as printed/written */
    int L_final;
    int64_t a_passes_ref;         /* A/A^T passes the reference would have run */
    int64_t a_passes_exec;        /* passes actually executed (X streamed from HBM) */
    double* prior_hist;           /* bin_class: (1 + 2*VAMPOMI_MAX_L) per iteration: the
                                     _prior.csv row L, probs[L], vars[L] (vars x N), zero padded */
} vampomi_result;

void vampomi_params_default(vampomi_params* p);   /* src/options.hpp:62-104 defaults */
vampomi_status vampomi_infere(vampomi_ctx* ctx, const vampomi_params* p, vampomi_result* r);
/* step-wise form of vampomi_infere: begin, then one VAMP iteration per step
 * (*stopped = 1 once the stopping rule fired or max_iter was reached), end. */
vampomi_status vampomi_vamp_begin(vampomi_ctx* ctx, const vampomi_params* p, vampomi_result* r);
vampomi_status vampomi_vamp_step(vampomi_ctx* ctx, int* stopped);
vampomi_status vampomi_vamp_end(vampomi_ctx* ctx);
/* Between vampomi_vamp_begin and vampomi_vamp_end of a bin_class run: the p1
 * (N, host; may be NULL) and tau1 that the NEXT vampomi_vamp_step's z-side
 * denoiser reads (whether that step queues it or the previous one did).
 * VAMPOMI_ERR_STATE otherwise. */
vampomi_status vampomi_get_probit_state(vampomi_ctx* ctx, double* p1, double* tau1);
/* the last step's phase times as the host sees them (rank-local wall clock),
 * replacing the reference's per-iteration stopwatches "CG took" / "onsager
 * took" (src/vamp.cpp:313-316, :326-333; one interval here: both solves share
 * every pass) and "Total iteration time" (:396-401): *solve_s from the start
 * of the step's CG solves to their stop (the linear model queues their start
 * at the end of the previous step, so the device begins a little earlier),
 * *step_s the whole vampomi_vamp_step.  Either pointer may be NULL. */
vampomi_status vampomi_step_phases(vampomi_ctx* ctx, double* solve_s, double* step_s);

/* ---- association tests (--run-mode association_test) ----
 * loo: src/main_meth.cpp:245-264 + data::pvals_loo src/data.cpp:385-417.
 * est = this shard's slice of the estimate file as stored (x1_hat/sqrt(N));
 * the engine multiplies by sqrt(N), forms y_mod = y - Ax(x1_hat) (COLLECTIVE),
 * then per marker the five sums over y_mark = y_mod + X_j/sqrt(N)*x1_hat_j with
 * the RAW marker values, and linear_reg1d_pvals (src/utilities.cpp:269-282;
 * Student-t tail restated, Boost absent).  stats (5*M: sumx sumsqx sumxy sumy
 * sumsqy per marker) may be NULL.
 * se: src/main_meth.cpp:218-242, p_j = P(N(r1_j, 1/(gam1 N)) <= 0), 1 - p_j when
 * r1_j <= 0; rank-local. */
vampomi_status vampomi_assoc_loo(vampomi_ctx* ctx, const double* est, double* pvals, double* stats,
                                 int mem);
vampomi_status vampomi_assoc_se(vampomi_ctx* ctx, const double* r1, double gam1, double* pvals, int mem);
/* COLLECTIVE.  vampomi_assoc_loo for T >= 1 phenotypes against the resident
 * shard; the context's own phenotype is neither needed nor touched.
 * Y (host): T columns of N values, stride ldY >= N; each goes through what
 * vampomi_set_phen does (the covariate projection of an adjusted context,
 * then `standardize` as vampomi_set_phen's).  est: T x M, phenotype-major,
 * in `mem`, each row this shard's slice of that phenotype's estimate file;
 * NULL (on every rank) stands for all zeros, the plain marginal tests, and
 * skips the A.x passes (y_mod = y exactly).  pvals (T x M) and stats
 * (T x M x 5), in `mem`, may each be NULL.
 * The phenotypes are served in chunks of up to four: per chunk ONE A.x pass
 * with that many right-hand sides and ONE pass over the raw matrix that forms
 * all their sums (a chunk of one uses vampomi_assoc_loo's own kernel), so T
 * phenotypes read the matrix 2*ceil(T/4) times instead of 2*T.
 * Block t of pvals and stats is, bit for bit, what vampomi_set_phen(ctx, Y_t,
 * standardize) followed by vampomi_assoc_loo(ctx, est_t, ...) returns on the
 * same context under the default association-pass variant, for every storage
 * and on any number of ranks.  The pass is counted in vampomi_stats.loo
 * (bytes of a chunk of KT: esize*N*M + 8*N*KT + 8*M*6*KT).
 * VAMPOMI_ERR_ARG: T < 1, Y NULL, ldY < N; VAMPOMI_ERR_STATE: no matrix loaded. */
vampomi_status vampomi_assoc_loo_multi(vampomi_ctx* ctx, int T, const double* Y, int64_t ldY, int standardize,
                                       const double* est, double* pvals, double* stats, int mem);

/* COLLECTIVE.  The leave-one-chromosome-out test (--pval-method loco).  Every
 * local marker j has a label labels[j] in [0, G), 1 <= G <= VAMPOMI_MAX_SEGMENTS
 * (labels: M values on the host, whatever `mem`).  With x1 = est * sqrt(N) and A
 * the operator of vampomi_ax,
 *   z_c = A (x1 restricted to the markers of label c), c = 0 .. G-1: the raw
 *         partial sums of all G vectors go through ONE all-reduce and are then
 *         divided by sqrt(N); a label without markers gives zeros;
 *   z   = z_0 + z_1 + .. + z_{G-1}, added in ascending c;
 *   y_c = (y - z) + z_c, in that order: y without the fitted effect of every
 *         marker outside label c;
 * and marker j is tested marginally against y_c, c = labels[j]: the five sums
 * sumx sumsqx sumxy sumy sumsqy over the RAW column and y_c, then
 * vampomi_assoc_loo's p-value (N - 2 degrees of freedom).  A marker's sums are,
 * bit for bit, those of vampomi_assoc_loo_multi(ctx, 1, y_c, .., standardize 0,
 * est NULL, ..) on a plain context.  est == NULL (on every rank) stands for all
 * zeros: every y_c is y exactly and no A.x pass runs.
 * pvals (M), stats (5*M) in `mem`, each may be NULL; resid (host, G x N, may be
 * NULL): y_c for every c, the same on every rank.
 * Two passes over the matrix whatever G is: a segmented A.x over the markers
 * sorted by (label, index), counted in vampomi_stats.ax (K = 1), and the marker
 * pass, counted in vampomi_stats.loo; every sum has a fixed order, so the
 * results are bitwise repeatable.  Workspaces are allocated at the first call.
 * VAMPOMI_ERR_ARG: labels NULL with M > 0, G outside [1, VAMPOMI_MAX_SEGMENTS],
 * a label outside [0, G); VAMPOMI_ERR_STATE: no matrix or no phenotype. */
vampomi_status vampomi_assoc_loco(vampomi_ctx* ctx, const double* est, const int32_t* labels, int G, double* pvals,
                                  double* stats, double* resid, int mem);
/* The label file of --loco-file; needs no device.  The file holds exactly Mt
 * whitespace-separated tokens (blanks, tabs, newlines, blank lines), one per
 * marker in file order; tokens are free text ("1", "X", "chr7") and are
 * numbered by first appearance.  labels (Mt entries, may be NULL) receives the
 * numbers, *G their count, names (may be NULL) the distinct tokens in that
 * order, each followed by '\n' and the whole by a NUL, if names_cap holds them
 * (VAMPOMI_ERR_ARG otherwise).  VAMPOMI_ERR_IO: the file cannot be opened;
 * VAMPOMI_ERR_ARG: a token count other than Mt, or more than
 * VAMPOMI_MAX_SEGMENTS distinct tokens (vampomi_last_error says which). */
vampomi_status vampomi_read_labels(const char* path, int64_t Mt, int32_t* labels, int* G, char* names,
                                   size_t names_cap);

/* ---- --run-mode test (src/main_meth.cpp:112-205) ----
 * On a context holding the TEST data set (N = N_test, its own marker
 * statistics, phenotype read like the training one): x = est*sqrt(N_test),
 * z = A x (COLLECTIVE); *r2 = 1 - |y - z|^2 / (calc_stdev(y)^2 * N_test),
 * *corr2 = (<z,y> / sqrt(|z|^2 |y|^2))^2 — one row of _test.csv. */
vampomi_status vampomi_test_metrics(vampomi_ctx* ctx, const double* est, double* r2, double* corr2, int mem);

/* ---- measurement ---- */
typedef struct {
    int64_t launches;             /* kernel launches of this class that did work (exact) */
    double ms_total;              /* their device time: ms_timed / timed x launches (per K; a
                                     class's is the sum over its K) */
    double bytes_total;           /* algorithmic HBM bytes of those launches */
    double flops_total;
    int64_t timed;                /* launches timed with HIP events (vampomi_set_timing) */
    double ms_timed;              /* device time of the timed launches */
} vampomi_kernel_stat;

typedef struct {
    vampomi_kernel_stat ax;       /* A.x partial-sum kernels (all batch widths) */
    vampomi_kernel_stat atx;      /* A^T.u kernels */
    vampomi_kernel_stat ax_k[4];  /* per batch width K = 1..4 (index K-1) */
    vampomi_kernel_stat atx_k[4];
    int64_t a_passes_exec;
    int64_t host_syncs;
    vampomi_kernel_stat loo;      /* association-test pass (vampomi_assoc_loo) */
    vampomi_kernel_stat op;       /* one-pass CG operator (A^T q and A d, batch_rhs 4) */
    vampomi_kernel_stat op_k[4];  /* index K-1 for K = 1, 2 systems; index 2: launches with a third
                                     operator system; index 3: the head-start launch
                                     (one system + 3 plain A.x right-hand sides, pcg.cpp) */
    vampomi_kernel_stat coll;     /* RCCL all-reduces (several ranks): launches, bytes; with timing
                                     on, HIP events on the stream around each (its time on the
                                     stream, waits for the slowest rank included) */
} vampomi_stats;

/* HIP-event timing of the A/A^T kernels: on = 0 off, 1 every launch, n > 1 one
 * launch in n of each (kernel class, K) (each timed launch carries an event
 * pair in its dispatch, a few microseconds; the first launch of each (class, K)
 * after a reset is always timed).  Launch counts and bytes in the stats are
 * always exact; ms_total extrapolates the timed average to them. */
vampomi_status vampomi_set_timing(vampomi_ctx* ctx, int on);
vampomi_status vampomi_get_stats(vampomi_ctx* ctx, vampomi_stats* out);
vampomi_status vampomi_reset_stats(vampomi_ctx* ctx);

/* ---- development hooks (kernel tuning; not part of the reference interface) ----
 * which: 0 = A.x partial-sum kernel, 1 = A^T.u kernel, 2 = association-test pass
 * (K = 1), 3 = one-pass CG operator (K = 1, 2).  Variants index the
 * tuning tables in vampomi_amd/csrc/kernels.hip and are settings of this
 * context only; the defaults are 0 (A.x), -1 (A^T.u: the per-K choice), 16
 * (association pass: loo_wg_kernel<4,2,8>; variants 8-19 are the kernels whose
 * workgroups share their markers, and they add the sums in another order than
 * the wave-per-marker variants 0-7, so results differ at rounding level) and
 * -1 (operator: whole columns per workgroup while
 * K*N fits the LDS, else teams of workgroups; 0 forces the whole-column
 * kernel, T*10 + c (c < 10) or 1000 + T*100 + c the team kernel with team size T and configuration c,
 * vampomi_amd/csrc/atax_team.hip).  which = 4 (the side stream of rounds
 * 2-5) was removed: VAMPOMI_ERR_ARG.
 * which = 5: the CG head start of the linear model (the Onsager solve's first
 * step in the pass that starts the x2 solve, pcg.cpp), 0 off, 1 on (default
 * on; VAMPOMI_HEADSTART=0 turns it off at vampomi_open).  which = 6: the
 * linear iteration's tail without host waits on several ranks, 0 off, 1 on
 * (default on; VAMPOMI_MR_TAIL=0 turns it off at vampomi_open).  On a context
 * with several ranks, which = 3, 5 and 6 take effect at the next
 * vampomi_vamp_begin (or vampomi_infere), where the ranks agree on them: the
 * one-pass operator runs only if every rank has a plan for it, the head start
 * and the host-free tail only if every rank has them on (each changes the
 * job's collective sequence).
 * which = 7: the pre-step of the linear model on one rank (an operator slot
 * whose system has stopped forms the next Onsager solve's first CG step,
 * pcg.cpp): 0 off, 1 on at any size, 2 auto (default: on where the head start
 * runs and the X shard is at least 256 MiB; VAMPOMI_PRESTEP sets the same
 * values at vampomi_open).  Takes effect at the next iteration's solve. */
vampomi_status vampomi_dev_set_variant(vampomi_ctx* ctx, int which, int variant);
/* pre-steps made and used since vampomi_vamp_begin (which = 7 above) */
vampomi_status vampomi_dev_prestep_counts(const vampomi_ctx* ctx, int64_t* made, int64_t* used);
/* average device time (HIP events) of `reps` back-to-back launches, K RHS */
vampomi_status vampomi_dev_time_pass(vampomi_ctx* ctx, int which, int K, int reps, double* avg_ms);
/* The HBM read ceiling of this device for this shard: a pure read stream of
 * the resident matrix (every byte once, 16-byte nontemporal loads, 8-byte ones
 * of an F32 context's floats, 16-byte ones again over a U16 context's bytes (a
 * pure read is tied to no summation order): *bytes is what is resident; variant 0
 * lockstep 8-wave workgroups, one per CU, variant 1 a 1 MiB contiguous chunk
 * per wave), `reps` timed launches of each; the faster variant's median launch
 * time in *us_med, the bytes it read in *bytes, the variant in *variant.  No
 * effect on the run's state or statistics. */
vampomi_status vampomi_dev_read_ceiling(vampomi_ctx* ctx, int reps, double* us_med, double* bytes, int* variant);
/* the kernel (as rocprofv3 names it) that pass `which` with K RHS launches now
 * (mode 1: the CG form, i.e. A^T.u with the lmmse_mult epilogue, A.x with the
 * fused direction update; which = 2: the association-test pass of
 * vampomi_assoc_loo, or with K = 2, 3, 4 that of a chunk of K phenotypes of
 * vampomi_assoc_loo_multi) */
/* (an F32 / U16 context launches the narrow entry points: the same names with
 * an _f32 / _u16 suffix before the template arguments) */
vampomi_status vampomi_dev_kernel_name(const vampomi_ctx* ctx, int which, int K, int mode, char* out, int cap);
/* The A.x plan for N samples, M markers and `cus` compute units under
 * `variant` (-1 the default, 0-6 the tile plans, 7 the team plan), no device
 * needed: team size T (0: a tile plan), rows per member TR, loads per lane S,
 * workgroups grid, partial slots nslots, and the kernel name for K
 * right-hand sides. */
vampomi_status vampomi_dev_ax_plan(int64_t N, int64_t M, int cus, int variant, int K, int* T, int* TR, int* S,
                                   int* grid, int* nslots, char* name, int cap);
/* The one-pass operator's plan for N samples, M markers and `cus` compute
 * units under `variant` (as vampomi_dev_set_variant(ctx, 3, variant)), no
 * device needed: team size T (0: the whole-column kernel), loads per lane per
 * column S, rows per team member TR, workgroups grid, partial-sum slots
 * nslots, and the kernel name for K right-hand sides.  VAMPOMI_ERR_ARG if
 * no such plan exists. */
vampomi_status vampomi_dev_op_plan(int64_t N, int64_t M, int cus, int variant, int K, int* T, int* S, int* TR,
                                   int* grid, int64_t* nslots, char* name, int cap);
/* The dynamic LDS layout (in doubles) a team-plan operator launch with K
 * systems uses for that plan, no device needed: out[0] head words (the folded
 * CG decision), [1] q offset, [2] q stride, [3] wave partials offset, [4]
 * hand-off totals offset, [5] total words.  The kernel's pointers, the plan's
 * feasibility check and the launch size all come from this one layout.
 * VAMPOMI_ERR_ARG if there is no such team plan (or it is the whole-column
 * kernel's). */
vampomi_status vampomi_dev_op_lds(int64_t N, int64_t M, int cus, int variant, int K, int64_t* out);
/* The plan of launches with a THIRD operator system (vampomi_dev_op_apply3)
 * beside the plan vampomi_dev_op_plan gives for the same arguments, no device
 * needed: team size T (2..16), S, TR, grid, the team kernel configuration cfg,
 * nslots, the kernel name, and (lds not null) its dynamic LDS layout with
 * three systems as vampomi_dev_op_lds gives it.  The same for every storage of
 * X.  VAMPOMI_ERR_ARG if there is none (whole-column and T = 1 plans, N beyond
 * 16 members' rows). */
vampomi_status vampomi_dev_op3_plan(int64_t N, int64_t M, int cus, int variant, int* T, int* S, int* TR, int* grid,
                                    int* cfg, int64_t* nslots, char* name, int cap, int64_t* lds);
/* Experiment builds only (atax_team.hip compiled with TM_TS=1, and
 * VAMPOMI_OP_TS=1 set before the context's first operator use): the last
 * operator launch's per-workgroup {start, end, XCC id, HW_ID} (s_memrealtime
 * ticks, 100 MHz), *n = min(cap, 4 x grid) words. VAMPOMI_ERR_STATE otherwise. */
vampomi_status vampomi_dev_op_timestamps(vampomi_ctx* ctx, unsigned long long* out, int cap, int* n);
/* Device bytes the context of `rank` (of nranks, markers split by
 * vampomi_divide_work) allocates for a VAMP run on N samples and Mt markers
 * with `cus` compute units: the shard, marker statistics, scratch, the
 * one-pass operator's buffers and the run state (probit != 0: the probit
 * model's too); the per-iteration output writer stages in pinned host memory
 * (`writer` is kept for the ABI and ignored).  No device needed; RCCL's
 * buffers and the HIP runtime are not included. */
vampomi_status vampomi_dev_mem_plan(int64_t N, int64_t Mt, int nranks, int rank, int cus, int probit, int writer,
                                    int64_t* bytes);
/* vampomi_dev_mem_plan with the storage named (the entry point above means
 * VAMPOMI_STORE_F64): VAMPOMI_STORE_F32 is smaller by the shard's M*ld*4
 * bytes, VAMPOMI_STORE_U16 by M*ld*6.  VAMPOMI_ERR_ARG for any other storage. */
vampomi_status vampomi_dev_mem_plan_storage(int64_t N, int64_t Mt, int nranks, int rank, int cus, int probit,
                                            int writer, int storage, int64_t* bytes);
/* One application of the one-pass CG operator (K <= 2 systems, one rank),
 * host buffers: q_k = ar_k/diag [+ beta_k*qo_k], p_k [= z_k + beta_k*p_k]
 * when z is not null (then qo and beta are required), and
 *   d_k = tau * A^T q_k + gam2 * p_k   (M doubles each, k-major),
 *   ad_k = A d_k                      (N doubles each),
 *   dp_k = <d_k, p_k>.
 * ar, qo: K x N; p, z: K x M. */
vampomi_status vampomi_dev_op_apply(vampomi_ctx* ctx, int K, const double* ar, const double* qo, const double* p,
                                    const double* z, const double* beta, double diag, double tau, double gam2,
                                    double* d, double* ad, double* dp);
/* One launch with THREE operator systems (one rank; VAMPOMI_ERR_ARG where the
 * context's plan has no 3-system plan beside it): systems 0 and 1 as
 * vampomi_dev_op_apply takes them with K = 2, and in the third slot the
 * alternate system on ar3 (N) and p3 (M) with diag = tau = 1, gam2 = 0 and no
 * direction update: d_2 = A^T ar3, ad_2 = A d_2.  d: 3 x M, ad: 3 x N, dp: 2
 * (the third slot has no <d, p>). */
vampomi_status vampomi_dev_op_apply3(vampomi_ctx* ctx, const double* ar, const double* qo, const double* p,
                                     const double* z, const double* beta, double diag, double tau, double gam2,
                                     const double* ar3, const double* p3, double* d, double* ad, double* dp);

#ifdef __cplusplus
}
#endif
#endif
