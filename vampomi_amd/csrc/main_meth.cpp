// main_meth.cpp — drop-in for the reference's main_meth.exe (src/main_meth.cpp)
// in --run-mode infere (--model linear | bin_class), test and
// association_test (--pval-method loo | se): same flags, same output files.
//
// Ranks: the reference is launched with `mpirun -np P`; this binary runs one
// process per GPU, rank/size from VAMPOMI_RANK/VAMPOMI_NRANKS (or the
// torchrun variables RANK/WORLD_SIZE, LOCAL_RANK for the device).  The RCCL
// communicator id is handed from rank 0 to the others through a rendezvous
// file (VAMPOMI_RDZV, default <out-dir>/.<out-name>.rdzv).
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vampomi.h"
#include "hostio.h"
#include "options.h"

static int env_int(const char* a, const char* b, int dflt) {
    const char* v = std::getenv(a);
    if (!v && b) v = std::getenv(b);
    return v ? std::atoi(v) : dflt;
}

// rank 0 publishes the RCCL id (removing any file an earlier job left there),
// the others wait for a file of THIS job (vio::rdzv_*) up to
// VAMPOMI_RDZV_TIMEOUT_S (default 120 s, the bench's collective limit: the
// ranks of one job start together, so a longer wait means rank 0 is gone)
static bool exchange_id(const std::string& path, int rank, double not_before, unsigned char* id) {
    const std::string nonce = vio::rdzv_nonce();
    if (rank == 0) return vampomi_comm_unique_id(id) == VAMPOMI_OK && vio::rdzv_publish(path, nonce, id, VAMPOMI_UNIQUE_ID_BYTES);
    const char* e = std::getenv("VAMPOMI_RDZV_TIMEOUT_S");
    const double s = e && std::atof(e) > 0 ? std::atof(e) : 120.0;
    return vio::rdzv_fetch(path, nonce, not_before, id, VAMPOMI_UNIQUE_ID_BYTES, (int)(s * 1000.0));
}

static vampomi_ctx* g_ctx = nullptr;  // the open context: die() ends the job's communicator

static int die(const char* what) {
    std::cout << "FATAL  : " << what << ": " << vampomi_last_error() << std::endl;
    if (g_ctx) vampomi_comm_abort(g_ctx);
    return EXIT_FAILURE;
}

// a rank-local outcome every rank must share before the next collective:
// false on every rank if it is false on any (src/main_meth.cpp exits rank-locally)
static bool all_ok(vampomi_ctx* ctx, bool ok) {
    int all = 0;
    if (vampomi_all_ok(ctx, ok ? 1 : 0, &all) != VAMPOMI_OK) return false;
    return all != 0;
}

// the iteration number of an estimate / r1 file name: the text between the
// last "it_" and the last ".bin" (src/main_meth.cpp:223-226, :249-252)
static bool iteration_of(const std::string& name, std::string& it_str) {
    const size_t pos1 = name.rfind("it_") + 3, pos2 = name.rfind(".bin");
    try {
        it_str = name.substr(pos1, pos2 - pos1);
        (void)std::stoi(it_str);
    } catch (...) {
        return false;
    }
    return true;
}

// --run-mode association_test (src/main_meth.cpp:206-264)
static int association_test(vampomi_ctx* ctx, const vopt::Options& opt, int rank, int64_t M, int64_t S,
                            const std::vector<int32_t>& labels, int G) {
    std::vector<double> in((size_t)std::max<int64_t>(M, 1)), pvals((size_t)std::max<int64_t>(M, 1));
    std::string it_str, out;
    if (opt.pval_method == "se") {
        if (!iteration_of(opt.r1_file, it_str)) {
            std::cout << "FATAL  : cannot parse the iteration from --r1-file \"" << opt.r1_file << "\"" << std::endl;
            return EXIT_FAILURE;
        }
        if (rank == 0) std::cout << opt.r1_file << std::endl;
        vio::read_vec(opt.r1_file, in.data(), S, M);
        if (vampomi_assoc_se(ctx, in.data(), opt.gam1, pvals.data(), VAMPOMI_MEM_HOST) != VAMPOMI_OK)
            return die("association test (se)");
        out = opt.out_dir + "/" + opt.out_name + "_it_" + it_str + "_pval_se.bin";
    } else if (opt.pval_method == "loo") {
        if (!iteration_of(opt.estimate_file, it_str)) {
            std::cout << "FATAL  : cannot parse the iteration from --estimate-file \"" << opt.estimate_file << "\""
                      << std::endl;
            return EXIT_FAILURE;
        }
        vio::read_vec(opt.estimate_file, in.data(), S, M);
        if (vampomi_assoc_loo(ctx, in.data(), pvals.data(), nullptr, VAMPOMI_MEM_HOST) != VAMPOMI_OK)
            return die("association test (loo)");
        out = opt.out_dir + "/" + opt.out_name + "_it_" + it_str + "_pval_loo.bin";
    } else if (opt.pval_method == "loco") {
        if (!iteration_of(opt.estimate_file, it_str)) {
            std::cout << "FATAL  : cannot parse the iteration from --estimate-file \"" << opt.estimate_file << "\""
                      << std::endl;
            return EXIT_FAILURE;
        }
        vio::read_vec(opt.estimate_file, in.data(), S, M);
        // (labels holds all Mt: this rank's slice is [S, S + M))
        if (vampomi_assoc_loco(ctx, in.data(), labels.data() + S, G, pvals.data(), nullptr, nullptr,
                               VAMPOMI_MEM_HOST) != VAMPOMI_OK)
            return die("association test (loco)");
        out = opt.out_dir + "/" + opt.out_name + "_it_" + it_str + "_pval_loco.bin";
    } else {
        return 0;  // the reference computes nothing for another --pval-method
    }
    if (rank == 0) std::cout << "Storing p-values to file " + out << std::endl;
    if (!vio::store_vec(out, pvals.data(), S, M)) {
        std::cout << "FATAL  : cannot write " << out << std::endl;
        return EXIT_FAILURE;
    }
    return 0;
}

// --trait-file: one phenotype per non-blank, non-# line, "<name> <phen-file>
// <estimate-file>".  False with *err set: a line without three fields, a
// duplicate name, an estimate name without a parsable it_K, no line at all
struct Trait {
    std::string name, phen, est, it_str;
};
static bool read_traits(const std::string& path, std::vector<Trait>& traits, std::string* err) {
    std::ifstream in(path);
    if (!in.is_open()) {
        *err = "could not open trait file: " + path;
        return false;
    }
    std::string line;
    for (int64_t lineno = 1; std::getline(in, line); ++lineno) {
        std::istringstream ls(line);
        std::vector<std::string> tok;
        for (std::string w; ls >> w;) tok.push_back(w);
        if (tok.empty() || tok[0][0] == '#') continue;
        const std::string where = "trait file " + path + ", line " + std::to_string(lineno) + ": ";
        if (tok.size() != 3) {
            *err = where + "expected <name> <phen-file> <estimate-file>, found " + std::to_string(tok.size()) +
                   (tok.size() == 1 ? " field" : " fields");
            return false;
        }
        Trait t{tok[0], tok[1], tok[2], ""};
        for (const Trait& o : traits)
            if (o.name == t.name) {
                *err = where + "duplicate name \"" + t.name + "\"";
                return false;
            }
        if (!iteration_of(t.est, t.it_str)) {
            *err = where + "cannot parse the iteration from estimate file \"" + t.est + "\"";
            return false;
        }
        traits.push_back(t);
    }
    if (traits.empty()) {
        *err = "trait file " + path + " names no phenotype";
        return false;
    }
    return true;
}

// --run-mode association_test --pval-method loo --trait-file: every trait's
// p-values from one load of the matrix (vampomi_assoc_loo_multi), each to the
// file a single run with --out-name <name> writes.  Y: T columns of n;
// standardize: as the single run's phenotype (raw 0/1 for --model bin_class)
static int association_test_traits(vampomi_ctx* ctx, const vopt::Options& opt, const std::vector<Trait>& traits,
                                   const std::vector<double>& Y, int64_t n, int standardize, int rank, int64_t M,
                                   int64_t S) {
    const size_t T = traits.size(), Mx = (size_t)std::max<int64_t>(M, 1);
    std::vector<double> est(T * Mx, 0.0), pvals(T * Mx, 0.0);
    for (size_t t = 0; t < T; ++t) vio::read_vec(traits[t].est, est.data() + t * (size_t)M, S, M);
    if (vampomi_assoc_loo_multi(ctx, (int)T, Y.data(), n, standardize, est.data(), pvals.data(), nullptr,
                                VAMPOMI_MEM_HOST) != VAMPOMI_OK)
        return die("association test (loo, several phenotypes)");
    for (size_t t = 0; t < T; ++t) {
        const std::string out = opt.out_dir + "/" + traits[t].name + "_it_" + traits[t].it_str + "_pval_loo.bin";
        if (rank == 0) std::cout << "Storing p-values to file " + out << std::endl;
        if (!vio::store_vec(out, pvals.data() + t * (size_t)M, S, M)) {
            std::cout << "FATAL  : cannot write " << out << std::endl;
            return EXIT_FAILURE;
        }
    }
    return 0;
}

// --run-mode test (src/main_meth.cpp:112-205): R2 and squared correlation of
// A.x_est on the test set for the estimate files of iterations
// --test-iter-range, one _test.csv row each.
static int test_run(vampomi_ctx* ctx, const vopt::Options& opt, int rank, int64_t M, int64_t S) {
    const std::string csv = opt.out_dir + "/" + opt.out_name + "_test.csv";
    const bool made = rank != 0 || vio::csv_create_with_header(csv, {"iteration", "R2 test", "z correlation test"});
    if (!all_ok(ctx, made)) {
        std::cout << "FATAL  : cannot create " << csv << std::endl;
        return EXIT_FAILURE;
    }
    // file names: <prefix>it_<it>.<ext>, prefix up to the last "it", ext after
    // the FIRST '.' of the given name (:152-168)
    const std::string& est = opt.estimate_file;
    const size_t pos_dot = est.find('.');
    const std::string ext = pos_dot == std::string::npos ? std::string() : est.substr(pos_dot + 1);
    const size_t pos_it = est.rfind("it");
    if (rank == 0) std::cout << "est_file_name = " << est << std::endl;
    const int min_it = opt.test_iter_range.size() > 0 ? opt.test_iter_range[0] : 1;
    const int max_it = opt.test_iter_range.size() > 1 ? opt.test_iter_range[1] : min_it;
    if (rank == 0) std::cout << "iter range = [" << min_it << ", " << max_it << "]" << std::endl;
    std::vector<double> x((size_t)std::max<int64_t>(M, 1));
    for (int it = min_it; it <= max_it; ++it) {
        const std::string name = est.substr(0, pos_it) + "it_" + std::to_string(it) + "." + ext;
        std::fill(x.begin(), x.end(), 0.0);
        const bool ok = ext == "bin" ? vio::read_vec(name, x.data(), S, M) : vio::read_text_vec(name, x.data(), S, M);
        if (!all_ok(ctx, ok)) {
            std::cout << "FATAL  : cannot read estimate file " << name << std::endl;
            return EXIT_FAILURE;
        }
        double row[2];
        if (vampomi_test_metrics(ctx, x.data(), &row[0], &row[1], VAMPOMI_MEM_HOST) != VAMPOMI_OK)
            return die("test metrics");
        if (rank == 0) std::cout << row[0] << ", ";
        if (!all_ok(ctx, rank != 0 || vio::csv_write_row(csv, it, row, 2))) {
            std::cout << "FATAL  : cannot write " << csv << std::endl;
            return EXIT_FAILURE;
        }
    }
    if (rank == 0) std::cout << std::endl;
    return 0;
}

int main(int argc, char** argv) {
    vopt::Options opt;
    std::string echo;
    const int rank = env_int("VAMPOMI_RANK", "RANK", 0);
    const int nranks = env_int("VAMPOMI_NRANKS", "WORLD_SIZE", 1);
    if (!vopt::parse(argc, argv, opt, echo)) return EXIT_FAILURE;
    if (rank == 0) std::cout << echo << std::endl;

    int64_t M = 0, S = 0, Mm = 0;
    vampomi_divide_work(opt.Mt, nranks, rank, &M, &S, &Mm);
    std::printf("INFO   : rank %4d has %lld markers over tot Mt = %u, max Mm = %lld, starting at S = %lld\n", rank,
                (long long)M, opt.Mt, (long long)Mm, (long long)S);

    if (opt.run_mode != "infere" && opt.run_mode != "association_test" && opt.run_mode != "test") {
        std::cout << "FATAL  : run mode \"" << opt.run_mode
                  << "\" is not provided by this build (infere, test, association_test)" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.model != "linear" && opt.model != "bin_class") {  // src/vamp.cpp:98-104
        std::cout << "FATAL  : Invalid model specification! (\"" << opt.model << "\")" << std::endl;
        return EXIT_FAILURE;
    }

    // --keep-file / --phen-na drop: the rows of the files that the run keeps,
    // on the host and on every rank before any device call, so that a bad keep
    // file or an NA that is fatal ends the job here on all of them.  --N /
    // --N-test stay the files' rows; the context is opened with the kept ones
    const bool test_mode = opt.run_mode == "test";  // the context holds the TEST data set (:128)
    const std::string& keep = test_mode ? opt.keep_file_test : opt.keep_file;
    const bool subset = !keep.empty() || opt.phen_na == "drop";
    const int64_t N_file = test_mode ? opt.N_test : opt.N;
    std::vector<int64_t> rows;
    // --trait-file: the traits, then the rows that all their phenotype files
    // keep (vio::phen_rows_common also holds the files to one sequence of
    // individuals), on every rank before any device call as well.  Y: the kept
    // rows of every trait's values; the context needs no phenotype of its own
    std::vector<Trait> traits;
    std::vector<double> Y;
    if (!opt.trait_file.empty()) {
        std::string err;
        if (!read_traits(opt.trait_file, traits, &err)) {
            std::cout << "FATAL  : " << err << std::endl;
            return EXIT_FAILURE;
        }
        std::vector<std::string> paths;
        for (const Trait& t : traits) paths.push_back(t.phen);
        std::vector<int64_t> nas;
        std::vector<std::vector<double>> values;  // every file is parsed once, here
        int64_t nf = 0, out = 0;
        if (vio::phen_rows_common(paths, keep, opt.phen_na == "drop", rows, &nf, &out, &nas, &values, &err) != 0) {
            std::cout << "FATAL  : sample subset: " << err << std::endl;
            return EXIT_FAILURE;
        }
        if (nf != N_file) {
            std::cout << "FATAL  : sample subset: the phenotype files have " << nf << " rows, --N is " << N_file
                      << std::endl;
            return EXIT_FAILURE;
        }
        if (rows.size() < 2) {
            std::cout << "FATAL  : sample subset: " << rows.size() << " of " << N_file
                      << " samples are kept (at least 2 are needed)" << std::endl;
            return EXIT_FAILURE;
        }
        for (const std::vector<double>& v : values)  // the kept rows of every trait's values, T columns of n
            for (const int64_t r : rows) Y.push_back(v[(size_t)r]);
        if (subset && rank == 0) {
            std::cout << "INFO   : kept " << rows.size() << " of " << N_file << " samples (" << out
                      << " not in the keep file, " << N_file - out - (int64_t)rows.size() << " with an NA phenotype)"
                      << std::endl;
            bool any = false;
            for (const int64_t v : nas) any = any || v != 0;
            if (any) {
                std::cout << "INFO   : NA phenotypes:";
                for (size_t t = 0; t < traits.size(); ++t) std::cout << " " << traits[t].name << " " << nas[t];
                std::cout << std::endl;
            }
        }
    } else if (subset) {
        int64_t nf = 0, out = 0, nas = 0;
        std::string err;
        if (vio::phen_rows(test_mode ? opt.phen_file_test : opt.phen_file, keep, opt.phen_na == "drop", rows, &nf, &out,
                           &nas, &err) != 0) {
            std::cout << "FATAL  : sample subset: " << err << std::endl;
            return EXIT_FAILURE;
        }
        if (nf != N_file) {
            std::cout << "FATAL  : sample subset: the phenotype file has " << nf << " rows, "
                      << (test_mode ? "--N-test" : "--N") << " is " << N_file << std::endl;
            return EXIT_FAILURE;
        }
        if (rows.size() < 2) {
            std::cout << "FATAL  : sample subset: " << rows.size() << " of " << N_file
                      << " samples are kept (at least 2 are needed)" << std::endl;
            return EXIT_FAILURE;
        }
        if (rank == 0)
            std::cout << "INFO   : kept " << rows.size() << " of " << N_file << " samples (" << out
                      << " not in the keep file, " << nas << " with an NA phenotype)" << std::endl;
    }
    const int64_t n = subset ? (int64_t)rows.size() : N_file;

    // --pval-method loco: the label file, all of it on every rank, before any
    // device call, so that a bad file ends the job here on all of them
    std::vector<int32_t> labels;
    int G = 0;
    if (!opt.loco_file.empty()) {
        std::vector<std::string> names;
        std::vector<int64_t> counts;
        std::string err;
        if (vio::read_labels(opt.loco_file, (int64_t)opt.Mt, VAMPOMI_MAX_SEGMENTS, labels, names, counts, &err) != 0) {
            std::cout << "FATAL  : --loco-file: " << err << std::endl;
            return EXIT_FAILURE;
        }
        G = (int)names.size();
        if (labels.empty()) labels.push_back(0);  // (never read: a non-null pointer)
        if (rank == 0) {
            std::cout << "INFO   : LOCO: " << G << " segments (";
            for (int c = 0; c < G; ++c) std::cout << (c ? " " : "") << names[(size_t)c] << ":" << counts[(size_t)c];
            std::cout << ")" << std::endl;
        }
    }

    // data::read_covariates (src/data.cpp:159-227), on every rank, before any
    // device call: a malformed table ends the job here as it ends the
    // reference's (every rank reads the same file and fails alike).  Only the
    // probit model uses them (src/vamp_probit.cpp:62-95)
    const bool use_cov = opt.run_mode == "infere" && opt.model == "bin_class" && opt.C > 0;
    std::vector<double> covs;
    if (use_cov) {
        if (opt.C <= VAMPOMI_MAX_C) covs.assign((size_t)opt.C * (size_t)opt.N, 0.0);
        // (with a subset: raw, the kept rows are taken and standardised below)
        if (vampomi_parse_covariates(opt.cov_file.c_str(), (int64_t)opt.N, (int)opt.C, subset ? 0 : 1, covs.data()) !=
            VAMPOMI_OK)
            return die("covariates");
        if (subset && opt.C <= VAMPOMI_MAX_C) {
            std::vector<double> kept((size_t)opt.C * (size_t)n);
            for (unsigned j = 0; j < opt.C; ++j)
                for (int64_t i = 0; i < n; ++i) kept[(size_t)j * n + i] = covs[(size_t)j * opt.N + rows[(size_t)i]];
            covs.swap(kept);
        }
    } else if (opt.run_mode == "infere" && opt.C > 0 && rank == 0 && opt.cov_adjust != "residual") {
        std::cout << "INFO   : --C " << opt.C << ": covariates are used by --model bin_class only and are ignored"
                  << std::endl;
    }
    // --cov-adjust residual (the linear model; vopt::parse has checked the
    // flags): the raw table of the files' rows, of which the kept ones are
    // taken, on every rank before any device call, as above
    const bool adjust = opt.cov_adjust == "residual";
    std::vector<double> adj;
    if (adjust) {
        if (opt.C <= VAMPOMI_MAX_C) adj.assign((size_t)opt.C * (size_t)N_file, 0.0);
        if (vampomi_parse_covariates((test_mode ? opt.cov_file_test : opt.cov_file).c_str(), N_file, (int)opt.C, 0,
                                     adj.data()) != VAMPOMI_OK)
            return die("covariate adjustment");
        if (subset) {
            std::vector<double> kept((size_t)opt.C * (size_t)n);
            for (unsigned j = 0; j < opt.C; ++j)
                for (int64_t i = 0; i < n; ++i) kept[(size_t)j * n + i] = adj[(size_t)j * N_file + rows[(size_t)i]];
            adj.swap(kept);
        }
    }

    unsigned char id[VAMPOMI_UNIQUE_ID_BYTES] = {0};
    std::string rdzv_path;
    // launch time (a job without a run nonce accepts only rendezvous files
    // written after it, minus a margin for ranks that start late)
    const double t_start = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    if (nranks > 1) {
        const char* rz = std::getenv("VAMPOMI_RDZV");
        const std::string path = rz ? rz : opt.out_dir + "/." + opt.out_name + ".rdzv";
        if (!exchange_id(path, rank, t_start - 120.0, id)) return die("communicator rendezvous failed");
        rdzv_path = path;
    }
    vampomi_shard_desc d{};
    d.N = n;
    d.Mt = opt.Mt;
    d.rank = rank;
    d.nranks = nranks;
    d.device = env_int("LOCAL_RANK", nullptr, -1);
    d.comm_id = nranks > 1 ? id : nullptr;
    d.alpha_scale = opt.alpha_scale;
    vampomi_ctx* ctx = nullptr;
    if (vampomi_open(&d, &ctx) != VAMPOMI_OK) return die("cannot open the device context");
    g_ctx = ctx;
    // (without the flag the context keeps its default, VAMPOMI_STORAGE included)
    if (opt.meth_storage_set &&
        vampomi_set_storage(ctx, opt.meth_storage == "u16"   ? VAMPOMI_STORE_U16
                                 : opt.meth_storage == "f32" ? VAMPOMI_STORE_F32
                                                             : VAMPOMI_STORE_F64) != VAMPOMI_OK)
        return die("methylation storage");
    if (subset && vampomi_set_row_subset(ctx, N_file, rows.data(), n) != VAMPOMI_OK) return die("sample subset");
    // (without the flag no call: the load is what it was)
    if (opt.meth_na != "pass" &&
        vampomi_set_meth_na(ctx, opt.meth_na == "mean" ? VAMPOMI_NA_MEAN : VAMPOMI_NA_FATAL, opt.meth_na_max_frac) !=
            VAMPOMI_OK)
        return die("missing-value policy");
    if (adjust) {  // (after the row subset, before the phenotype)
        if (vampomi_set_adjust(ctx, adj.data(), (int)opt.C, n) != VAMPOMI_OK) return die("covariate adjustment");
        int R = 0;
        std::vector<int> dropped((size_t)opt.C, 0);
        if (vampomi_get_adjust(ctx, &R, dropped.data(), nullptr) != VAMPOMI_OK) return die("covariate adjustment");
        if (rank == 0) {
            std::string names;
            for (unsigned j = 0; j < opt.C; ++j)
                if (dropped[j]) names += (names.empty() ? "" : ", ") + std::to_string(j);
            std::cout << "INFO   : adjusting for " << R - 1 << " of " << opt.C << " covariates + intercept (dropped: "
                      << (names.empty() ? "none" : names) << ")" << std::endl;
        }
    }
    // every rank has joined the communicator (its init is collective): the
    // rendezvous file has served and must not be read by a later job
    if (rank == 0 && !rdzv_path.empty()) vio::rdzv_remove(rdzv_path);

    // data::data: phenotype first (standardised for the linear model, raw 0/1
    // for bin_class, src/data.cpp:40-43), then the shard
    auto t0 = std::chrono::steady_clock::now();
    const int standardize = opt.model == "bin_class" ? 0 : 1;
    const std::string& phen = test_mode ? opt.phen_file_test : opt.phen_file;
    const std::string& meth = test_mode ? opt.meth_file_test : opt.meth_file;
    if (traits.empty() && vampomi_read_phen(ctx, phen.c_str(), standardize) != VAMPOMI_OK) return die("phenotype");
    if (rank == 0) std::cout << "meth file name = " << meth << std::endl;
    if ((opt.meth_dtype == "u16"   ? vampomi_load_meth_file_u16(ctx, meth.c_str())
         : opt.meth_dtype == "f32" ? vampomi_load_meth_file_f32(ctx, meth.c_str())
                                   : vampomi_load_meth_file(ctx, meth.c_str())) != VAMPOMI_OK)
        return die("methylation data");
    {  // what --meth-na mean found in this rank's shard
        int64_t missing = 0, with = 0, masked = 0;
        if (vampomi_get_missing_stats(ctx, &missing, &with, &masked, nullptr) != VAMPOMI_OK)
            return die("missing-value counts");
        if (missing)
            std::printf("INFO   : markers [%lld, %lld): %lld missing values in %lld markers, %lld masked\n",
                        (long long)S, (long long)(S + M), (long long)missing, (long long)with, (long long)masked);
    }
    if (adjust) {  // the markers of this rank's shard with nothing left outside the covariates' span
        int64_t absorbed = 0;
        if (vampomi_get_adjust_stats(ctx, &absorbed, nullptr) != VAMPOMI_OK) return die("covariate adjustment");
        if (absorbed)
            std::printf("INFO   : markers [%lld, %lld): %lld absorbed by the covariates\n", (long long)S,
                        (long long)(S + M), (long long)absorbed);
    }
    // the ranks' shards load at their own pace (one rank's file may come off
    // slower storage): they meet here under a limit of their own, so the
    // first collective of the run is not the one that waits for the slowest
    // load under VAMPOMI_COLL_TIMEOUT_S
    if (nranks > 1) {
        const char* lt = std::getenv("VAMPOMI_LOAD_TIMEOUT_S");
        const double lim = lt && std::atof(lt) > 0 ? std::atof(lt) : 3600.0;
        if (vampomi_barrier_timeout(ctx, lim) != VAMPOMI_OK) return die("waiting for the other ranks' shards");
    }
    if (rank == 0)
        std::cout << "reading methylation data took "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " seconds."
                  << std::endl;

    if (opt.run_mode == "association_test" || test_mode) {
        const int rc = test_mode          ? test_run(ctx, opt, rank, M, S)
                       : !traits.empty() ? association_test_traits(ctx, opt, traits, Y, n, standardize, rank, M, S)
                                         : association_test(ctx, opt, rank, M, S, labels, G);
        vampomi_barrier(ctx);
        vampomi_close(ctx);
        return rc;
    }

    std::vector<double> ts, init;
    if (!opt.true_signal_file.empty()) {  // src/main_meth.cpp:69-73
        ts.assign((size_t)M, 0.0);
        vio::read_vec(opt.true_signal_file, ts.data(), S, M);
    }
    if (!opt.estimate_file.empty()) {  // src/main_meth.cpp:75-80
        init.assign((size_t)M, 0.0);
        vio::read_vec(opt.estimate_file, init.data(), S, M);
    }

    vampomi_params p;
    vampomi_params_default(&p);
    p.gam1 = opt.gam1;
    p.h2 = opt.h2;
    p.max_iter = (int)opt.iterations;
    p.CG_max_iter = (int)opt.CG_max_iter;
    p.CG_err_tol = opt.CG_err_tol;
    p.EM_max_iter = (int)opt.EM_max_iter;
    p.EM_err_thr = opt.EM_err_thr;
    p.rho = opt.rho;
    p.learn_vars = (int)opt.learn_vars;
    p.learn_prior_delay = (int)opt.learn_prior_delay;
    p.stop_criteria_thr = opt.stop_criteria_thr;
    p.merge_vars_thr = opt.merge_vars_thr;
    if (opt.vars.size() != opt.probs.size() || opt.vars.empty() || opt.vars.size() > VAMPOMI_MAX_L) {
        std::cout << "FATAL  : --vars and --probs must have the same number (1.." << VAMPOMI_MAX_L << ") of entries"
                  << std::endl;
        return EXIT_FAILURE;
    }
    p.L = (int)opt.vars.size();
    for (int j = 0; j < p.L; ++j) {
        p.vars[j] = opt.vars[j];
        p.probs[j] = opt.probs[j];
    }
    p.seed = opt.seed;
    p.out_dir = opt.out_dir.c_str();
    p.out_name = opt.out_name.c_str();
    p.verbosity = opt.verbosity;
    p.true_signal = ts.empty() ? nullptr : ts.data();
    p.x1hat_init = init.empty() ? nullptr : init.data();
    p.batch_rhs = opt.batch_rhs;
    p.model = opt.model.c_str();

    std::vector<int> cg((size_t)p.max_iter), ons((size_t)p.max_iter);
    vampomi_result r{};
    r.cg_iters = cg.data();
    r.ons_iters = ons.data();
    // vampomi_infere step by step, so that every iteration reports its time
    // as the reference does (src/vamp.cpp:396-401, rank 0): one step is one
    // iteration, and the host waits once per iteration, at its end
    auto t1 = std::chrono::steady_clock::now();
    if (use_cov && vampomi_set_covariates(ctx, covs.data(), (int)opt.C, n, subset ? 1 : 0) != VAMPOMI_OK)
        return die("covariates");
    if (vampomi_vamp_begin(ctx, &p, &r) != VAMPOMI_OK) return die("inference");
    if (use_cov) {  // src/vamp_probit.cpp:84-91, and the effects as a file
        std::vector<double> eff((size_t)opt.C);
        if (vampomi_get_cov_eff(ctx, eff.data()) != VAMPOMI_OK) return die("covariate effects");
        if (rank == 0) {
            for (unsigned i0 = 0; i0 < opt.C; i0++) {
                std::cout << "cov_eff[" << i0 << "] = " << eff[i0] << ", ";
                if (i0 % 4 == 3) std::cout << std::endl;
            }
            std::cout << std::endl;
            if (!opt.out_dir.empty()) {
                const std::string path = opt.out_dir + "/" + opt.out_name + "_cov_eff.bin";
                ::unlink(path.c_str());
                if (!vio::store_vec(path, eff.data(), 0, (int64_t)opt.C)) {
                    std::cout << "FATAL  : cannot write " << path << std::endl;
                    vampomi_comm_abort(ctx);
                    return EXIT_FAILURE;
                }
            }
        }
    }
    double total = 0.0;
    for (int stopped = 0; !stopped;) {
        const auto ts0 = std::chrono::steady_clock::now();
        if (vampomi_vamp_step(ctx, &stopped) != VAMPOMI_OK) return die("inference");
        const double it_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - ts0).count();
        total += it_s;
        const int it = r.iterations_run;
        double solve_s = 0.0;
        if (vampomi_step_phases(ctx, &solve_s, nullptr) != VAMPOMI_OK) return die("inference");
        if (rank == 0 && it >= 1)
            std::cout << "it " << it << ": CG iterations " << cg[it - 1] << ", onsager CG iterations " << ons[it - 1]
                      << "\nCG and onsager (one pass over the markers per step for both) took " << solve_s
                      << " seconds.\nTotal iteration time = " << it_s << "\nTotal computation time so far = " << total
                      << std::endl;
    }
    if (vampomi_vamp_end(ctx) != VAMPOMI_OK) return die("inference");
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    if (rank == 0)
        std::cout << "iterations run = " << r.iterations_run << ", total computation time = " << secs
                  << " s, A-passes executed = " << r.a_passes_exec << " (reference-equivalent " << r.a_passes_ref
                  << ")" << std::endl;
    vampomi_barrier(ctx);
    vampomi_close(ctx);
    return 0;
}
