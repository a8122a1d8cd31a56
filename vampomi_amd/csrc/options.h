// options.h — main_meth.exe command line (restates src/options.hpp / options.cpp)
#pragma once
#include <string>
#include <vector>

namespace vopt {

struct Options {
    std::string meth_file, meth_file_test, phen_file, phen_file_test, true_signal_file;
    std::string estimate_file, r1_file, cov_estimate_file, cov_file, cov_file_test;
    std::string run_mode = "infere", out_dir, out_name, model = "linear", pval_method = "se";
    double stop_criteria_thr = 0.01, merge_vars_thr = 5e-1, EM_err_thr = 1e-2;
    unsigned EM_max_iter = 1, CG_max_iter = 500;
    double CG_err_tol = 1e-5;
    unsigned Mt = 0, N = 0, N_test = 0, Mt_test = 0, num_mix_comp = 10, learn_vars = 1, learn_prior_delay = 1;
    double alpha_scale = 1.0;
    unsigned redglob = 0, C = 0;
    double probit_var = 1, rho = 0.5, h2 = 0.5, gam1 = 1e-6;
    int verbosity = 0;
    unsigned iterations = 50;
    std::vector<double> vars{0, 1e-06, 6e-06, 3e-05, 2e-04, 1e-03, 6e-03, 3e-02, 2e-01, 1e+00};
    std::vector<double> probs{9.90000e-01, 5.00000e-03, 2.50000e-03, 1.25000e-03, 6.25000e-04,
                              3.12500e-04, 1.56250e-04, 7.81250e-05, 3.90625e-05, 3.90625e-05};
    std::vector<int> test_iter_range{1, 50};
    // engine extensions (not in the reference): Bernoulli seed, RHS batching
    unsigned long long seed = 0x5EED5EEDULL;
    int batch_rhs = 4;
    // how the methylation shard is held on the device (--meth-storage) and the
    // element type of --meth-file / --meth-file-test (--meth-dtype): f64 | f32 | u16
    // (u16: 16-bit fixed point, k * 2^-16)
    std::string meth_storage = "f64", meth_dtype = "f64";
    bool meth_storage_set = false;  // --meth-storage was given (else the context's default stands)
    // the samples of the files that the run keeps: --keep-file / --keep-file-test
    // (PLINK --keep style, FID and IID per line; the latter for the test-mode
    // trio) and --phen-na fatal | drop (an NA phenotype ends the job, the
    // reference's behaviour, or drops its row).  --N / --N-test stay the files' rows
    std::string keep_file, keep_file_test, phen_na = "fatal";
    // missing methylation values (NaN) in --meth-file / --meth-file-test:
    // --meth-na pass | fatal | mean (nobody looks; the load fails; the marker's
    // mean is stored) and, with mean, --meth-na-max-frac F in [0, 1]: a marker
    // with more than F of its entries missing is stored as zeros
    std::string meth_na = "pass";
    double meth_na_max_frac = 1.0;
    bool meth_na_max_frac_set = false;
    // --cov-adjust none | residual: with residual the linear model's matrix and
    // phenotype are replaced at ingest by their residuals on the intercept and
    // the --C columns of --cov-file (--cov-file-test in --run-mode test)
    std::string cov_adjust = "none";
    // --trait-file F (--run-mode association_test --pval-method loo only):
    // several phenotypes against one load of the matrix; per non-blank, non-#
    // line of F: <name> <phen-file> <estimate-file>.  Stands instead of
    // --phen-file / --estimate-file
    std::string trait_file;
    std::string loco_file;  // --pval-method loco: one label per marker (vio::read_labels)
};

// Parses argv exactly like Options::read_command_line_options + check_options:
// on a bad or unknown flag prints the reference's FATAL message to stdout and
// returns false (the CLI then exits with EXIT_FAILURE).  `echo` receives the
// "ardyh command line options" summary.
bool parse(int argc, char** argv, Options& o, std::string& echo);

}  // namespace vopt
