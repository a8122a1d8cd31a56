// hostio.h — byte-compatible file formats of gVAMPomi (host C++).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace vio {

// PLINK "FID IID value" rows, std::regex("\\s+") token split
// (src/data.cpp:58-110).  Returns rows read, -1 cannot open, -2 "NA".
int64_t read_phen(const std::string& path, std::vector<double>& y);
// read_phen's standardisation: scale to unit variance, NOT centred
// (src/data.cpp:97-104).  Returns the scale factor.
double standardize_phen(std::vector<double>& y);

// read_phen's rows with their IDs, "NA" kept as a flag instead of ending the
// read: fid / iid are tokens 0 and 1 of the same split, na[i] says token 2 ==
// "NA" (value[i] is then 0).  False: cannot open.
struct PhenTable {
    std::vector<std::string> fid, iid;
    std::vector<double> value;
    std::vector<char> na;
};
bool read_phen_table(const std::string& path, PhenTable& t);
// The rows of a phenotype file that an analysis keeps, ascending.  keep_path
// ("" for none): PLINK --keep style, per non-blank line FID and IID (tokens 0
// and 1 of read_phen's split, further fields ignored); a row is kept iff its
// pair is named, whatever the keep file's order or duplicates.  drop_na: rows
// with "NA" are dropped too; else an "NA" in a row that would be kept is an
// error.  0 ok; -1 a file cannot be opened; -2 that "NA"; -3 a keep line
// without two fields, or a pair that is in no phenotype row (*err names the
// pair and its line).  *N_file: the file's rows; *not_kept / *na_dropped: the
// rows the keep file and the "NA"s took out (each may be null).
int phen_rows(const std::string& phen_path, const std::string& keep_path, bool drop_na, std::vector<int64_t>& rows,
              int64_t* N_file, int64_t* not_kept, int64_t* na_dropped, std::string* err);
// The rows that an analysis of all the phenotype files keeps: phen_rows per
// file, intersected, each file parsed once.  The files must have the same
// number of rows and the same (FID, IID) sequence, else -3 naming the first
// differing file and row; a -2 names the file when there are several.
// *na_per_file: the "NA"s in each file's rows that the keep file names;
// *values: each file's values, all its rows ("NA" as 0) (each may be null).
int phen_rows_common(const std::vector<std::string>& phen_paths, const std::string& keep_path, bool drop_na,
                     std::vector<int64_t>& rows, int64_t* N_file, int64_t* not_kept,
                     std::vector<int64_t>* na_per_file, std::vector<std::vector<double>>* values, std::string* err);

// The label file of the leave-one-chromosome-out test (--loco-file): exactly Mt
// whitespace-separated tokens (any mix of blanks, tabs, newlines, blank lines),
// one per marker in file order, free text; labels[i] numbers marker i's token
// by first appearance, names[c] is token c and counts[c] its markers.  0 ok;
// -1 cannot open; -2 a token count other than Mt; -3 more than max_labels
// distinct tokens (*err says what was found).
int read_labels(const std::string& path, int64_t Mt, int max_labels, std::vector<int32_t>& labels,
                std::vector<std::string>& names, std::vector<int64_t>& counts, std::string* err);

// data::read_covariates (src/data.cpp:159-227): a header line, then per row
// two IDs and exactly C numeric fields, split like read_phen's.  out: C
// columns of N (covariate-major).  0 ok; -1 cannot open; -2 a row without
// exactly C fields (the reference's FATAL line is printed to stdout, where the
// reference exits); -3 not N rows; -4 a field that is not a number.  *err
// receives the message.  C == 0: nothing is read (:161-162).
int read_covariates(const std::string& path, int64_t N, int C, bool standardize, double* out, std::string* err);
// its standardisation (:205-226), per column (stride ld): mean and population
// standard deviation (divided by N) accumulated in long double; a column with
// csig < 1e-8 becomes zeros, else (v - mean)/csig
void standardize_covariates(double* Z, int64_t N, int C, int64_t ld);

// mpi_store_vec_to_file (src/utilities.cpp:241-249): CREATE|WRONLY without
// truncation, M doubles at byte offset S*8.
bool store_vec(const std::string& path, const double* v, int64_t S, int64_t M);
// mpi_read_vec_from_file (src/utilities.cpp:251-267): M doubles from byte S*8;
// missing bytes (short file) read as 0.
bool read_vec(const std::string& path, double* v, int64_t S, int64_t M);

// read_vec_from_file (src/utilities.cpp:104-122): whitespace-separated text,
// values with index [S, S+M); missing ones stay as they are (callers zero).
bool read_text_vec(const std::string& path, double* v, int64_t S, int64_t M);

// setup_io + write_ofile_csv_header (src/vamp.cpp:854-882,
// src/utilities.cpp:388-401): delete, create exclusively, header at offset 0.
bool csv_create_with_header(const std::string& path, const std::vector<std::string>& fields);
// setup_io alone: delete, create exclusively, no header (the probit path
// writes none, src/vamp_probit.cpp)
bool csv_create(const std::string& path);
// write_ofile_csv (src/utilities.cpp:366-385): "%5d" + n x ", %20.15f" + "\n"
// at byte offset it * strlen(row).
bool csv_write_row(const std::string& path, int it, const double* vals, int n);
std::string csv_format_row(int it, const double* vals, int n);

// Rendezvous file of a multi-process CLI job (replaces mpirun's bootstrap):
// rank 0 publishes the RCCL id, the other ranks fetch it.  The file carries a
// run nonce (VAMPOMI_RUN_ID, torchrun's TORCHELASTIC_RUN_ID, the MPI / PMIx
// job namespace, slurm's job.step, else MASTER_ADDR:MASTER_PORT); a reader
// accepts only a file with its own nonce.  Without any of them: only a file
// written after not_before (seconds since the epoch) whose id is still there,
// unchanged, 3 s later (rank 0 of a new job replaces a stale file as it
// starts).  Rank 0 removes the file once the communicator is up (rdzv_remove).
std::string rdzv_nonce();
bool rdzv_publish(const std::string& path, const std::string& nonce, const void* id, int nbytes);
bool rdzv_fetch(const std::string& path, const std::string& nonce, double not_before, void* id, int nbytes,
                int timeout_ms);
void rdzv_remove(const std::string& path);

}  // namespace vio
