// hostio.cpp — gVAMPomi file formats (see hostio.h for the reference lines).
#include "hostio.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <fstream>
#include <iterator>
#include <map>
#include <set>
#include <thread>

#include <sys/stat.h>

namespace vio {

static bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; }

// std::sregex_token_iterator over "\\s+" with submatch -1: the text between
// whitespace runs; a leading run gives an empty first token, a trailing one
// no token
static void split_ws(const std::string& line, std::vector<std::string>& tok) {
    tok.clear();
    size_t i = 0;
    const size_t n = line.size();
    for (;;) {
        size_t j = i;
        while (j < n && !is_ws(line[j])) ++j;
        if (j == n) {  // suffix after the last separator: only if non-empty
            if (j > i || tok.empty()) tok.push_back(line.substr(i, j - i));
            break;
        }
        tok.push_back(line.substr(i, j - i));  // text before a separator (may be empty)
        while (j < n && is_ws(line[j])) ++j;
        i = j;
        if (i == n) break;
    }
}

int64_t read_phen(const std::string& path, std::vector<double>& y) {
    std::ifstream in(path);
    if (!in.is_open()) return -1;
    y.clear();
    std::string line;
    std::vector<std::string> tok;
    while (std::getline(in, line)) {
        // third token of the "\\s+" split with submatch -1: a leading run of
        // whitespace produces an empty first token.
        split_ws(line, tok);
        if (tok.size() < 3) continue;
        if (tok[2] == "NA") return -2;
        y.push_back(std::atof(tok[2].c_str()));
    }
    return (int64_t)y.size();
}

bool read_phen_table(const std::string& path, PhenTable& t) {
    std::ifstream in(path);
    if (!in.is_open()) return false;
    t = PhenTable();
    std::string line;
    std::vector<std::string> tok;
    while (std::getline(in, line)) {
        split_ws(line, tok);  // read_phen's rows: the lines with a third token
        if (tok.size() < 3) continue;
        const bool na = tok[2] == "NA";
        t.fid.push_back(tok[0]);
        t.iid.push_back(tok[1]);
        t.na.push_back(na ? 1 : 0);
        t.value.push_back(na ? 0.0 : std::atof(tok[2].c_str()));
    }
    return true;
}

// named[i]: the keep file names row i of t (all rows without a keep file).
// 0, or phen_rows' -1 / -3
static int keep_mask(const PhenTable& t, const std::string& phen_path, const std::string& keep_path,
                     std::vector<char>& named, std::string* err) {
    typedef std::pair<std::string, std::string> Id;
    std::map<Id, int64_t> keep;  // the pair and the first line that names it
    named.assign(t.value.size(), 1);
    if (!keep_path.empty()) {
        std::ifstream in(keep_path);
        if (!in.is_open()) {
            *err = "FATAL: could not open keep file: " + keep_path;
            return -1;
        }
        std::string line;
        std::vector<std::string> tok;
        int64_t lineno = 0;
        while (std::getline(in, line)) {
            ++lineno;
            bool blank = true;
            for (const char ch : line) blank = blank && is_ws(ch);
            if (blank) continue;
            split_ws(line, tok);
            if (tok.size() < 2) {
                *err = "keep file " + keep_path + ", line " + std::to_string(lineno) + ": expected FID and IID";
                return -3;
            }
            keep.emplace(Id(tok[0], tok[1]), lineno);
        }
        std::set<Id> have;
        for (size_t i = 0; i < t.fid.size(); ++i) have.insert(Id(t.fid[i], t.iid[i]));
        const std::pair<const Id, int64_t>* missing = nullptr;  // the one named first in the keep file
        for (const auto& k : keep)
            if (!have.count(k.first) && (!missing || k.second < missing->second)) missing = &k;
        if (missing) {
            *err = "keep file " + keep_path + ", line " + std::to_string(missing->second) + ": no individual \"" +
                   missing->first.first + " " + missing->first.second + "\" in phenotype file " + phen_path;
            return -3;
        }
        for (size_t i = 0; i < t.value.size(); ++i) named[i] = keep.count(Id(t.fid[i], t.iid[i])) ? 1 : 0;
    }
    return 0;
}

// the named rows without an "NA", ascending.  0, or phen_rows' -2
static int rows_of(const std::vector<char>& named, const std::vector<char>& na, bool drop_na,
                   std::vector<int64_t>& rows, int64_t* na_dropped, std::string* err) {
    rows.clear();
    int64_t nas = 0;
    for (size_t i = 0; i < named.size(); ++i) {
        if (!named[i]) continue;
        if (na[i]) {
            if (!drop_na) {
                *err = "NAN in data!";
                return -2;
            }
            ++nas;
            continue;
        }
        rows.push_back((int64_t)i);
    }
    if (na_dropped) *na_dropped = nas;
    return 0;
}

int phen_rows(const std::string& phen_path, const std::string& keep_path, bool drop_na, std::vector<int64_t>& rows,
              int64_t* N_file, int64_t* not_kept, int64_t* na_dropped, std::string* err) {
    PhenTable t;
    if (!read_phen_table(phen_path, t)) {
        *err = "FATAL: could not open phenotype file: " + phen_path;
        return -1;
    }
    std::vector<char> named;
    if (const int rc = keep_mask(t, phen_path, keep_path, named, err)) return rc;
    if (const int rc = rows_of(named, t.na, drop_na, rows, na_dropped, err)) return rc;
    if (N_file) *N_file = (int64_t)t.value.size();
    if (not_kept) *not_kept = (int64_t)std::count(named.begin(), named.end(), (char)0);
    return 0;
}

int phen_rows_common(const std::vector<std::string>& phen_paths, const std::string& keep_path, bool drop_na,
                     std::vector<int64_t>& rows, int64_t* N_file, int64_t* not_kept,
                     std::vector<int64_t>* na_per_file, std::vector<std::vector<double>>* values, std::string* err) {
    const size_t T = phen_paths.size();
    PhenTable first;
    std::vector<std::vector<char>> na(T);
    if (values) values->assign(T, std::vector<double>());
    for (size_t t = 0; t < T; ++t) {  // every file once: its values and NA flags, its IDs held against the first's
        PhenTable cur;
        PhenTable& tab = t == 0 ? first : cur;
        if (!read_phen_table(phen_paths[t], tab)) {
            *err = "FATAL: could not open phenotype file: " + phen_paths[t];
            return -1;
        }
        if (t > 0 && cur.value.size() != first.value.size()) {
            *err = "phenotype file " + phen_paths[t] + " has " + std::to_string(cur.value.size()) + " rows, " +
                   phen_paths[0] + " has " + std::to_string(first.value.size());
            return -3;
        }
        for (size_t i = 0; t > 0 && i < cur.value.size(); ++i)
            if (cur.fid[i] != first.fid[i] || cur.iid[i] != first.iid[i]) {
                *err = "phenotype file " + phen_paths[t] + ", row " + std::to_string(i + 1) + ": individual \"" +
                       cur.fid[i] + " " + cur.iid[i] + "\" where " + phen_paths[0] + " has \"" + first.fid[i] + " " +
                       first.iid[i] + "\"";
                return -3;
            }
        na[t] = tab.na;
        if (values) (*values)[t] = tab.value;
    }
    std::vector<char> named;  // (the same individuals in every file: one mask)
    if (const int rc = keep_mask(first, phen_paths[0], keep_path, named, err)) return rc;
    if (na_per_file) na_per_file->assign(T, 0);
    std::vector<int64_t> cur, both;
    for (size_t t = 0; t < T; ++t) {
        if (const int rc = rows_of(named, na[t], drop_na, cur, na_per_file ? &(*na_per_file)[t] : nullptr, err)) {
            if (T > 1) *err += " (phenotype file " + phen_paths[t] + ")";
            return rc;
        }
        if (t == 0) {
            rows.swap(cur);
        } else {
            both.clear();
            std::set_intersection(rows.begin(), rows.end(), cur.begin(), cur.end(), std::back_inserter(both));
            rows.swap(both);
        }
    }
    if (N_file) *N_file = (int64_t)first.value.size();
    if (not_kept) *not_kept = (int64_t)std::count(named.begin(), named.end(), (char)0);
    return 0;
}

void standardize_covariates(double* Z, int64_t N, int C, int64_t ld) {
    for (int j = 0; j < C; ++j) {  // src/data.cpp:205-226
        double* col = Z + (int64_t)j * ld;
        long double cavg = 0.0, csig = 0.0;
        for (int64_t i = 0; i < N; ++i) cavg += col[i];
        cavg = cavg / double(N);
        for (int64_t i = 0; i < N; ++i) csig += ((col[i] - cavg) * (col[i] - cavg));
        csig = std::sqrt(csig / double(N));
        for (int64_t i = 0; i < N; ++i) {
            if (csig < 0.00000001)
                col[i] = 0;
            else
                col[i] = (double)((col[i] - cavg) / csig);
        }
    }
}

int read_labels(const std::string& path, int64_t Mt, int max_labels, std::vector<int32_t>& labels,
                std::vector<std::string>& names, std::vector<int64_t>& counts, std::string* err) {
    std::ifstream in(path);
    if (!in) {
        if (err) *err = "cannot open label file " + path;
        return -1;
    }
    labels.clear();
    names.clear();
    counts.clear();
    std::map<std::string, int32_t> seen;
    std::string tok;
    int64_t n = 0;
    while (in >> tok) {  // operator>> splits on any run of whitespace
        ++n;
        if (n > Mt) continue;  // (counted on, for the message)
        auto it = seen.find(tok);
        if (it == seen.end()) {
            if ((int)names.size() == max_labels) {
                if (err)
                    *err = "label file " + path + " has more than " + std::to_string(max_labels) +
                           " distinct labels (the next is '" + tok + "' at marker " + std::to_string(n - 1) + ")";
                return -3;
            }
            it = seen.emplace(tok, (int32_t)names.size()).first;
            names.push_back(tok);
            counts.push_back(0);
        }
        labels.push_back(it->second);
        counts[it->second]++;
    }
    if (n != Mt) {
        if (err)
            *err = "label file " + path + " has " + std::to_string(n) + " labels, expected " + std::to_string(Mt) +
                   " (one per marker)";
        return -2;
    }
    return 0;
}

int read_covariates(const std::string& path, int64_t N, int C, bool standardize, double* out, std::string* err) {
    if (C == 0) return 0;  // :161-162
    std::ifstream in(path);
    if (!in.is_open()) {
        *err = "FATAL: could not open covariate file: " + path;
        return -1;
    }
    std::string line;
    std::vector<std::string> tok;
    int64_t row = 0, lineno = 0;
    while (std::getline(in, line)) {
        if (++lineno == 1) continue;  // the header (:176)
        split_ws(line, tok);
        const int Cobs = tok.size() > 2 ? (int)(tok.size() - 2) : 0;  // after the two IDs (:183-184)
        if (Cobs != C) {  // :191-194 (the reference exits here)
            std::printf("FATAL: number of covariates = %d does not match to the specified number of covariates = %d\n",
                        Cobs, C);
            std::fflush(stdout);
            *err = "FATAL: number of covariates = " + std::to_string(Cobs) +
                   " does not match to the specified number of covariates = " + std::to_string(C);
            return -2;
        }
        if (row < N) {
            for (int j = 0; j < C; ++j) {
                const char* s = tok[2 + j].c_str();
                char* end = nullptr;
                const double v = std::strtod(s, &end);  // std::stod (:187)
                if (end == s) {
                    *err = "covariate file " + path + ": \"" + tok[2 + j] + "\" is not a number";
                    return -4;
                }
                out[(int64_t)j * N + row] = v;
            }
        }
        ++row;
    }
    if (row != N) {  // (the reference would index covs[i] out of bounds, :210-225)
        *err = "covariate rows (" + std::to_string(row) + ") != N (" + std::to_string(N) + ")";
        return -3;
    }
    if (standardize) standardize_covariates(out, N, C, N);
    return 0;
}

double standardize_phen(std::vector<double>& y) {
    double sum = 0.0;
    for (double v : y) sum += v;
    const int64_t nonas = (int64_t)y.size();
    const double avg = sum / double(nonas);
    double sqn = 0.0;
    for (size_t i = 0; i < y.size(); ++i)
        if (y[i] != DBL_MAX) sqn += (y[i] - avg) * (y[i] - avg);
    sqn = std::sqrt(double(nonas - 1) / sqn);
    for (size_t i = 0; i < y.size(); ++i) y[i] *= sqn;
    return sqn;
}

bool store_vec(const std::string& path, const double* v, int64_t S, int64_t M) {
    int fd = ::open(path.c_str(), O_CREAT | O_WRONLY, 0666);
    if (fd < 0) return false;
    const size_t want = (size_t)M * sizeof(double);
    size_t done = 0;
    while (done < want) {
        ssize_t w = ::pwrite(fd, (const char*)v + done, want - done, (off_t)S * 8 + (off_t)done);
        if (w <= 0) break;
        done += (size_t)w;
    }
    ::close(fd);
    return done == want;
}

bool read_vec(const std::string& path, double* v, int64_t S, int64_t M) {
    int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    std::memset(v, 0, (size_t)M * sizeof(double));
    const size_t want = (size_t)M * sizeof(double);
    size_t done = 0;
    while (done < want) {
        ssize_t r = ::pread(fd, (char*)v + done, want - done, (off_t)S * 8 + (off_t)done);
        if (r <= 0) break;
        done += (size_t)r;
    }
    ::close(fd);
    return true;
}

bool csv_create_with_header(const std::string& path, const std::vector<std::string>& fields) {
    ::unlink(path.c_str());
    int fd = ::open(path.c_str(), O_CREAT | O_WRONLY | O_EXCL, 0666);
    if (fd < 0) return false;
    std::string s = fields.empty() ? std::string() : fields[0];
    for (size_t i = 1; i < fields.size(); ++i) s += ", " + fields[i];
    s += "\n";
    ssize_t w = ::pwrite(fd, s.data(), s.size(), 0);
    ::close(fd);
    return w == (ssize_t)s.size();
}

bool read_text_vec(const std::string& path, double* v, int64_t S, int64_t M) {
    std::ifstream f(path);
    if (!f) return false;
    double value;
    int64_t it = 0;
    while (f >> value) {
        if (it >= S + M) break;
        if (it >= S) v[it - S] = value;
        ++it;
    }
    return true;
}

bool csv_create(const std::string& path) {
    ::unlink(path.c_str());
    int fd = ::open(path.c_str(), O_CREAT | O_WRONLY | O_EXCL, 0666);
    if (fd < 0) return false;
    ::close(fd);
    return true;
}

std::string csv_format_row(int it, const double* vals, int n) {
    char buf[50000];
    int cx = std::snprintf(buf, sizeof buf, "%5d", it);
    for (int i = 0; i < n; ++i) cx += std::snprintf(buf + cx, sizeof buf - (size_t)cx, ", %20.15f", vals[i]);
    cx += std::snprintf(buf + cx, sizeof buf - (size_t)cx, "\n");
    return std::string(buf, (size_t)cx);
}

bool csv_write_row(const std::string& path, int it, const double* vals, int n) {
    const std::string row = csv_format_row(it, vals, n);
    int fd = ::open(path.c_str(), O_WRONLY);
    if (fd < 0) return false;
    ssize_t w = ::pwrite(fd, row.data(), row.size(), (off_t)it * (off_t)row.size());
    ::close(fd);
    return w == (ssize_t)row.size();
}

static const char kRdzvMagic[] = "VAMPOMI-RDZV1";

std::string rdzv_nonce() {
    // a job id every rank of the job sees: ours, torchrun's, the MPI / PMIx
    // namespace (mpirun), slurm's job and step
    for (const char* v : {"VAMPOMI_RUN_ID", "TORCHELASTIC_RUN_ID", "PMIX_NAMESPACE", "OMPI_MCA_ess_base_jobid",
                          "PMI_KVSNAME"}) {
        const char* e = std::getenv(v);
        if (e && *e) return std::string(v) + "=" + e;
    }
    const char* sj = std::getenv("SLURM_JOB_ID");
    const char* ss = std::getenv("SLURM_STEP_ID");
    if (sj && *sj) return std::string("slurm=") + sj + "." + (ss ? ss : "");
    const char* a = std::getenv("MASTER_ADDR");
    const char* p = std::getenv("MASTER_PORT");
    if (a && p && *a && *p) return std::string("master=") + a + ":" + p;
    return std::string();
}

// magic '\n' nonce '\n' id bytes, written to path.tmp and renamed into place
// (readers never see a partial file); any file already at path is removed first
bool rdzv_publish(const std::string& path, const std::string& nonce, const void* id, int nbytes) {
    ::unlink(path.c_str());
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        if (!f) return false;
        f << kRdzvMagic << '\n' << nonce << '\n';
        f.write((const char*)id, nbytes);
        if (!f.good()) return false;
    }
    return std::rename(tmp.c_str(), path.c_str()) == 0;
}

static bool rdzv_try(const std::string& path, const std::string& nonce, double not_before, void* id, int nbytes) {
    struct stat st;
    if (::stat(path.c_str(), &st) != 0) return false;
    if (nonce.empty() && (double)st.st_mtime < not_before) return false;  // an earlier job's file
    std::ifstream f(path, std::ios::binary);
    std::string magic, n;
    if (!std::getline(f, magic) || magic != kRdzvMagic || !std::getline(f, n) || n != nonce) return false;
    f.read((char*)id, nbytes);
    return f.gcount() == nbytes;
}

bool rdzv_fetch(const std::string& path, const std::string& nonce, double not_before, void* id, int nbytes,
                int timeout_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<unsigned char> first((size_t)nbytes), again((size_t)nbytes);
    for (;;) {
        // checked on every path round the loop: a file rewritten or flapping
        // within the recheck below must not keep this rank here past the limit
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms)) return false;
        if (rdzv_try(path, nonce, not_before, first.data(), nbytes)) {
            if (!nonce.empty()) {
                std::memcpy(id, first.data(), (size_t)nbytes);
                return true;
            }
            // No job id: a file left by an earlier job whose rank 0 died before
            // removing it could pass the time window.  Rank 0 of THIS job
            // replaces any such file as it starts; accept only an id that is
            // still there, unchanged, 3 s later.
            std::this_thread::sleep_for(std::chrono::seconds(3));
            if (rdzv_try(path, nonce, not_before, again.data(), nbytes) &&
                std::memcmp(first.data(), again.data(), (size_t)nbytes) == 0) {
                std::memcpy(id, again.data(), (size_t)nbytes);
                return true;
            }
            continue;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
}

void rdzv_remove(const std::string& path) { ::unlink(path.c_str()); }

}  // namespace vio
