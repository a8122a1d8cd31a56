// Stand-alone driver of the kept-rows reader (vio::phen_rows, vio::read_phen_table)
// for tests/test_row_subset.py, which builds it with the sanitizers:
//   phen_rows_harness <phen> <keep | -> <drop_na>
// prints: status [N_file not_kept na_dropped rows...]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hostio.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string keep = std::string(argv[2]) == "-" ? std::string() : std::string(argv[2]);
    std::vector<int64_t> rows;
    int64_t nf = 0, out = 0, nas = 0;
    std::string err;
    const int st = vio::phen_rows(argv[1], keep, std::atoi(argv[3]) != 0, rows, &nf, &out, &nas, &err);
    std::printf("%d", st);
    if (st == 0) {
        std::printf(" %lld %lld %lld", (long long)nf, (long long)out, (long long)nas);
        for (const int64_t r : rows) std::printf(" %lld", (long long)r);
        vio::PhenTable t;  // the table agrees with the rows
        if (!vio::read_phen_table(argv[1], t) || (int64_t)t.value.size() != nf || t.na.size() != t.value.size() ||
            t.fid.size() != t.value.size() || t.iid.size() != t.value.size())
            return 3;
        for (const int64_t r : rows)
            if (t.na[(size_t)r]) return 4;
    } else if (err.empty()) {
        return 5;
    }
    std::printf("\n");
    return 0;
}
