// slice_host.cpp -- slice_core.hpp compiled for the host (tests/test_slice_core_cpu.py), plainly and under ASan + UBSan.
//   slice_host predicates   every (pos, cov, beg, end) of a small box against loops written out here; prints the number of cases
//   slice_host splice       stdin: "n  out_off[0..n]  a b" per line; prints head_beg head_end blk0 blk1 tail_beg tail_end
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/slice_core.hpp"

using namespace sbx;

static int predicates() {
    long cases = 0;
    for (int ref = -1; ref <= 2; ++ref)
        for (int pos = -1; pos <= 9; ++pos)
            for (unsigned cov = 0; cov <= 6; ++cov)
                for (unsigned beg = 0; beg <= 9; ++beg) {
                    // R1 of region (1, beg, .): on the contig, starts in front of beg, some covered position is >= beg ... and it is beg
                    bool want = false;
                    if (ref == 1 && pos < (int)beg)
                        for (unsigned k = 0; k < cov; ++k) want = want || pos + (int)k == (int)beg;
                    if (slicec::in_r1(ref, pos, cov, 1u, beg) != want) { printf("in_r1 ref=%d pos=%d cov=%u beg=%u\n", ref, pos, cov, beg); return 1; }
                    // R1 is the overlap with [beg, end) of a record that starts in front: the same for every end behind beg
                    for (unsigned end = beg + 1; end <= 11; ++end) {
                        const bool ov = viewc::overlaps(ref, pos, cov, 1u, beg, end) && pos < (int)beg;
                        if (ov != want) { printf("overlap ref=%d pos=%d cov=%u beg=%u end=%u\n", ref, pos, cov, beg, end); return 1; }
                        ++cases;
                    }
                    const bool ge = ref < 0 || ref > 1 || (ref == 1 && pos >= (int)beg);
                    if (slicec::at_or_behind(ref, pos, 1u, beg) != ge) { printf("at_or_behind ref=%d pos=%d beg=%u\n", ref, pos, beg); return 1; }
                    // a record is never both in R1 and at or behind beg; with cov == 0 or pos == beg it is not in R1
                    if (want && ge) return 1;
                    if ((cov == 0 || pos == (int)beg) && slicec::in_r1(ref, pos, cov, 1u, beg)) return 1;
                }
    printf("%ld\n", cases);
    return 0;
}

static int splice_lines() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t n = 0;
        in >> n;
        std::vector<uint64_t> off(n + 1);
        for (auto& o : off) in >> o;
        uint64_t a = 0, b = 0;
        in >> a >> b;
        const slicec::Splice s = slicec::splice(a, b, off.data(), n);
        printf("%llu %llu %u %u %llu %llu\n", (unsigned long long)s.head_beg, (unsigned long long)s.head_end, s.blk0, s.blk1,
               (unsigned long long)s.tail_beg, (unsigned long long)s.tail_end);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "predicates")) return predicates();
    if (argc == 2 && !strcmp(argv[1], "splice")) return splice_lines();
    fprintf(stderr, "usage: slice_host predicates|splice\n");
    return 2;
}
