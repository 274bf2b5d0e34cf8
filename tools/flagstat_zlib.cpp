// flagstat_zlib.cpp -- the CPU yardstick of `sbx-flagstat`: one thread inflates a BAM with zlib block by block
// and counts the records the way computeFlagStatistics does (sambamba/flagstat.d:31-58).  A timing tool, not a test oracle
// (tests/flagstat_ref.py is that).  Prints the 13 lines of the plain form (counts only) and the wall time on stderr.
//   make flagstat_zlib && ./flagstat_zlib file.bam
#include <zlib.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: flagstat_zlib file.bam\n"); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<uint8_t> in(65536), u;
    uint64_t c[13][2] = {};
    size_t at = 0;          // first byte of U not yet consumed
    bool header = true;
    unsigned char hd[18];
    while (fread(hd, 1, 18, f) == 18) {
        const unsigned bsize = hd[16] | hd[17] << 8;            // BC subfield right behind XLEN = 6 (every BGZF writer)
        if (fread(in.data(), 1, bsize + 1 - 18, f) != bsize + 1 - 18) { fprintf(stderr, "truncated\n"); return 1; }
        uint32_t isize;
        memcpy(&isize, in.data() + bsize + 1 - 18 - 4, 4);
        if (!isize) break;
        const size_t old = u.size();
        u.resize(old + isize);
        z_stream z{};
        inflateInit2(&z, -15);
        z.next_in = in.data(); z.avail_in = bsize + 1 - 26;
        z.next_out = u.data() + old; z.avail_out = isize;
        if (inflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "bad deflate stream\n"); return 1; }
        inflateEnd(&z);
        if (header) {
            if (u.size() < 12) continue;
            int32_t l_text, n_ref;
            memcpy(&l_text, &u[4], 4);
            size_t p = 8 + (size_t)l_text;
            if (u.size() < p + 4) continue;
            memcpy(&n_ref, &u[p], 4);
            p += 4;
            bool whole = true;
            for (int32_t r = 0; r < n_ref && whole; ++r) {
                int32_t l;
                if (u.size() < p + 4) { whole = false; break; }
                memcpy(&l, &u[p], 4);
                p += 8 + (size_t)l;
                whole = u.size() >= p;
            }
            if (!whole) continue;
            at = p;
            header = false;
        }
        for (;;) {
            int32_t bs;
            if (u.size() - at < 4) break;
            memcpy(&bs, &u[at], 4);
            if (u.size() - at < 4 + (size_t)bs) break;
            int32_t ref, next_ref;
            uint32_t bmn, fnc;
            memcpy(&ref, &u[at + 4], 4); memcpy(&bmn, &u[at + 12], 4); memcpy(&fnc, &u[at + 16], 4); memcpy(&next_ref, &u[at + 24], 4);
            const uint32_t flag = fnc >> 16, mapq = (bmn >> 8) & 0xFF, fl = (flag & 0x200) ? 1 : 0;
            ++c[0][fl];
            if (!(flag & 0x4)) ++c[4][fl];
            if (flag & 0x400) ++c[3][fl];
            if (flag & 0x100) ++c[1][fl];
            else if (flag & 0x800) ++c[2][fl];
            else if (flag & 0x1) {
                ++c[5][fl];
                if ((flag & 0x2) && !(flag & 0x4)) ++c[8][fl];
                if (flag & 0x40) ++c[6][fl];
                if (flag & 0x80) ++c[7][fl];
                if ((flag & 0x8) && !(flag & 0x4)) ++c[10][fl];
                if (!(flag & 0x4) && !(flag & 0x8)) {
                    ++c[9][fl];
                    if (ref != next_ref) { ++c[11][fl]; if (mapq >= 5) ++c[12][fl]; }
                }
            }
            at += 4 + (size_t)bs;
        }
        u.erase(u.begin(), u.begin() + (ptrdiff_t)at);   // keep the unfinished record
        at = 0;
    }
    fclose(f);
    const char* names[13] = {"in total", "secondary", "supplementary", "duplicates", "mapped", "paired in sequencing", "read1", "read2",
                             "properly paired", "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
                             "with mate mapped to a different chr (mapQ>=5)"};
    for (int k = 0; k < 13; ++k) printf("%llu + %llu %s\n", (unsigned long long)c[k][0], (unsigned long long)c[k][1], names[k]);
    fprintf(stderr, "flagstat_zlib: %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
