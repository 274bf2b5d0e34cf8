// fasta_host.cpp -- sambamba_amd/csrc/fasta_core.hpp and bins_core.hpp on the CPU (tests/test_fasta_core_cpu.py), through the very
// functions the library compiles.
//   fasta_host fai      stdin: one hex-encoded FASTA text per line ("-": empty).  Every text goes through the chunk-and-carry logic at
//                       chunk sizes 16, 32, 48, 4096 and whole; what the kernels compute for a chunk is restated serially
//                       (chunk_result_serial) with the kernels' own per-line functions.  Every chunk lies in an allocation of exactly
//                       its size, so a sanitizer build sees every read behind it.  Per text and size one row:
//                       "<text number> <chunk size> ok <hex of the .fai>|-" or "... seq" or "... bare <count> <first line>".
//   fasta_host reg2bin  stdin: "beg end" per line -> sampc::reg2bin(beg, end) per line
//   fasta_host records  stdin: one hex-encoded BAM record (from its block_size field on) per line -> "ok <expected bin> <stored bin>"
//                       or "bad" (binc::expected_bin; the record lies in an allocation of exactly its size)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/bins_core.hpp"
#include "../../sambamba_amd/csrc/fasta_core.hpp"

using namespace sbx;

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    out.reserve(h.size() / 2);
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((uint8_t)(v(h[k]) << 4 | v(h[k + 1])));
    return out;
}

static std::string hex(const std::string& s) {
    static const char* digits = "0123456789abcdef";
    std::string h;
    for (unsigned char c : s) { h.push_back(digits[c >> 4]); h.push_back(digits[c & 15]); }
    return h.empty() ? "-" : h;
}

// what sbx_index_fasta does with a file, the device's part restated serially
static std::string index_text(const std::vector<uint8_t>& text, uint64_t chunk) {
    fastac::FastaCarry carry;
    if (!text.empty() && text[0] != '>') return "seq";
    fastac::TerminatorProbe probe;
    for (size_t at = 0; at < text.size(); at += 7)                  // (the probe sees the file in pieces too)
        if (probe.feed(text.data() + at, std::min<size_t>(7, text.size() - at))) break;
    carry.crlf = probe.crlf;
    if (!chunk) chunk = text.size();
    for (uint64_t at = 0; at < text.size(); at += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, text.size() - at);
        uint8_t* piece = (uint8_t*)malloc(n);
        memcpy(piece, text.data() + at, n);
        const fastac::ChunkResult r = fastac::chunk_result_serial(piece, n, carry.crlf);
        carry.consume(piece, r);
        free(piece);
    }
    carry.finish();
    if (carry.seq_before_header) return "seq";
    if (carry.n_bare) return "bare " + std::to_string(carry.n_bare) + " " + std::to_string(carry.first_bare_line);
    return "ok " + hex(carry.fai_text());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string mode = argv[1];
    std::string row;
    if (mode == "fai") {
        unsigned long long number = 0;
        while (std::getline(std::cin, row)) {
            const std::vector<uint8_t> text = unhex(row);
            for (uint64_t chunk : {16ull, 32ull, 48ull, 4096ull, 0ull})
                printf("%llu %llu %s\n", number, (unsigned long long)chunk, index_text(text, chunk).c_str());
            ++number;
        }
        return 0;
    }
    if (mode == "reg2bin") {
        long long beg, end;
        while (std::cin >> beg >> end) printf("%u\n", sampc::reg2bin((int32_t)beg, (int32_t)end));
        return 0;
    }
    if (mode == "records") {
        while (std::getline(std::cin, row)) {
            const std::vector<uint8_t> bytes = unhex(row);
            if (bytes.size() < 36) { printf("bad\n"); continue; }
            uint8_t* rec = (uint8_t*)malloc(bytes.size());
            memcpy(rec, bytes.data(), bytes.size());
            uint32_t want = 0;
            const uint32_t bs = binc::load32(rec);
            if (bs >= 32 && 4ull + bs <= bytes.size() && binc::expected_bin(rec, bs, &want)) printf("ok %u %u\n", want, binc::stored_bin(rec));
            else printf("bad\n");
            free(rec);
        }
        return 0;
    }
    return 2;
}
