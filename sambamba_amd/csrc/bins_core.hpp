// bins_core.hpp -- the bin a BAM record should carry: reg2bin(position, position + basesCovered()), what `sambamba index -c`
// (IndexBuilder.checkThatBinIsCorrect, BioD bio/std/hts/bam/bai/indexing.d:248-257) compares the stored bin with and `sambamba
// fixbins` (sambamba/fixbins.d) writes.  `__host__ __device__`: K16a / K16b (bins.hip) run it per record, the host runs it once more on
// the first record `index -c` complains about, and tests/native/fasta_host.cpp checks its arithmetic on the CPU.  The bin arithmetic
// itself is sampc::reg2bin (samparse_core.hpp), the one copy of bin.d:82-92 in the tree.
#pragma once
#include "samparse_core.hpp"

namespace sbx {
namespace binc {

SBX_FMT_HD uint32_t load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// rec: the record from its block_size field on, bs = that field; the caller has checked that 4 + bs bytes are readable and bs >= 32.
// false: the name and the CIGAR the record states run past its block_size (nothing behind the fixed part is read then).
// basesCovered (read.d:255-262): 0 for a read flagged unmapped, else the lengths of the M, D, N, = and X operations, added up in 32 bits.
SBX_FMT_HD bool expected_bin(const uint8_t* rec, uint32_t bs, uint32_t* bin) {
    const int32_t pos = (int32_t)load32(rec + 8);
    const uint32_t l_name = rec[12], fnc = load32(rec + 16);
    const uint32_t n_cigar = fnc & 0xFFFFu, flag = fnc >> 16;
    if (32ull + l_name + 4ull * n_cigar > bs) return false;
    uint32_t span = 0;
    if (!(flag & 0x4u)) {
        const uint8_t* cg = rec + 36 + l_name;
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t op = load32(cg + 4u * k), ty = op & 15u;
            if (ty == 0u || ty == 2u || ty == 3u || ty == 7u || ty == 8u) span += op >> 4;
        }
    }
    *bin = sampc::reg2bin(pos, (int32_t)((uint32_t)pos + span));
    return true;
}

SBX_FMT_HD uint32_t stored_bin(const uint8_t* rec) { return (uint32_t)rec[14] | (uint32_t)rec[15] << 8; }

}  // namespace binc
}  // namespace sbx
