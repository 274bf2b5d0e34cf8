// namesort.hpp -- launchers of K14 (namesort.hip): the sort keys of `sambamba sort -n / -N / -M`.
#pragma once
#include "kernels.hpp"
#include "namesort_core.hpp"

namespace sbx {

// Words of the accumulators K14a adds to over the batches of a file.  The OR and the AND of word w of the keys are at
// kNameAccOr + w and kNameAccAnd + w; a wave adds to them only for the words one of its records has, so the AND of word w is
// meaningful only for w < the smallest key of the file (kNameAccMinWords) -- from there on some record has ended and counts as 0.
enum NameAcc : uint32_t {
    kNameAccBadName = 0, kNameAccBadHi = 1, kNameAccMinWords = 2, kNameAccMaxWords = 3, kNameAccMateOr = 4, kNameAccMateAnd = 5,
    kNameAccOr = 6, kNameAccAnd = kNameAccOr + nsc::kMaxKeyWords, kNameAccWords = kNameAccAnd + nsc::kMaxKeyWords
};
// the state of the accumulators before the first batch
inline void name_acc_init(unsigned long long* acc) {
    for (uint32_t k = 0; k < kNameAccWords; ++k) acc[k] = 0ull;
    acc[kNameAccMinWords] = ~0ull;
    acc[kNameAccMateAnd] = ~0ull;
    for (uint32_t w = 0; w < nsc::kMaxKeyWords; ++w) acc[kNameAccAnd + w] = ~0ull;
}

struct NameKeyArgs {
    const uint8_t* store;           // the resident record store
    const uint64_t* off;            // [first + ...) offset and length of the kept records (K9a wrote them)
    const uint32_t* len;
    uint64_t first, n;              // the batch's kept records are [first, first + n)
    uint32_t order;                 // nsc::kOrderLex / kOrderNatural
    uint32_t match_mates;
    uint32_t* words;                // [n] of the batch: key words of every record (measure writes, the scan reads)
    const uint64_t* word_base;      // [n + 1] of the batch: exclusive scan of words (emit)
    uint64_t key_base;              // key words of the batches before
    uint64_t* key_store;            // the keys, record behind record
    uint64_t* key_off;              // [first + ...], and [first + n] behind the last: where a record's key starts in key_store
    uint64_t* mate_word;            // [first + ...) with match_mates
    unsigned long long* acc;        // [kNameAccWords]
};
constexpr uint32_t kNameKeyThreads = 256;
inline uint32_t name_key_groups(uint64_t n) { return (uint32_t)((n + kNameKeyThreads - 1) / kNameKeyThreads); }
// K14a, first half: words[i] of every record of the batch (0 for a record whose name is refused), the bad names and bad HI tags
// counted, the -M words written and folded.
void launch_name_key_measure(const NameKeyArgs& a, hipStream_t stream);
// K14a, second half: the key words at key_store[key_base + word_base[i] ...), key_off, and the OR / AND of every word index.
void launch_name_key_emit(const NameKeyArgs& a, hipStream_t stream);

// K14b: d_key[i] = word r of the key of record d_perm[i], 0 when the key is shorter
void launch_name_word_gather(const uint64_t* d_key_store, const uint64_t* d_key_off, const uint32_t* d_perm, uint64_t n, uint32_t r,
                             uint64_t* d_key, hipStream_t stream);
// d_key[i] = d_word[d_perm[i]] (the -M word)
void launch_name_mate_gather(const uint64_t* d_word, const uint32_t* d_perm, uint64_t n, uint64_t* d_key, hipStream_t stream);

}  // namespace sbx
