// namesort.hip -- K14: the sort keys of `sambamba sort -n / -N / -M` (sambamba/sort.d:221-298; the orders: namesort_core.hpp).
//
//   K14a k_name_key_measure  one lane per kept record of a batch, after K9a has compacted the batch and its bytes are in the record
//                            store: the name is checked (its frame against the record's length, every byte in 0x01..0x7F) and
//                            measured -- the number of 64-bit words of its key.  With -M the HI tag is looked up among the aux
//                            fields (find_hi refuses a tag that runs past the record) and the -M word written.  Bad names and
//                            bad HI tags are counted, once per wave.
//        k_name_key_emit     after an exclusive scan of the word counts (launch_count_scan): the same walker writes the key words
//                            into the key store, 8-byte aligned, the last word zero-padded.  Then the wave folds, per word index
//                            one of its records has, an OR and an AND (a record that has ended contributes 0) -- one wave
//                            reduction and one pair of atomics per wave and word index -- so the host knows before any sorting
//                            which words vary at all.
//   K14b k_name_word_gather  key[i] = word r of the key of record perm[i], 0 when the key is shorter: the input of K9b for one
//                            word of the LSD sort over words.
//
// Per record (name of l bytes, key of w words): measure reads 12 bytes of per-record arrays, the 36 fixed bytes and l name bytes of
// the record (-M: also its aux fields) and writes 4 (-M: 12); emit reads 12 + 8, the l name bytes again and its own 8 w, and writes
// 8 w + 8; a gather reads 4 (perm) + 16 (two offsets) + 8 (the word, when the key has it) and writes 8.
#include "common.hpp"
#include "namesort.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// ---- K14a ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNameKeyThreads) void k_name_key_measure(NameKeyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kNameKeyThreads + threadIdx.x;
    const bool live = i < a.n;
    bool bad_name = false, bad_hi = false;
    uint32_t nw = 0;
    uint64_t mw = 0;
    if (live) {
        const uint64_t j = a.first + i;
        const uint8_t* rec = a.store + a.off[j];
        const uint64_t len = a.len[j];
        nsc::NameFrame f;
        if (!nsc::name_frame(rec, len, &f) || !nsc::name_ok(rec + 36, f.name_len)) bad_name = true;
        else {
            nw = nsc::key_words(rec + 36, f.name_len, a.order);
            if (a.match_mates) {
                int32_t hi = 0;
                bad_hi = !f.aux_ok || !nsc::find_hi(rec, f.aux, len, &hi);
                mw = nsc::mate_word(hi, f.flag);
            }
        }
        a.words[i] = nw;
        if (a.match_mates) a.mate_word[j] = mw;
    }
    const unsigned long long m_live = __ballot(live), m_name = __ballot(bad_name), m_hi = __ballot(bad_hi);
    const uint32_t w_min = wave_min<uint32_t>(live ? nw : 0xFFFFFFFFu), w_max = wave_max<uint32_t>(nw);
    unsigned long long m_or = 0, m_and = ~0ull;
    if (a.match_mates) { m_or = wave_or(live ? mw : 0ull); m_and = wave_and(live ? mw : ~0ull); }      // (a.match_mates is uniform)
    if ((threadIdx.x & 63u) == 0 && m_live) {
        if (m_name) atomicAdd(a.acc + kNameAccBadName, (unsigned long long)__popcll(m_name));
        if (m_hi) atomicAdd(a.acc + kNameAccBadHi, (unsigned long long)__popcll(m_hi));
        atomicMin(a.acc + kNameAccMinWords, (unsigned long long)w_min);
        atomicMax(a.acc + kNameAccMaxWords, (unsigned long long)w_max);
        if (a.match_mates) {
            atomicOr(a.acc + kNameAccMateOr, m_or);
            atomicAnd(a.acc + kNameAccMateAnd, m_and);
        }
    }
}

__global__ __launch_bounds__(kNameKeyThreads) void k_name_key_emit(NameKeyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kNameKeyThreads + threadIdx.x;
    const bool live = i < a.n;
    uint32_t nw = 0;
    uint64_t dst = 0;
    if (live) {
        const uint64_t j = a.first + i;
        nw = a.words[i];
        dst = a.key_base + a.word_base[i];
        a.key_off[j] = dst;
        if (i + 1 == a.n) a.key_off[j + 1] = a.key_base + a.word_base[a.n];
        if (nw) {
            // (measure admitted the record: its name lies inside it and has nw key words -- the writer stops there whatever it reads)
            const uint8_t* rec = a.store + a.off[j];
            uint32_t got;
            nsc::key_emit(rec + 36, (uint32_t)rec[12] - 1u, a.order, a.key_store + dst, nw, &got);
        }
    }
    uint32_t w_max = wave_max<uint32_t>(nw);
    if (w_max > nsc::kMaxKeyWords) w_max = nsc::kMaxKeyWords;
    for (uint32_t w = 0; w < w_max; ++w) {               // (wave-uniform)
        const unsigned long long v = w < nw ? a.key_store[dst + w] : 0ull;
        const unsigned long long k_or = wave_or(v), k_and = wave_and(live ? v : ~0ull);
        if ((threadIdx.x & 63u) == 0) {
            atomicOr(a.acc + kNameAccOr + w, k_or);
            atomicAnd(a.acc + kNameAccAnd + w, k_and);
        }
    }
}

// ---- K14b ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_name_word_gather(const uint64_t* __restrict__ key_store, const uint64_t* __restrict__ key_off,
                                                          const uint32_t* __restrict__ perm, uint64_t n, uint32_t r, uint64_t* __restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = perm[i];
    const uint64_t o = key_off[p], e = key_off[p + 1];
    key[i] = o + r < e ? key_store[o + r] : 0ull;
}

__global__ __launch_bounds__(256) void k_name_mate_gather(const uint64_t* __restrict__ word, const uint32_t* __restrict__ perm, uint64_t n,
                                                          uint64_t* __restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = word[perm[i]];
}

}  // namespace

void launch_name_key_measure(const NameKeyArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_name_key_measure, dim3(name_key_groups(a.n)), dim3(kNameKeyThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_name_key_emit(const NameKeyArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_name_key_emit, dim3(name_key_groups(a.n)), dim3(kNameKeyThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_name_word_gather(const uint64_t* d_key_store, const uint64_t* d_key_off, const uint32_t* d_perm, uint64_t n, uint32_t r,
                             uint64_t* d_key, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_name_word_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_key_store, d_key_off, d_perm, n, r, d_key);
    SBX_HIP(hipGetLastError());
}

void launch_name_mate_gather(const uint64_t* d_word, const uint32_t* d_perm, uint64_t n, uint64_t* d_key, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_name_mate_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_word, d_perm, n, d_key);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
