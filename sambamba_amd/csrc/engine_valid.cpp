// engine_valid.cpp -- sbx_validate_bam / sbx_format_validate_report: which records of a BAM are valid (isValid, BioD
// bio/std/hts/bam/validation/alignment.d), and why not.  The body `sambamba validate` (sambamba/validate.d) does not have.
//
// One index-mode pass like sbx_flagstat's (for_each_record_batch: K1 + K2 per batch, no filter, nothing resident); per batch K19
// (valid.hip) adds the records of every class of error to eleven device counters and keeps the lowest ordinal of an invalid record.
// The counters are read back after every batch (twelve words): the first batch that reports an invalid record still holds it in U,
// so its bytes are fetched there -- as sbx_index_bam fetches the first record with a wrong bin -- and the mask the report carries
// is validc::record_mask of those bytes on the host, the same statements the device ran.
#include "engine_stream.hpp"
#include "valid.hpp"

namespace {

const char* const kClassNames[SBX_VALIDATE_CLASSES] = {"name-empty", "name-chars", "position", "qualities", "cigar-hard", "cigar-soft",
                                                       "cigar-length", "tag-value", "tag-duplicate", "malformed"};

}  // namespace

extern "C" {

int sbx_validate_bam(const char* in_path, int device, sbx_validate_report* report, sbx_validate_stats* stats, char* err, size_t errlen) {
    static_assert(SBX_VALIDATE_CLASSES == validc::kClasses, "the report has one count per class of valid_core.hpp");
    return run_entry(err, errlen, [&] {
        if (!in_path || !report) throw Error(SBX_EINVAL, "null argument");
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, false);      // no filter: every record is described
        hipStream_t s = c->stream.get();
        DevBuf<unsigned long long> d_acc(kValidAccWords);
        unsigned long long acc[kValidAccWords] = {0};
        acc[kValidAccFirst] = kValidNone;
        SBX_HIP(hipMemcpyAsync(d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));
        sbx_validate_report r{};
        sbx_validate_stats st{};
        EventTimer t_k;
        bool have_first = false;
        uint64_t n_records = 0;
        for_each_record_batch(c.get(), index_batch_bytes(), &st.n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const uint64_t u_end = next - base;
            t_k.start(s);
            launch_valid_masks(ValidArgs{c->U(), c->d_desc.p, nrec, u_end, n_records, nullptr, d_acc.p}, s);
            t_k.stop(s);
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            // (the next batch's K1 / K2 overwrite U and the descriptors: K19 ends first)
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index;
            if (nrec) st.ms_valid += t_k.ms();
            if (acc[kValidAccInvalid] && !have_first) {
                const uint64_t i = acc[kValidAccFirst] - n_records;
                if (i >= nrec) throw Error(SBX_EFORMAT, "internal error: the first invalid record is not in its batch");
                RecDesc d;
                SBX_HIP(hipMemcpy(&d, c->d_desc.p + i, sizeof d, hipMemcpyDeviceToHost));
                // 36 bytes and the name when the batch holds them; the whole record only to name its classes
                uint64_t len = d.rec_off < u_end ? std::min<uint64_t>(u_end - d.rec_off, 36) : 0;
                std::vector<uint8_t> rec((size_t)len);
                if (len) SBX_HIP(hipMemcpy(rec.data(), c->U() + d.rec_off, (size_t)len, hipMemcpyDeviceToHost));
                if (len == 36) {
                    const uint64_t bs = validc::rd32(rec.data());
                    if (bs >= 32 && bs <= 0x7FFFFFF0u && d.rec_off + 4 + bs <= u_end) {
                        len = 4 + bs;
                        rec.resize((size_t)len);
                        SBX_HIP(hipMemcpy(rec.data(), c->U() + d.rec_off, (size_t)len, hipMemcpyDeviceToHost));
                    }
                }
                r.first_ordinal = acc[kValidAccFirst];
                r.first_mask = validc::record_mask(rec.data(), len);
                if (!r.first_mask) throw Error(SBX_EFORMAT, "internal error: the first invalid record is valid on the host");
                if (len >= 36 && rec[12] && 36ull + rec[12] <= len) {      // the record holds the name it states
                    r.first_name_len = rec[12] - 1u;
                    memcpy(r.first_name, rec.data() + 36, r.first_name_len);
                }
                have_first = true;
            }
            n_records += nrec;
            return true;
        });
        r.n_records = n_records;
        r.n_invalid = acc[kValidAccInvalid];
        for (int k = 0; k < SBX_VALIDATE_CLASSES; ++k) r.class_count[k] = acc[k];
        st.inflated_bytes = c->blocks.out_off.back();
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] validate: n_records=%llu n_invalid=%llu inflated_bytes=%llu n_batches=%u ms_inflate=%.2f ms_index=%.2f "
                            "ms_valid=%.3f ms_total_wall=%.1f\n", (unsigned long long)r.n_records, (unsigned long long)r.n_invalid,
                    (unsigned long long)st.inflated_bytes, st.n_batches, st.ms_inflate, st.ms_index, st.ms_valid, st.ms_total_wall);
        *report = r;
        if (stats) *stats = st;
    });
}

int sbx_format_validate_report(const char* path, const sbx_validate_report* report, char* buf, size_t cap, size_t* len) {
    if (!path || !report || !len) return SBX_EINVAL;
    const sbx_validate_report& r = *report;
    std::string out = std::string("file\t") + path + "\n";
    out += "records\t" + std::to_string(r.n_records) + "\n";
    out += "invalid\t" + std::to_string(r.n_invalid) + "\n";
    for (int k = 0; k < SBX_VALIDATE_CLASSES; ++k) out += std::string(kClassNames[k]) + "\t" + std::to_string(r.class_count[k]) + "\n";
    if (r.n_invalid) {
        out += "first-invalid\t" + std::to_string(r.first_ordinal) + "\t";
        const uint32_t n = std::min<uint32_t>(r.first_name_len, 254u);
        for (uint32_t k = 0; k < n; ++k) {
            const unsigned ch = (uint8_t)r.first_name[k];
            if (ch < '!' || ch > '~' || ch == '\\') {
                char hex[8];
                snprintf(hex, sizeof hex, "\\x%02X", ch);
                out += hex;
            } else out += (char)ch;
        }
        out += "\t";
        bool any = false;
        for (int k = 0; k < SBX_VALIDATE_CLASSES; ++k)
            if (r.first_mask >> k & 1u) { out += (any ? "," : ""); out += kClassNames[k]; any = true; }
        out += "\n";
    }
    *len = out.size();
    if (!buf || cap < out.size() + 1) return SBX_ENOMEM;
    memcpy(buf, out.c_str(), out.size() + 1);
    return SBX_OK;
}

}  // extern "C"
