// cli_pipeline.hpp -- `depth base` on one device as a pipeline of slices.
// `depth base` without -L and with -c > 0: the text is a pure function of the position, so the genome is cut into
// slices that flow through three overlapping stages -- file -> device (sbx_prefetch_interval), the kernels
// (sbx_run_interval), device -> text (sbx_stream_base_rows) -- on two contexts that alternate.  PCIe is full duplex:
// the upload of slice k + 1 and the text of slice k - 1 travel while slice k is computed.
#pragma once
#include "cli_base.hpp"

namespace sbx {

struct BasePipeline {
    enum Outcome { Done, DoesNotFit, Failed };       // DoesNotFit: SBX_ENOMEM before any text was written -- the caller runs one pass
    sbx_ctx* ctx;                                    // the caller's context; the second one is opened (and closed) here
    BasePrinter& bp;
    const std::vector<const char*>& paths;
    const sbx_filter& filt;
    int mode_id;
    const Options& o;
    // Contexts: TWO in the detached child (SBX_DETACH=1: upload, kernels and text of three different slices overlap; the exit of two
    // contexts is the child's business), ONE in the default one-process form (round 5): two contexts cost more at exit than their
    // overlap saves (0.86 s against 0.75 s for config 2 in round 3), but slices through ONE context still pay: the upload of slice
    // k + 1 travels while the text of slice k leaves -- the two PCIe directions -- and the buffers hold a quarter of the job, so
    // the process has a quarter of the device memory to give back when it ends (config 2: 0.66 -> see profiles/round5).
    // The slices are cut by positions, not by the planner's byte budget: when one does not fit (SBX_ENOMEM before any text was
    // written) the run falls back to the one-pass form, which goes through sbx_plan_batches.
    size_t n_ctx;
    StageSync sync{"pipeline stage failed"};
    sbx_ctx* cx[2] = {nullptr, nullptr};
    std::vector<Slice> sl;
    double busy_up = 0, busy_run = 0, busy_print = 0, t_open2 = 0, t0 = 0;       // seconds every stage was working (SBX_TIMING)
    std::vector<double> done_at;

    Outcome run(int n_ref) {
        if (const char* e = getenv("SBX_PIPELINE_CONTEXTS")) n_ctx = atoi(e) == 2 ? 2 : 1;
        std::vector<Slice> contigs;
        for (int r = 0; r < n_ref; ++r) contigs.push_back({(uint32_t)r, 0, ref_len(ctx, r), 0, 0});
        // four slices of a chromosome-sized job: each slice still fills the device once (the lane-per-block Huffman kernel takes
        // one residency, ~16 ms, however few blocks it gets), and the text of the whole job -- what the pipeline is
        // bound by -- starts to flow after a quarter of the upload
        sl = cut_slices(ctx, contigs, std::max<uint64_t>(total_positions(ctx, n_ref) / 4, 16u << 20));
        cx[0] = ctx;
        std::vector<int> uploaded(sl.size(), 0), computed(sl.size(), 0), printed(sl.size(), 0);
        bool opened2 = false, all_printed = false;
        done_at.assign(sl.size(), 0);
        auto mark = [&](std::vector<int>& v, size_t k) { sync.mark([&] { v[k] = 1; }); };
        t0 = now();
        size_t n_printed = 0;
        {
            StageThreads stages(sync);
            stages.start([&] {       // the second context opens while the first slice is on its way
                const double to = now();
                sbx_ctx* c2 = nullptr;
                try { if (n_ctx == 2 && sl.size() > 1) c2 = open_configured(paths, -1, filt, mode_id, o, nullptr); }
                catch (const Fail& f) { sync.fail(f.msg); return; }
                t_open2 = now() - to;
                sync.mark([&] { cx[1] = c2; opened2 = true; });
            });
            stages.start([&] {       // uploader
                for (size_t k = 0; k < sl.size(); ++k) {
                    if (!sync.wait_for([&] { return k % n_ctx == 0 || opened2; })) return;
                    if (k >= n_ctx && !sync.wait_for([&] { return computed[k - n_ctx] != 0; })) return;       // the context's compressed bytes are free again
                    sbx_ctx* c = cx[k % n_ctx];
                    const double tu = now();
                    const int rc = sbx_prefetch_interval(c, sl[k].ref, (uint32_t)sl[k].beg, (uint32_t)sl[k].end);
                    if (rc != SBX_OK) { sync.fail(sbx_last_error(c), rc); return; }
                    busy_up += now() - tu;
                    mark(uploaded, k);
                }
            });
            stages.start([&] {       // computer
                for (size_t k = 0; k < sl.size(); ++k) {
                    // (the run of slice k replaces the counters of slice k - n_ctx in its context: that text must have left)
                    if (!sync.wait_for([&] { return uploaded[k] != 0 && (k < n_ctx || printed[k - n_ctx] != 0); })) return;
                    sbx_ctx* c = cx[k % n_ctx];
                    const double tr = now();
                    const int rc = sbx_run_interval(c, sl[k].ref, (uint32_t)sl[k].beg, (uint32_t)sl[k].end);
                    if (rc != SBX_OK) { sync.fail(sbx_last_error(c), rc); return; }
                    busy_run += now() - tr;
                    mark(computed, k);
                }
            });
            for (size_t k = 0; k < sl.size(); ++k) {       // the text leaves on this thread
                if (!sync.wait_for([&] { return computed[k] != 0; })) break;
                const double tp = now();
                try { bp.run_slice(cx[k % n_ctx], sl[k].ref, sl[k].beg, sl[k].print_end); }
                catch (const Fail& f) { sync.fail(f.msg); break; }
                busy_print += now() - tp;
                done_at[k] = now() - t0;
                mark(printed, k);
                ++n_printed;
            }
            std::lock_guard<std::mutex> g(sync.mu);
            all_printed = n_printed == sl.size() && sync.failure.empty();
            stages.regular = all_printed;       // (every stage is past its last wait: nothing to release)
        }
        if (all_printed) return Done;
        if (cx[1]) sbx_close(cx[1]);
        cx[1] = nullptr;
        // nothing was written yet: the one-pass form sizes its batches from the device's free memory
        return sync.failure_code == SBX_ENOMEM && n_printed == 0 ? DoesNotFit : Failed;
    }
    void report(double t_start, double t_open) const {
        fprintf(stderr, "[sbx-depth] open %.3f s, %zu slices through upload / kernels / text on %zu context(s) in %.3f s (stages busy: upload %.3f, "
                        "kernels %.3f, text %.3f; second context opened in %.3f s), total %.3f s since main\n",
                t_open - t_start, sl.size(), n_ctx, now() - t0, busy_up, busy_run, busy_print, t_open2, now() - t_start);
        std::string tl;
        for (double x : done_at) { char b[32]; snprintf(b, sizeof b, " %.3f", x); tl += b; }
        fprintf(stderr, "[sbx-depth] slices printed at%s s\n", tl.c_str());
    }
};

}  // namespace sbx
