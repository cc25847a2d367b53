// run.h — internal to pipeline.cpp and extras.cpp: the state that the statistics, the tables and the extra outputs of ONE
// `pandepth` invocation share (what pandepth_main's lambdas used to capture), and the few helpers both files spell the same way.
#ifndef PD_RUN_H_
#define PD_RUN_H_
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "bam.h"
#include "engine_api.h"
#include "fasta.h"
#include "options.h"
#include "alnstats.h"
#include "recstats.h"
#include "regions.h"
#include "report.h"
#include "rowcounts.h"

namespace pdh {

// PANDEPTH_TIMING=1: phase wall times on stderr (diagnostics only)
struct PhaseTimer {
    bool on = getenv("PANDEPTH_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[timing] %-28s %8.3f s   (total %.3f s)\n", what,
                std::chrono::duration<double>(now - last).count(), std::chrono::duration<double>(now - t0).count());
        last = now;
    }
};

struct Engine {
    const pd_engine_api *api = nullptr;
    pd_ctx *ctx = nullptr;
    std::mutex err_mu;
    std::string err;
    RecStats rs; std::mutex rs_mu;              // -readstats: the records of this context's inputs (threaded readers merge theirs under rs_mu)
    AlnStats as; std::mutex as_mu;              // -alnstats: the CIGAR operations and read lengths of this context's inputs (likewise)
    RowCounts rc; std::mutex rc_mu;             // -rowreads: the same per bin of the run's table (Run::row_bins)
    std::atomic<bool> cancel{false};            // the run is being abandoned: a writer working behind the statistics stops where it is
    void fail(const std::string &m) { std::lock_guard<std::mutex> lk(err_mu); if (err.empty()) err = m; }
    bool ok() { std::lock_guard<std::mutex> lk(err_mu); return err.empty(); }
    std::string message() { std::lock_guard<std::mutex> lk(err_mu); return err; }
    bool ck(int rc, const char *what)
    {
        if (rc == 0) return true;
        const char *m = api->strerror(ctx);
        fail(std::string(what) + ": " + (m ? m : "engine error"));
        return false;
    }
};

struct Comms;                                    // pipeline.cpp: the contexts' communicators

struct Run {
    PhaseTimer tm;                               // (starts at process entry)
    const pd_engine_api *api;
    const int device;
    Options o;
    bool list_mode = false, paf = false;
    int n_dev = 1, n_ctx = 1;                    // one context per GPU for a `#.list` input (round robin over the files)
    AlnHeader hdr;
    RefSeqs ref;                                 // -c -r: the GC(%) column (PD:3506-3538); host-side text work
    RegionModel rm;
    bool gc = false, synthetic = false;          // GC column wanted and loaded; whole-contig bins (modes 0/5/6)
    RowBins row_bins;                            // -rowreads: the elementary intervals of the table's rows (rowreads_bins, before the first input is read)
    std::string prefix, header_line;             // output names' stem (PD:4057-4090); the main table's first line
    GzWriter OUT;                                // the main table
    std::vector<std::unique_ptr<Engine>> engs;
    Engine *eng = nullptr;                       // engs[0]: the context the statistics are taken from
    Comms *comm = nullptr;
    bool wrap18 = false;                         // the reference's cell type: SiteInfo (18 bits) or uint32
    unsigned wrap_bits = 0;
    uint32_t min_dep = 1;
    // Several GPUs hold one partial sample each.  Wide-window statistics are summed in slices over the communicator
    // (pd_sliced_window_sum: every GPU receives 1/n of the others' 4-bit images, no GPU ever holds everybody's arrays); whatever
    // needs the summed cells themselves (per-site output, annotation intervals, narrow windows) adds the contexts into the first one.
    bool merged = false, scanned = false;
    // The per-site file is written behind the statistics and the tables: both read the same depth cells, the engine serialises
    // its entry points, and the file's gzip stream keeps the host threads busy only part of the time.
    struct SiteJob { std::thread th; bool ok = true; void wait() { if (th.joinable()) th.join(); } } site;

    Run(const pd_engine_api *a, int dev) : api(a), device(dev) {}
    ~Run();                                      // the per-site job is waited for, the table forgets the engine, the contexts go
    bool merge_contexts();
    bool need_scan();
    void abandon_site_file();                    // a failed run does not wait for the whole per-site file: the writer is told to stop, and what it wrote is removed
    bool site_done();
    int bail();                                  // the run failed: no per-site file, no table, the engine's message, exit code 2
    bool read_cells(int32_t tid, uint64_t beg, uint64_t n, uint32_t *out);    // depth cells [beg, beg + n) of a contig, read back in 2^22-cell calls
};

// `fn(item, worker)` for every item of [0, n), handed out one at a time to at most `workers` threads, the caller's among them
// (worker 0); worker < max(1, min(workers, n)).
inline int host_workers(int threads) { return std::max(1, std::min(threads, 16)); }
template <class F>
void parallel_for(size_t n, int workers, F fn)
{
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, workers), n));
    std::atomic<size_t> next{0};
    auto work = [&](int k) { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i, k); };
    std::vector<std::thread> th;
    for (int k = 1; k < nt; ++k) th.emplace_back(work, k);
    work(0);
    for (auto &t : th) t.join();
}

// The rows of a contig in the -w < 150 table (PD:4352-4394): `for (j = 1; j < len; j += w)` drops a final 1-base window.
inline size_t window_rows(int64_t len, uint32_t w) { return len > 1 ? (size_t)((len - 1 + (int64_t)w - 1) / (int64_t)w) : 0; }
inline std::pair<int64_t, int64_t> window_row(size_t k, int64_t len, uint32_t w)       // (start, end), 1-based inclusive
{
    const int64_t j = 1 + (int64_t)k * w;
    return {j, std::min<int64_t>(j - 1 + w, len)};
}

// A contig's genes in the order of the table's rows: by start; equal starts keep the id order of the map (PD:5032-5041)
typedef std::pair<const std::string, Gene> GeneEntry;
inline std::vector<const GeneEntry *> genes_in_table_order(const std::map<std::string, Gene> &genes)
{
    std::vector<const GeneEntry *> order;
    order.reserve(genes.size());
    for (auto &g : genes) order.push_back(&g);
    std::stable_sort(order.begin(), order.end(), [](const GeneEntry *a, const GeneEntry *b) { return a->second.start < b->second.start; });
    return order;
}

// extras.cpp — the outputs the reference does not have (-dist, -levels, -quantile, -thresholds, -gcbias, -readstats, -rowreads, -alnstats), one entry each
struct Extra {
    const char *suffix;                          // <prefix><suffix>
    bool (*enabled)(const Options &o);
    std::string (*empty_text)(const Run &r);     // what the file holds when there are no targets at all
    bool (*write)(Run &r);                       // false: the engine holds the message
};
void rowreads_bins(const Run &r, RowBins *b);    // -rowreads: the bin table of this run's rows (needs the first context: pd_window_layout)
extern const Extra EXTRAS[];
extern const size_t N_EXTRAS;

} // namespace pdh
#endif
