// extras.cpp — the outputs the reference does not have: -dist, -levels, -quantile, -thresholds, -gcbias, -readstats, -rowreads and -alnstats.  Each is made after the main table is
// written and the per-site job started, so that their path and timing stay as they are; each is one entry of EXTRAS, which the
// finish step of every table family and the exit for a PAF without targets (pipeline.cpp) walk in order.
#include <string.h>
#include "run.h"

namespace pdh {

namespace {

const char DIST_HEADER[] = "#Chr\tDepth\tSites\tAtLeast\tAtLeast(%)\n";       // -dist's table

// the main table's identity columns under the main table's names (-quantile's, -rowreads')
std::string identity_header(const Run &r)
{
    std::string h = "#Chr";
    if (r.o.mode != 0) h += "\tStart\tEnd";
    if (!r.synthetic) h += r.o.mode == 3 ? "\tRegionID" : "\tGeneID";
    return h;
}

// -quantile's table: the identity columns, the row's cell count, one column per percentage
std::string quantile_header(const Run &r)
{
    std::string h = identity_header(r);
    h += "\tCells";
    for (uint32_t p : r.o.quantile) { h += "\tQ"; h += std::to_string(p); }
    h += '\n';
    return h;
}

// -thresholds' table: -quantile's identity columns and Cells, then one column per threshold
std::string thresholds_header(const Run &r)
{
    std::string h = "#Chr";
    if (r.o.mode != 0) h += "\tStart\tEnd";
    if (!r.synthetic) h += r.o.mode == 3 ? "\tRegionID" : "\tGeneID";
    h += "\tCells";
    for (uint32_t t : r.o.thresholds) { h += "\tGE"; h += std::to_string(t); }
    h += '\n';
    return h;
}

// The cells the tables count, shared by -dist and -levels: the tables' contigs in their order and, in the region modes, the
// sorted, merged union of the table's regions (1-based first, as pd_region has it; merged regions neither overlap nor touch).
void covered_cells(const Run &r, std::vector<int32_t> &tids, std::vector<pd_region> &regs)
{
    if (r.synthetic) {
        if (r.o.mode == 6) { for (size_t t = 0; t < r.hdr.lens.size(); ++t) if (r.rm.has((int32_t)t)) tids.push_back((int32_t)t); }
        else for (auto &kv : r.rm.bins) tids.push_back(kv.first);
        return;
    }
    for (auto &kv : r.rm.genes) {
        const int64_t len = (int64_t)r.hdr.lens[(size_t)kv.first];
        std::vector<std::pair<int64_t, int64_t>> sp;     // cells [b, e)
        for (auto &g : kv.second)
            for (auto &c : g.second.cds) {
                const int64_t b = std::max<int64_t>((int64_t)c.first - 1, 0), e = std::min<int64_t>(c.second, len);
                if (b < e) sp.emplace_back(b, e);
            }
        if (sp.empty()) continue;
        tids.push_back(kv.first);
        std::sort(sp.begin(), sp.end());
        int64_t cb = sp[0].first, ce = sp[0].second;
        for (size_t k = 1; k <= sp.size(); ++k) {
            if (k < sp.size() && sp[k].first <= ce) { ce = std::max(ce, sp[k].second); continue; }
            regs.push_back(pd_region{kv.first, (int32_t)(cb + 1), (int32_t)ce});
            if (k < sp.size()) { cb = sp[k].first; ce = sp[k].second; }
        }
    }
}

// -dist on engines without the histogram entry points: the cells are read back and binned on the host threads
bool host_histogram(Run &r, const std::vector<int32_t> &tids, const std::vector<pd_region> &regs, uint32_t nb, std::vector<uint64_t> *hist)
{
    struct Piece { int32_t tid; uint32_t beg; size_t n; };
    std::vector<Piece> pieces;
    constexpr size_t CH = (size_t)1 << 22;
    auto add = [&](int32_t t, uint64_t b, uint64_t e) { for (uint64_t p = b; p < e; p += CH) pieces.push_back(Piece{t, (uint32_t)p, (size_t)std::min<uint64_t>(CH, e - p)}); };
    if (r.synthetic) for (int32_t t : tids) add(t, 0, r.hdr.lens[(size_t)t]);
    else for (const pd_region &g : regs) add(g.tid, (uint64_t)g.first - 1, (uint64_t)g.second);
    const int nt = host_workers(r.o.threads);
    std::vector<std::vector<uint32_t>> d((size_t)nt);
    std::vector<std::vector<uint64_t>> h((size_t)nt, std::vector<uint64_t>(nb));
    std::mutex mu;
    bool ok = true;
    parallel_for(pieces.size(), nt, [&](size_t i, int k) {
        const Piece &pc = pieces[i];
        d[(size_t)k].resize(pc.n);
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!ok) return;
            if (!r.read_cells(pc.tid, pc.beg, pc.n, d[(size_t)k].data())) { ok = false; return; }
        }
        std::fill(h[(size_t)k].begin(), h[(size_t)k].end(), 0);
        for (uint32_t x : d[(size_t)k]) ++h[(size_t)k][x < nb - 1 ? x : nb - 1];
        std::lock_guard<std::mutex> lk(mu);
        uint64_t *row = &(*hist)[(size_t)pc.tid * nb];
        for (uint32_t b = 0; b < nb; ++b) row[b] += h[(size_t)k][b];
    });
    return ok;
}

// -dist N: the depth distribution of the cells the tables count — every cell of the tables' contigs in the whole-contig modes,
// the union of the regions in -g / -b — per contig and genome-wide (Chr "*"), in <prefix>.dist.stat.gz.
bool write_dist(Run &r)
{
    const pd_engine_api *api = r.api;
    Engine &eng = *r.eng;
    const uint32_t nb = (uint32_t)r.o.dist + 1;              // depths 0 .. N-1 exact, the last bin >= N
    std::vector<int32_t> tids;                               // the tables' contigs, in their order
    std::vector<pd_region> regs;                             // region modes: the sorted, merged union of the table's regions
    covered_cells(r, tids, regs);
    std::vector<uint64_t> hist(r.hdr.lens.size() * nb, 0);
    if (r.synthetic && !r.scanned && api->scan_depth_histogram) {
        if (!r.merge_contexts()) return false;
        if (!eng.ck(api->scan_depth_histogram(eng.ctx, nb, r.wrap_bits, hist.data()), "pd_scan_depth_histogram")) return false;
    } else if (api->depth_histogram) {
        if (!r.need_scan()) return false;
        if ((r.synthetic || !regs.empty()) && !eng.ck(api->depth_histogram(eng.ctx, r.synthetic ? nullptr : regs.data(), r.synthetic ? 0 : regs.size(), nb, hist.data()),
                                                      "pd_depth_histogram")) return false;
    } else {
        if (!r.need_scan()) return false;
        if (!host_histogram(r, tids, regs, nb, &hist)) return false;
    }
    std::string txt = DIST_HEADER;
    auto block = [&](const std::string &name, const uint64_t *h) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < nb; ++k) total += h[k];
        uint64_t at = total;
        for (uint32_t k = 0; k < nb; ++k) {
            if (!h[k]) continue;
            txt += name; txt += '\t';
            if (k == nb - 1) txt += ">=";
            txt += std::to_string(k); txt += '\t'; txt += std::to_string(h[k]); txt += '\t'; txt += std::to_string(at); txt += '\t';
            txt += fmt2(at * 100.0 / total); txt += '\n';
            at -= h[k];
        }
    };
    std::vector<uint64_t> all(nb, 0);
    for (int32_t t : tids) {
        const uint64_t *h = &hist[(size_t)t * nb];
        block(r.hdr.names[(size_t)t], h);
        for (uint32_t k = 0; k < nb; ++k) all[k] += h[k];
    }
    block("*", all.data());
    GzWriter D;
    const std::string path = r.prefix + ".dist.stat.gz";
    if (!D.open(path)) { eng.fail("cannot open " + path); return false; }
    D.write(txt);
    if (!D.close()) { eng.fail("cannot write " + path); return false; }
    r.tm.mark("depth distribution");
    return true;
}

// The runs of cells [p, p + n) of contig t, from the engine (pd_depth_levels: 8 bytes per run cross the link) or, without that
// member, from the cells read back.  `runs` holds at least n.
bool level_runs(Run &r, int32_t t, uint64_t p, size_t n, pd_level *runs, size_t *nr, std::vector<uint32_t> *cells)
{
    const std::vector<uint32_t> &edges = r.o.levels_edges;
    const bool exact = edges.empty();
    *nr = 0;
    if (r.api->depth_levels)
        return r.eng->ck(r.api->depth_levels(r.eng->ctx, t, (uint32_t)p, n, exact ? nullptr : edges.data(), (uint32_t)edges.size(), runs, n, nr), "pd_depth_levels");
    cells->resize(n);
    if (!r.read_cells(t, p, n, cells->data())) return false;
    uint32_t prev = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t v = exact ? (*cells)[i] : (uint32_t)(std::upper_bound(edges.begin(), edges.end(), (*cells)[i]) - edges.begin()) - 1u;
        if (i == 0 || v != prev) runs[(*nr)++] = pd_level{(uint32_t)(p + i), v};
        prev = v;
    }
    return true;
}

// -levels SPEC: the same cells as runs, in <prefix>.levels.bed.gz — "<contig>\t<start>\t<end>\t<value>\n", 0-based half-open,
// maximal stretches of equal depth ("exact": value = the depth) or of equal depth class (value "lo:hi", the last class "lo:inf";
// cells below the first edge are not written).  The host joins a chunk's first run to the run left open by the chunk before, and
// formats the rows on its threads.  A chunk is 2^24 cells (-X levels_chunk=N): 64 MiB of depth on the device, at most 128 MiB of
// runs on the host, 12 calls for a 200 Mb contig.  Quantised text is small and goes through the table writer's threaded gzip;
// exact text can be as long as the per-site file and is streamed through zlib as it is made, never held.
bool write_levels(Run &r)
{
    Engine &eng = *r.eng;
    std::vector<int32_t> tids;
    std::vector<pd_region> regs;
    covered_cells(r, tids, regs);
    if (!r.need_scan()) return false;
    const std::vector<uint32_t> &edges = r.o.levels_edges;
    const bool exact = edges.empty();
    std::vector<std::string> label(edges.size());
    for (size_t k = 0; k < edges.size(); ++k) label[k] = std::to_string(edges[k]) + ":" + (k + 1 < edges.size() ? std::to_string(edges[k + 1]) : std::string("inf"));
    const long long chunk_ll = tune_int("levels_chunk", (long long)1 << 24);
    const size_t CH = (size_t)std::min<long long>(std::max<long long>(chunk_ll, 1), (long long)1 << 27);
    GzWriter LV;
    if (!exact) LV.set_threads(r.o.threads);
    const std::string path = r.prefix + ".levels.bed.gz";
    if (!LV.open(path)) { eng.fail("cannot open " + path); return false; }
    struct Row { uint32_t start, end, value; };
    std::vector<Row> rows;
    std::unique_ptr<pd_level[]> runs;
    size_t runs_cap = 0;
    std::vector<uint32_t> cells;
    const int nt = host_workers(r.o.threads);
    std::vector<std::string> part((size_t)nt);
    auto flush_rows = [&](const std::string &name) {
        if (rows.empty()) return;
        const size_t n = rows.size(), k = n < 65536 ? 1 : (size_t)nt, per = (n + k - 1) / k;
        parallel_for(k, nt, [&](size_t j, int) {
            std::string *out = &part[j];
            out->clear();
            for (size_t i = std::min(n, j * per); i < std::min(n, (j + 1) * per); ++i) {
                *out += name; *out += '\t'; append_u64(out, rows[i].start); *out += '\t'; append_u64(out, rows[i].end); *out += '\t';
                if (exact) append_u64(out, rows[i].value); else *out += label[rows[i].value];
                *out += '\n';
            }
        });
        for (size_t j = 0; j < k; ++j) LV.write(part[j]);
        rows.clear();
    };
    size_t ri = 0;
    for (int32_t t : tids) {
        const std::string &name = r.hdr.names[(size_t)t];
        std::vector<std::pair<uint64_t, uint64_t>> spans;    // cells [b, e) of this contig, ascending, not touching
        if (r.synthetic) { if (r.hdr.lens[(size_t)t]) spans.emplace_back(0, r.hdr.lens[(size_t)t]); }
        else for (; ri < regs.size() && regs[ri].tid == t; ++ri) spans.emplace_back((uint64_t)regs[ri].first - 1, (uint64_t)regs[ri].second);
        for (auto &sp : spans) {
            bool open = false; uint32_t ostart = 0, ovalue = 0;                // the run left open by the cells so far
            auto close_run = [&](uint32_t end) { if (open && (exact || ovalue != 0xFFFFFFFFu)) rows.push_back(Row{ostart, end, ovalue}); };
            for (uint64_t p = sp.first; p < sp.second; p += CH) {
                const size_t n = (size_t)std::min<uint64_t>(CH, sp.second - p);
                if (runs_cap < n) { runs.reset(); runs.reset(new pd_level[n]); runs_cap = n; }
                size_t nr = 0;
                if (!level_runs(r, t, p, n, runs.get(), &nr, &cells)) { LV.abandon(); return false; }
                for (size_t j = 0; j < nr; ++j) {
                    if (open && runs[j].value == ovalue) continue;             // (a chunk's first run continuing the one before)
                    close_run(runs[j].start);
                    open = true; ostart = runs[j].start; ovalue = runs[j].value;
                }
                if (rows.size() >= ((size_t)1 << 20)) flush_rows(name);
            }
            close_run((uint32_t)sp.second);
        }
        flush_rows(name);
    }
    if (!LV.close()) { ::remove(path.c_str()); eng.fail("cannot write " + path); return false; }
    r.tm.mark("depth levels");
    return true;
}

// One row of -quantile's table, and the cells it is taken from: segs[roff[i] .. roff[i + 1]) for row i (1-based inclusive, not
// yet clipped), or — the window tables on an engine with pd_window_quantiles — window `qi` of pd_window_layout.
struct QRow { int32_t tid; int64_t start, end; const std::string *id; uint64_t cells, qi; };      // qi: the row's place in qv
struct QPlan {
    std::vector<QRow> rows;
    std::vector<pd_region> segs;
    std::vector<uint64_t> roff = std::vector<uint64_t>(1, 0);
    std::vector<uint64_t> woff;                  // modes 5/6: pd_window_layout
    void add_row(const QRow &q) { rows.push_back(q); }
    void close_row() { roff.push_back(segs.size()); }
};

// the main table's rows, in its order
void quantile_rows(const Run &r, bool by_window, QPlan *q)
{
    const Options &o = r.o;
    if (o.mode == 5 || o.mode == 6) {
        const uint32_t w = (uint32_t)o.win;
        q->woff.resize(r.hdr.lens.size() + 1);
        r.api->window_layout(r.eng->ctx, w, q->woff.data());
        if (o.mode == 6) {
            for (size_t t = 0; t < r.hdr.lens.size(); ++t) {
                if (!r.rm.has((int32_t)t)) continue;
                const int64_t len = r.hdr.lens[t];
                for (size_t k = 0, n = window_rows(len, w); k < n; ++k) {
                    const auto se = window_row(k, len, w);
                    q->add_row(QRow{(int32_t)t, se.first, se.second, nullptr, (uint64_t)(se.second - se.first + 1), q->woff[t] + k});
                }
            }
        } else {
            for (auto &kv : r.rm.bins)
                for (const Bin &b : kv.second)
                    q->add_row(QRow{kv.first, b.start, b.end, nullptr, (uint64_t)(b.end - b.start + 1), q->woff[(size_t)kv.first] + (uint64_t)(b.start - 1) / w});
        }
        if (by_window) return;
        for (size_t i = 0; i < q->rows.size(); ++i) {
            q->segs.push_back(pd_region{q->rows[i].tid, (int32_t)q->rows[i].start, (int32_t)q->rows[i].end});
            q->close_row();
            q->rows[i].qi = i;
        }
    } else if (o.mode == 0) {
        for (auto &kv : r.rm.bins) {
            const int64_t len = r.hdr.lens[(size_t)kv.first];
            q->add_row(QRow{kv.first, 1, len, nullptr, 0, q->rows.size()});
            q->segs.push_back(pd_region{kv.first, 1, (int32_t)len});
            q->close_row();
        }
    } else {
        for (auto &kv : r.rm.genes)
            for (const GeneEntry *g : genes_in_table_order(kv.second)) {
                q->add_row(QRow{kv.first, g->second.start, g->second.end, &g->first, 0, q->rows.size()});
                for (auto &cd : g->second.cds) q->segs.push_back(pd_region{kv.first, cd.first, cd.second});
                q->close_row();
            }
    }
}

// -quantile on engines without the entry points: a contig's cells are read back once, its rows selected on the threads
bool host_quantiles(Run &r, const QPlan &q, std::vector<uint64_t> *cells, std::vector<uint32_t> *qv)
{
    const std::vector<uint32_t> &pct = r.o.quantile;
    const uint32_t np = (uint32_t)pct.size();
    const size_t n_rows = q.rows.size();
    const int nt = host_workers(r.o.threads);
    std::vector<uint32_t> d;
    std::vector<std::vector<uint32_t>> sel((size_t)nt);
    for (size_t r0 = 0, r1; r0 < n_rows; r0 = r1) {
        const int32_t t = q.rows[r0].tid;
        for (r1 = r0; r1 < n_rows && q.rows[r1].tid == t;) ++r1;
        const uint64_t len = r.hdr.lens[(size_t)t];
        d.resize(len);
        if (!r.read_cells(t, 0, len, d.data())) return false;
        parallel_for(r1 - r0, nt, [&](size_t item, int k) {
            const size_t i = r0 + item;
            std::vector<uint32_t> &v = sel[(size_t)k];
            v.clear();
            for (uint64_t s = q.roff[i]; s < q.roff[i + 1]; ++s) {
                const int64_t b = std::max<int64_t>((int64_t)q.segs[s].first - 1, 0), e = std::min<int64_t>(q.segs[s].second, (int64_t)len);
                if (b < e) v.insert(v.end(), d.begin() + b, d.begin() + e);
            }
            (*cells)[i] = v.size();
            for (uint32_t j = 0; j < np && !v.empty(); ++j) {
                const uint64_t rank = std::max<uint64_t>(1, ((uint64_t)pct[j] * v.size() + 99) / 100);
                std::nth_element(v.begin(), v.begin() + (ptrdiff_t)(rank - 1), v.end());
                (*qv)[i * np + j] = v[rank - 1];
            }
        });
    }
    return true;
}

// -quantile SPEC: nearest-rank depth percentiles of the cells of every row of the main table, in the table's row order, in
// <prefix>.quantile.stat.gz.  A row's cells: the whole contig, the window, or — in -g / -b — the multiset union of the id's
// entries clipped to the contig (overlapping entries count twice, as in Length / TotalDepth).  Q<p> is the r-th smallest cell,
// r = max(1, ceil(p * Cells / 100)); a row without cells prints NA.  The rows are selected on the engine (pd_window_quantiles /
// pd_depth_quantiles: only the results come back) or, without those members, on the host threads.
bool write_quantile(Run &r)
{
    const pd_engine_api *api = r.api;
    Engine &eng = *r.eng;
    const Options &o = r.o;
    if (!r.need_scan()) return false;
    const std::vector<uint32_t> &pct = o.quantile;
    const uint32_t np = (uint32_t)pct.size();
    const bool dev = api->depth_quantiles && api->window_quantiles && !(tune("quantile_device") && tune("quantile_device")[0] == '0');
    if (dev && api->set_param)
        for (const char *k : {"quantile_wave_max", "quantile_split_cells"})
            if (const char *e = tune(k)) (void)api->set_param(eng.ctx, k, (uint64_t)strtoull(e, nullptr, 10));
    const bool by_window = dev && (o.mode == 5 || o.mode == 6);
    QPlan q;
    quantile_rows(r, by_window, &q);
    std::vector<uint32_t> qv;
    if (by_window) {
        qv.resize((size_t)std::max<uint64_t>(1, q.woff.back() * np));
        if (!eng.ck(api->window_quantiles(eng.ctx, (uint32_t)o.win, pct.data(), np, qv.data()), "pd_window_quantiles")) return false;
    } else {
        const size_t n_rows = q.rows.size();
        std::vector<uint64_t> cells(n_rows ? n_rows : 1);
        qv.assign(n_rows ? n_rows * np : 1, 0xFFFFFFFFu);
        if (dev) {
            if (!eng.ck(api->depth_quantiles(eng.ctx, q.segs.data(), q.segs.size(), q.roff.data(), n_rows, pct.data(), np, cells.data(), qv.data()), "pd_depth_quantiles")) return false;
        } else if (!host_quantiles(r, q, &cells, &qv)) return false;
        for (size_t i = 0; i < n_rows; ++i) q.rows[i].cells = cells[i];
    }
    GzWriter Q;
    Q.set_threads(o.threads);
    const std::string path = r.prefix + ".quantile.stat.gz";
    if (!Q.open(path)) { eng.fail("cannot open " + path); return false; }
    std::string out = quantile_header(r);
    for (const QRow &row : q.rows) {
        out += r.hdr.names[(size_t)row.tid];
        if (o.mode != 0) { out += '\t'; append_i64(&out, row.start); out += '\t'; append_i64(&out, row.end); }
        if (row.id) { out += '\t'; out += *row.id; }
        out += '\t'; append_u64(&out, row.cells);
        for (uint32_t j = 0; j < np; ++j) {
            out += '\t';
            if (row.cells) append_u64(&out, qv[row.qi * np + j]); else out += "NA";
        }
        out += '\n';
        if (out.size() > (1u << 22)) { Q.write(out); out.clear(); }
    }
    Q.write(out);
    if (!Q.close()) { ::remove(path.c_str()); eng.fail("cannot write " + path); return false; }
    r.tm.mark("depth quantiles");
    return true;
}

// -thresholds on engines without the entry points: a contig's cells are read back once, its rows counted on the threads
bool host_thresholds(Run &r, const QPlan &q, std::vector<uint64_t> *cells, std::vector<uint64_t> *cnt)
{
    const std::vector<uint32_t> &thr = r.o.thresholds;
    const uint32_t nt = (uint32_t)thr.size();
    const size_t n_rows = q.rows.size();
    const int nw = host_workers(r.o.threads);
    std::vector<uint32_t> d;
    for (size_t r0 = 0, r1; r0 < n_rows; r0 = r1) {
        const int32_t t = q.rows[r0].tid;
        for (r1 = r0; r1 < n_rows && q.rows[r1].tid == t;) ++r1;
        const uint64_t len = r.hdr.lens[(size_t)t];
        d.resize(len);
        if (!r.read_cells(t, 0, len, d.data())) return false;
        parallel_for(r1 - r0, nw, [&](size_t item, int) {
            const size_t i = r0 + item;
            uint64_t C = 0, *row = &(*cnt)[i * nt];
            for (uint64_t s = q.roff[i]; s < q.roff[i + 1]; ++s) {
                const int64_t b = std::max<int64_t>((int64_t)q.segs[s].first - 1, 0), e = std::min<int64_t>(q.segs[s].second, (int64_t)len);
                if (b >= e) continue;
                C += (uint64_t)(e - b);
                for (int64_t p = b; p < e; ++p)                          // class = the thresholds <= the cell; suffix sums below
                    if (const size_t k = (size_t)(std::upper_bound(thr.begin(), thr.end(), d[(size_t)p]) - thr.begin())) ++row[k - 1];
            }
            for (uint32_t j = nt; j-- > 1;) row[j - 1] += row[j];
            (*cells)[i] = C;
        });
    }
    return true;
}

// -thresholds SPEC: for every row of the main table, in the table's row order, the number of the row's cells whose value is at
// or above each depth of SPEC, in <prefix>.thresholds.stat.gz.  The rows and their cells are -quantile's (quantile_rows); a row
// without cells prints zeros.  Counted on the engine in one pass over the cells (pd_window_thresholds / pd_depth_thresholds:
// only the results come back) or, without those members, on the host threads.
bool write_thresholds(Run &r)
{
    const pd_engine_api *api = r.api;
    Engine &eng = *r.eng;
    const Options &o = r.o;
    if (!r.need_scan()) return false;
    const std::vector<uint32_t> &thr = o.thresholds;
    const uint32_t nt = (uint32_t)thr.size();
    const bool dev = api->depth_thresholds && api->window_thresholds && !(tune("thresholds_device") && tune("thresholds_device")[0] == '0');
    if (dev && api->set_param)
        if (const char *e = tune("threshold_wave_max")) (void)api->set_param(eng.ctx, "threshold_wave_max", (uint64_t)strtoull(e, nullptr, 10));
    const bool by_window = dev && (o.mode == 5 || o.mode == 6);
    QPlan q;
    quantile_rows(r, by_window, &q);
    std::vector<uint32_t> wcnt;                  // by_window: the windows' counts, at qi
    std::vector<uint64_t> cnt;                   // else the rows'
    if (by_window) {
        wcnt.resize((size_t)std::max<uint64_t>(1, q.woff.back() * nt));
        if (!eng.ck(api->window_thresholds(eng.ctx, (uint32_t)o.win, thr.data(), nt, wcnt.data()), "pd_window_thresholds")) return false;
    } else {
        const size_t n_rows = q.rows.size();
        std::vector<uint64_t> cells(n_rows ? n_rows : 1);
        cnt.assign(n_rows ? n_rows * nt : 1, 0);
        if (dev) {
            if (!eng.ck(api->depth_thresholds(eng.ctx, q.segs.data(), q.segs.size(), q.roff.data(), n_rows, thr.data(), nt, cells.data(), cnt.data()), "pd_depth_thresholds")) return false;
        } else if (!host_thresholds(r, q, &cells, &cnt)) return false;
        for (size_t i = 0; i < n_rows; ++i) q.rows[i].cells = cells[i];
    }
    GzWriter W;
    W.set_threads(o.threads);
    const std::string path = r.prefix + ".thresholds.stat.gz";
    if (!W.open(path)) { eng.fail("cannot open " + path); return false; }
    std::string out = thresholds_header(r);
    for (const QRow &row : q.rows) {
        out += r.hdr.names[(size_t)row.tid];
        if (o.mode != 0) { out += '\t'; append_i64(&out, row.start); out += '\t'; append_i64(&out, row.end); }
        if (row.id) { out += '\t'; out += *row.id; }
        out += '\t'; append_u64(&out, row.cells);
        for (uint32_t j = 0; j < nt; ++j) { out += '\t'; append_u64(&out, by_window ? wcnt[row.qi * nt + j] : cnt[row.qi * nt + j]); }
        out += '\n';
        if (out.size() > (1u << 22)) { W.write(out); out.clear(); }
    }
    W.write(out);
    if (!W.close()) { ::remove(path.c_str()); eng.fail("cannot write " + path); return false; }
    r.tm.mark("depth thresholds");
    return true;
}

constexpr uint32_t GC_BINS = 101;

// -gcbias' file from the 203 numbers: 101 rows, GC 0 .. 100, and the closing line
std::string gcbias_text(uint32_t W, const uint64_t *win, const uint64_t *sum, uint64_t skipped)
{
    auto f = [](const char *fmt, double v) { char b[64]; snprintf(b, sizeof b, fmt, v); return std::string(b); };
    uint64_t n = 0, total = 0;
    for (uint32_t b = 0; b < GC_BINS; ++b) { n += win[b]; total += sum[b]; }
    const double mean_all = n ? (double)total / (double)(n * W) : 0.0;
    std::string txt = "#GC\tWindows\tTotalDepth\tMeanDepth\tNormalized\n";
    for (uint32_t b = 0; b < GC_BINS; ++b) {
        txt += std::to_string(b); txt += '\t'; txt += std::to_string(win[b]); txt += '\t'; txt += std::to_string(sum[b]); txt += '\t';
        if (!win[b]) { txt += "NA\tNA\n"; continue; }
        const double mean = (double)sum[b] / (double)(win[b] * W);
        txt += f("%.2f", mean); txt += '\t';
        txt += total ? f("%.4f", mean / mean_all) : std::string("NA");
        txt += '\n';
    }
    txt += "##WindowSize: " + std::to_string(W) + "\tWindows: " + std::to_string(n) + "\tSkipped: " + std::to_string(skipped) + "\tMeanDepth: " + (n ? f("%.2f", mean_all) : std::string("NA")) + "\n";
    return txt;
}

std::string gcbias_empty(const Run &r)
{
    const uint64_t zero[GC_BINS] = {};
    return gcbias_text(r.o.gcbias, zero, zero, 0);
}

// -gcbias on engines without the entry point: the spans' cells are read back, a stretch of whole windows at a time, and binned here
bool host_gc_bias(Run &r, const std::vector<pd_region> &regs, const std::vector<const char *> &bases,
                  const std::vector<uint32_t> &n_bases, uint64_t *win, uint64_t *sum, uint64_t *skipped)
{
    const uint64_t W = r.o.gcbias, per = std::max<uint64_t>(1, ((uint64_t)1 << 22) / W);          // windows per read
    std::vector<uint32_t> d;
    auto span = [&](int32_t t, uint64_t b, uint64_t e) {
        const unsigned char *s = (const unsigned char *)bases[(size_t)t];
        const uint64_t have = s ? n_bases[(size_t)t] : 0;
        for (uint64_t left = (e - b) / W, p = b; left;) {
            const uint64_t take = std::min(left, per);
            d.resize((size_t)(take * W));
            if (!r.read_cells(t, p, take * W, d.data())) return false;
            for (uint64_t k = 0; k < take; ++k, p += W) {
                if (p + W > have) { ++*skipped; continue; }
                uint64_t g = 0, tot = 0; bool bad = false;
                for (uint64_t i = 0; i < W && !bad; ++i) {
                    const unsigned c = s[p + i] | 0x20u;
                    if (c == 'c' || c == 'g') ++g; else if (c != 'a' && c != 't') bad = true;
                    tot += d[(size_t)(k * W + i)];
                }
                if (bad) { ++*skipped; continue; }
                const uint64_t bin = (200 * g + W) / (2 * W);
                ++win[bin]; sum[bin] += tot;
            }
            left -= take;
        }
        return true;
    };
    for (const pd_region &g : regs) if (!span(g.tid, (uint64_t)g.first - 1, (uint64_t)g.second)) return false;
    return true;
}

// -gcbias W: depth by GC content, in <prefix>.gcbias.stat.gz.  The cells are -dist's (covered_cells); every contig — in -g / -b every
// merged region — is tiled from its first cell by windows of exactly W cells, a shorter rest belonging to none (simpler than Picard's
// window sliding by one base).  A contig's bases are those of the first FASTA record that carries its name (RefSeqs::named); a window
// with a cell that is not A / C / G / T in either case, or that the record does not reach, is skipped; any other goes to the bin of its GC
// percentage rounded half up.  Binned on the engine (pd_depth_gc_bias: the bases go up, 203 numbers come back) or, without that member,
// on the host from cells read back.  The arena has been kept for this and is given back here.
bool write_gcbias(Run &r)
{
    const pd_engine_api *api = r.api;
    Engine &eng = *r.eng;
    const uint32_t W = r.o.gcbias;
    std::vector<int32_t> tids;
    std::vector<pd_region> regs;
    covered_cells(r, tids, regs);
    if (!r.need_scan()) return false;
    const size_t nc = r.hdr.names.size();
    std::vector<const char *> bases(nc ? nc : 1, nullptr);
    std::vector<uint32_t> n_bases(nc ? nc : 1, 0);
    for (size_t t = 0; t < nc; ++t) {
        const char *p; size_t n;
        if (r.ref.named(r.hdr.names[t], &p, &n)) { bases[t] = p; n_bases[t] = (uint32_t)std::min<size_t>(n, 0xFFFFFFFFu); }
    }
    uint64_t win[GC_BINS] = {}, sum[GC_BINS] = {}, skipped = 0;
    const bool dev = api->depth_gc_bias && !(tune("gcbias_device") && tune("gcbias_device")[0] == '0');
    if (dev && api->set_param)
        for (const char *k : {"gcbias_piece_cells", "gcbias_wave_max"})
            if (const char *e = tune(k)) (void)api->set_param(eng.ctx, k, (uint64_t)strtoull(e, nullptr, 10));
    if (r.synthetic) {                                       // whole contigs, but only the table's: one region each
        regs.clear();
        for (int32_t t : tids) if (r.hdr.lens[(size_t)t]) regs.push_back(pd_region{t, 1, (int32_t)r.hdr.lens[(size_t)t]});
    }
    if (dev) {
        if (!regs.empty() && !eng.ck(api->depth_gc_bias(eng.ctx, regs.data(), regs.size(), W, bases.data(), n_bases.data(), win, sum, &skipped), "pd_depth_gc_bias")) return false;
    } else if (!host_gc_bias(r, regs, bases, n_bases, win, sum, &skipped)) return false;
    r.ref.clear();
    GzWriter G;
    const std::string path = r.prefix + ".gcbias.stat.gz";
    if (!G.open(path)) { eng.fail("cannot open " + path); return false; }
    G.write(gcbias_text(W, win, sum, skipped));
    if (!G.close()) { ::remove(path.c_str()); eng.fail("cannot write " + path); return false; }
    r.tm.mark("gc bias");
    return true;
}

// -readstats N: what the records were, in <prefix>.reads.stat.gz.  The numbers are the contexts' accumulators (Engine::rs, fed by the
// device's k_record_stats or by the host readers as every input was read), not the engine's depth: nothing is asked of the engine here.
std::string readstats_empty(const Run &r)
{
    RecStats z;
    z.init(r.o.flag_mask, r.o.min_mapq, r.o.readstats, (int32_t)r.hdr.names.size());
    return z.text(r.hdr.names, r.hdr.lens);
}

bool write_readstats(Run &r)
{
    RecStats all;
    all.init(r.o.flag_mask, r.o.min_mapq, r.o.readstats, (int32_t)r.hdr.names.size());
    for (auto &e : r.engs) all.merge(e->rs);
    GzWriter G;
    const std::string path = r.prefix + ".reads.stat.gz";
    if (!G.open(path)) { r.eng->fail("cannot open " + path); return false; }
    G.write(all.text(r.hdr.names, r.hdr.lens));
    if (!G.close()) { ::remove(path.c_str()); r.eng->fail("cannot write " + path); return false; }
    r.tm.mark("read statistics");
    return true;
}

// -alnstats W: the CIGAR operations and read lengths of the records, in <prefix>.aln.stat.gz.  As -readstats: the numbers are the contexts'
// accumulators (Engine::as, fed by the device's k_aln_stats or by the host readers as every input was read); nothing is asked of the engine here.
std::string alnstats_empty(const Run &r)
{
    AlnStats z;
    z.init(r.o.flag_mask, r.o.min_mapq, r.o.alnstats, (int32_t)r.hdr.names.size());
    return z.text();
}

bool write_alnstats(Run &r)
{
    AlnStats all;
    all.init(r.o.flag_mask, r.o.min_mapq, r.o.alnstats, (int32_t)r.hdr.names.size());
    for (auto &e : r.engs) all.merge(e->as);
    GzWriter G;
    const std::string path = r.prefix + ".aln.stat.gz";
    if (!G.open(path)) { r.eng->fail("cannot open " + path); return false; }
    G.write(all.text());
    if (!G.close()) { ::remove(path.c_str()); r.eng->fail("cannot write " + path); return false; }
    r.tm.mark("alignment statistics");
    return true;
}

// -rowreads: the records that START in every row of the main table, in <prefix>.rowreads.stat.gz — -quantile's rows and identity columns,
// then Records Passed MapQ0 Kept Forward MeanMapQ (rowcounts.h).  The numbers are the contexts' accumulators over the run's bins
// (Engine::rc, fed by the device's k_row_counts or by the host readers as every input was read): nothing is asked of the engine here.
// A window row or a contig row is one bin; a -g / -b row is the sum over its entries (the multiset: overlapping entries of one id count
// twice, as in Length / TotalDepth) of P[bin of `second`] - P[bin of `first - 1`], P = the prefix sums over the contig's bins.
std::string rowreads_header(const Run &r) { return identity_header(r) + "\tRecords\tPassed\tMapQ0\tKept\tForward\tMeanMapQ\n"; }

bool write_rowreads(Run &r)
{
    const Options &o = r.o;
    const RowBins &B = r.row_bins;
    const int W = RowCounts::WORDS;
    // the contexts' bins summed into the first one's (no further copy: with a small -w on a large genome the array is hundreds of MB)
    RowCounts &all = r.eng->rc;
    for (auto &e : r.engs) if (e.get() != r.eng) { all.merge(e->rc); e->rc.cnt.assign(e->rc.cnt.size(), 0); }
    QPlan q;
    quantile_rows(r, o.mode == 5 || o.mode == 6, &q);
    GzWriter G;
    G.set_threads(o.threads);
    const std::string path = r.prefix + ".rowreads.stat.gz";
    if (!G.open(path)) { r.eng->fail("cannot open " + path); return false; }
    std::string out = rowreads_header(r);
    std::vector<uint64_t> P;                                     // the prefix sums of one contig's bins (-g / -b)
    int32_t p_tid = -1;
    for (size_t i = 0; i < q.rows.size(); ++i) {
        const QRow &row = q.rows[i];
        uint64_t k[RowCounts::WORDS] = {0, 0, 0, 0, 0, 0};
        if (r.synthetic) {
            const uint64_t bin = B.w ? row.qi : (uint64_t)row.tid;
            for (int j = 0; j < W; ++j) k[j] = all.cnt[bin * W + (size_t)j];
        } else {
            const size_t t = (size_t)row.tid;
            const uint64_t first_bin = B.off[t] + t, n_b = B.off[t + 1] - B.off[t] + 1;
            if (row.tid != p_tid) {
                p_tid = row.tid;
                P.assign((size_t)(n_b + 1) * W, 0);
                for (uint64_t b = 0; b < n_b; ++b) for (int j = 0; j < W; ++j) P[(b + 1) * W + (size_t)j] = P[b * W + (size_t)j] + all.cnt[(first_bin + b) * W + (size_t)j];
            }
            const int64_t len = (int64_t)B.lens[t];
            for (uint64_t s = q.roff[i]; s < q.roff[i + 1]; ++s) {
                const int64_t b0 = std::max<int64_t>((int64_t)q.segs[s].first - 1, 0), e0 = std::min<int64_t>(q.segs[s].second, len);
                if (b0 >= e0) continue;
                const uint64_t jb = B.bin_of(row.tid, (uint32_t)b0) - first_bin, je = B.bin_of(row.tid, (uint32_t)e0) - first_bin;
                // (b0 and e0 are edges: bin jb begins at b0, bin je at e0, and P[j] is the sum of the bins before j)
                for (int j = 0; j < W; ++j) k[j] += P[je * W + (size_t)j] - P[jb * W + (size_t)j];
            }
        }
        out += r.hdr.names[(size_t)row.tid];
        if (o.mode != 0) { out += '\t'; append_i64(&out, row.start); out += '\t'; append_i64(&out, row.end); }
        if (row.id) { out += '\t'; out += *row.id; }
        for (int j = 0; j < RowCounts::MAPQ_SUM; ++j) { out += '\t'; append_u64(&out, k[j]); }
        out += '\t';
        if (k[RowCounts::KEPT]) { char t[64]; snprintf(t, sizeof t, "%.2f", (double)k[RowCounts::MAPQ_SUM] / (double)k[RowCounts::KEPT]); out += t; } else out += "NA";
        out += '\n';
        if (out.size() > (1u << 22)) { G.write(out); out.clear(); }
    }
    G.write(out);
    if (!G.close()) { ::remove(path.c_str()); r.eng->fail("cannot write " + path); return false; }
    r.tm.mark("row read counts");
    return true;
}

} // namespace

// -rowreads: the run's bin table, from the rows the main table will have — the window form with -w, one bin per contig for whole
// contigs, and with -g / -b every entry's `first - 1` and `second` clipped to its contig as edges, sorted and unique per contig
void rowreads_bins(const Run &r, RowBins *b)
{
    const Options &o = r.o;
    const size_t n = r.hdr.lens.size();
    b->lens = r.hdr.lens;
    b->off.assign(n + 1, 0);
    b->edges.clear();
    b->w = 0;
    if (o.mode == 5 || o.mode == 6) {
        b->w = (uint32_t)o.win;
        r.api->window_layout(r.eng->ctx, b->w, b->off.data());
        b->n_bins = b->off[n];
        return;
    }
    if (!r.synthetic) {
        std::vector<std::vector<uint32_t>> ed(n);
        for (auto &kv : r.rm.genes) {
            const int64_t len = (int64_t)r.hdr.lens[(size_t)kv.first];
            for (auto &g : kv.second)
                for (auto &c : g.second.cds) {
                    const int64_t b0 = std::max<int64_t>((int64_t)c.first - 1, 0), e0 = std::min<int64_t>(c.second, len);
                    if (b0 < e0) { ed[(size_t)kv.first].push_back((uint32_t)b0); ed[(size_t)kv.first].push_back((uint32_t)e0); }
                }
        }
        for (size_t t = 0; t < n; ++t) {
            std::sort(ed[t].begin(), ed[t].end());
            ed[t].erase(std::unique(ed[t].begin(), ed[t].end()), ed[t].end());
            b->edges.insert(b->edges.end(), ed[t].begin(), ed[t].end());
            b->off[t + 1] = b->edges.size();
        }
    }
    b->n_bins = b->off[n] + n;
}

const Extra EXTRAS[] = {
    {".dist.stat.gz", [](const Options &o) { return o.dist != 0; }, [](const Run &) { return std::string(DIST_HEADER); }, write_dist},
    {".levels.bed.gz", [](const Options &o) { return o.levels; }, [](const Run &) { return std::string(); }, write_levels},
    {".quantile.stat.gz", [](const Options &o) { return !o.quantile.empty(); }, quantile_header, write_quantile},
    {".thresholds.stat.gz", [](const Options &o) { return !o.thresholds.empty(); }, thresholds_header, write_thresholds},
    {".gcbias.stat.gz", [](const Options &o) { return o.gcbias != 0; }, gcbias_empty, write_gcbias},
    {".reads.stat.gz", [](const Options &o) { return o.readstats != 0; }, readstats_empty, write_readstats},
    {".rowreads.stat.gz", [](const Options &o) { return o.rowreads; }, rowreads_header, write_rowreads},
    {".aln.stat.gz", [](const Options &o) { return o.alnstats != 0; }, alnstats_empty, write_alnstats},
};
const size_t N_EXTRAS = sizeof(EXTRAS) / sizeof(EXTRAS[0]);

} // namespace pdh
