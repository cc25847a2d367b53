// tests/harness/rowcounts_check.cpp — TEST INFRASTRUCTURE: the product's row counting pass (pandepth_amd/csrc/pd_rowcounts.h, the source
// k_row_counts compiles) with its 64 lanes emulated on the host.  Over every file: the existing pass 1 (walk_segment, default instance) and
// chain check, then rows_segment over the confirmed lanes.  The bins go to <file>.<tag>.rc (uint64: PD_ROWCOUNT_WORDS per bin) for
// tests/test_rowreads_walk.py to compare with tests/rowreads_model.py; the line printed says how many records the walk counted.
//   rowcounts_check [-x flagmask] [-q mapq] [-seg KiB] [-w W | -edges table] -tag name file.bam ...
// `table`: uint64 edge_off[n_ref + 1], then uint32 edges[edge_off[n_ref]] (pd_decode_row_bins' arrays); neither -w nor -edges: no edges.
// A stand-alone program: the test builds it with -fsanitize=address,undefined and runs it as its own process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pandepth_amd/csrc/pd_rowcounts.h"

using namespace pdb2;

static bool gunzip_all(const char *path, std::vector<uint8_t> &out)
{
    gzFile g = gzopen(path, "rb");
    if (!g) return false;
    std::vector<uint8_t> buf(1 << 16); int n;
    while ((n = gzread(g, buf.data(), (unsigned)buf.size())) > 0) out.insert(out.end(), buf.begin(), buf.begin() + n);
    gzclose(g);
    return true;
}

int main(int argc, char **argv)
{
    uint32_t mask = 1796, w = 0; int mapq = 0; int seg_kb = 64; std::string tag = "rc", edge_path;
    int bad_files = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "-x") && a + 1 < argc) { mask = (uint32_t)atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-q") && a + 1 < argc) { mapq = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-seg") && a + 1 < argc) { seg_kb = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-w") && a + 1 < argc) { w = (uint32_t)strtoul(argv[++a], nullptr, 10); continue; }
        if (!strcmp(argv[a], "-edges") && a + 1 < argc) { edge_path = argv[++a]; continue; }
        if (!strcmp(argv[a], "-tag") && a + 1 < argc) { tag = argv[++a]; continue; }
        const char *path = argv[a];
        std::vector<uint8_t> d;
        if (!gunzip_all(path, d) || d.size() < 12) { fprintf(stderr, "cannot read %s\n", path); return 2; }
        size_t o = 4; uint32_t l_text = rd32(d.data() + o); o += 4 + l_text;
        const uint32_t n_ref = rd32(d.data() + o); o += 4;
        std::vector<uint32_t> lens(n_ref); std::vector<uint8_t> on(n_ref, 1);
        for (uint32_t i = 0; i < n_ref; ++i) { const uint32_t ln = rd32(d.data() + o); o += 4 + ln; lens[i] = rd32(d.data() + o); o += 4; on[i] = lens[i] >= 2; }
        const size_t n_bytes = d.size();
        d.resize(n_bytes + 64, 0);
        Cfg c; c.buf = d.data(); c.avail = n_bytes; c.n_ref = (int32_t)n_ref; c.contig_len = lens.data(); c.contig_on = on.data();
        c.flag_mask = mask; c.min_mapq = mapq; c.span_off = nullptr; c.spans = nullptr; c.near_span = 0xFFFFFFFFu;
        // the bin table, its arrays at their exact sizes
        std::vector<uint64_t> off((size_t)n_ref + 1, 0);
        std::vector<uint32_t> edges;
        uint64_t n_bins;
        if (w) {
            if (!edge_path.empty()) { fprintf(stderr, "-w and -edges exclude each other\n"); return 2; }
            uint64_t k = 0;
            for (uint32_t i = 0; i < n_ref; ++i) { off[i] = k; k += ((uint64_t)lens[i] + w - 1) / w; }
            off[n_ref] = n_bins = k;
        } else {
            if (!edge_path.empty()) {
                FILE *f = fopen(edge_path.c_str(), "rb");
                if (!f || fread(off.data(), 8, off.size(), f) != off.size()) { fprintf(stderr, "cannot read %s\n", edge_path.c_str()); return 2; }
                edges.resize((size_t)off[n_ref]);
                if (!edges.empty() && fread(edges.data(), 4, edges.size(), f) != edges.size()) { fprintf(stderr, "short table %s\n", edge_path.c_str()); return 2; }
                fclose(f);
            }
            n_bins = off[n_ref] + n_ref;
        }
        const pdrc::Bins B{w, off.data(), edges.data(), n_bins};
        std::vector<Seg> segs;
        const uint64_t SB = (uint64_t)seg_kb * 1024;
        for (uint64_t b = o; b < c.avail; b += SB) {
            Seg s; memset(&s, 0, sizeof s);
            s.begin = b; s.end = std::min<uint64_t>(b + SB, c.avail); s.hint = b == o ? o : NONE; s.unit_first = b == o; s.avail = c.avail;
            segs.push_back(s);
        }
        // exact size, so that the sanitizer sees a store behind the bins
        std::vector<unsigned long long> counts((size_t)n_bins * PD_ROWCOUNT_WORDS, 0);
        uint64_t n_rec = 0; uint32_t flags = 0;
        if (!segs.empty()) {
            std::vector<LaneOut> lanes(segs.size() * 64);
            for (size_t j = 0; j < segs.size(); ++j) walk_segment<pdw::HostWave>(c, segs[j], &lanes[j * 64]);
            int rounds = 0;
            std::vector<uint32_t> redo;
            while (check_chain(segs, &redo) > 0 && rounds < 24) {
                ++rounds;
                for (uint32_t j : redo) walk_segment<pdw::HostWave>(c, segs[j], &lanes[(size_t)j * 64]);
            }
            for (auto &s : segs) { flags |= s.flags; n_rec += s.n_rec; }
            for (size_t j = 0; j < segs.size(); ++j)
                if (segs[j].n_rec) pdrc::rows_segment<pdw::HostWave>(c, segs[j], &lanes[j * 64], B, counts.data());
        }
        unsigned long long started = 0;
        for (uint64_t b = 0; b < n_bins; ++b) started += counts[(size_t)b * PD_ROWCOUNT_WORDS];
        const std::string out = std::string(path) + "." + tag + ".rc";
        FILE *f = fopen(out.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 2; }
        fwrite(counts.data(), 8, counts.size(), f);
        fclose(f);
        printf("%s: %llu records walked, %llu started, %llu bins, %zu segments, %u contigs, flags %u\n", path, (unsigned long long)n_rec, started,
               (unsigned long long)n_bins, segs.size(), n_ref, flags);
        if (flags) ++bad_files;
    }
    return bad_files ? 1 : 0;
}
