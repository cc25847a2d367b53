// tests/harness/alnstats_check.cpp — TEST INFRASTRUCTURE: the product's CIGAR statistics pass (pandepth_amd/csrc/pd_alnstats.h, the source
// k_aln_stats compiles) with its 64 lanes emulated on the host.  Over every file: the existing pass 1 (walk_segment, default instance) and
// chain check, then stats_segment over the confirmed lanes — four segments to one zeroed copy of the LDS words, flushed behind them, as the
// kernel's workgroups do.  The array goes to <file>.<tag>.as (uint64: the PD_ALNSTAT_WORDS sums) for tests/test_alnstats_walk.py to compare
// with tests/alnstats_model.py; the line printed says how many records the walk counted.
//   alnstats_check [-x flagmask] [-q mapq] [-seg KiB] [-w width] -tag name file.bam ...
// A stand-alone program: the test builds it with -fsanitize=address,undefined and runs it as its own process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pandepth_amd/csrc/pd_alnstats.h"

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
    uint32_t mask = 1796, width = 1; int mapq = 0; int seg_kb = 64; std::string tag = "as";
    int bad_files = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "-x") && a + 1 < argc) { mask = (uint32_t)atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-q") && a + 1 < argc) { mapq = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-seg") && a + 1 < argc) { seg_kb = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-w") && a + 1 < argc) { width = (uint32_t)strtoul(argv[++a], nullptr, 10); continue; }
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
        std::vector<Seg> segs;
        const uint64_t SB = (uint64_t)seg_kb * 1024;
        for (uint64_t b = o; b < c.avail; b += SB) {
            Seg s; memset(&s, 0, sizeof s);
            s.begin = b; s.end = std::min<uint64_t>(b + SB, c.avail); s.hint = b == o ? o : NONE; s.unit_first = b == o; s.avail = c.avail;
            segs.push_back(s);
        }
        // exact size, so that the sanitizer sees a store behind the array
        std::vector<unsigned long long> sums((size_t)PD_ALNSTAT_WORDS, 0);
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
            for (size_t j0 = 0; j0 < segs.size(); j0 += 4) {
                std::vector<unsigned long long> hist((size_t)pdas::AS_LDS_WORDS, 0);
                for (size_t j = j0; j < std::min(j0 + 4, segs.size()); ++j)
                    if (segs[j].n_rec) pdas::stats_segment<pdw::HostWave>(c, segs[j], &lanes[j * 64], width, sums.data(), hist.data());
                pdas::flush_hist(hist.data(), sums.data(), 0, 1);
            }
        }
        const std::string out = std::string(path) + "." + tag + ".as";
        FILE *f = fopen(out.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 2; }
        fwrite(sums.data(), 8, sums.size(), f);
        fclose(f);
        printf("%s: %llu records walked, %llu counted, %zu segments, %u contigs, flags %u\n", path, (unsigned long long)n_rec, sums[0], segs.size(), n_ref, flags);
        if (flags) ++bad_files;
    }
    return bad_files ? 1 : 0;
}
