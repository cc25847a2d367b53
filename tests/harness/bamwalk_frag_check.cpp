// tests/harness/bamwalk_frag_check.cpp — TEST INFRASTRUCTURE: the product's wave-parallel BAM record walk
// (pandepth_amd/csrc/pd_bamwalk.h, the source the gfx950 kernels compile) in its `-frag` instances (FRAG = true, Cfg::fragments = 1:
// a properly paired read with tlen > 0 is the one run [pos, pos + tlen), its mate none) with its 64 lanes emulated on the host.  Both
// passes run over every file; pass 2 must write exactly the places pass 1 counted.  The runs go to <file>.<tag>.runs (int32 triples
// tid, beg, end: the first runs in file order, then the others), for tests/test_bamwalk_frag.py to compare with tests/frag_model.py.
// Modelled on bamwalk_del_check.cpp (same reading of the file, same segments, same chain rounds, same sentinel check).  What differs:
// the instance is chosen on the command line — -frag 1 takes FRAG = true, -del 1 takes DEL = true, and without either the DEFAULT
// instance walks the same bytes (Cfg filled as callers from before the mode fill it: fragments and frag_max keep their defaults).
//   bamwalk_frag_check [-x flagmask] [-q mapq] [-seg KiB] [-near span] [-frag 0|1] [-fragmax N] [-del 0|1] -tag name file.bam ...
// A stand-alone program: tests/test_bamwalk_frag.py builds it with -fsanitize=address,undefined and runs it as its own process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pandepth_amd/csrc/pd_bamwalk.h"

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

struct Out { uint64_t n_rec = 0, tf = 0, to = 0, tfar = 0; uint32_t flags = 0; bool agree = true; std::vector<pd_iv> first, other, far; };

template <bool DEL, bool FRAG>
static Out both_passes(const Cfg &c, std::vector<Seg> segs)
{
    Out r;
    std::vector<LaneOut> lanes(segs.size() * 64);
    for (size_t j = 0; j < segs.size(); ++j) walk_segment<pdw::HostWave, DEL, FRAG>(c, segs[j], &lanes[j * 64]);
    int rounds = 0;
    std::vector<uint32_t> redo;
    while (check_chain(segs, &redo) > 0 && rounds < 24) {
        ++rounds;
        for (uint32_t j : redo) walk_segment<pdw::HostWave, DEL, FRAG>(c, segs[j], &lanes[(size_t)j * 64]);
    }
    for (auto &s : segs) { s.base_first = r.tf; s.base_other = r.to; s.base_far = r.tfar; r.tf += s.n_first; r.to += s.n_other; r.tfar += s.n_far; r.flags |= s.flags; r.n_rec += s.n_rec; }
    // pass 2 into arrays of sentinels with 64 spare places each: every counted place written, no other one touched
    const pd_iv none{-2, -2, -2};
    r.first.assign(r.tf + 64, none); r.other.assign(r.to + 64, none); r.far.assign(r.tfar + 64, none);
    for (size_t j = 0; j < segs.size(); ++j)
        if (segs[j].n_first | segs[j].n_other | segs[j].n_far) emit_segment<pdw::HostWave, DEL, FRAG>(c, segs[j], &lanes[j * 64], r.first.data(), r.other.data(), r.far.data());
    const auto check = [&](const std::vector<pd_iv> &v, uint64_t n) {
        for (uint64_t i = 0; i < v.size(); ++i) if ((v[i].tid == -2) != (i >= n)) r.agree = false;
    };
    check(r.first, r.tf); check(r.other, r.to); check(r.far, r.tfar);
    return r;
}

int main(int argc, char **argv)
{
    uint32_t mask = 1796, near_span = 0xFFFFFFFFu, frag_max = 0; int mapq = 0; int seg_kb = 64; std::string tag = "frag";
    bool frag = false, del = false;
    int bad_files = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "-x") && a + 1 < argc) { mask = (uint32_t)atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-q") && a + 1 < argc) { mapq = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-seg") && a + 1 < argc) { seg_kb = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-near") && a + 1 < argc) { near_span = (uint32_t)strtoul(argv[++a], nullptr, 10); continue; }
        if (!strcmp(argv[a], "-frag") && a + 1 < argc) { frag = atoi(argv[++a]) != 0; continue; }
        if (!strcmp(argv[a], "-fragmax") && a + 1 < argc) { frag_max = (uint32_t)strtoul(argv[++a], nullptr, 10); continue; }
        if (!strcmp(argv[a], "-del") && a + 1 < argc) { del = atoi(argv[++a]) != 0; continue; }
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
        c.flag_mask = mask; c.min_mapq = mapq; c.span_off = nullptr; c.spans = nullptr; c.near_span = near_span;
        if (del) c.count_del = 1;
        if (frag) { c.fragments = 1; if (frag_max) c.frag_max = frag_max; }          // (the default instance: both members as Cfg's defaults leave them)
        std::vector<Seg> segs;
        const uint64_t SB = (uint64_t)seg_kb * 1024;
        for (uint64_t b = o; b < c.avail; b += SB) {
            Seg s; memset(&s, 0, sizeof s);
            s.begin = b; s.end = std::min<uint64_t>(b + SB, c.avail); s.hint = b == o ? o : NONE; s.unit_first = b == o; s.avail = c.avail;
            segs.push_back(s);
        }
        if (segs.empty()) { printf("%s: no records\n", path); continue; }
        const Out r = frag ? (del ? both_passes<true, true>(c, segs) : both_passes<false, true>(c, segs))
                           : (del ? both_passes<true, false>(c, segs) : both_passes<false, false>(c, segs));
        const std::string out = std::string(path) + "." + tag + ".runs";
        FILE *f = fopen(out.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 2; }
        fwrite(r.first.data(), sizeof(pd_iv), r.tf, f); fwrite(r.other.data(), sizeof(pd_iv), r.to, f); fwrite(r.far.data(), sizeof(pd_iv), r.tfar, f);
        fclose(f);
        printf("%s: %llu records, %zu segments, first runs %llu, other runs %llu, far runs %llu, flags %u, passes %s\n", path, (unsigned long long)r.n_rec,
               segs.size(), (unsigned long long)r.tf, (unsigned long long)r.to, (unsigned long long)r.tfar, r.flags, r.agree ? "agree" : "DISAGREE");
        if (!r.agree || r.flags) ++bad_files;
    }
    return bad_files ? 1 : 0;
}
