// tests/harness/bamwalk_del_check.cpp — TEST INFRASTRUCTURE: the product's wave-parallel BAM record walk
// (pandepth_amd/csrc/pd_bamwalk.h, the source the gfx950 kernels compile) in its `-del` instance (DEL = true, Cfg::count_del = 1:
// one run per group of M/=/X/D operations that no N splits) with its 64 lanes emulated on the host.  Both passes run over every
// file; pass 2 must write exactly the places pass 1 counted.  The runs go to <file>.<tag>.runs (int32 triples tid, beg, end: the
// first runs in file order, then the others), for tests/test_bamwalk_del.py to compare with tests/del_model.py.
// Modelled on bamwalk_check.cpp (same reading of the file, same segments, same chain rounds).  What differs: the walk's instance
// (<HostWave, true>, count_del = 1), contig_on (contigs of >= 2 bases, as the program sets it), no comparison with the host reader
// (the model is in Python), the sentinel check of pass 2 against pass 1's counts, and the runs written out instead of compared here.
//   bamwalk_del_check [-x flagmask] [-q mapq] [-seg KiB] [-near span] -tag name file.bam ...
// -near (any value but 4294967295) makes every lane walk its CIGARs itself, as in bamwalk_check: no CIGAR is left to the wave.
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
    uint8_t buf[1 << 16]; int n;
    while ((n = gzread(g, buf, sizeof buf)) > 0) out.insert(out.end(), buf, buf + n);
    gzclose(g);
    return true;
}

int main(int argc, char **argv)
{
    uint32_t mask = 1796, near_span = 0xFFFFFFFFu; int mapq = 0; int seg_kb = 64; std::string tag = "del";
    int bad_files = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "-x")) { mask = (uint32_t)atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-q")) { mapq = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-seg")) { seg_kb = atoi(argv[++a]); continue; }
        if (!strcmp(argv[a], "-near")) { near_span = (uint32_t)strtoul(argv[++a], nullptr, 10); continue; }
        if (!strcmp(argv[a], "-tag")) { tag = argv[++a]; continue; }
        const char *path = argv[a];
        std::vector<uint8_t> d;
        if (!gunzip_all(path, d) || d.size() < 12) { fprintf(stderr, "cannot read %s\n", path); return 2; }
        size_t o = 4; uint32_t l_text = rd32(d.data() + o); o += 4 + l_text;
        const uint32_t n_ref = rd32(d.data() + o); o += 4;
        std::vector<uint32_t> lens(n_ref); std::vector<uint8_t> on(n_ref, 1);
        for (uint32_t i = 0; i < n_ref; ++i) { const uint32_t ln = rd32(d.data() + o); o += 4 + ln; lens[i] = rd32(d.data() + o); o += 4; on[i] = lens[i] >= 2; }
        d.resize(d.size() + 64, 0);
        Cfg c; c.buf = d.data(); c.avail = d.size() - 64; c.n_ref = (int32_t)n_ref; c.contig_len = lens.data(); c.contig_on = on.data();
        c.flag_mask = mask; c.min_mapq = mapq; c.span_off = nullptr; c.spans = nullptr; c.near_span = near_span; c.count_del = 1;
        std::vector<Seg> segs;
        const uint64_t SB = (uint64_t)seg_kb * 1024;
        for (uint64_t b = o; b < c.avail; b += SB) {
            Seg s; memset(&s, 0, sizeof s);
            s.begin = b; s.end = std::min<uint64_t>(b + SB, c.avail); s.hint = b == o ? o : NONE; s.unit_first = b == o; s.avail = c.avail;
            segs.push_back(s);
        }
        if (segs.empty()) { printf("%s: no records\n", path); continue; }
        std::vector<LaneOut> lanes(segs.size() * 64);
        for (size_t j = 0; j < segs.size(); ++j) walk_segment<pdw::HostWave, true>(c, segs[j], &lanes[j * 64]);
        int rounds = 0;
        std::vector<uint32_t> redo;
        while (check_chain(segs, &redo) > 0 && rounds < 24) {
            ++rounds;
            for (uint32_t j : redo) walk_segment<pdw::HostWave, true>(c, segs[j], &lanes[(size_t)j * 64]);
        }
        uint64_t tf = 0, to = 0, tfar = 0, n_rec = 0; uint32_t fl = 0;
        for (auto &s : segs) { s.base_first = tf; s.base_other = to; s.base_far = tfar; tf += s.n_first; to += s.n_other; tfar += s.n_far; fl |= s.flags; n_rec += s.n_rec; }
        // pass 2 into arrays of sentinels with 64 spare places each: every counted place written, no other one touched
        const pd_iv none{-2, -2, -2};
        std::vector<pd_iv> first(tf + 64, none), other(to + 64, none), far(tfar + 64, none);
        for (size_t j = 0; j < segs.size(); ++j)
            if (segs[j].n_first | segs[j].n_other | segs[j].n_far) emit_segment<pdw::HostWave, true>(c, segs[j], &lanes[j * 64], first.data(), other.data(), far.data());
        bool agree = true;
        const auto check = [&](const std::vector<pd_iv> &v, uint64_t n) {
            for (uint64_t i = 0; i < v.size(); ++i) if ((v[i].tid == -2) != (i >= n)) agree = false;
        };
        check(first, tf); check(other, to); check(far, tfar);
        const std::string out = std::string(path) + "." + tag + ".runs";
        FILE *f = fopen(out.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 2; }
        fwrite(first.data(), sizeof(pd_iv), tf, f); fwrite(other.data(), sizeof(pd_iv), to, f); fwrite(far.data(), sizeof(pd_iv), tfar, f);
        fclose(f);
        printf("%s: %llu records, %zu segments, first runs %llu, other runs %llu, far runs %llu, flags %u, passes %s\n", path, (unsigned long long)n_rec,
               segs.size(), (unsigned long long)tf, (unsigned long long)to, (unsigned long long)tfar, fl, agree ? "agree" : "DISAGREE");
        if (!agree || fl) ++bad_files;
    }
    return bad_files ? 1 : 0;
}
