// tests/harness/guess_chain_check.cpp — TEST INFRASTRUCTURE: units whose start is guessed (PD_UNIT_GUESS: no hint, any offset) through the
// product's walk with its 64 lanes emulated on the host (pandepth_amd/csrc/pd_bamwalk.h: walk_segment) and the host's chain check
// (pdb2::check_chain), the way dec_collect runs them.  Prints, per unit, the flags, the first record found and the records counted.
//   guess_chain_check file.bam (start stop avail)...      (offsets into the inflated file)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <vector>
#include "../../pandepth_amd/csrc/pd_bamwalk.h"
using namespace pdb2;
int main(int argc, char **argv)
{
    gzFile g = gzopen(argv[1], "rb"); std::vector<uint8_t> d; uint8_t buf[1 << 16]; int n;
    while ((n = gzread(g, buf, sizeof buf)) > 0) d.insert(d.end(), buf, buf + n);
    gzclose(g);
    size_t o = 4; uint32_t l_text = rd32(d.data() + o); o += 4 + l_text;
    const uint32_t n_ref = rd32(d.data() + o); o += 4;
    std::vector<uint32_t> lens(n_ref); std::vector<uint8_t> on(n_ref, 1);
    for (uint32_t i = 0; i < n_ref; ++i) { const uint32_t ln = rd32(d.data() + o); o += 4 + ln; lens[i] = rd32(d.data() + o); o += 4; on[i] = lens[i] >= 2; }
    d.resize(d.size() + 64, 0);
    for (int a = 2; a + 2 < argc; a += 3) {
        const uint64_t start = strtoull(argv[a], 0, 10), stop = strtoull(argv[a + 1], 0, 10), avail = strtoull(argv[a + 2], 0, 10);
        Cfg c{}; c.buf = d.data(); c.avail = avail; c.n_ref = (int32_t)n_ref; c.contig_len = lens.data(); c.contig_on = on.data();
        c.flag_mask = 1796; c.min_mapq = -1; c.near_span = 0xFFFFFFFFu;
        std::vector<Seg> segs;
        for (uint64_t b = start; b < stop; b += SEG_BYTES) { Seg s; memset(&s, 0, sizeof s); s.begin = b; s.end = std::min<uint64_t>(b + SEG_BYTES, stop); s.avail = avail; s.unit_first = b == start; s.hint = NONE; segs.push_back(s); }
        std::vector<LaneOut> lanes(segs.size() * 64);
        for (size_t j = 0; j < segs.size(); ++j) walk_segment<pdw::HostWave>(c, segs[j], &lanes[j * 64]);
        std::vector<uint32_t> redo; int rounds = 0;
        while (check_chain(segs, &redo) > 0 && rounds < 24) { ++rounds; for (uint32_t j : redo) walk_segment<pdw::HostWave>(c, segs[j], &lanes[(size_t)j * 64]); }
        uint32_t fl = 0; uint64_t fs = NONE, nrec = 0;
        for (auto &s : segs) { fl |= s.flags; if (fs == NONE && s.used_start != NONE) fs = s.used_start; nrec += s.n_rec; }
        printf("unit [%llu, %llu): %zu segments, %d rounds, flags %u, first_start %lld, records %llu\n", (unsigned long long)start, (unsigned long long)stop, segs.size(), rounds, fl, (long long)fs, (unsigned long long)nrec);
    }
    return 0;
}
