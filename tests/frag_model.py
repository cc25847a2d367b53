"""The model the `-frag` tests compare with, and the fragment corpus they run on.

Written from the rule of DESIGN.md §6b, independent of the product.  A KEPT read passes the flag mask, the mapq bound and the contig
test (a contig of at least 2 bases), as in tests/del_model.py.  A kept read is a FRAGMENT READ when
    flag & 0x3 == 0x3, flag & 0x908 == 0, next_refID == refID, tlen != 0 and |tlen| <= frag_max
(|tlen| as an unsigned 32-bit value: INT32_MIN is 2^31 and never passes).  With tlen > 0 it adds exactly one run
[pos, (int32)((uint32)pos + (uint32)tlen)), clamped to the contig, a run with end <= begin being empty; it is the read's first run
and its CIGAR plays no part.  With tlen < 0 it adds nothing and counts in neither n_first nor n_other.  Every other kept read is
walked as tests/del_model.py walks it (count_del chooses the rule).

The module also holds a record encoder that writes the three mate fields (bam_craft's writes -1, -1, 0), readers of SAM text and of
a BAM's inflated bytes that return them, and the fragment corpus.  A helper module, not a conftest."""
import os
import struct

import numpy as np

import bam_craft as B
import del_model as DM

M, I, D, N, S, H, P, EQ, X = range(9)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NO_BOUND = INT32_MAX


# ---------------------------------------------------------------------------------------------------------------------
# records: (tid, pos, flag, mapq, name, ops, l_seq, tags, mtid, mpos, tlen) — bam_craft's eight fields and the mate's three
# ---------------------------------------------------------------------------------------------------------------------
def encode_record(rec, cg_tag=True):
    """one record's bytes, block_size included: bam_craft's encoding with next_refID, next_pos and tlen written in"""
    b = bytearray(B.encode_record(tuple(rec[:8]), cg_tag))
    struct.pack_into("<iii", b, 24, rec[8], rec[9], rec[10])
    return bytes(b)


def mate_fields(inf, off):
    """(next_refID, next_pos, tlen) of the record at `off` of a BAM's inflated bytes"""
    return struct.unpack_from("<iii", inf, off + 24)


def name_of(inf, off):
    return bytes(inf[off + 36:off + 36 + inf[off + 12] - 1])


def records_of(inf, parsed):
    """bam_craft.parse_bam's records -> the model's tuples (tid, pos, flag, mapq, cigar — the CG tag's where it holds it —, mtid, tlen)"""
    out = []
    for r in parsed:
        mtid, _, tlen = mate_fields(inf, r["off"])
        out.append((r["tid"], r["pos"], r["flag"], r["mapq"], B.real_cigar(r), mtid, tlen))
    return out


def plain_records(recs):
    """the model's tuples -> tests/del_model.py's"""
    return [r[:5] for r in recs]


def read_sam(path):
    """-> names, lens, the model's tuples.  RNEXT: '=' is the read's own reference, '*' none, a name that reference."""
    names, lens, recs = [], [], []
    for line in open(path):
        if line.startswith("@"):
            if line.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in line.rstrip("\n").split("\t")[1:])
                names.append(f["SN"]); lens.append(int(f["LN"]))
            continue
        c = line.rstrip("\n").split("\t")
        if len(c) < 9:
            continue
        tid = names.index(c[2]) if c[2] != "*" else -1
        mtid = tid if c[6] == "=" else -1 if c[6] == "*" else names.index(c[6])
        recs.append((tid, int(c[3]) - 1, int(c[1]), int(c[4]), DM.parse_cigar(c[5]), mtid, int(c[8])))
    return names, lens, recs


def wrap32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def fragment_class(rec, frag_max=NO_BOUND):
    """0: not a fragment read, 1: it carries the fragment's run, 2: silent — of a record that is kept"""
    tid, pos, flag, mapq, cig, mtid, tlen = rec
    if flag & 0x3 != 0x3 or flag & 0x908 or mtid != tid or tlen == 0:
        return 0
    if abs(tlen) > frag_max:                                                 # (INT32_MIN: 2^31, above every bound)
        return 0
    return 1 if tlen > 0 else 2


def model(lens, recs, flag_mask=1796, min_mapq=-1, count_del=False, frag_max=NO_BOUND):
    """-> per-contig uint32 depth (None for contigs shorter than 2 bases), n_first, n_other"""
    diff = [np.zeros(l + 1, dtype=np.int64) if l >= 2 else None for l in lens]
    n_first = 0
    walked = []                                                              # the kept reads that are no fragment reads
    for rec in recs:
        tid, pos, flag, mapq, cig, mtid, tlen = rec
        if flag & flag_mask or mapq < min_mapq or not 0 <= tid < len(lens) or diff[tid] is None:
            continue
        k = fragment_class(rec, frag_max)
        if k == 0:
            walked.append(rec[:5])
        elif k == 1:
            L = lens[tid]
            b, e = min(max(pos, 0), L), min(max(wrap32(pos + tlen), 0), L)
            if e > b:
                diff[tid][b] += 1; diff[tid][e] -= 1
            n_first += 1
    dep, f2, n_other = DM.model(lens, walked, 0, -(1 << 30), count_del)      # (these were selected above: no filter here)
    out = []
    for d, w in zip(diff, dep):
        out.append(None if d is None else (np.cumsum(d[:-1]) + w.astype(np.int64)).astype(np.uint32))
    return out, n_first + f2, n_other


def depth_of_runs(lens, runs):
    """per-contig depth of (tid, beg, end) int32 triples as the engine takes them: both ends clamped to the contig, end <= begin empty"""
    out = []
    for t, L in enumerate(lens):
        r = runs[runs[:, 0] == t].astype(np.int64)
        b, e = np.clip(r[:, 1], 0, L), np.clip(r[:, 2], 0, L)
        keep = e > b
        diff = np.zeros(L + 1, dtype=np.int64)
        np.add.at(diff, b[keep], 1)
        np.add.at(diff, e[keep], -1)
        out.append(np.cumsum(diff[:-1]).astype(np.uint32) if L >= 2 else None)
    return out


def region_endpos(rec, frag_max=NO_BOUND):
    """the end the -g / -b region test takes for a kept read: the fragment's for the read that carries it (pos + 1 where it is empty)"""
    tid, pos, flag, mapq, cig, mtid, tlen = rec
    if fragment_class(rec, frag_max) == 1:
        e = wrap32(pos + tlen)
        return pos + 1 if e == pos else e
    adv = int(((cig >> 4)[np.isin(cig & 0xf, (M, D, N, EQ, X))]).sum(dtype=np.int64)) if not flag & 4 else 0
    return pos + (adv or 1)


# ---------------------------------------------------------------------------------------------------------------------
# the fragment corpus: one coordinate-sorted file, as BAM (bam_craft's BGZF writer) and as SAM text
# ---------------------------------------------------------------------------------------------------------------------
FRAG_NAMES, FRAG_LENS = ["fa", "fb", "fc"], [100000, 70000, 5000]
EDGE_DISTS = (1, 4, 35, 36)
FRAGMAX_CASE = 1000                      # the corpus holds pairs with |tlen| equal to this and one above: the tests' -fragmax
STEP = 20                                # cells between the left mates of the filler pairs
CASES = ["left_low_mapq", "right_low_mapq", "proper_without_paired", "mate_unmapped", "secondary_pair", "supplementary_pair", "mate_elsewhere",
         "tlen_zero", "tlen_inside_read", "ends_at_contig_end", "ends_one_past", "ends_far_past", "tlen_int32_max", "tlen_int32_max_wraps",
         "tlen_int32_min", "tlen_at_bound", "tlen_above_bound", "cells_511", "cells_512", "cells_513", "cells_65535", "cells_65537",
         "carry_96_ops", "silent_96_ops", "carry_cg_tag", "silent_cg_tag", "carry_no_cigar", "plain_deletion", "plain_skip"]


def _alternating(n):
    return [((M, 2), (I, 1), (M, 2), (D, 1))[k % 4] for k in range(n)]


def _read(tid, pos, flag, mapq, name, ops, mtid, tlen, tags=b"", l_seq=None):
    return (tid, pos, flag, mapq, name, B.pack(ops), B.qlen(ops) if l_seq is None else l_seq, tags, mtid, max(pos, 0), tlen)


def _cg_read(tid, pos, flag, mapq, name, ops, mtid, tlen):
    """a read whose CIGAR sits in the CG tag behind the <l_seq>S<ref>N placeholder (SAM §4.2.2), here with a CIGAR short enough to keep the file small"""
    real = B.pack(ops)
    l_seq = B.qlen(real)
    tags = b"CGBI" + struct.pack("<I", real.size) + real.astype("<u4").tobytes()
    return (tid, pos, flag, mapq, name, B.pack([(S, l_seq), (N, B.rlen(real))]), l_seq, tags, mtid, max(pos, 0), tlen)


def special_reads():
    """-> [record] of the named cases (the name says which), all behind cell 60 000 of fa or on fb / fc; pairs are flag 99 / 147"""
    L, R = 99, 147                                                             # 0x63: paired, proper, mate reverse, first; 0x93: ... reverse, second
    m100 = [(M, 100)]
    out = []

    def pair(name, tid, pos, tlen, lq=60, rq=60, lops=m100, rops=m100):
        out.append(_read(tid, pos, L, lq, name + b"/L", lops, tid, tlen))
        out.append(_read(tid, pos + tlen - B.rlen(rops), R, rq, name + b"/R", rops, tid, -tlen))

    pair(b"left_low_mapq", 0, 60000, 400, lq=5)
    pair(b"right_low_mapq", 0, 60100, 400, rq=5)
    out.append(_read(0, 61000, 0x2 | 0x20, 60, b"proper_without_paired", m100, 0, 300))
    out.append(_read(0, 61100, 0x3 | 0x8, 60, b"mate_unmapped", m100, 0, 300))
    out.append(_read(0, 61200, 0x103, 60, b"secondary_pair", m100, 0, 300))
    out.append(_read(0, 61300, 0x803, 60, b"supplementary_pair", m100, 0, 300))
    out.append(_read(0, 61400, L, 60, b"mate_elsewhere", m100, 1, 300))
    out.append(_read(0, 61500, L, 60, b"tlen_zero", m100, 0, 0))
    out.append(_read(0, 61600, L, 60, b"tlen_inside_read", m100, 0, 40))
    out.append(_read(0, 62000, L, 60, b"tlen_int32_min", m100, 0, INT32_MIN))
    pair(b"tlen_at_bound", 0, 63000, FRAGMAX_CASE, lops=[(M, 40), (D, 7), (M, 53)])
    pair(b"tlen_above_bound", 0, 65000, FRAGMAX_CASE + 1, rops=[(M, 30), (N, 50), (M, 70)])
    out.append(_read(0, 67000, L, 60, b"carry_96_ops", _alternating(96), 0, 500))
    out.append(_read(0, 67400, R, 60, b"silent_96_ops", _alternating(96), 0, -500))
    out.append(_cg_read(0, 68000, L, 60, b"carry_cg_tag", _alternating(130), 0, 450))
    out.append(_cg_read(0, 68300, R, 60, b"silent_cg_tag", _alternating(130), 0, -450))
    out.append(_read(0, 69000, 0x3 | 0x4 | 0x40, 60, b"carry_no_cigar", [], 0, 350, l_seq=30))          # (unmapped flag: kept under -x 0 only)
    out.append(_read(0, 70000, 0, 60, b"plain_deletion", [(M, 10), (D, 5), (M, 10)], -1, 0))
    out.append(_read(0, 70100, 16, 60, b"plain_skip", [(M, 10), (N, 5), (M, 10)], -1, 0))
    # run sizes on fb: either side of a 512-cell bucket and of the 16-bit halves of the compact planes
    for k, n in enumerate((511, 512, 513)):
        out.append(_read(1, 1024 + 2048 * k, L, 60, b"cells_%d" % n, m100, 1, n))
    out.append(_read(1, 100, L, 60, b"cells_65535", m100, 1, 65535))
    out.append(_read(1, 200, L, 60, b"cells_65537", m100, 1, 65537))
    # bounds and arithmetic on fc (5 000 cells)
    out.append(_read(2, 0, L, 60, b"tlen_int32_max", m100, 2, INT32_MAX))                               # covers the whole contig
    out.append(_read(2, 4000, L, 60, b"tlen_int32_max_wraps", m100, 2, INT32_MAX))                      # pos + tlen wraps below 0: an empty run
    out.append(_read(2, 4700, L, 60, b"ends_at_contig_end", m100, 2, 300))
    out.append(_read(2, 4701, L, 60, b"ends_one_past", m100, 2, 300))
    out.append(_read(2, 4702, L, 60, b"ends_far_past", m100, 2, 100000))
    return out


def _sized(fields, size):
    """a 50M filler read of exactly `size` bytes (block_size included): its name and a Z tag take up the slack, as in bam_craft._sized"""
    tid, pos, flag, mapq, name, mtid, tlen = fields
    pad = size - (4 + 32 + len(name) + 1 + 4 + 25 + 50)
    assert pad >= 0, (size, name)
    if 0 < pad < 4:
        name += b"n" * pad; pad = 0
    tags = B.tag_Z(b"XP", bytes(97 + (j * 7 + pos) % 26 for j in range(pad - 4))) if pad else b""
    rec = encode_record(_read(tid, pos, flag, mapq, name, [(M, 50)], mtid, tlen, tags))
    assert len(rec) == size
    return rec


def corpus_records(sub, seg):
    """-> [encoded record].  The first four segments are filler pairs on fa, both mates present (every filler is a fragment read), laid
    out byte by byte as bam_craft.layout_records lays out its file: with one unit over the whole file a fragment record starts 1, 4, 35
    and 36 bytes before the end of a lane's stretch and of a segment.  The special reads follow in coordinate order."""
    import heapq
    rng = np.random.default_rng(20241020)
    r0 = len(B.header_bytes(FRAG_NAMES, FRAG_LENS))
    recs, o = [], r0
    state = dict(cur=0, k=0)
    pending = []                                                               # right mates waiting for their place: (pos, k, fields)

    def next_fields():
        if pending and pending[0][0] <= state["cur"] + STEP:
            return heapq.heappop(pending)[2]
        state["cur"] += STEP; state["k"] += 1
        k, pos = state["k"], state["cur"]
        tlen = 120 + (k * 37) % 330
        name = b"p%04d" % k
        if k % 5:                                                              # (one filler in five is a left mate whose right mate is not in the file)
            heapq.heappush(pending, (pos + tlen - 50, k, (0, pos + tlen - 50, 147, (60, 30, 60, 10)[k % 4], name, 0, -tlen)))
        return (0, pos, 99, (60, 60, 10, 30)[k % 4], name, 0, tlen)

    def put(size):
        nonlocal o
        recs.append(_sized(next_fields(), size)); o += size

    def fill_to(target):
        while target - o > 1000:
            put(int(rng.integers(126, 480)))
        gap = target - o
        assert gap == 0 or gap >= 260, gap
        if gap:
            put(gap // 2)
            put(target - o)
        assert o == target

    for k, d in enumerate(EDGE_DISTS):
        fill_to(r0 + (3 + 2 * k) * sub - d)
        put(150)
    for k, d in enumerate(EDGE_DISTS):
        fill_to(r0 + (k + 1) * seg - d)
        put(150 + k)
    fill_to(r0 + 4 * seg + 3 * sub + 77)
    assert state["cur"] + 500 < 60000, state
    tail = [encode_record(_read(*f[:5], [(M, 50)], f[5], f[6])) for _, _, f in sorted(pending)]
    sp = sorted(special_reads(), key=lambda r: (r[0], r[1]))
    return recs + tail + [encode_record(r, cg_tag=False) for r in sp]


def crafted_stops(offs):
    """stops of a split whose units end 1, 4, 35 and 36 bytes behind the start of their last record, a filler (fragment) record each"""
    return [int(offs[300 * (k + 1)]) + d for k, d in enumerate(EDGE_DISTS)]


def fragment_corpus(d):
    """writes frag.bam and frag.sam into directory d -> a file dict like bam_craft.build_corpus's (path, blocks, inf, offs, lens, recs,
    data, cases) with sam (the text's path), names, and model_recs (the model's tuples, CG-tag CIGARs resolved)"""
    sub, seg, coop = B.walk_geometry()
    path = os.path.join(str(d), "frag.bam")
    blocks, inf, offs = B.write_bam(path, FRAG_NAMES, FRAG_LENS, corpus_records(sub, seg), member_size=20000)
    lens, parsed = B.parse_bam(inf)
    assert lens == FRAG_LENS and [r["off"] for r in parsed] == offs
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, names=FRAG_NAMES, recs=parsed, data=open(path, "rb").read(), cases={})
    f["model_recs"] = records_of(inf, parsed)
    for r in parsed:
        nm = name_of(inf, r["off"]).split(b"/")[0].decode()
        if nm in CASES:
            f["cases"].setdefault(nm, r["off"])
    f["sam"] = os.path.join(str(d), "frag.sam")
    with open(f["sam"], "w") as out:
        out.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(FRAG_NAMES, FRAG_LENS)))
        for r, m in zip(parsed, f["model_recs"]):
            mtid, mpos, tlen = mate_fields(inf, r["off"])
            cig = "".join("%d%s" % (c >> 4, "MIDNSHP=X"[c & 0xf]) for c in m[4].tolist()) or "*"
            rnext = "*" if mtid < 0 else "=" if mtid == r["tid"] else FRAG_NAMES[mtid]
            out.write("\t".join([name_of(inf, r["off"]).decode(), str(r["flag"]), FRAG_NAMES[r["tid"]], str(r["pos"] + 1), str(r["mapq"]), cig, rnext,
                                 str(mpos + 1), str(tlen), "*", "*"]) + "\n")
    check_corpus(f, sub, seg, coop)
    return f


def check_corpus(f, sub, seg, coop):
    """the corpus is not vacuous: every case class is there — told from the parsed bytes —, and fragments change the depth"""
    assert (sub, seg, coop) == (4096, 262144, 96), "the corpus was laid out for these; look at the cases again when they change"
    inf, offs, recs = f["inf"], f["offs"], f["model_recs"]
    assert set(CASES) <= set(f["cases"]), sorted(set(CASES) - set(f["cases"]))
    assert all(recs[k][:2] <= recs[k + 1][:2] for k in range(len(recs) - 1)), "not coordinate-sorted"
    assert 2000 <= len(recs) <= 9000 and max(FRAG_LENS) <= 100000
    by = {c: recs[offs.index(o)] for c, o in f["cases"].items()}
    raw = {c: f["recs"][offs.index(o)] for c, o in f["cases"].items()}
    cls = {c: fragment_class(r) for c, r in by.items()}
    for c in ("proper_without_paired", "mate_unmapped", "secondary_pair", "supplementary_pair", "mate_elsewhere", "tlen_zero", "tlen_int32_min",
              "plain_deletion", "plain_skip"):
        assert cls[c] == 0 and (by[c][6] != 0 or c in ("tlen_zero", "plain_deletion", "plain_skip")), c
    assert by["proper_without_paired"][2] & 3 == 2 and by["mate_unmapped"][2] & 0xb == 0xb and by["secondary_pair"][2] & 0x103 == 0x103
    assert by["supplementary_pair"][2] & 0x803 == 0x803 and by["mate_elsewhere"][5] not in (-1, by["mate_elsewhere"][0]) and by["tlen_int32_min"][6] == INT32_MIN
    for c in set(CASES) - {k for k, v in cls.items() if v == 0} - {"silent_96_ops", "silent_cg_tag"}:
        assert cls[c] == 1, c
    assert cls["silent_96_ops"] == 2 and cls["silent_cg_tag"] == 2
    names = [name_of(inf, o) for o in offs]
    both = lambda c: (recs[names.index(c + b"/L")], recs[names.index(c + b"/R")])
    assert both(b"left_low_mapq")[0][3] < 20 <= both(b"left_low_mapq")[1][3] and both(b"right_low_mapq")[1][3] < 20 <= both(b"right_low_mapq")[0][3]
    assert both(b"tlen_at_bound")[0][6] == FRAGMAX_CASE == -both(b"tlen_at_bound")[1][6] and both(b"tlen_above_bound")[0][6] == FRAGMAX_CASE + 1 == -both(b"tlen_above_bound")[1][6]
    ref_len = lambda r: int((r[4] >> 4)[np.isin(r[4] & 0xf, (M, D, N, EQ, X))].sum())
    assert 0 < by["tlen_inside_read"][6] < ref_len(by["tlen_inside_read"])
    L = lambda c: f["lens"][by[c][0]]
    assert by["ends_at_contig_end"][1] + by["ends_at_contig_end"][6] == L("ends_at_contig_end") and by["ends_one_past"][1] + by["ends_one_past"][6] == L("ends_one_past") + 1
    assert by["ends_far_past"][1] + by["ends_far_past"][6] > 10 * L("ends_far_past")
    assert by["tlen_int32_max"][6] == INT32_MAX == by["tlen_int32_max_wraps"][6] and wrap32(by["tlen_int32_max_wraps"][1] + INT32_MAX) < 0 < wrap32(by["tlen_int32_max"][1] + INT32_MAX)
    for n in (511, 512, 513, 65535, 65537):
        r = by["cells_%d" % n]
        assert r[6] == n and r[1] + n <= f["lens"][r[0]], n
    assert by["cells_512"][1] % 512 == 0
    assert raw["carry_96_ops"]["cigar"].size == coop == raw["silent_96_ops"]["cigar"].size
    for c in ("carry_cg_tag", "silent_cg_tag"):
        assert raw[c]["cigar"].size == 2 and by[c][4].size > coop and any(t[0] == b"CG" for t in raw[c]["tags"]), c
    assert by["carry_no_cigar"][4].size == 0 and by["carry_no_cigar"][2] & 1796 and by["carry_no_cigar"][3] >= 20
    # the layout: fragment records 1, 4, 35, 36 bytes before the end of a lane's stretch, of a segment (one unit) and of a unit (the crafted stops)
    total = len(inf)
    starts = np.asarray(offs, dtype=np.int64)
    frag_at = np.array([fragment_class(r) != 0 for r in recs])
    rel = starts - starts[0]
    for d in EDGE_DISTS:
        assert np.any(frag_at & ((rel + d) % sub == 0) & ((rel + d) % seg != 0)), ("lane", d)
        assert np.any(frag_at & ((rel + d) % seg == 0)), ("segment", d)
    one = B.census(offs, total, B.split_units(f["blocks"], offs, total, 1), sub, seg)
    assert set(EDGE_DISTS) <= one["lane_end"] and set(EDGE_DISTS) <= one["seg_end"], one
    cr = B.census(offs, total, B.units_from_stops(f["blocks"], offs, total, crafted_stops(offs)), sub, seg)
    assert set(EDGE_DISTS) <= cr["unit_end"], cr
    assert all(frag_at[300 * (k + 1)] for k in range(len(EDGE_DISTS)))
    # both mates present, and fragments change the depth
    assert sum(1 for r in recs if fragment_class(r) == 1) > 1000 and sum(1 for r in recs if fragment_class(r) == 2) > 1000
    frag, plain = model(f["lens"], recs)[0], DM.model(f["lens"], plain_records(recs), count_del=False)[0]
    assert all(not np.array_equal(a, b) for a, b in zip(frag, plain))
    assert max(int(x.max()) for x in frag) < 1 << 18                              # (below the no-index tables' 18-bit cells)


def splits_of(f):
    """{split name: units} of the fragment corpus, as bam_craft.splits_of's with the crafted stops of this file"""
    total = len(f["inf"])
    out = {"%d" % n: B.split_units(f["blocks"], f["offs"], total, n) for n in (1, 3, 64)}
    out["crafted"] = B.units_from_stops(f["blocks"], f["offs"], total, crafted_stops(f["offs"]))
    return out
