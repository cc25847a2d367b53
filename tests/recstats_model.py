"""The model the `-readstats` tests compare with, and the corpus they run on.

Written from the rule of DESIGN.md §6c, independent of the product.  Every record is in exactly one class, tested in this order
(n_ref: the header's contigs, X: the flag mask, Q: the mapq bound):
    unplaced      refID < 0 or refID >= n_ref
    dropped_flag  flag & X
    dropped_mapq  mapq < Q
    kept          everything else (the FILTER's verdict: contigs without targets or of fewer than two bases are kept all the same)
An INSERT PAIR is a kept record with flag & 0x3 == 0x3, flag & 0x908 == 0, next_refID == refID and tlen > 0; its bin is min(tlen, N).
The arrays are pd_decode_record_stats' (include/pandepth_amd.h): sums[PD_RECSTAT_FIXED + N + 1] and per_contig[n_ref][3].

`Model.add` takes one record — frag_model's tuple (tid, pos, flag, mapq, cigar, mtid, tlen) — at a time; `text_of` writes the arrays as
`<prefix>.reads.stat.gz` holds them.  The corpus is frag_model's fragment corpus (pairs with mate fields, records 1, 4, 35 and 36 bytes
before the end of a lane's stretch, a segment and a unit, the tlen edges) on a header with two more contigs — a one-base contig and one
that gets no record — plus records for what this option alone looks at.  A helper module, not a conftest."""
import math
import os
import struct

import numpy as np

import bam_craft as B
import frag_model as FM

FIXED = 275
RECORDS, UNPLACED, DROPPED_FLAG, DROPPED_MAPQ, KEPT, PAIRS, TLEN, FLAG0, MAPQ0 = 0, 1, 2, 3, 4, 5, 6, 7, 19
BINS = (1, 1000)                          # the tests' N

NAMES, LENS = FM.FRAG_NAMES + ["one", "empty"], FM.FRAG_LENS + [1, 3000]
M = 0


class Model:
    def __init__(self, names, lens, flag_mask=1796, min_mapq=0, n_bins=1000):
        self.names, self.lens, self.x, self.q, self.n = list(names), list(lens), int(flag_mask), int(min_mapq), int(n_bins)
        self.sums = np.zeros(FIXED + self.n + 1, dtype=np.uint64)
        self.per = np.zeros((len(self.lens), 3), dtype=np.uint64)

    def add(self, rec):
        tid, pos, flag, mapq, cig, mtid, tlen = rec
        s = self.sums
        s[RECORDS] += 1
        for k in range(12):
            if flag >> k & 1:
                s[FLAG0 + k] += 1
        if tid < 0 or tid >= len(self.lens):
            s[UNPLACED] += 1
            return
        self.per[tid, 0] += 1
        if flag & self.x:
            s[DROPPED_FLAG] += 1
            return
        s[MAPQ0 + mapq] += 1
        if mapq < self.q:
            s[DROPPED_MAPQ] += 1
            return
        s[KEPT] += 1
        self.per[tid, 1] += 1
        self.per[tid, 2] += mapq
        if flag & 0x3 == 0x3 and not flag & 0x908 and mtid == tid and tlen > 0:
            s[PAIRS] += 1
            s[TLEN] += tlen
            s[FIXED + min(tlen, self.n)] += 1

    def add_all(self, recs):
        for r in recs:
            self.add(r)
        return self

    def arrays(self):
        return self.sums.copy(), self.per.copy()

    def text(self):
        return text_of(self.names, self.lens, self.sums, self.per, self.x, self.q, self.n)


def text_of(names, lens, sums, per, flag_mask, min_mapq, n):
    """the text of <prefix>.reads.stat.gz for these arrays"""
    s = [int(v) for v in sums]
    pairs = s[PAIRS]
    out = ["# SN\tkey\tvalue"]
    for key, k in (("records", RECORDS), ("unplaced", UNPLACED), ("dropped_flag", DROPPED_FLAG), ("dropped_mapq", DROPPED_MAPQ), ("kept", KEPT)):
        out.append("SN\t%s\t%d" % (key, s[k]))
    out += ["SN\tflag_mask\t%d" % flag_mask, "SN\tmin_mapq\t%d" % min_mapq, "SN\tinsert_bins\t%d" % n, "SN\tinsert_pairs\t%d" % pairs]
    if pairs:
        rank, cum, med = max(1, math.ceil(pairs / 2)), 0, None
        for b in range(1, n + 1):
            cum += s[FIXED + b]
            if cum >= rank:
                med = b
                break
        out += ["SN\tinsert_mean\t%.2f" % (s[TLEN] / pairs), "SN\tinsert_median\t%s" % (">=%d" % n if med == n else "%d" % med)]
    else:
        out += ["SN\tinsert_mean\tNA", "SN\tinsert_median\tNA"]
    out.append("# FL\tbit\tcount")
    out += ["FL\t0x%x\t%d" % (1 << k, s[FLAG0 + k]) for k in range(12)]
    out.append("# CT\tcontig\tLength\tRecords\tKept\tMeanMapQ")
    for t, (nm, ln) in enumerate(zip(names, lens)):
        rec, kept, mq = (int(v) for v in per[t])
        out.append("CT\t%s\t%d\t%d\t%d\t%s" % (nm, ln, rec, kept, "%.2f" % (mq / kept) if kept else "NA"))
    out.append("CT\t*\t0\t%d\t0\tNA" % s[UNPLACED])
    out.append("# MQ\tmapq\tcount")
    out += ["MQ\t%d\t%d" % (q, s[MAPQ0 + q]) for q in range(256) if s[MAPQ0 + q]]
    out.append("# IS\tsize\tcount")
    out += ["IS\t%d\t%d" % (b, s[FIXED + b]) for b in range(1, n) if s[FIXED + b]]
    if s[FIXED + n]:
        out.append("IS\t>=%d\t%d" % (n, s[FIXED + n]))
    return "\n".join(out) + "\n"


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
def extra_reads():
    """the records this option alone looks at (names say which); all behind the fragment corpus's own on their contigs"""
    m50 = [(M, 50)]
    out = []
    for k in range(12):                                                        # every flag bit set alone
        out.append(FM._read(0, 80000 + 10 * k, 1 << k, 60, b"flag_bit_%d" % k, m50, -1, 0))
    out.append(FM._read(0, 81000, 0, 0, b"mapq_0", m50, -1, 0))
    out.append(FM._read(0, 81010, 0, 255, b"mapq_255", m50, -1, 0))
    for k, n in enumerate(BINS):                                               # either side of the cap: N - 1, N, N + 1
        for j, t in enumerate((n - 1, n, n + 1)):
            out.append(FM._read(1, 20000 + 1000 * k + 10 * j, 99, 60, b"cap_%d_%d" % (n, t), m50, 1, t))
    for k in range(3):                                                         # the one-base contig: kept by the filter, never walked
        out.append(FM._read(3, 0, 99 if k == 2 else 0, 60, b"one_base_%d" % k, m50, 3, 7 if k == 2 else 0))
    # the unplaced tail: without and with pair flags (the second would be an insert pair were it placed)
    out.append((-1, -1, 4, 0, b"unplaced_plain", B.pack([]), 30, b"", -1, -1, 0))
    out.append((-1, -1, 0x4D, 0, b"unplaced_paired", B.pack([]), 30, b"", -1, -1, 0))
    out.append((-1, -1, 99, 60, b"unplaced_pair_flags", B.pack([]), 30, b"", -1, -1, 300))
    return out


def _key(rec_bytes):
    tid, pos = struct.unpack_from("<ii", rec_bytes, 4)
    return (tid if tid >= 0 else 1 << 31, pos)


def corpus_records(sub, seg):
    """frag_model's records, laid out against THIS header (its layout counts from the header's length), and the extra ones merged in by
    (tid, pos) — a stable sort, and every extra record lies behind the laid-out stretch, which therefore stays byte for byte where it is"""
    saved = FM.FRAG_NAMES, FM.FRAG_LENS
    FM.FRAG_NAMES, FM.FRAG_LENS = NAMES, LENS
    try:
        base = FM.corpus_records(sub, seg)
    finally:
        FM.FRAG_NAMES, FM.FRAG_LENS = saved
    extra = [FM.encode_record(r, cg_tag=False) for r in extra_reads()]
    laid = next(k for k, r in enumerate(base) if _key(r) >= (0, 60000))
    assert all(_key(r) >= (0, 60000) for r in extra)
    return base[:laid] + sorted(base[laid:] + extra, key=_key)


def write_sam(path, names, inf, parsed, model_recs):
    with open(path, "w") as out:
        out.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, LENS)))
        for r, m in zip(parsed, model_recs):
            mtid, mpos, tlen = FM.mate_fields(inf, r["off"])
            cig = "".join("%d%s" % (c >> 4, "MIDNSHP=X"[c & 0xf]) for c in m[4].tolist()) or "*"
            rname = names[r["tid"]] if r["tid"] >= 0 else "*"
            rnext = "*" if mtid < 0 else "=" if mtid == r["tid"] else names[mtid]
            out.write("\t".join([FM.name_of(inf, r["off"]).decode(), str(r["flag"]), rname, str(r["pos"] + 1), str(r["mapq"]), cig, rnext,
                                 str(mpos + 1), str(tlen), "*", "*"]) + "\n")


def corpus(d):
    """writes rs.bam and rs.sam into directory d -> a file dict like frag_model.fragment_corpus's"""
    sub, seg, coop = B.walk_geometry()
    path = os.path.join(str(d), "rs.bam")
    blocks, inf, offs = B.write_bam(path, NAMES, LENS, corpus_records(sub, seg), member_size=20000)
    lens, parsed = B.parse_bam(inf)
    assert lens == LENS and [r["off"] for r in parsed] == offs
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, names=NAMES, recs=parsed, data=open(path, "rb").read(), cases={})
    f["model_recs"] = FM.records_of(inf, parsed)
    f["sam"] = os.path.join(str(d), "rs.sam")
    write_sam(f["sam"], NAMES, inf, parsed, f["model_recs"])
    check_corpus(f, sub, seg)
    return f


def session_cuts(f):
    """{label: batches} for the decode-session tests: 1, 3 and 16 batches of two units cut at record starts, and the crafted stops (units
    that end 1, 4, 35 and 36 bytes behind the start of their last record) one unit to a batch"""
    offs = f["offs"]
    out = {}
    for nb in (1, 3, 16):
        out["%d" % nb] = B.cut_batches(f, [offs[(len(offs) * k) // (2 * nb)] for k in range(1, 2 * nb)], 2)
    out["crafted"] = B.cut_batches(f, FM.crafted_stops(offs), 1)
    return out


def check_corpus(f, sub, seg):
    """not vacuous, told from the parsed bytes: every class under both filters, every flag bit, both sides of the cap for every N, the
    layout edges, the contigs' special cases"""
    recs, offs, total = f["model_recs"], f["offs"], len(f["inf"])
    keys = [(r[0] if r[0] >= 0 else 1 << 31, r[1]) for r in recs]
    assert all(a <= b for a, b in zip(keys, keys[1:])), "not coordinate-sorted"
    for x, q in B.FILTERS:
        for n in BINS:
            s, per = Model(NAMES, LENS, x, q, n).add_all(recs).arrays()
            assert int(s[RECORDS]) == len(recs) == int(s[UNPLACED] + s[DROPPED_FLAG] + s[DROPPED_MAPQ] + s[KEPT])
            assert s[UNPLACED] >= 3 and s[KEPT] > 1000 and s[PAIRS] > 500
            assert (x == 0) == (s[DROPPED_FLAG] == 0) and (q <= 0) == (s[DROPPED_MAPQ] == 0)
            assert all(s[FLAG0 + k] > 0 for k in range(12))
            assert s[MAPQ0 + 255] > 0 and (x != 0 or s[MAPQ0] > 0)
            assert s[FIXED + n] > 0 and (n == 1 or (s[FIXED + n - 1] > 0 and s[FIXED + 1:FIXED + n].sum() > 0))
            assert per[3, 0] == 3 and per[3, 1] > 0 and per[4].sum() == 0 and int(per[:, 0].sum() + s[UNPLACED]) == len(recs)
    assert any(r[2] & x for x, _ in B.FILTERS for r in recs) and any(r[3] < 20 for r in recs) and any(r[3] >= 20 for r in recs)
    flags_alone = {r[2] for r in recs}
    assert all(1 << k in flags_alone for k in range(12))
    tl = {r[6] for r in recs if r[2] & 3 == 3 and not r[2] & 0x908 and r[5] == r[0] >= 0}
    assert {0, 1, 2, 999, 1000, 1001, FM.INT32_MAX} <= tl and FM.INT32_MIN in {r[6] for r in recs} and any(t < 0 for t in tl)
    assert any(r[0] == -1 and r[2] & 3 == 3 and r[6] > 0 for r in recs) and any(r[0] == -1 and not r[2] & 1 for r in recs)
    # the layout: records 1, 4, 35, 36 bytes before the end of a lane's stretch, a segment (one unit) and a unit (the crafted stops)
    one = B.census(offs, total, B.split_units(f["blocks"], offs, total, 1), sub, seg)
    assert set(FM.EDGE_DISTS) <= one["lane_end"] and set(FM.EDGE_DISTS) <= one["seg_end"], one
    cr = B.census(offs, total, B.units_from_stops(f["blocks"], offs, total, FM.crafted_stops(offs)), sub, seg)
    assert set(FM.EDGE_DISTS) <= cr["unit_end"], cr
