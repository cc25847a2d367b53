"""The model the `-rowreads` tests compare with, and the corpus they run on.

Written from the rule of DESIGN.md §6d, independent of the product.  A record STARTS AT cell (refID, pos) when 0 <= refID < n_ref and
0 <= pos < contig_len[refID]; every other record starts nowhere.  A ROW is a list of cell stretches [b, e) on one contig (a multiset: a
cell that lies in two stretches of a row counts twice).  Over the records that start in a row's cells (X: the flag mask, Q: the mapq
bound) the six numbers of the row are
    records   all of them                      passed    those with flag & X == 0        mapq0     the passed ones with mapq == 0
    kept      the passed ones with mapq >= Q   forward   the kept ones with flag & 0x10 == 0         mapq_sum  the sum of the kept ones' mapq
`Model.add` takes one record — frag_model's tuple (tid, pos, flag, mapq, cigar, mtid, tlen) — at a time and TESTS THE CELLS OF EVERY ROW
of the record's contig against pos (no prefix sums, no search; rows of equal windows are first narrowed to the one window pos / w can
lie in, and that window's cells are then tested like any other row's).

Row sets: the rows of the executable's tables (`rows_chr`, `rows_windows`, `rows_regions`: the identity columns come with them) and
the BINS of pd_decode_row_bins seen as rows (`bins_windows`, `bins_edges`: every bin is the one stretch of its elementary interval,
possibly empty), so that one model serves the file and the device's arrays.

The corpus is recstats_model's records (imported, not copied) on its header, plus records at the smallest places where the lookup can
go wrong (extra_reads), and a second, unsorted file.  A helper module, not a conftest."""
import os

import numpy as np

import bam_craft as B
import frag_model as FM
import recstats_model as RM

WORDS = 6
RECORDS, PASSED, MAPQ0, KEPT, FORWARD, MAPQ_SUM = range(6)
NAMES, LENS = RM.NAMES, RM.LENS                      # fa 100 000, fb 70 000, fc 5 000, one 1, empty 3 000
WINDOWS = (1, 7, 1000, 150000)                       # the tests' w: 150 000 is longer than the longest contig
M = 0

# the crafted regions, 1-based inclusive (contig, first, second, id), all on cells the extra records reach
REGIONS = [("fa", 85101, 85900, "g_plain"),
           ("fa", 86501, 87500, "g_overlap"), ("fa", 87001, 88000, "g_overlap"),      # two overlapping entries of one id: cells 87000 .. 87499 twice
           ("fa", 88001, 89000, "g_left"), ("fa", 89001, 90000, "g_right"),           # two ids sharing an edge (89000); g_left's first - 1 is g_overlap's second
           ("fb", 1025, 2048, "g_fb"),
           ("fc", 1, 100, "g_first"),                                                  # first - 1 = 0
           ("fc", 4001, 6000, "g_overhang"),                                           # overhangs the contig: clipped to 5 000
           ("one", 1, 1, "g_one"),
           ("empty", 1, 3000, "g_empty")]


# ---------------------------------------------------------------------------------------------------------------------
# row sets: [(tid, start, end, id or None, [(b, e), ...])] — start / end are the identity columns (1-based inclusive)
# ---------------------------------------------------------------------------------------------------------------------
def rows_chr(lens):
    """the whole-contig table: one row per contig of at least two bases"""
    return [(t, 1, ln, None, [(0, ln)]) for t, ln in enumerate(lens) if ln >= 2]


def rows_windows(lens, w):
    """the -w table: window k of a contig is cells [k w, min((k + 1) w, len)); a window that would begin at the contig's last cell (and
    every window of a contig shorter than two bases) is not a row of the table"""
    out = []
    for t, ln in enumerate(lens):
        k = 0
        while k * w + 1 < ln:
            out.append((t, k * w + 1, min((k + 1) * w, ln), None, [(k * w, min((k + 1) * w, ln))]))
            k += 1
    return out


def rows_regions(names, lens, regions):
    """the -g / -b table: one row per (contig, id); contigs in header order, a contig's ids by their smallest `first`, ties in the order
    of the ids as strings; the row's cells are its entries [first - 1, second) clipped to the contig, each entry counted"""
    out = []
    for t, ln in enumerate(lens):
        ids = {}
        for c, first, second, gid in regions:
            if names.index(c) == t:
                ids.setdefault(gid, []).append((first, second))
        for gid in sorted(sorted(ids), key=lambda g: min(f for f, _ in ids[g])):      # (the second sort is stable)
            ent = ids[gid]
            out.append((t, min(f for f, _ in ent), max(s for _, s in ent), gid, [(max(f - 1, 0), min(s, ln)) for f, s in ent]))
    return out


def bins_windows(lens, w):
    """pd_decode_row_bins(w): ceil(len / w) bins per contig, the last one short"""
    return [(t, k * w + 1, min((k + 1) * w, ln), None, [(k * w, min((k + 1) * w, ln))]) for t, ln in enumerate(lens) for k in range((ln + w - 1) // w)]


def bins_edges(lens, edges):
    """pd_decode_row_bins(0, edges): edges[t] strictly ascending -> k + 1 bins on contig t: [0, e0), [e0, e1), ... [e_last, len); a bin that
    begins at or behind the contig's end is empty"""
    out = []
    for t, ln in enumerate(lens):
        cut = [0] + [int(e) for e in edges[t]] + [ln]
        for j in range(len(cut) - 1):
            b, e = min(cut[j], ln), min(cut[j + 1], ln)
            out.append((t, b + 1, e, None, [(b, e)]))
    return out


def region_edges(names, lens, regions):
    """the edges of the crafted regions: every entry's first - 1 and second clipped to its contig, sorted and unique per contig"""
    ed = [set() for _ in lens]
    for c, first, second, _ in regions:
        t = names.index(c)
        b, e = max(first - 1, 0), min(second, lens[t])
        if b < e:
            ed[t] |= {b, e}
    return [sorted(s) for s in ed]


def edge_table(edges):
    """-> (edge_off uint64[n + 1], edges uint32) of pd_decode_row_bins"""
    off = np.zeros(len(edges) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(e) for e in edges])
    flat = np.array([v for e in edges for v in e], dtype=np.uint32)
    return off, flat


def bin_tables(names, lens):
    """{form: (the table as ("w", W) or ("edges", [a contig's edges]), the model's row set, uniform w)} for a header.  regions: the crafted regions' edges where the
    header is the corpus's, else edges at the same cells clipped to the header's contigs; every_cell: every cell of the 5 000-base
    contig (index 2 of the corpus's header, 1 of bam_craft's) an edge."""
    out = {}
    for w in WINDOWS:
        out["w%d" % w] = (("w", w), bins_windows(lens, w), w)
    out["no_edges"] = (("edges", None), bins_edges(lens, [[] for _ in lens]), 0)
    if names == NAMES:
        ed = region_edges(names, lens, REGIONS)
    else:
        ed = [sorted({min(e, ln) for e in (100, 899, 900, 1000, 65536, 70000)}) if ln > 1 else [] for ln in lens]
    out["regions"] = (("edges", ed), bins_edges(lens, ed), 0)
    small = lens.index(5000)
    cells = [list(range(ln)) if t == small else [] for t, ln in enumerate(lens)]
    out["every_cell"] = (("edges", cells), bins_edges(lens, cells), 0)
    return out


def session_table(table):
    """a table of bin_tables -> DecodeSession.begin's row_counts="""
    if table[0] == "w":
        return ("w", table[1])
    return ("edges", None, None) if table[1] is None else ("edges",) + edge_table(table[1])


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, lens, rows, flag_mask=1796, min_mapq=-1, uniform_w=0):
        """uniform_w: the rows are windows of that width in contig order (rows_windows / bins_windows) — add() then tests only the window
        pos // w of the contig, if the row set has it"""
        self.lens, self.rows, self.x, self.q, self.w = list(lens), rows, int(flag_mask), int(min_mapq), int(uniform_w)
        self.counts = np.zeros((len(rows), WORDS), dtype=np.uint64)
        self.nowhere = 0
        self.by_tid = {}
        for i, (t, _, _, _, segs) in enumerate(rows):
            d = self.by_tid.setdefault(t, dict(b=[], e=[], row=[], first=i))
            for b, e in segs:
                d["b"].append(b); d["e"].append(e); d["row"].append(i)
        for d in self.by_tid.values():
            d["b"], d["e"], d["row"] = (np.array(d[k], dtype=np.int64) for k in ("b", "e", "row"))

    def add(self, rec):
        tid, pos, flag, mapq = rec[:4]
        if tid < 0 or tid >= len(self.lens) or pos < 0 or pos >= self.lens[tid]:
            self.nowhere += 1
            return
        d = self.by_tid.get(tid)
        if d is None:
            return
        if self.w:
            k = pos // self.w
            hit = d["row"][k:k + 1][(d["b"][k:k + 1] <= pos) & (pos < d["e"][k:k + 1])]
        else:
            hit = d["row"][(d["b"] <= pos) & (pos < d["e"])]
        for i in hit:                                                      # (a row once per stretch that holds the cell)
            c = self.counts[i]
            c[RECORDS] += 1
            if flag & self.x:
                continue
            c[PASSED] += 1
            if mapq == 0:
                c[MAPQ0] += 1
            if mapq < self.q:
                continue
            c[KEPT] += 1
            c[MAPQ_SUM] += mapq
            if not flag & 0x10:
                c[FORWARD] += 1

    def add_all(self, recs):
        for r in recs:
            self.add(r)
        return self

    def text(self, names, mode):
        return text_of(names, self.rows, self.counts, mode)


def header(mode):
    """mode: "chr", "w", "g" (GeneID) or "b" (a 4-column BED: GeneID as well; RegionID is the 3-column BED's)"""
    ident = {"chr": "#Chr", "w": "#Chr\tStart\tEnd", "g": "#Chr\tStart\tEnd\tGeneID", "b": "#Chr\tStart\tEnd\tGeneID", "b3": "#Chr\tStart\tEnd\tRegionID"}[mode]
    return ident + "\tRecords\tPassed\tMapQ0\tKept\tForward\tMeanMapQ\n"


def text_of(names, rows, counts, mode):
    """the text of <prefix>.rowreads.stat.gz"""
    out = [header(mode)]
    for (t, start, end, gid, _), c in zip(rows, counts):
        c = [int(v) for v in c]
        ident = [names[t]] + ([] if mode == "chr" else [str(start), str(end)]) + ([gid] if gid is not None else [])
        out.append("\t".join(ident + [str(v) for v in c[:MAPQ_SUM]] + ["%.2f" % (c[MAPQ_SUM] / c[KEPT]) if c[KEPT] else "NA"]) + "\n")
    return "".join(out)


def started(lens, recs):
    """the records that start somewhere"""
    return sum(1 for r in recs if 0 <= r[0] < len(lens) and 0 <= r[1] < lens[r[0]])


def write_regions(d):
    """the crafted regions as a 4-column BED and as a GFF (feature CDS, Parent = the id) -> (bed path, gff path)"""
    bed, gff = os.path.join(str(d), "rr.bed4"), os.path.join(str(d), "rr.gff")
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\n" % r for r in REGIONS))
    with open(gff, "w") as f:
        f.write("##gff-version 3\n" + "".join("%s\tcraft\tCDS\t%d\t%d\t.\t+\t0\tID=c%d;Parent=%s\n" % (c, a, b, k, g) for k, (c, a, b, g) in enumerate(REGIONS)))
    return bed, gff


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
def extra_reads():
    """the records this option alone looks at (names say which); all behind recstats_model's laid-out stretch"""
    m50 = [(M, 50)]
    out = []

    def at(tid, pos, name, flag=0, mapq=60, ops=m50):
        out.append(FM._read(tid, pos, flag, mapq, name, ops, -1, 0, l_seq=None if ops else 30))

    # pos of -1 and len on a placed record (no CIGAR: they start nowhere and add no depth), 0 and len - 1 beside them
    for tid, ln in ((0, LENS[0]), (1, LENS[1]), (2, LENS[2])):
        at(tid, ln - 1, b"pos_len_minus_1_t%d" % tid)
        at(tid, ln, b"pos_len_t%d" % tid, ops=[])
    at(1, -1, b"pos_minus_1", flag=4, ops=[])
    at(1, 0, b"pos_0_fb")
    at(3, 1, b"pos_len_one_base", ops=[])
    # w - 1, w, w + 1 for w = 7 and w = 1000 at once: 83 999 = 7 * 11 999 + 6
    for p in (83999, 84000, 84001):
        at(0, p, b"window_edge_%d" % p)
    # mapq 0 and 255 on both strands, and dropped by the default mask on both
    for k, (flag, mapq) in enumerate(((0, 0), (16, 0), (0, 255), (16, 255), (0x400, 255), (0x410, 0), (0, 19), (16, 20))):
        at(0, 84500 + 3 * k, b"strand_mapq_%d" % k, flag=flag, mapq=mapq)
    # the regions' edges: first - 2, first - 1, second - 1, second of every entry on fa and fb; fc's overhang has len - 1 and len above
    for c, first, second, gid in REGIONS:
        t = NAMES.index(c)
        if t > 1:
            continue
        for p in (first - 2, first - 1, second - 1, second):
            at(t, p, b"edge_%s_%d" % (gid.encode(), p), flag=16 if p & 1 else 0, mapq=(0, 30, 60)[p % 3])
    at(2, 99, b"edge_g_first_99"); at(2, 100, b"edge_g_first_100"); at(2, 3999, b"edge_g_overhang_3999"); at(2, 4000, b"edge_g_overhang_4000")
    return out


def corpus_records(sub, seg):
    """recstats_model's records with the extra ones merged in by (tid, pos), as it merges its own: a stable sort behind the laid-out stretch"""
    base = RM.corpus_records(sub, seg)
    extra = [FM.encode_record(r, cg_tag=False) for r in extra_reads()]
    laid = next(k for k, r in enumerate(base) if RM._key(r) >= (0, 60000))
    assert all(RM._key(r) >= (0, 60000) for r in extra)
    return base[:laid] + sorted(base[laid:] + extra, key=RM._key)


def _file(d, stem, records):
    path = os.path.join(str(d), stem + ".bam")
    blocks, inf, offs = B.write_bam(path, NAMES, LENS, records, member_size=20000)
    lens, parsed = B.parse_bam(inf)
    assert lens == LENS and [r["off"] for r in parsed] == offs
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, names=NAMES, recs=parsed, data=open(path, "rb").read(), cases={})
    f["model_recs"] = FM.records_of(inf, parsed)
    f["sam"] = os.path.join(str(d), stem + ".sam")
    RM.write_sam(f["sam"], NAMES, inf, parsed, f["model_recs"])
    return f


def corpus(d):
    """writes rr.bam and rr.sam (coordinate-sorted) into directory d -> a file dict like recstats_model.corpus's"""
    sub, seg, _ = B.walk_geometry()
    f = _file(d, "rr", corpus_records(sub, seg))
    check_corpus(f, sub, seg)
    return f


def unsorted_records():
    """a file no sorted reader would take: a run in descending pos across the regions and windows the sorted corpus uses, contigs that
    alternate from record to record, and a second descending run that steps over one edge at a time"""
    m50 = [(M, 50)]
    out, k = [], 0

    def at(tid, pos, flag=0, mapq=60):
        nonlocal k
        out.append(FM._read(tid, pos, flag, mapq, b"u%05d" % k, m50, -1, 0))
        k += 1

    for p in range(91000, 83000, -7):                                         # descending over every crafted edge on fa
        at(0, p, flag=16 if p % 3 == 0 else 0, mapq=(0, 10, 20, 60, 255)[p % 5])
    for j in range(600):                                                      # the contig changes at every record
        at((0, 1, 2, 1)[j % 4], (j * 131) % 5000, flag=0x400 if j % 7 == 0 else 0, mapq=j % 61)
    for p in range(4999, -1, -1):                                             # every cell of fc, descending
        at(2, p, flag=16 if p & 4 else 0, mapq=p % 41)
    for j in range(300):                                                      # ascending again, then unplaced
        at(1, 1000 + 9 * j)
    out.append((-1, -1, 4, 0, b"u_unplaced", B.pack([]), 30, b"", -1, -1, 0))
    return [FM.encode_record(r, cg_tag=False) for r in out]


def unsorted(d):
    """writes rr_unsorted.bam into directory d -> a file dict; its cuts: 1 and 3 batches of two units"""
    f = _file(d, "rr_unsorted", unsorted_records())
    keys = [(r[0] if r[0] >= 0 else 1 << 31, r[1]) for r in f["model_recs"]]
    assert sum(1 for a, b in zip(keys, keys[1:]) if a > b) > 2000
    offs = f["offs"]
    f["cuts"] = {"%d" % nb: B.cut_batches(f, [offs[(len(offs) * k) // (2 * nb)] for k in range(1, 2 * nb)], 2) for nb in (1, 3)}
    return f


def session_cuts(f):
    return RM.session_cuts(f)


def check_corpus(f, sub, seg):
    """not vacuous, told from the parsed bytes"""
    recs = f["model_recs"]
    keys = [(r[0] if r[0] >= 0 else 1 << 31, r[1]) for r in recs]
    assert all(a <= b for a, b in zip(keys, keys[1:])), "not coordinate-sorted"
    at = {(r[0], r[1]) for r in recs}
    for t in (0, 1, 2):
        assert {(t, LENS[t] - 1), (t, LENS[t])} <= at
    assert {(1, -1), (1, 0), (2, 0), (3, 0), (3, 1), (0, 83999), (0, 84000), (0, 84001)} <= at and not any(r[0] == 4 for r in recs)
    for c, first, second, _ in REGIONS[:6]:
        t = NAMES.index(c)
        assert {(t, first - 1), (t, second - 1), (t, second)} <= at, (c, first, second)
    n_start = started(LENS, recs)
    assert 0 < len(recs) - n_start and sum(1 for r in recs if r[0] >= 0 and not 0 <= r[1] < LENS[r[0]]) >= 5
    for x, q in B.FILTERS:
        for rows in (rows_chr(LENS), rows_regions(NAMES, LENS, REGIONS)):
            c = Model(LENS, rows, x, q).add_all(recs).counts
            assert (c[:, RECORDS] >= c[:, PASSED]).all() and (c[:, PASSED] >= c[:, KEPT]).all() and (c[:, KEPT] >= c[:, FORWARD]).all()
            assert c[:, FORWARD].sum() > 0 and (c[:, KEPT] - c[:, FORWARD]).sum() > 0 and c[:, MAPQ0].sum() > 0
            assert (c[:, RECORDS] == c[:, PASSED]).all() if x == 0 else (c[:, RECORDS] > c[:, PASSED]).any() or rows[0][3] is not None
    whole = Model(LENS, rows_chr(LENS), 0, 0).add_all(recs).counts
    assert int(whole[:, RECORDS].sum()) == n_start - 3                         # (the one-base contig has three starts and no row)
    reg = Model(LENS, rows_regions(NAMES, LENS, REGIONS), 0, 0).add_all(recs)
    by_id = {r[3]: int(c[RECORDS]) for r, c in zip(reg.rows, reg.counts)}
    assert by_id["g_empty"] == 0 and by_id["g_one"] == 3 and all(v > 0 for k, v in by_id.items() if k != "g_empty"), by_id
    twice = sum(1 for r in recs if r[0] == 0 and 87000 <= r[1] < 87500)
    once = sum(1 for r in recs if r[0] == 0 and (86500 <= r[1] < 87000 or 87500 <= r[1] < 88000))
    assert twice > 0 and by_id["g_overlap"] == once + 2 * twice
    # a lane's stretch in which the contig changes: neighbouring records on different contigs, a few hundred bytes apart where a stretch has `sub`
    offs = f["offs"]
    assert sum(1 for a, b, oa, ob in zip(recs, recs[1:], offs, offs[1:]) if a[0] != b[0] and a[0] >= 0 and b[0] >= 0 and ob - oa < sub // 8) >= 3
