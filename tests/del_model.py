"""The model the `-del` tests compare with: depth where deletions count as covered, and the number of runs the walkers must emit.

Written from the rule of DESIGN.md §6a and the SAM specification (§1.4 the CIGAR operations), independent of the product: it parses SAM text
(or takes the records bam_craft.parse_bam read from a BAM's inflated bytes, or a PAF's cg:Z: strings) itself, keeps what the
program keeps — the flag mask, the mapq bound, contigs of at least 2 bases — and
  * adds 1 over every M/=/X/D operation (over M/=/X alone with count_del=False), each clipped to its contig: the depth is taken
    per OPERATION, so it does not depend on how operations are grouped into runs;
  * counts GROUPS: maximal sequences of M/=/X/D operations with no N between them (I/S/H/P inside do not split one; an N of any
    length, 0 included, does; a group of total length 0 still counts).  The group no N comes before is the record's first run, every
    later one an "other" run.
A helper module, not a conftest."""
import gzip
import re
import zlib

import numpy as np

import bam_craft as B

M, I, D, N, S, H, P, EQ, X = range(9)
_CODE = {c: k for k, c in enumerate("MIDNSHP=X")}
_COVER_DEL = np.array([k in (M, EQ, X, D) for k in range(16)])
_COVER_REF = np.array([k in (M, EQ, X) for k in range(16)])
_ADVANCE = np.array([k in (M, EQ, X, D, N) for k in range(16)])


def parse_cigar(text):
    """'10M5D' -> packed uint32 (len << 4 | op); '*' -> empty"""
    if text == "*":
        return np.zeros(0, dtype=np.uint32)
    return np.array([(int(n) << 4) | _CODE[c] for n, c in re.findall(r"(\d+)([MIDNSHP=X])", text)], dtype=np.uint32)


def read_sam(path):
    """-> names, lens, records [(tid, pos0, flag, mapq, packed cigar)]"""
    names, lens, recs = [], [], []
    for line in open(path):
        if line.startswith("@"):
            if line.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in line.rstrip("\n").split("\t")[1:])
                names.append(f["SN"]); lens.append(int(f["LN"]))
            continue
        c = line.rstrip("\n").split("\t")
        if len(c) < 6:
            continue
        recs.append((names.index(c[2]) if c[2] != "*" else -1, int(c[3]) - 1, int(c[1]), int(c[4]), parse_cigar(c[5])))
    return names, lens, recs


def read_bam(path):
    """the same from a BAM file, read with bam_craft's parser of the inflated bytes (CIGARs in the CG tag resolved)"""
    data = open(path, "rb").read()
    inf = b"".join(zlib.decompress(data[b[0]:b[0] + b[2]], -15) for b in _members(data))
    lens, parsed = B.parse_bam(inf)
    return lens, crafted_records(parsed)


def _members(data):
    import struct
    o = 0
    while o + 18 <= len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bs = struct.unpack_from("<H", data, o + 16)[0] + 1
        yield (o + 12 + xlen, 0, bs - 12 - xlen - 8)
        o += bs


def crafted_records(parsed):
    """bam_craft.parse_bam's records -> the model's tuples"""
    return [(r["tid"], r["pos"], r["flag"], r["mapq"], B.real_cigar(r)) for r in parsed]


def groups(cigar):
    """-> (n_first, n_other) of one record's CIGAR under the group rule"""
    n_first = n_other = 0
    is_open, cut = False, False
    for op in (cigar & 0xf).tolist():
        if op in (M, EQ, X, D):
            is_open = True
        elif op == N:
            if is_open:
                n_first, n_other = n_first + (not cut), n_other + cut
            is_open, cut = False, True
    if is_open:
        n_first, n_other = n_first + (not cut), n_other + cut
    return int(n_first), int(n_other)


def model(lens, recs, flag_mask=1796, min_mapq=-1, count_del=True):
    """-> per-contig uint32 depth (None for contigs shorter than 2 bases), n_first, n_other (the group counts; with count_del=False
    the reference's: one run per M/=/X, the first one first when no D / N comes before it)"""
    cover = _COVER_DEL if count_del else _COVER_REF
    diff = [np.zeros(l + 1, dtype=np.int64) if l >= 2 else None for l in lens]
    n_first = n_other = 0
    for tid, pos, flag, mapq, cig in recs:
        if flag & flag_mask or mapq < min_mapq or not 0 <= tid < len(lens) or diff[tid] is None:
            continue
        op, ln = cig & 0xf, (cig >> 4).astype(np.int64)
        adv = np.where(_ADVANCE[op], ln, 0)
        beg = pos + np.cumsum(adv) - adv
        run = cover[op]
        L = lens[tid]
        np.add.at(diff[tid], np.clip(beg[run], 0, L), 1)
        np.add.at(diff[tid], np.clip(beg[run] + ln[run], 0, L), -1)
        if count_del:
            f, o = groups(cig)
        else:
            gap = np.isin(op, (D, N))
            runs = np.flatnonzero(run)
            f = int(runs.size > 0 and not gap[:runs[0]].any())
            o = int(runs.size) - f
        n_first += f; n_other += o
    return [None if d is None else np.cumsum(d[:-1]).astype(np.uint32) for d in diff], n_first, n_other


def has_gaps(recs):
    """does any CIGAR hold a D or an N?"""
    return any(np.isin(c & 0xf, (D, N)).any() for *_, c in recs)


def paf_model(path, names, lens, min_mapq=-1, count_del=True, flag_mask=1796):
    """Depth of a PAF file (plain or gzip) on the targets `names` / `lens`: a line with cg:Z: is walked from its target start
    (column 8) like a CIGAR, a line without one covers [tstart - 1, tend) as the program always did.  -> per-contig uint32 depth,
    the number of cg values with D or N"""
    diff = [np.zeros(l + 1, dtype=np.int64) for l in lens]
    opener = gzip.open if path.endswith(".gz") else open
    n_gap = 0
    for line in opener(path, "rt"):
        c = line.split()
        n_gap += any(x.startswith("cg:Z:") and re.search(r"\d[DN]", x) is not None for x in c[12:])       # (of every line, kept or not)
        if len(c) < 12 or int(c[11]) < min_mapq or (flag_mask & 0x100 and "tp:A:S" in line):      # (secondary alignments go with flag 256)
            continue
        tid, L = names.index(c[5]), lens[names.index(c[5])]
        s, e = sorted((int(c[7]), int(c[8])))
        cg = [x[5:] for x in c[12:] if x.startswith("cg:Z:")]
        if cg:
            cur = s
            ops = re.findall(r"(\d+)(.)", cg[0])
            for n, o in ops:
                n = int(n)
                if o in "M=X" or (o == "D" and count_del):
                    diff[tid][min(max(cur, 0), L)] += 1; diff[tid][min(max(cur + n, 0), L)] -= 1
                if o in "M=XDN":
                    cur += n
        elif e > s - 1:
            diff[tid][min(max(s - 1, 0), L)] += 1; diff[tid][min(max(e, 0), L)] -= 1
    return [np.cumsum(d[:-1]).astype(np.uint32) for d in diff], n_gap


# ---------------------------------------------------------------------------------------------------------------------
# the deletion corpus: one small BAM (bam_craft's writer) with every group edge of the lane walk and of the wave walk
# ---------------------------------------------------------------------------------------------------------------------
DEL_NAMES, DEL_LENS = ["c5000", "one"], [5000, 1]
_SHORT = ["10M5D10M", "5D10M", "10D", "10M5N10M", "10M0N10M", "5N10M", "10M5D5N5D10M", "10M2I10M", "5S10M3D", "10N", "5I"]


def _alternating(n):
    """n operations 2M 1I 2M 1D 2M 1I ..."""
    return [((M, 2), (I, 1), (M, 2), (D, 1))[k % 4] for k in range(n)]


def deletion_cigars():
    """-> [(name, ops)]: the short CIGARs a lane walks on its own, and CIGARs at the wave walk's threshold (96 operations) and step (64)"""
    out = [(t, [(_CODE[c], int(n)) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", t)]) for t in _SHORT]
    for n in (95, 96, 127, 128, 129, 192):
        out.append(("alt%d" % n, _alternating(n)))
    for n in (129, 192):
        for at in (63, 64, 65):
            for op, ln in ((D, 1), (N, 3), (N, 0)):
                ops = _alternating(n); ops[at] = (op, ln)
                out.append(("alt%d_%s%d_at%d" % (n, "MIDN"[op], ln, at), ops))
    ops = _alternating(192)
    ops[64:128] = [((D, 1), (I, 1))[k % 2] for k in range(64)]                 # one whole step of D and I: the group stays open across three steps
    out.append(("step_of_D_I", ops))
    ops = list(ops); ops[128] = (N, 2)                                         # ... and is closed by the first operation of the third
    out.append(("step_of_D_I_then_N", ops))
    ops = _alternating(192); ops[64:128] = [(I, 1)] * 64; ops[63] = (I, 1); ops[128] = (N, 4)
    out.append(("N_behind_a_step_without_reference", ops))
    for n in (96, 128, 192):
        ops = _alternating(n); ops[0] = (N, 2); out.append(("N_first_%d" % n, ops))
        ops = _alternating(n); ops[-1] = (N, 2); out.append(("N_last_%d" % n, ops))
    for at in (63, 100, 127):
        ops = _alternating(192); ops[at] = (N, 1); ops[at + 1] = (N, 2); out.append(("NN_at%d" % at, ops))
    ops = _alternating(192); ops[0:3] = [(D, 2), (I, 1), (D, 1)]; out.append(("opens_with_D_192", ops))
    ops = _alternating(65536); ops[40000] = (N, 7); out.append(("cg65536", ops))
    return out


def deletion_corpus(d):
    """writes del.bam into directory d -> a file dict like bam_craft.build_corpus's (path, blocks, inf, offs, lens, recs, data)"""
    import os
    recs = []
    cigs = deletion_cigars()
    for k, (name, ops) in enumerate(cigs):
        pos = min(10 + 37 * k, 4400)
        recs.append((0, pos, 1024 if k % 7 == 3 else 0, 5 if k % 5 == 2 else 60, name.encode(), B.pack(ops), B.qlen(ops), b""))
    recs.append((0, 4990, 0, 60, b"overhang", B.pack([(M, 5), (D, 20)]), 5, b""))
    recs.append((0, 4995, 16, 30, b"overhang_N", B.pack([(M, 2), (N, 1), (D, 20), (M, 3)]), 5, b""))
    recs.append((1, 0, 0, 60, b"one_cell", B.pack([(M, 1), (D, 1)]), 1, b""))
    recs.sort(key=lambda r: (r[0], r[1]))
    path = os.path.join(str(d), "del.bam")
    blocks, inf, offs = B.write_bam(path, DEL_NAMES, DEL_LENS, recs, member_size=20000)
    lens, parsed = B.parse_bam(inf)
    assert lens == DEL_LENS and [r["off"] for r in parsed] == offs
    return dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=parsed, data=open(path, "rb").read(), cases={})
