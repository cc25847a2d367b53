"""The model the `-alnstats` tests compare with, and the crafted file `aln_edges` they run on beside bam_craft's corpus.

Written from the rule of DESIGN.md §6e, one record at a time, independent of the product.

THE CIGAR of a record is its own operations, or htslib's CG-tag rule where it applies: the first operation is <l_seq>S, refID >= 0 and
pos >= 0, and the record's FIRST CG tag is of type B,I or B,i and has at least n_cigar_op entries — then the tag's entries are the CIGAR.
An operation is a 32-bit word, code = word & 0xf, len = word >> 4; its class is the code for codes 0 .. 8 (M I D N S H P = X) and 9,
`other`, for 9 .. 15.  An ALIGNED record has 0 <= refID < n_ref, flag & X == 0, mapq >= Q, flag & 4 == 0 and at least one operation; a
PRIMARY record is an aligned one with flag & 0x900 == 0.  Per aligned record: q = the lengths of M I S = X, h = of H, L = q + h,
a = of M I = X, r = of M D N = X; it is clipped when an S or H has a length above 0.

The array is pd_decode_aln_stats' (include/pandepth_amd.h), PD_ALNSTAT_WORDS words; `text_of` writes it as `<prefix>.aln.stat.gz` holds
it.  A helper module, not a conftest."""
import os
import struct

import numpy as np

import bam_craft as B

LEN_BINS, INDEL_BINS = 8192, 256
RECORDS, ALIGNED, PRIMARY, CLIPPED, READ_MAX, READ_BASES, ALIGNED_BASES, REF_BASES, OPS = range(9)
INS = OPS + 20
DEL = INS + INDEL_BINS + 1
AF = DEL + INDEL_BINS + 1
RL = AF + 101
AL = RL + 2 * LEN_BINS
WORDS = AL + 2 * LEN_BINS
OP_NAMES = ["M", "I", "D", "N", "S", "H", "P", "=", "X", "other"]
WIDTHS = (1, 100)                         # the tests' W
LDS_BINS = 512                            # pd_alnstats.h's AS_LDS_BINS: length bins below it are kept in LDS, the others go to global memory
MAXLEN = (1 << 28) - 1


def lds_bins():
    """AS_LDS_BINS as pd_alnstats.h defines it"""
    import re
    text = open(os.path.join(B.ROOT, "pandepth_amd", "csrc", "pd_alnstats.h")).read()
    return int(re.search(r"AS_LDS_BINS\s*=\s*(\d+)", text).group(1))


def cigar_of(r):
    """the CIGAR of a record of bam_craft.parse_bam: htslib's CG-tag rule"""
    c = r["cigar"]
    if c.size >= 1 and r["tid"] >= 0 and r["pos"] >= 0 and int(c[0]) & 0xf == B.S and int(c[0]) >> 4 == r["l_seq"]:
        for name, ty, val in r["tags"]:
            if name == b"CG":
                if ty == b"B" and val[0] in (b"I", b"i") and val[1].size >= c.size:
                    return val[1].astype(np.uint32)
                break
    return c


class Model:
    def __init__(self, n_ref, flag_mask=1796, min_mapq=0, width=1):
        self.n_ref, self.x, self.q, self.w = int(n_ref), int(flag_mask), int(min_mapq), int(width)
        self.s = [0] * WORDS                                                   # Python integers: nothing wraps

    def add(self, tid, flag, mapq, cigar):
        s = self.s
        s[RECORDS] += 1
        if not 0 <= tid < self.n_ref or flag & self.x or mapq < self.q or flag & 4 or len(cigar) < 1:
            return
        b = [0] * 10
        for word in (int(v) for v in cigar):
            code, ln = word & 0xf, word >> 4
            k = code if code <= 8 else 9
            s[OPS + 2 * k] += 1
            s[OPS + 2 * k + 1] += ln
            b[k] += ln
            if k == 1:
                s[INS + min(ln, INDEL_BINS)] += 1
            if k == 2:
                s[DEL + min(ln, INDEL_BINS)] += 1
        a = b[0] + b[1] + b[7] + b[8]
        L = a + b[4] + b[5]
        s[ALIGNED] += 1
        s[CLIPPED] += 1 if b[4] > 0 or b[5] > 0 else 0
        s[ALIGNED_BASES] += a
        s[REF_BASES] += b[0] + b[2] + b[3] + b[7] + b[8]
        s[AL + 2 * min(a // self.w, LEN_BINS - 1)] += 1
        s[AL + 2 * min(a // self.w, LEN_BINS - 1) + 1] += a
        if flag & 0x900:
            return
        s[PRIMARY] += 1
        s[READ_BASES] += L
        s[READ_MAX] = max(s[READ_MAX], L)
        s[RL + 2 * min(L // self.w, LEN_BINS - 1)] += 1
        s[RL + 2 * min(L // self.w, LEN_BINS - 1) + 1] += L
        if L > 0:
            s[AF + 100 * a // L] += 1

    def add_parsed(self, recs):
        """bam_craft.parse_bam's records"""
        for r in recs:
            self.add(r["tid"], r["flag"], r["mapq"], cigar_of(r))
        return self

    def add_tuples(self, recs):
        """frag_model's tuples (tid, pos, flag, mapq, cigar, ...), the CIGAR already the real one"""
        for r in recs:
            self.add(r[0], r[2], r[3], r[4])
        return self

    def array(self):
        assert max(self.s) < 1 << 64
        return np.array(self.s, dtype=np.uint64)

    def text(self):
        return text_of(self.s, self.x, self.q, self.w)


def text_of(sums, flag_mask, min_mapq, w):
    """the text of <prefix>.aln.stat.gz for this array"""
    s = [int(v) for v in sums]
    out = ["# SN\tkey\tvalue"]
    out += ["SN\t%s\t%d" % (key, s[k]) for k, key in enumerate(("records", "aligned", "primary", "clipped"))]
    out += ["SN\tflag_mask\t%d" % flag_mask, "SN\tmin_mapq\t%d" % min_mapq, "SN\tbin_width\t%d" % w, "SN\tlen_bins\t%d" % LEN_BINS]
    out.append("SN\tread_bases\t%d" % s[READ_BASES])
    out.append("SN\tread_mean\t%s" % ("%.2f" % (s[READ_BASES] / s[PRIMARY]) if s[PRIMARY] else "NA"))
    out.append("SN\tread_max\t%s" % ("%d" % s[READ_MAX] if s[PRIMARY] else "NA"))
    n50 = "NA"
    if s[READ_BASES]:
        half, cum = (s[READ_BASES] + 1) // 2, 0
        for b in range(LEN_BINS - 1, -1, -1):
            cum += s[RL + 2 * b + 1]
            if cum >= half:
                n50 = (">=" if b == LEN_BINS - 1 else "") + "%d" % (b * w)
                break
    out.append("SN\tread_n50\t%s" % n50)
    out.append("SN\taligned_bases\t%d" % s[ALIGNED_BASES])
    out.append("SN\taligned_mean\t%s" % ("%.2f" % (s[ALIGNED_BASES] / s[ALIGNED]) if s[ALIGNED] else "NA"))
    out.append("SN\tref_bases\t%d" % s[REF_BASES])
    out.append("# OP\top\tops\tbases")
    out += ["OP\t%s\t%d\t%d" % (nm, s[OPS + 2 * k], s[OPS + 2 * k + 1]) for k, nm in enumerate(OP_NAMES)]
    out.append("# ID\tlength\tinsertions\tdeletions")
    out += ["ID\t%s\t%d\t%d" % (">=%d" % b if b == INDEL_BINS else "%d" % b, s[INS + b], s[DEL + b]) for b in range(INDEL_BINS + 1) if s[INS + b] or s[DEL + b]]
    for tag, base in (("RL", RL), ("AL", AL)):
        out.append("# %s\tfrom\tto\trecords\tbases" % tag)
        out += ["%s\t%d\t%s\t%d\t%d" % (tag, b * w, "inf" if b == LEN_BINS - 1 else "%d" % (b * w + w - 1), s[base + 2 * b], s[base + 2 * b + 1])
                for b in range(LEN_BINS) if s[base + 2 * b]]
    out.append("# AF\tpercent\trecords")
    out += ["AF\t%d\t%d" % (p, s[AF + p]) for p in range(101) if s[AF + p]]
    return "\n".join(out) + "\n"


def sorted_n50(lengths):
    """the N50 by its definition: the largest length such that the reads at least that long hold half of all bases (rounded up)"""
    total, cum = sum(lengths), 0
    for L in sorted(lengths, reverse=True):
        cum += L
        if cum >= (total + 1) // 2:
            return L
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the crafted file: what bam_craft.special_reads lacks
# ---------------------------------------------------------------------------------------------------------------------
M, I, D, N, S, H, P, EQ, X = range(9)
ONE = B.NAMES.index("one")
HOSTILE = (0, 1, 255, 256, 257, MAXLEN)
# read lengths: k W - 1 and k W for both widths, the last bin's edge +- 1 for both widths, and both sides of the LDS bin limit for both widths
LENGTHS = sorted({99, 100, 299, 300, 8190, 8191, 8192, 8191 * 100 - 1, 8191 * 100, 8191 * 100 + 1,
                  LDS_BINS - 1, LDS_BINS, LDS_BINS * 100 - 1, LDS_BINS * 100})


def edge_reads():
    """-> [(case, record)] in file order: on contig 0 at rising positions, then on the one-base contig, the unplaced one last.  l_seq is small whatever the CIGAR
    says (the sequence bytes are not what is tested)."""
    out = []
    pos = [1000]

    def add(case, ops, flag=0, mapq=60, tags=b"", l_seq=0, tid=0):
        out.append((case, (tid, pos[0] if tid == 0 else 0 if tid > 0 else -1, flag, mapq, case.encode(), B.pack(ops), l_seq, tags)))
        pos[0] += 37

    add("codes_9_15", [(M, 10), (9, 5), (15, 7), (M, 3), (12, 0)])
    add("hard_both_ends", [(H, 5), (M, 20), (H, 7)])
    add("only_h_p", [(H, 30), (P, 2)])
    add("only_d", [(D, 12)])
    add("zero_len_clips", [(S, 0), (M, 9), (H, 0)])                             # an S and an H of length 0: not clipped
    for L in LENGTHS:
        add("len_%d" % L, [(M, L)])
    add("len_%d_hard" % (LDS_BINS * 100), [(H, LDS_BINS * 100 - 40), (M, 40)])   # L across the LDS limit, a far below it
    read = [(S, 10), (M, 50), (I, 2), (M, 40)]
    add("copy_primary", read)
    add("copy_secondary", read, flag=0x100)
    add("copy_supplementary", [(H, 10), (M, 50), (H, 42)], flag=0x800)
    add("unmapped_with_cigar", [(M, 30)], flag=4)
    add("no_cigar", [])
    add("low_mapq", [(M, 25), (I, 1)], mapq=5)
    real = B.pack([((M, 3), (I, 1), (M, 2), (D, 1))[k % 4] for k in range(300)])
    ph = [(S, B.qlen(real)), (N, B.rlen(real))]
    cg = b"CGBI" + struct.pack("<I", real.size) + real.astype("<u4").tobytes()
    add("cg_dropped", ph, flag=1024, mapq=5, tags=cg, l_seq=B.qlen(real))
    add("cg_kept_300", ph, tags=B.tag_i(b"NM", 3) + cg, l_seq=B.qlen(real))
    small = B.pack([(M, 4), (I, 2), (EQ, 3)])
    add("cg_kept_3_signed", [(S, 9), (N, 7)], tags=b"CGBi" + struct.pack("<I", 3) + small.astype("<u4").tobytes(), l_seq=9)
    add("cg_too_short", [(S, 9), (N, 7), (M, 1)], tags=b"CGBI" + struct.pack("<I", 2) + small[:2].astype("<u4").tobytes(), l_seq=9)
    add("cg_wrong_type", [(S, 9), (N, 7)], tags=B.tag_B(b"CG", b"S", [64, 64]), l_seq=9)
    add("cg_second_tag_ignored", [(S, 9), (N, 7)], tags=B.tag_B(b"CG", b"S", [64]) + b"CGBI" + struct.pack("<I", 3) + small.astype("<u4").tobytes(), l_seq=9)
    # the lengths no reference holds, on the one-base contig: the depth walk leaves such a contig alone (contig_on, which plays no part here), so
    # these CIGARs are read by this pass and by nothing else
    hostile = [(M, 1)]
    for ln in HOSTILE:
        hostile += [(I, ln), (M, 1), (D, ln), (M, 1)]
    add("hostile_indels", hostile, tid=ONE)
    add("coop_max_m", [((M, MAXLEN), (I, 3), (M, MAXLEN), (D, 2))[k % 4] for k in range(200)], tid=ONE)
    coop = [(H, MAXLEN), (S, 4)] + [((EQ, 7), (X, 1), (I, HOSTILE[k % 6]), (9, 3), (D, HOSTILE[(k + 1) % 6]), (15, MAXLEN), (N, 50), (P, 1))[k % 8] for k in range(126)] + [(S, 0), (H, 1)]
    add("coop_every_class", coop, tid=ONE)
    add("coop_secondary", coop, flag=0x100, tid=ONE)
    add("unplaced_with_cigar", [(M, 30)], tid=-1)
    return out


def edges_file(d):
    """writes aln_edges.bam into directory d -> a file dict like bam_craft.build_corpus's, checked"""
    cases = edge_reads()
    path = os.path.join(str(d), "aln_edges.bam")
    blocks, inf, offs = B.write_bam(path, B.NAMES, B.LENS, [r for _, r in cases], member_size=3000, cg_tag=False)
    lens, recs = B.parse_bam(inf)
    assert lens == B.LENS and [r["off"] for r in recs] == offs
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=recs, data=open(path, "rb").read(), cases={c: offs[k] for k, (c, _) in enumerate(cases)})
    check_edges(f)
    return f


def _sums(c):
    ln = (c >> 4).astype(object)
    cls = np.minimum(c & 0xf, 9)
    b = [int(sum(ln[cls == k])) for k in range(10)]
    a = b[0] + b[1] + b[7] + b[8]
    return a, a + b[4] + b[5], b


def check_edges(f):
    """not vacuous, told from the parsed bytes (the issue's list)"""
    recs = f["recs"]
    cig = [cigar_of(r) for r in recs]
    assert LDS_BINS == lds_bins()
    codes = set(int(v) & 0xf for c in cig for v in c)
    assert {9, 15} <= codes
    assert any(c.size >= 3 and int(c[0]) & 0xf == H and int(c[-1]) & 0xf == H for c in cig)
    aligned = [(r, c) for r, c in zip(recs, cig) if r["tid"] >= 0 and not r["flag"] & 4 and c.size]
    assert any(set(int(v) & 0xf for v in c) == {H, P} and _sums(c)[1] > 0 and _sums(c)[0] == 0 for _, c in aligned)
    assert any(set(int(v) & 0xf for v in c) == {D} and _sums(c)[1] == 0 for _, c in aligned)
    for op in (I, D):
        assert set(HOSTILE) <= set(int(v) >> 4 for c in cig for v in c if int(v) & 0xf == op)
    coop = B.walk_geometry()[2]
    assert any(c.size == 200 >= coop and all(int(v) >> 4 == MAXLEN for v in c if int(v) & 0xf == M) and sum(1 for v in c if int(v) & 0xf == M) == 100 for c in cig)
    assert any(c.size >= coop and set(int(v) & 0xf for v in c) >= {H, S, EQ, X, I, D, N, P, 9, 15} for c in cig)
    lengths = {_sums(c)[1] for r, c in aligned if not r["flag"] & 0x900}
    for w in WIDTHS:
        assert {3 * w - 1, 3 * w, (LEN_BINS - 1) * w - 1, (LEN_BINS - 1) * w, (LEN_BINS - 1) * w + 1, LDS_BINS * w - 1, LDS_BINS * w} <= lengths or w == 1, w
    assert {8190, 8191, 8192, 99, 100, LDS_BINS - 1, LDS_BINS} <= lengths
    assert any(_sums(c)[1] // 100 >= LDS_BINS > _sums(c)[0] // 100 for _, c in aligned)
    flags = [r["flag"] for r in recs]
    assert any(fl & 0x100 for fl in flags) and any(fl & 0x800 for fl in flags)
    assert any(r["flag"] & 4 and r["cigar"].size for r in recs) and any(r["tid"] < 0 and r["cigar"].size for r in recs)
    dropped = [r for r in recs if any(t[0] == b"CG" for t in r["tags"]) and all(r["flag"] & x or r["mapq"] < q for x, q in B.FILTERS)]
    assert dropped and all(cigar_of(r).size > r["cigar"].size for r in dropped)
    kept_cg = [r for r in recs if any(t[0] == b"CG" for t in r["tags"]) and not r["flag"] & 1796 and r["mapq"] >= 20]
    assert any(cigar_of(r).size >= coop for r in kept_cg) and any(r["cigar"].size < cigar_of(r).size < coop for r in kept_cg)
    assert sum(1 for r in kept_cg if cigar_of(r) is r["cigar"]) >= 3                    # placeholders that stay: too short, wrong type, a second tag
    for x, q in B.FILTERS:
        s = Model(len(f["lens"]), x, q, 1).add_parsed(recs).array()
        assert s[RECORDS] == len(recs) > s[ALIGNED] > s[PRIMARY] > 0 and 0 < s[CLIPPED] < s[ALIGNED]
        assert s[INS:INS + INDEL_BINS + 1].sum() == s[OPS + 2 * I] and s[DEL:DEL + INDEL_BINS + 1].sum() == s[OPS + 2 * D]
        assert s[AF] > 0 and s[AF + 100] > 0 and s[RL + 2 * (LEN_BINS - 1)] > 0 and int(s[READ_MAX]) > 1 << 34


def session_cuts(f):
    """{label: batches} for the decode-session tests: bam_craft's 1 / 3 / 16 batches of two units, and one unit to a batch cut at every fourth record"""
    out = {k: v for k, v in B.session_cuts(f, "aln_edges").items() if k != "guess"}
    out["crafted"] = B.cut_batches(f, f["offs"][4::4], 1)
    return out
