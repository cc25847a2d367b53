"""Crafted-record BAM files for the tests of the device record walk (pandepth_amd/csrc/pd_bamwalk.h), and a reference for their depth.

Three independent parts (a helper module, not a conftest):
  * a WRITER: BGZF BAM from a Python list of records (tid, pos, flag, mapq, name, cigar_ops, l_seq, tags) through zlib, with the
    member size as an option (records then straddle members) and htslib's storage of CIGARs above 65 535 operations
    (<l_seq>S<reflen>N in the record, the real CIGAR in CG:B,I) as another; it returns the members' table in the form
    test_gpu_bgzf.scan_bgzf yields;
  * a REFERENCE written from the SAM specification (§4.2 record layout, §4.2.2 the CG tag, §1.4 the CIGAR operations), which parses
    the inflated bytes itself and adds 1 over every M/=/X run of every kept record, clipped to the contig — plain numpy, nothing of
    the product's walk;
  * the CORPUS of tests/test_bamwalk_edges.py and tests/test_gpu_bamwalk_edges.py: every CIGAR and layout edge of the walk by
    construction, with a census (taken from the record offsets alone) that says which edges a file and a split into units hold.
"""
import os
import re
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

M, I, D, N, S, H, P, EQ, X = range(9)
_REF_OPS = (M, D, N, EQ, X)          # consume reference
_QRY_OPS = (M, I, S, EQ, X)          # consume query
_RUN_OPS = (M, EQ, X)
_IS_REF, _IS_QRY, _IS_RUN = (np.array([k in ops for k in range(16)]) for ops in (_REF_OPS, _QRY_OPS, _RUN_OPS))     # by operation code


def walk_geometry():
    """(PD_WALK_SUB, SEG_BYTES, COOP_MIN) as pd_bamwalk.h defines them"""
    text = open(os.path.join(ROOT, "pandepth_amd", "csrc", "pd_bamwalk.h")).read()
    sub = int(re.search(r"#define\s+PD_WALK_SUB\s+(\d+)", text).group(1))
    lanes = int(re.search(r"SEG_BYTES\s*=\s*(\d+)\s*\*\s*SUB", text).group(1))
    coop = int(re.search(r"COOP_MIN\s*=\s*(\d+)", text).group(1))
    return sub, lanes * sub, coop


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------
def pack(ops):
    """[(op, len), ...] or a packed array -> packed uint32 (len << 4 | op)"""
    if isinstance(ops, np.ndarray):
        return ops.astype(np.uint32)
    return np.array([(ln << 4) | op for op, ln in ops], dtype=np.uint32)


def qlen(ops):
    c = pack(ops)
    return int((c[_IS_QRY[c & 0xf]] >> 4).sum(dtype=np.int64))


def rlen(ops):
    c = pack(ops)
    return int((c[_IS_REF[c & 0xf]] >> 4).sum(dtype=np.int64))


def tag_Z(name, s, ty=b"Z"):
    return name + ty + s + b"\0"


def tag_A(name, ch):
    return name + b"A" + ch


def tag_i(name, v):
    return name + b"i" + struct.pack("<i", v)


def tag_B(name, sub, values):
    fmt = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I", b"f": "f"}[sub]
    values = list(values)
    return name + b"B" + sub + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values)


def _reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def encode_record(rec, cg_tag=True):
    """one record's bytes, block_size included"""
    tid, pos, flag, mapq, name, ops, l_seq, tags = rec
    cig = pack(ops)
    tags = tags or b""
    ref = rlen(cig)
    if cg_tag and cig.size > 65535:
        tags = tags + b"CGBI" + struct.pack("<I", cig.size) + cig.astype("<u4").tobytes()
        cig = pack([(S, l_seq), (N, ref)])
    assert cig.size <= 65535 and len(name) <= 254
    end = pos + (ref if ref and not flag & 4 else 1)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, _reg2bin(max(pos, 0), max(end, 1)) if tid >= 0 else 4680, cig.size, flag, l_seq, -1, -1, 0)
    body += name + b"\0" + cig.astype("<u4").tobytes() + b"\x11" * ((l_seq + 1) // 2) + b"\x1e" * l_seq + tags
    return struct.pack("<i", len(body)) + body


def header_bytes(names, lens):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(names, lens))
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(names))
    for n, l in zip(names, lens):
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return out


def bgzf(inflated, member_size=0xff00, level=1):
    """-> file bytes, blocks [(in_off, out_off, in_len, out_len)] (the EOF member included, as scan_bgzf reports it)"""
    assert 0 < member_size <= 0xff00
    out, blocks = bytearray(), []
    for uo in list(range(0, len(inflated), member_size)) + [len(inflated)]:
        piece = inflated[uo:uo + member_size] if uo < len(inflated) else b""
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = z.compress(piece) + z.flush()
        bsize = 18 + len(comp) + 8
        assert bsize <= 65536
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1)
        blocks.append((len(out), uo, len(comp), len(piece)))
        out += comp + struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece))
    return bytes(out), blocks


def write_bam(path, names, lens, records, member_size=0xff00, cg_tag=True, level=1):
    """-> blocks, inflated bytes, record offsets"""
    parts, offs, o = [header_bytes(names, lens)], [], 0
    o = len(parts[0])
    for rec in records:
        b = rec if isinstance(rec, (bytes, bytearray)) else encode_record(rec, cg_tag)
        offs.append(o); parts.append(b); o += len(b)
    inf = b"".join(parts)
    data, blocks = bgzf(inf, member_size, level)
    with open(path, "wb") as f:
        f.write(data)
    return blocks, inf, offs


# ---------------------------------------------------------------------------------------------------------------------
# units (rows of pd_push_bgzf_units: start, stop, avail, first_block, n_blocks)
# ---------------------------------------------------------------------------------------------------------------------
def units_from_stops(blocks, offs, total, stops):
    """Units [start, stop): unit k starts at the first record at or behind the previous stop and owns the records that START before
    its stop, wherever that lies; its bytes (avail) are the members up to the one that holds its last record's last byte."""
    offs = np.asarray(offs, dtype=np.int64)
    ends = np.append(offs[1:], total)
    bstart = np.array([b[1] for b in blocks], dtype=np.int64)
    bend = np.array([b[1] + b[3] for b in blocks], dtype=np.int64)
    units, at = [], 0
    for stop in list(stops) + [total]:
        if at >= len(offs):
            break
        stop = min(int(stop), total)
        last = int(np.searchsorted(offs, stop, side="left")) - 1          # the last record that starts before stop
        if last < at:
            continue
        start = int(offs[at])
        fb = int(np.searchsorted(bend, start, side="right"))
        lb = int(np.searchsorted(bstart, ends[last] - 1, side="right")) - 1
        units.append((start, stop, int(bend[lb]), fb, lb - fb + 1))
        at = last + 1
    return units


def split_units(blocks, offs, total, n_units):
    """n_units of (nearly) as many records each, cut at record starts"""
    return units_from_stops(blocks, offs, total, [offs[(len(offs) * k) // n_units] for k in range(1, n_units)])


# ---------------------------------------------------------------------------------------------------------------------
# batches (pd_decode_submit / pd_decode_queue: whole members, tables in the batch's own coordinates)
# ---------------------------------------------------------------------------------------------------------------------
def member_spans(f):
    """file offsets [begin, end) of every BGZF member of a corpus file (header and trailer included)"""
    ends = [b[0] + b[2] + 8 for b in f["blocks"]]
    return list(zip([0] + ends[:-1], ends))


def unit_at(f, start, stop, flags=0):
    """The unit [start, stop) of a corpus file in FILE coordinates, for any start: (start, stop, avail, first_block, n_blocks, flags).
    It owns the records that start in [start, stop); its members run from the one that holds `start` to the one that holds the last
    byte of its last record (of `stop - 1` when it owns none)."""
    offs = np.asarray(f["offs"], dtype=np.int64)
    total = len(f["inf"])
    ends = np.append(offs[1:], total)
    bstart = np.array([b[1] for b in f["blocks"]], dtype=np.int64)
    bend = np.array([b[1] + b[3] for b in f["blocks"]], dtype=np.int64)
    stop = min(int(stop), total)
    lo, hi = int(np.searchsorted(offs, start, side="left")), int(np.searchsorted(offs, stop, side="left"))
    last_byte = int(ends[hi - 1]) - 1 if hi > lo else max(stop - 1, start)
    fb = int(np.searchsorted(bend, start, side="right"))
    lb = int(np.searchsorted(bstart, last_byte, side="right")) - 1
    return (int(start), stop, int(bend[lb]), fb, lb - fb + 1, int(flags))


def batch_of_units(f, units, order=0):
    """One batch from units in FILE coordinates (rows of units_from_stops / unit_at), the way the executable's readers build theirs
    (host/pipeline.cpp): the whole members from the first unit's first to the last one any unit needs, in_off pointing at the deflate
    payload inside the batch's own bytes, out_off restarting at 0, the units' start / stop / avail in the batch's inflated space and
    first_block counted from the batch's first member.
    -> dict(data, blocks, units, inflated, order — what DecodeSession takes — and base: the file's inflated offset of the batch's byte
    0, members: (first, last) member of the file, units_file)"""
    span = member_spans(f)
    m0 = min(u[3] for u in units)
    m1 = max(u[3] + u[4] - 1 for u in units)
    f0 = span[m0][0]
    base = f["blocks"][m0][1]
    blocks = [(b[0] - f0, b[1] - base, b[2], b[3]) for b in f["blocks"][m0:m1 + 1]]
    inflated = f["blocks"][m1][1] + f["blocks"][m1][3] - base
    rows = [(u[0] - base, u[1] - base, u[2] - base, u[3] - m0, u[4], u[5] if len(u) > 5 else 0) for u in units]
    for r in rows:
        assert 0 <= r[0] <= r[2] <= inflated and r[3] + r[4] <= len(blocks), r
    return dict(data=f["data"][f0:span[m1][1]], blocks=blocks, units=rows, inflated=inflated, order=order, base=base, members=(m0, m1),
                units_file=[tuple(u) for u in units])


def cut_batches(f, stops, units_per_batch, guess=False):
    """A corpus file as the batches of a decode session: the units of units_from_stops(stops), units_per_batch to a batch, orders
    0, 1, ... in file order.  Neighbouring batches share the members their edge records straddle.
    guess: the no-index form — the stops are moved down to member starts, and every batch is ONE unit that begins at its member's first
    byte with PD_UNIT_GUESS (batch 0 at the first record, without the flag) and ends where the next one begins; stops that would leave
    a unit without a record are dropped."""
    total = len(f["inf"])
    if not guess:
        units = units_from_stops(f["blocks"], f["offs"], total, stops)
        return [batch_of_units(f, units[k:k + units_per_batch], k // units_per_batch) for k in range(0, len(units), units_per_batch)]
    assert units_per_batch == 1
    offs = np.asarray(f["offs"], dtype=np.int64)
    bstart = np.array([b[1] for b in f["blocks"]], dtype=np.int64)
    cuts, prev = [], int(offs[0])
    for s in sorted(set(int(bstart[np.searchsorted(bstart, s, side="right") - 1]) for s in stops)) + [total]:
        if s > prev and np.searchsorted(offs, s, side="left") > np.searchsorted(offs, prev, side="left"):
            cuts.append((prev, s)); prev = s
    return [batch_of_units(f, [unit_at(f, a, b, 0 if k == 0 else 1)], k) for k, (a, b) in enumerate(cuts)]


def session_cuts(f, name):
    """{label: batches}: the cuts of a corpus file that the decode-session tests use — on the CPU (tests/test_decode_batches.py) and on
    the device (tests/test_gpu_decode_session.py) alike: 1, 3 and 16 batches of two units cut at record starts, the crafted stops of
    `layout` one unit to a batch, and the no-index form cut at eighths of the file ("guess")"""
    total, offs = len(f["inf"]), f["offs"]
    out = {}
    for nb in (1, 3, 16):
        out["%d" % nb] = cut_batches(f, [offs[(len(offs) * k) // (2 * nb)] for k in range(1, 2 * nb)], 2)
        assert len(out["%d" % nb]) == nb, (name, nb)
    if name == "layout":
        out["crafted"] = cut_batches(f, layout_crafted_stops(offs, walk_geometry()[1]), 1)
    out["guess"] = cut_batches(f, [total * k // 8 for k in range(1, 8)], 1, guess=True)
    return out


def long_decoy_file(d, seg):
    """A file of its own for guessed starts: ordinary reads, ONE record of more than two segments whose Z tag holds a decoy header
    (decoy_tag) one and a half segments into the record, ordinary reads again.
    -> the file (as build_corpus describes one), the long record's offset, the decoy's offset"""
    size, at = 2 * seg + 70000, seg + seg // 2
    recs = [_sized(150 + k, 100 + 9 * k, k) for k in range(20)]
    long_rec = bytearray(_sized(size, 400, 20, tag=b"XL"))
    s = decoy_tag()
    long_rec[at:at + len(s)] = s
    recs.append(bytes(long_rec))
    recs += [_sized(150 + k % 40, 500 + 9 * k, k) for k in range(21, 400)]
    path = os.path.join(str(d), "long_decoy.bam")
    blocks, inf, offs = write_bam(path, NAMES, LENS, recs)
    lens, parsed = parse_bam(inf)
    assert [r["off"] for r in parsed] == offs and parsed[20]["size"] == size
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=parsed, data=open(path, "rb").read(), cases={})
    assert inf[offs[20] + at:offs[20] + at + len(s)] == s and inf.count(s) == 1
    return f, offs[20], offs[20] + at


def owners(f, batches):
    """how many units of `batches` own each record of the file (a record belongs to the unit in whose [start, stop) it starts)"""
    offs = np.asarray(f["offs"], dtype=np.int64)
    n = np.zeros(offs.size, dtype=np.int64)
    for b in batches:
        for (start, stop, avail, fb, nb, flags), (fs, fe, fa) in zip(b["units"], [u[:3] for u in b["units_file"]]):
            assert (start + b["base"], stop + b["base"], avail + b["base"]) == (fs, fe, fa)
            mine = (offs >= fs) & (offs < fe)
            n += mine
    return n


def census(offs, total, units, sub, seg):
    """Where the records of a file lie against the lanes, segments and units of a split — from the offsets alone.
    -> dict: lane_end / seg_end / unit_end: sets of distances (<= 64) from a record start to the end of its lane's stretch / its
    segment / its unit; empty_lanes / empty_segs: stretches and segments (inside a unit's range) in which no record starts;
    stop_mod_seg: (stop - start) % seg of every unit; recs_per_unit."""
    offs = np.asarray(offs, dtype=np.int64)
    out = dict(lane_end=set(), seg_end=set(), unit_end=set(), empty_lanes=0, empty_segs=0, stop_mod_seg=set(), recs_per_unit=[], longest=0)
    ends = np.append(offs[1:], total)
    out["longest"] = int((ends - offs).max())
    for start, stop, avail, fb, nb in units:
        mine = offs[(offs >= start) & (offs < stop)]
        assert mine.size and mine[0] == start and ends[np.searchsorted(offs, mine[-1])] <= avail
        out["recs_per_unit"].append(int(mine.size))
        out["stop_mod_seg"].add((stop - start) % seg)
        rel = mine - start
        seg_i = rel // seg
        seg_stop = np.minimum((seg_i + 1) * seg, stop - start)
        lane_stop = np.minimum((rel // sub + 1) * sub, seg_stop)
        out["lane_end"] |= set(int(d) for d in (lane_stop - rel) if d <= 64)
        out["seg_end"] |= set(int(d) for d in (seg_stop - rel) if d <= 64)
        out["unit_end"] |= set(int(d) for d in (stop - start - rel) if d <= 64)
        n_lanes = -(-(stop - start) // sub)
        out["empty_lanes"] += int(n_lanes - np.unique(rel // sub).size)
        out["empty_segs"] += int(-(-(stop - start) // seg) - np.unique(seg_i).size)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference (SAM specification)
# ---------------------------------------------------------------------------------------------------------------------
_TAG_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def parse_bam(inf):
    """-> contig lengths, records [dict(off, size, tid, pos, flag, mapq, l_seq, cigar (packed uint32, the record's own), tags [(name, type, value)])]"""
    assert inf[:4] == b"BAM\x01"
    o = 8 + struct.unpack_from("<i", inf, 4)[0]
    n_ref = struct.unpack_from("<i", inf, o)[0]; o += 4
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", inf, o)[0]
        lens.append(struct.unpack_from("<i", inf, o + 4 + l_name)[0]); o += 8 + l_name
    recs = []
    while o < len(inf):
        bs, tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", inf, o)
        end = o + 4 + bs
        c = o + 36 + l_rn
        assert inf[c - 1] == 0 and end <= len(inf)
        cigar = np.frombuffer(inf, dtype="<u4", count=n_cig, offset=c).astype(np.uint32)
        a = c + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        tags = []
        while a < end:
            name, ty = inf[a:a + 2], inf[a + 2:a + 3]; a += 3
            if ty in _TAG_SIZE:
                val = inf[a:a + _TAG_SIZE[ty]]; a += _TAG_SIZE[ty]
            elif ty in (b"Z", b"H"):
                z = inf.index(b"\0", a); val = inf[a:z]; a = z + 1
            else:
                assert ty == b"B"
                sub = inf[a:a + 1]; cnt = struct.unpack_from("<I", inf, a + 1)[0]
                size = _TAG_SIZE[sub] * cnt
                val = (sub, np.frombuffer(inf, dtype={1: "<u1", 2: "<u2", 4: "<u4"}[_TAG_SIZE[sub]], count=cnt, offset=a + 5)); a += 5 + size
            tags.append((name, ty, val))
        assert a == end
        recs.append(dict(off=o, size=4 + bs, tid=tid, pos=pos, flag=flag, mapq=mapq, l_seq=l_seq, cigar=cigar, tags=tags))
        o = end
    return lens, recs


def real_cigar(r):
    """SAM §4.2.2: a CIGAR of more than 65 535 operations is stored in the CG:B,I tag and the record holds kSmN (k = l_seq,
    m = the reference length) in its place; anything else is the CIGAR itself."""
    c = r["cigar"]
    if c.size == 2 and int(c[0]) == ((r["l_seq"] << 4) | S) and int(c[1]) & 0xf == N and r["tid"] >= 0 and r["pos"] >= 0:
        for name, ty, val in r["tags"]:
            if name == b"CG":
                if ty == b"B" and val[0] == b"I":
                    return val[1].astype(np.uint32)
                break
    return c


def kept(r, n_ref, flag_mask, min_mapq):
    return not (r["flag"] & flag_mask) and r["mapq"] >= min_mapq and 0 <= r["tid"] < n_ref


def runs_of(r):
    """(begin, end) arrays of the M/=/X runs of a record, unclipped"""
    c = real_cigar(r)
    op, ln = c & 0xf, (c >> 4).astype(np.int64)
    adv = np.where(_IS_REF[op], ln, 0)
    beg = r["pos"] + np.cumsum(adv) - adv
    run = _IS_RUN[op]
    return beg[run], beg[run] + ln[run]


def reference_depth(lens, recs, flag_mask, min_mapq):
    """-> per-contig uint32 depth (None for contigs shorter than 2, which the program skips), kept records, their runs"""
    diff = [np.zeros(l + 1, dtype=np.int64) if l >= 2 else None for l in lens]
    n_kept = n_runs = 0
    for r in recs:
        if not kept(r, len(lens), flag_mask, min_mapq) or diff[r["tid"]] is None:
            continue
        n_kept += 1
        L = lens[r["tid"]]
        b, e = runs_of(r)
        n_runs += b.size
        np.add.at(diff[r["tid"]], np.clip(b, 0, L), 1)
        np.add.at(diff[r["tid"]], np.clip(e, 0, L), -1)
    return [None if d is None else np.cumsum(d[:-1]).astype(np.uint32) for d in diff], n_kept, n_runs


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["big", "small", "one", "mid"]
LENS = [400000, 5000, 1, 70000]
OP_COUNTS = [1, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 4096, 65535]
EDGE_DISTS = (1, 4, 35, 36, 37)
FILTERS = [(1796, -1), (0, 20)]


def _mixed(n, rng):
    """n operations, M I M D M I ... with small lengths; an even count ends in a soft clip"""
    op = np.tile(np.array([M, I, M, D], dtype=np.uint32), n // 4 + 1)[:n]
    ln = np.where(op == M, rng.integers(1, 4, n), np.where(op == I, 1, rng.integers(1, 3, n))).astype(np.uint32)
    if n > 1 and op[-1] != M:
        op[-1] = S; ln[-1] = 3
    if n == 1:
        ln[0] = 30
    return (ln << 4) | op


def _lead(n_lead):
    """n_lead operations that consume no reference: H, S, then I and P taking turns"""
    ops = [(H, 5), (S, 3)][:n_lead]
    while len(ops) < n_lead:
        ops.append((I, 1 + len(ops) % 2) if len(ops) % 2 == 0 else (P, 1))
    return ops


def _tail(n, first=I):
    """n operations behind a run: I M I M ... (or D M D M ...)"""
    return [((first if k % 2 == 0 else M), 1 + k % 3) for k in range(n)]


def special_reads(rng):
    """-> [(case name, record)]: every CIGAR edge as one read (unsorted; the files sort them)"""
    out = []

    def add(case, tid, pos, ops, flag=0, mapq=60, tags=b"", l_seq=None):
        c = pack(ops)
        out.append((case, (tid, pos, flag, mapq, case.encode(), c, qlen(c) if l_seq is None else l_seq, tags)))

    for k, n in enumerate(OP_COUNTS):
        add("ops%d" % n, 0, 2000 + 700 * k, _mixed(n, rng), flag=16 * (k % 2))
        if n <= 4096:       # the same count once more with a flag or a mapq that one of the two filter settings drops
            add("ops%d_drop" % n, 0, 2100 + 700 * k, _mixed(n, rng), flag=1024 if k % 2 else 0, mapq=60 if k % 2 else 5)
    for i in (0, 63, 64, 65):
        add("first_at%d" % i, 0, 20000 + 100 * i, _lead(i) + [(M, 50)] + _tail(max(100, i + 40) - i - 1))
    # the first run behind a D / N: it belongs to the stream of later runs.  (run at, gap op, gap at)
    for at, gop, gat in ((63, D, 5), (64, N, 63), (64, D, 10), (65, D, 10), (65, D, 64), (65, N, 64), (130, N, 70), (130, D, 129), (130, D, 3)):
        ops = _lead(at)
        ops[gat] = (gop, 7)
        add("first_at%d_behind_%s%d" % (at, "MIDN"[gop], gat), 0, 30000 + 40 * at + gat, ops + [(M, 50)] + _tail(max(100, at + 40) - at - 1))
    add("no_run_120", 0, 40000, [(S, 4)] + [((I, 1), (D, 3), (P, 1), (N, 11))[k % 4] for k in range(119)])
    add("no_run_3", 0, 40100, [(S, 4), (I, 2), (D, 9)])
    add("no_reference_bases_100", 0, 40200, [(S, 4)] + [((I, 1), (P, 1))[k % 2] for k in range(99)])
    add("only_run_last_behind_gaps", 0, 41000, [(S, 4)] + [((I, 1), (D, 2), (P, 1))[k % 3] for k in range(98)] + [(M, 40)])
    add("only_run_last_first", 0, 41500, _lead(99) + [(M, 40)])
    add("zero_len_runs", 0, 42000, [(M, 0), (M, 10), (I, 1), (M, 0), (D, 2), (M, 0), (M, 5)])
    add("zero_len_runs_100", 0, 42100, [(M, 0)] + [((I, 1), (M, 0), (D, 1), (M, 2))[k % 4] for k in range(99)])
    add("zero_len_first_behind_lead", 0, 42200, _lead(64) + [(M, 0)] + _tail(60, D))
    add("eq_x", 0, 43000, [(EQ, 20), (X, 1), (EQ, 30), (I, 2), (X, 3), (EQ, 10)])
    add("eq_x_128", 0, 43100, [((EQ, 4), (X, 1), (I, 1), (EQ, 2), (D, 1))[k % 5] for k in range(128)])
    add("gap_200k", 0, 150000, [(M, 50), (N, 200000), (M, 60)])
    add("gap_200k_100", 0, 150100, _tail(49, I) + [(M, 3), (N, 200000)] + _tail(49, D) + [(M, 9)])
    add("past_end", 3, LENS[3] - 50, [(M, 100)])
    add("past_end_100", 3, LENS[3] - 100, _tail(99, D) + [(M, 20)])
    add("pos0", 0, 0, [(M, 75)])
    add("pos0_small", 1, 0, [(S, 5), (M, 70)], flag=16)
    add("pos0_97", 0, 0, _mixed(97, rng))
    add("ends_at_len_small", 1, LENS[1] - 100, [(M, 100)])
    add("ends_at_len_big", 0, LENS[0] - 100, [(M, 40), (D, 10), (M, 50)])
    add("ends_at_len_96", 0, LENS[0] - 96 * 2, [(M, 1), (D, 1)] * 95 + [(M, 1), (EQ, 1)])
    add("no_cigar_placed", 0, 5000, [], l_seq=50)
    add("no_cigar_placed_q5", 0, 5001, [], l_seq=50, mapq=5)
    add("unmapped_placed", 0, 6000, [], flag=4 | 1, mapq=0, l_seq=50)
    add("unmapped_placed_q30", 0, 6001, [], flag=4, mapq=30, l_seq=50)
    add("unmapped_placed_with_cigar", 0, 6002, _mixed(100, rng), flag=4, mapq=30)
    for k in range(3):
        add("unplaced%d" % k, -1, -1, [], flag=4, mapq=(0, 30, 60)[k], l_seq=40)
    add("one_base_contig", 2, 0, [(M, 1)])
    add("one_base_contig_clip", 2, 0, [(S, 10), (M, 1), (S, 100)], mapq=30)
    add("one_base_contig_97", 2, 0, _mixed(97, rng))
    # CIGARs in the CG tag
    add("cg65536", 0, 50000, _mixed(65536, rng))
    add("cg70000", 0, 60000, _mixed(70001, rng), flag=16)
    real = _mixed(65601, rng)
    before = (tag_Z(b"XZ", b"text") + tag_Z(b"XH", b"1AE301", b"H") + tag_B(b"Xc", b"c", [-1, 2, -3]) + tag_B(b"Xs", b"s", [-300, 300]) +
              tag_B(b"Xf", b"f", [1.5, -2.0]) + tag_A(b"XA", b"q") + tag_i(b"Xi", -77))
    add("cg_not_first_tag", 0, 70000, [(S, qlen(real)), (N, rlen(real))], l_seq=qlen(real),
        tags=before + tag_B(b"CG", b"I", real.tolist()) + tag_i(b"NM", 3))
    add("placeholder_without_cg", 0, 80000, [(S, 100), (N, 5000)], l_seq=100, tags=tag_i(b"NM", 0))
    add("placeholder_cg_BS", 0, 80100, [(S, 100), (N, 5000)], l_seq=100, tags=tag_B(b"CG", b"S", [(50 << 4) | M, (50 << 4) | M] * 50))
    add("placeholder_cg_dropped", 0, 80200, _mixed(65537, rng), flag=1024, mapq=5)
    return out


def _sort_key(rec):
    return (rec[0] & 0xffffffff, rec[1])


def short_reads(rng, n):
    out = []
    for k in range(n):
        tid = int(rng.choice([0, 0, 0, 0, 1, 3, 3]))
        pos = int(rng.integers(0, LENS[tid] - 100))
        flag = int(rng.choice([0, 16, 0, 16, 1024, 256, 4 if k % 50 == 0 else 0]))
        out.append((tid, pos, flag, int(rng.choice([0, 19, 20, 30, 60])), b"s%05d" % k, pack([(M, 100)]), 100, b""))
    return out


def _sized(size, pos, k, name=None, tag=b"XP"):
    """an ordinary read (50M) of exactly `size` bytes, block_size included: its name and a Z tag take up the slack"""
    name = b"r" if name is None else name
    base = 4 + 32 + len(name) + 1 + 4 + 25 + 50
    pad = size - base
    assert pad >= 0, (size, base)
    if 0 < pad < 4:
        name += b"n" * pad; pad = 0
    tags = tag_Z(tag, bytes(97 + (j * 7 + k) % 26 for j in range(pad - 4))) if pad else b""
    rec = encode_record((0, pos, (0, 16, 1024, 0)[k % 4], (60, 30, 60, 10)[k % 4], name, pack([(M, 50)]), 50, tags))
    assert len(rec) == size
    return rec


def decoy_tag(l_name=9):
    """The bytes of a Z tag that pass for a record header (SAM §4.2): no NUL inside (it is a string), so every dword field
    is a value whose four bytes are non-zero — block_size 0x07010101 (117 MB: "the record runs past the bytes"), refID and next
    refID -1, pos and next pos 0x01010101, l_seq 0x01010101 — and the string's terminator is the NUL where the name would end."""
    hdr = struct.pack("<iiiBBHHHiiii", 0x07010101, -1, 0x01010101, l_name, 0x21, 0x1249, 0x0101, 0x0101, 0x01010101, -1, 0x01010101, 0x01010101)
    s = hdr + b"d" * (l_name - 1)
    assert b"\0" not in s and len(s) == 36 + l_name - 1
    return s


def layout_records(rng, sub, seg):
    """Records (encoded) of the layout file: with ONE unit over the whole file (lanes and segments counted from the first record) a
    record starts 1, 4, 35, 36, 37 bytes before the end of a lane's stretch and of a segment, a 5 000-byte record covers a whole
    stretch, a 300 000-byte record a whole segment, and two Z tags that look like record headers sit at the first bytes of a lane's
    stretch and of a segment."""
    r0 = len(header_bytes(NAMES, LENS))
    recs, o = [], r0
    pos = [0]

    def put(size, **kw):
        nonlocal o
        pos[0] += 9
        recs.append(_sized(size, pos[0], len(recs), **kw)); o += size

    def fill_to(target):
        while target - o > 500:
            put(int(rng.integers(121, 240)))
        gap = target - o
        assert gap == 0 or gap >= 242, gap
        if gap >= 242:
            put(gap // 2)
        if target - o:
            put(target - o)
        assert o == target

    def decoy_at(boundary):
        # record header 36 + name "r\0" + one operation + 75 bytes of bases = 117, the tag's "XDZ" = 120: the string begins at the boundary
        fill_to(boundary - 120)
        s = decoy_tag()
        put(120 + len(s) + 1 + 4 + 20, tag=b"XD")
        # (put() pads with lower-case letters: plant the decoy at the head of the string)
        rec = bytearray(recs[-1])
        rec[120:120 + len(s)] = s
        rec[120 + len(s)] = 0
        rec[120 + len(s) + 1:] = tag_Z(b"XQ", b"q" * 20)
        recs[-1] = bytes(rec)
        assert recs[-1][117:120] == b"XDZ" and len(recs[-1]) == 120 + len(s) + 25

    for k, d in enumerate(EDGE_DISTS):
        fill_to(r0 + (3 + 2 * k) * sub - d)
        put(150)
    fill_to(r0 + 20 * sub - 10)
    put(5000)
    put(116, name=b"")                     # l_read_name = 1: only the NUL
    put(4 + 32 + 255 + 4 + 75, name=b"N" * 254)
    decoy_at(r0 + 30 * sub)
    for k, d in enumerate(EDGE_DISTS):
        fill_to(r0 + (k + 1) * seg - d)
        put(150 + k)
    decoy_at(r0 + 6 * seg)
    fill_to(r0 + 7 * seg - 10)
    put(300000)
    fill_to(r0 + 9 * seg + 5 * sub + 77)
    return recs


def layout_crafted_stops(offs, seg):
    """stops of the crafted split of the layout file: units that end exactly on, one byte short of and one byte past a segment
    boundary (counted from their own start), one two segments long, and units whose last record starts 1, 4, 35, 36, 37 bytes
    before their stop"""
    offs = np.asarray(offs)
    stops, start = [], int(offs[0])
    for length in (seg, seg - 1, seg + 1, 2 * seg):
        stops.append(start + length)
        start = int(offs[np.searchsorted(offs, stops[-1], side="left")])
    at = int(np.searchsorted(offs, start))
    for d in EDGE_DISTS:
        at += 150
        stops.append(int(offs[at]) + d)
        at += 1
    return stops


def build_corpus(d):
    """Writes the corpus into directory d.  -> {name: dict(path, blocks, inf, offs, lens, recs (parsed back), cases {case: offsets})}"""
    sub, seg, coop = walk_geometry()
    rng = np.random.default_rng(20240607)
    files = {}

    def emit(name, records, member_size=0xff00, cases=None):
        path = os.path.join(str(d), name + ".bam")
        blocks, inf, offs = write_bam(path, NAMES, LENS, records, member_size)
        lens, recs = parse_bam(inf)
        assert lens == LENS and [r["off"] for r in recs] == offs
        files[name] = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=recs, data=open(path, "rb").read(),
                           cases={} if cases is None else {c: offs[k] for k, c in cases})
        return files[name]

    sp = special_reads(rng)
    order = sorted(range(len(sp)), key=lambda k: _sort_key(sp[k][1]))
    emit("alone", [sp[k][1] for k in order], cases=[(j, sp[k][0]) for j, k in enumerate(order)])
    # the same reads packed among ordinary short reads, members of 24 000 bytes
    sp2 = special_reads(rng)
    both = [(c, r) for c, r in sp2] + [(None, r) for r in short_reads(rng, 5000)]
    order = sorted(range(len(both)), key=lambda k: _sort_key(both[k][1]))
    emit("packed", [both[k][1] for k in order], member_size=24000, cases=[(j, both[k][0]) for j, k in enumerate(order) if both[k][0]])
    emit("layout", layout_records(rng, sub, seg), member_size=4093)
    # 64 records, for 64 units of one record each: a few of every kind
    few = [r for c, r in special_reads(rng) if r[5].size <= 200][:40] + short_reads(rng, 24)
    emit("few", sorted(few, key=_sort_key))
    # two adjacent records swapped out of coordinate order (the CLI's fall-back): short reads and the wave-walked reads
    mixed = sorted([r for c, r in special_reads(rng) if 90 <= r[5].size <= 4096 and r[0] == 0 and not r[2] & 4] + short_reads(rng, 3000), key=_sort_key)
    k = next(k for k in range(len(mixed) // 2, len(mixed) - 1) if mixed[k][0] == 0 and mixed[k + 1][0] == 0 and mixed[k + 1][1] > mixed[k][1] + 10)
    mixed[k], mixed[k + 1] = mixed[k + 1], mixed[k]
    emit("unsorted", mixed, member_size=30000)
    check_corpus(files, sub, seg, coop)
    return files


def splits_of(f, name, seg):
    """{split name: units} of a corpus file"""
    total = len(f["inf"])
    out = {"1": split_units(f["blocks"], f["offs"], total, 1), "3": split_units(f["blocks"], f["offs"], total, 3),
           "64": split_units(f["blocks"], f["offs"], total, 64)}
    if name == "layout":
        out["crafted"] = units_from_stops(f["blocks"], f["offs"], total, layout_crafted_stops(f["offs"], seg))
    return out


def check_corpus(files, sub, seg, coop):
    """Every named case is in the files — counted by the reference's own parse of the bytes, never by the code under test."""
    assert (sub, seg) == (4096, 262144) and coop == 96, "the corpus was laid out for these; look at the cases again when they change"
    for name in ("alone", "packed"):
        f = files[name]
        by_off = {r["off"]: r for r in f["recs"]}
        n_ops = lambda r: int(real_cigar(r).size)
        for mask, mq in FILTERS:
            special = set(f["cases"].values())                  # (the short reads between them are not what is counted here)
            keep = [r for r in f["recs"] if r["off"] in special and kept(r, len(LENS), mask, mq) and LENS[r["tid"]] >= 2]
            dropped_special = [c for c, o in f["cases"].items() if not kept(by_off[o], len(LENS), mask, mq)]
            assert len(dropped_special) >= 5, (name, mask, mq)
            counts = {n_ops(r) for r in keep}
            assert set(OP_COUNTS) <= counts and {65536, 70001, 65601} <= counts, (name, mask, mq, sorted(set(OP_COUNTS) - counts))
            # the first run at operation 0, 63, 64, 65 behind S / I / H / P only; and behind a D / N in an earlier and in the same step of 64
            for r in keep:
                c = real_cigar(r); r["_first_run"] = int(np.argmax(np.isin(c & 0xf, _RUN_OPS))) if np.isin(c & 0xf, _RUN_OPS).any() else -1
                gaps = np.flatnonzero(np.isin(c & 0xf, (D, N)))
                r["_gap_before"] = [int(g) for g in gaps if g < r["_first_run"]] if r["_first_run"] >= 0 else []
            big = [r for r in keep if n_ops(r) >= coop]
            assert {0, 63, 64, 65} <= {r["_first_run"] for r in big if not r["_gap_before"]}
            assert any(r["_gap_before"] and r["_gap_before"][-1] // 64 < r["_first_run"] // 64 for r in big)
            assert any(r["_gap_before"] and r["_gap_before"][-1] // 64 == r["_first_run"] // 64 and r["_first_run"] >= 64 for r in big)
            assert any(r["_first_run"] == -1 for r in big) and any(r["_first_run"] == n_ops(r) - 1 and n_ops(r) >= coop for r in big)
            assert any((real_cigar(r) >> 4)[np.isin(real_cigar(r) & 0xf, _RUN_OPS)].min(initial=1) == 0 for r in big)
            assert any(np.isin(real_cigar(r) & 0xf, (EQ, X)).any() for r in big)
            assert any(runs_of(r)[0].size and runs_of(r)[0].max() - r["pos"] >= 200000 for r in keep)
            assert any(runs_of(r)[1].size and runs_of(r)[1].max() > LENS[r["tid"]] for r in keep)
            assert any(runs_of(r)[1].size and runs_of(r)[1].max() == LENS[r["tid"]] for r in keep)
            assert any(r["pos"] == 0 for r in keep) and any(r["cigar"].size == 0 and not r["flag"] & 4 for r in keep)
        recs = f["recs"]
        assert any(r["flag"] & 4 and r["tid"] >= 0 for r in recs) and any(r["tid"] == -1 for r in recs) and any(r["tid"] == 2 for r in recs)
        cg = [r for r in recs if any(t[0] == b"CG" for t in r["tags"])]
        assert any(r["tags"][0][0] != b"CG" and real_cigar(r).size > 65535 for r in cg) and any(real_cigar(r).size == 2 for r in cg)
        assert any(r["cigar"].size == 2 and not r["tags"][0][0] == b"CG" and real_cigar(r) is r["cigar"] for r in recs if r["tags"])
        assert all(recs[k]["tid"] & 0xffffffff < recs[k + 1]["tid"] & 0xffffffff or (recs[k]["tid"] == recs[k + 1]["tid"] and recs[k]["pos"] <= recs[k + 1]["pos"])
                   for k in range(len(recs) - 1)), name + " is not coordinate-sorted"
    f = files["layout"]
    total = len(f["inf"])
    one = census(f["offs"], total, split_units(f["blocks"], f["offs"], total, 1), sub, seg)
    assert set(EDGE_DISTS) <= one["lane_end"] and set(EDGE_DISTS) <= one["seg_end"], one
    assert one["empty_lanes"] >= 1 and one["empty_segs"] >= 1 and one["longest"] >= 300000
    sizes = {r["size"] for r in f["recs"]}
    assert 5000 in sizes and 300000 in sizes
    names = {f["inf"][r["off"] + 12] for r in f["recs"]}
    assert 1 in names and 255 in names
    s = decoy_tag()
    at = [m.start() for m in re.finditer(re.escape(s), f["inf"])]
    assert len(at) == 2 and (at[0] - f["offs"][0]) % sub == 0 and (at[1] - f["offs"][0]) % seg == 0 and not set(at) & set(f["offs"])
    cr = census(f["offs"], total, units_from_stops(f["blocks"], f["offs"], total, layout_crafted_stops(f["offs"], seg)), sub, seg)
    assert set(EDGE_DISTS) <= cr["unit_end"] and {0, seg - 1, 1} <= cr["stop_mod_seg"], cr
    # members smaller than the records: records straddle members
    bend = np.array([b[1] + b[3] for b in f["blocks"]])
    assert np.any(np.searchsorted(bend, np.array(f["offs"][:-1]), side="right") != np.searchsorted(bend, np.array(f["offs"][1:]) - 1, side="right"))
    f = files["few"]
    assert len(f["offs"]) == 64 and census(f["offs"], len(f["inf"]), split_units(f["blocks"], f["offs"], len(f["inf"]), 64), sub, seg)["recs_per_unit"] == [1] * 64
    recs = files["unsorted"]["recs"]
    bad = [k for k in range(len(recs) - 1) if recs[k]["tid"] == recs[k + 1]["tid"] and recs[k]["pos"] > recs[k + 1]["pos"]]
    assert len(bad) == 1
