"""-gcbias in numpy: depth by GC content of fixed windows, and the text of <prefix>.gcbias.stat.gz.

Cells are given per contig; a span (tid, b, e) — cells [b, e), 0-based — is tiled from b by windows of exactly W cells, and what is
left over belongs to no window.  After `| 0x20` the bytes c / g are GC and a / t are AT; every other byte, and every cell the
contig's bases do not reach, is invalid, and a window with an invalid cell is skipped.  A counted window with g GC cells goes to
bin (200 g + W) // (2 W)."""
import numpy as np

BINS = 101
HEADER = "#GC\tWindows\tTotalDepth\tMeanDepth\tNormalized\n"


def as_bytes(b):
    if b is None:
        return np.zeros(0, dtype=np.uint8)
    if isinstance(b, (bytes, bytearray)):
        return np.frombuffer(bytes(b), dtype=np.uint8)
    return np.asarray(b, dtype=np.uint8)


def whole_contigs(lens, tids=None):
    return [(t, 0, int(lens[t])) for t in (range(len(lens)) if tids is None else tids)]


def spans_of_regions(regs, lens):
    """(tid, first, second) rows as pd_region has them -> cells [first - 1, second) clipped to the contig"""
    out = []
    for t, f, s in regs:
        b, e = max(int(f) - 1, 0), min(int(s), int(lens[t]))
        if b < e:
            out.append((int(t), b, e))
    return out


def merged_spans(entries, lens):
    """{tid: [(start, end), ...]} 1-based inclusive entries -> the sorted union per contig; overlapping and touching entries
    become one span, and the tiling restarts at each"""
    out = []
    for t in sorted(entries):
        sp = sorted((max(s - 1, 0), min(e, int(lens[t]))) for s, e in entries[t])
        sp = [(b, e) for b, e in sp if b < e]
        if not sp:
            continue
        cb, ce = sp[0]
        for b, e in sp[1:]:
            if b <= ce:
                ce = max(ce, e)
            else:
                out.append((t, cb, ce))
                cb, ce = b, e
        out.append((t, cb, ce))
    return out


def gc_bias(depth, bases, spans, W):
    """depth: one uint32 array per contig; bases: one bytes-like or None per contig -> (windows uint64[101], sum uint64[101], skipped)"""
    W = int(W)
    windows = np.zeros(BINS, dtype=np.uint64)
    total = np.zeros(BINS, dtype=np.uint64)
    skipped = 0
    for t, b, e in spans:
        nw = (e - b) // W
        if nw == 0:
            continue
        n = nw * W
        d = np.asarray(depth[t][b:b + n], dtype=np.uint64).reshape(nw, W).sum(axis=1, dtype=np.uint64)
        have = as_bytes(bases[t])[b:b + n]
        seq = np.zeros(n, dtype=np.uint8)
        seq[:have.size] = have
        y = seq | 0x20
        gc = (y == ord("c")) | (y == ord("g"))
        valid = gc | (y == ord("a")) | (y == ord("t"))
        ok = valid.reshape(nw, W).all(axis=1)
        g = gc.reshape(nw, W).sum(axis=1, dtype=np.int64)
        bins = (200 * g + W) // (2 * W)
        skipped += int(nw - ok.sum())
        np.add.at(windows, bins[ok], np.uint64(1))
        np.add.at(total, bins[ok], d[ok])
    return windows, total, skipped


def text(W, windows, total, skipped):
    W = int(W)
    n = int(sum(int(x) for x in windows))
    tot = int(sum(int(x) for x in total))
    mean_all = float(tot) / float(n * W) if n else 0.0
    out = [HEADER]
    for b in range(BINS):
        w, s = int(windows[b]), int(total[b])
        if not w:
            out.append("%d\t%d\t%d\tNA\tNA\n" % (b, w, s))
            continue
        mean = float(s) / float(w * W)
        out.append("%d\t%d\t%d\t%.2f\t%s\n" % (b, w, s, mean, "%.4f" % (mean / mean_all) if tot else "NA"))
    out.append("##WindowSize: %d\tWindows: %d\tSkipped: %d\tMeanDepth: %s\n" % (W, n, skipped, "%.2f" % mean_all if n else "NA"))
    return "".join(out)
