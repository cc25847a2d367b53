"""GPU parity tests of the threshold counts (pd_depth_thresholds / pd_window_thresholds, the -thresholds table): the HIP counting
kernels against numpy — (cells >= T).sum() — on the CPU oracle's depth (oracle/pd_oracle.c), exact for every row, in both launch
shapes (a group of lanes per row, pieces of 16384 cells added into the row) and across the row batches."""
import numpy as np
import pytest

import pandepth_amd as pda
from test_depth_quantiles_gpu import LENS, MULTI, REGIONS, WIDTHS, flat, oracle_depth, rand_intervals, sample

pytestmark = pytest.mark.gpu

PD_EINVAL, PD_ESTATE = -1, -4           # include/pandepth_amd.h
# 0, a value present in the data (1), the piece size's neighbours, the 300 000-read pile as an 18-bit cell (300000 - 2^18 = 37856)
# and as it is, the 18-bit limit, and a value above every cell
THR16 = [0, 1, 2, 5, 30, 500, 4095, 4096, 37856, 37857, 262143, 262144, 299999, 300000, 300001, 2 ** 31 - 1]
THRS = [[1], [0, 1, 5], THR16]
WAVE_MAX = [65536, 0, 0xFFFFFFFF]        # "threshold_wave_max": the default, every row in pieces, every row by a group of lanes


def counts_of(x, thr):
    s = np.sort(x)
    return x.size - np.searchsorted(s, np.asarray(thr, dtype=np.uint32), side="left")


def windows_ref(d, off, w, thr):
    out = []
    t32 = np.asarray(thr, dtype=np.uint32)
    for t, ln in enumerate(LENS):
        x = d[off[t]:off[t] + ln]
        full = ln // w
        if full:
            out.append((x[:full * w].reshape(full, w)[:, :, None] >= t32[None, None, :]).sum(axis=1) if w <= 64
                       else np.stack([np.add.reduceat((x[:full * w] >= v).astype(np.int64), np.arange(0, full * w, w)) for v in t32], axis=1))
        if ln % w:
            out.append(np.array([counts_of(x[full * w:], thr)]))
    return np.concatenate(out).astype(np.uint32)


def rows_ref(d, off, rows, thr):
    cells, cnt = [], []
    for segs in rows:
        parts = [d[off[t] + min(max(f - 1, 0), LENS[t]):off[t] + min(max(s, 0), LENS[t])] for t, f, s in segs]
        x = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        cells.append(x.size)
        cnt.append(counts_of(x, thr))
    return np.array(cells, dtype=np.uint64), np.array(cnt, dtype=np.uint64).reshape(len(rows), len(thr))


ROWS = ([[tuple(int(x) for x in r)] for r in REGIONS] + MULTI + [
    [tuple(int(x) for x in r) for r in REGIONS],             # all of them in one row: a multiset across contigs
    [(0, 19000, 21000), (0, 19000, 21000), (0, 20000, 20050)],       # a row that overlaps itself, over the pile
    [],                                                      # an empty row
    [(0, 4097, 4096 + 16384)],                               # exactly one piece, aligned
    [(0, 4097, 4096 + 16385)],                               # one cell more: a second piece of one cell
    [(0, 19999, 19998 + 16384)],                             # first cell 19998: not a multiple of 4, an unaligned head
    [(0, 20002, 20004)],                                     # three cells, all head
    [(0, 1, LENS[0])], [(1, 1, LENS[1])],                    # whole contigs
])


class Ctx:
    """one scanned engine and the oracle's depth per wrap, shared by the tests of this module; references computed once"""

    def __init__(self, wrap):
        self.wrap = wrap
        self.iv = sample(41 + wrap)
        self.d, self.off = oracle_depth(LENS, self.iv, wrap == 18)
        self.e = pda.Engine(LENS)
        self.e.push_intervals(self.iv, pda.PD_PUSH_DEFAULT)
        self.e.scan(wrap)
        self.win = {}
        self.rows = {}

    def windows(self, w):
        if w not in self.win:
            self.win[w] = windows_ref(self.d, self.off, w, THR16)
        return self.win[w]

    def row_ref(self):
        if not self.rows:
            self.rows["ref"] = rows_ref(self.d, self.off, ROWS, THR16)
        return self.rows["ref"]


@pytest.fixture(scope="module", params=[0, 18], ids=["wrap0", "wrap18"])
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.e.close()


def cols(thr):
    return [THR16.index(t) for t in thr]


def test_the_sample_reaches_the_thresholds(ctx):
    """what the sixteen values are there for: the pile is 300 000 deep in 32-bit cells and 37 856 in 18-bit ones"""
    pile = ctx.d[ctx.off[0] + 20000:ctx.off[0] + 20100]
    base = 37856 if ctx.wrap == 18 else 300000
    assert base <= int(pile.min()) and int(pile.max()) < base + 1000 and int(ctx.d.max()) == int(pile.max())
    ref = ctx.windows(10000000)
    assert ref[0, THR16.index(0)] == LENS[0] and (ref[:, -1] == 0).all()
    assert ref[0, THR16.index(37856)] == 100 and ref[0, THR16.index(300000)] == (0 if ctx.wrap == 18 else 100)


@pytest.mark.parametrize("thr", THRS, ids=lambda t: "n%d" % len(t))
@pytest.mark.parametrize("w", WIDTHS)
def test_windows_equal_oracle(ctx, w, thr):
    ctx.e.set_param("threshold_wave_max", WAVE_MAX[0])
    ref = ctx.windows(w)[:, cols(thr)]
    woff, cnt = ctx.e.window_thresholds(w, thr)
    assert np.array_equal(woff, ctx.e.window_layout(w))
    assert cnt.dtype == np.uint32 and cnt.shape == ref.shape
    bad = np.argwhere(cnt != ref)
    assert bad.size == 0, (bad[:5], cnt[bad[:5, 0]], ref[bad[:5, 0]])
    if w == 1:
        assert cnt.shape[0] == sum(LENS) > 2 ** 20             # more than one batch of rows
    if w == 10000000:
        assert cnt.shape[0] == len(LENS)                       # one clipped row per contig, the 1-cell and 3-cell contigs too


@pytest.mark.parametrize("wave_max", WAVE_MAX[1:], ids=["pieces", "lanes"])
@pytest.mark.parametrize("w", [7, 100, 8192, 10000, 10000000])
def test_windows_in_the_other_launch_shape(ctx, w, wave_max):
    ctx.e.set_param("threshold_wave_max", wave_max)
    try:
        _, cnt = ctx.e.window_thresholds(w, THR16)
    finally:
        ctx.e.set_param("threshold_wave_max", WAVE_MAX[0])
    ref = ctx.windows(w)
    assert np.array_equal(cnt, ref), np.argwhere(cnt != ref)[:5]


@pytest.mark.parametrize("wave_max", WAVE_MAX, ids=["default", "pieces", "lanes"])
def test_rows_equal_oracle(ctx, wave_max):
    ctx.e.set_param("threshold_wave_max", wave_max)
    segs, roff = flat(ROWS)
    cells_ref, ref = ctx.row_ref()
    try:
        for thr in THRS:
            cells, cnt = ctx.e.depth_thresholds(segs, roff, thr)
            assert cnt.dtype == np.uint64 and np.array_equal(cells, cells_ref)
            assert np.array_equal(cnt, ref[:, cols(thr)]), (thr, np.argwhere(cnt != ref[:, cols(thr)])[:5])
    finally:
        ctx.e.set_param("threshold_wave_max", WAVE_MAX[0])
    n = len(REGIONS) + len(MULTI)
    assert cells_ref[n] == cells_ref[:len(REGIONS)].sum()                      # the row of all regions
    assert cells_ref[n + 1] == 2001 + 2001 + 51 and cells_ref[n + 2] == 0 and (ref[n + 2] == 0).all()
    assert list(cells_ref[n + 3:n + 7]) == [16384, 16385, 16384, 3]
    assert (ref[:, 0] == cells_ref).all()                                      # GE0 == Cells


@pytest.mark.parametrize("wave_max", WAVE_MAX[:2], ids=["default", "pieces"])
def test_row_batch_edge(ctx, wave_max):
    """2^20 + 5 single-cell rows: the last five are a second batch"""
    n = 2 ** 20 + 5
    pos = (np.arange(n, dtype=np.int64) * 7) % LENS[0]
    pos[-5:] = [20000, 20001, 20099, 20100, 0]                                # the pile's edges in the second batch
    segs = np.stack([np.zeros(n, dtype=np.int64), pos + 1, pos + 1], axis=1).astype(np.int32)
    roff = np.arange(n + 1, dtype=np.uint64)
    thr = [0, 1, 5, 30000]
    x = ctx.d[ctx.off[0] + pos]
    ref = (x[:, None] >= np.asarray(thr, dtype=np.uint32)[None, :]).astype(np.uint64)
    ctx.e.set_param("threshold_wave_max", wave_max)
    try:
        cells, cnt = ctx.e.depth_thresholds(segs, roff, thr)
    finally:
        ctx.e.set_param("threshold_wave_max", WAVE_MAX[0])
    assert (cells == 1).all()
    assert np.array_equal(cnt, ref), np.argwhere(cnt != ref)[:5]
    assert ref[-5:, 3].sum() >= 3                                              # the second batch is not all zeros


def test_errors():
    rng = np.random.default_rng(3)
    iv = rand_intervals(rng, LENS, 20000)
    rows = [[(0, 1, 100)], [(1, 5, 50), (2, 1, 10)]]
    segs, roff = flat(rows)

    def code(fn, *a):
        with pytest.raises(pda.PdError) as x:
            fn(*a)
        return x.value.code

    with pda.Engine(LENS) as e:
        e.push_intervals(iv)
        assert code(e.depth_thresholds, segs, roff, [1]) == PD_ESTATE            # before pd_scan
        assert code(e.window_thresholds, 100, [1]) == PD_ESTATE
        e.scan(0)
        for thr in ([], list(range(17)), [5, 5], [6, 5]):
            assert code(e.depth_thresholds, segs, roff, thr) == PD_EINVAL, thr
            assert code(e.window_thresholds, 100, thr) == PD_EINVAL, thr
        assert code(e.depth_thresholds, segs, [0, 2, 1, 3], [1]) == PD_EINVAL     # row_off decreasing
        assert code(e.depth_thresholds, segs, [0, 1, 2], [1]) == PD_EINVAL        # ... not ending at n_segs
        assert code(e.depth_thresholds, segs, [1, 1, 3], [1]) == PD_EINVAL        # ... not starting at 0
        for tid in (-1, len(LENS)):
            bad = segs.copy(); bad[1, 0] = tid
            assert code(e.depth_thresholds, bad, roff, [1]) == PD_EINVAL
        assert code(e.window_thresholds, 0, [1]) == PD_EINVAL
        # the context is usable afterwards
        d, off = oracle_depth(LENS, iv, False)
        cells, cnt = e.depth_thresholds(segs, roff, [0, 1, 3])
        cells_ref, ref = rows_ref(d, off, rows, [0, 1, 3])
        assert np.array_equal(cells, cells_ref) and np.array_equal(cnt, ref)


def test_repeatable_and_leaves_the_depth_alone(ctx):
    ctx.e.set_param("threshold_wave_max", WAVE_MAX[0])
    segs, roff = flat(ROWS)
    a = ctx.e.depth_thresholds(segs, roff, THR16)
    b = ctx.e.depth_thresholds(segs, roff, THR16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for w in (7, 10000, 10000000):
        assert np.array_equal(ctx.e.window_thresholds(w, THR16)[1], ctx.e.window_thresholds(w, THR16)[1])
    for t in (0, 1, len(LENS) - 1):
        assert np.array_equal(ctx.e.read_depth(t, 0, LENS[t]), ctx.d[ctx.off[t]:ctx.off[t] + LENS[t]]), t
    # and the table's own statistic agrees: CoveredSite at -d 5 is GE5
    cover, tot = ctx.e.reduce_intervals(np.array([[0, 1, LENS[0]]], dtype=np.int32), 5)
    assert int(cover[0]) == int(a[1][len(ROWS) - 2, THR16.index(5)])
