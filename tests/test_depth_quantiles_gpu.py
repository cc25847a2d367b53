"""GPU parity tests of the depth percentiles (pd_depth_quantiles / pd_window_quantiles, the -quantile table): the HIP selection
kernels against numpy — np.sort(cells)[r - 1], r = max(1, ceil(p * C / 100)) — on the CPU oracle's depth (oracle/pd_oracle.c),
exact for every row, in every launch shape (group of lanes, workgroup, pieces) and through the refinement of cells >= 4095."""
import numpy as np
import pytest

import pd_oracle as O
import pandepth_amd as pda

pytestmark = pytest.mark.gpu

PD_EINVAL, PD_ESTATE = -1, -4           # include/pandepth_amd.h
NA = 0xFFFFFFFF

LENS = [700001, 250000, 50001, 1, 8192, 8191, 16384, 3, 100000]
WIDTHS = [1, 7, 64, 100, 4096, 8192, 10000, 10000000]
PCT_ALL = [0, 1, 5, 25, 50, 75, 95, 99, 100]
PCTS = [[50], [0, 100], PCT_ALL]
# (quantile_wave_max, quantile_split_cells): the defaults, every row one workgroup, every row in pieces, lanes or pieces,
# and a split between the 100-cell and the 5000-cell row
REGIMES = [(512, 262144), (0, 0xFFFFFFFF), (0, 0), (2048, 0), (0, 4999), (2048, 0xFFFFFFFF)]


# ---- the sample builders of test_depth_dist_gpu.py ----
def rand_intervals(rng, lens, n, max_len=300):
    tid = rng.integers(0, len(lens), n).astype(np.int32)
    L = np.asarray(lens, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L + 40)).astype(np.int64) - 5
    end = beg + rng.integers(0, max_len, n)
    return np.stack([tid, beg.astype(np.int32), end.astype(np.int32)], axis=1).astype(np.int32)


def clip(iv, lens):
    L = np.asarray(lens, dtype=np.int64)[iv[:, 0]]
    out = iv.copy()
    out[:, 1] = np.clip(iv[:, 1], 0, L)
    out[:, 2] = np.clip(iv[:, 2], 0, L)
    return out[out[:, 1] < out[:, 2]]


def oracle_depth(lens, iv, wrap18):
    return O.depth_from_intervals(lens, clip(iv, lens), wrap18)


def sample(seed):
    """random runs on LENS plus a 300 000-read pile in contig 0 (depth above 2^18: wraps in 18-bit cells) and a 500-read pile
    across the tile edge of contig 1"""
    rng = np.random.default_rng(seed)
    iv = rand_intervals(rng, LENS, 120000)
    return np.concatenate([iv, np.tile(np.array([[0, 20000, 20100]], dtype=np.int32), (300000, 1)),
                           np.tile(np.array([[1, 8180, 8300]], dtype=np.int32), (500, 1))])


REGIONS = np.array([
    [0, 1, 100], [0, 101, 8200],                     # touching but disjoint, the second across a tile edge
    [0, 8300, 8300], [0, 8302, 8302],                # single cells
    [0, 16380, 40000],                               # longer than one piece, across several tile edges
    [0, 40001, 40001],                               # touches the one before
    [1, 8190, 8195], [1, 200000, 250000],            # across a tile edge; ends at the contig's end
    [2, 50001, 50001],                               # the contig's last cell
    [3, 1, 1],                                       # a contig of one cell
    [5, 8000, 9000],                                 # past the end of an 8191-cell contig: clipped
    [7, 1, 3],
    [8, 5, 4],                                       # empty (no cells)
    [8, 10, 99990],
], dtype=np.int32)


# ---- the reference ----
def rank(p, c):
    return max(1, (p * c + 99) // 100)


def q_ref(cells, pct):
    if cells.size == 0:
        return [NA] * len(pct)
    s = np.sort(cells)
    return [int(s[rank(p, cells.size) - 1]) for p in pct]


def windows_ref(lens, d, off, w, pct):
    out = []
    for t, ln in enumerate(lens):
        x = d[off[t]:off[t] + ln]
        full = ln // w
        if full:
            s = np.sort(x[:full * w].reshape(full, w), axis=1)
            out.append(s[:, [rank(p, w) - 1 for p in pct]])
        if ln % w:
            out.append(np.array([q_ref(x[full * w:], pct)]))
    return np.concatenate(out).astype(np.uint32)


def rows_ref(lens, d, off, rows, pct):
    cells, q = [], []
    for segs in rows:
        parts = [d[off[t] + min(max(f - 1, 0), lens[t]):off[t] + min(max(s, 0), lens[t])] for t, f, s in segs]
        x = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        cells.append(x.size)
        q.append(q_ref(x, pct))
    return np.array(cells, dtype=np.uint64), np.array(q, dtype=np.uint32).reshape(len(rows), len(pct))


def flat(rows):
    segs = np.array([s for r in rows for s in r], dtype=np.int32).reshape(-1, 3)
    return segs, np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)


class Ctx:
    """one scanned engine and the oracle's depth per wrap, shared by the tests of this module; references computed once"""

    def __init__(self, wrap):
        self.iv = sample(41 + wrap)
        self.d, self.off = oracle_depth(LENS, self.iv, wrap == 18)
        self.e = pda.Engine(LENS)
        self.e.push_intervals(self.iv, pda.PD_PUSH_DEFAULT)
        self.e.scan(wrap)
        self.win = {}

    def windows(self, w):
        if w not in self.win:
            self.win[w] = windows_ref(LENS, self.d, self.off, w, PCT_ALL)
        return self.win[w]


@pytest.fixture(scope="module", params=[0, 18], ids=["wrap0", "wrap18"])
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.e.close()


@pytest.fixture(scope="module")
def ctx0():
    c = Ctx(0)
    yield c
    c.e.close()


def set_regime(e, wave_max, split):
    e.set_param("quantile_wave_max", wave_max)
    e.set_param("quantile_split_cells", split)


@pytest.mark.parametrize("pct", PCTS, ids=lambda p: "p" + "_".join(map(str, p)))
@pytest.mark.parametrize("w", WIDTHS)
def test_windows_equal_oracle(ctx, w, pct):
    set_regime(ctx.e, *REGIMES[0])
    ref = ctx.windows(w)[:, [PCT_ALL.index(p) for p in pct]]
    woff, q = ctx.e.window_quantiles(w, pct)
    assert np.array_equal(woff, ctx.e.window_layout(w))
    assert q.dtype == np.uint32 and q.shape == ref.shape
    bad = np.argwhere(q != ref)
    assert bad.size == 0, (bad[:5], q[bad[:5, 0]], ref[bad[:5, 0]])


def test_wrap0_pile_needs_the_refinement(ctx0):
    """the window of w = 64 that holds cells 20000 .. 20063 lies in the 300 000-read pile: its maximum is far above the 4095
    the first histogram resolves, so the windows test above cannot pass without the refinement passes"""
    ref = ctx0.windows(64)
    k = 20000 // 64 + (1 if 20000 % 64 else 0)                 # the first window wholly inside [20000, 20100)
    assert k * 64 >= 20000 and k * 64 + 64 <= 20100
    assert ref[k, PCT_ALL.index(100)] >= 300000 and ref[k, PCT_ALL.index(0)] >= 300000
    assert (ref >= 4095).any(axis=1).sum() >= 2
    assert ctx0.windows(10000000)[0, PCT_ALL.index(100)] >= 300000


MULTI = [
    [(0, 19000, 20050), (0, 20010, 21000)],                  # two overlapping segments: cells 20009 .. 20049 count twice
    [(2, 100, 300), (8, 5000, 5100), (4, 8000, 8192)],       # segments on three contigs
    [(8, 5, 4)],                                             # the only segment is empty
    [(1, 200000, 200100), (1, 100, 200), (1, 8100, 8300)],   # segments in reverse position order
    [],                                                      # a row without segments
    [(5, 8000, 9000), (5, 9000, 9100)],                      # clipped, and wholly past the contig's end
]


@pytest.mark.parametrize("regime", REGIMES[:4], ids=lambda r: "wave%d_split%d" % r)
def test_regions_equal_oracle(ctx, regime):
    set_regime(ctx.e, *regime)
    rows = [[tuple(int(x) for x in r)] for r in REGIONS] + MULTI
    segs, roff = flat(rows)
    for pct in ([50], PCT_ALL):
        cells_ref, q_exp = rows_ref(LENS, ctx.d, ctx.off, rows, pct)
        cells, q = ctx.e.depth_quantiles(segs, roff, pct)
        assert np.array_equal(cells, cells_ref)
        assert np.array_equal(q, q_exp), np.argwhere(q != q_exp)[:5]
    assert cells_ref[len(REGIONS) + 2] == 0 and (q[len(REGIONS) + 2] == NA).all() and (q[len(REGIONS) + 4] == NA).all()
    assert cells_ref[len(REGIONS)] == 1051 + 991             # the overlap is in the row twice


def test_whole_contigs(ctx):
    set_regime(ctx.e, *REGIMES[0])
    rows = [[(t, 1, ln)] for t, ln in enumerate(LENS)]
    segs, roff = flat(rows)
    cells, q = ctx.e.depth_quantiles(segs, roff, PCT_ALL)
    woff, qw = ctx.e.window_quantiles(10000000, PCT_ALL)
    assert np.array_equal(woff, np.arange(len(LENS) + 1, dtype=np.uint64))       # every contig is one window long
    assert np.array_equal(cells, np.array(LENS, dtype=np.uint64))
    assert np.array_equal(q, qw) and np.array_equal(q, ctx.windows(10000000))


def test_regimes_agree(ctx0):
    """a 100-cell row (inside the pile), a 5000-cell row (around it) and the 700 001-cell contig through every launch shape
    that can take them: the same bits, and the oracle's"""
    rows = [[(0, 20001, 20100)], [(0, 18001, 23000)], [(0, 1, LENS[0])]]
    segs, roff = flat(rows)
    cells_ref, q_exp = rows_ref(LENS, ctx0.d, ctx0.off, rows, PCT_ALL)
    assert list(cells_ref) == [100, 5000, 700001] and (q_exp[:, -1] >= 300000).all()
    for regime in REGIMES:
        set_regime(ctx0.e, *regime)
        cells, q = ctx0.e.depth_quantiles(segs, roff, PCT_ALL)
        assert np.array_equal(cells, cells_ref), regime
        assert np.array_equal(q, q_exp), (regime, q, q_exp)
        for w in (100, 5000):
            _, qw = ctx0.e.window_quantiles(w, PCT_ALL)
            ref = ctx0.windows(w)
            assert np.array_equal(qw, ref), (regime, w, np.argwhere(qw != ref)[:5])
    set_regime(ctx0.e, *REGIMES[0])


def test_more_wide_rows_than_one_launch(ctx0):
    """1024 + 7 rows that all go in pieces: two pieces + pick launches in one batch (1024 histogram rows a launch), the second with
    the seven rows left over, two of them with a second segment on another contig"""
    n = 1024 + 7
    rows = [[(0, 37 * i + 1, 37 * i + 17 + i % 23)] for i in range(n)]
    rows[-2].append((1, 8185, 8200))                           # across the tile edge of contig 1, inside its pile
    rows[-1].append((1, 100, 130))
    segs, roff = flat(rows)
    pct = [0, 50, 100]
    cells_ref, q_exp = rows_ref(LENS, ctx0.d, ctx0.off, rows, pct)
    assert cells_ref[0] == 17 and cells_ref[22] == 39 and cells_ref[-2] == 17 + (n - 2) % 23 + 16 and cells_ref[-1] == 17 + (n - 1) % 23 + 31
    set_regime(ctx0.e, *REGIMES[2])
    try:
        cells, q = ctx0.e.depth_quantiles(segs, roff, pct)
    finally:
        set_regime(ctx0.e, *REGIMES[0])
    assert np.array_equal(cells, cells_ref)
    assert np.array_equal(q, q_exp), np.argwhere(q != q_exp)[:5]
    assert q_exp[-2, 2] >= 500                                 # the second launch's rows are not all alike


def test_row_batch_edge(ctx0):
    """2^20 + 5 single-cell rows: the last five are a second batch; every quantile of a row is its one cell's depth"""
    n = 2 ** 20 + 5
    pos = np.arange(n, dtype=np.int64) % LENS[0]
    segs = np.stack([np.zeros(n, dtype=np.int64), pos + 1, pos + 1], axis=1).astype(np.int32)
    roff = np.arange(n + 1, dtype=np.uint64)
    ref = ctx0.d[ctx0.off[0] + pos].astype(np.uint32).reshape(n, 1)
    set_regime(ctx0.e, *REGIMES[0])
    cells, q = ctx0.e.depth_quantiles(segs, roff, [50])
    assert (cells == 1).all()
    assert q.shape == ref.shape and np.array_equal(q, ref), np.argwhere(q != ref)[:5]
    assert ref[20000:20100].min() >= 300000                    # the pile is among the rows


@pytest.mark.parametrize("regime", REGIMES[:3], ids=lambda r: "wave%d_split%d" % r)
def test_ties_and_tiny_rows(regime):
    """C in {1, 2, 3, 100, 101} and every p in 0 .. 100: an all-zero context (every cell ties), then a staircase (cell k of a
    contig has depth k + 1, so that the r-th smallest IS r and a rank off by one shows)"""
    lens = [1, 2, 3, 100, 101]
    rows = [[(t, 1, ln)] for t, ln in enumerate(lens)]
    segs, roff = flat(rows)
    stairs = np.array([[t, k, ln] for t, ln in enumerate(lens) for k in range(ln)], dtype=np.int32)
    for iv in (None, stairs):
        with pda.Engine(lens) as e:
            set_regime(e, *regime)
            if iv is not None:
                e.push_intervals(iv, pda.PD_PUSH_DEFAULT)
            e.scan(0)
            for p0 in range(0, 101, 16):
                pct = list(range(p0, min(p0 + 16, 101)))
                exp = np.array([[0 if iv is None else rank(p, ln) for p in pct] for ln in lens], dtype=np.uint32)
                cells, q = e.depth_quantiles(segs, roff, pct)
                assert np.array_equal(cells, np.array(lens, dtype=np.uint64))
                assert np.array_equal(q, exp), (pct, q, exp)
                _, qw = e.window_quantiles(1000, pct)
                assert np.array_equal(qw, exp), (pct, qw, exp)


def test_errors():
    rng = np.random.default_rng(3)
    iv = rand_intervals(rng, LENS, 20000)
    segs, roff = flat([[(0, 1, 100)], [(1, 5, 50), (2, 1, 10)]])

    def code(fn, *a):
        with pytest.raises(pda.PdError) as x:
            fn(*a)
        return x.value.code

    with pda.Engine(LENS) as e:
        e.push_intervals(iv)
        assert code(e.depth_quantiles, segs, roff, [50]) == PD_ESTATE            # before pd_scan
        assert code(e.window_quantiles, 100, [50]) == PD_ESTATE
        e.scan(0)
        for pct in ([], list(range(17)), [50, 50], [60, 50], [101]):
            assert code(e.depth_quantiles, segs, roff, pct) == PD_EINVAL, pct
            assert code(e.window_quantiles, 100, pct) == PD_EINVAL, pct
        assert code(e.depth_quantiles, segs, [0, 2, 1, 3], [50]) == PD_EINVAL     # row_off decreasing
        assert code(e.depth_quantiles, segs, [0, 1, 2], [50]) == PD_EINVAL        # ... not ending at n_segs
        assert code(e.depth_quantiles, segs, [1, 1, 3], [50]) == PD_EINVAL        # ... not starting at 0
        for tid in (-1, len(LENS)):
            bad = segs.copy(); bad[1, 0] = tid
            assert code(e.depth_quantiles, bad, roff, [50]) == PD_EINVAL
        assert code(e.window_quantiles, 0, [50]) == PD_EINVAL
        # the context is usable afterwards
        d, off = oracle_depth(LENS, iv, False)
        cells, q = e.depth_quantiles(segs, roff, [0, 50, 100])
        cells_ref, q_exp = rows_ref(LENS, d, off, [[(0, 1, 100)], [(1, 5, 50), (2, 1, 10)]], [0, 50, 100])
        assert np.array_equal(cells, cells_ref) and np.array_equal(q, q_exp)


def test_repeatable_and_leaves_the_depth_alone(ctx):
    set_regime(ctx.e, *REGIMES[0])
    rows = [[tuple(int(x) for x in r)] for r in REGIONS] + MULTI + [[(0, 1, LENS[0])]]
    segs, roff = flat(rows)
    a = ctx.e.depth_quantiles(segs, roff, PCT_ALL)
    b = ctx.e.depth_quantiles(segs, roff, PCT_ALL)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for w in (7, 10000, 10000000):
        assert np.array_equal(ctx.e.window_quantiles(w, PCT_ALL)[1], ctx.e.window_quantiles(w, PCT_ALL)[1])
    for t in (0, 1, len(LENS) - 1):
        assert np.array_equal(ctx.e.read_depth(t, 0, LENS[t]), ctx.d[ctx.off[t]:ctx.off[t] + LENS[t]]), t
    # and the other statistics still answer as before
    cover, tot = ctx.e.reduce_intervals(np.array([[0, 1, LENS[0]]], dtype=np.int32), 1)
    assert int(tot[0]) == int(ctx.d[ctx.off[0]:ctx.off[0] + LENS[0]].astype(np.uint64).sum())
