"""GPU parity tests of pd_depth_gc_bias (the -gcbias file): the HIP kernel and its piece-wise upload, through capi.py, against
tests/gcbias_model.py on the CPU oracle's depth (oracle/pd_oracle.c) — exact integers — in both launch shapes, in every group
size of the narrow shape, across piece boundaries, and at the edges of the byte classification."""
import numpy as np
import pytest

import pd_oracle as O
import pandepth_amd as pda
import gcbias_model as M

pytestmark = pytest.mark.gpu

PD_EINVAL, PD_ESTATE = -1, -4           # include/pandepth_amd.h
BIG = 5 * 2 ** 20 + 13                  # room for regions of W - 1, W, W + 1 and 2W - 1 cells at W = 2^20
LENS = [BIG, 70001, 8192, 8191, 4099, 3, 1, 100000]
# the issue's widths, and both sides of every width at which the launch changes: the group of lanes doubles at 16, 32, ... 1024
# cells ("about sixteen cells a lane"), a workgroup takes the window above "gcbias_wave_max" = 4096
WIDTHS = [1, 2, 3, 7, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025, 4096, 4097, 8191, 8192, 8193, 65537, 2 ** 20]


def clip(iv, lens):
    L = np.asarray(lens, dtype=np.int64)[iv[:, 0]]
    out = iv.copy()
    out[:, 1] = np.clip(iv[:, 1], 0, L)
    out[:, 2] = np.clip(iv[:, 2], 0, L)
    return out[out[:, 1] < out[:, 2]]


def rand_intervals(rng, lens, n, max_len=300):
    tid = rng.integers(0, len(lens), n).astype(np.int32)
    L = np.asarray(lens, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L + 40)).astype(np.int64) - 5
    end = beg + rng.integers(0, max_len, n)
    return np.stack([tid, beg.astype(np.int32), end.astype(np.int32)], axis=1).astype(np.int32)


def rand_bases(rng, n, block=2048):
    """ACGT in both cases whose GC share changes from block to block, so that windows of every width land in many bins"""
    p_gc = rng.random((n + block - 1) // block).repeat(block)[:n]
    gc = rng.random(n) < p_gc
    pick = rng.integers(0, 4, n)
    return np.where(gc, np.frombuffer(b"CGcg", dtype=np.uint8)[pick], np.frombuffer(b"ATat", dtype=np.uint8)[pick]).astype(np.uint8)


class Ctx:
    """one scanned engine, the oracle's depth and the bases, shared by the tests of this module"""

    def __init__(self, wrap):
        rng = np.random.default_rng(77 + wrap)
        self.wrap = wrap
        iv = np.concatenate([rand_intervals(rng, LENS, 150000), rand_intervals(rng, LENS[1:2], 60000),
                             np.tile(np.array([[0, 20000, 20100]], dtype=np.int32), (300000, 1)),      # above 2^18: wraps in 18-bit cells
                             np.array([[0, 0, BIG]] * 3, dtype=np.int32)])
        d, off = O.depth_from_intervals(LENS, clip(iv, LENS), wrap == 18)
        self.depth = [d[off[t]:off[t] + LENS[t]] for t in range(len(LENS))]
        self.bases = [rand_bases(rng, n) for n in LENS]
        self.bases[0][3 * 2 ** 20 + 77] = ord("N")               # one invalid byte far inside the long contig
        b1 = self.bases[1]                                       # contig 1: invalid bytes at every residue modulo 16, 64 and 100
        b1[1000 + 65 * np.arange(200)] = ord("N")
        b1[[30000, 30015, 30016, 30031, 30032]] = np.frombuffer(b"RnX-\0", dtype=np.uint8)
        self.bases[4] = self.bases[4][:2000]                     # a record shorter than its contig
        self.bases[7] = None                                     # a contig without a record
        self.e = pda.Engine(LENS)
        self.e.push_intervals(iv, pda.PD_PUSH_DEFAULT)
        self.e.scan(wrap)

    def model(self, W, regs=None):
        spans = M.whole_contigs(LENS) if regs is None else M.spans_of_regions(regs, LENS)
        return M.gc_bias(self.depth, self.bases, spans, W)

    def check(self, W, regs=None, two_bins=True):
        win, tot, sk = self.e.depth_gc_bias(W, self.bases, regs)
        rw, rt, rs = self.model(W, regs)
        assert np.array_equal(win, rw), (W, np.flatnonzero(win != rw)[:5], win[win != rw][:5], rw[win != rw][:5])
        assert np.array_equal(tot, rt), (W, np.flatnonzero(tot != rt)[:5])
        assert sk == rs, (W, sk, rs)
        if two_bins:
            assert int((rw > 0).sum()) >= 2
        return rw, rt, rs


@pytest.fixture(scope="module", params=[0, 18], ids=["wrap0", "wrap18"])
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.e.close()


def width_regions(W):
    """on the long contig, from an unaligned first cell: regions of W - 1, W, W + 1 and 2W - 1 cells, each touching the one before;
    then the other contigs whole"""
    regs, p = [], 5
    for n in (W - 1, W, W + 1, 2 * W - 1):
        if n:
            regs.append([0, p + 1, p + n])
        p += n
    return np.array(regs + [[t, 1, LENS[t]] for t in range(1, len(LENS))], dtype=np.int32)


@pytest.mark.parametrize("W", WIDTHS)
def test_widths(ctx, W):
    rw, rt, rs = ctx.check(W, width_regions(W), two_bins=W < 2 ** 20)
    if W == 2 ** 20:
        assert rw.sum() == 2 and rs == 1                        # W, W + 1 and 2W - 1 give a window each; the last holds the N


@pytest.mark.parametrize("W", [1, 7, 100, 4096, 65537])
def test_whole_contigs(ctx, W):
    rw, rt, rs = ctx.check(W)
    if W == 1:
        assert rs == 200 + 5 + (4099 - 2000) + 100000 + 1


def test_the_pile_wraps(ctx):
    pile = ctx.depth[0][20000:20100]
    base = 300000 - 2 ** 18 if ctx.wrap == 18 else 300000
    assert base <= int(pile.min()) and int(pile.max()) < base + 1000
    ctx.check(100, np.array([[0, 19901, 20300]], dtype=np.int32), two_bins=False)


# 1024; values that are no multiple of W; a window per piece; the largest
@pytest.mark.parametrize("W,piece", [(7, 1024), (7, 777), (100, 1024), (100, 777), (100, 2 ** 26), (4096, 1024), (4096, 1), (8193, 1), (8193, 20000)])
def test_piece_size_changes_nothing(ctx, W, piece):
    regs = width_regions(W)[1:]                                # from the region of W cells on
    ctx.e.set_param("gcbias_piece_cells", piece)
    try:
        ctx.check(W, regs)
    finally:
        ctx.e.set_param("gcbias_piece_cells", 2 ** 25)


@pytest.mark.parametrize("W,wave_max", [(1, 0), (7, 0), (100, 0), (1000, 0), (4097, 2 ** 20), (8192, 2 ** 20), (65537, 2 ** 20)])
def test_the_other_launch_shape(ctx, W, wave_max):
    ctx.e.set_param("gcbias_wave_max", wave_max)
    try:
        ctx.check(W, width_regions(W)[:6])                       # the long contig's regions, contigs 1 and 2
    finally:
        ctx.e.set_param("gcbias_wave_max", 4096)


def test_region_lists(ctx):
    regs = np.array([[1, 0, 250], [1, 251, 300], [1, 301, 650], [1, 651, 651], [1, 69950, 80000],      # first < 1; touching; shorter than W; one cell; clipped at the end
                     [4, 1901, 2100], [4, 2101, 2300], [7, 1, 500]], dtype=np.int32)                  # the record ends at a window edge of the first; none for the second; no record
    rw, rt, rs = ctx.check(100, regs)
    assert M.spans_of_regions(regs, LENS)[0] == (1, 0, 250) and M.spans_of_regions(regs, LENS)[4] == (1, 69949, 70001)
    assert rs >= 1 + 2 + 5
    ctx.check(50, regs)


def test_errors_and_the_context_is_left_as_found(ctx):
    def code(*a):
        with pytest.raises(pda.PdError) as x:
            ctx.e.depth_gc_bias(*a)
        return x.value.code

    before = ctx.e.depth_histogram(64)
    assert code(0, ctx.bases) == PD_EINVAL and code(2 ** 20 + 1, ctx.bases) == PD_EINVAL
    assert code(100, ctx.bases, np.array([[1, 500, 600], [1, 100, 200]], dtype=np.int32)) == PD_EINVAL        # unsorted
    assert code(100, ctx.bases, np.array([[1, 100, 200], [0, 100, 200]], dtype=np.int32)) == PD_EINVAL
    assert code(100, ctx.bases, np.array([[1, 100, 200], [1, 200, 300]], dtype=np.int32)) == PD_EINVAL        # overlapping by one cell
    assert code(100, ctx.bases, np.array([[len(LENS), 1, 2]], dtype=np.int32)) == PD_EINVAL
    a = ctx.e.depth_gc_bias(100, ctx.bases)
    b = ctx.e.depth_gc_bias(100, ctx.bases)                      # set, not added to
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(ctx.e.depth_histogram(64), before)
    for t in (1, 4):
        assert np.array_equal(ctx.e.read_depth(t, 0, LENS[t]), ctx.depth[t])


def test_before_scan():
    with pda.Engine([1000]) as e:
        e.push_intervals(np.array([[0, 10, 500]], dtype=np.int32))
        with pytest.raises(pda.PdError) as x:
            e.depth_gc_bias(10, [b"ACGT" * 250])
        assert x.value.code == PD_ESTATE


# ---- small contexts --------------------------------------------------------------------------------------------------------
class Small:
    """a scanned engine of its own and the oracle's depth; check() compares one call with the model"""

    def __init__(self, lens, iv):
        iv = np.asarray(iv, dtype=np.int32).reshape(-1, 3)
        d, off = O.depth_from_intervals(lens, clip(iv, lens), False)
        self.lens = lens
        self.depth = [d[off[t]:off[t] + lens[t]] for t in range(len(lens))]
        self.e = pda.Engine(lens)
        self.e.push_intervals(iv)
        self.e.scan(0)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.e.close()

    def check(self, bases, W, regs=None, piece=None, wave_max=None):
        self.e.set_param("gcbias_piece_cells", 2 ** 25 if piece is None else piece)
        self.e.set_param("gcbias_wave_max", 4096 if wave_max is None else wave_max)
        got = self.e.depth_gc_bias(W, bases, regs)
        spans = M.whole_contigs(self.lens) if regs is None else M.spans_of_regions(regs, self.lens)
        ref = M.gc_bias(self.depth, bases, spans, W)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], (got[0].nonzero(), ref[0].nonzero(), got[2], ref[2])
        return ref


def small(lens, iv, bases, W, regs=None, piece=None, wave_max=None):
    with Small(lens, iv) as s:
        return s.check(bases, W, regs, piece, wave_max)


def test_all_byte_values():
    win, tot, sk = small([256], [[0, 0, 256], [0, 60, 90]], [bytes(range(256))], 1)
    assert win[100] == 4 and win[0] == 4 and win.sum() == 8 and sk == 248
    assert tot[100] == 4 + 2 and tot[0] == 4 + 2                 # C G c g / A T a t: the upper-case ones lie under the second run


@pytest.mark.parametrize("W", [7, 64])
def test_contig_lengths_around_the_width(W):
    lens = [W - 1, W, W + 1, 2 * W - 1, 1, 3 * W + 5]
    rng = np.random.default_rng(W)
    win, tot, sk = small(lens, rand_intervals(rng, lens, 400, 20), [rand_bases(rng, n, 5) for n in lens], W)
    assert win.sum() + sk == 0 + 1 + 1 + 1 + 0 + 3


def test_invalid_bytes_at_the_edges():
    """an invalid byte at a window's first and last cell, on either side of a piece boundary (1024 cells) and, the contig
    starting at byte 16 of the piece, of a 16-byte boundary; a record cut inside a window, at a window edge, and none"""
    lens = [4096 + 37, 4096, 4096, 300]
    rng = np.random.default_rng(5)
    with Small(lens, rand_intervals(rng, lens, 3000, 200)) as s:
        for bad in ([0], [63], [64], [1023], [1024], [1023, 1024], [2047], [2048], [15], [16], [17], [4095], [4096 + 36], [4031, 4032]):
            bases = [rand_bases(rng, n, 256) for n in lens]
            bases[0][bad] = ord("N")
            bases[1] = bases[1][:1000]                           # cut inside a window (1000 = 15 * 64 + 40 = 62 * 16 + 8)
            bases[2] = bases[2][:1024]                           # cut at a window edge, and at a piece's
            bases[3] = None
            for W in (64, 16):
                for piece in (None, 1024):
                    win, tot, sk = s.check(bases, W, piece=piece)
                    assert sk >= len(set(b // W for b in bad if b < 4096)) + (4096 - 1000 + W - 1) // W + (4096 - 1024) // W + 300 // W


def test_one_bin_under_full_contention():
    """2^20 windows of one cell, all G: every add of every workgroup goes to bin 100"""
    n = 2 ** 20
    win, tot, sk = small([n], [[0, 0, n], [0, 5, n - 5], [0, 1000, 2000]], [b"G" * n], 1)
    assert win[100] == n and win.sum() == n and sk == 0 and tot[100] == n + n - 10 + 1000


@pytest.mark.parametrize("W,wave_max", [(1, None), (1024, None), (2 ** 17, None), (2 ** 17, 2 ** 20), (1000, 0)])
def test_sums_above_32_bits(W, wave_max):
    """depth 70 000 over 2^17 cells of one bin — one long run pushed 70 000 times: 9.2e9"""
    n = 2 ** 17
    iv = np.tile(np.array([[0, 0, n]], dtype=np.int32), (70000, 1))
    win, tot, sk = small([n], iv, [b"C" * n], W, wave_max=wave_max)
    assert tot[100] == 70000 * (n // W * W) > 2 ** 32 and win[100] == n // W
