"""GPU tests of pd_depth_levels (the -levels intervals): the HIP run-finding kernels (k_levels count / k_levels_scan / k_levels
emit) against numpy run-finding on the same cells read back with pd_read_depth — exact starts and values for every (beg, n) of a
grid of aligned, unaligned and tile-straddling ranges, in exact mode and with several edge lists — and the entry point's error
returns.  Every launch is small and bounded (the largest contig here has 9 000 001 cells)."""
import ctypes

import numpy as np
import pytest

import pandepth_amd as pda

pytestmark = pytest.mark.gpu

PD_EINVAL, PD_ESTATE, PD_ERANGE = -1, -4, -6           # include/pandepth_amd.h

#        0  1  2     3     4     5       6 (no reads)  7 (the pile)
LENS = [1, 7, 8191, 8192, 8193, 100003, 5000, 30011]
EMPTY, PILE = 6, 7
GAPS = [(30000, 31000), (8190, 8195)]                       # cells of contig 5 that no read covers (one straddles a tile edge)
N_GRID = [1, 2, 3, 4, 5, 255, 256, 257, 8192, None]      # None: up to the contig's end
BEG_GRID = [0, 1, 2, 3, 5, 255, 2046, 2047, 2049, 8189, 8190, 8191, 8192, 8195, 65534]
EDGE_SETS = {
    "exact": None,
    "e0": [0],
    "e1": [1],
    "e0_1_5_15": [0, 1, 5, 15],
    "e64": list(range(2, 2 + 3 * 62, 3)) + [1000, 262144],   # 64 edges: the table's depths, the search's, and one above 2^18
    "above": [1 << 30, (1 << 31) - 1],                       # above every depth: one run of "below the first edge"
}
assert len(EDGE_SETS["e64"]) == 64


def sample(seed):
    """random runs on every contig but EMPTY (depth 0 .. ~40), and a 300 000-read pile on PILE (above 2^18: wraps in 18-bit cells)"""
    rng = np.random.default_rng(seed)
    iv = []
    for t, ln in enumerate(LENS):
        if t == EMPTY:
            continue
        k = max(4, ln // 12)
        beg = rng.integers(-20, ln + 20, k)
        end = beg + rng.integers(1, 300, k)
        if t == 5:                                            # two stretches without a read: depth 0 inside a covered contig
            keep = np.ones(k, dtype=bool)
            for gb, ge in GAPS:
                keep &= (end <= gb) | (beg >= ge)
            beg, end = beg[keep], end[keep]
        iv.append(np.stack([np.full(beg.size, t), beg, end], axis=1))
    iv.append(np.tile(np.array([[PILE, 4090, 4100 + 17]]), (300000, 1)))
    iv.append(np.tile(np.array([[PILE, 4095, 12000]]), (400, 1)))
    return np.concatenate(iv).astype(np.int32)


def ref_levels(d, beg, n, edges):
    """(n_levels, 2) uint32 by numpy: the first cell and the value of every maximal run of d[beg : beg + n]"""
    x = d[beg:beg + n].astype(np.int64)
    cls = x if edges is None else np.searchsorted(np.asarray(edges, dtype=np.int64), x, side="right") - 1
    brk = np.ones(n, dtype=bool)
    brk[1:] = cls[1:] != cls[:-1]
    idx = np.nonzero(brk)[0]
    return np.stack([idx + beg, cls[idx] & 0xFFFFFFFF], axis=1).astype(np.uint32)


def ranges_of(ln):
    seen = []
    for beg in BEG_GRID:
        for n in N_GRID:
            m = ln - beg if n is None else n
            if beg < ln and m >= 1 and beg + m <= ln and (beg, m) not in seen:
                seen.append((beg, m))
    return seen


@pytest.fixture(scope="module", params=[0, 18], ids=["wrap0", "wrap18"])
def scanned(request):
    with pda.Engine(LENS) as e:
        e.push_intervals(sample(3 + request.param), pda.PD_PUSH_DEFAULT)
        e.scan(request.param)
        depth = [e.read_depth(t, 0, ln) for t, ln in enumerate(LENS)]
        yield e, depth, request.param


def test_sample_is_what_the_cases_need(scanned):
    e, depth, wrap = scanned
    assert not depth[EMPTY].any()
    if wrap == 18:
        assert int(depth[PILE].max()) < (1 << 18) and 300400 - (1 << 18) <= int(depth[PILE][4096]) < 300400 - (1 << 18) + 200
    else:
        assert int(depth[PILE].max()) >= 300000
    assert int(depth[5].max()) >= 16 and all(not depth[5][gb:ge].any() for gb, ge in GAPS) and depth[5][:8190].any()


@pytest.mark.parametrize("edges", list(EDGE_SETS), ids=list(EDGE_SETS))
@pytest.mark.parametrize("tid", range(len(LENS)))
def test_levels_equal_numpy_on_the_grid(scanned, tid, edges):
    e, depth, _ = scanned
    ed = EDGE_SETS[edges]
    for beg, n in ranges_of(LENS[tid]):
        got = e.depth_levels(tid, beg, n, ed)
        exp = ref_levels(depth[tid], beg, n, ed)
        assert got.dtype == np.uint32 and got.shape == exp.shape, (beg, n, got.shape, exp.shape)
        assert np.array_equal(got, exp), (beg, n)
        assert got[0, 0] == beg
    if edges == "above":
        whole = e.depth_levels(tid, 0, LENS[tid], ed)
        assert whole.tolist() == [[0, 0xFFFFFFFF]]


def test_defaults_cover_the_whole_contig(scanned):
    e, depth, _ = scanned
    assert np.array_equal(e.depth_levels(5), ref_levels(depth[5], 0, LENS[5], None))
    assert np.array_equal(e.depth_levels(5, 77, edges=[0, 1, 5, 15]), ref_levels(depth[5], 77, LENS[5] - 77, [0, 1, 5, 15]))
    assert e.depth_levels(5, 10, 0).shape == (0, 2)


def test_runs_tile_the_range(scanned):
    e, depth, _ = scanned
    for ed in (None, [0, 1, 5, 15], [3]):
        r = e.depth_levels(5, 13, 90000, ed)
        assert r[0, 0] == 13 and np.all(np.diff(r[:, 0].astype(np.int64)) > 0) and np.all(r[1:, 1] != r[:-1, 1])
        ends = np.append(r[1:, 0], 13 + 90000).astype(np.int64)
        x = np.repeat(r[:, 1], ends - r[:, 0].astype(np.int64))
        d = depth[5][13:13 + 90000]
        if ed is None:
            assert np.array_equal(x, d)
        else:
            assert np.array_equal(x.astype(np.int64), (np.searchsorted(ed, d.astype(np.int64), side="right") - 1) & 0xFFFFFFFF)


def _raw(e, tid, beg, n, edges, cap, fill=0xA5A5A5A5, rows=None):
    L = pda.load()
    out = np.full((rows if rows is not None else max(cap, 1) + 8, 2), fill, dtype=np.uint32)
    got = ctypes.c_size_t(12345)
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.uint32)
    rc = L.pd_depth_levels(e.h, tid, beg, n, None if ed is None else ed.ctypes.data_as(ctypes.c_void_p), 0 if ed is None else len(ed),
                           out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(got))
    return rc, got.value, out


@pytest.mark.parametrize("edges", [None, [0, 1, 5, 15]], ids=["exact", "edges"])
def test_cap_too_small_is_erange_with_the_true_count(scanned, edges):
    e, depth, _ = scanned
    exp = ref_levels(depth[5], 3, 50000, edges)
    assert exp.shape[0] > 40
    for cap in (0, 1, 7, exp.shape[0] - 1):
        rc, got, out = _raw(e, 5, 3, 50000, edges, cap)
        assert rc == PD_ERANGE and got == exp.shape[0], (cap, rc, got)
        assert np.array_equal(out[:cap], exp[:cap])
        assert np.all(out[cap:] == 0xA5A5A5A5), "rows beyond cap were written"
    rc, got, out = _raw(e, 5, 3, 50000, edges, exp.shape[0])                 # exactly enough
    assert rc == 0 and got == exp.shape[0] and np.array_equal(out[:got], exp) and np.all(out[got:] == 0xA5A5A5A5)


def test_invalid_arguments(scanned):
    e, depth, _ = scanned
    n = LENS[5]
    for bad in ([5, 1], [1, 1], [0, 1, 5, 5], [0, 7, 3, 9]):
        assert _raw(e, 5, 0, n, bad, n)[0] == PD_EINVAL, bad
    assert _raw(e, 5, 0, 100, list(range(65)), 100)[0] == PD_EINVAL
    assert _raw(e, 5, 0, 100, list(range(64)), 100)[0] == 0
    assert _raw(e, 5, 0, n + 1, None, n + 1)[0] == PD_EINVAL               # past the contig's end
    assert _raw(e, 5, n, 1, None, 1)[0] == PD_EINVAL
    assert _raw(e, 5, 0xFFFFFFFF, 2, None, 2)[0] == PD_EINVAL
    assert _raw(e, 0, 0, 2, None, 2)[0] == PD_EINVAL                       # contig 0 has one cell
    assert _raw(e, -1, 0, 1, None, 1)[0] == PD_EINVAL
    assert _raw(e, len(LENS), 0, 1, None, 1)[0] == PD_EINVAL
    rc, got, out = _raw(e, 5, 0, n, [9, 3], n)
    assert rc == PD_EINVAL and got == 0 and np.all(out == 0xA5A5A5A5)
    # the context still works
    assert np.array_equal(e.depth_levels(5, 0, n), ref_levels(depth[5], 0, n, None))


def test_needs_scan():
    with pda.Engine(LENS) as e:
        e.push_intervals(sample(1), pda.PD_PUSH_DEFAULT)
        assert _raw(e, 5, 0, 10, None, 10)[0] == PD_ESTATE


def test_long_contig_takes_several_rounds_of_the_offset_scan():
    """9 000 001 cells are 4395 waves: the one-workgroup scan of their counts runs more than one round of 4096 entries"""
    lens = [9000001, 12]
    rng = np.random.default_rng(9)
    k = 60000
    beg = rng.integers(0, lens[0], k)
    iv = np.stack([np.zeros(k, dtype=np.int64), beg, beg + rng.integers(1, 400, k)], axis=1).astype(np.int32)
    with pda.Engine(lens) as e:
        e.push_intervals(iv, pda.PD_PUSH_DEFAULT)
        e.scan(0)
        d = e.read_depth(0, 0, lens[0])
        for ed in (None, [0, 1, 5, 15], [2]):
            for beg0, n in ((0, lens[0]), (8388607, 611394), (5, 8388608 + 3)):
                assert np.array_equal(e.depth_levels(0, beg0, n, ed), ref_levels(d, beg0, n, ed)), (ed, beg0, n)
