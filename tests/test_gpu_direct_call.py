"""What pd_scan_reduce_windows' direct path does AROUND k_direct_c8: the pile-up pass launched only for a sample that has pile-up tiles
(counted when the compact sample is made; the call fails if k_direct_c8 lists another number), the window offsets kept on the device from
call to call and keyed by the width, the results coming back in one copy up to 1 MiB and straight into the caller's arrays above it, and
pd_reset's four spans zeroed by one kernel.  Every result
is compared with the numpy depth model of tests/test_gpu_runs_planes.py and with a FRESH engine fed the same sample."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_runs_planes import oracle_depth, oracle_windows, sort_iv

gpu = pytest.mark.gpu

TILE = 8192
LENS = (20 * TILE + 123, 3 * TILE, 5000)                 # contig 0: tiles 0 .. 20 (the last holds 123 cells), contig 1: tiles 21 .. 24, contig 2: tile 25
WS = (8192, 3 * 8192 + 1, 10000000)
MIN_DEPS = (0, 1, 3)
WRAPS = (0, 18)
PILE = 40000                                             # identical runs in one tile: more candidates than k_direct_c8's window takes
# where the pile-ups are: (contig, begin) of 100-cell runs
POSITIONS = {
    "none": (),
    "tile0": ((0, 300),),
    "last_partial": ((0, 20 * TILE + 10),),              # contig 0's last tile, 123 cells
    "adjacent": ((0, 5 * TILE + 100), (0, 6 * TILE + 7000)),
    "behind_seam": ((1, 50),),                           # contig 1's first tile: no look-back across the seam
    "other": ((0, 11 * TILE + 4000),),                   # (for the three-samples test: another tile than any above)
}
PILED = ("tile0", "last_partial", "adjacent", "behind_seam")


def rand_runs(rng, lens, n, length=150):
    lens = np.asarray(lens)
    tid = rng.choice(len(lens), n, p=lens / lens.sum())
    beg = (rng.random(n) * (lens[tid] + 40)).astype(np.int64) - 5            # some begin before cell 0, some end past the contig
    return np.stack([tid, beg, beg + length], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def sample(position, lens=LENS):
    """(sorted first runs, later runs in any order): a few thousand random 150-cell runs, crafted ones at the contigs' ends, the position's pile-ups"""
    n = 4000 if sum(lens) < (1 << 20) else 20000
    rng = np.random.default_rng(sum(map(ord, position)) + len(lens))
    crafted = np.array([[0, -5, 40], [0, TILE - 1, TILE + 1], [0, lens[0] - 10, lens[0] + 7], [len(lens) - 1, 0, 1], [len(lens) - 1, lens[-1] - 3, lens[-1] + 9]], dtype=np.int32)
    parts = [rand_runs(rng, lens, n), crafted]
    for tid, beg in POSITIONS[position]:
        parts.append(np.tile(np.array([[tid, beg, beg + 100]], dtype=np.int32), (PILE, 1)))
    first = sort_iv(np.concatenate(parts))
    other = rand_runs(rng, lens, n // 8)
    return first, other


@functools.lru_cache(maxsize=None)
def depth_ref(position, lens=LENS):
    first, other = sample(position, lens)
    return oracle_depth(list(lens), np.concatenate([first, other]))


@functools.lru_cache(maxsize=None)
def windows_ref(position, w, md, wrap, lens=LENS):
    return oracle_windows(depth_ref(position, lens), w, md, wrap)


def _device(first, other):
    import torch
    dev = torch.device("cuda", 0)
    return torch.from_numpy(np.ascontiguousarray(first)).to(dev), torch.from_numpy(np.ascontiguousarray(other)).to(dev)


class Compact:
    """a compact sample of an engine (pd_runs_create), destroyed with the block"""

    def __init__(self, e, first, other):
        self.e = e
        self.ft, self.ot = _device(first, other)
        self.runs = e.runs_create(self.ft.data_ptr(), self.ft.shape[0], self.ot.data_ptr() if self.ot.shape[0] else 0, self.ot.shape[0])

    def __enter__(self):
        return self.runs

    def __exit__(self, *exc):
        self.e.reset()
        self.e.runs_destroy(self.runs)


def direct_call(e, runs, w, md, wrap):
    """reset, push, one window call through the direct path -> (cover, total, launches under the "direct_tiles" events)"""
    e.reset()
    e.push_runs(runs, pda.PD_PUSH_MORE)
    e.profile(True)
    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
    passes = e.profile_get("direct_tiles")[1]
    assert e.profile_get("scatter_tiles")[1] == 0 and e.profile_get("scan_reduce_windows")[1] == 0, "the call left the direct path"
    e.profile(False)
    return cover.copy(), tot.copy(), passes


@functools.lru_cache(maxsize=None)
def fresh(position, w, md, wrap, lens=LENS):
    """the same call on an engine that has done nothing else"""
    first, other = sample(position, lens)
    with pda.Engine(list(lens)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            cover, tot, _ = direct_call(e, runs, w, md, wrap)
    return cover, tot


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_samples_are_what_they_claim():
    for position in PILED + ("other",):
        d = depth_ref(position)
        for tid, beg in POSITIONS[position]:
            assert int(d[tid][beg + 50]) >= PILE
    assert max(int(x.max()) for x in depth_ref("none")) < 100
    assert depth_ref("last_partial")[0].size - 20 * TILE == 123
    first, other = sample("adjacent")
    assert int((first[:, 2] - first[:, 1]).max()) <= 150 and int((other[:, 2] - other[:, 1]).max()) <= 150


@pytest.fixture(scope="module")
def shared():
    """one engine and compact sample per pile-up position, made by the position's first case and reused by its other seventeen"""
    made = {}

    def get(position):
        if position not in made:
            e = pda.Engine(list(LENS))
            e.keep_deferred(True)
            made[position] = (e, Compact(e, *sample(position)))
        return made[position]

    yield get
    for e, cs in made.values():
        cs.__exit__()
        e.close()


@gpu
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("md", MIN_DEPS)
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("position", PILED)
def test_pile_up_tiles(shared, position, w, md, wrap):
    """the sample's own count of pile-up tiles launches the int-window pass behind k_direct_c8: without it these tiles' windows stay unwritten"""
    e, cs = shared(position)
    cover, tot, passes = direct_call(e, cs.runs, w, md, wrap)
    assert passes == 1
    assert same((cover, tot), windows_ref(position, w, md, wrap)), "against the depth model"
    assert same((cover, tot), fresh(position, w, md, wrap)), "against a fresh engine"
    e.reset()


@gpu
@pytest.mark.parametrize("w", [8192, 10000000])
def test_three_samples_in_turn(w):
    """no pile-up, pile-up, no pile-up on ONE engine: a stale count would skip the pass (or fail the call's check of it), a stale TilePart
    would change a window"""
    order = ("none", "other", "none", "adjacent", "tile0", "none")
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        for position in order:
            with Compact(e, *sample(position)) as runs:
                cover, tot, passes = direct_call(e, runs, w, 1, 0)
                assert passes == 1, position
                assert same((cover, tot), windows_ref(position, w, 1, 0)), position
                assert same((cover, tot), fresh(position, w, 1, 0)), position


LENS_B = (3 * TILE + 5, TILE, TILE - 1, 1, 2 * TILE)     # another contig table: other offsets for every width


@gpu
def test_cached_window_offsets():
    """One engine, calls with w = 8192, 16384, 8192 — each through the direct path and, after a histogram call has materialised the sample
    (it uses the scratch buffer the offsets used to live in), through the arrays path with the OTHER width — beside a second engine with
    another contig table: offsets kept for the wrong width or the wrong table would move windows."""
    other_w = {8192: 16384, 16384: 8192}
    with pda.Engine(list(LENS)) as e, pda.Engine(list(LENS_B)) as eb:
        e.keep_deferred(True)
        eb.keep_deferred(True)
        with Compact(e, *sample("tile0")) as runs, Compact(eb, *sample("none", LENS_B)) as runs_b:
            hist0 = None
            for w in (8192, 16384, 8192):
                cover, tot, passes = direct_call(e, runs, w, 1, 0)
                assert passes == 1
                assert same((cover, tot), windows_ref("tile0", w, 1, 0)) and same((cover, tot), fresh("tile0", w, 1, 0)), w
                got_b = direct_call(eb, runs_b, other_w[w], 1, 0)
                assert same(got_b, windows_ref("none", other_w[w], 1, 0, LENS_B)) and same(got_b, fresh("none", other_w[w], 1, 0, LENS_B)), w
                hist = e.scan_depth_histogram(64, 0)                          # materialises the sample; the rows go through c->scratch
                if hist0 is None:
                    hist0 = hist.copy()
                    d = depth_ref("tile0")
                    assert [int(h.sum()) for h in hist] == [x.size for x in d] and int(hist[2][0]) == int((d[2] == 0).sum())
                assert np.array_equal(hist, hist0)
                _, cover, tot = e.scan_reduce_windows(other_w[w], 1, 0)       # the arrays path, the other width
                assert same((cover, tot), windows_ref("tile0", other_w[w], 1, 0)), ("arrays", w)
                _, cover, tot = e.scan_reduce_windows(w, 3, 0)
                assert same((cover, tot), windows_ref("tile0", w, 3, 0)), ("arrays", w)


BIG = (8 << 20,)                                         # one 8 Mb contig


@gpu
@pytest.mark.parametrize("w", [64, 128])
def test_results_on_both_sides_of_the_one_copy_limit(w):
    """w = 64: 131 072 windows, 1.5 MiB of results — above the 1 MiB up to which the results come back in one copy, so they go straight to
    the caller's arrays; w = 128: 65 536 windows, 0.75 MiB, the one copy.  Narrow windows: the 12-byte form of the direct path."""
    runs = sort_iv(np.concatenate(sample("none", BIG)))  # one sorted batch
    d = depth_ref("none", BIG)[0].astype(np.uint64)
    with pda.Engine(list(BIG)) as e:
        e.keep_deferred(True)
        for md in (1, 3):
            rows = d.reshape(-1, w)
            want = ((rows >= md).sum(axis=1).astype(np.uint32), np.where(rows >= md, rows, 0).sum(axis=1).astype(np.uint64))
            for _ in range(2):                           # the second call finds every buffer in place
                e.reset()
                e.push_intervals(runs, pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
                e.profile(True)
                _, cover, tot = e.scan_reduce_windows(w, md, 0)
                assert e.profile_get("direct_tiles")[1] == 1 and e.profile_get("scatter_tiles")[1] == 0
                e.profile(False)
                assert cover.size == BIG[0] // w
                assert np.array_equal(cover, want[0]) and np.array_equal(tot, want[1]), md
        e.reset()


# n_half (one flag byte per 4096 cells = 2 per tile): 52, 18 and 16 bytes — a 16-byte part with a tail, and 16 bytes exactly; the tile sums are
# (tiles rounded up to 4) words, a multiple of 16 bytes for every genome; the two small spans are 32 and 320 bytes
RESET_GENOMES = (LENS, (7 * TILE + 5, 100), (8 * TILE - 1,))


@gpu
@pytest.mark.parametrize("lens", RESET_GENOMES)
def test_reset_after_an_arrays_call_and_an_error(lens):
    """pd_reset zeroes the half-tile flags, the tile sums, the check words and the batch descriptors in one launch: after an arrays-path call
    (flags and sums set) and a batch that broke its promise of order (error bits in the check words and descriptors), a clean sample succeeds
    on the direct path and on the arrays path and gives a fresh engine's results"""
    first, other = sample("none", lens)
    ref = windows_ref("none", 8192, 1, 0, lens)
    with pda.Engine(list(lens)) as e:
        e.push_intervals(first, pda.PD_PUSH_SORTED)
        e.push_intervals(other)
        e.scan(0)                                        # every half-tile written, tile sums set
        assert np.array_equal(e.read_depth(0), depth_ref("none", lens)[0])
        e.reset()
        e.push_intervals(first[::-1].copy(), pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
        with pytest.raises(pda.PdError):
            e.scan_reduce_windows(8192, 1, 0)
        e.reset()
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            cover, tot, passes = direct_call(e, runs, 8192, 1, 0)
            assert passes == 1
            assert same((cover, tot), ref) and same((cover, tot), fresh("none", 8192, 1, 0, lens))
        e.keep_deferred(False)
        e.push_intervals(first, pda.PD_PUSH_SORTED)
        e.push_intervals(other)
        _, cover, tot = e.scan_reduce_windows(8192, 1, 0)
        assert same((cover, tot), ref)
        e.scan(0)
        for t in range(len(lens)):
            assert np.array_equal(e.read_depth(t), depth_ref("none", lens)[t]), t
    with pda.Engine(list(lens)) as e2:                   # the arrays path of an engine that has done nothing else
        e2.push_intervals(first, pda.PD_PUSH_SORTED)
        e2.push_intervals(other)
        _, cover, tot = e2.scan_reduce_windows(8192, 1, 0)
        assert same((cover, tot), ref)
