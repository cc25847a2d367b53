"""k_direct_c8's cover pass gives a whole tile to ONE wave and walks groups of four consecutive tiles (wave k sweeps tile 4 g + k: chunks of
512 sorted candidates, eight consecutive runs per lane, three register buffers in turn; then one barrier, the gate played over the four
outcomes in tile order, and the window path for the tiles the pass left).  Here: genomes of 1 .. 5 and 23 tiles (partial last group, groups
across contig ends), every (grid, w, min_dep, wrap); the settled count against the set of tiles the sorted stream covers, computed in numpy (the
single segment is exact); candidate counts around the chunk size; a one-cell hole at every place of the new layout; a group that holds a settled,
a declined, a contig-end and a pile-up tile; and a swept tile that the gate, closed by an earlier tile of its group, must not count.

Tables are compared with a numpy difference-array reference, with pd_set_param("direct_cover", 0) and with the arrays path."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_direct_cover import GRIDS, LENS, MODES, T, WS, _create, _device, chain, sample, sort_iv

gpu = pytest.mark.gpu

CW = 512                                                 # runs per chunk of the sweep (pd_direct.hip: k_direct_c8, COVER)
W1 = 10000000


def depths(lens, first, other):
    iv = np.concatenate([first, other]).astype(np.int64)
    out = []
    for t, ln in enumerate(lens):
        x = iv[iv[:, 0] == t]
        b, e = np.clip(x[:, 1], 0, ln), np.clip(x[:, 2], 0, ln)
        diff = np.zeros(ln + 1, dtype=np.int64)
        np.add.at(diff, b, 1)
        np.subtract.at(diff, e, 1)
        out.append(np.cumsum(diff[:ln]))
    return out


def windows(dep, w, min_dep, wrap):
    cov, tot = [], []
    for d in dep:
        x = (d & ((1 << wrap) - 1) if wrap else d).astype(np.uint64)
        for s in range(0, x.size, w):
            seg = x[s:s + w]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


def covered_by_sorted(lens, first):
    """interior tiles (whole, inside their contig) every cell of which lies in a run of the sorted stream"""
    n = 0
    for t, d in enumerate(depths(lens, first, np.zeros((0, 3), dtype=np.int32))):
        for k in range(lens[t] // T):
            n += int(d[k * T:(k + 1) * T].min() >= 1)
    return n


def interior(lens):
    return sum(ln // T for ln in lens)


def dense(lens, seed, every=3, length=150):
    rng = np.random.default_rng(seed)
    f = []
    for tid, ln in enumerate(lens):
        n = max(ln // every, 1)
        beg = np.sort(rng.integers(0, ln, n))
        f.append(np.stack([np.full(n, tid), beg, beg + length], axis=1))
        f.append(np.array([[tid, 0, length], [tid, max(ln - length, 0), ln]]))
    first = sort_iv(np.concatenate(f).astype(np.int32))
    k = rng.random(first.shape[0]) < 0.2
    other = first[k].copy()
    other[:, 1] = first[k][:, 2] + rng.integers(1, 400, int(k.sum())).astype(np.int32)
    other[:, 2] = other[:, 1] + rng.integers(1, 200, other.shape[0]).astype(np.int32)
    return first, other[rng.permutation(other.shape[0])]


def run_case(lens, first, other, lmax, grids=GRIDS, ws=WS, modes=MODES, arrays=True):
    """every (grid, w, mode): the cover form's tables = the form without the pass = numpy (= the arrays path); returns the settled counts"""
    dep = depths(lens, first, other)
    ft, ot = _device(first, other)
    settled = {}
    with pda.Engine(lens) as e:
        e.set_param("lmax", lmax)
        e.set_param("direct_cover_min", 0)
        ref = {(w, md, wrap): windows(dep, w, md, wrap) for w in ws for md, wrap in modes}
        if arrays:
            for (w, md, wrap), r in ref.items():
                e.reset()
                if first.shape[0]: e.push_intervals(first, pda.PD_PUSH_SORTED)
                if other.shape[0]: e.push_intervals(other, pda.PD_PUSH_DEFAULT)
                _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                assert np.array_equal(cover, r[0]) and np.array_equal(tot, r[1]), ("arrays", w, md, wrap)
        e.reset()
        e.keep_deferred(True)
        runs = _create(e, ft, ot)
        for grid in grids:
            e.set_param("grid_tiles", grid)
            for (w, md, wrap), r in ref.items():
                got = {}
                for cover_on in (0, 1):
                    e.set_param("direct_cover", cover_on)
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                    got[cover_on] = (cover.copy(), tot.copy())
                    n = e.profile_get("direct_cover_settled")[1]
                    if not cover_on or md > 1: assert n == 0, (grid, w, md, wrap, cover_on)
                settled[(grid, w, md, wrap)] = (n, e.profile_get("direct_pileup_tiles")[1])
                key = (grid, w, md, wrap)
                assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), key
                assert np.array_equal(got[1][0], r[0]) and np.array_equal(got[1][1], r[1]), key
        e.reset()
        e.runs_destroy(runs)
    return settled


GENOMES = {1: [T], 2: [T + 5], 3: [2 * T, 7], 4: [T, 3 * T], 5: [3 * T + 1, T], 23: LENS}


@gpu
@pytest.mark.parametrize("tiles", sorted(GENOMES))
def test_groups_of_four_tiles_on_genomes_of_every_size(tiles):
    """1 .. 5 tiles: the partial last group, a group across contig ends (edge and interior tiles together); 23: six groups, one workgroup
    walking all of them, two, and the default grid — every (w, min_dep, wrap)"""
    lens = GENOMES[tiles]
    assert sum((ln + T - 1) // T for ln in lens) == tiles
    first, other = dense(lens, 100 + tiles)
    settled = run_case(lens, first, other, 512)
    want = covered_by_sorted(lens, first)
    assert want == interior(lens)                                      # (the dense sample covers every interior tile)
    for grid in GRIDS:
        assert settled[(grid, W1, 1, 0)][0] == want, (tiles, grid)
        assert settled[(grid, W1, 0, 0)][0] == want, (tiles, grid)


@gpu
@pytest.mark.parametrize("name", ["dense", "dense_hole", "crafted", "later_only"])
def test_the_single_segment_is_exact(name):
    """default grid (a workgroup per group: no gate can close), every tile tried: the pass settles exactly the interior tiles whose sorted-stream
    runs cover them (min_dep = 1), and every interior tile for min_dep = 0"""
    first, other = sample(name)
    want = covered_by_sorted(LENS, first)
    settled = run_case(LENS, first, other, 256, grids=(0,), ws=(W1,), modes=((1, 0), (0, 0)), arrays=False)
    assert settled[(0, W1, 1, 0)][0] == want, name
    assert settled[(0, W1, 0, 0)][0] == interior(LENS), name


COUNTS = (3, 63, 64, 65, CW - 1, CW, CW + 1, 2 * CW, 2 * CW + 1)


@functools.lru_cache(maxsize=None)
def boundary_sample():
    """one contig; tile 1: 64 abutting runs (so that no later tile's candidates end inside the array's first eight words); then, every other tile,
    a tile of exactly n sorted candidates that abut and cover it, and one whose middle run is a cell short, for each n of COUNTS.  The tiles between
    hold nothing, so no tile has candidates from the bucket before it (lmax = 4096)."""
    f = chain(0, T, 2 * T)
    covered = 1
    t = 3
    for n in COUNTS:
        for hole in (False, True):
            b = [t * T + (i * T) // n for i in range(n + 1)]
            for i in range(n):
                f.append([0, b[i], b[i + 1] - (1 if hole and i == n // 2 else 0)])
            covered += 0 if hole else 1
            t += 2
    lens = [t * T]
    return lens, sort_iv(np.array(f, dtype=np.int32)), np.zeros((0, 3), dtype=np.int32), covered


@gpu
def test_candidate_counts_around_the_chunk_size():
    lens, first, other, covered = boundary_sample()
    assert int((first[:, 2] - first[:, 1]).max()) <= 4096 and covered == 1 + len(COUNTS)
    d = depths(lens, first, other)[0]
    assert int((d[T:2 * T] == 0).sum()) == 0 and int((d == 0).sum()) == (lens[0] // T - 1 - 2 * len(COUNTS)) * T + len(COUNTS)
    settled = run_case(lens, first, other, 4096, modes=((1, 0), (0, 0), (2, 0)))
    assert covered_by_sorted(lens, first) == covered
    assert settled[(0, W1, 1, 0)][0] == covered
    assert settled[(0, W1, 0, 0)][0] == interior(lens)


def hole_places(lmax):
    """Cells H of contig 0's tile 3 such that, with the dense sample's runs over H replaced by [H - 150, H) and [H + 1, H + 151), the first run behind
    the hole is candidate idx of the tile's sorted candidates with (idx // CW, idx % CW // 8, idx % 8) = (chunk, lane, place): every place of a
    lane inside a full chunk, the first run of chunks 1, 2 and 3 (one of each of the three buffers), and a run of the last, partial chunk."""
    first = sample("dense")[0]
    B = first[first[:, 0] == 0][:, 1].astype(np.int64)
    lo = 3 * T - lmax
    n0 = int(np.searchsorted(B, 4 * T, "left") - np.searchsorted(B, lo, "left"))
    found = {}
    for H in range(3 * T + 400, 4 * T - 400):
        removed = int(np.searchsorted(B, H, "right") - np.searchsorted(B, H - 150, "right"))
        ns = n0 - removed + 2
        idx = int(np.searchsorted(B, H - 150, "right") - np.searchsorted(B, lo, "left")) + 1
        chunk, full = idx // CW, ns // CW
        keys = []
        if chunk < full:
            keys.append(("place", idx % 8))
            if idx % CW == 0 and chunk in (1, 2, 3): keys.append(("chunk", chunk))
        elif ns % CW and idx % CW > 8: keys.append(("tail", 0))
        for key in keys:
            found.setdefault(key, H)
    return found


HOLE_KEYS = {("place", k) for k in range(8)} | {("chunk", 1), ("chunk", 2), ("chunk", 3), ("tail", 0)}


@gpu
def test_a_hole_at_every_place_of_the_sweep_declines_the_tile():
    lmax = 512
    where = hole_places(lmax)
    assert set(where) == HOLE_KEYS, where
    first, other = sample("dense")
    cases = sorted(where.items()) + [(("other stream only", 0), where[("place", 3)])]
    for key, H in cases:
        keep = lambda iv: iv[~((iv[:, 0] == 0) & (iv[:, 1] <= H) & (iv[:, 2] > H))]
        f = sort_iv(np.concatenate([keep(first), np.array([[0, H - 150, H], [0, H + 1, H + 151]], dtype=np.int32)]))
        o = keep(other)
        if key[0] == "other stream only":                                 # a run of the other stream closes the hole: what it covers is ignored
            o = np.concatenate([o, np.array([[0, H - 5, H + 5]], dtype=np.int32)])
        d = depths(LENS, f, o)[0]
        assert int((d == 0).sum()) == (0 if key[0] == "other stream only" else 1), key
        settled = run_case(LENS, f, o, lmax, grids=(0,), ws=(W1,), modes=((1, 0),), arrays=False)
        assert settled[(0, W1, 1, 0)][0] == interior(LENS) - 1, (key, H)


@gpu
def test_a_group_of_a_settled_a_declined_a_pileup_and_a_contig_end_tile():
    """tiles 0 .. 3 of contig 0 are one group: covered; one cell short; 32 001 identical runs on top of a cover (more than 32 000 candidates: the
    int-window pass does it); the contig's last 100 cells"""
    lens = [3 * T + 100, 2 * T]
    f = chain(0, 0, T) + chain(0, T, T + 4096) + chain(0, T + 4097, 2 * T) + chain(0, 2 * T, 3 * T) + chain(0, 3 * T, 3 * T + 100, 10)
    f += [[0, 2 * T + 1000, 2 * T + 1150]] * 32001
    second = dense([2 * T], 7)[0]
    second[:, 0] = 1
    first = sort_iv(np.concatenate([np.array(f, dtype=np.int32), second]))
    other = np.array([[0, 50, 200], [0, 3 * T + 10, 3 * T + 60], [1, 100, 250]], dtype=np.int32)
    heavy = sum(int(((first[:, 0] == 0) & (first[:, 1] >= max(t * T - 512, 0)) & (first[:, 1] < (t + 1) * T)).sum()) > 32000 for t in range(4))
    assert heavy == 1
    settled = run_case(lens, first, other, 512, ws=(W1, 8192), modes=((1, 0), (0, 0), (3, 18)))
    for key, (n, piled) in settled.items():
        assert piled == heavy, key
    assert settled[(0, W1, 1, 0)][0] == 3                                  # tile 0 of contig 0, both of contig 1
    assert settled[(0, W1, 0, 0)][0] == 4                                  # ... and the tile that is a cell short (not the pile-up tile)


@gpu
def test_a_swept_tile_the_gate_had_closed_on_is_not_counted():
    """one contig of 24 whole tiles: tile 0 covered, 1 .. 4 a cell short, the rest covered.  One workgroup walking them in order: tile 4's decline — the
    first tile of group 1 — brings the score to COVER_CLOSE, so tiles 5 .. 19 are not tried, although the waves of group 1 had swept 5, 6 and 7
    before the group's barrier: 0, 20, 21, 22, 23 settle.  A workgroup per group: every covered tile settles."""
    lens = [24 * T]
    f = chain(0, 0, T)
    for t in (1, 2, 3, 4): f += chain(0, t * T, t * T + 4096) + chain(0, t * T + 4097, (t + 1) * T)
    f += chain(0, 5 * T, 24 * T)
    first, other = sort_iv(np.array(f, dtype=np.int32)), np.zeros((0, 3), dtype=np.int32)
    settled = run_case(lens, first, other, 512, grids=(1, 0), ws=(W1,), modes=((1, 0),), arrays=False)
    assert settled[(1, W1, 1, 0)][0] == 5
    assert settled[(0, W1, 1, 0)][0] == 20
