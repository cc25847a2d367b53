"""k_direct_c8's cover pass settles an interior tile from its runs alone — CoveredSite = all cells, TotalDepth = the clipped lengths — when
the sorted stream's runs leave no gap (pandepth_amd/csrc/pd_cover_rule.h; the rule itself: tests/test_direct_cover_rule.py), and hands
every other tile to the window path.  Here: tiles crafted around the rule's edges, a dense sample whose interior tiles all settle, the
same with one uncovered cell, thin samples and a sample without a sorted stream, for every bucket width, walked by one workgroup, by two
and by the default grid — against a numpy difference-array reference, against the arrays path of the same engine, and with
pd_set_param("direct_cover", 0), the kernel form without the pass, element for element.

That the pass is taken is shown by a count: the kernel adds the tiles it settled to a word of the direct path's result words, which
pd_profile_get("direct_cover_settled") returns for the last call."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda

gpu = pytest.mark.gpu

TILE = 8192
T = TILE
# contig 0: tiles 0 .. 16 whole (first flat cells 57344, 65536, 131072 among them: the seams of the 16-bit arithmetic) + 5 cells; then exactly
# one tile, 8191 cells, one cell, 2 tiles
LENS = [17 * TILE + 5, TILE, TILE - 1, 1, 2 * TILE]
INTERIOR = 17 + 1 + 2                                    # tiles inside their contig (and inside one window, for w = 10 000 000)
MAXLEN = 200                                             # no run longer than the narrowest bucket (256 cells)
WS = (8192, 10000, 10000000)
MODES = ((0, 0), (1, 0), (2, 0), (3, 18), (1, 4))        # (min_dep, wrap); (1, 4): depths above 15 wrap, so a covered tile must NOT settle
GRIDS = (1, 2, 0)


def sort_iv(iv):
    return iv[np.lexsort((iv[:, 1], iv[:, 0]))]          # stable: runs with one begin keep their order


def chain(tid, a, b, step=128):
    """abutting runs of `step` cells from a up to b"""
    return [[tid, x, min(x + step, b)] for x in range(a, b, step)]


def crafted_sample():
    f, o = [], []
    f += chain(0, 0, T)                                                             # tile 0: covered, ends on the tile's edge (no look-back cover for tile 1)
    f += chain(0, T + 1, 2 * T)                                                     # tile 1: a one-cell gap at cell 0
    f += chain(0, 2 * T, 3 * T)                                                     # tile 2: covered (its last cells by tile 3's look-back run too)
    f += [[0, 3 * T - 100, 3 * T]] + chain(0, 3 * T + 1, 4 * T)                     # tile 3: a look-back run ending exactly at the first cell: not covered
    f += [[0, 4 * T - 100, 4 * T + 1]] + chain(0, 4 * T + 1, 5 * T)                 # tile 4: ... ending one cell past it: covered
    f += [[0, 5 * T, 5 * T + 200], [0, 5 * T + 10, 5 * T + 20], [0, 5 * T + 50, 5 * T + 250]] + chain(0, 5 * T + 250, 6 * T)   # tile 5: a short run, then a begin beyond its end
    f += chain(0, 6 * T, 6 * T + 4096) + [[0, 6 * T + 4096, 6 * T + 4096], [0, 6 * T + 4097, 6 * T + 4097]] + chain(0, 6 * T + 4097, 7 * T)   # tile 6: empty runs at a gap's edges
    f += [[0, 7 * T - 5, 7 * T + 1]] + chain(0, 7 * T + 1, 8 * T)                   # tile 7 (flat 57344): cell 0 by a look-back run only
    f += [[0, 8 * T - 200, 8 * T]] + chain(0, 8 * T, 9 * T) + chain(0, 8 * T + 37, 9 * T, 101)   # tile 8 (flat 65536): two layers
    for k, t in zip((15, 16, 17, 18), (9, 10, 11, 12)):                             # tiles 9 .. 12: a one-cell gap behind the k-th run: on a wave's seam for some bucket width
        f += chain(0, t * T, t * T + 128 * k) + chain(0, t * T + 128 * k + 1, (t + 1) * T)
    f += chain(0, 13 * T, 14 * T - 300) + [[0, 14 * T - 300, 14 * T - 200], [0, 14 * T - 199, 14 * T - 100]] + chain(0, 14 * T - 100, 14 * T)   # tile 13: a gap among the last runs,
    o += [[0, 13 * T + 10, 13 * T + 100], [0, 14 * T - 150, 14 * T - 50], [0, 13 * T - 20, 13 * T + 10]]                                  # ... the other stream's runs behind them
    f += chain(0, 14 * T, 14 * T + 4096) + chain(0, 14 * T + 4097, 15 * T)          # tile 14: a gap that only a run of the other stream covers
    o += [[0, 14 * T + 4090, 14 * T + 4110], [0, 14 * T - 3, 14 * T], [0, 14 * T - 3, 14 * T + 1]]
    f += chain(0, 15 * T, 16 * T) + [[0, 15 * T, 15 * T], [0, 15 * T + 128, 15 * T + 128], [0, 16 * T - 1, 16 * T - 1]]   # tile 15: empty runs, no gap
    f += chain(0, 16 * T, 17 * T)                                                   # tile 16 (flat 131072): reach ends at TILE exactly
    f += chain(0, 17 * T, 17 * T + 5)                                               # the contig's last 5 cells
    f += chain(1, 0, T - 1) + chain(1, 0, T - 1, 77)                                # contig 1: two layers, a one-cell gap at cell TILE - 1 (reach ends at TILE - 1)
    f += chain(2, 0, T - 1)
    f += [[3, 0, 1]]
    f += chain(4, 0, 2 * T) + chain(4, 0, 2 * T, 77) + chain(4, 0, 2 * T, 191)      # contig 4: three layers
    o += [[4, 100, 250], [4, T - 10, T + 10]]
    return sort_iv(np.array(f, dtype=np.int32)), np.array(o, dtype=np.int32)


CRAFTED_SETTLE = 10                                      # tiles 0, 2, 4, 5, 7, 8, 15, 16 of contig 0, both of contig 4
CRAFTED_SETTLE_ONE_WORKGROUP = 6                         # ... walked by ONE workgroup: tiles 9 .. 12 are four declined in a row, the 15 tiles behind them are not tried


def dense_runs(rng, every=3, length=150):
    """a begin every `every` cells on average, runs of `length` cells; every contig's first and last cells covered"""
    f = []
    for tid, ln in enumerate(LENS):
        n = max(ln // every, 1)
        beg = np.sort(rng.integers(0, ln, n))
        f.append(np.stack([np.full(n, tid), beg, beg + length], axis=1))
        f.append(np.array([[tid, 0, length], [tid, max(ln - length, 0), ln]]))
    return sort_iv(np.concatenate(f).astype(np.int32))


def later_runs(rng, first, frac=0.2):
    k = rng.random(first.shape[0]) < frac
    other = first[k].copy()
    other[:, 1] = first[k][:, 2] + rng.integers(1, 400, int(k.sum())).astype(np.int32)
    other[:, 2] = other[:, 1] + rng.integers(1, MAXLEN, other.shape[0]).astype(np.int32)
    return other[rng.permutation(other.shape[0])]


HOLE = 3 * T + 5000                                      # dense_hole: the one uncovered cell (contig 0, tile 3)


@functools.lru_cache(maxsize=None)
def sample(name):
    """(sorted first runs, later runs in any order)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    none = np.zeros((0, 3), dtype=np.int32)
    if name == "crafted":
        return crafted_sample()
    if name in ("dense", "dense_hole"):
        first = dense_runs(rng)
        other = later_runs(rng, first)
        if name == "dense_hole":
            keep = lambda iv: iv[~((iv[:, 0] == 0) & (iv[:, 1] <= HOLE) & (iv[:, 2] > HOLE))]
            first = sort_iv(np.concatenate([keep(first), np.array([[0, HOLE - 150, HOLE], [0, HOLE + 1, HOLE + 151]], dtype=np.int32)]))
            other = keep(other)
        return first, other
    if name == "thin":                                   # 2.5x: gaps in every tile, the gate closes
        first = dense_runs(rng, every=60)
        return first, later_runs(rng, first)
    if name == "later_only":                             # no sorted stream at all: nothing can settle for min_dep >= 1
        return none, dense_runs(rng, every=6)[rng.permutation(sum(max(ln // 6, 1) + 2 for ln in LENS))]
    raise KeyError(name)


SAMPLES = ("crafted", "dense", "dense_hole", "thin", "later_only")


@functools.lru_cache(maxsize=None)
def depth_ref(name):
    first, other = sample(name)
    iv = np.concatenate([first, other]).astype(np.int64)
    out = []
    for t, ln in enumerate(LENS):
        x = iv[iv[:, 0] == t]
        b, e = np.clip(x[:, 1], 0, ln), np.clip(x[:, 2], 0, ln)
        ok = b < e
        diff = np.zeros(ln + 1, dtype=np.int64)
        np.add.at(diff, b[ok], 1)
        np.subtract.at(diff, e[ok], 1)
        out.append(np.cumsum(diff[:ln]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def windows_ref(name, w, min_dep, wrap):
    cov, tot = [], []
    for d in depth_ref(name):
        x = (d & ((1 << wrap) - 1) if wrap else d).astype(np.uint64)
        for s in range(0, x.size, w):
            seg = x[s:s + w]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


def test_reference_samples_are_what_they_claim():
    """checked on the numpy reference, no engine involved"""
    for name in SAMPLES:
        for iv in sample(name):
            if iv.shape[0]: assert int((iv[:, 2] - iv[:, 1]).max()) <= MAXLEN and int((iv[:, 2] - iv[:, 1]).min()) >= 0, name
    f = sample("crafted")[0]
    assert all(np.all(np.diff(f[f[:, 0] == t][:, 1]) >= 0) for t in range(len(LENS)))
    c = depth_ref("crafted")[0]
    zero = set(np.flatnonzero(c == 0).tolist())
    assert zero == {T, 3 * T, 6 * T + 4096, 14 * T - 200} | {t * T + 128 * k for k, t in zip((15, 16, 17, 18), (9, 10, 11, 12))}
    assert int(c[14 * T + 4096]) == 1 and int(c[7 * T]) == 1 and int(c[4 * T]) == 1     # covered by the other stream / by a look-back run only
    c1 = depth_ref("crafted")[1]
    assert int(depth_ref("crafted")[4].min()) == 3 and int(c1[:T - 1].min()) == 2 and int(c1[T - 1]) == 0
    d = depth_ref("dense")
    assert all(int(x.min()) >= 1 for x in d) and 40 <= np.concatenate(d).mean() <= 75 and int(np.concatenate(d).max()) > 15
    h = depth_ref("dense_hole")
    assert [int((x == 0).sum()) for x in h] == [1, 0, 0, 0, 0] and int(h[0][HOLE]) == 0
    first_only = np.zeros(LENS[0] + 1, dtype=np.int64)               # the sorted stream alone covers the dense sample: every interior tile can settle
    f = sample("dense")[0]; f = f[f[:, 0] == 0]
    np.add.at(first_only, np.clip(f[:, 1], 0, LENS[0]), 1); np.subtract.at(first_only, np.clip(f[:, 2], 0, LENS[0]), 1)
    assert int(np.cumsum(first_only[:-1]).min()) >= 1
    thin = depth_ref("thin")[0]
    assert all(int((thin[t * T:(t + 1) * T] == 0).sum()) > 0 for t in range(17))
    assert sample("later_only")[0].shape[0] == 0 and int(depth_ref("later_only")[0].min()) >= 1


def _device(first, other):
    import torch
    dev = torch.device("cuda", 0)
    return torch.from_numpy(np.ascontiguousarray(first)).to(dev), torch.from_numpy(np.ascontiguousarray(other)).to(dev)


def _create(e, ft, ot):
    return e.runs_create(ft.data_ptr() if ft.shape[0] else 0, ft.shape[0], ot.data_ptr() if ot.shape[0] else 0, ot.shape[0])


def _arrays(e, name, first, other):
    out = {}
    for w in WS:
        for md, wrap in MODES:
            e.reset()
            if first.shape[0]: e.push_intervals(first, pda.PD_PUSH_SORTED)
            if other.shape[0]: e.push_intervals(other, pda.PD_PUSH_DEFAULT)
            _, cover, tot = e.scan_reduce_windows(w, md, wrap)
            ref = windows_ref(name, w, md, wrap)
            assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), ("arrays", w, md, wrap)
            out[(w, md, wrap)] = (cover.copy(), tot.copy())
    return out


@gpu
@pytest.mark.parametrize("lmax", [256, 512, 4096])
@pytest.mark.parametrize("name", SAMPLES)
def test_cover_pass_equals_window_path_reference_and_arrays(name, lmax):
    """every (grid, w, min_dep, wrap), with the pass and without it; grid_tiles = 1: ONE workgroup walks all tiles, so its gate closes and
    opens on the way"""
    first, other = sample(name)
    ft, ot = _device(first, other)
    with pda.Engine(LENS) as e:
        e.set_param("lmax", lmax)
        e.set_param("direct_cover_min", 0)               # (by default tiles with fewer than 2048 candidates are left to the window: most tiles here)
        arrays = _arrays(e, name, first, other)
        e.reset()
        e.keep_deferred(True)
        runs = _create(e, ft, ot)
        for grid in GRIDS:
            e.set_param("grid_tiles", grid)
            for w in WS:
                for md, wrap in MODES:
                    got = {}
                    for cover_on in (0, 1):
                        e.set_param("direct_cover", cover_on)
                        e.reset()
                        e.push_runs(runs, pda.PD_PUSH_MORE)
                        _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                        got[cover_on] = (cover.copy(), tot.copy())
                        settled = e.profile_get("direct_cover_settled")[1]
                        if not cover_on or md > 1: assert settled == 0, (grid, w, md, wrap, cover_on)
                        if wrap == 4 and name in ("dense", "dense_hole"): assert settled == 0       # thousands of candidates per tile: any depth may wrap
                    ref = windows_ref(name, w, md, wrap)
                    key = (grid, w, md, wrap)
                    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), key
                    assert np.array_equal(got[1][0], ref[0]) and np.array_equal(got[1][1], ref[1]), key
                    assert np.array_equal(got[1][0], arrays[(w, md, wrap)][0]) and np.array_equal(got[1][1], arrays[(w, md, wrap)][1]), key
        e.reset()
        e.runs_destroy(runs)


def _settled(e, runs, w, md, wrap):
    e.reset()
    e.push_runs(runs, pda.PD_PUSH_MORE)
    e.scan_reduce_windows(w, md, wrap)
    return e.profile_get("direct_cover_settled")[1]


@gpu
@pytest.mark.parametrize("lmax", [256, 4096])
def test_the_pass_is_taken(lmax):
    """the settled count of the last call: all interior tiles of the dense sample, all but the one with the hole, exactly the crafted
    tiles the rule can prove; every interior tile for min_dep = 0; none with the pass switched off, with another kernel form, or where a
    depth could wrap"""
    with pda.Engine(LENS) as e:
        e.set_param("lmax", lmax)
        e.set_param("direct_cover_min", 0)
        e.keep_deferred(True)
        e.profile(True)
        for name, want in (("dense", INTERIOR), ("dense_hole", INTERIOR - 1), ("crafted", CRAFTED_SETTLE), ("later_only", 0)):
            ft, ot = _device(*sample(name))
            runs = _create(e, ft, ot)
            e.set_param("direct_cover", 1)
            assert _settled(e, runs, 10000000, 1, 0) == want, name
            assert e.profile_get("direct_tiles")[1] >= 1
            assert _settled(e, runs, 10000000, 0, 0) == INTERIOR, name
            assert _settled(e, runs, 8192, 1, 0) == want, name              # (contig slots start on tile boundaries: a tile is one window of 8192)
            assert _settled(e, runs, 10000, 1, 0) <= want, name             # windows of 10 000 cells cut most tiles
            assert _settled(e, runs, 10000000, 2, 0) == 0, name
            if name != "crafted": assert _settled(e, runs, 10000000, 1, 4) == 0, name
            e.set_param("direct_un", 704)
            assert _settled(e, runs, 10000000, 1, 0) == 0, name
            e.set_param("direct_un", 0)
            e.set_param("direct_cover", 0)
            assert _settled(e, runs, 10000000, 1, 0) == 0, name
            e.reset()
            e.runs_destroy(runs)


@gpu
def test_the_gate_closes_on_a_thin_sample_and_changes_nothing():
    """one workgroup walks all 23 tiles.  Thin: none covered, nothing settles.  Crafted: tiles 9 .. 12 decline in a row, which closes the
    gate (a declined tile adds COVER_DECLINE = 2 to the workgroup's score, a settled one takes 1 off, COVER_CLOSE = 8), so the COVER_SKIP = 15 tiles
    behind them are not tried although four of them are covered — the
    count says that the gate closed, the tables of the first test (grid_tiles = 1) that nothing depends on it"""
    with pda.Engine(LENS) as e:
        e.keep_deferred(True)
        e.set_param("grid_tiles", 1)
        e.set_param("direct_cover_min", 0)
        ft, ot = _device(*sample("thin"))
        runs = _create(e, ft, ot)
        assert _settled(e, runs, 10000000, 1, 0) == 0
        e.reset(); e.runs_destroy(runs)
        ft, ot = _device(*sample("crafted"))
        runs = _create(e, ft, ot)
        n = _settled(e, runs, 10000000, 1, 0)
        assert n == CRAFTED_SETTLE_ONE_WORKGROUP
        e.reset(); e.runs_destroy(runs)


@gpu
def test_tiles_with_few_candidates_are_left_to_the_window_by_default():
    """"direct_cover_min" (default 2048 candidates): the crafted sample holds a few hundred runs per tile and runs the kernel form without the
    pass, the dense sample's 3 000 per tile are tried; the tables are the same either way (first test)"""
    with pda.Engine(LENS) as e:
        e.keep_deferred(True)
        for name, want in (("crafted", 0), ("dense", INTERIOR)):
            ft, ot = _device(*sample(name))
            runs = _create(e, ft, ot)
            assert _settled(e, runs, 10000000, 1, 0) == want, name
            e.set_param("direct_cover_min", 100000)
            assert _settled(e, runs, 10000000, 1, 0) == 0, name
            e.set_param("direct_cover_min", 2048)
            e.reset(); e.runs_destroy(runs)


def hole_variants(lmax):
    """Cells H of contig 0's tile 3 such that, with the dense sample's runs over H replaced by [H - 150, H) and [H + 1, H + 151), the first run behind
    the hole is — in its wave's quarter of the tile's sorted candidates (k_direct_c8: quarters of ceil(n / 4) runs, chunks of 256, four consecutive
    runs per lane) — inside a FULL chunk at each of the four in-lane positions, the first run of a lane (position 0), and the first run of a chunk."""
    first = sample("dense")[0]
    B = first[first[:, 0] == 0][:, 1].astype(np.int64)             # sorted begins of contig 0 (every run 150 cells)
    lo = 3 * T - lmax                                              # the tile's candidates begin in [lo, 4 T)
    n0 = int(np.searchsorted(B, 4 * T, "left") - np.searchsorted(B, lo, "left"))
    found = {}
    for H in range(3 * T + 400, 4 * T - 400):
        removed = int(np.searchsorted(B, H, "right") - np.searchsorted(B, H - 150, "right"))      # H - 150 < begin <= H
        ns = n0 - removed + 2
        idx = int(np.searchsorted(B, H - 150, "right") - np.searchsorted(B, lo, "left")) + 1        # candidates in front of the run [H + 1, ..)
        qs = (ns + 3) // 4
        wave, pos = divmod(idx, qs)
        n_w = min(qs, ns - wave * qs)
        if pos >= (n_w // 256) * 256: continue                     # the quarter's last, partial chunk: the crafted tiles run that path
        for key in (("lane", pos % 4), ("chunk", 0) if pos % 256 == 0 and pos else None):
            if key and key not in found: found[key] = H
        if len(found) == 5: break
    return found


@gpu
def test_a_hole_at_every_place_of_a_full_chunk_declines_the_tile():
    """the sweep of 256 runs per wave and step (four per lane, a DPP maximum across lanes, the reach carried between chunks) must see a one-cell
    hole wherever its far edge falls: each in-lane position, a lane's first run, a chunk's first run"""
    lmax = 512
    where = hole_variants(lmax)
    assert set(where) == {("lane", 0), ("lane", 1), ("lane", 2), ("lane", 3), ("chunk", 0)}, where
    first, other = sample("dense")
    with pda.Engine(LENS) as e:
        e.set_param("lmax", lmax)
        e.set_param("direct_cover_min", 0)
        e.keep_deferred(True)
        for key, H in sorted(where.items()):
            keep = lambda iv: iv[~((iv[:, 0] == 0) & (iv[:, 1] <= H) & (iv[:, 2] > H))]
            f = sort_iv(np.concatenate([keep(first), np.array([[0, H - 150, H], [0, H + 1, H + 151]], dtype=np.int32)]))
            o = keep(other)
            iv = np.concatenate([f, o]).astype(np.int64)
            cov_ref, tot_ref = [], []
            for t, ln in enumerate(LENS):
                x = iv[iv[:, 0] == t]
                diff = np.zeros(ln + 1, dtype=np.int64)
                np.add.at(diff, np.clip(x[:, 1], 0, ln), 1); np.subtract.at(diff, np.clip(x[:, 2], 0, ln), 1)
                d = np.cumsum(diff[:ln])
                cov_ref.append(int((d >= 1).sum())); tot_ref.append(int(d.sum()))
            assert cov_ref[0] == LENS[0] - 1, key
            ft, ot = _device(f, o)
            runs = _create(e, ft, ot)
            got = {}
            for cover_on in (0, 1):
                e.set_param("direct_cover", cover_on)
                e.reset()
                e.push_runs(runs, pda.PD_PUSH_MORE)
                _, cover, tot = e.scan_reduce_windows(10000000, 1, 0)
                got[cover_on] = (cover.copy(), tot.copy())
            assert e.profile_get("direct_cover_settled")[1] == INTERIOR - 1, (key, H)
            assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), (key, H)
            assert got[1][0].tolist() == cov_ref and got[1][1].tolist() == tot_ref, (key, H)
            e.reset(); e.runs_destroy(runs)
