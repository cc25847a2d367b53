"""How k_direct_c8's cover sweeps END: the three-buffer pipeline (pdcover::sweep3; on the CPU: tests/test_sweep3_order.py) leaves its loop behind the last
chunk or behind the chunk that met a gap, in each of its three rotations, or works on the last one or two chunks in its tail, without a load.  One genome, one engine for the module: tile 2 i + 1 of the contig holds SORTED[i // 6] sorted candidates (1 .. 5 chunks of 512:
the walk ends in each rotation, right at a chunk boundary and one run past it) and OTHER[i % 6] candidates of the other stream (0 .. 2 chunks of 256 in the
narrow form), the tiles between them hold nothing; a sample per place of a TRUE gap — none, or one bare cell in front of a run of chunk 0, 1, 2, 3 or 4 of
every tile that has such a chunk, so that for min_dep 1 the stop fires in each rotation.  Every sample is walked by one workgroup (a wave sweeps tile after
tile: the next sweep begins behind the last one's loads), by two and by the default grid, for min_dep 1 and 0 (which never stops), with "cover_narrow" 1 and
0 and "direct_cover" 1 and 0, each with "cover_fast" 1 and 0 (the cover pass off with the narrow plane off is one launch: the knob is not read then).  Every table is compared element for element with a numpy difference-array reference and with the arrays path;
"direct_cover_settled" must be what the model of tests/test_gpu_cover_fast.py finds covered, eligible and reached by an open gate — the same for the three
cover forms —, "direct_cover_fast" the model's count, "direct_cover_narrow" 1 exactly for the narrow forms."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_cover_fast import CW, DECLINED, SETTLED, model, sweep_tile
from test_gpu_cover_wave import W1, depths, windows
from test_gpu_direct_cover import T, _create, _device, sort_iv

gpu = pytest.mark.gpu

SORTED = (8, 511, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049)
OTHER = (0, 1, 255, 256, 257, 512)
GAPS = (None, 0, 1, 2, 3, 4)                             # the chunk of the sorted stream that holds the run behind the bare cell
GRIDS = (1, 2, 0)
LMAX = 512
N_TILES = 2 * len(SORTED) * len(OTHER) + 1
LENS = [N_TILES * T]
FORMS = (("fast", (1, 1, 1)), ("rule", (1, 1, 0)), ("wide", (1, 0, 1)), ("wide, fast off", (1, 0, 0)), ("window", (0, 1, 1)), ("window, fast off", (0, 1, 0)))


def gap_run(gap):
    """the number, among a tile's sorted candidates, of the run that gets a bare cell in front of it: inside chunk `gap` (its first run, for the last chunk)"""
    return gap * CW + (100 if gap < 4 else 0)


@functools.lru_cache(maxsize=None)
def sample(gap):
    """-> (first, other, {tile: (sorted candidates, other candidates, has the gap)}).  A tile of n sorted candidates: eight runs at its first cell, the others
    spread evenly (4 cells apart or more, below 256: the narrow form's end check passes), 150 cells each and none beyond the tile's end: covered, but for n = 8.
    The gap: every run in front of run j ends at or before the cell in front of run j's begin."""
    rng = np.random.default_rng(20)
    f, o, tiles = [], [], {}
    for i in range(len(SORTED) * len(OTHER)):
        t, n, m = 2 * i + 1, SORTED[i // len(OTHER)], OTHER[i % len(OTHER)]
        b = np.array([max(k - 7, 0) * T // (n - 7) for k in range(n)], dtype=np.int64)
        e = np.minimum(b + 150, T)
        j = gap_run(gap) if gap is not None else n
        if 0 < j < n:
            assert b[j] - b[j - 1] >= 4
            e[:j] = np.minimum(e[:j], b[j] - 1)
        f.append(np.stack([np.zeros(n, dtype=np.int64), t * T + b, t * T + e], axis=1))
        ob = rng.integers(0, T // 2, m)                  # (in the tile's first half: no candidates of the tile behind it)
        o.append(np.stack([np.zeros(m, dtype=np.int64), t * T + ob, t * T + ob + rng.integers(0, 200, m)], axis=1))
        tiles[t] = (n, m, 0 < j < n)
    first, other = sort_iv(np.concatenate(f).astype(np.int32)), np.concatenate(o).astype(np.int32)
    return first, other, tiles


@functools.lru_cache(maxsize=None)
def reference(gap):
    first, other, _ = sample(gap)
    dep = depths(LENS, first, other)
    return {md: windows(dep, W1, md, 0) for md in (1, 0)}


def test_the_samples_are_what_they_claim():
    """(no GPU) candidate counts; the sweep of every tile ends where it should: a tile with the gap is declined for min_dep 1 in the gap's chunk, every other tile
    of more than eight candidates is settled; among the tiles the stop fires behind chunk 0, 1, 2, 3 and 4 and the walk ends behind 1, 2, 3, 4 and 5 chunks"""
    ends = set()
    for gap in GAPS:
        first, other, tiles = sample(gap)
        d = depths(LENS, first, other)[0]
        for t, (n, m, has_gap) in tiles.items():
            c = first[(first[:, 1] >= t * T - LMAX) & (first[:, 1] < (t + 1) * T)]
            oc = other[(other[:, 1] >= t * T - LMAX) & (other[:, 1] < (t + 1) * T)]
            assert c.shape[0] == n and oc.shape[0] == m and int(np.diff(c[:, 1]).max(initial=0)) < 256
            b, ln = c[:, 1].astype(np.int64) - t * T, (c[:, 2] - c[:, 1]).astype(np.int64)
            oc1 = sweep_tile(b, ln, 1)[0]
            assert oc1 == (DECLINED if has_gap or n == 8 else SETTLED) and sweep_tile(b, ln, 0)[0] == SETTLED
            if has_gap:
                bare = t * T + int(b[gap_run(gap)]) - 1
                assert m or int(d[bare]) == 0
                ends.add(("stop", gap, (n + CW - 1) // CW))
            else:
                assert n == 8 or m or int(d[t * T:(t + 1) * T].min()) >= 1
                ends.add(("end", (n + CW - 1) // CW))
    assert {e[1] for e in ends if e[0] == "end"} == {1, 2, 3, 4, 5}
    assert {e[1] for e in ends if e[0] == "stop"} == {0, 1, 2, 3, 4}
    assert ("stop", 0, 1) in ends and ("stop", 4, 5) in ends         # a stop in the walk's last chunk as well


@pytest.fixture(scope="module")
def engine():
    with pda.Engine(LENS) as e:
        e.set_param("lmax", LMAX)
        e.set_param("direct_cover_min", 0)
        yield e


@gpu
@pytest.mark.parametrize("gap", GAPS, ids=lambda g: "none" if g is None else "chunk%d" % g)
def test_the_sweeps_end_in_every_rotation(engine, gap):
    e = engine
    first, other, _ = sample(gap)
    ref = reference(gap)
    e.keep_deferred(False)
    for md, r in ref.items():
        e.reset()
        e.push_intervals(first, pda.PD_PUSH_SORTED)
        e.push_intervals(other, pda.PD_PUSH_DEFAULT)
        _, cover, tot = e.scan_reduce_windows(W1, md, 0)
        assert np.array_equal(cover, r[0]) and np.array_equal(tot, r[1]), ("arrays", md)
    ft, ot = _device(first, other)
    e.reset()
    e.keep_deferred(True)
    runs = _create(e, ft, ot)
    try:
        for grid in GRIDS:
            e.set_param("grid_tiles", grid)
            for md, r in ref.items():
                settled, accepted = {}, {}
                for form, (cover_on, narrow_on, fast_on) in FORMS:
                    e.set_param("direct_cover", cover_on)
                    e.set_param("cover_narrow", narrow_on)
                    e.set_param("cover_fast", fast_on)
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(W1, md, 0)
                    assert np.array_equal(cover, r[0]) and np.array_equal(tot, r[1]), (form, grid, md)
                    settled[form] = e.profile_get("direct_cover_settled")[1]
                    accepted[form] = e.profile_get("direct_cover_fast")[1]
                    assert e.profile_get("direct_cover_narrow")[1] == (1 if narrow_on and cover_on else 0), (form, grid, md)
                want_fast, want_settled = model(LENS, first, LMAX, W1, md, grid)
                print(gap, grid, md, "settled", settled, "accepted", accepted, "model", (want_fast, want_settled))
                assert all(settled[f] == want_settled for f in ("fast", "rule", "wide", "wide, fast off")), (grid, md, settled, want_settled)
                assert settled["window"] == 0 and settled["window, fast off"] == 0, (grid, md, settled)
                assert accepted["fast"] == want_fast and all(v == 0 for f, v in accepted.items() if f != "fast"), (grid, md, accepted, want_fast)
    finally:
        for name in ("direct_cover", "cover_narrow", "cover_fast"):
            e.set_param(name, 1)
        e.set_param("grid_tiles", 0)
        e.reset()
        e.runs_destroy(runs)
