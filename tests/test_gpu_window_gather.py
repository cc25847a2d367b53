"""k_window_gather: for windows of a tile or more, every tile leaves its shares of the two windows it can touch and the gather adds up, per
window, the shares of the tiles the window spans — a wave per window below 256 tiles per window, a workgroup per window from there on, several
loads in flight per lane, and the tile's first or second share chosen by comparing where the tile begins with where the window begins.
Here: a 5 M-cell contig (610 tiles and three cells) between 600 contigs of one to three tiles, windows of one tile, of 10 000 cells (borders
inside tiles), of 300 tiles and a cell (the workgroup form, borders inside tiles, a last window that ends mid-tile) and wider than any contig,
min_dep 0 and 2 — against the numpy depth model of test_gpu_runs_planes.py, on the direct path (a compact sample, kept deferred) and on the
arrays path's fused sweep."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_runs_planes import oracle_depth, oracle_windows, sort_iv, _device

gpu = pytest.mark.gpu

TILE = 8192
BIG = 5_000_003


@functools.lru_cache(maxsize=None)
def genome():
    rng = np.random.default_rng(42)
    small = rng.integers(1, 3 * TILE + 1, 600)
    small[:6] = (1, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE)
    return [int(x) for x in small[:300]] + [BIG] + [int(x) for x in small[300:]]


WS = (8192, 10_000, 300 * 8192 + 1, 10_000_000)
MIN_DEPS = (0, 2)


@functools.lru_cache(maxsize=None)
def sample():
    lens = np.asarray(genome())
    rng = np.random.default_rng(7)
    n = 120_000
    tid = rng.choice(lens.size, n, p=lens / lens.sum())
    beg = (rng.random(n) * (lens[tid] + 40)).astype(np.int64) - 5
    iv = np.stack([tid, beg, beg + rng.integers(0, 400, n)], axis=1).astype(np.int32)
    first, other = sort_iv(iv[:100_000]), iv[100_000:]
    return first, other, oracle_depth(genome(), iv)


@functools.lru_cache(maxsize=None)
def windows(w, md):
    return oracle_windows(sample()[2], w, md, 0)


def test_the_genome_is_what_it_claims():
    lens = genome()
    assert len(lens) == 601 and max(lens) == BIG and BIG % TILE and sorted(lens)[-2] <= 3 * TILE
    assert BIG // TILE > 2 * 300 and (BIG % (300 * TILE + 1)) % TILE           # more than two windows of 300 tiles, the last one ends mid-tile
    assert all(w >= TILE for w in WS) and WS[2] // TILE >= 256 and WS[1] % TILE and WS[3] > BIG
    d = sample()[2][300]
    assert int(d.max()) >= 3 and int((d < 2).sum()) > 1000                      # min_dep 2 leaves cells out


@gpu
@pytest.mark.parametrize("path", ["direct", "arrays"])
def test_window_gather_against_the_model(path):
    first, other, _ = sample()
    ft, ot = _device(first, other)
    with pda.Engine(genome()) as e:
        e.keep_deferred(path == "direct")
        runs = e.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        for w in WS:
            for md in MIN_DEPS:
                e.reset()
                e.push_runs(runs, pda.PD_PUSH_MORE)
                _, cover, tot = e.scan_reduce_windows(w, md, 0)
                ref = windows(w, md)
                assert cover.shape == ref[0].shape
                assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (w, md)
        e.reset()
        e.runs_destroy(runs)
