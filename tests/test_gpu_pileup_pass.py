"""The pile-up pass of a compact sample (k_c8_heavy: the tiles with more than 32 000 candidates, which k_direct_c8 leaves to a window of ints in
LDS).  Its candidates arrive in chunks of 8 192 runs with every load of a chunk in flight at once, and neighbouring lanes that name the same
cell add once (pd_pile_rule.h).  Here: piles of every shape the grouping and the chunking can get wrong, on a small genome, for windows of a
tile, of three tiles and a cell, and wider than any contig, min_dep 0 / 1 / 3, wrap 0 / 18 — each against the numpy depth model of
test_gpu_runs_planes.py and against the same call on the arrays path (keep_deferred(False)); and the export form (pd_export_i4) against the
export of the arrays.  Every sample also says how many of its tiles are pile-up tiles, which the engine must report for the call
(pd_profile_get("direct_pileup_tiles")): a sample that does not reach the pass checks nothing here."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_runs_planes import oracle_depth, oracle_windows, sort_iv, _device

gpu = pytest.mark.gpu

TILE = 8192
BUCKET = 512                                             # the default look-back bound: a tile's candidates begin in it or in the 512 cells before it
HEAVY = 32000                                            # more candidates than this: a pile-up tile
LENS = [6 * TILE + 123, 3 * TILE, 5000]                  # contig 0: tiles 0 .. 6 (the last one 123 cells), contig 1: tiles 7 .. 9, contig 2: tile 10
WS = (8192, 3 * 8192 + 1, 10_000_000)
MODES = tuple((md, wrap) for md in (0, 1, 3) for wrap in (0, 18))
CHUNK = 1024 * 8                                         # runs per chunk of the kernel: a workgroup's 1024 threads, 8 loads each


def pile(tid, beg, lens):
    lens = np.asarray(lens, dtype=np.int64)
    b = np.broadcast_to(np.asarray(beg, dtype=np.int64), lens.shape)
    return np.stack([np.full(lens.shape, tid, dtype=np.int64), b, b + lens], axis=1).astype(np.int32)


def background(seed, n, tids=(0, 1, 2)):
    """a few hundred ordinary runs, some clipped at their contig's ends"""
    rng = np.random.default_rng(seed)
    tid = rng.choice(np.asarray(tids), n)
    beg = (rng.random(n) * (np.asarray(LENS)[tid] + 40)).astype(np.int64) - 5
    return np.stack([tid, beg, beg + rng.integers(0, 300, n)], axis=1).astype(np.int32)


def sample(first_parts, other_parts):
    first = sort_iv(np.concatenate(first_parts))
    other = np.concatenate(other_parts) if other_parts else np.zeros((0, 3), dtype=np.int32)
    return first, other


def build(name):
    T = TILE
    if name == "threshold":                              # 32 001 identical runs: the smallest pile-up tile; 32 000 beside it: not one (nothing else near either)
        return sample([pile(0, 2 * T + 1000, np.full(32001, 150)), pile(0, 4 * T + 1000, np.full(32000, 150)), background(1, 300, (1, 2))], [background(2, 100, (1, 2))])
    if name == "one_begin_many_lengths":
        return sample([pile(0, 2 * T + 300, 1 + np.arange(40000) % 150), background(3, 500)], [background(4, 200)])
    if name == "two_cells_in_turn":                      # (the sorted stream cannot alternate: the other stream does, beside a sorted pile on the same two cells)
        return sample([pile(0, 2 * T + 300, np.full(10000, 150)), pile(0, 2 * T + 301, np.full(10000, 150)), background(5, 500)],
                      [pile(0, 2 * T + 300 + np.arange(40000) % 2, np.full(40000, 150)), background(6, 200)])
    if name == "carry_in":                               # the pile begins in the bucket before tile 3: tile 2's own, tile 3's carry-in; some end at tile 3's first cell
        return sample([pile(0, 3 * T - 100, np.where(np.arange(40000) % 4 == 0, 100, 150)), background(7, 500)], [pile(0, 3 * T - 100, np.full(500, 101)), background(8, 200)])
    if name == "tile_end":                               # ends at the tile's last cell, at its end, one past it
        return sample([pile(0, 3 * T - 150, np.repeat([149, 150, 151], 14000)), background(9, 500)], [background(10, 200)])
    if name == "other_stream_only":
        return sample([background(11, 500)], [pile(1, 1 * T + 77, np.full(40000, 150)), background(12, 200)])
    if name == "tail_chunks":                            # a stream's candidates k * CHUNK - 1, + 0, + 1, for k even and odd (the two register buffers), in either stream and in both
        C = CHUNK
        return sample([pile(0, 1 * T + 1000, np.full(4 * C - 1, 150)), pile(0, 2 * T + 1000, np.full(4 * C + 1, 150)), pile(0, 3 * T + 1000, np.full(5 * C - 1, 150)),
                       pile(0, 4 * T + 1000, np.full(5 * C + 1, 150)), pile(1, 1 * T + 1000, np.full(3 * C, 150)), pile(1, 2 * T + 2000, np.ones(1))],
                      [pile(1, 0 * T + 1000, np.full(4 * C, 150)), pile(1, 1 * T + 1000, np.full(C + 1, 150)), pile(1, 2 * T + 1000, np.full(5 * C, 150))])
    if name == "depth_wraps":                            # 300 000 runs on one cell: 2^18 = 262 144
        return sample([pile(0, 2 * T + 4095, np.full(300000, 150)), background(13, 500)], [background(14, 200)])
    if name == "runs_without_cells":
        return sample([pile(0, 2 * T + 300, np.where(np.arange(40000) % 3 == 1, 0, 150)), background(15, 500)], [pile(0, 2 * T + 300, np.zeros(3000)), background(16, 200)])
    if name == "side_by_side":
        return sample([pile(0, 2 * T + 5000, np.full(35000, 150)), pile(0, 3 * T + 10, 100 + np.arange(36000) % 3), background(17, 500)], [background(18, 200)])
    raise KeyError(name)


# the sample's pile-up tiles, counted here from the runs (below)
SAMPLES = {"threshold": 1, "one_begin_many_lengths": 1, "two_cells_in_turn": 1, "carry_in": 2, "tile_end": 2, "other_stream_only": 1, "tail_chunks": 7,
           "depth_wraps": 1, "runs_without_cells": 1, "side_by_side": 2}


def candidates(first, other):
    """candidates per tile: the runs that begin (clamped to their contig) in the tile or in the bucket before it — not across a contig's first cell"""
    tiles = [(ln + TILE - 1) // TILE for ln in LENS]
    first_tile = np.concatenate([[0], np.cumsum(tiles)])
    cand = np.zeros(int(first_tile[-1]), dtype=np.int64)
    iv = np.concatenate([first, other]).astype(np.int64)
    for t, ln in enumerate(LENS):
        b = np.clip(iv[iv[:, 0] == t][:, 1], 0, ln)
        for k in range(tiles[t]):
            lo = k * TILE - (BUCKET if k else 0)
            cand[first_tile[t] + k] = int(((b >= lo) & (b < (k + 1) * TILE)).sum())
    return cand


@functools.lru_cache(maxsize=None)
def sample_of(name):
    first, other = build(name)
    return first, other, oracle_depth(LENS, np.concatenate([first, other]))


@functools.lru_cache(maxsize=None)
def windows_of(name, w, md, wrap):
    return oracle_windows(sample_of(name)[2], w, md, wrap)


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_samples_are_what_they_claim(name):
    first, other, depth = sample_of(name)
    cand = candidates(first, other)
    assert int((cand > HEAVY).sum()) == SAMPLES[name]
    L = np.asarray(LENS)[first[:, 0]]
    assert int((np.clip(first[:, 2], 0, L) - np.clip(first[:, 1], 0, L)).max()) <= BUCKET
    if name == "threshold": assert sorted(cand[cand >= HEAVY].tolist()) == [HEAVY, HEAVY + 1]
    if name == "tail_chunks":
        C = CHUNK
        assert sorted(cand[cand > HEAVY].tolist()) == sorted([4 * C - 1, 4 * C + 1, 5 * C - 1, 5 * C + 1, 4 * C, 3 * C + C + 1, 5 * C + 1])
    if name == "depth_wraps": assert int(depth[0].max()) > (1 << 18)
    if name == "carry_in": assert int(depth[0][3 * TILE - 1]) >= 40000 and int(depth[0][3 * TILE]) >= 30000 + 500


@gpu
@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_pileup_tiles_against_the_model_and_the_arrays(name):
    first, other, _ = sample_of(name)
    ft, ot = _device(first, other)
    with pda.Engine(LENS) as e:
        e.keep_deferred(True)
        runs = e.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        for w in WS:
            for md, wrap in MODES:
                ref = windows_of(name, w, md, wrap)
                e.keep_deferred(True)
                e.reset()
                e.push_runs(runs, pda.PD_PUSH_MORE)
                _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                assert e.profile_get("direct_pileup_tiles")[1] == SAMPLES[name], (w, md, wrap)
                assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (w, md, wrap)
                e.keep_deferred(False)                   # the arrays path
                e.reset()
                e.push_runs(runs, pda.PD_PUSH_MORE)
                _, cover_a, tot_a = e.scan_reduce_windows(w, md, wrap)
                assert e.profile_get("direct_pileup_tiles")[1] == 0
                assert np.array_equal(cover, cover_a) and np.array_equal(tot, tot_a), (w, md, wrap)
        e.reset()
        e.runs_destroy(runs)


@gpu
@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_pileup_tiles_in_the_export_form(name):
    """pd_export_i4 of the compact sample equals k_export_i4 of the arrays: image and exception set"""
    import torch
    dev = torch.device("cuda", 0)
    first, other, _ = sample_of(name)
    ft, ot = _device(first, other)
    B = 8192

    def export(e):
        n_cells, _ = e.device_layout()
        img = torch.zeros(n_cells // 2, dtype=torch.uint8, device=dev)
        exc = torch.zeros((B, 2), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.export_i4(img.data_ptr(), exc.data_ptr(), B, cnt.data_ptr())
        e.synchronize()
        assert int(cnt.item()) <= B
        return img, exc[:int(cnt.item())].cpu().numpy()

    with pda.Engine(LENS) as ea, pda.Engine(LENS) as ed:
        ea.push_intervals(first, pda.PD_PUSH_SORTED)
        if other.shape[0]: ea.push_intervals(other, pda.PD_PUSH_DEFAULT)
        img_a, exc_a = export(ea)
        ed.keep_deferred(True)
        runs = ed.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        ed.push_runs(runs, pda.PD_PUSH_MORE)
        img_d, exc_d = export(ed)
        assert torch.equal(img_a, img_d)
        key = lambda x: sorted(map(tuple, x.tolist()))
        assert key(exc_a) == key(exc_d) and len(exc_a) >= 2
        ed.reset()
        ed.runs_destroy(runs)
