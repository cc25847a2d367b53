"""The FAST CHUNK of k_direct_c8's narrow cover sweep: a full chunk of the sorted stream (512 runs, eight per lane) behind a run that begins at or behind
cell 0 is judged from a summary per lane — the lane's last begin against P = max(reach, the largest end of the lanes before it), the chunk's largest end
against the tile — and, accepted, adds the sum of its length bytes; every other chunk, and a refused one, goes through the rule as before
(pandepth_amd/csrc/pd_cover_rule.h; on the CPU: tests/test_cover_fast_rule.py).  pd_set_param("cover_fast", 0) runs the sweep without it;
pd_profile_get("direct_cover_fast") is the number of chunks the last call accepted.

Every case is compared element for element with a numpy difference-array reference, the arrays path, and the same call with "cover_fast" 0, with
"cover_narrow" 0 and with "direct_cover" 0, walked by one workgroup, by two and by the default grid, for min_dep 1 and 0 and windows of 10 000 000 and
8192 cells.  "direct_cover_settled" must be the same with "cover_fast" 1 and 0; "direct_cover_fast" must be 0 with "cover_fast" 0 and otherwise EXACTLY
what model() below works out from the case's runs: the sweep of every tile chunk by chunk (rebuilt begins, the acceptance test, the rule for what is
not accepted, the stop at a gap for min_dep 1) and the gate of every workgroup over the tiles it walks, which decides which tiles are swept at all.

Which of these 12 tests fail for a mutation of the fast chunk (each run as a library of its own; tests/harness/cover_fast_check.cpp fails for all five):
  the lane test `>` replaced by `>=`   1: test_tiles_of_exactly_512_513_and_1024_sorted_candidates (a first lane AT the reach, 0, must be accepted: the count)
  P formed without `reach`             12: lane 0 is never within P, nothing is accepted — every count
  `pb` not carried on acceptance       4: the last full chunk beyond the tile, the counted tiles, the step of 256 at a chunk boundary, the decode session's sample
                                       (the step into the next chunk is taken from a stale byte, the end check fails, the tile takes the window: the settled counts;
                                       512 runs of the background advance 1536 cells, a multiple of 256, so ITS chunks hide a stale byte)
  `top <= TILE` dropped                2: test_the_last_full_chunk_reaches_beyond_the_tile and test_runs_of_255_cells[8] (lengths not clipped: the sums, and the count)
  the dot selector 0x01010101          12: the begin bytes are added to the lengths — every sum"""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_cover_narrow import LENS, NONE, W1, background, dense_bam, with_step  # noqa: F401  (dense_bam: the fixture)
from test_gpu_cover_wave import depths, windows
from test_gpu_direct_cover import T, _create, _device, sort_iv

gpu = pytest.mark.gpu

CW = 512                                                 # sorted runs per chunk of the narrow sweep
GRIDS = (1, 2, 0)
WS = (W1, 8192)
MODES = ((1, 0), (0, 0))
NO_END = -32768                                          # pdcover::NONE
WINDOW, DECLINED, SETTLED = 1, 2, 3                      # a tile's outcome in the cover pass (k_direct_c8: COV_*)
COVER_DECLINE, COVER_CLOSE, COVER_SKIP = 2, 8, 15        # the gate (pd_direct.hip)


def sweep_tile(b, ln, min_dep):
    """the narrow sweep of one tile: b, ln: tile-relative begins and lengths of its sorted candidates in order -> (outcome, chunks accepted as fast chunks)"""
    n, reach, gap, fast = int(b.size), 0, False, 0
    if n:
        rb = b[0] + np.concatenate([[0], np.cumsum(np.diff(b) & 255)])      # the begins as the sweep rebuilds them
        e = rb + ln
    for q in range(0, n, CW):
        cnt, base = min(CW, n - q), int(rb[q - 1] if q else rb[0])
        accepted = False
        if cnt == CW and base >= 0:
            incl = np.maximum.accumulate(e[q:q + CW].reshape(64, 8).max(axis=1))
            p = np.maximum(np.concatenate([[NO_END], incl[:-1]]), reach)
            accepted = bool((rb[q + 7:q + CW:8] <= p).all()) and int(incl[-1]) <= T
            if accepted:
                fast += 1
                reach = max(reach, int(incl[-1]))
        if not accepted:                                 # the rule, run by run
            before = np.maximum.accumulate(np.concatenate([[reach], e[q:q + cnt]]))[:-1]
            gap = gap or bool((rb[q:q + cnt] > before).any())
            reach = max(reach, int(e[q:q + cnt].max()))
        if gap and min_dep:
            break
    if gap and min_dep:
        return DECLINED, fast
    if n and int(rb[-1]) != int(b[-1]):
        return WINDOW, fast                              # the end check: not tried
    return (SETTLED if (not gap and reach >= T) or not min_dep else DECLINED), fast


def tiles_of(lens, first, lmax, w, min_dep):
    """every flat tile in order -> [(swept when the gate is open, outcome, fast chunks)]"""
    out, seen = [], 0
    for tid, ln in enumerate(lens):
        x = first[first[:, 0] == tid].astype(np.int64)
        for k in range((ln + T - 1) // T):
            pc = k * T
            c = x[(x[:, 1] >= (pc - lmax if k else 0)) & (x[:, 1] < pc + T)]
            shi = seen + int((x[:, 1] < pc + T).sum())   # where the tile's sorted candidates end in the sample's array
            eligible = ln - pc >= T and (pc // w + 1) * w - pc >= T and not (c.shape[0] and shi < 8)
            if eligible:
                oc, fast = sweep_tile(c[:, 1] - pc, c[:, 2] - c[:, 1], min_dep)
                out.append((True, oc, fast))
            else:
                out.append((False, WINDOW, 0))
        seen += x.shape[0]
    return out


def model(lens, first, lmax, w, min_dep, grid):
    """-> (chunks accepted as fast chunks, tiles settled) of one call: workgroup g of `grid` walks the groups g, g + grid, ... of four tiles and plays its gate"""
    tiles = tiles_of(lens, first, lmax, w, min_dep)
    groups = (len(tiles) + 3) // 4
    grid = grid or groups                                # the default grid of these few tiles is a workgroup per group
    fast = settled = 0
    for g in range(min(grid, groups)):
        miss = skip = 0
        for it in range(g, groups, grid):
            at_start = skip
            for k, (eligible, oc, nf) in enumerate(tiles[4 * it:4 * it + 4]):
                swept = eligible and at_start <= k
                fast += nf if swept else 0
                if skip:
                    skip -= 1
                elif swept and oc == SETTLED:
                    settled += 1
                    miss -= 1 if miss else 0
                elif swept and oc == DECLINED:
                    miss += COVER_DECLINE
                    if miss >= COVER_CLOSE:
                        miss, skip = COVER_CLOSE, COVER_SKIP
    return fast, settled


FORMS = (("fast", (1, 1, 1)), ("rule", (1, 1, 0)), ("wide", (1, 0, 1)), ("window", (0, 1, 1)))


def run_case(lens, first, other, lmax, grids=GRIDS, ws=WS, modes=MODES):
    """-> {(grid, w, min_dep): chunks accepted}, everything else asserted on the way"""
    dep = depths(lens, first, other)
    ft, ot = _device(first, other)
    out = {}
    with pda.Engine(lens) as e:
        e.set_param("lmax", lmax)
        e.set_param("direct_cover_min", 0)
        ref = {(w, md, wrap): windows(dep, w, md, wrap) for w in ws for md, wrap in modes}
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
                key = (grid, w, md)
                settled, accepted = {}, {}
                for form, (cover_on, narrow_on, fast_on) in FORMS:
                    e.set_param("direct_cover", cover_on)
                    e.set_param("cover_narrow", narrow_on)
                    e.set_param("cover_fast", fast_on)
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                    assert np.array_equal(cover, r[0]) and np.array_equal(tot, r[1]), (form, key)
                    settled[form] = e.profile_get("direct_cover_settled")[1]
                    accepted[form] = e.profile_get("direct_cover_fast")[1]
                    assert e.profile_get("direct_cover_narrow")[1] == (1 if narrow_on and cover_on else 0), (form, key)
                want_fast, want_settled = model(lens, first, lmax, w, md, grid)
                print(key, "accepted", accepted, "settled", settled, "model", (want_fast, want_settled))
                assert accepted["rule"] == 0 and accepted["wide"] == 0 and accepted["window"] == 0, (key, accepted)
                assert settled["fast"] == settled["rule"] and settled["window"] == 0, (key, settled)
                assert settled["fast"] == want_settled, (key, settled, want_settled)
                assert accepted["fast"] == want_fast, (key, accepted, want_fast)
                out[key] = accepted["fast"]
        for name in ("direct_cover", "cover_narrow", "cover_fast"):
            e.set_param(name, 1)
        e.reset()
        e.runs_destroy(runs)
    return out


@functools.lru_cache(maxsize=None)
def base_first():
    f = background(LENS)
    f.setflags(write=False)
    return f


def candidates(first, tid, k, lmax=512):
    """the sorted candidates of tile k of contig tid"""
    x = first[first[:, 0] == tid]
    return x[(x[:, 1] >= (k * T - lmax if k else 0)) & (x[:, 1] < (k + 1) * T)]


def test_the_model_on_the_dense_background():
    """(no GPU) a tile of the background, a 150-cell run every 3 cells with 512 cells of look-back: 170 + 2731 candidates, five full chunks; chunk 0 begins
    before cell 0 and is not tried, chunks 1 .. 4 are accepted (a lane spans 21 cells, every run 150).  A contig's first tile has no look-back: its chunk 0
    begins AT cell 0, but its first lane's last begin, 21, is beyond the reach, 0 — refused; 2731 candidates, chunks 1 .. 4 accepted."""
    first = base_first()
    c = candidates(first, 0, 3)
    assert c.shape[0] == 170 + 2731
    assert sweep_tile(c[:, 1].astype(np.int64) - 3 * T, (c[:, 2] - c[:, 1]).astype(np.int64), 1) == (SETTLED, 4)
    c = candidates(first, 0, 0)
    assert c.shape[0] == 2731 and sweep_tile(c[:, 1].astype(np.int64), (c[:, 2] - c[:, 1]).astype(np.int64), 1) == (SETTLED, 4)
    # 12 interior tiles (9 + 3), the gate never closes: whatever the grid
    for grid in GRIDS:
        assert model(LENS, first, 512, W1, 1, grid) == (48, 12) and model(LENS, first, 512, 8192, 0, grid) == (48, 12)


@gpu
def test_the_dense_background_accepts_the_middle_chunks():
    first = base_first()
    rng = np.random.default_rng(5)
    k = rng.random(first.shape[0]) < 0.1
    other = first[k].copy()
    other[:, 1] += 160 + rng.integers(0, 300, other.shape[0]).astype(np.int32)
    other[:, 2] = other[:, 1] + rng.integers(0, 250, other.shape[0]).astype(np.int32)
    other = other[rng.permutation(other.shape[0])]
    out = run_case(LENS, first, other, 512)
    assert all(v == 48 for v in out.values()), out


# where, in tile 3 of contig 0, the run behind a true gap stands among the tile's sorted candidates
GAP_AT = {"in the middle of a lane": 2 * CW + 8 * 20 + 3, "at a lane boundary": 2 * CW + 8 * 20, "at a chunk boundary": 2 * CW,
          "in the first chunk that is tried": CW + 8 * 5 + 1}


@gpu
@pytest.mark.parametrize("where", sorted(GAP_AT))
def test_a_true_gap(where):
    """tile 3 of contig 0: the background's runs that begin in [x, x + 200) replaced by a run of 100 cells at x and one at x + 200, candidate number j of its
    tile — 53 bare cells in front of it (the runs before x end before x + 150).  The chunk that holds run j is refused and the rule finds the gap: for
    min_dep 1 the sweep ends there (chunks 1 .. j // 512 - 1 accepted), for min_dep 0 it goes on and accepts the full chunks behind it."""
    j = GAP_AT[where]
    c0 = int(candidates(base_first(), 0, 3)[0, 1])
    x = c0 + 3 * (j - 1)
    first = with_step(base_first(), 0, x, 200)
    c = candidates(first, 0, 3)
    assert int(c[j, 1]) == x + 200 and int(c[j - 1, 1]) == x
    b, ln = c[:, 1].astype(np.int64) - 3 * T, (c[:, 2] - c[:, 1]).astype(np.int64)
    n_full = c.shape[0] // CW
    assert sweep_tile(b, ln, 1) == (DECLINED, j // CW - 1)
    assert sweep_tile(b, ln, 0) == (SETTLED, n_full - 2)                   # every full chunk but chunk 0 and the gap's
    out = run_case(LENS, first, NONE, 512)
    assert out[(0, W1, 1)] == 44 + j // CW - 1 and out[(0, W1, 0)] == 44 + n_full - 2


@gpu
def test_the_last_full_chunk_reaches_beyond_the_tile():
    """contig 1's first tile (flat tile 10, no look-back): its 2731 background runs and 341 runs of 10 cells at cell 1000 are 6 * 512 candidates exactly, so
    the last FULL chunk holds the runs that end behind the tile: refused (its largest end is 8340), its lengths are clipped by the rule"""
    extra = np.tile(np.array([[1, 1000, 1010]], dtype=np.int32), (341, 1))
    first = sort_iv(np.concatenate([base_first(), extra]))
    c = candidates(first, 1, 0)
    assert c.shape[0] == 6 * CW and int(c[:, 2].max()) == 8340
    assert sweep_tile(c[:, 1].astype(np.int64), (c[:, 2] - c[:, 1]).astype(np.int64), 1) == (SETTLED, 4)      # chunks 1 .. 4 of 0 .. 5
    out = run_case(LENS, first, NONE, 512)
    assert all(v == 48 for v in out.values()), out


COUNTS = (CW, CW + 1, 2 * CW)


@functools.lru_cache(maxsize=None)
def counts_sample():
    """one contig; tile 1 dense; tiles 3, 5, 7: exactly n sorted candidates for n of COUNTS, nothing in the tiles between (no look-back candidates): eight
    runs at the tile's first cell, the others spread evenly over the tile, 150 cells each but none beyond the tile's end.  Chunk 0 begins AT cell 0 with its first
    lane AT the reach, 0, and its largest end is the tile's last cell exactly: accepted; so is the second full chunk of 1024."""
    f = [background([T], every=3, length=150) + np.array([0, T, T], dtype=np.int32)]
    t = 3
    for n in COUNTS:
        b = np.array([t * T + max(i - 7, 0) * T // (n - 7) for i in range(n)], dtype=np.int64)
        f.append(np.stack([np.zeros(n, dtype=np.int64), b, np.minimum(b + 150, (t + 1) * T)], axis=1).astype(np.int32))
        t += 2
    return [t * T], sort_iv(np.concatenate(f))


@gpu
def test_tiles_of_exactly_512_513_and_1024_sorted_candidates():
    lens, first = counts_sample()
    for k, n in zip((3, 5, 7), COUNTS):
        c = candidates(first, 0, k, lmax=0)
        assert c.shape[0] == n and int(c[:, 2].max()) == (k + 1) * T
        assert sweep_tile(c[:, 1].astype(np.int64) - k * T, (c[:, 2] - c[:, 1]).astype(np.int64), 1) == (SETTLED, n // CW)
    out = run_case(lens, first, NONE, 512)
    # tile 1 (its look-back is the empty tile 0: 2731 candidates, chunk 0 from cell 0
    # refused, 4 accepted) + 1 + 1 + 2; the empty tiles decline one by one between settled ones: no gate closes in the default grid
    assert out[(0, W1, 1)] == 4 + 1 + 1 + 2 and out[(0, W1, 0)] == 4 + 1 + 1 + 2


@gpu
@pytest.mark.parametrize("d", (255, 256))
def test_a_step_at_a_chunk_boundary_where_the_end_check_decides(d):
    """tile 3 of contig 0: a run of 255 cells at x, the next begin d behind it as the FIRST run of chunk 2.  255: the run abuts, no gap, the tile settles (chunk 2's
    first lane ends 21 cells beyond the reach: refused, the rule sweeps it).  256: one bare cell that the rebuild hides — the step is rebuilt as 0, chunk 2 is
    ACCEPTED with every begin 256 too small — and the end check alone keeps the tile from settling: it takes the window, the sums stay right."""
    j = 2 * CW
    c0 = int(candidates(base_first(), 0, 3)[0, 1])
    x = c0 + 3 * (j - 1)
    first = with_step(base_first(), 0, x, d, len_x=255)
    c = candidates(first, 0, 3)
    assert int(c[j, 1]) == x + d and int(c[j - 1, 1]) == x and int(c[j - 1, 2]) == x + 255
    b, ln = c[:, 1].astype(np.int64) - 3 * T, (c[:, 2] - c[:, 1]).astype(np.int64)
    n_full = c.shape[0] // CW
    assert sweep_tile(b, ln, 1) == ((SETTLED, n_full - 2) if d == 255 else (WINDOW, n_full - 1))
    bare = int((depths(LENS, first, NONE)[0] == 0).sum())
    assert bare == (0 if d == 255 else 1)
    run_case(LENS, first, NONE, 512)


@gpu
@pytest.mark.parametrize("every", (5, 8))
def test_runs_of_255_cells(every):
    """every 5 cells: 1740 candidates to a tile, three full chunks; every 8: 1088, two.  The chunks behind cell 0 are accepted, with sums of 512 * 255"""
    lens = [3 * T, 2 * T + 1]
    first = background(lens, every=every, length=255)
    out = run_case(lens, first, NONE, 512, grids=(2, 0))
    assert all(v > 0 for v in out.values()), out


@gpu
def test_the_sample_of_a_decode_session(dense_bam):
    """the sample of a PD_DECODE_COMPACT session (three batches; 150-base reads every 3 cells over tiles 6 .. 9 of contig 0 among short reads, one run per read):
    the dense tiles' middle chunks are accepted, the count is the model's on the kept reads in file order"""
    import bam_craft as B
    from test_gpu_decode_session import check_results, run_compact, windows_of
    f = dense_bam["narrow"]
    flt = B.FILTERS[0]
    dep = B.reference_depth(f["lens"], f["recs"], *flt)[0]
    kept = np.array([[r["tid"], int(B.runs_of(r)[0][0]), int(B.runs_of(r)[1][0])] for r in f["recs"] if B.kept(r, len(f["lens"]), *flt)], dtype=np.int64)
    kept = kept[np.lexsort((kept[:, 1], kept[:, 0]))]
    with pda.Engine(f["lens"]) as e:
        e.keep_deferred(True)
        e.set_param("direct_cover_min", 0)
        check_results(f, run_compact(e, f["cuts"]["3"], flt))
        assert e.profile_get("decode_end_compact")[1] == 1
        for w, md in ((W1, 1), (8192, 1), (W1, 0)):
            got = {}
            for fast_on in (1, 0):
                e.set_param("cover_fast", fast_on)
                _, cover, tot = e.scan_reduce_windows(w, md, 0)
                want = windows_of(f["lens"], dep, w, md)
                assert np.array_equal(cover, want[0]) and np.array_equal(tot, want[1]), (fast_on, w, md)
                assert e.profile_get("direct_cover_narrow")[1] == 1
                got[fast_on] = (e.profile_get("direct_cover_fast")[1], e.profile_get("direct_cover_settled")[1])
            want_fast, want_settled = model(f["lens"], kept, 512, w, md, 0)
            print((w, md), got, (want_fast, want_settled))
            assert got[0][0] == 0 and got[1][1] == got[0][1] == want_settled
            assert got[1][0] == want_fast and want_fast >= 4 * 3
        e.set_param("cover_fast", 1)
