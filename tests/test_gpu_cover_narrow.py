"""The NARROW form of k_direct_c8's cover pass: a tile's sorted candidates are swept from the nar plane — two bytes per run, (begin & 0xFF) |
(min(len, 255) << 8), written beside lo | hi by every producer of a sorted stream — with the begins rebuilt from the differences of their low
bytes and an END CHECK that says whether the rebuild was exact (pandepth_amd/csrc/pd_cover_rule.h; on the CPU: tests/test_cover_narrow_rule.py).
launch_direct_c8 takes the form when the cover form would run, the sample has no sorted run above 255 cells (pd_runs::n_wide_sorted) and
pd_set_param("cover_narrow") is not 0; pd_profile_get("direct_cover_narrow") says whether the last call took it.

Every case is compared element for element with a numpy difference-array reference, the arrays path, the same call with "cover_narrow" 0 (the wide
form) and with "direct_cover" 0 (no pass), walked by one workgroup, by two and by the default grid; "direct_cover_settled" must equal the wide form's
wherever the end check passes on every tile, and be lower by exactly the tiles on which it cannot."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
from test_gpu_cover_wave import covered_by_sorted, depths, interior, windows
from test_gpu_direct_cover import T, _create, _device, sort_iv

gpu = pytest.mark.gpu

CW = 512                                                 # sorted runs per chunk of the narrow sweep (pd_direct.hip: k_direct_c8, NARROW)
W1 = 10000000
LENS = [9 * T + 5, 3 * T]                                # contig 0: tiles 0 .. 8 whole (first flat cells 57344 and 65536 among them) + 5 cells; contig 1: tiles 10 .. 12
NONE = np.zeros((0, 3), dtype=np.int32)
GRIDS = (1, 2, 0)


def background(lens, every=3, length=150):
    """a run of `length` cells every `every` cells of every contig, from its first cell on"""
    f = []
    for tid, ln in enumerate(lens):
        beg = np.arange(0, ln, every)
        f.append(np.stack([np.full(beg.size, tid), beg, beg + length], axis=1))
    return sort_iv(np.concatenate(f).astype(np.int32))


def with_step(first, tid, x, d, len_x=100, len_y=150):
    """the runs of contig tid that begin in [x, x + d) replaced by one at x; then one at x + d: two consecutive begins that differ by exactly d"""
    keep = first[~((first[:, 0] == tid) & (first[:, 1] >= x) & (first[:, 1] < x + d))]
    return sort_iv(np.concatenate([keep, np.array([[tid, x, x + len_x], [tid, x + d, x + d + len_y]], dtype=np.int32)]))


def run_case(lens, first, other, lmax, narrow_expected=1, grids=GRIDS, ws=(W1, 8192), modes=((1, 0), (0, 0))):
    """-> {(grid, w, min_dep, wrap): (tiles the narrow form settled, tiles the wide form settled)}"""
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
                key = (grid, w, md, wrap)
                settled = {}
                for form, (cover_on, narrow_on) in (("narrow", (1, 1)), ("wide", (1, 0)), ("window", (0, 1))):
                    e.set_param("direct_cover", cover_on)
                    e.set_param("cover_narrow", narrow_on)
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                    assert np.array_equal(cover, r[0]) and np.array_equal(tot, r[1]), (form, key)
                    settled[form] = e.profile_get("direct_cover_settled")[1]
                    took = e.profile_get("direct_cover_narrow")[1]
                    assert took == (narrow_expected if form == "narrow" else 0), (form, key, took)
                assert settled["window"] == 0, key
                out[key] = (settled["narrow"], settled["wide"])
        e.set_param("direct_cover", 1); e.set_param("cover_narrow", 1)
        e.reset()
        e.runs_destroy(runs)
    return out


def gaps_below_256(lens, first, lmax):
    """per interior tile: do all consecutive begins of its sorted candidates (its own cells and the bucket of lmax cells before it) differ by less than 256?"""
    ok = []
    for tid, ln in enumerate(lens):
        b = first[first[:, 0] == tid][:, 1].astype(np.int64)
        for k in range(ln // T):
            c = b[(b >= max(k * T - lmax, 0)) & (b < (k + 1) * T)]
            ok.append(bool(c.size < 2 or int(np.diff(c).max()) < 256))
    return ok


def tiles_covered(lens, first):
    out = []
    for t, d in enumerate(depths(lens, first, NONE)):
        out += [bool(d[k * T:(k + 1) * T].min() >= 1) for k in range(lens[t] // T)]
    return out


def expect(lens, first, lmax):
    """(tiles the wide form settles for min_dep 1, tiles the narrow form does, interior tiles whose end check fails)"""
    cov, ok = tiles_covered(lens, first), gaps_below_256(lens, first, lmax)
    return sum(cov), sum(c and o for c, o in zip(cov, ok)), sum(not o for o in ok)


def check_settled(out, lens, first, lmax, grids=GRIDS):
    wide, narrow, failing = expect(lens, first, lmax)
    assert wide == covered_by_sorted(lens, first)
    for grid in grids:                                   # (no case here has four declined tiles in a row: the gate stays open, whatever the grid)
        assert out[(grid, W1, 1, 0)] == (narrow, wide), (grid, out[(grid, W1, 1, 0)], narrow, wide)
        # min_dep 0: every interior tile settles with its sum — but for the tiles the narrow form could not rebuild
        assert out[(grid, W1, 0, 0)] == (interior(lens) - failing, interior(lens)), (grid, out[(grid, W1, 0, 0)])
    return wide, narrow, failing


@functools.lru_cache(maxsize=None)
def base_first():
    f = background(LENS)
    f.setflags(write=False)
    return f


@gpu
def test_the_dense_background_settles_every_interior_tile_in_the_narrow_form():
    first = base_first()
    rng = np.random.default_rng(5)
    k = rng.random(first.shape[0]) < 0.1
    other = first[k].copy()
    other[:, 1] += 160 + rng.integers(0, 300, other.shape[0]).astype(np.int32)
    other[:, 2] = other[:, 1] + rng.integers(0, 250, other.shape[0]).astype(np.int32)
    other = other[rng.permutation(other.shape[0])]
    out = run_case(LENS, first, other, 512, ws=(W1, 8192, 10000))
    assert check_settled(out, LENS, first, 512) == (interior(LENS), interior(LENS), 0)


STEPS = (0, 1, 255, 256, 257, 512)


@gpu
@pytest.mark.parametrize("d", STEPS)
def test_a_step_among_the_runs_before_cell_0(d):
    """tile 7 (flat 57344) of contig 0, buckets of 2048 cells: two of its look-back candidates begin d cells apart, the tile itself is covered, so only the
    end check stands between the rebuild and a wrong sum.  (Tile 6, whose own runs they are, has the gap that d opens.)"""
    first = with_step(base_first(), 0, 7 * T - 1400, d)
    out = run_case(LENS, first, NONE, 2048)
    wide, narrow, failing = check_settled(out, LENS, first, 2048)
    assert tiles_covered(LENS, first)[7] and failing == (2 if d >= 256 else 0)          # tiles 6 and 7 see the step
    assert wide - narrow == (1 if d >= 256 else 0)                                       # ... and tile 7 is the covered one of them


@gpu
@pytest.mark.parametrize("d", STEPS)
def test_a_step_inside_the_tile(d):
    """tile 8 (flat 65536), the first of its group: beyond the run's 100 cells (and the 150 of the runs before it) the step is a true gap — the tile is
    declined in both forms, by the gap itself, and the three tiles behind it in the group settle"""
    first = with_step(base_first(), 0, 8 * T + 3000, d)
    out = run_case(LENS, first, NONE, 512)
    wide, narrow, failing = check_settled(out, LENS, first, 512)
    assert tiles_covered(LENS, first)[8] == (d <= 1) and wide == narrow
    assert failing == (1 if d >= 256 else 0)


@gpu
def test_a_step_of_256_that_only_the_rebuild_would_close():
    """a run of 255 cells and the next begin 256 behind it, nothing else over that cell: ONE uncovered cell, and rebuilt without the end check the second
    run would begin where the first does.  min_dep 0 as well: the sum of a tile whose begins were rebuilt wrong must not be used."""
    x = 8 * T + 3000
    first = with_step(base_first(), 0, x, 256, len_x=255)      # (the runs that begin before x end before x + 150)
    d = depths(LENS, first, NONE)[0]
    assert int((d == 0).sum()) == 1 and int(d[x + 255]) == 0
    out = run_case(LENS, first, NONE, 512)
    assert check_settled(out, LENS, first, 512) == (interior(LENS) - 1, interior(LENS) - 1, 1)


@gpu
@pytest.mark.parametrize("length", (0, 1, 254, 255))
def test_every_run_of_one_length(length):
    lens = [3 * T, 2 * T + 1]
    first = background(lens, every=1 if length <= 1 else 200, length=length)
    out = run_case(lens, first, NONE, 512, grids=(2, 0))
    wide, narrow, failing = check_settled(out, lens, first, 512, grids=(2, 0))
    assert failing == 0 and wide == (interior(lens) if length else 0)


@gpu
@pytest.mark.parametrize("where", ("sorted", "other"))
def test_a_run_of_256_cells(where):
    """in the sorted stream: the sample counts it (n_wide_sorted = 1) and the WIDE form is the one launched, whatever "cover_narrow" says; in the other
    stream only: the narrow form stays (the other stream is read from lo)"""
    long_run = np.array([[0, 2 * T + 77, 2 * T + 77 + 256]], dtype=np.int32)
    first = base_first()
    if where == "sorted":
        first = sort_iv(np.concatenate([first, long_run]))
    out = run_case(LENS, first, long_run if where == "other" else NONE, 512, narrow_expected=0 if where == "sorted" else 1, grids=(0,))
    assert out[(0, W1, 1, 0)] == (interior(LENS), interior(LENS))


COUNTS = (1, 7, 8, 9, 17, CW - 1, CW, CW + 1, 2 * CW - 1, 2 * CW, 2 * CW + 1, 3 * CW, 3 * CW + 1)


@functools.lru_cache(maxsize=None)
def counts_sample():
    """one contig; tile 1: dense (so that no later tile's candidates end inside the plane's first eight half-words); then, every other tile, a tile of
    exactly n sorted candidates, and the same with its middle run a cell short, for each n of COUNTS: from 33 runs on they abut and cover the tile, fewer
    runs (200 cells each) cannot.  The tiles between hold nothing: no tile has candidates from the bucket before it."""
    f = [background([T], every=3, length=150) + np.array([0, T, T], dtype=np.int32)]
    covered, t = 1, 3
    for n in COUNTS:
        for hole in (False, True):
            b = [t * T + ((i * T) // n if n >= 33 else i * 200) for i in range(n + 1)]
            f.append(np.array([[0, b[i], b[i + 1] - (1 if hole and i == n // 2 else 0)] for i in range(n)], dtype=np.int32))
            covered += 1 if n >= 33 and not hole else 0
            t += 2
    return [t * T], sort_iv(np.concatenate(f)), covered


@gpu
def test_sorted_candidate_counts_around_the_chunk_size():
    lens, first, covered = counts_sample()
    assert int((first[:, 2] - first[:, 1]).max()) <= 255
    out = run_case(lens, first, NONE, 512)
    # (the empty tiles and those of fewer than 33 runs decline one after the other: one or two workgroups walking them close their gates — the same way in
    # both forms, no end check fails here)
    assert check_settled(out, lens, first, 512, grids=(0,)) == (covered, covered, 0)
    assert all(n == w for n, w in out.values())


@gpu
def test_the_first_tile_s_sorted_stream_ends_inside_the_first_eight_half_words():
    """tile 0 has 3 sorted candidates (the plane's first three half-words: no 16-byte load fits in front of their end) and takes the window path; the
    tiles behind it are swept"""
    rest = background([3 * T], every=3, length=150)
    rest = rest[rest[:, 1] >= T + 600]
    first = sort_iv(np.concatenate([np.array([[0, 10, 200], [0, 100, 300], [0, 250, 500]], dtype=np.int32), rest]))
    other = np.array([[0, 5, 50], [0, 2 * T + 9, 2 * T + 99]], dtype=np.int32)
    out = run_case([3 * T], first, other, 512)
    for grid in GRIDS:
        assert out[(grid, W1, 1, 0)] == (1, 1)             # tile 2; tile 1's first 600 cells are bare
        assert out[(grid, W1, 0, 0)] == (2, 2)             # ... and tile 1 with its sum; tile 0 is never tried


@gpu
def test_tiles_with_other_stream_candidates_only_and_with_none():
    """tile 1: runs of the other stream only (they cover it: what they cover is ignored, their lengths count); tile 2: nothing at all; tiles 0 and 3 dense"""
    lens = [4 * T]
    bg = background(lens)
    first = bg[(bg[:, 1] < T - 600) | (bg[:, 1] >= 3 * T)]
    other = bg[(bg[:, 1] >= T) & (bg[:, 1] < 2 * T - 600)][::-1].copy()
    out = run_case(lens, first, other, 512)
    for grid in GRIDS:
        assert out[(grid, W1, 1, 0)] == (1, 1)             # tile 3 (tile 0's last cells are bare)
        assert out[(grid, W1, 0, 0)] == (4, 4)


@gpu
def test_the_largest_span_of_a_tile_s_candidates():
    """the widest buckets there are (4096 cells, "lmax" 4096): tile 7's first sorted candidate begins one full bucket before it, its last at cell 8191"""
    first = sort_iv(np.concatenate([base_first(), np.array([[0, 7 * T - 4096, 7 * T - 4096 + 255], [0, 8 * T - 1, 8 * T]], dtype=np.int32)]))
    c = first[(first[:, 0] == 0) & (first[:, 1] >= 7 * T - 4096) & (first[:, 1] < 8 * T)][:, 1]
    assert int(c.min()) == 7 * T - 4096 and int(c.max()) == 8 * T - 1
    out = run_case(LENS, first, NONE, 4096, grids=(2, 0))
    assert check_settled(out, LENS, first, 4096, grids=(2, 0)) == (interior(LENS), interior(LENS), 0)


@pytest.fixture(scope="module")
def dense_bam(tmp_path_factory):
    """a crafted sorted BAM: 150-base reads every 3 cells over tiles 6 .. 9 of contig 0 (flat 57344 and 65536 among their first cells), among short
    reads; `wide`: the same with one read of 256 bases"""
    import bam_craft as B
    rng = np.random.default_rng(11)
    out = {}
    for name in ("narrow", "wide"):
        recs = [(0, x, 0, 60, b"d%06d" % x, B.pack([(B.M, 150)]), 150, b"") for x in range(6 * T - 600, 10 * T, 3)] + B.short_reads(rng, 2000)
        if name == "wide":
            recs.append((0, 7 * T + 100, 0, 60, b"w", B.pack([(B.M, 256)]), 256, b""))
        recs = sorted(recs, key=B._sort_key)
        path = str(tmp_path_factory.mktemp(name) / "dense.bam")
        blocks, inf, offs = B.write_bam(path, B.NAMES, B.LENS, recs, member_size=24000)
        lens, parsed = B.parse_bam(inf)
        f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=parsed, data=open(path, "rb").read())
        f["cuts"] = B.session_cuts(f, name)
        out[name] = f
    return out


@gpu
@pytest.mark.parametrize("name", ("narrow", "wide"))
def test_the_sample_of_a_decode_session(dense_bam, name):
    """the narrow plane of a PD_DECODE_COMPACT session's sample is written where its batches' first runs are placed (k_copy_planes_nar, three batches),
    and the runs it cannot hold are counted there: tiles 6 .. 9 settle in the narrow form; with one read of 256 bases the wide form is launched"""
    import bam_craft as B
    from test_gpu_decode_session import check_results, run_compact, windows_of
    f = dense_bam[name]
    flt = B.FILTERS[0]
    dep = B.reference_depth(f["lens"], f["recs"], *flt)[0]
    with pda.Engine(f["lens"]) as e:
        e.keep_deferred(True)
        e.set_param("direct_cover_min", 0)
        check_results(f, run_compact(e, f["cuts"]["3"], flt))
        assert e.profile_get("decode_end_compact")[1] == 1
        settled = {}
        for form, (cover_on, narrow_on) in (("narrow", (1, 1)), ("wide", (1, 0)), ("window", (0, 1))):
            e.set_param("direct_cover", cover_on)
            e.set_param("cover_narrow", narrow_on)
            for w, md in ((W1, 1), (8192, 1), (W1, 0)):
                _, cover, tot = e.scan_reduce_windows(w, md, 0)
                want = windows_of(f["lens"], dep, w, md)
                assert np.array_equal(cover, want[0]) and np.array_equal(tot, want[1]), (form, w, md)
                assert e.profile_get("direct_cover_narrow")[1] == (1 if form == "narrow" and name == "narrow" else 0), (form, w, md)
                settled[(form, w, md)] = e.profile_get("direct_cover_settled")[1]
        assert settled[("narrow", W1, 1)] == settled[("wide", W1, 1)] == 4 and settled[("window", W1, 1)] == 0
        # min_dep 0: the wide form settles every interior tile with its sum; the narrow form those whose sorted candidates it could rebuild (the thin
        # tiles around the dense ones have begins 256 cells apart and more) — or as many, where the wide form is what "narrow" launched
        kept = np.array([[r["tid"], r["pos"], r["pos"]] for r in f["recs"] if B.kept(r, len(f["lens"]), *flt)], dtype=np.int64)
        failing = sum(not ok for ok in gaps_below_256(f["lens"], kept[np.lexsort((kept[:, 1], kept[:, 0]))], 512))
        assert failing > 0 and settled[("wide", W1, 0)] == interior(f["lens"])
        assert settled[("narrow", W1, 0)] == interior(f["lens"]) - (failing if name == "narrow" else 0)
