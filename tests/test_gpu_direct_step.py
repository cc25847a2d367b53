"""One whole step of the direct path — pd_reset, pd_push_runs, pd_scan_reduce_windows — as it is after the call's small launches went:
the call's status words are two sets zeroed in turn by the gather of the call before, the gather stores the windows (and the words)
to the page-locked buffer itself, and the pile-up pass works beside k_direct_c8 from the list the sample made of its pile-up tiles;
and resets between direct steps, arrays steps, a direct export and the 12-byte direct path, each of which leaves other things for a
reset to zero.  Every table is compared with the numpy depth model of
tests/test_gpu_runs_planes.py and with the same call on a FRESH engine; samples, genomes and helpers are those of
tests/test_gpu_direct_call.py, tests/test_gpu_pileup_pass.py and tests/test_gpu_decode_session.py."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda
import bam_craft as B
import test_gpu_pileup_pass as PP
from test_gpu_cover_wave import dense
from test_gpu_direct_call import LENS, PILE, PILED, POSITIONS, TILE, Compact, _device, depth_ref, direct_call, fresh, same, sample, windows_ref
from test_gpu_runs_planes import oracle_depth, oracle_windows, sort_iv

gpu = pytest.mark.gpu

# (w, min_dep, wrap): every width with every min_dep and both wraps between them, not the whole product
CASES = [(8192, 0, 0), (8192, 3, 18), (3 * 8192 + 1, 1, 0), (3 * 8192 + 1, 0, 18), (10000000, 1, 18), (10000000, 3, 0)]
HEAVY = 32000                                            # more candidates than this: a pile-up tile
BUCKET = 512                                             # the default look-back


def pileup_tiles(lens, first, other):
    """The model's pile-up tiles, numbered like the engine's buffer (a contig's slot: len // 8192 + 1 tiles): those with more than 32 000
    candidates — runs that begin, clamped to their contig, in the tile or in the 512 cells before it, never across a contig's first cell."""
    iv = np.concatenate([first, other]).astype(np.int64)
    out, tile0 = [], 0
    for t, ln in enumerate(lens):
        b = np.clip(iv[iv[:, 0] == t][:, 1], 0, ln)
        n = ln // TILE + 1
        for k in range(n):
            lo = k * TILE - (BUCKET if k else 0)
            if int(((b >= lo) & (b < (k + 1) * TILE)).sum()) > HEAVY:
                out.append(tile0 + k)
        tile0 += n
    return np.array(out, dtype=np.uint32)


def arrays_step(e, first, other, w, md, wrap):
    """reset already done by the caller: the sample through the difference arrays"""
    ft, ot = _device(first, other)
    e.keep_deferred(False)
    e.profile(True)
    e.push_intervals_device(ft.data_ptr(), ft.shape[0], pda.PD_PUSH_SORTED)
    if ot.shape[0]:
        e.push_intervals_device(ot.data_ptr(), ot.shape[0], pda.PD_PUSH_DEFAULT)
    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
    assert e.profile_get("direct_tiles")[1] == 0 and e.profile_get("scatter_tiles")[1] == 1, "not the arrays path"
    e.profile(False)
    e.keep_deferred(True)
    return cover.copy(), tot.copy()


def check(got, position, w, md, wrap, what, lens=LENS):
    assert same(got, windows_ref(position, w, md, wrap, lens)), (what, "against the depth model", w, md, wrap)
    assert same(got, fresh(position, w, md, wrap, lens)), (what, "against a fresh engine", w, md, wrap)


# ---------------------------------------------------------------------------------------------------------------------
# pd_reset behind every kind of step
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,md,wrap", CASES)
def test_reset_between_direct_and_arrays_steps(w, md, wrap):
    """direct step -> reset -> arrays step -> reset -> direct step: the second reset must zero what the arrays step wrote (flags, tile sums)"""
    first, other = sample("tile0")
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            cover, tot, passes = direct_call(e, runs, w, md, wrap)
            assert passes == 1
            check((cover, tot), "tile0", w, md, wrap, "first direct step")
            e.reset()
            assert same(arrays_step(e, first, other, w, md, wrap), windows_ref("tile0", w, md, wrap)), "arrays step"
            cover, tot, passes = direct_call(e, runs, w, md, wrap)
            assert passes == 1
            check((cover, tot), "tile0", w, md, wrap, "direct step behind the arrays step")
            e.reset()
            assert same(arrays_step(e, first, other, w, md, wrap), windows_ref("tile0", w, md, wrap)), "second arrays step"


@gpu
@pytest.mark.parametrize("position", ["none", "tile0"])
def test_reset_behind_a_direct_export(position):
    """pd_export_i4's direct form writes the tile sums of a sample that stays deferred: the reset behind it has to zero them"""
    import torch
    dev = torch.device("cuda", 0)
    first, other = sample(position)
    w, md, wrap = CASES[2]
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            e.push_runs(runs, pda.PD_PUSH_MORE)
            n_cells, _ = e.device_layout()
            img = torch.zeros(n_cells // 2, dtype=torch.uint8, device=dev)
            exc = torch.zeros((8192, 2), dtype=torch.int64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            e.profile(True)
            e.export_i4(img.data_ptr(), exc.data_ptr(), 8192, cnt.data_ptr())
            e.synchronize()
            assert e.profile_get("direct_export")[1] == 1, "not the direct export"
            e.profile(False)
            e.reset()
            assert same(arrays_step(e, first, other, w, md, wrap), windows_ref(position, w, md, wrap)), "arrays step behind the export"
            cover, tot, _ = direct_call(e, runs, w, md, wrap)
            check((cover, tot), position, w, md, wrap, "direct step at the end")


@gpu
@pytest.mark.parametrize("w,md,wrap", [CASES[0], CASES[3], (128, 1, 0)])
def test_reset_behind_the_12_byte_direct_path(w, md, wrap):
    """no compact sample: the direct kernels of 12-byte runs build their index in the batch descriptors, which a reset zeroes"""
    first, other = sample("none")
    one = sort_iv(np.concatenate([first, other]))
    ft, _ = _device(one, other)
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        e.profile(True)
        e.push_intervals_device(ft.data_ptr(), ft.shape[0], pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
        _, cover, tot = e.scan_reduce_windows(w, md, wrap)
        assert e.profile_get("direct_tiles")[1] == 1 and e.profile_get("scatter_index")[1] == 1 and e.profile_get("scatter_tiles")[1] == 0
        e.profile(False)
        ref = oracle_windows(depth_ref("none"), w, md, wrap)
        assert same((cover, tot), ref), "12-byte direct path"
        e.reset()
        assert same(arrays_step(e, first, other, w, md, wrap), ref), "arrays step behind it"
        e.reset()


@gpu
def test_two_resets_in_a_row_on_a_fresh_engine():
    first, other = sample("adjacent")
    w, md, wrap = CASES[4]
    with pda.Engine(list(LENS)) as e:
        e.reset()
        e.reset()
        e.keep_deferred(True)
        assert same(arrays_step(e, first, other, w, md, wrap), windows_ref("adjacent", w, md, wrap))
        e.reset()
        e.reset()
        with Compact(e, first, other) as runs:
            cover, tot, _ = direct_call(e, runs, w, md, wrap)
            check((cover, tot), "adjacent", w, md, wrap, "direct step")


@gpu
def test_a_sorted_batch_alone_between_resets():
    """arrays step of ONE sorted batch (the owner-tile pass is the only writer of flags and tile sums), reset, the same again: sums left
    behind would be added to.  (A reset that launches nothing while the spans are clean was built and taken out — profiles/r14 —; these
    sequences are what such a skip has to survive.)"""
    first, other = sample("tile0")
    one = sort_iv(np.concatenate([first, other]))
    w, md, wrap = CASES[3]
    ref = windows_ref("tile0", w, md, wrap)
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            direct_call(e, runs, w, md, wrap)
            for k in range(2):
                e.reset()
                assert same(arrays_step(e, one, one[:0], w, md, wrap), ref), k
            e.profile(True)
            e.reset()
            e.reset()
            assert e.profile_get("reset")[1] == 2
            e.profile(False)
            cover, tot, _ = direct_call(e, runs, w, md, wrap)
            check((cover, tot), "tile0", w, md, wrap, "direct step at the end")


# ---------------------------------------------------------------------------------------------------------------------
# the status words: two sets in turn, the gather zeroes the next call's
# ---------------------------------------------------------------------------------------------------------------------
COVERED_LENS = (9 * TILE + 77, 2 * TILE)


@functools.lru_cache(maxsize=None)
def covered_sample():
    """a dense sample (the cover pass settles tiles of it) with one pile-up tile"""
    first, other = dense(list(COVERED_LENS), 5)
    pile = np.tile(np.array([[0, 4 * TILE + 300, 4 * TILE + 400]], dtype=np.int32), (PILE, 1))
    first = sort_iv(np.concatenate([first, pile]))
    return first, other, oracle_depth(list(COVERED_LENS), np.concatenate([first, other]))


@functools.lru_cache(maxsize=None)
def covered_fresh(w, md, wrap):
    first, other, _ = covered_sample()
    with pda.Engine(list(COVERED_LENS)) as e:
        e.keep_deferred(True)
        e.set_param("direct_cover_min", 0)
        with Compact(e, first, other) as runs:
            e.push_runs(runs, pda.PD_PUSH_MORE)
            _, cover, tot = e.scan_reduce_windows(w, md, wrap)
            return cover.copy(), tot.copy(), e.profile_get("direct_cover_settled")[1], e.profile_get("direct_pileup_tiles")[1]


def covered_call(e, w, md, wrap, what):
    first, other, dep = covered_sample()
    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
    f = covered_fresh(w, md, wrap)
    assert same((cover, tot), oracle_windows(dep, w, md, wrap)), (what, "against the depth model")
    assert same((cover, tot), f[:2]), (what, "against a fresh engine")
    if w >= TILE:
        assert e.profile_get("direct_pileup_tiles")[1] == 1 == f[3], what
        assert e.profile_get("direct_cover_settled")[1] == f[2], what
        if md <= 1: assert f[2] > 0, "the sample settles no tile: the count checks nothing"


@pytest.fixture(scope="module")
def covered_engine():
    first, other, _ = covered_sample()
    e = pda.Engine(list(COVERED_LENS))
    e.keep_deferred(True)
    e.set_param("direct_cover_min", 0)
    cs = Compact(e, first, other)
    yield e, cs.runs
    cs.__exit__()
    e.close()


@gpu
@pytest.mark.parametrize("w,md,wrap", CASES)
def test_three_direct_calls_without_a_reset(covered_engine, w, md, wrap):
    """odd and even sets: a set that is not zero when its call begins doubles the counts, and the call's check of the pile-up count fails"""
    e, runs = covered_engine
    e.reset()
    e.push_runs(runs, pda.PD_PUSH_MORE)
    for k in range(3):
        covered_call(e, w, md, wrap, "call %d" % k)
    e.reset()


@gpu
@pytest.mark.parametrize("between", ["narrow", "grown", "failed", "other_width", "arrays"])
def test_a_call_of_another_kind_between_two_wide_ones(covered_engine, between):
    """behind a call that zeroed no set for its successor — narrow windows (no gather), a result that outgrows the kept buffer, arguments
    that fail, windows of another width (the sets lie elsewhere), a call through the arrays — the next wide call still counts from zero"""
    e, runs = covered_engine
    w, md, wrap = CASES[2]
    e.reset()
    e.push_runs(runs, pda.PD_PUSH_MORE)
    covered_call(e, w, md, wrap, "before")
    covered_call(e, w, md, wrap, "before, the other set")
    if between in ("narrow", "grown"):                   # (w = 64: more windows than the kept buffer holds)
        covered_call(e, 4096 if between == "narrow" else 64, 1, 0, between)
        e.reset()                                         # (narrow windows expanded the pending sample to 12-byte runs: pushed again, it is compact again)
        e.push_runs(runs, pda.PD_PUSH_MORE)
    elif between == "failed":
        with pytest.raises(pda.PdError):
            e.scan_reduce_windows(w, md, 33)
        with pytest.raises(pda.PdError):
            e.scan_reduce_windows(0, md, wrap)
    elif between == "other_width":
        covered_call(e, 8192, 1, 0, "w = 8192")
    else:
        first, other, dep = covered_sample()
        e.reset()
        assert same(arrays_step(e, first, other, w, md, wrap), oracle_windows(dep, w, md, wrap))
        e.reset()
        e.push_runs(runs, pda.PD_PUSH_MORE)
    for k in range(3):
        covered_call(e, w, md, wrap, "behind, call %d" % k)
    e.reset()


# ---------------------------------------------------------------------------------------------------------------------
# the gather writes what the host reads
# ---------------------------------------------------------------------------------------------------------------------
N_BIG = 87400                                            # windows of a tile: 12 bytes each and the words are just above the page-locked buffer's 1 MiB
BIG = (N_BIG * TILE - 5,)


@functools.lru_cache(maxsize=None)
def big_sample():
    """runs at both ends of a 716 Mb contig and a pile-up in its last whole tile; everything between is empty"""
    rng = np.random.default_rng(11)
    near = np.sort(rng.integers(-5, 4 * TILE, 3000))
    far = np.sort(rng.integers(BIG[0] - 4 * TILE, BIG[0] + 30, 3000))
    pile = np.full(PILE, (N_BIG - 2) * TILE + 17)
    beg = np.sort(np.concatenate([near, far, pile]))
    first = np.stack([np.zeros_like(beg), beg, beg + 150], axis=1).astype(np.int32)
    other = first[::7].copy()
    other[:, 1] += 200; other[:, 2] += 260
    return first, other


def big_windows(w, md):
    """the model on the contig's two ends only: between them the depth is zero"""
    first, other = big_sample()
    edge = 6 * TILE                                          # (whole windows of either width)
    iv = np.concatenate([first, other]).astype(np.int64)
    head = oracle_depth([edge], iv[iv[:, 1] < edge])[0]
    tail_iv = iv[iv[:, 1] >= edge].copy()
    base = BIG[0] - edge - (BIG[0] - edge) % w               # a window boundary in front of the tail's first run
    assert int(tail_iv[:, 1].min()) >= base
    tail_iv[:, 1:] -= base
    tail = oracle_depth([BIG[0] - base], tail_iv)[0]
    nw = (BIG[0] + w - 1) // w
    cover, tot = np.zeros(nw, dtype=np.uint32), np.zeros(nw, dtype=np.uint64)
    if md == 0: cover[:] = w                                 # every cell of an empty window is at depth 0
    c, t = oracle_windows([head], w, md, 0)
    cover[:c.size] = c; tot[:t.size] = t
    c, t = oracle_windows([tail], w, md, 0)
    cover[base // w:] = c; tot[base // w:] = t
    return cover, tot


@gpu
def test_results_through_the_page_locked_buffer_and_above_it():
    """w = 8192 on 87 400 tiles: 1 048 800 bytes of results, above the 1 MiB that go through the page-locked buffer (three copies);
    w = 16384: half of it, stored there by the gather.  Twice each: both sets of status words."""
    first, other = big_sample()
    with pda.Engine(list(BIG)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            assert list(e.runs_pileup_tiles(runs)) == [N_BIG - 2]
            for w, md in ((8192, 1), (16384, 1), (8192, 3), (16384, 0)):
                assert (N_BIG * 12 > (1 << 20)) and (N_BIG // 2 * 12 + 128 < (1 << 20))
                want = big_windows(w, md)
                for k in range(2):
                    cover, tot, passes = direct_call(e, runs, w, md, 0)
                    assert passes == 1 and cover.size == (BIG[0] + w - 1) // w
                    assert same((cover, tot), want), (w, md, k)
                    assert e.profile_get("direct_pileup_tiles")[1] == 1


def rows_of(tid, w, woff, cov_ref, tot_ref):
    """the rows of the `-w` table for contig tid, formatted from the model's windows"""
    rows = []
    for k in range(int(woff[tid + 1] - woff[tid])):
        j = 1 + k * w
        end = min(j - 1 + w, LENS[tid])
        ln = end - j + 1
        c, d = int(cov_ref[int(woff[tid]) + k]), int(tot_ref[int(woff[tid]) + k])
        rows.append("c%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.2f\n" % (tid, j, end, ln, c, d, c * 100.0 / ln, d * 1.0 / ln))
    return rows


def kept_rows_are(e, w, what):
    """every contig's rows, formatted by the device from the kept windows of the last call, are the model's"""
    cov_ref, tot_ref = windows_ref("tile0", w, 1, 0)
    woff = e.window_layout(w)
    with e.text_open(1 << 20) as t:
        at = 0
        for tid in range(len(LENS)):
            rows = rows_of(tid, w, woff, cov_ref, tot_ref)
            want = "".join(rows).encode()
            assert t.append_window_rows(tid, w, 0, len(rows), "c%d" % tid) == len(want), (what, tid)
            assert t.read(at, len(want)) == want, (what, tid)
            at += len(want)


def kept_rows_are_refused(e, w, what):
    with e.text_open(1 << 20) as t:
        for tid in range(len(LENS)):
            try:
                t.append_window_rows(tid, w, 0, 1, "c%d" % tid)
            except pda.PdError:
                continue
            raise AssertionError("rows of width %d were served %s" % (w, what))


@gpu
@pytest.mark.parametrize("w", [8192, 3 * 8192 + 1])
def test_the_kept_windows_are_what_the_text_rows_come_from(w):
    """pd_text_append_window_rows formats from the device's copy of the last call's windows, which the gather still writes beside the
    page-locked buffer: the rows of the `-w` table, formatted here from the model's windows — behind every producer that commits its
    windows (the direct wide call, a direct narrow call on 12-byte runs, the arrays path, pd_reduce_windows behind pd_scan), and refused
    behind pd_reset, a call of another width and a call that failed on its arguments"""
    first, other = sample("tile0")
    ref = windows_ref("tile0", w, 1, 0)
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            for call in range(2):                        # (the second call finds the other set, and every buffer in place)
                cover, tot, passes = direct_call(e, runs, w, 1, 0)
                assert passes == 1 and same((cover, tot), ref)
                kept_rows_are(e, w, "direct wide call %d" % call)
            kept_rows_are_refused(e, 4096, "behind a call of another width")
            kept_rows_are_refused(e, w + 1, "behind a call of another width")
            with pytest.raises(pda.PdError):             # wrap_bits
                e.scan_reduce_windows(w, 1, 33)
            kept_rows_are_refused(e, w, "behind a call that failed on its arguments")
            cover, tot, passes = direct_call(e, runs, 4096, 1, 0)             # narrow windows: the sample goes on as 12-byte runs, no gather
            assert passes == 1 and same((cover, tot), windows_ref("tile0", 4096, 1, 0))
            kept_rows_are(e, 4096, "direct narrow call")
            kept_rows_are_refused(e, w, "behind a call of another width")
            e.reset()
            kept_rows_are_refused(e, 4096, "behind pd_reset")
            assert same(arrays_step(e, first, other, w, 1, 0), ref)
            kept_rows_are(e, w, "arrays path")
            e.reset()
            kept_rows_are_refused(e, w, "behind pd_reset")
            ft, ot = _device(first, other)
            e.keep_deferred(False)
            e.push_intervals_device(ft.data_ptr(), ft.shape[0], pda.PD_PUSH_SORTED)
            e.push_intervals_device(ot.data_ptr(), ot.shape[0], pda.PD_PUSH_DEFAULT)
            e.scan(0)
            kept_rows_are_refused(e, w, "behind pd_scan alone")
            _, cover, tot = e.reduce_windows(w, 1)
            assert same((cover, tot), ref)
            kept_rows_are(e, w, "pd_reduce_windows behind pd_scan")
            e.keep_deferred(True)


# ---------------------------------------------------------------------------------------------------------------------
# the pile-up pass works from the sample's own list
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("position", PILED)
def test_the_list_of_every_piled_position(position):
    first, other = sample(position)
    want = pileup_tiles(LENS, first, other)
    assert want.size == len(POSITIONS[position])
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        with Compact(e, first, other) as runs:
            got = e.runs_pileup_tiles(runs)
            assert got.size == want.size and set(got.tolist()) == set(want.tolist())
            for w, md, wrap in CASES:
                cover, tot, passes = direct_call(e, runs, w, md, wrap)
                assert passes == 1 and e.profile_get("direct_pileup_tiles")[1] == want.size
                check((cover, tot), position, w, md, wrap, position)


@gpu
@pytest.mark.parametrize("name", sorted(PP.SAMPLES))
def test_the_list_of_every_pile_up_sample(name):
    first, other, _ = PP.sample_of(name)
    want = pileup_tiles(PP.LENS, first, other)
    assert want.size == PP.SAMPLES[name]
    with pda.Engine(PP.LENS) as e, pda.Engine(PP.LENS) as ef:
        for x in (e, ef):
            x.keep_deferred(True)
        with Compact(e, first, other) as runs, Compact(ef, first, other) as runs_f:
            got = e.runs_pileup_tiles(runs)
            assert got.size == want.size and set(got.tolist()) == set(want.tolist())
            for k, (w, md, wrap) in enumerate(CASES):
                cover, tot, _ = direct_call(e, runs, w, md, wrap)
                assert e.profile_get("direct_pileup_tiles")[1] == want.size
                assert same((cover, tot), PP.windows_of(name, w, md, wrap)), (name, w, md, wrap)
                if k < 2:                                 # (the other engine does nothing but these two calls)
                    assert same((cover, tot), direct_call(ef, runs_f, w, md, wrap)[:2]), ("fresh", name, w, md, wrap)


@pytest.fixture(scope="module")
def piled_bam(tmp_path_factory):
    """a crafted BAM with 32 001 records that begin on one cell of contig 0's tile 2, among short reads"""
    rng = np.random.default_rng(3)
    pile = [(0, 2 * TILE + 1000, 0, 60, b"p%05d" % k, B.pack([(B.M, 100)]), 100, b"") for k in range(HEAVY + 1)]
    recs = sorted(pile + B.short_reads(rng, 3000), key=B._sort_key)
    path = str(tmp_path_factory.mktemp("piled") / "piled.bam")
    blocks, inf, offs = B.write_bam(path, B.NAMES, B.LENS, recs, member_size=24000)
    lens, parsed = B.parse_bam(inf)
    f = dict(path=path, blocks=blocks, inf=inf, offs=offs, lens=lens, recs=parsed, data=open(path, "rb").read())
    f["cuts"] = B.session_cuts(f, "piled")
    return f


@gpu
@pytest.mark.parametrize("cut", ["1", "3"])
def test_the_list_of_a_decode_session(piled_bam, cut):
    """the sample a PD_DECODE_COMPACT session leaves lists its pile-up tile too (pd_decode_end goes through the same finish), and the direct
    call's tables and the per-base depth are the reference's"""
    from test_gpu_decode_session import check_depth, check_results, run_compact, windows_of
    f = piled_bam
    flt = B.FILTERS[0]
    dep, n_kept, _ = B.reference_depth(f["lens"], f["recs"], *flt)
    assert int(dep[0][2 * TILE + 1050]) >= HEAVY + 1
    kept = np.array([[r["tid"], r["pos"], r["pos"] + 100] for r in f["recs"] if B.kept(r, len(f["lens"]), *flt)], dtype=np.int32)
    want = pileup_tiles(f["lens"], kept, np.zeros((0, 3), dtype=np.int32))
    assert want.tolist() == [2]
    with pda.Engine(f["lens"]) as e:
        e.keep_deferred(True)
        e.profile(True)
        check_results(f, run_compact(e, f["cuts"][cut], flt))
        assert e.profile_get("decode_end_compact")[1] == 1
        assert e.runs_pileup_tiles().tolist() == want.tolist()
        for k in range(2):
            for w, md in ((8192, 1), (3 * 8192 + 1, 3), (10000000, 0)):
                _, cover, tot = e.scan_reduce_windows(w, md, 0)
                assert e.profile_get("direct_pileup_tiles")[1] == 1
                assert same((cover, tot), windows_of(f["lens"], dep, w, md)), (w, md, k)
        e.profile(False)
        check_depth(e, f["lens"], dep)


@gpu
def test_destroy_and_reset_right_behind_a_direct_call():
    """the lifetime across the join: pd_reset and pd_runs_destroy right behind a call whose pile-up pass ran on the side stream free what it
    read; a new sample on the same engine, with its pile-ups elsewhere, then gives its own tables"""
    w, md, wrap = CASES[2]
    with pda.Engine(list(LENS)) as e:
        e.keep_deferred(True)
        for position in ("adjacent", "tile0", "behind_seam", "none", "last_partial"):
            first, other = sample(position)
            ft, ot = _device(first, other)
            runs = e.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
            e.push_runs(runs, pda.PD_PUSH_MORE)
            _, cover, tot = e.scan_reduce_windows(w, md, wrap)
            e.reset()
            e.runs_destroy(runs)
            got = (cover.copy(), tot.copy())
            check(got, position, w, md, wrap, position)
