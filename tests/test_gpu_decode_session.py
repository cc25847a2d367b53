"""The batched decode session (pd_decode_begin / acquire / submit | queue + collect / end | abort: include/pandepth_amd.h,
pandepth_amd/csrc/pd_decode.hip) called directly, on the crafted corpus of tests/bam_craft.py cut into batches the way the executable's
readers cut a file (bam_craft.cut_batches; held to the file on the CPU in tests/test_decode_batches.py), against the per-base depth of
the reference written from the SAM specification (bam_craft.reference_depth).  Every comparison is of exact integers, per base or per
window; no unit may be handed back except where a guessed start lies inside a decoy record.

Which branch of pd_decode.hip a group reaches is shown by the session's counters (pd_profile_get "decode_*": which way pd_decode_end
went, who confirmed the record chains, how often the compact sample grew), by the kernels' launch counts, by a status or by the
library's own message."""
import ctypes
import re

import numpy as np
import pytest

import bam_craft as B
import pandepth_amd as pda
from pandepth_amd.capi import PD_DECODE_COMPACT, PD_NONE, PD_UNIT_GUESS

pytestmark = pytest.mark.gpu
SORTED_FILES = ["alone", "packed", "layout", "few"]
CUTS = [(n, c) for n in SORTED_FILES for c in ("1", "3", "16")] + [("layout", "crafted")]
MODES = ["plain", "queued", "compact"]
WINDOWS = [(w, m) for w in (8192, 10000) for m in (1, 3)]
PD_EINVAL, PD_ESTATE = -1, -4


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once per file, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------
def windows_of(lens, dep, w, min_dep):
    cov, tot = [], []
    for t, ln in enumerate(lens):
        x = np.zeros(ln, dtype=np.uint64) if dep[t] is None else dep[t].astype(np.uint64)
        for s in range(0, ln, w):
            seg = x[s:min(s + w, ln)]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


def freeze(dep):
    for x in dep:
        if x is not None:
            x.setflags(write=False)
    return dep


def add_depth(a, b):
    return [None if x is None else x + y for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    files = B.build_corpus(tmp_path_factory.mktemp("session"))       # (asserts that every named case is present)
    _, seg, _ = B.walk_geometry()
    for name, f in list(files.items()):
        f["name"] = name
        f["depth"] = {flt: freeze(B.reference_depth(f["lens"], f["recs"], *flt)[0]) for flt in B.FILTERS}
        f["windows"] = {(flt, w, m): windows_of(f["lens"], f["depth"][flt], w, m) for flt in B.FILTERS for w, m in WINDOWS}
        f["cuts"] = B.session_cuts(f, name)        # (the batches tests/test_decode_batches.py holds to the file on the CPU)
    files["long_decoy"] = B.long_decoy_file(tmp_path_factory.mktemp("long_decoy"), seg)
    return files


# ---------------------------------------------------------------------------------------------------------------------
# running a session
# ---------------------------------------------------------------------------------------------------------------------
def as_batch(b, order=None):
    return (b["data"], b["blocks"], b["units"], b["inflated"], b["order"] if order is None else order)


def empty_batch(order):
    return (b"", [], [], 0, order)


def counter(e, name):
    return e.profile_get(name)[1]


def run_plain(e, batches, flt, queued=False, **cfg):
    """-> [(status, result)] in file order.  queued: two batches in flight at a time, collected in reverse arrival order."""
    s = e.decode_session()
    s.begin(flt[0], flt[1], sorted=cfg.pop("sorted", 1), bytes_hint=sum(len(b["data"]) for b in batches), **cfg)
    out = [None] * len(batches)
    if not queued:
        for k, b in enumerate(batches):
            s.acquire(len(b["data"]))
            out[k] = s.submit(as_batch(b))
    else:
        for k in range(0, len(batches), 2):
            pair = list(range(k, min(k + 2, len(batches))))
            tickets = []
            for j in pair:
                s.acquire(len(batches[j]["data"]))
                tickets.append(s.queue(as_batch(batches[j])))
            for j, t in reversed(list(zip(pair, tickets))):
                out[j] = s.collect(t, len(batches[j]["units"]))
    s.end()
    return out


def run_compact(e, batches, flt, **cfg):
    """A PD_DECODE_COMPACT session of len(batches) + 1 orders: one order in the middle is an empty batch, the orders arrive pairwise
    swapped (1, 0, 3, 2, ...); the buffers of a pair are acquired before its orders are taken (pd_decode_cfg::n_batches).
    -> [(status, result)] of the real batches in file order"""
    n = len(batches) + 1
    mid = n // 2
    by_order = {(k if k < mid else k + 1): b for k, b in enumerate(batches)}
    s = e.decode_session()
    s.begin(flt[0], flt[1], sorted=1, bytes_hint=sum(len(b["data"]) for b in batches), flags=PD_DECODE_COMPACT, n_batches=n, **cfg)
    got = {}
    for k in range(0, n, 2):
        pair = [o for o in (k + 1, k) if o < n]
        for o in pair:
            s.acquire(len(by_order[o]["data"]) if o in by_order else 0)
        for o in pair:
            if o in by_order:
                got[o] = s.submit(as_batch(by_order[o], o))
            else:
                st, res = s.submit(empty_batch(o))
                assert st.size == 0 and res["n_reads"] == 0 and res["n_first"] == 0
    s.end()
    return [got[o] for o in sorted(got)]


def run_mode(e, mode, batches, flt, **cfg):
    if mode == "compact":
        return run_compact(e, batches, flt, **cfg)
    return run_plain(e, batches, flt, queued=(mode == "queued"), **cfg)


def check_results(f, results, n_records=None, sorted_file=True):
    assert all(not st.any() for st, _ in results), [list(st) for st, _ in results]
    assert sum(r["n_reads"] for _, r in results) == (len(f["offs"]) if n_records is None else n_records)
    prev = None
    for _, r in results:
        if not r["n_first"]:
            continue
        assert r["first_key"] <= r["last_key"]
        if sorted_file:
            assert r["unsorted"] == 0
            assert prev is None or prev <= r["first_key"], (prev, r["first_key"])
        prev = r["last_key"]


def check_depth(e, lens, dep):
    e.scan(0)
    for t, ln in enumerate(lens):
        got = e.read_depth(t, 0, ln)
        want = np.zeros(ln, dtype=np.uint32) if dep[t] is None else dep[t]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (t, bad[:8], got[bad[:8]], want[bad[:8]])


def check_windows(e, f, flt, compact_direct):
    """the four window tables of a deferred sample; compact_direct: they came from the compact direct kernel (one "direct_tiles" launch
    per call, no run index built and nothing expanded to 12-byte runs)"""
    for w, m in WINDOWS:
        _, cover, tot = e.scan_reduce_windows(w, m, 0)
        cov_ref, tot_ref = f["windows"][(flt, w, m)]
        assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref), (w, m)
    if compact_direct:
        assert counter(e, "direct_tiles") == len(WINDOWS) and counter(e, "scatter_index") == 0 and counter(e, "expand_runs") == 0
        assert counter(e, "compact_finish") >= 1


# ---------------------------------------------------------------------------------------------------------------------
# (a) the session as a function (batching, mode, arrival) -> depth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,cut", CUTS, ids=["%s_batches_%s" % c for c in CUTS])
def test_session_gives_the_per_base_depth(corpus, name, cut, mode, flt):
    f = corpus[name]
    batches = f["cuts"][cut]
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, batches, flt)
        check_results(f, results)
        if mode == "compact":
            # pd_decode_end's compact branch: places from c8_counted, launch_c8_marks_to_index, runs_finish
            assert counter(e, "decode_end_compact") == 1 and counter(e, "decode_end_c8_fallback") == 0 and counter(e, "decode_end_scatter") == 0
        else:
            assert counter(e, "decode_end_scatter") == 1 and counter(e, "decode_end_unsorted") == 0 and counter(e, "decode_end_compact") == 0
        assert counter(e, "decode_chain_device") + counter(e, "decode_chain_host") == len(batches)
        check_depth(e, f["lens"], f["depth"][flt])
    with pda.Engine(f["lens"]) as e:
        e.keep_deferred(True)
        e.profile(True)
        check_results(f, run_mode(e, mode, batches, flt))
        check_windows(e, f, flt, compact_direct=(mode == "compact"))


TRANSPORTS = [("decode_h2d_fifo", 0), ("decode_h2d_lanes", 2), ("decode_h2d_kernel", 1), ("decode_h2d_kernel", 2), ("decode_h2d_kernel", 3),
              ("decode_sync_event", 0)]


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("param,value", TRANSPORTS, ids=["%s_%d" % t for t in TRANSPORTS])
def test_transport_variants_give_the_per_base_depth(corpus, param, value, mode):
    """the ways a batch's bytes reach the device and a collect waits for it that are off by default (dec_queue's upload, dec_collect's
    wait): the batches' own streams instead of the copy FIFO, two copy lanes, the three copy-kernel forms, the stream wait"""
    f = corpus["packed"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        e.set_param(param, value)
        check_results(f, run_mode(e, mode, batches, flt))
        assert counter(e, "decode_end_compact" if mode == "compact" else "decode_end_scatter") == 1
        assert counter(e, "decode_chain_device") + counter(e, "decode_chain_host") == len(batches)
        check_depth(e, f["lens"], f["depth"][flt])


# ---------------------------------------------------------------------------------------------------------------------
# (b) growth of the compact sample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cut,min_grow", [("packed", "16", 1), ("few", "3", 1)], ids=["packed_16", "few_3"])
def test_compact_sample_grows_and_moves(corpus, name, cut, min_grow):
    """"decode_c8_reserve" = 1024: the first estimate is 1024 first runs and 256 later runs and growth has no slack, so c8_counted's
    c8_reserve moves the placed runs (and oth(), whose offset depends on both capacities) while later batches are still arriving"""
    f = corpus[name]
    flt = B.FILTERS[0]
    with pda.Engine(f["lens"]) as e:
        e.set_param("decode_c8_reserve", 1024)
        check_results(f, run_compact(e, f["cuts"][cut], flt))
        assert counter(e, "decode_c8_grow") >= min_grow and counter(e, "decode_end_compact") == 1
        check_depth(e, f["lens"], f["depth"][flt])
    with pda.Engine(f["lens"]) as e:
        e.set_param("decode_c8_reserve", 1024)
        e.keep_deferred(True)
        e.profile(True)
        check_results(f, run_compact(e, f["cuts"][cut], flt))
        assert counter(e, "decode_c8_grow") >= min_grow
        check_windows(e, f, flt, compact_direct=True)                     # the tables of (a): both equal the reference's
    with pda.Engine(f["lens"]) as e:                                       # off by default: no small file grows the sample
        check_results(f, run_compact(e, f["cuts"][cut], flt))
        assert counter(e, "decode_c8_grow") == 0


# ---------------------------------------------------------------------------------------------------------------------
# (c) filters inside the session
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "compact"])
def test_contig_switched_off(corpus, mode):
    f = corpus["packed"]
    flt = B.FILTERS[0]
    on = [1, 0, 0, 1]                                                      # "small" (which has reads) and the one-base contig off
    dep = B.reference_depth(f["lens"], [r for r in f["recs"] if r["tid"] < 0 or on[r["tid"]]], *flt)[0]
    assert f["depth"][flt][1].any() and not dep[1].any()
    with pda.Engine(f["lens"]) as e:
        check_results(f, run_mode(e, mode, f["cuts"]["3"], flt, contig_on=on))
        check_depth(e, f["lens"], dep)


def endpos(r):
    """oracle/pd_oracle.c:121 pdo_endpos (htslib's bam_endpos): pos + reference length; an unmapped read or one without a CIGAR
    counts as one base, and so does a reference length of zero"""
    rlen = 0
    if not r["flag"] & 4 and r["cigar"].size:
        c = B.real_cigar(r)
        rlen = int((c >> 4)[np.isin(c & 0xf, (0, 2, 3, 7, 8))].sum(dtype=np.int64))
    else:
        rlen = 1
    return r["pos"] + (rlen if rlen else 1)


def region_hit(r, spans):
    """the read selection the -b comparisons rest on (oracle/pd_oracle.py:384 _select_indexed over oracle/pd_oracle.c:121
    pdo_endpos, htslib's multi-region fetch): pos < span end and endpos > span begin0 for some span of the read's contig"""
    return any(r["pos"] < e and endpos(r) > b for b, e in spans.get(r["tid"], ()))


def crafted_spans(f):
    at = lambda case: next(r for r in f["recs"] if r["off"] == f["cases"][case])
    big = [(100, 130), (350060, 350100), (350200, 350260)]                 # (350060, 350100): only the later run of gap_200k
    for case in ("no_cigar_placed", "unmapped_placed_q30", "no_reference_bases_100"):      # placed reads without reference bases: one base
        big.append((at(case)["pos"], at(case)["pos"] + 1))
    r = at("ops4096")                                                      # touched at its last base only / missed by one base
    big.append((endpos(r) - 1, endpos(r) + 3))
    r2 = at("eq_x")
    big.append((endpos(r2), endpos(r2) + 3))
    r3 = at("ops65535")
    b, e = B.runs_of(r3)
    big.append((int(b[b.size // 2]), int(b[b.size // 2]) + 1))             # one base of a later run
    spans = {0: sorted(big), 1: [], 3: [(69900, 70000)]}
    for v in spans.values():
        assert all(v[k][1] <= v[k + 1][0] for k in range(len(v) - 1)), v   # sorted and disjoint
    return spans, (r, r2)


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact_flag"])
@pytest.mark.parametrize("name", ["alone", "packed"])
def test_spans(corpus, name, compact):
    """a session with spans keeps 12-byte runs whatever the flags (pd_decode_begin's `!cfg->spans`): with PD_DECODE_COMPACT and
    n_batches it ends through the general branch (runs_make or the scatter), never through the compact one"""
    f = corpus[name]
    flt = B.FILTERS[0]
    spans, (last_base, missed) = crafted_spans(f)
    off = np.zeros(len(f["lens"]) + 1, dtype=np.uint32)
    flat = []
    for t in range(len(f["lens"])):
        flat += spans.get(t, [])
        off[t + 1] = len(flat)
    sel = [r for r in f["recs"] if r["tid"] >= 0 and region_hit(r, spans)]
    assert last_base in sel and missed not in sel
    names = {c for c, o in f["cases"].items() if any(r["off"] == o for r in sel)}
    assert {"gap_200k", "no_cigar_placed", "unmapped_placed_q30", "no_reference_bases_100", "ops65535"} <= names
    dep = B.reference_depth(f["lens"], sel, *flt)[0]
    assert not dep[1].any() and f["depth"][flt][1].any() and dep[0].any() and dep[3].any()
    kw = dict(contig_on=[1, 1, 0, 1], span_off=off, spans=flat)
    with pda.Engine(f["lens"]) as e:
        if compact:
            results = run_compact(e, f["cuts"]["3"], flt, **kw)
            assert counter(e, "decode_end_compact") == 0 and counter(e, "decode_end_runs_make") + counter(e, "decode_end_scatter") == 1
        else:
            results = run_plain(e, f["cuts"]["3"], flt, **kw)
        check_results(f, results)
        check_depth(e, f["lens"], dep)


# ---------------------------------------------------------------------------------------------------------------------
# (d) guessed starts
# ---------------------------------------------------------------------------------------------------------------------
def true_boundary(f, at):
    """the first record start at or after file offset `at` (None: there is none)"""
    k = int(np.searchsorted(np.asarray(f["offs"]), at, side="left"))
    return f["offs"][k] if k < len(f["offs"]) else None


@pytest.mark.parametrize("name", ["alone", "packed", "layout"])
def test_guessed_starts_at_member_starts(corpus, name):
    f = corpus[name]
    flt = B.FILTERS[0]
    total = len(f["inf"])
    batches = f["cuts"]["guess"]
    assert len(batches) >= 3 and all(b["units"][0][5] == (PD_UNIT_GUESS if k else 0) for k, b in enumerate(batches))
    assert any(b["units_file"][0][0] not in f["offs"] for b in batches[1:])            # a member start inside a record
    with pda.Engine(f["lens"]) as e:
        results = run_plain(e, batches, flt)
        check_results(f, results)
        # dec_queue's `guess`: such batches leave the chain to the host (dec_collect's loop over dec_finish)
        assert counter(e, "decode_guess_units") == len(batches) - 1 and counter(e, "decode_chain_host") >= len(batches) - 1
        for k, (b, (_, r)) in enumerate(zip(batches, results)):
            start, stop = b["units_file"][0][:2]
            assert r["first_start"] + b["base"] == true_boundary(f, start), k
            nxt = true_boundary(f, stop)
            if nxt is not None:
                assert r["next_start"] + b["base"] == nxt, k
                assert r["next_start"] + b["base"] == results[k + 1][1]["first_start"] + batches[k + 1]["base"]
            else:
                assert r["next_start"] + b["base"] == total, k            # (the end of the last record: where a next one would begin)
        check_depth(e, f["lens"], f["depth"][flt])


def test_guessed_starts_around_record_starts_and_in_decoys(corpus):
    """units that begin 1 .. 37 bytes before and behind a record start find the true boundary; a unit that begins inside one of the two
    records that carry a decoy header in a Z tag may be handed back — as unfollowable (3), or as 1: the decoy's block size says 117 MB,
    which is the header's "a record runs past the unit's bytes", and for a guessed start nothing tells the two apart; the executable
    declines the device pass on either — but is never counted (0) from a wrong boundary"""
    f = corpus["layout"]
    flt = B.FILTERS[0]
    offs = f["offs"]
    s = B.decoy_tag()
    tag_at = [m.start() for m in re.finditer(re.escape(s), f["inf"])]
    decoy_rec = [max(k for k in range(len(offs)) if offs[k] < a) for a in tag_at]
    by_size = {r["size"]: k for k, r in enumerate(f["recs"])}
    targets = [40, by_size[5000] + 1, by_size[4 + 32 + 255 + 4 + 75], len(offs) // 2]
    assert not set(targets) & set(decoy_rec) and not set(t - 1 for t in targets) & set(decoy_rec)
    units = []                                                             # (start, index of the record the stop is, inside a decoy record)
    for k in targets:
        for d in range(1, 38):
            units += [(offs[k] - d, k + 12, False), (offs[k] + d, k + 12, False)]
    for a, k in zip(tag_at, decoy_rec):
        for st in sorted(set([offs[k] + 1, offs[k] + 36, a - 37, a - 4, a - 1, a, a + 1, a + 4, a + 35, a + 36, a + 37, a + len(s)])):
            assert offs[k] < st < offs[k + 1]
            units.append((st, k + 12, True))
    counted = []
    with pda.Engine(f["lens"]) as e:
        ses = e.decode_session()
        ses.begin(flt[0], flt[1], sorted=0)
        for j, (start, kstop, in_decoy) in enumerate(units):
            b = B.batch_of_units(f, [B.unit_at(f, start, offs[kstop], PD_UNIT_GUESS)], j)
            ses.acquire(len(b["data"]))
            st, r = ses.submit(as_batch(b))
            want = true_boundary(f, start)
            if in_decoy and start <= tag_at[decoy_rec.index(int(np.searchsorted(offs, start, side="right")) - 1)]:
                assert st[0] in (0, 1, 3), (start, st[0])                  # the decoy header lies ahead of the start
            else:
                assert st[0] == 0, (start, st[0])                          # (behind the decoy header: nothing to mistake)
            if st[0] == 0:
                assert r["first_start"] + b["base"] == want, (start, in_decoy)
                assert r["next_start"] + b["base"] == offs[kstop], (start, in_decoy)
                first = offs.index(want)
                assert r["n_reads"] == kstop - first
                counted += f["recs"][first:kstop]
        ses.end()
        assert counter(e, "decode_guess_units") == len(units)
        check_depth(e, f["lens"], B.reference_depth(f["lens"], counted, *flt)[0])


def test_guessed_start_with_a_decoy_behind_an_empty_first_segment(corpus):
    """A unit that begins inside a record of more than two segments: its first segment holds no record start, the second one's own
    guess stands (pdb2::check_chain), and there a Z tag passes for a record header.  The unit may be left to the host but is never
    counted from the decoy; units that begin behind the decoy find the true boundary."""
    f, rec, decoy = corpus["long_decoy"]
    flt = B.FILTERS[0]
    _, seg, _ = B.walk_geometry()
    offs = f["offs"]
    true, kstop = offs[21], 60
    before = [rec + d for d in (1, 4096, seg // 2 - 1)]
    behind = [decoy + 1, decoy + 37, decoy + seg // 2]
    assert all(decoy - s > seg for s in before) and all(s < true for s in behind)
    counted = []
    with pda.Engine(f["lens"]) as e:
        ses = e.decode_session()
        ses.begin(flt[0], flt[1], sorted=0)
        for j, start in enumerate(before + behind):
            b = B.batch_of_units(f, [B.unit_at(f, start, offs[kstop], PD_UNIT_GUESS)], j)
            ses.acquire(len(b["data"]))
            st, r = ses.submit(as_batch(b))
            assert st[0] in ((0, 1, 3) if start in before else (0,)), (start, st[0])
            if st[0] == 0:
                assert r["first_start"] + b["base"] == true and r["next_start"] + b["base"] == offs[kstop] and r["n_reads"] == kstop - 21
                counted += f["recs"][21:kstop]
        ses.end()
        check_depth(e, f["lens"], B.reference_depth(f["lens"], counted, *flt)[0])


# ---------------------------------------------------------------------------------------------------------------------
# (e) order violations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("where", ["same_batch", "cut_between"])
def test_order_violation(corpus, where, mode):
    f = corpus["unsorted"]
    flt = B.FILTERS[0]
    recs, offs = f["recs"], f["offs"]
    k = next(k for k in range(len(recs) - 1) if recs[k]["tid"] == recs[k + 1]["tid"] and recs[k]["pos"] > recs[k + 1]["pos"])
    assert all(B.kept(recs[j], len(f["lens"]), *flt) and B.runs_of(recs[j])[0][0] == recs[j]["pos"] for j in (k, k + 1))
    stops = [offs[k // 2], offs[k + 1] if where == "cut_between" else offs[k + 2], offs[(k + len(offs)) // 2]]
    batches = B.cut_batches(f, stops, 1)
    assert len(batches) == 4
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, batches, flt)
        check_results(f, results, sorted_file=False)
        flags = [r["unsorted"] for _, r in results]
        if where == "same_batch":
            assert flags == [0, 1, 0, 0]
            assert all(results[j][1]["last_key"] <= results[j + 1][1]["first_key"] for j in range(3))
        else:
            assert flags == [0, 0, 0, 0]
            assert results[2][1]["first_key"] < results[1][1]["last_key"]
            assert results[0][1]["last_key"] <= results[1][1]["first_key"] and results[2][1]["last_key"] <= results[3][1]["first_key"]
        assert counter(e, "decode_end_unsorted") == 1
        if mode == "compact":
            assert counter(e, "decode_end_c8_fallback") == 1 and counter(e, "decode_end_compact") == 0      # back to 12-byte runs
        else:
            assert counter(e, "decode_end_scatter") == 1                                                    # pushed as PD_PUSH_DEFAULT
        check_depth(e, f["lens"], f["depth"][flt])


# ---------------------------------------------------------------------------------------------------------------------
# (f) lifecycle
# ---------------------------------------------------------------------------------------------------------------------
def test_abort_with_batches_queued_then_a_good_session(corpus):
    f = corpus["packed"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        for compact in (False, True):
            s = e.decode_session()
            s.begin(flt[0], flt[1], flags=PD_DECODE_COMPACT if compact else 0, n_batches=3 if compact else 0)
            for b in batches[:2]:
                s.acquire(len(b["data"]))
            for b in batches[:2]:
                s.queue(as_batch(b))
            s.abort()
            check_depth(e, f["lens"], [None] * len(f["lens"]))            # nothing was counted
            e.reset()
            check_results(f, run_mode(e, "compact" if compact else "plain", batches, flt))
            check_depth(e, f["lens"], f["depth"][flt])
            e.reset()


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
def test_end_counts_the_batches_still_queued(corpus, compact):
    f = corpus["packed"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        s.begin(flt[0], flt[1], flags=PD_DECODE_COMPACT if compact else 0, n_batches=3 if compact else 0)
        s.acquire(len(batches[0]["data"]))
        st, r = s.submit(as_batch(batches[0]))
        assert not st.any()
        for b in batches[1:]:
            s.acquire(len(b["data"]))
        for b in batches[1:]:
            s.queue(as_batch(b))
        s.end()                                                            # dec_drain(finish): the two are collected and counted
        assert counter(e, "decode_chain_device") + counter(e, "decode_chain_host") == 3
        assert counter(e, "decode_end_compact") == (1 if compact else 0)
        check_depth(e, f["lens"], f["depth"][flt])


@pytest.mark.parametrize("mode", ["plain", "compact"])
def test_two_sessions_without_a_reset(corpus, mode):
    """the second pd_decode_end finds the first sample still deferred on the context's arrays (flush_pending at its head); a second
    compact session cannot be one (pd_decode_begin's `c->pend.empty()`) and goes on with 12-byte runs"""
    few, alone = corpus["few"], corpus["alone"]
    flt = B.FILTERS[0]
    assert few["lens"] == alone["lens"]
    with pda.Engine(few["lens"]) as e:
        check_results(few, run_mode(e, mode, few["cuts"]["3"], flt))
        if mode == "compact":
            assert counter(e, "decode_end_compact") == 1
        check_results(alone, run_mode(e, mode, alone["cuts"]["3"], flt))
        if mode == "compact":
            assert counter(e, "decode_end_compact") == 0 and counter(e, "decode_end_runs_make") + counter(e, "decode_end_scatter") == 1
        check_depth(e, few["lens"], add_depth(few["depth"][flt], alone["depth"][flt]))
    with pda.Engine(few["lens"]) as e:                                     # the same file twice
        for _ in range(2):
            check_results(alone, run_mode(e, mode, alone["cuts"]["3"], flt))
        check_depth(e, few["lens"], add_depth(alone["depth"][flt], alone["depth"][flt]))


def test_compact_session_with_host_intervals_before_end(corpus):
    """runs pushed by the host between the last collect and pd_decode_end (units it decoded itself): pd_decode_end's non-empty `pend`
    branch scatters them and pushes the compact sample behind them"""
    f = corpus["packed"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    iv = np.array([[0, 10, 500], [0, 8190, 8200], [0, 399990, 400000], [1, 0, 5000], [3, 100, 101]], dtype=np.int32)
    dep = [None if x is None else x.copy() for x in f["depth"][flt]]
    for t, b, en in iv.tolist():
        dep[t][b:en] += 1
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        s.begin(flt[0], flt[1], flags=PD_DECODE_COMPACT, n_batches=3, bytes_hint=len(f["data"]))
        results = []
        for k, b in enumerate(batches):
            s.acquire(len(b["data"]))
            results.append(s.submit(as_batch(b)))
        e.push_intervals(iv, pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
        s.end()
        check_results(f, results)
        assert counter(e, "decode_end_pending") == 1 and counter(e, "decode_end_compact") == 1
        check_depth(e, f["lens"], dep)


def test_errors_leave_the_context_usable(corpus):
    f = corpus["few"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]

    def good(e):
        for mode in ("plain", "compact"):
            check_results(f, run_mode(e, mode, batches, flt))
            check_depth(e, f["lens"], f["depth"][flt])
            e.reset()

    def fails(code, text, call, *a):
        with pytest.raises(pda.PdError) as x:
            call(*a)
        assert x.value.code == code and text in str(x.value), str(x.value)

    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        fails(PD_ESTATE, "call pd_decode_begin first", s.acquire, 1000)
        good(e)
        # a buffer that was not acquired
        s.begin(flt[0], flt[1])
        mine = ctypes.create_string_buffer(len(batches[0]["data"]) + 4096)
        fails(PD_EINVAL, "was not handed out by pd_decode_acquire", s.submit, as_batch(batches[0]), ctypes.addressof(mine))
        fails(PD_EINVAL, "was not handed out by pd_decode_acquire", s.queue, as_batch(batches[0]), ctypes.addressof(mine))
        s.abort()
        good(e)
        # a ticket collected twice
        s.begin(flt[0], flt[1])
        s.acquire(len(batches[0]["data"]))
        t = s.queue(as_batch(batches[0]))
        st, r = s.collect(t, len(batches[0]["units"]))
        assert not st.any() and r["n_reads"] > 0
        fails(PD_EINVAL, "not the ticket of a queued batch", s.collect, t, len(batches[0]["units"]))
        s.abort()
        good(e)
        # a compact session ended with one order missing
        s.begin(flt[0], flt[1], flags=PD_DECODE_COMPACT, n_batches=3)
        for b in batches[:2]:
            s.acquire(len(b["data"]))
            s.submit(as_batch(b))
        fails(PD_ESTATE, "not every batch of the compact session was submitted", s.end)
        good(e)
        # ... and with one order submitted twice
        s.begin(flt[0], flt[1], flags=PD_DECODE_COMPACT, n_batches=3)
        for b in (batches[0], batches[1], batches[1], batches[2]):
            s.acquire(len(b["data"]))
            s.submit(as_batch(b))
        fails(PD_ESTATE, "a batch number was submitted twice", s.end)
        good(e)
