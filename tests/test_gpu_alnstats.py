"""The CIGAR statistics of a decode session on the MI355X (PD_DECODE_ALN_STATS: k_aln_stats behind every batch's emission,
pd_decode_aln_stats after pd_decode_end), on bam_craft's crafted files, on `aln_edges` of tests/alnstats_model.py and on the records corpus
of tests/recstats_model.py, against the model of tests/alnstats_model.py.  Every comparison is exact: the sums, and sums[records] against
the sum of the results' n_reads."""
import numpy as np
import pytest

import alnstats_model as AM
import bam_craft as B
import del_model as DM
import frag_model as FM
import pandepth_amd as pda
import recstats_model as RM
from test_gpu_decode_session import as_batch, check_depth, counter, run_mode, run_plain

pytestmark = pytest.mark.gpu
CRAFT = ["alone", "packed", "layout", "few"]
MODES = ["plain", "queued", "compact"]
W = 100


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the files, their cuts and every model, computed once, shared, never changed"""
    d = tmp_path_factory.mktemp("alnstats_gpu")
    files = {"records": dict(RM.corpus(d), names=RM.NAMES)}
    files["records"]["cuts"] = RM.session_cuts(files["records"])
    files["aln_edges"] = AM.edges_file(d)
    files["aln_edges"]["cuts"] = AM.session_cuts(files["aln_edges"])
    crafted = B.build_corpus(d)
    for n in CRAFT:
        files[n] = dict(crafted[n], cuts=B.session_cuts(crafted[n], n))
    for f in files.values():
        f["want"] = {}
        for flt in B.FILTERS:
            for w in AM.WIDTHS:
                s = AM.Model(len(f["lens"]), flt[0], flt[1], w).add_parsed(f["recs"]).array()
                s.setflags(write=False)
                f["want"][(flt, w)] = s
    return files


def check_stats(e, f, flt, w, results):
    sums = e.decode_session().aln_stats()
    want = f["want"][(flt, w)]
    assert all(not st.any() for st, _ in results), [list(st) for st, _ in results]
    assert int(sums[AM.RECORDS]) == sum(r["n_reads"] for _, r in results) == len(f["offs"])
    assert np.array_equal(sums, want), [(int(k), int(sums[k]), int(want[k])) for k in np.flatnonzero(sums != want)[:20]]
    assert sums[AM.INS:AM.INS + AM.INDEL_BINS + 1].sum() == sums[AM.OPS + 2] and sums[AM.DEL:AM.DEL + AM.INDEL_BINS + 1].sum() == sums[AM.OPS + 4]


CUTS = [("aln_edges", c) for c in ("1", "3", "16", "crafted")] + [(n, "3") for n in CRAFT] + [("layout", "crafted"), ("records", "1"), ("records", "crafted")]


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,cut", CUTS, ids=["%s_batches_%s" % c for c in CUTS])
def test_session_statistics_equal_the_model(corpus, name, cut, mode, flt):
    f = corpus[name]
    batches = f["cuts"][cut]
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, batches, flt, aln_stats=W)
        check_stats(e, f, flt, W, results)
        assert counter(e, "decode_aln_stats") == len(batches)             # one launch that counted, per batch — whoever confirmed its chain


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("name", ["aln_edges", "alone"])
def test_bins_of_one_base(corpus, name, mode):
    f = corpus[name]
    for flt in B.FILTERS:
        with pda.Engine(f["lens"]) as e:
            check_stats(e, f, flt, 1, run_mode(e, mode, f["cuts"]["3"], flt, aln_stats=1))


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("param", ["decode_spoil", "decode_fast"])
@pytest.mark.parametrize("name", ["records", "alone", "aln_edges"])
def test_repaired_chains_and_the_hosts_chain_check(corpus, name, param, mode):
    """"decode_spoil" = 1: every segment behind a unit's first walks again on the device; "decode_fast" = 0: the host confirms the chain
    and the pass follows the host's emission"""
    f = corpus[name]
    flt = B.FILTERS[0]
    for cut in ("1", "3"):
        with pda.Engine(f["lens"]) as e:
            e.set_param(param, 1 if param == "decode_spoil" else 0)
            results = run_mode(e, mode, f["cuts"][cut], flt, aln_stats=W)
            check_stats(e, f, flt, W, results)
            if param == "decode_fast":
                assert counter(e, "decode_chain_host") == len(f["cuts"][cut]) and counter(e, "decode_chain_device") == 0
            elif name == "records" and cut == "1":                                  # (two units of several segments each; a unit of cut "3" is one segment)
                assert counter(e, "decode_segments_redone") > 0


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("kw", [dict(fragments=True), dict(count_deletions=True), dict(fragments=True, count_deletions=True, frag_max=FM.FRAGMAX_CASE)],
                         ids=["fragments", "deletions", "both_with_a_bound"])
def test_the_depth_rules_do_not_change_the_statistics(corpus, kw, mode):
    f = corpus["records"]
    flt = B.FILTERS[1]
    dep = FM.model(f["lens"], f["model_recs"], *flt, count_del=bool(kw.get("count_deletions")), frag_max=kw.get("frag_max", FM.NO_BOUND))[0] if kw.get("fragments") \
        else DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=True)[0]
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, f["cuts"]["3"], flt, aln_stats=W, **kw)
        check_stats(e, f, flt, W, results)
        check_depth(e, f["lens"], dep)


@pytest.mark.parametrize("mode", ["plain", "compact"])
def test_with_the_other_record_passes_in_one_session(corpus, mode):
    """record_stats, row_counts and aln_stats together: three kernels behind every batch, each with its own numbers"""
    f = corpus["records"]
    flt = B.FILTERS[0]
    want_s, want_p = RM.Model(f["names"], f["lens"], flt[0], flt[1], 1000).add_all(f["model_recs"]).arrays()
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        results = run_mode(e, mode, f["cuts"]["3"], flt, aln_stats=W, record_stats=1000, row_counts=("w", 1000))
        check_stats(e, f, flt, W, results)
        s.n_isize = 1000
        sums, per = s.record_stats()
        assert np.array_equal(sums, want_s) and np.array_equal(per, want_p)
        s.n_row_bins = int(e.window_layout(1000)[-1])
        rows = s.row_counts()
        assert int(rows[:, 0].sum()) == int(want_s[RM.RECORDS] - want_s[RM.UNPLACED]) and int(rows[:, 3].sum()) == int(want_s[RM.KEPT])
        assert counter(e, "decode_aln_stats") == counter(e, "decode_record_stats") == counter(e, "decode_row_counts") == len(f["cuts"]["3"])


@pytest.mark.parametrize("fast", [1, 0], ids=["device_chain", "host_chain"])
def test_a_unit_handed_back_is_not_counted(corpus, fast):
    """unit 0 of the batch ends its bytes inside its last record: an ordinary status 1, the host decodes the unit — and counts it.  The
    device's numbers are the model's over the records of unit 1 alone."""
    f = corpus["records"]
    flt = B.FILTERS[0]
    b = dict(f["cuts"]["1"][0])
    assert len(b["units"]) == 2
    offs = np.asarray(f["offs"], dtype=np.int64)
    u0, u1 = b["units_file"]
    last0 = int(offs[(offs >= u0[0]) & (offs < u0[1])][-1])
    units = [tuple(b["units"][0][:2]) + (last0 - b["base"] + 40,) + tuple(b["units"][0][3:]), b["units"][1]]
    b["units"] = units
    mine = [r for r in f["recs"] if u1[0] <= r["off"] < u1[1]]
    assert 0 < len(mine) < len(f["offs"])
    want = AM.Model(len(f["lens"]), flt[0], flt[1], W).add_parsed(mine).array()
    with pda.Engine(f["lens"]) as e:
        e.set_param("decode_fast", fast)
        s = e.decode_session()
        s.begin(flt[0], flt[1], sorted=1, bytes_hint=len(b["data"]), aln_stats=W)
        s.acquire(len(b["data"]))
        st, res = s.submit(as_batch(b))
        s.end()
        assert list(st) == [1, 0] and res["n_reads"] == len(mine)
        assert counter(e, "decode_aln_stats") == 1                        # (device_chain: the launch the chain kernel's verdict stopped is not counted)
        assert np.array_equal(s.aln_stats(), want) and want[AM.ALIGNED] > 0


def test_an_abort_leaves_nothing(corpus):
    f = corpus["aln_edges"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        s.begin(flt[0], flt[1], sorted=1, aln_stats=W)
        s.acquire(len(batches[0]["data"]))
        st, _ = s.submit(as_batch(batches[0]))
        assert not st.any()
        s.abort()
        with pytest.raises(pda.PdError):
            s.aln_stats()
        check_stats(e, f, flt, W, run_plain(e, batches, flt, aln_stats=W))                 # only the second session's numbers (no reset in between)
        e.reset()
        check_stats(e, f, flt, 1, run_plain(e, batches, flt, aln_stats=1))                 # another width
        U64P = pda.capi.ctypes.POINTER(pda.capi.ctypes.c_uint64)
        short = np.zeros(AM.WORDS - 1, dtype=np.uint64)
        assert e.L.pd_decode_aln_stats(e.h, short.ctypes.data_as(U64P), short.size) != 0   # (a wrong n_sums)
        assert not short.any()


@pytest.mark.parametrize("mode", ["plain", "compact"])
def test_two_sessions_without_a_reset_do_not_add_up(corpus, mode):
    """what a context does with the inputs of a list: one session each into the same arrays, the numbers fetched after every end.  The
    second session's numbers are one session's (read_max included); the depth is the sum of both."""
    f = corpus["records"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    one = DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=False)[0]
    with pda.Engine(f["lens"]) as e:
        check_stats(e, f, flt, W, run_mode(e, mode, batches, flt, aln_stats=W))
        check_stats(e, f, flt, W, run_mode(e, mode, batches, flt, aln_stats=W))            # (no reset in between)
        assert counter(e, "decode_aln_stats") == len(batches)
        check_depth(e, f["lens"], [None if d is None else 2 * d for d in one])


def test_a_session_without_the_flag(corpus):
    f = corpus["records"]
    flt = B.FILTERS[0]
    dep = DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=False)[0]
    with pda.Engine(f["lens"]) as e:
        results = run_plain(e, f["cuts"]["3"], flt)
        assert sum(r["n_reads"] for _, r in results) == len(f["offs"])
        with pytest.raises(pda.PdError) as err:
            e.decode_session().aln_stats()
        assert "PD_DECODE_ALN_STATS" in str(err.value)
        assert e.profile_get("decode_aln_stats") == (0.0, 0)
        check_depth(e, f["lens"], dep)
    with pda.Engine(f["lens"]) as e:                                                       # the flag without its parameter: refused, and the context is as it was
        s = e.decode_session()
        with pytest.raises(pda.PdError) as err:
            s.begin(flt[0], flt[1], flags=pda.PD_DECODE_ALN_STATS)
        assert "decode_len_bin_width" in str(err.value)
        with pytest.raises(pda.PdError):
            e.set_param("decode_len_bin_width", 65537)
        check_stats(e, f, flt, W, run_plain(e, f["cuts"]["3"], flt, aln_stats=W))
    with pda.Engine(f["lens"]) as e:                                                       # a session with the flag, then one without: refused again
        check_stats(e, f, flt, W, run_plain(e, f["cuts"]["3"], flt, aln_stats=W))
        run_plain(e, f["cuts"]["3"], flt)                                                  # (no reset: the flag does not stick to the context)
        with pytest.raises(pda.PdError):
            e.decode_session().aln_stats()
        assert counter(e, "decode_aln_stats") == 0
        check_depth(e, f["lens"], [None if d is None else 2 * d for d in dep])             # (the depth of both sessions, as it would be without the flag)
