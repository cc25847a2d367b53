"""The records per bin of a decode session on the MI355X (PD_DECODE_ROW_COUNTS: k_row_counts behind every batch's emission,
pd_decode_row_bins before pd_decode_begin, pd_decode_row_counts after pd_decode_end), on the corpus of tests/rowreads_model.py, its
unsorted file and bam_craft's crafted files, against the model there.  Every comparison is exact: every word of every bin, and the bins'
records against the model's count of records that start somewhere."""
import ctypes

import numpy as np
import pytest

import bam_craft as B
import del_model as DM
import frag_model as FM
import pandepth_amd as pda
import recstats_model as RM
import rowreads_model as RR
from test_gpu_decode_session import as_batch, check_depth, counter, run_mode, run_plain

pytestmark = pytest.mark.gpu
CRAFT = ["alone", "packed", "layout", "few"]
MODES = ["plain", "queued", "compact"]
FORMS = ["w7", "w1000", "no_edges", "regions"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the files, their cuts and tables; every model is computed once (want), shared, never changed"""
    d = tmp_path_factory.mktemp("rowreads_gpu")
    files = {"corpus": RR.corpus(d), "unsorted": RR.unsorted(d)}
    files["corpus"]["cuts"] = RR.session_cuts(files["corpus"])
    crafted = B.build_corpus(d)
    for n in CRAFT:
        f = crafted[n]
        files[n] = dict(f, names=B.NAMES, model_recs=FM.records_of(f["inf"], f["recs"]), cuts=B.session_cuts(f, n))
    for f in files.values():
        f["tables"] = RR.bin_tables(f["names"], f["lens"])
        f["want"] = {}
    return files


def want(f, form, flt, recs=None):
    if recs is not None:
        _, rows, w = f["tables"][form]
        return RR.Model(f["lens"], rows, flt[0], flt[1], uniform_w=w).add_all(recs).counts
    if (form, flt) not in f["want"]:
        c = want(f, form, flt, f["model_recs"])
        c.setflags(write=False)
        f["want"][(form, flt)] = c
    return f["want"][(form, flt)]


def table(f, form):
    return RR.session_table(f["tables"][form][0])


def counts_of(e, f, form):
    s = e.decode_session()
    s.n_row_bins = len(f["tables"][form][1])
    return s.row_counts()


def check_counts(e, f, form, flt, results):
    got = counts_of(e, f, form)
    exp = want(f, form, flt)
    assert all(not st.any() for st, _ in results), [list(st) for st, _ in results]
    assert sum(r["n_reads"] for _, r in results) == len(f["offs"])
    assert got.shape == exp.shape and np.array_equal(got, exp), np.argwhere(got != exp)[:20]
    assert int(got[:, RR.RECORDS].sum()) == RR.started(f["lens"], f["model_recs"])


CUTS = [("corpus", c) for c in ("1", "3", "16", "crafted")] + [(n, "3") for n in CRAFT] + [("layout", "crafted")]
SESSIONS = [(n, c, m, FORMS[(i + j) % len(FORMS)], B.FILTERS[(i + j) % 2]) for i, (n, c) in enumerate(CUTS) for j, m in enumerate(MODES)]


@pytest.mark.parametrize("name,cut,mode,form,flt", SESSIONS, ids=["%s_batches_%s_%s_%s_x%d" % (s[0], s[1], s[2], s[3], s[4][0]) for s in SESSIONS])
def test_session_counts_equal_the_model(corpus, name, cut, mode, form, flt):
    f = corpus[name]
    batches = f["cuts"][cut]
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, batches, flt, row_counts=table(f, form))
        check_counts(e, f, form, flt, results)
        assert counter(e, "decode_row_counts") == len(batches)            # one launch that counted, per batch — whoever confirmed its chain


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("form", ["w1", "w7", "w1000", "w150000", "no_edges", "regions", "every_cell"])
def test_every_form_on_the_corpus(corpus, form, flt):
    f = corpus["corpus"]
    with pda.Engine(f["lens"]) as e:
        check_counts(e, f, form, flt, run_mode(e, "plain", f["cuts"]["3"], flt, row_counts=table(f, form)))


@pytest.mark.parametrize("form", ["w7", "w1000", "regions", "every_cell"])
@pytest.mark.parametrize("cut", ["1", "3"])
def test_the_unsorted_file(corpus, cut, form):
    f = corpus["unsorted"]
    flt = B.FILTERS[1]
    with pda.Engine(f["lens"]) as e:
        results = run_plain(e, f["cuts"][cut], flt, sorted=0, row_counts=table(f, form))
        check_counts(e, f, form, flt, results)


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("param", ["decode_spoil", "decode_fast"])
@pytest.mark.parametrize("name", ["corpus", "alone"])
def test_repaired_chains_and_the_hosts_chain_check(corpus, name, param, mode):
    """"decode_spoil" = 1: every segment behind a unit's first walks again on the device; "decode_fast" = 0: the host confirms the chain
    and the pass follows the host's emission"""
    f = corpus[name]
    flt = B.FILTERS[0]
    for cut, form in (("1", "regions"), ("3", "w1000")):
        with pda.Engine(f["lens"]) as e:
            e.set_param(param, 1 if param == "decode_spoil" else 0)
            results = run_mode(e, mode, f["cuts"][cut], flt, row_counts=table(f, form))
            check_counts(e, f, form, flt, results)
            if param == "decode_fast":
                assert counter(e, "decode_chain_host") == len(f["cuts"][cut]) and counter(e, "decode_chain_device") == 0
            elif name == "corpus" and cut == "1":
                assert counter(e, "decode_segments_redone") > 0


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("form", ["w1000", "regions"])
def test_together_with_the_record_statistics(corpus, form, mode):
    """both flags: both kernels run, both results are right, and -readstats' numbers are those of a session without row_counts"""
    f = corpus["corpus"]
    flt = B.FILTERS[1]
    n = 1000
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        run_mode(e, mode, batches, flt, record_stats=n)
        s = e.decode_session(); s.n_isize = n
        alone = s.record_stats()
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, batches, flt, record_stats=n, row_counts=table(f, form))
        check_counts(e, f, form, flt, results)
        s = e.decode_session(); s.n_isize = n
        sums, per = s.record_stats()
        want_s, want_p = RM.Model(f["names"], f["lens"], flt[0], flt[1], n).add_all(f["model_recs"]).arrays()
        assert np.array_equal(sums, want_s) and np.array_equal(per, want_p)
        assert np.array_equal(sums, alone[0]) and np.array_equal(per, alone[1])
        assert counter(e, "decode_row_counts") == len(batches) == counter(e, "decode_record_stats")


@pytest.mark.parametrize("mode", ["plain", "compact"])
@pytest.mark.parametrize("kw", [dict(fragments=True), dict(count_deletions=True), dict(fragments=True, count_deletions=True, frag_max=FM.FRAGMAX_CASE)],
                         ids=["fragments", "deletions", "both_with_a_bound"])
def test_the_depth_rules_do_not_change_the_counts(corpus, kw, mode):
    f = corpus["corpus"]
    flt = B.FILTERS[1]
    dep = FM.model(f["lens"], f["model_recs"], *flt, count_del=bool(kw.get("count_deletions")), frag_max=kw.get("frag_max", FM.NO_BOUND))[0] if kw.get("fragments") \
        else DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=True)[0]
    with pda.Engine(f["lens"]) as e:
        results = run_mode(e, mode, f["cuts"]["3"], flt, row_counts=table(f, "regions"), **kw)
        check_counts(e, f, "regions", flt, results)
        check_depth(e, f["lens"], dep)                                    # (the depth is what it is without the flag: the model's)


@pytest.mark.parametrize("fast", [1, 0], ids=["device_chain", "host_chain"])
def test_a_unit_handed_back_is_not_counted(corpus, fast):
    """unit 0 of the batch ends its bytes inside its last record: an ordinary status 1, the host decodes the unit — and counts it.  The
    device's bins are the model's over the records of unit 1 alone."""
    f = corpus["corpus"]
    flt = B.FILTERS[0]
    b = dict(f["cuts"]["1"][0])
    assert len(b["units"]) == 2
    offs = np.asarray(f["offs"], dtype=np.int64)
    u0, u1 = b["units_file"]
    last0 = int(offs[(offs >= u0[0]) & (offs < u0[1])][-1])
    b["units"] = [tuple(b["units"][0][:2]) + (last0 - b["base"] + 40,) + tuple(b["units"][0][3:]), b["units"][1]]
    mine = [r for r, o in zip(f["model_recs"], f["offs"]) if u1[0] <= o < u1[1]]
    assert 0 < RR.started(f["lens"], mine) < RR.started(f["lens"], f["model_recs"])
    exp = want(f, "w1000", flt, mine)
    with pda.Engine(f["lens"]) as e:
        e.set_param("decode_fast", fast)
        s = e.decode_session()
        s.begin(flt[0], flt[1], sorted=1, bytes_hint=len(b["data"]), row_counts=table(f, "w1000"))
        s.acquire(len(b["data"]))
        st, res = s.submit(as_batch(b))
        s.end()
        assert list(st) == [1, 0] and res["n_reads"] == len(mine)
        assert counter(e, "decode_row_counts") == 1                       # (device_chain: the launch the chain kernel's verdict stopped is not counted)
        assert np.array_equal(s.row_counts(), exp)


def test_an_abort_leaves_nothing(corpus):
    f = corpus["corpus"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        s.begin(flt[0], flt[1], sorted=1, row_counts=table(f, "w1000"))
        s.acquire(len(batches[0]["data"]))
        st, _ = s.submit(as_batch(batches[0]))
        assert not st.any()
        s.abort()
        with pytest.raises(pda.PdError):
            s.row_counts()
        check_counts(e, f, "w1000", flt, run_plain(e, batches, flt, row_counts=table(f, "w1000")))      # only the second session's numbers (no reset in between)
        # an aborted session whose bins are looked at: begin zeroes, so a session of no batches over the same table reads zeros
        s = e.decode_session()
        s.begin(flt[0], flt[1], sorted=1, row_counts=table(f, "w1000"))
        s.acquire(len(batches[0]["data"]))
        s.submit(as_batch(batches[0]))
        s.abort()
        s.begin(flt[0], flt[1], sorted=1, row_counts=table(f, "w1000"))
        s.end()
        assert not s.row_counts().any()


@pytest.mark.parametrize("mode", ["plain", "compact"])
def test_two_sessions_with_different_tables(corpus, mode):
    """what a context does with the inputs of a list, and more: one session each into the same context, another table for the second,
    the numbers fetched after every end.  Each session's numbers are its own; the depth is the sum of both."""
    f = corpus["corpus"]
    flt = B.FILTERS[0]
    batches = f["cuts"]["3"]
    one = DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=False)[0]
    with pda.Engine(f["lens"]) as e:
        check_counts(e, f, "regions", flt, run_mode(e, mode, batches, flt, row_counts=table(f, "regions")))
        check_counts(e, f, "w7", flt, run_mode(e, mode, batches, flt, row_counts=table(f, "w7")))          # (no reset in between)
        with pytest.raises(pda.PdError):
            counts_of(e, f, "regions")                                                                    # (n_bins of the other session)
        assert counter(e, "decode_row_counts") == len(batches)
        check_depth(e, f["lens"], [None if d is None else 2 * d for d in one])


def test_a_session_without_the_flag(corpus):
    f = corpus["corpus"]
    flt = B.FILTERS[0]
    dep = DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=False)[0]
    with pda.Engine(f["lens"]) as e:
        results = run_plain(e, f["cuts"]["3"], flt)
        assert sum(r["n_reads"] for _, r in results) == len(f["offs"])
        with pytest.raises(pda.PdError) as err:
            counts_of(e, f, "w1000")
        assert "PD_DECODE_ROW_COUNTS" in str(err.value)
        assert e.profile_get("decode_row_counts") == (0.0, 0)
        check_depth(e, f["lens"], dep)
    with pda.Engine(f["lens"]) as e:                                                       # the flag without a table: refused, and the context is as it was
        s = e.decode_session()
        with pytest.raises(pda.PdError) as err:
            s.begin(flt[0], flt[1], flags=pda.PD_DECODE_ROW_COUNTS)
        assert "pd_decode_row_bins" in str(err.value)
        check_counts(e, f, "w1000", flt, run_plain(e, f["cuts"]["3"], flt, row_counts=table(f, "w1000")))
    with pda.Engine(f["lens"]) as e:                                                       # a session with the flag, then one without: refused again
        check_counts(e, f, "w1000", flt, run_plain(e, f["cuts"]["3"], flt, row_counts=table(f, "w1000")))
        run_plain(e, f["cuts"]["3"], flt)                                                  # (no reset: the flag does not stick to the context)
        with pytest.raises(pda.PdError):
            counts_of(e, f, "w1000")
        assert counter(e, "decode_row_counts") == 0
        check_depth(e, f["lens"], [None if d is None else 2 * d for d in dep])             # (the depth of both sessions, as it would be without the flag)


def test_bad_tables(corpus):
    f = corpus["corpus"]
    flt = B.FILTERS[0]
    n = len(f["lens"])
    with pda.Engine(f["lens"]) as e:
        s = e.decode_session()
        off = np.zeros(n + 1, dtype=np.uint64); off[1:] = 3
        U64P, U32P = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        for edges, what in (([5, 5, 9], "strictly ascending"), ([9, 5, 12], "strictly ascending")):
            with pytest.raises(pda.PdError) as err:
                s.row_bins("edges", off, np.array(edges, dtype=np.uint32))
            assert what in str(err.value)
        ed = np.array([1, 2, 3], dtype=np.uint32)
        with pytest.raises(pda.PdError) as err:                                            # w > 0 with edges
            e._ck(e.L.pd_decode_row_bins(e.h, 1000, off.ctypes.data_as(U64P), ed.ctypes.data_as(U32P)))
        assert "takes no edges" in str(err.value)
        many = np.zeros(n + 1, dtype=np.uint64); many[1:] = (1 << 28) + 1                  # too many bins (refused before an edge is read)
        with pytest.raises(pda.PdError) as err:
            s.row_bins("edges", many, ed)
        assert "2^28" in str(err.value)
        down = off.copy(); down[2] = 1
        with pytest.raises(pda.PdError):
            s.row_bins("edges", down, ed)
        # none of them left a table: the flag is still refused; and a good table after them counts
        with pytest.raises(pda.PdError):
            s.begin(flt[0], flt[1], flags=pda.PD_DECODE_ROW_COUNTS)
        check_counts(e, f, "regions", flt, run_plain(e, f["cuts"]["3"], flt, row_counts=table(f, "regions")))
