"""Deletions counted as covered on the MI355X: the `-del` instance of the device record walk (pd_bamwalk.h, DEL = true: one run per
group of M/=/X/D operations that no N splits — the lane walk and the wave-walked CIGARs of 96 operations and more) through
pd_push_bgzf_units ("decode_deletions") and through a decode session (PD_DECODE_DELETIONS), on the bam_craft corpus and on the
deletion corpus of tests/del_model.py, against the model there.  All comparisons are exact; no unit may be handed back — a
hand-back would hide the walk behind the host reader."""
import numpy as np
import pytest

import bam_craft as B
import del_model as DM
import pandepth_amd as pda
from test_gpu_decode_session import check_depth, counter, run_compact, run_plain, windows_of

pytestmark = pytest.mark.gpu
FILES = ["alone", "packed", "layout", "few", "del"]
SPLITS = [(n, s) for n in FILES for s in ("1", "3", "64")] + [("layout", "crafted")]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("del_gpu")
    files = B.build_corpus(d)
    files["del"] = DM.deletion_corpus(d)
    _, seg, _ = B.walk_geometry()
    for name in FILES:
        f = files[name]
        recs = DM.crafted_records(f["recs"])
        f["splits"] = B.splits_of(f, name, seg)
        f["cuts"] = B.session_cuts(f, name)
        f["model"] = {flt: DM.model(f["lens"], recs, *flt) for flt in B.FILTERS}          # computed once, shared, never changed
        f["plain"] = {flt: B.reference_depth(f["lens"], f["recs"], *flt)[0] for flt in B.FILTERS}
        for dep in [m[0] for m in f["model"].values()] + list(f["plain"].values()):
            for x in dep:
                if x is not None:
                    x.setflags(write=False)
        if name != "layout":                                      # (not vacuous: the deletions change this file's depth; layout's reads are 50M)
            assert any(not np.array_equal(a, b) for a, b in zip(f["model"][B.FILTERS[0]][0], f["plain"][B.FILTERS[0]]) if a is not None)
    return files


def push_and_compare(f, units, flt, params=()):
    dep = f["model"][flt][0]
    with pda.Engine(f["lens"]) as e:
        for k, v in params:
            e.set_param(k, v)
        st, nrec = e.push_bgzf_units(f["data"], f["blocks"], units, len(f["inf"]), flt[0], flt[1], count_deletions=True)
        assert not st.any(), list(st)
        assert nrec == len(f["offs"])
        check_depth(e, f["lens"], dep)


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("name,split", SPLITS, ids=["%s_units_%s" % s for s in SPLITS])
def test_unit_splits(corpus, name, split, flt):
    push_and_compare(corpus[name], corpus[name]["splits"][split], flt)


@pytest.mark.parametrize("params", [[("decode_spoil", 1)], [("decode_fast", 0)]], ids=["spoil_every", "host_chain"])
@pytest.mark.parametrize("name", ["alone", "del"])
def test_parameter_variants(corpus, name, params):
    f = corpus[name]
    for split in ("1", "3"):
        push_and_compare(f, f["splits"][split], B.FILTERS[0], params)


def test_the_flag_does_not_outlive_the_call(corpus):
    f = corpus["del"]
    flt = B.FILTERS[0]
    with pda.Engine(f["lens"]) as e:
        st, _ = e.push_bgzf_units(f["data"], f["blocks"], f["splits"]["1"], len(f["inf"]), *flt, count_deletions=True)
        assert not st.any()
        e.reset()
        st, _ = e.push_bgzf_units(f["data"], f["blocks"], f["splits"]["1"], len(f["inf"]), *flt)
        assert not st.any()
        check_depth(e, f["lens"], f["plain"][flt])


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("name", FILES)
def test_decode_session(corpus, name, compact, flt):
    """one begin(count_deletions=True) on a sorted file, with and without PD_DECODE_COMPACT + n_batches: the depth (cells, and windows
    of 8192 from the deferred sample) and the results' run counts are the model's; the same context without the flag on the same
    bytes gives the reference depth again"""
    f = corpus[name]
    batches = f["cuts"]["3"]
    dep, n_first, n_other = f["model"][flt]
    run = run_compact if compact else run_plain
    with pda.Engine(f["lens"]) as e:
        results = run(e, batches, flt, count_deletions=True)
        assert all(not st.any() for st, _ in results), [list(st) for st, _ in results]
        assert sum(r["n_reads"] for _, r in results) == len(f["offs"])
        assert (sum(r["n_first"] for _, r in results), sum(r["n_other"] for _, r in results)) == (n_first, n_other)
        # how pd_decode_end made the sample: a compact session as ONE compact sample or, where it cannot be one, 12-byte runs; a plain one by scatter
        if compact:
            assert counter(e, "decode_end_compact") + counter(e, "decode_end_c8_fallback") == 1 and counter(e, "decode_end_scatter") == 0
        else:
            assert counter(e, "decode_end_scatter") == 1 and counter(e, "decode_end_compact") == 0
        check_depth(e, f["lens"], dep)
        e.reset()
        results = run(e, batches, flt)                                # (the flag does not stick to the context)
        assert all(not st.any() for st, _ in results)
        check_depth(e, f["lens"], f["plain"][flt])
    with pda.Engine(f["lens"]) as e:
        e.keep_deferred(True)
        run(e, batches, flt, count_deletions=True)
        _, cover, tot = e.scan_reduce_windows(8192, 1, 0)
        cov_ref, tot_ref = windows_of(f["lens"], dep, 8192, 1)
        assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref)
