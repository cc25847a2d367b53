"""Whole fragments of properly paired reads on the MI355X: the `-frag` instances of the device record walk (pd_bamwalk.h, FRAG = true:
a properly paired read with tlen > 0 is the one run [pos, pos + tlen), its mate none) through pd_push_bgzf_units ("decode_fragments",
"decode_frag_max") and through a decode session (PD_DECODE_FRAGMENTS), on the fragment corpus of tests/frag_model.py against the
model there, and on the bam_craft corpus, none of whose records is a fragment read (its writer leaves the mate fields -1, -1, 0), so
that its depth is the plain depth.  All comparisons are exact; no unit may be handed back — a hand-back would hide the walk behind
the host reader."""
import numpy as np
import pytest

import bam_craft as B
import del_model as DM
import frag_model as FM
import pandepth_amd as pda
from test_gpu_decode_session import check_depth, counter, run_compact, run_plain, windows_of

pytestmark = pytest.mark.gpu
CRAFT = ["alone", "packed", "layout", "few"]
FILES = ["frag"] + CRAFT
SPLITS = [(n, s) for n in FILES for s in ("1", "3", "64")] + [("layout", "crafted"), ("frag", "crafted")]


def frozen(dep):
    for x in dep:
        if x is not None:
            x.setflags(write=False)
    return dep


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """every model computed once, shared, never changed"""
    d = tmp_path_factory.mktemp("frag_gpu")
    files = B.build_corpus(d)
    files["frag"] = FM.fragment_corpus(d)
    _, seg, _ = B.walk_geometry()
    for name in CRAFT:
        f = files[name]
        f["splits"] = B.splits_of(f, name, seg)
        f["cuts"] = B.session_cuts(f, name)
        recs = FM.records_of(f["inf"], f["recs"])
        assert all(FM.fragment_class(r) == 0 for r in recs)
        f["plain"] = {flt: frozen(B.reference_depth(f["lens"], f["recs"], *flt)[0]) for flt in B.FILTERS}
        f["model"] = {flt: (f["plain"][flt],) + DM.model(f["lens"], DM.crafted_records(f["recs"]), *flt, count_del=False)[1:] for flt in B.FILTERS}
    f = files["frag"]
    f["splits"] = FM.splits_of(f)
    f["cuts"] = B.session_cuts(f, "frag")
    f["model"], f["plain"] = {}, {}
    for flt in B.FILTERS:
        dep, nf, no = FM.model(f["lens"], f["model_recs"], *flt)
        f["model"][flt] = (frozen(dep), nf, no)
        f["plain"][flt] = frozen(DM.model(f["lens"], FM.plain_records(f["model_recs"]), *flt, count_del=False)[0])
        assert any(not np.array_equal(a, b) for a, b in zip(dep, f["plain"][flt]))            # (not vacuous)
    return files


def push_and_compare(f, units, flt, params=(), dep=None, **kw):
    dep = f["model"][flt][0] if dep is None else dep
    with pda.Engine(f["lens"]) as e:
        for k, v in params:
            e.set_param(k, v)
        st, nrec = e.push_bgzf_units(f["data"], f["blocks"], units, len(f["inf"]), flt[0], flt[1], fragments=True, **kw)
        assert not st.any(), list(st)
        assert nrec == len(f["offs"])
        check_depth(e, f["lens"], dep)


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("name,split", SPLITS, ids=["%s_units_%s" % s for s in SPLITS])
def test_unit_splits(corpus, name, split, flt):
    push_and_compare(corpus[name], corpus[name]["splits"][split], flt)


@pytest.mark.parametrize("params", [[("decode_spoil", 1)], [("decode_fast", 0)]], ids=["spoil_every", "host_chain"])
@pytest.mark.parametrize("name", ["alone", "frag"])
def test_parameter_variants(corpus, name, params):
    f = corpus[name]
    for split in ("1", "3"):
        push_and_compare(f, f["splits"][split], B.FILTERS[0], params)


def test_push_with_a_bound_and_with_deletions(corpus):
    f = corpus["frag"]
    flt = B.FILTERS[0]
    bound = frozen(FM.model(f["lens"], f["model_recs"], *flt, frag_max=FM.FRAGMAX_CASE)[0])
    both = frozen(FM.model(f["lens"], f["model_recs"], *flt, count_del=True)[0])
    assert any(not np.array_equal(a, b) for a, b in zip(bound, f["model"][flt][0])) and any(not np.array_equal(a, b) for a, b in zip(both, f["model"][flt][0]))
    push_and_compare(f, f["splits"]["3"], flt, dep=bound, frag_max=FM.FRAGMAX_CASE)
    push_and_compare(f, f["splits"]["3"], flt, dep=both, count_deletions=True)


def test_the_flag_does_not_outlive_the_call(corpus):
    f = corpus["frag"]
    flt = B.FILTERS[0]
    with pda.Engine(f["lens"]) as e:
        st, _ = e.push_bgzf_units(f["data"], f["blocks"], f["splits"]["1"], len(f["inf"]), *flt, fragments=True, frag_max=FM.FRAGMAX_CASE)
        assert not st.any()
        e.reset()
        st, _ = e.push_bgzf_units(f["data"], f["blocks"], f["splits"]["1"], len(f["inf"]), *flt)
        assert not st.any()
        check_depth(e, f["lens"], f["plain"][flt])
        e.reset()
        st, _ = e.push_bgzf_units(f["data"], f["blocks"], f["splits"]["1"], len(f["inf"]), *flt, fragments=True)      # (nor does the bound)
        assert not st.any()
        check_depth(e, f["lens"], f["model"][flt][0])


@pytest.mark.parametrize("flt", B.FILTERS, ids=["flag1796", "mapq20"])
@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("name", FILES)
def test_decode_session(corpus, name, compact, flt):
    """one begin(fragments=True) on a sorted file, with and without PD_DECODE_COMPACT + n_batches: the depth (cells, and windows of 8192
    from the deferred sample) and the results' run counts are the model's; the same context without the flag on the same bytes gives
    the plain depth again"""
    f = corpus[name]
    batches = f["cuts"]["3"]
    dep, n_first, n_other = f["model"][flt]
    run = run_compact if compact else run_plain
    with pda.Engine(f["lens"]) as e:
        results = run(e, batches, flt, fragments=True)
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
        run(e, batches, flt, fragments=True)
        _, cover, tot = e.scan_reduce_windows(8192, 1, 0)
        cov_ref, tot_ref = windows_of(f["lens"], dep, 8192, 1)
        assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref)


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("kw", [dict(count_deletions=True), dict(frag_max=FM.FRAGMAX_CASE)], ids=["with_deletions", "with_a_bound"])
def test_session_combinations(corpus, kw, compact):
    f = corpus["frag"]
    flt = B.FILTERS[0]
    dep, n_first, n_other = FM.model(f["lens"], f["model_recs"], *flt, count_del=bool(kw.get("count_deletions")), frag_max=kw.get("frag_max", FM.NO_BOUND))
    assert any(not np.array_equal(a, b) for a, b in zip(dep, f["model"][flt][0]))
    with pda.Engine(f["lens"]) as e:
        results = (run_compact if compact else run_plain)(e, f["cuts"]["3"], flt, fragments=True, **kw)
        assert all(not st.any() for st, _ in results)
        assert (sum(r["n_first"] for _, r in results), sum(r["n_other"] for _, r in results)) == (n_first, n_other)
        check_depth(e, f["lens"], dep)
        e.reset()
        results = run_plain(e, f["cuts"]["3"], flt, fragments=True)  # (the bound is each begin's own argument)
        check_depth(e, f["lens"], f["model"][flt][0])


def test_session_with_spans(corpus):
    """-g / -b sessions: a read counts when [pos, endpos) meets a span, and a carrying read's endpos is its fragment's end — spans that
    only fragment interiors reach select the pairs around them, whose left mates end long before"""
    f = corpus["frag"]
    flt = B.FILTERS[0]
    spans = {0: [(60209, 60290), (63199, 63800)], 1: [(29999, 30100)], 2: []}            # (begin0, end) per contig, sorted
    span_off = np.cumsum([0] + [len(spans[t]) for t in range(len(f["lens"]))]).astype(np.uint32)
    flat = np.array([x for t in range(len(f["lens"])) for x in spans[t]], dtype=np.int32).reshape(-1, 2)
    picked = []
    for r in f["model_recs"]:
        if r[2] & flt[0] or r[3] < flt[1]:
            continue
        end = FM.region_endpos(r)
        if any(r[1] < e and end > b for b, e in spans[r[0]]):
            picked.append(r)
    dep, n_first, n_other = FM.model(f["lens"], picked, *flt)
    assert n_first >= 4 and all(int(dep[t][b:e].min()) >= 1 for t in spans for b, e in spans[t])
    assert all(int(f["plain"][flt][t][b:e].max()) == 0 for t in spans for b, e in spans[t])
    with pda.Engine(f["lens"]) as e:
        results = run_plain(e, f["cuts"]["3"], flt, fragments=True, span_off=span_off, spans=flat)
        assert all(not st.any() for st, _ in results)
        assert (sum(r["n_first"] for _, r in results), sum(r["n_other"] for _, r in results)) == (n_first, n_other)
        check_depth(e, f["lens"], dep)
