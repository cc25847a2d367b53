"""The device record walk (pandepth_amd/csrc/pd_bamwalk.h on the MI355X: the speculative 64-lane walk, the wave-walked CIGARs of
COOP_MIN operations and more, CIGARs in the CG tag, compact emission, the chain confirmed on the device) on the crafted corpus of
tests/bam_craft.py — operation counts 1 .. 65 535 on both sides of COOP_MIN and of the 64-operation step, first runs at operation
0 / 63 / 64 / 65 behind clips and behind gaps, CIGARs without a run, records that start 1 .. 37 bytes before the end of a lane's
stretch, of a segment and of a unit, records longer than a stretch and than a segment, Z tags that look like record headers —
against a reference written from the SAM specification that two CPU implementations agree with (tests/test_bamwalk_edges.py).
All comparisons are exact; no unit may be handed back."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import pandepth_amd as pda

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
ORACLE_CLI = os.path.join(HERE, "harness", "pandepth_oracle_cli")
SORTED_FILES = ["alone", "packed", "layout", "few"]
SPLITS = [(n, s) for n in SORTED_FILES for s in ("1", "3", "64")] + [("layout", "crafted")]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("edges_gpu")
    files = B.build_corpus(d)                                     # (asserts that every named case is present)
    sub, seg, _ = B.walk_geometry()
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    for name, f in files.items():
        if name != "unsorted":                                    # (the indexer refuses a file that is not in coordinate order)
            subprocess.run([os.path.join(ROOT, "pandepth_amd", "pandepth_index"), f["path"]], check=True)
        f["splits"] = B.splits_of(f, name, seg)
        f["depth"] = {flt: B.reference_depth(f["lens"], f["recs"], *flt)[0] for flt in B.FILTERS}      # computed once, shared, never changed
        for dep in f["depth"].values():
            for x in dep:
                if x is not None:
                    x.setflags(write=False)
    # target spans that meet the special reads only through a later run, or only through the one-base end of a read without
    # reference bases (no CIGAR, unmapped, only clips and insertions); and plain ones
    at = lambda name, case: next(r for r in files[name]["recs"] if r["off"] == files[name]["cases"][case])
    spans = [("big", 350060, 350100), ("big", 350200, 350260)]
    for case in ("no_cigar_placed", "unmapped_placed_q30", "unmapped_placed_with_cigar", "no_reference_bases_100"):
        spans.append(("big", at("alone", case)["pos"], at("alone", case)["pos"] + 1))
    r = at("alone", "ops65535")
    b, e = B.runs_of(r)
    spans += [("big", int(b[-1]), int(e[-1])), ("big", int(b[b.size // 2]), int(b[b.size // 2]) + 1), ("big", 100, 130), ("small", 0, 100), ("small", 4990, 5000), ("mid", 69900, 70000)]
    with open(os.path.join(str(d), "t.bed"), "w") as fh:
        fh.write("".join("%s\t%d\t%d\tt%d\n" % (c, s, e, k) for k, (c, s, e) in enumerate(sorted(spans))))
    files["dir"] = str(d)
    return files


def _push_and_compare(f, units, flag_mask, min_mapq, params=()):
    lens = f["lens"]
    dep = f["depth"][(flag_mask, min_mapq)]
    with pda.Engine(lens) as e:
        for k, v in params:
            e.set_param(k, v)
        st, nrec = e.push_bgzf_units(f["data"], f["blocks"], units, len(f["inf"]), flag_mask, min_mapq)
        assert not st.any(), list(st)                             # (a hand-back would hide the walk behind the host reader)
        assert nrec == len(f["offs"])
        e.scan(0)
        for t, ln in enumerate(lens):
            if ln >= 2:
                got = e.read_depth(t, 0, ln)
                bad = np.flatnonzero(got != dep[t])
                assert bad.size == 0, (t, bad[:8], got[bad[:8]], dep[t][bad[:8]])


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("name,split", SPLITS, ids=["%s_units_%s" % s for s in SPLITS])
def test_unit_splits(corpus, name, split, flag_mask, min_mapq):
    f = corpus[name]
    units = f["splits"][split]
    if split in ("1", "3"):
        assert len(units) == int(split)
    _push_and_compare(f, units, flag_mask, min_mapq)


VARIANTS = [
    ("spoil_every", [("decode_spoil", 1)]),
    ("spoil_third", [("decode_spoil", 3)]),
    ("spoil_left_to_host", [("decode_spoil", 2), ("decode_max_redo", 1)]),
    ("host_chain", [("decode_fast", 0)]),
    ("near_span_1024", [("decode_near_span", 1024)]),            # no wave-walked CIGARs; the far stream on
]


@pytest.mark.parametrize("vname,params", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("name", SORTED_FILES)
def test_parameter_variants(corpus, name, vname, params):
    f = corpus[name]
    for split in ("1", "crafted" if name == "layout" else "3"):
        _push_and_compare(f, f["splits"][split], 1796, -1, params)


CLI_CASES = [
    ("chr", ["-i", "{f}.bam"], ["chr.stat.gz"]),
    ("w10000", ["-i", "{f}.bam", "-w", "10000"], ["win.stat.gz"]),
    ("bed", ["-i", "{f}.bam", "-b", "t.bed"], ["bed.stat.gz"]),
    ("noindex", ["-i", "{f}.bam", "-s"], ["chr.stat.gz"]),
]


def _run(exe, args, tag, cwd, tune=None):
    env = dict(os.environ, PANDEPTH_TIMING="1")
    if tune:
        env["PANDEPTH_TUNE"] = tune
    p = subprocess.run([exe] + args + ["-o", tag, "-t", "4"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode()[-600:]
    return p.stderr.decode()


@pytest.mark.parametrize("mode,args,suffixes", CLI_CASES, ids=[c[0] for c in CLI_CASES])
@pytest.mark.parametrize("name", ["alone", "packed", "layout"])
def test_cli_equals_oracle_cli(corpus, name, mode, args, suffixes):
    """the executable (compact emission in the whole-contig modes, the region test on the device with -b, guessed unit starts
    without the index) = the product's host code on the oracle engine, byte for byte; nothing handed back, nothing declined"""
    d = corpus["dir"]
    args = [a.format(f=name) for a in args]
    _run(ORACLE_CLI, args, "o_%s_%s" % (name, mode), d)
    for tune in (None, "dd_batch_mb=1"):
        tag = "p_%s_%s_%s" % (name, mode, "dd1" if tune else "def")
        err = _run(CLI, args, tag, d, tune)
        for s in suffixes:
            assert open(os.path.join(d, tag + "." + s), "rb").read() == open(os.path.join(d, "o_%s_%s.%s" % (name, mode, s)), "rb").read(), (tune, s)
        m = re.search(r"device decode: (\d+) batches.*?(\d+) records on the device, (\d+) units handed back", err)
        assert m and int(m.group(1)) >= 1 and int(m.group(3)) == 0 and "DECLINED" not in err, err[-800:]


@pytest.mark.parametrize("name", ["packed", "layout"])
def test_cli_chain_repaired_on_the_device(corpus, name):
    """spoilt guesses in the executable's compact session: the device walks segments again (the count the engine reports), same bytes"""
    d = corpus["dir"]
    _run(ORACLE_CLI, ["-i", name + ".bam"], "o_%s_spoil" % name, d)
    err = _run(CLI, ["-i", name + ".bam"], "p_%s_spoil" % name, d, "dd_batch_mb=1,decode_spoil=1")
    assert open(os.path.join(d, "p_%s_spoil.chr.stat.gz" % name), "rb").read() == open(os.path.join(d, "o_%s_spoil.chr.stat.gz" % name), "rb").read()
    m = re.search(r"chain confirmed on the device for (\d+) batches, by the host for (\d+); segments the device walked again: (\d+)", err)
    assert m, err[-800:]
    dev, host, redo = (int(x) for x in m.groups())
    assert redo > 0 and dev + host > 0, (dev, host, redo)
    # `packed` is one batch whose later runs (the 65 535-operation and CG-tag reads: ~137 000 runs in 3 MB) outnumber the slots a batch's
    # array has (a slot per 41 inflated bytes): the chain kernel repairs the segments, counts, finds no room (CH_ROOM) and leaves the
    # batch to the host's chain, as pd_capi.hip documents; `layout` has no later runs and is confirmed on the device
    if name == "layout":
        assert dev > 0 and host == 0, (dev, host, redo)


def test_unsorted_file_falls_back(corpus):
    """two adjacent records out of coordinate order under a header that says SO:coordinate: the order check that rides on the
    emission makes the session decline (the host reader takes the file); the table is the oracle's"""
    d = corpus["dir"]
    _run(ORACLE_CLI, ["-i", "unsorted.bam"], "o_unsorted", d)
    for tune in (None, "dd_batch_mb=1"):
        err = _run(CLI, ["-i", "unsorted.bam"], "p_unsorted", d, tune)
        assert open(os.path.join(d, "p_unsorted.chr.stat.gz"), "rb").read() == open(os.path.join(d, "o_unsorted.chr.stat.gz"), "rb").read()
        assert "DECLINED (the records are not in the order SO:coordinate promises" in err, err[-800:]
