"""The record statistics pass (pandepth_amd/csrc/pd_recstats.h, the source k_record_stats compiles) with its 64 lanes emulated on the
host (tests/harness/recstats_check): the existing pass 1 and chain check, then the new core over the confirmed lanes — on the corpus of
tests/recstats_model.py and on bam_craft's crafted files, against the model there.  Everything is exact: the sums, the contig triples,
and `records` against the walk's own record count.  The harness is a stand-alone program built with -fsanitize=address,undefined and
run as its own process; its arrays are allocated at their exact sizes.
No GPU here; tests/test_gpu_recstats.py runs the same files through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import frag_model as FM
import recstats_model as RM

HERE = os.path.dirname(os.path.abspath(__file__))
H = os.path.join(HERE, "harness")
CRAFTED = ["alone", "packed", "layout", "few"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("recstats_walk")
    out = {"corpus": dict(RM.corpus(d), names=RM.NAMES)}
    crafted = B.build_corpus(d)
    for n in CRAFTED:
        f = crafted[n]
        out[n] = dict(f, names=B.NAMES, model_recs=FM.records_of(f["inf"], f["recs"]))
    return out


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(H, "recstats_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(H, "recstats_check.cpp"), "-lz", "-o", exe], check=True)
    return exe


def run(checker, f, opts, n_bins, tag):
    """-> (records the walk counted, sums, per_contig)"""
    p = subprocess.run([checker] + opts + ["-bins", str(n_bins), "-tag", tag, f["path"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, (out[-1500:], p.stderr.decode()[-1500:])                  # (no flag on any segment; no sanitizer report)
    m = re.search(r": (\d+) records walked, (\d+) counted, \d+ segments, (\d+) contigs, flags 0", out)
    assert m, out
    a = np.fromfile(f["path"] + "." + tag + ".rs", dtype=np.uint64)
    n_ref = int(m.group(3))
    assert a.size == RM.FIXED + n_bins + 1 + 3 * n_ref and int(m.group(2)) == int(a[0])
    return int(m.group(1)), a[:RM.FIXED + n_bins + 1], a[RM.FIXED + n_bins + 1:].reshape(n_ref, 3)


@pytest.mark.parametrize("n_bins", RM.BINS)
@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("seg", ["64", "4"])
@pytest.mark.parametrize("name", ["corpus"] + CRAFTED)
def test_emulated_pass_equals_the_model(files, checker, name, seg, flag_mask, min_mapq, n_bins):
    f = files[name]
    walked, sums, per = run(checker, f, ["-x", str(flag_mask), "-q", str(min_mapq), "-seg", seg], n_bins, "s%s_x%d_n%d" % (seg, flag_mask, n_bins))
    want_s, want_p = RM.Model(f["names"], f["lens"], flag_mask, min_mapq, n_bins).add_all(f["model_recs"]).arrays()
    assert walked == len(f["recs"]) == int(sums[RM.RECORDS])
    assert np.array_equal(sums, want_s), np.flatnonzero(sums != want_s)[:20]
    assert np.array_equal(per, want_p)
    assert int(sums[RM.UNPLACED:RM.KEPT + 1].sum()) == walked
