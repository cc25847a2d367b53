"""The device walk's `-frag` instances (pandepth_amd/csrc/pd_bamwalk.h with FRAG = true: a properly paired read with tlen > 0 is the
one run [pos, pos + tlen), its mate none) with their 64 lanes emulated on the host (tests/harness/bamwalk_frag_check), both passes,
on the fragment corpus of tests/frag_model.py — against the model there: the depth of the emitted runs, the numbers of first and
other runs, pass 2 writing exactly what pass 1 counted; and the default instance on the same bytes still gives the plain depth.
The harness is a stand-alone program built with -fsanitize=address,undefined and run as its own process.
No GPU here; tests/test_gpu_fragment.py runs the same file through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import del_model as DM
import frag_model as FM

HERE = os.path.dirname(os.path.abspath(__file__))
H = os.path.join(HERE, "harness")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return FM.fragment_corpus(tmp_path_factory.mktemp("frag_edges"))


@pytest.fixture(scope="module")
def walker():
    exe = os.path.join(H, "bamwalk_frag_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(H, "bamwalk_frag_check.cpp"), "-lz", "-o", exe], check=True)
    return exe


def walk(walker, f, opts, tag):
    """-> (n_records, n_first, n_other + n_far, runs (n, 3) int32)"""
    p = subprocess.run([walker] + opts + ["-tag", tag, f["path"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "DISAGREE" not in out, (out[-1500:], p.stderr.decode()[-1500:])            # (pass 1 and pass 2 agree; no sanitizer report)
    m = re.search(r": (\d+) records, \d+ segments, first runs (\d+), other runs (\d+), far runs (\d+), flags 0, passes agree", out)
    assert m, out
    runs = np.fromfile(f["path"] + "." + tag + ".runs", dtype=np.int32).reshape(-1, 3)
    assert runs.shape[0] == int(m.group(2)) + int(m.group(3)) + int(m.group(4))
    return int(m.group(1)), int(m.group(2)), int(m.group(3)) + int(m.group(4)), runs


def same_depth(lens, runs, dep):
    return all(g is None or np.array_equal(g, d) for g, d in zip(FM.depth_of_runs(lens, runs), dep))


MODES = [("frag", dict()), ("frag_del", dict(count_del=True)), ("frag_max", dict(frag_max=FM.FRAGMAX_CASE)), ("frag_max_del", dict(count_del=True, frag_max=FM.FRAGMAX_CASE))]


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("seg", ["64", "4"])
@pytest.mark.parametrize("mode,kw", MODES, ids=[m[0] for m in MODES])
def test_emulated_walk_equals_the_model(corpus, walker, flag_mask, min_mapq, seg, mode, kw):
    f = corpus
    opts = ["-x", str(flag_mask), "-q", str(min_mapq), "-seg", seg, "-frag", "1", "-del", "1" if kw.get("count_del") else "0"]
    if "frag_max" in kw:
        opts += ["-fragmax", str(kw["frag_max"])]
    dep, n_first, n_other = FM.model(f["lens"], f["model_recs"], flag_mask, min_mapq, **kw)
    n_rec, nf, no, runs = walk(walker, f, opts, "wave")
    assert n_rec == len(f["recs"]) and (nf, no) == (n_first, n_other)
    assert same_depth(f["lens"], runs, dep)
    # a carrying read's run is a FIRST run and begins at its pos: the first runs come in file order, so they are the kept reads' in order
    lane = walk(walker, f, opts + ["-near", "4294967294"], "lane")            # (every CIGAR walked by its lane: the same runs)
    assert (lane[1], lane[2]) == (nf, no) and np.array_equal(lane[3][:nf], runs[:nf])
    assert np.array_equal(lane[3][nf:][np.lexsort(lane[3][nf:].T[::-1])], runs[nf:][np.lexsort(runs[nf:].T[::-1])])
    # not vacuous: the rule changes this depth
    plain = DM.model(f["lens"], FM.plain_records(f["model_recs"]), flag_mask, min_mapq, count_del=bool(kw.get("count_del")))[0]
    assert any(not np.array_equal(a, b) for a, b in zip(dep, plain))


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
def test_the_fragment_runs_themselves(corpus, walker, flag_mask, min_mapq):
    """every carrying read that is kept leaves the run (tid, pos, (int32)(pos + tlen)) among the first runs, unclamped; a silent read leaves none"""
    f = corpus
    _, nf, _, runs = walk(walker, f, ["-x", str(flag_mask), "-q", str(min_mapq), "-frag", "1"], "runs")
    first = {tuple(int(v) for v in r) for r in runs[:nf]}
    n = 0
    for r in f["model_recs"]:
        if r[2] & flag_mask or r[3] < min_mapq or f["lens"][r[0]] < 2 or FM.fragment_class(r) != 1:
            continue
        assert (r[0], r[1], FM.wrap32(r[1] + r[6])) in first, r
        n += 1
    assert n > 1000


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("count_del", [False, True], ids=["default", "del"])
def test_the_instances_without_frag_give_the_plain_depth(corpus, walker, flag_mask, min_mapq, count_del):
    f = corpus
    dep, n_first, n_other = DM.model(f["lens"], FM.plain_records(f["model_recs"]), flag_mask, min_mapq, count_del=count_del)
    n_rec, nf, no, runs = walk(walker, f, ["-x", str(flag_mask), "-q", str(min_mapq), "-del", "1" if count_del else "0"], "plain")
    assert n_rec == len(f["recs"]) and (nf, no) == (n_first, n_other)
    assert same_depth(f["lens"], runs, dep)
