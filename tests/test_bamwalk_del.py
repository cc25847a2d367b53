"""The device walk's `-del` instance (pandepth_amd/csrc/pd_bamwalk.h with DEL = true: one run per group of M/=/X/D operations that
no N splits) with its 64 lanes emulated on the host (tests/harness/bamwalk_del_check), both passes, on the whole bam_craft corpus
and on the deletion corpus of tests/del_model.py — against the model there: the depth of the emitted runs, the numbers of first and
other runs, pass 2 writing exactly what pass 1 counted, and the wave-walked CIGARs giving the runs the lane-walked ones give.
No GPU here; tests/test_gpu_count_deletions.py runs the same files through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import del_model as DM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = os.path.join(HERE, "harness")
FILES = ["alone", "packed", "layout", "few", "unsorted", "del"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("del_edges")
    files = B.build_corpus(d)
    files["del"] = DM.deletion_corpus(d)
    return files


@pytest.fixture(scope="module")
def walker():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(H, "bamwalk_del_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(H, "bamwalk_del_check.cpp"),
                    os.path.join(ROOT, "pandepth_amd", "libpandepth_host.a"), "-lz", "-ldl", "-o", exe], check=True)
    return exe


def walk(walker, corpus, opts, tag):
    """-> {file: (n_records, n_first, n_other + n_far, runs (n, 3) int32)}"""
    p = subprocess.run([walker] + opts + ["-tag", tag] + [corpus[n]["path"] for n in FILES], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0 and "DISAGREE" not in out, (out[-1500:], p.stderr.decode()[-400:])       # (pass 1 and pass 2 agree)
    res = {}
    for name in FILES:
        line = next(l for l in out.splitlines() if l.startswith(corpus[name]["path"] + ":"))
        m = re.search(r": (\d+) records, \d+ segments, first runs (\d+), other runs (\d+), far runs (\d+), flags 0, passes agree", line)
        assert m, line
        runs = np.fromfile(corpus[name]["path"] + "." + tag + ".runs", dtype=np.int32).reshape(-1, 3)
        assert runs.shape[0] == int(m.group(2)) + int(m.group(3)) + int(m.group(4))
        res[name] = int(m.group(1)), int(m.group(2)), int(m.group(3)) + int(m.group(4)), runs
    return res


def depth_of(lens, runs):
    out = []
    for t, L in enumerate(lens):
        r = runs[runs[:, 0] == t].astype(np.int64)
        diff = np.zeros(L + 1, dtype=np.int64)
        np.add.at(diff, np.clip(r[:, 1], 0, L), 1)
        np.add.at(diff, np.clip(r[:, 2], 0, L), -1)
        out.append(np.cumsum(diff[:-1]).astype(np.uint32) if L >= 2 else None)
    return out


def test_the_deletion_corpus_holds_its_cases(corpus):
    f = corpus["del"]
    sub, seg, coop = B.walk_geometry()
    assert coop == 96 and all(r["size"] < 1500 for r in f["recs"] if B.real_cigar(r).size <= 192)
    sizes = {int(B.real_cigar(r).size) for r in f["recs"]}
    assert {95, 96, 127, 128, 129, 192, 65536} <= sizes
    big = [B.real_cigar(r) & 0xf for r in f["recs"] if B.real_cigar(r).size >= coop]
    for at in (63, 64, 65):
        assert any(c[at] == DM.D for c in big) and any(c[at] == DM.N for c in big)
    assert any(c[0] == DM.N for c in big) and any(c[-1] == DM.N for c in big) and any(((c[:-1] == DM.N) & (c[1:] == DM.N)).any() for c in big)
    assert any(c.size >= 192 and np.isin(c[64:128], (DM.D, DM.I)).all() for c in big)
    assert any(r["tid"] == 1 for r in f["recs"]) and any(r["pos"] + 20 > f["lens"][0] for r in f["recs"] if r["tid"] == 0)
    with_d, without = DM.model(f["lens"], DM.crafted_records(f["recs"]))[0], DM.model(f["lens"], DM.crafted_records(f["recs"]), count_del=False)[0]
    assert not np.array_equal(with_d[0], without[0])


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("seg", ["64", "4"])
def test_emulated_walk_equals_the_model(corpus, walker, flag_mask, min_mapq, seg):
    opts = ["-x", str(flag_mask), "-q", str(min_mapq), "-seg", seg]
    wave = walk(walker, corpus, opts, "wave")
    lane = walk(walker, corpus, opts + ["-near", "4294967294"], "lane")           # every CIGAR walked by its lane
    for name in FILES:
        f = corpus[name]
        dep, n_first, n_other = DM.model(f["lens"], DM.crafted_records(f["recs"]), flag_mask, min_mapq)
        n_rec, nf, no, runs = wave[name]
        assert n_rec == len(f["recs"]) and (nf, no) == (n_first, n_other), name
        got = depth_of(f["lens"], runs)
        assert all(g is None or np.array_equal(g, d) for g, d in zip(got, dep)), name
        assert sum(int(d.sum(dtype=np.uint64)) for d in dep if d is not None) > 0
        # the lane-walked and the wave-walked CIGARs: the same first runs in the same order, the same later runs
        _, lf, lo, lruns = lane[name]
        assert (lf, lo) == (nf, no) and np.array_equal(lruns[:lf], runs[:nf]), name
        assert np.array_equal(lruns[lf:][np.lexsort(lruns[lf:].T[::-1])], runs[nf:][np.lexsort(runs[nf:].T[::-1])]), name
