"""The row counting pass (pandepth_amd/csrc/pd_rowcounts.h, the source k_row_counts compiles) with its 64 lanes emulated on the host
(tests/harness/rowcounts_check): the existing pass 1 and chain check, then the new core over the confirmed lanes — on the corpus of
tests/rowreads_model.py, its unsorted file and bam_craft's crafted files, against the model there.  Everything is exact: every word of
every bin, and the bins' records against the model's count of records that start somewhere.  The harness is a stand-alone program
built with -fsanitize=address,undefined and run as its own process; its arrays are allocated at their exact sizes.
No GPU here; tests/test_gpu_rowreads.py runs the same files through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import frag_model as FM
import rowreads_model as RR

HERE = os.path.dirname(os.path.abspath(__file__))
H = os.path.join(HERE, "harness")
CRAFTED = ["alone", "packed", "layout", "few"]
FORMS = ["w1", "w7", "w1000", "w150000", "no_edges", "regions", "every_cell"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowreads_walk")
    out = {"corpus": RR.corpus(d), "unsorted": RR.unsorted(d)}
    crafted = B.build_corpus(d)
    for n in CRAFTED:
        f = crafted[n]
        out[n] = dict(f, names=B.NAMES, model_recs=FM.records_of(f["inf"], f["recs"]))
    for f in out.values():
        f["tables"] = RR.bin_tables(f["names"], f["lens"])
        f["want"] = {}
    check_forms(out)
    return out


def want(f, form, flt):
    """the model's bins, computed once per (file, form, filter)"""
    if (form, flt) not in f["want"]:
        _, rows, w = f["tables"][form]
        c = RR.Model(f["lens"], rows, flt[0], flt[1], uniform_w=w).add_all(f["model_recs"]).counts
        c.setflags(write=False)
        f["want"][(form, flt)] = c
    return f["want"][(form, flt)]


def check_forms(files):
    """the forms are not vacuous on these files, told from the model's bins (part of the fixture: it checks the tests' inputs, not the product)"""
    f = files["corpus"]
    flt = B.FILTERS[1]
    for form in FORMS:
        c = want(f, form, flt)
        assert (c[:, RR.RECORDS] > 0).sum() >= (3 if form in ("w150000", "no_edges") else 10), form
        assert c[:, RR.KEPT].sum() < c[:, RR.PASSED].sum() and c[:, RR.MAPQ0].sum() > 0 and 0 < c[:, RR.FORWARD].sum() < c[:, RR.KEPT].sum()
    assert len(want(f, "w7", flt)) == sum((ln + 6) // 7 for ln in f["lens"]) and f["lens"][0] % 7 and f["lens"][2] % 7      # short last windows
    u = want(files["unsorted"], "every_cell", flt)
    assert (u[:, RR.RECORDS] > 0).sum() >= 5000


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(H, "rowcounts_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(H, "rowcounts_check.cpp"), "-lz", "-o", exe], check=True)
    return exe


def run(checker, f, opts, table, tag):
    """-> (records the walk counted, counts[n_bins, 6])"""
    if table[0] == "w":
        opts = opts + ["-w", str(table[1])]
    elif table[1] is not None:
        off, flat = RR.edge_table(table[1])
        path = f["path"] + "." + tag + ".edges"
        with open(path, "wb") as out:
            out.write(off.tobytes() + flat.tobytes())
        opts = opts + ["-edges", path]
    p = subprocess.run([checker] + opts + ["-tag", tag, f["path"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, (out[-1500:], p.stderr.decode()[-1500:])                  # (no flag on any segment; no sanitizer report)
    m = re.search(r": (\d+) records walked, (\d+) started, (\d+) bins, \d+ segments, \d+ contigs, flags 0", out)
    assert m, out
    a = np.fromfile(f["path"] + "." + tag + ".rc", dtype=np.uint64)
    assert a.size == RR.WORDS * int(m.group(3))
    a = a.reshape(-1, RR.WORDS)
    assert int(m.group(2)) == int(a[:, RR.RECORDS].sum())
    return int(m.group(1)), a


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("seg", ["64", "4"])
@pytest.mark.parametrize("name", ["corpus", "unsorted"] + CRAFTED)
def test_emulated_pass_equals_the_model(files, checker, name, seg, flag_mask, min_mapq, form):
    f = files[name]
    table = f["tables"][form][0]
    walked, got = run(checker, f, ["-x", str(flag_mask), "-q", str(min_mapq), "-seg", seg], table, "s%s_x%d_%s" % (seg, flag_mask, form))
    exp = want(f, form, (flag_mask, min_mapq))
    assert walked == len(f["recs"])
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:20]
    assert int(got[:, RR.RECORDS].sum()) == RR.started(f["lens"], f["model_recs"])
