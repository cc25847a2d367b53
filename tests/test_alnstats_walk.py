"""The CIGAR statistics pass (pandepth_amd/csrc/pd_alnstats.h, the source k_aln_stats compiles) with its 64 lanes emulated on the host
(tests/harness/alnstats_check): the existing pass 1 and chain check, then the new core over the confirmed lanes — on bam_craft's crafted
files (their OP_COUNTS are the cooperative edges, `layout` puts records 1, 4, 35 and 36 bytes from stretch, segment and unit ends) and on
`aln_edges` of tests/alnstats_model.py, against the model there.  Everything is exact.  The harness is a stand-alone program built with
-fsanitize=address,undefined and run as its own process; its arrays are allocated at their exact sizes.
No GPU here; tests/test_gpu_alnstats.py runs the same files through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import alnstats_model as AM
import bam_craft as B

HERE = os.path.dirname(os.path.abspath(__file__))
H = os.path.join(HERE, "harness")
CRAFTED = ["alone", "packed", "layout", "few"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("alnstats_walk")
    crafted = B.build_corpus(d)
    out = {n: crafted[n] for n in CRAFTED}
    out["aln_edges"] = AM.edges_file(d)
    return out


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(H, "alnstats_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(H, "alnstats_check.cpp"), "-lz", "-o", exe], check=True)
    return exe


def run(checker, f, opts, width, tag):
    """-> (records the walk counted, sums)"""
    p = subprocess.run([checker] + opts + ["-w", str(width), "-tag", tag, f["path"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, (out[-1500:], p.stderr.decode()[-1500:])                  # (no flag on any segment; no sanitizer report)
    m = re.search(r": (\d+) records walked, (\d+) counted, \d+ segments, (\d+) contigs, flags 0", out)
    assert m, out
    a = np.fromfile(f["path"] + "." + tag + ".as", dtype=np.uint64)
    assert a.size == AM.WORDS and int(m.group(2)) == int(a[0])
    return int(m.group(1)), a


@pytest.mark.parametrize("width", AM.WIDTHS)
@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("seg", ["64", "4"])
@pytest.mark.parametrize("name", CRAFTED + ["aln_edges"])
def test_emulated_pass_equals_the_model(files, checker, name, seg, flag_mask, min_mapq, width):
    f = files[name]
    walked, sums = run(checker, f, ["-x", str(flag_mask), "-q", str(min_mapq), "-seg", seg], width, "s%s_x%d_w%d" % (seg, flag_mask, width))
    want = AM.Model(len(f["lens"]), flag_mask, min_mapq, width).add_parsed(f["recs"]).array()
    assert walked == len(f["recs"]) == int(sums[AM.RECORDS])
    assert np.array_equal(sums, want), [(int(k), int(sums[k]), int(want[k])) for k in np.flatnonzero(sums != want)[:20]]
    assert sums[AM.INS:AM.INS + AM.INDEL_BINS + 1].sum() == sums[AM.OPS + 2] and sums[AM.DEL:AM.DEL + AM.INDEL_BINS + 1].sum() == sums[AM.OPS + 4]


def test_the_header_and_the_model_agree_on_the_layout():
    text = open(os.path.join(B.ROOT, "include", "pandepth_amd.h")).read()
    val = {}
    for name, expr in re.findall(r"#define\s+PD_ALNSTAT_(\w+)\s+(.+)", text):
        val[name] = eval(re.sub(r"PD_ALNSTAT_(\w+)", lambda m: str(val[m.group(1)]), expr))
    assert (val["RECORDS"], val["ALIGNED"], val["PRIMARY"], val["CLIPPED"], val["READ_MAX"], val["READ_BASES"], val["ALIGNED_BASES"], val["REF_BASES"]) == tuple(range(8))
    assert (val["OPS"], val["INS"], val["DEL"], val["AF"], val["RL"], val["AL"], val["WORDS"]) == (AM.OPS, AM.INS, AM.DEL, AM.AF, AM.RL, AM.AL, AM.WORDS)
    assert (val["LEN_BINS"], val["INDEL_BINS"]) == (8192, 256) == (AM.LEN_BINS, AM.INDEL_BINS)
