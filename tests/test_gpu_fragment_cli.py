"""`pandepth -frag` on the MI355X: the executable with the device decode on (the `-frag` kernels of the record walk) on the golden
pair file f7 and on the fragment corpus of tests/frag_model.py — against its own host decode (`-X device_decode=0`) byte for byte,
and against the model there."""
import os
import subprocess

import numpy as np
import pytest

import frag_model as FM
from test_count_deletions_cli import cover_total, rows_of, same_sites, sites, stat

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")

MODES = [("chr", []), ("sites", ["-a"]), ("w1000", ["-w", "1000"]), ("w8192", ["-w", "8192"]), ("del", ["-del", "-a"]),
         ("fragmax", ["-fragmax", str(FM.FRAGMAX_CASE), "-a"]), ("q20", ["-q", "20", "-a"])]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{name: (BAM path, contig names, lens, the model's records)}"""
    f = FM.fragment_corpus(tmp_path_factory.mktemp("frag_gpu_cli"))
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f7", "m.sam"))
    return {"frag": (f["path"], f["names"], f["lens"], f["model_recs"]), "f7": (os.path.join(GOLDEN, "f7", "m.bam"), names, lens, recs)}


def run(args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([CLI] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(GOLDEN, "f7"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, PANDEPTH_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p.stderr.decode(), {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def model_args(margs):
    kw = dict(count_del="-del" in margs)
    if "-fragmax" in margs:
        kw["frag_max"] = int(margs[margs.index("-fragmax") + 1])
    if "-q" in margs:
        kw["min_mapq"] = int(margs[margs.index("-q") + 1])
    return kw


@pytest.mark.parametrize("mode,margs", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name", ["f7", "frag"])
def test_device_decode_equals_host_decode_and_the_model(inputs, name, mode, margs, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    path, names, lens, recs = inputs[name]
    args = ["-i", path, "-frag"] + margs
    err, got = run(args, str(tmp_path / "dev"))
    assert "device decode:" in err and "DECLINED" not in err and " 0 units handed back" in err, err[-800:]
    _, host = run(args + ["-X", "device_decode=0"], str(tmp_path / "host"))
    assert got and (host == got) is True
    dep = FM.model(lens, recs, **model_args(margs))[0]
    kept = [(n, d) for n, d in zip(names, dep) if d is not None]
    if "-a" in margs:
        assert same_sites(sites(got), names, dep)
    if "-w" in margs:
        head, rows = rows_of(got, "win.stat.gz")
        assert rows and cover_total(head, rows) == [stat(dep[names.index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
    else:
        head, rows = rows_of(got, "chr.stat.gz")
        assert [r[0] for r in rows] == [n for n, _ in kept] and cover_total(head, rows) == [stat(d, 1) for _, d in kept]
    _, plain = run([a for a in args if a != "-frag" and a != "-fragmax" and a != str(FM.FRAGMAX_CASE)] + ["-s"], str(tmp_path / "plain"))
    assert (plain != got) is True                                     # (both inputs hold fragments)
