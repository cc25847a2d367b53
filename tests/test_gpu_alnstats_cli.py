"""`pandepth -alnstats` on the MI355X: the executable with the device decode on (k_aln_stats behind every batch) on `aln_edges` of
tests/alnstats_model.py, on bam_craft's `alone` (CIGARs of up to 70 001 operations, CG tags) and on the goldens f1 and f7, indexed and
`-s` — against its own host decode (`-X device_decode=0`) byte for byte, and against the model; and every other output against the run
without the option."""
import gzip
import os
import re
import subprocess

import pytest

import alnstats_model as AM
import bam_craft as B
import frag_model as FM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
STAT = "o.aln.stat.gz"
W = 100


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{name: (BAM path, number of contigs, records, how the model takes them)}"""
    d = tmp_path_factory.mktemp("alnstats_gpu_cli")
    f = AM.edges_file(d)
    out = {"aln_edges": (f["path"], len(f["lens"]), f["recs"], "parsed")}
    f = B.build_corpus(d)["alone"]
    out["alone"] = (f["path"], len(f["lens"]), f["recs"], "parsed")
    for fx, sam, bam in (("f1", "f1.sam", "f1.bam"), ("f7", "m.sam", "m.bam")):
        names, lens, recs = FM.read_sam(os.path.join(GOLDEN, fx, sam))
        out[fx] = (os.path.join(GOLDEN, fx, bam), len(lens), recs, "tuples")
    return out


def run(args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([CLI] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(GOLDEN, "f7"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, PANDEPTH_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p.stderr.decode(), {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


MODES = [("chr", []), ("s", ["-s"]), ("sites", ["-a"]), ("w8192_q20", ["-w", "8192", "-q", "20"]), ("x0_s", ["-x", "0", "-s"])]
CASES = [(n, m) for n in ("f1", "f7") for m in MODES] + [(n, m) for n in ("aln_edges", "alone") for m in (MODES[0], MODES[3], ("x0", ["-x", "0"]))]


@pytest.mark.parametrize("name,mode", CASES, ids=["%s_%s" % (n, m[0]) for n, m in CASES])
def test_device_decode_equals_host_decode_and_the_model(inputs, name, mode, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    path, n_ref, recs, how = inputs[name]
    margs = mode[1]
    args = ["-i", path, "-alnstats", str(W)] + margs
    err, got = run(args, str(tmp_path / "dev"))
    assert "device decode:" in err and "DECLINED" not in err and " 0 units handed back" in err, err[-800:]
    m = re.search(r"alignment statistics: (\d+) records counted on the device", err)
    assert m and int(m.group(1)) == len(recs) and "k_aln_stats:" in err, err[-800:]     # every record, on the device
    _, host = run(args + ["-X", "device_decode=0"], str(tmp_path / "host"))
    assert STAT in got and got[STAT] == host[STAT] and (host == got) is True            # (the .gz bytes)
    x = int(margs[margs.index("-x") + 1]) if "-x" in margs else 1796
    q = int(margs[margs.index("-q") + 1]) if "-q" in margs else -1
    model = AM.Model(n_ref, x, q, W)
    (model.add_parsed if how == "parsed" else model.add_tuples)(recs)
    assert gzip.decompress(got[STAT]).decode() == model.text()
    err0, plain = run(["-i", path] + margs, str(tmp_path / "plain"))
    assert plain and STAT not in plain and all(got[f] == plain[f] for f in plain)
    assert "alignment statistics" not in err0 and "k_aln_stats" not in err0
