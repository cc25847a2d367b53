"""`pandepth -rowreads` on the MI355X: the executable with the device decode on (k_row_counts behind every batch) on the corpus of
tests/rowreads_model.py — against its own host decode (`-X device_decode=0`) byte for byte, and against the model there; every other
output against the run without the option; and the timing lines say that the device counted."""
import gzip
import os
import re
import subprocess

import pytest

import rowreads_model as RR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
STAT = "o.rowreads.stat.gz"


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowreads_gpu_cli")
    f = RR.corpus(d)
    f["bed"], f["gff"] = RR.write_regions(d)
    return f


def run(args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([CLI] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(GOLDEN, "f7"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, PANDEPTH_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p.stderr.decode(), {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def table_of(kind, f):
    """(the model's row set, uniform w, the header's mode, the run's arguments)"""
    if kind == "chr":
        return RR.rows_chr(f["lens"]), 0, "chr", []
    if kind[0] == "w":
        w = int(kind[1:])
        return RR.rows_windows(f["lens"], w), w, "w", ["-w", kind[1:]]
    rows = RR.rows_regions(f["names"], f["lens"], RR.REGIONS)
    return (rows, 0, "g", ["-g", f["gff"], "-s"]) if kind == "gff" else (rows, 0, "b", ["-b", f["bed"], "-s"])


CASES = [("chr", []), ("chr", ["-x", "0", "-q", "20"]), ("chr", ["-a"]), ("w1000", []), ("w7", ["-q", "20"]), ("w150000", ["-x", "0"]), ("gff", []),
         ("bed4", ["-x", "0", "-q", "20"]), ("w1000", ["-readstats", "300"]), ("bed4", ["-frag", "-del"])]


@pytest.mark.parametrize("kind,margs", CASES, ids=["%s_%s" % (k, "_".join(m).replace("-", "") or "plain") for k, m in CASES])
def test_device_decode_equals_host_decode_and_the_model(corpus, kind, margs, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    f = corpus
    rows, w, mode, targs = table_of(kind, f)
    args = ["-i", f["path"], "-rowreads"] + targs + margs
    err, got = run(args, str(tmp_path / "dev"))
    if kind in ("gff", "bed4"):
        # -g / -b without an index fetch is the no-index span cursor, which stays on the host: its reader counts, no kernel is launched
        assert "row counts:" not in err and "k_row_counts" not in err, err[-800:]
    else:
        assert "device decode:" in err and "DECLINED" not in err and " 0 units handed back" in err, err[-800:]
        m = re.search(r"row counts: (\d+) records counted on the device in (\d+) bins", err)
        assert m and int(m.group(1)) == RR.started(f["lens"], f["model_recs"]), err[-800:]   # every record that starts somewhere, on the device
        k = re.search(r"k_row_counts: (\d+) launches, ([0-9.]+) ms", err)
        assert k and int(k.group(1)) >= 1 and float(k.group(2)) > 0, err[-800:]
    _, host = run(args + ["-X", "device_decode=0"], str(tmp_path / "host"))
    assert STAT in got and got[STAT] == host[STAT] and (host == got) is True                 # (the .gz bytes)
    x = int(margs[margs.index("-x") + 1]) if "-x" in margs else 1796
    q = int(margs[margs.index("-q") + 1]) if "-q" in margs else -1
    assert gzip.decompress(got[STAT]).decode() == RR.Model(f["lens"], rows, x, q, uniform_w=w).add_all(f["model_recs"]).text(f["names"], mode)
    err0, plain = run(["-i", f["path"]] + targs + margs, str(tmp_path / "plain"))
    assert plain and STAT not in plain and all(got[n] == plain[n] for n in plain)
    assert "row counts" not in err0 and "k_row_counts" not in err0
