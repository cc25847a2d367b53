"""-dist, -levels and -quantile behind the device-resident window table on the MI355X: `-w 100` with
`-X table_resident_min=1` makes f1's small table take the exit the large tables take (rows formatted, parsed and check-summed
on the device).  The table stays byte-identical to the reference's, and the three extra files hold the text the host fallbacks
(the same host code on the CPU oracle engine, tests/harness/pandepth_oracle_cli) write for the command line without the -X."""
import gzip
import hashlib
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
ORACLE_CLI = os.path.join(HERE, "harness", "pandepth_oracle_cli")
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
ARGS = ["-i", "f1.bam", "-w", "100"]
EXTRAS = ["-dist", "8", "-levels", "exact", "-quantile", "5,50,95"]
EXTRA_FILES = ["o.dist.stat.gz", "o.levels.bed.gz", "o.quantile.stat.gz"]


def run(cli, out_dir, extra):
    os.makedirs(out_dir, exist_ok=True)
    return subprocess.run([cli] + ARGS + extra + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(HERE, "golden", "f1"),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, PANDEPTH_TIMING="1"))


def test_extras_behind_the_resident_table(tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    case = next(c for c in MANIFEST if c["fixture"] == "f1" and c["args"] == ARGS)
    p = run(CLI, str(tmp_path / "gpu"), ["-X", "table_resident_min=1"] + EXTRAS)
    assert p.returncode == case["returncode"], p.stderr.decode()[-500:]
    assert p.stdout.decode() == case["stdout"]
    assert b"rows, parse and checksums on the device" in p.stderr, "the table did not take the device-resident exit"
    assert sorted(os.listdir(tmp_path / "gpu")) == sorted(EXTRA_FILES + ["o.win.stat.gz"])
    gz = (tmp_path / "gpu" / "o.win.stat.gz").read_bytes()
    assert hashlib.sha256(gz).hexdigest() == case["outputs"]["win.stat.gz"]["gz_sha256"]
    q = run(ORACLE_CLI, str(tmp_path / "cpu"), EXTRAS)
    assert q.returncode == case["returncode"], q.stderr.decode()[-500:]
    for f in EXTRA_FILES:
        got = gzip.decompress((tmp_path / "gpu" / f).read_bytes()).decode()
        assert got and got == gzip.decompress((tmp_path / "cpu" / f).read_bytes()).decode(), f
