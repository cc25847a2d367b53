"""-quantile on the MI355X: the `pandepth` binary on every golden case with `-quantile 5,50,95` added.  The existing outputs,
stdout and exit code stay exactly as the reference's (so: byte-identical to a run without the option); one extra file,
o.quantile.stat.gz, appears, and its text equals what the host fallback (the same host code on the CPU oracle engine,
tests/harness/pandepth_oracle_cli, which selects with std::nth_element) writes for the same command line."""
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
SPEC = "5,50,95"


@pytest.fixture(scope="module")
def oracle_cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return ORACLE_CLI


def run(cli, case, out_dir, extra):
    d = os.path.join(HERE, "golden", case["fixture"])
    os.makedirs(out_dir, exist_ok=True)
    args = [cli] + case["args"] + extra + ["-o", os.path.join(out_dir, "o")]
    if "-t" not in case["args"]:
        args += ["-t", "4"]
    return subprocess.run(args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.mark.parametrize("case", MANIFEST, ids=lambda e: "%s-%s" % (e["fixture"], e["name"]))
def test_quantile_on_every_golden_case(case, oracle_cli, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    p = run(CLI, case, str(tmp_path / "gpu"), ["-quantile", SPEC])
    assert p.returncode == case["returncode"], p.stderr.decode()[-500:]
    assert p.stdout.decode() == case["stdout"]
    for suffix, meta in case["outputs"].items():
        gz = (tmp_path / "gpu" / ("o." + suffix)).read_bytes()
        assert hashlib.sha256(gz).hexdigest() == meta["gz_sha256"], suffix
    files = sorted(os.listdir(tmp_path / "gpu"))
    listed = sorted("o." + s for s in case["outputs"])
    if not case["outputs"]:                                   # a run that writes no table writes no percentiles either
        assert files == [], files
        return
    assert files == sorted(listed + ["o.quantile.stat.gz"]), files
    q = run(oracle_cli, case, str(tmp_path / "cpu"), ["-quantile", SPEC])
    assert q.returncode == case["returncode"], q.stderr.decode()[-500:]
    got = gzip.decompress((tmp_path / "gpu" / "o.quantile.stat.gz").read_bytes()).decode()
    exp = gzip.decompress((tmp_path / "cpu" / "o.quantile.stat.gz").read_bytes()).decode()
    assert got.startswith("#Chr\t") and got.splitlines()[0].endswith("\tCells\tQ5\tQ50\tQ95")
    assert got == exp


def test_overlapping_and_overhanging_rows(oracle_cli, tmp_path):
    """the hand-written q_overlap.bed4 (an id whose entries overlap, a region over the contig's end, one wholly past it), through
    every launch shape of the kernels: the same text as the host fallback's"""
    case = {"fixture": "f1", "args": ["-i", "f1.bam", "-b", "q_overlap.bed4"]}
    q = run(oracle_cli, case, str(tmp_path / "cpu"), ["-quantile", "0,50,100"])
    assert q.returncode == 0
    exp = gzip.decompress((tmp_path / "cpu" / "o.quantile.stat.gz").read_bytes()).decode()
    assert "\tNA\tNA\tNA\n" in exp
    for k, tune in enumerate(("quantile_wave_max=2048", "quantile_wave_max=0,quantile_split_cells=4294967295", "quantile_wave_max=0,quantile_split_cells=0")):
        p = run(CLI, case, str(tmp_path / ("gpu%d" % k)), ["-quantile", "0,50,100", "-X", tune])
        assert p.returncode == 0, p.stderr.decode()[-500:]
        assert gzip.decompress((tmp_path / ("gpu%d" % k) / "o.quantile.stat.gz").read_bytes()).decode() == exp, tune
