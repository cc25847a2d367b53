"""-levels on the MI355X: the `pandepth` binary on every golden case with `-levels 0,1,5,15` added, and on every third case
(by index) with `-levels exact`.  The existing outputs, stdout and exit code stay exactly as the reference's; one extra file,
o.levels.bed.gz, appears, and its text equals what the host fallback (the same host code on the CPU oracle engine,
tests/harness/pandepth_oracle_cli) writes for the same command line.  One case is repeated in chunks of 1000 cells."""
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
RUNS = [(case, "0,1,5,15") for case in MANIFEST] + [(case, "exact") for case in MANIFEST[::3]]


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


def levels_text(d):
    return gzip.decompress((d / "o.levels.bed.gz").read_bytes()).decode()


@pytest.mark.parametrize("case,spec", RUNS, ids=lambda x: "%s-%s" % (x["fixture"], x["name"]) if isinstance(x, dict) else x.replace(",", "_"))
def test_levels_on_golden_cases(case, spec, oracle_cli, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    p = run(CLI, case, str(tmp_path / "gpu"), ["-levels", spec])
    assert p.returncode == case["returncode"], p.stderr.decode()[-500:]
    assert p.stdout.decode() == case["stdout"]
    for suffix, meta in case["outputs"].items():
        gz = (tmp_path / "gpu" / ("o." + suffix)).read_bytes()
        assert hashlib.sha256(gz).hexdigest() == meta["gz_sha256"], suffix
    files = sorted(os.listdir(tmp_path / "gpu"))
    listed = sorted("o." + s for s in case["outputs"])
    if not case["outputs"]:                                   # a run that writes no table writes no levels file either
        assert files == [], files
        return
    assert files == sorted(listed + ["o.levels.bed.gz"]), files
    q = run(oracle_cli, case, str(tmp_path / "cpu"), ["-levels", spec])
    assert q.returncode == case["returncode"], q.stderr.decode()[-500:]
    got, exp = levels_text(tmp_path / "gpu"), levels_text(tmp_path / "cpu")
    assert got == exp
    for ln in got.splitlines()[:50]:
        c = ln.split("\t")
        assert len(c) == 4 and int(c[1]) < int(c[2]) and ((":" in c[3]) == (spec != "exact"))


def test_chunked_on_the_gpu_path_gives_the_same_text(tmp_path):
    case = next(c for c in MANIFEST if c["fixture"] == "f1" and c["args"] == ["-i", "f1.bam"])
    for spec in ("0,1,5,15", "exact"):
        p = run(CLI, case, str(tmp_path / ("whole" + spec[0])), ["-levels", spec])
        q = run(CLI, case, str(tmp_path / ("chunk" + spec[0])), ["-levels", spec, "-X", "levels_chunk=1000"])
        assert p.returncode == 0 and q.returncode == 0, (p.stderr + q.stderr).decode()[-500:]
        whole = levels_text(tmp_path / ("whole" + spec[0]))
        assert whole and levels_text(tmp_path / ("chunk" + spec[0])) == whole
