"""`pandepth -del` on the MI355X: the executable (device decode: the `-del` kernels of the record walk; CRAM and PAF through the host
walkers) against the product's host code on the oracle-backed engine run with `-X device_decode=0` (the harness's emulated decode
session does not know the flag), byte for byte; and for the BAMs the executable's own host decode against its device decode."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
ORACLE_CLI = os.path.join(HERE, "harness", "pandepth_oracle_cli")

INPUTS = [("f1", "f1.bam", ["-g", "f1.gff"]), ("f5", "c.bam", ["-b", "c.bed4"]), ("f7", "m.bam", ["-b", "m.bed4"]), ("f7", "m.cram", ["-g", "m.gff"]),
          ("f6", "p.paf", ["-g", "p.gff"])]
MODES = [("chr", []), ("w1000", ["-w", "1000"]), ("w100_a", ["-w", "100", "-a"]), ("regions", None)]


@pytest.fixture(scope="module")
def oracle_cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return ORACLE_CLI


def run(exe, fixture, args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([exe] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(HERE, "golden", fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, PANDEPTH_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p.stderr.decode(), {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


@pytest.mark.parametrize("mode,margs", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("fixture,inp,region", INPUTS, ids=[i[1] for i in INPUTS])
def test_executable_equals_oracle_cli(oracle_cli, fixture, inp, region, mode, margs, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    args = ["-i", inp, "-del"] + (region if margs is None else margs)
    _, want = run(oracle_cli, fixture, args + ["-X", "device_decode=0"], str(tmp_path / "oracle"))
    err, got = run(CLI, fixture, args, str(tmp_path / "dev"))
    assert want and (got == want) is True, (sorted(got), sorted(want))
    _, plain = run(CLI, fixture, [a for a in args if a != "-del"], str(tmp_path / "plain"))
    assert (plain != got) is True                                     # (every one of these inputs holds deletions)
    if inp.endswith(".bam"):
        assert "device decode:" in err and "DECLINED" not in err, err[-800:]
        _, host = run(CLI, fixture, args + ["-X", "device_decode=0"], str(tmp_path / "host"))
        assert (host == got) is True
