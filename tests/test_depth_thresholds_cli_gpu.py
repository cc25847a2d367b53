"""-thresholds SPEC on the MI355X: the `pandepth` executable on the golden fixtures, one case per mode plus a `#.list` and a PAF.
The file counted on the device (pd_window_thresholds / pd_depth_thresholds) is, after gunzip, the file the host fallback writes
(-X thresholds_device=0) and the rows numpy counts on the CPU oracle's depth; the main tables are those of the run without the
option; and the file is the same behind the device-resident window table."""
import gzip
import os
import subprocess

import pytest

from test_depth_thresholds_cli import HERE, IDS, expected, main_suffix
from test_depth_quantiles_cli import table_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")
ORACLE_CLI = os.path.join(HERE, "harness", "pandepth_oracle_cli")
SPEC = "0,1,5,10,300"

CASES = [
    ("f1", ["-i", "f1.bam"]),                                # whole contigs
    ("f1", ["-i", "f1.bam", "-w", "100"]),                   # windows below 150
    ("f1", ["-i", "f1.bam", "-w", "200", "-d", "3"]),        # windows from 150
    ("f1", ["-i", "f1.bam", "-g", "f1.gff"]),
    ("f1", ["-i", "f1.bam", "-g", "f1.gtf"]),
    ("f1", ["-i", "f1.bam", "-b", "f1.bed3"]),
    ("f1", ["-i", "f1.bam", "-b", "q_overlap.bed4"]),
    ("f1", ["-i", "f1_3.list", "-b", "f1.bed4"]),
    ("f6", ["-i", "p.paf", "-w", "100"]),
    ("f6", ["-i", "p.list", "-g", "p.gff"]),
]


def run(cli, fixture, args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([cli] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=os.path.join(HERE, "golden", fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, PANDEPTH_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return p, {f: gzip.decompress(open(os.path.join(out_dir, f), "rb").read()) for f in os.listdir(out_dir)}


@pytest.mark.parametrize("fixture,args", CASES, ids=IDS)
def test_device_file_equals_host_file_and_oracle(fixture, args, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    _, plain = run(CLI, fixture, args, str(tmp_path / "plain"))
    _, dev = run(CLI, fixture, args + ["-thresholds", SPEC], str(tmp_path / "dev"))
    _, host = run(CLI, fixture, args + ["-thresholds", SPEC, "-X", "thresholds_device=0"], str(tmp_path / "host"))
    assert sorted(dev) == sorted(list(plain) + ["o.thresholds.stat.gz"])
    assert {f: dev[f] for f in plain} == plain                                  # the tables do not change
    assert dev["o.thresholds.stat.gz"] == host["o.thresholds.stat.gz"]
    head, rows = table_rows(tmp_path / "dev", main_suffix(tmp_path / "dev"))
    thead, trows = table_rows(tmp_path / "dev", "thresholds.stat.gz")
    thr = [int(x) for x in SPEC.split(",")]
    exp, _ = expected(fixture, args, thr, head, rows)
    assert exp and trows == exp
    assert thead[-len(thr) - 1:] == ["Cells"] + ["GE%d" % x for x in thr]


def test_behind_the_resident_table(tmp_path):
    """`-w 100 -X table_resident_min=1`: f1's small table takes the exit the large tables take, the sample stays on the device
    and the extra goes through need_scan()"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    args = ["-i", "f1.bam", "-w", "100"]
    p, gpu = run(CLI, "f1", args + ["-X", "table_resident_min=1", "-thresholds", SPEC], str(tmp_path / "gpu"))
    assert b"rows, parse and checksums on the device" in p.stderr, "the table did not take the device-resident exit"
    _, cpu = run(ORACLE_CLI, "f1", args + ["-thresholds", SPEC], str(tmp_path / "cpu"))
    assert sorted(gpu) == sorted(cpu) == ["o.thresholds.stat.gz", "o.win.stat.gz"]
    assert gpu["o.thresholds.stat.gz"] and gpu["o.thresholds.stat.gz"] == cpu["o.thresholds.stat.gz"]
