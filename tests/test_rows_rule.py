"""The arithmetic of the row statistics (pandepth_amd/csrc/pd_rows_rule.h: the segment clip to a contig's length and to its slot, the cutter of
16384-cell pieces, the piece feed and its flushes, the end of a batch of rows, the launch shape of a row, the group shifts, rows per group and rows
per batch, the cell span of a window) at its edges, with every expected number written out: tests/harness/rows_rule_check.cpp, a stand-alone
program built with -fsanitize=address,undefined.  The product's limits (2^20 rows and 2^21 segments a batch, a flush every 2^21 pieces) are beyond
what a GPU test can reach; the program runs the same code with limits of a handful."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_rows_rule_at_its_edges(tmp_path):
    exe = os.path.join(str(tmp_path), "rows_rule_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "rows_rule_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"rows_rule_check: (\d+) checks, (\d+) failed", out)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0          # (the program counts its checks: a run that checked nothing does not pass)
    assert "rows_rule_check: ok" in out
