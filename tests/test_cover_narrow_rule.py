"""The narrow plane of a compact sample's sorted stream (pandepth_amd/csrc/pd_cover_rule.h: two bytes per run, begins rebuilt from the differences
of their low bytes, the end check that says whether the rebuild was exact) against the lo words and a per-cell union on the CPU:
tests/harness/cover_narrow_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  The end check must pass exactly when every
consecutive difference of begins is below 256; where it passes, begins, sum, carry and "covered" must equal the sweep of the lo words; a tile must
never be reported covered when a cell is not.  The program prints how many tiles took each outcome and fails when one is hardly represented."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_narrow_rebuild_against_the_lo_words_and_the_per_cell_union(tmp_path):
    exe = os.path.join(str(tmp_path), "cover_narrow_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "cover_narrow_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"tiles x offsets checked: (\d+), end check passed: (\d+), failed: (\d+), settled: (\d+)", out)
    assert m and int(m.group(2)) >= 1000 and int(m.group(3)) >= 500 and int(m.group(4)) >= 500
    assert "cover_narrow_check: ok" in out
