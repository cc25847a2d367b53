"""The rule by which k_direct_c8 settles a tile from its runs alone (pandepth_amd/csrc/pd_cover_rule.h: one forward sweep with a running
maximum, cut into up to four segments, in the kernel's 16-bit arithmetic) against a per-cell union on the CPU:
tests/harness/cover_rule_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  "Covered" must never be said of a tile
with an uncovered cell; the clipped-length sum and the carry-in must always equal the per-cell figures; of the covered 50x-like random
tiles at most 1 in 100 may be declined (the program prints the share), so that a rule that declines everything does not pass."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_cover_rule_against_the_per_cell_union(tmp_path):
    exe = os.path.join(str(tmp_path), "cover_rule_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "cover_rule_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"covered 50x-like tiles: (\d+), declined by the four quarters: (\d+), share ([0-9.]+)", out)
    assert m and int(m.group(1)) >= 290
    assert int(m.group(2)) * 100 <= int(m.group(1))
    assert "cover_rule_check: ok" in out
