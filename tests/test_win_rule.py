"""The arithmetic of a window call (pandepth_amd/csrc/pd_win_rule.h: the wrap mask, the layout of the result buffer and the 1 MiB boundary of
the page-locked read-back, the turn of the direct call's two sets of status words over a sequence of calls, the grids of the tile passes, the form
of k_direct_c8 a call launches) at its edges, with every expected number written out: tests/harness/win_rule_check.cpp, a stand-alone program
built with -fsanitize=address,undefined.  The sequence of calls is that of tests/test_gpu_direct_step.py's
test_a_call_of_another_kind_between_two_wide_ones, visible here without a GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_win_rule_at_its_edges(tmp_path):
    exe = os.path.join(str(tmp_path), "win_rule_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "win_rule_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"win_rule_check: (\d+) checks, (\d+) failed", out)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0          # (the program counts its checks: a run that checked nothing does not pass)
    assert "win_rule_check: ok" in out
