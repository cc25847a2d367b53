"""The fast chunk of the narrow cover sweep (pandepth_amd/csrc/pd_cover_rule.h: the packed step nar_pair_steps, the lane summary (T, Mrel, lens),
the acceptance test chunk_fast_entry / chunk_fast_lane_ok / chunk_fast_ok, and chunk_fast, the same test lane after lane) against the rule run by run on
the CPU: tests/harness/cover_fast_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  An accepted chunk must leave exactly the
state seg_sweep_nar has behind the same runs (the last run's begin, the largest end, the sum, no new gap); a chunk that holds a gap, a begin < 0 or an
end > tile must never be accepted; a refused chunk must have changed nothing.  The program prints how many chunks took each outcome and fails when one
is hardly represented."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_fast_chunk_against_the_rule_run_by_run(tmp_path):
    exe = os.path.join(str(tmp_path), "cover_fast_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "cover_fast_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"full chunks checked: (\d+), accepted: (\d+), refused with a gap: (\d+), with a begin < 0: (\d+), with an end > tile: (\d+)", out)
    assert m and int(m.group(2)) >= 1000 and int(m.group(3)) >= 300 and int(m.group(4)) >= 100 and int(m.group(5)) >= 20
    assert "cover_fast_check: ok" in out
