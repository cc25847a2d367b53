"""The software pipeline of k_direct_c8's cover sweeps (pandepth_amd/csrc/pd_cover_rule.h: pdcover::sweep3, three register buffers in turn: a loop of whole
rotations with ONE exit, and a tail without loads) on the CPU: tests/harness/sweep3_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  For every number of chunks 1 .. 10, a stop behind every chunk position and none: work is
called for exactly the chunks 0 .. min(nq - 1, the stop's chunk) in order, each with the buffer its load filled and nothing loaded over it in between, no
load's index exceeds nq + 3, and the loop the sweeps had before (kept in the program) makes the same work calls."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "harness")


def test_sweep3_works_on_every_chunk_in_order_from_the_buffer_its_load_filled(tmp_path):
    exe = os.path.join(str(tmp_path), "sweep3_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "sweep3_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out + p.stderr.decode()[-3000:]
    m = re.search(r"sweeps (\d+), work calls (\d+), loads (\d+), of them behind the last chunk (\d+)", out)
    # 2 buffer sizes x (sweep3, the reference) x sum over nq = 1 .. 10 of (nq + 2) stops
    assert m and int(m.group(1)) == 2 * 2 * sum(nq + 2 for nq in range(1, 11)) and int(m.group(2)) > 0
    assert "sweep3_check: ok" in out
