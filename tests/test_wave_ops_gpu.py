"""The wave primitives the kernels execute — pdw::DevWave (pd_inflate_wave.h: DPP row shifts and broadcasts, readlane, mbcnt,
Hillis-Steele scans) and pdz::DevWaveZ (pd_lz77_devwave.h) — against the 64-lanes-in-a-loop forms every CPU test of the inflate,
record walk, chain and LZ77 code runs instead (pdw::HostWave, pdz::HostWave): tests/harness/wave_ops_gpu_check applies every
primitive to fixed vectors (zeros, all ones, one value on every row and half-wave seam, monotone vectors, 64-bit values equal
below bit 32, every head layout of the segmented scan) and a few hundred seeded random ones, one wave per case, and compares every
lane bit for bit."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
H = os.path.join(HERE, "harness")


@pytest.mark.gpu
def test_device_wave_primitives_equal_the_host_emulation():
    subprocess.run(["make", "-C", H, "wave_ops_gpu_check"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(H, "wave_ops_gpu_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    m = re.search(r"(\d+) cases, 0 differ", p.stdout)
    assert p.returncode == 0 and m, p.stdout[-1500:] + p.stderr[-1500:]
    assert int(m.group(1)) >= 500
