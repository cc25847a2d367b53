"""The batch cutter of tests/bam_craft.py (cut_batches: what tests/test_gpu_decode_session.py feeds the decode session) on the CPU:
every record of a file is owned by exactly one unit, and a batch's tables describe its own bytes — the members inflate, from in_off,
to the file's inflated bytes at the batch's base, and every unit's records lie inside what the unit may read.  No GPU."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bam_craft as B

FILES = ["alone", "packed", "layout", "few", "unsorted"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return B.build_corpus(tmp_path_factory.mktemp("batches"))


def cuttings(f, name):
    return B.session_cuts(f, name)               # the very batches tests/test_gpu_decode_session.py submits


@pytest.mark.parametrize("name", FILES)
def test_every_record_is_owned_by_exactly_one_unit(corpus, name):
    f = corpus[name]
    for label, batches in cuttings(f, name).items():
        if label in ("1", "3", "16"):
            assert len(batches) == int(label), (label, len(batches))
        n = B.owners(f, batches)
        assert n.size == len(f["offs"]) and (n == 1).all(), (name, label, np.flatnonzero(n != 1)[:8])
        assert [b["order"] for b in batches] == list(range(len(batches)))


@pytest.mark.parametrize("name", FILES)
def test_a_batch_describes_its_own_bytes(corpus, name):
    f = corpus[name]
    offs = np.asarray(f["offs"], dtype=np.int64)
    ends = np.append(offs[1:], len(f["inf"]))
    shared = 0
    for label, batches in cuttings(f, name).items():
        for k, b in enumerate(batches):
            at = 0
            for in_off, out_off, in_len, out_len in b["blocks"]:
                assert out_off == at and b["data"][in_off - 18:in_off - 14] == b"\x1f\x8b\x08\x04"
                piece = zlib.decompress(b["data"][in_off:in_off + in_len], -15)
                assert len(piece) == out_len and piece == f["inf"][b["base"] + out_off:b["base"] + out_off + out_len]
                at += out_len
            assert at == b["inflated"] and b["blocks"][0][1] == 0
            for start, stop, avail, fb, nb, flags in b["units"]:
                lo, hi = b["blocks"][fb], b["blocks"][fb + nb - 1]
                assert lo[1] <= start < lo[1] + lo[3] and avail == hi[1] + hi[3]
                mine = (offs >= start + b["base"]) & (offs < stop + b["base"])
                assert mine.any() and ends[mine].max() <= avail + b["base"]
                assert ends[mine].max() > hi[1] + b["base"]                 # (no member behind the last one the unit needs)
                if not flags & 1:
                    assert start + b["base"] == offs[mine][0]
                else:
                    assert label == "guess" and k > 0 and start == 0 and len(b["units"]) == 1
            if k and batches[k - 1]["members"][1] >= b["members"][0]:
                shared += 1
    assert shared > 0                                                       # neighbouring batches share the members their edge records straddle


def guess_chain_check():
    """builds tests/harness/guess_chain_check (the host compiler and zlib, like the other harness programs) -> its path"""
    import shutil
    here = os.path.dirname(os.path.abspath(__file__))
    assert shutil.which("g++"), "no host C++ compiler (g++) to build tests/harness/guess_chain_check.cpp with"
    exe = os.path.join(here, "harness", "guess_chain_check")
    p = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(here, "harness", "guess_chain_check.cpp"), "-lz", "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "tests/harness/guess_chain_check.cpp does not build (it needs zlib's headers):\n" + p.stdout.decode()[-1500:]
    return exe


def run_guess_units(exe, f, units):
    """-> [(flags, first_start, records)] of units (start, stop, avail) in file coordinates"""
    out = subprocess.run([exe, f["path"]] + [str(x) for u in units for x in u[:3]], check=True, stdout=subprocess.PIPE).stdout.decode()
    got = [tuple(int(x) for x in m) for m in re.findall(r"flags (\d+), first_start (-?\d+), records (\d+)", out)]
    assert len(got) == len(units)
    return got


@pytest.mark.parametrize("name", ["alone", "packed", "layout"])
def test_guessed_units_follow_their_chain_on_the_host(corpus, name):
    """The no-index batches through the walk with its lanes emulated on the host and pdb2::check_chain (tests/harness/
    guess_chain_check.cpp): every unit finds the first record at or after its member start and counts its own records, no flag.  In
    `alone` and `packed` a unit begins inside a record longer than a segment, so its first segment holds no record start: the chain
    check used to hold the next segment to a chain end of 0, walked it again from the batch's first byte and left the unit to the host."""
    exe = guess_chain_check()
    f = corpus[name]
    offs = np.asarray(f["offs"], dtype=np.int64)
    _, seg, _ = B.walk_geometry()
    units = [b["units_file"][0] for b in B.cut_batches(f, [len(f["inf"]) * k // 8 for k in range(1, 8)], 1, guess=True)[1:]]
    if name != "layout":
        assert any(offs[np.searchsorted(offs, u[0])] - u[0] > seg for u in units)          # an empty first segment
    got = run_guess_units(exe, f, units)
    want = [(0, int(offs[np.searchsorted(offs, u[0])]), int(((offs >= u[0]) & (offs < u[1])).sum())) for u in units]
    assert got == want


def test_decoy_behind_an_empty_first_segment(tmp_path):
    """A guessed unit that begins inside a record of more than two segments: its first segment holds no record start, so the second
    segment's own guess stands — and there a Z tag passes for a record header.  Such a unit may be left to the host (the decoy's
    block size runs past the unit's bytes) but is never accepted from the decoy; a unit that begins behind the decoy finds the
    true boundary."""
    _, seg, _ = B.walk_geometry()
    f, rec, decoy = B.long_decoy_file(tmp_path, seg)
    offs = f["offs"]
    true = offs[21]
    before = [rec + d for d in (1, 4096, seg // 2 - 1)]                    # more than a segment before the decoy
    behind = [decoy + 1, decoy + 37, decoy + seg // 2]
    assert all(decoy - s > seg for s in before) and all(s < true for s in behind)
    units = [B.unit_at(f, s, offs[60], 1) for s in before + behind]
    got = run_guess_units(guess_chain_check(), f, units)
    for s, (flags, first, n_rec) in zip(before, got):
        assert flags != 0 or (first, n_rec) == (true, 60 - 21), (s, flags, first)
        assert first != decoy or flags != 0
    for s, (flags, first, n_rec) in zip(behind, got[len(before):]):
        assert (flags, first, n_rec) == (0, true, 60 - 21), (s, flags, first)
