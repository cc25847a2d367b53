"""The DEFLATE decoders (pandepth_amd/csrc/pd_inflate_wave.h, pd_inflate_core.h) on CONSTRUCTED hostile streams: well-formed
streams that expand as far as the format allows, overflow a counter or a scratch area, or are wrong in one chosen field
(tests/harness/deflate_builder.h, hostile_corpus.h), judged against zlib inside fenced memory on the CPU; then the same
members through the three GPU kernels, the device forms of the match copier's arithmetic against integers, and the
executable on a BAM whose middle member is damaged."""
import gzip
import os
import re
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(HERE, "harness")
sys.path.insert(0, ROOT)
from tools import synth  # noqa: E402

FAMILIES = ("maximal-expansion", "wrap-targets", "token-scratch", "header-abuse", "body-abuse", "many-tiny-blocks", "long-codes", "structured-mutation")
BODY_LEVEL = tuple(f for f in FAMILIES if f != "header-abuse")
# streams zlib inflates that the wave decoder hands to the host decoder (PD_W_HOST), per family: one in all — the literal/length code
# of a single one-bit code (hostile_corpus.h, gen_header)
DECLINED = {f: 0 for f in FAMILIES}
DECLINED["header-abuse"] = 1
# the sanitizer build of the corpus (697 cases x 4 decoder runs) on one core of the development machine took CORPUS_SECONDS
# (69 of them the one member of 70 001 empty blocks); the test allows ten times that
CORPUS_SECONDS = 89
CORPUS_TIMEOUT = 900


def _table(stdout):
    rows = {}
    for ln in stdout.splitlines():
        m = re.match(r"(\S+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", ln)
        if m and m.group(1) in FAMILIES:
            over = re.search(r", (\d+) over", ln)
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:]) + (int(over.group(1)),)    # cases, reached decode_body, zlib accepts, declined, sub-table areas exceeded
    return rows


def _check_report(stdout):
    rows = _table(stdout)
    assert sorted(rows) == sorted(FAMILIES), stdout[-2000:]
    for f in FAMILIES:
        cases, body, _zok, declined, over = rows[f]
        assert cases > 0, f
        if f in BODY_LEVEL:
            assert body > 0, "no case of %s reached decode_body" % f
        assert declined == DECLINED[f], "%s: %d streams zlib inflates were declined, expected %d" % (f, declined, DECLINED[f])
        assert over == 0, "%s: a complete code needed more sub-table entries than the tables hold" % f
    assert re.search(r"corpus: \d+ cases, 0 families without a case in decode_body, 0 rule violations", stdout), stdout[-2000:]
    m = re.search(r"wrap-targets: (\d+) merges .*?, (\d+) of them with a byte count above 17 bits", stdout)
    assert m and int(m.group(2)) > 0, "the merge path never ran with a count above 17 bits"


def test_hostile_corpus_on_host():
    """Every family of hostile_corpus.h through pdw::inflate_block<HostWave>, pdw::inflate_member<HostWave> and both modes of
    pdi::inflate_block, built with -fsanitize=address,undefined, every buffer between inaccessible pages.  The harness prints,
    per family, the cases, how many reached decode_body, how many zlib accepts, how many the wave decoder declined, the
    histogram of result codes and the largest sub-table areas needed; a broken rule names its case, a stray access stops the
    run with "FENCE: case ...".  Timing: CORPUS_SECONDS above."""
    exe = os.path.join(HARNESS, "inflate_wave_check_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    os.path.join(HARNESS, "inflate_wave_check.cpp"), "-lz", "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="handle_segv=0:allow_user_segv_handler=1:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "-c"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CORPUS_TIMEOUT, env=env)
    out, err = p.stdout.decode(), p.stderr.decode()
    print(out)
    assert p.returncode == 0, (out[-1500:], err[-1500:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-1500:]
    _check_report(out)


@pytest.fixture(scope="module")
def hostile_members(tmp_path_factory):
    """The corpus as BGZF members (those that fit one: 64 KiB) with its sidecar, written by the harness — a binary of this module's own,
    under the module's temporary directory — only after every case passed the host judge."""
    d = tmp_path_factory.mktemp("hostile")
    exe = str(d / "inflate_wave_check_hostile")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HARNESS, "inflate_wave_check.cpp"), "-lz", "-o", exe], check=True)
    members = str(d / "hostile.bgzf")
    p = subprocess.run([exe, "-c", "-w", members], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, (p.stdout.decode()[-1500:], p.stderr.decode()[-1500:])
    _check_report(p.stdout.decode())
    assert os.path.getsize(members) > 0
    return members


@pytest.mark.gpu
def test_hostile_members_on_gpu(hostile_members):
    """One member per pd_x_bgzf_inflate call, variants 0, 1 and 2: a member zlib inflates to ISIZE bytes must come back as zlib's
    bytes (the wave kernel may decline where the family is tagged, and refuses a wrong CRC-32 with -20), every other member must be
    refused BY THE DECODER (PD_X_BGZF_REFUSED; any other error stops the loop).  One child process, one time limit, it stops at
    the first failure.  pd_x_bgzf_inflate does not allocate through the guarded allocations, so the guard check after this test
    says nothing about it: out-of-bounds stores are what the host run inside its fences excludes (see hostile_gpu_run.py)."""
    q = subprocess.run([sys.executable, os.path.join(HARNESS, "hostile_gpu_run.py"), hostile_members, ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = q.stdout.decode()
    print(out[-800:])
    assert q.returncode == 0, (out[-800:], q.stderr.decode()[-800:])
    assert ", 0 failures" in out


@pytest.mark.gpu
def test_device_arithmetic_of_the_match_copier():
    """small_mod (v_rcp_f32 on the device), gather8 (v_perm_b32) and period_selector as the GPU executes them, against % and a
    byte loop: every off < 65536 with every d <= 300; every period 1 .. 7, every phase, 4096 words.  Expected: 0 disagreements."""
    subprocess.run(["make", "-C", HARNESS, "wave_arith_check"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(HARNESS, "wave_arith_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, (out, p.stderr.decode()[-400:])
    assert "small_mod: 19660800 pairs, 0 disagreements" in out and "gather8 / period_selector: 114688 cases, 0 disagreements" in out


# ---- the executable on a BAM whose middle member is damaged ------------------------------------------------------------------
def _members(d):
    o, out = 0, []
    while o + 18 <= len(d):
        bs = d[o + 16] + (d[o + 17] << 8) + 1
        out.append((o, bs))
        o += bs
    return out


def _bgzf_member(payload, crc, isize):
    bs = len(payload) + 26 - 1
    return bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, bs & 255, bs >> 8]) + payload + struct.pack("<II", crc, isize)


def _maximal_expansion_member(members_path):
    """The member of the maximal-expansion family with the most matches among those zlib does not take."""
    rows = [ln.rstrip("\n").split("\t") for ln in open(members_path + ".tsv") if not ln.startswith("#")]
    rows = [r for r in rows if r[6] == "maximal-expansion" and r[3] == "0"]
    r = max(rows, key=lambda r: int(re.search(r"(\d+) matches", r[7]).group(1)))
    assert int(re.search(r"(\d+) matches", r[7]).group(1)) >= 60000, r[7]
    with open(members_path, "rb") as f:
        f.seek(int(r[0]))
        return f.read(int(r[1]))


@pytest.fixture(scope="module")
def damaged_bams(tmp_path_factory, hostile_members):
    d = tmp_path_factory.mktemp("dmg")
    names, lens = synth.genome_c2(scale=0.001)
    rec = synth.gen_records_numpy(lens, 20000, seed=8)
    good = str(d / "good.bam")
    synth.write_bam(good, names, lens, rec, procs=1, payload=True, level=6)
    data = open(good, "rb").read()
    ms = _members(data)
    assert len(ms) > 20
    o, bs = ms[len(ms) // 2]
    m = data[o:o + bs]
    crc, isize = struct.unpack("<II", m[-8:])
    # a final fixed block: the literal 'q', then length symbol 286 (code 11000110), which no stream may use
    bits = [1, 1, 0] + [int(c) for c in format(0x30 + ord("q"), "08b")] + [1, 1, 0, 0, 0, 1, 1, 0] + [0] * 12
    by = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        by[i >> 3] |= b << (i & 7)
    new = {"wrong CRC": m[:-8] + bytes([m[-8] ^ 0x10]) + m[-7:],
           "invalid code": _bgzf_member(bytes(by), crc, isize),
           "maximal expansion": _maximal_expansion_member(hostile_members)}
    out = {"good": good}
    for k, v in new.items():
        p = str(d / (k.replace(" ", "_") + ".bam"))
        open(p, "wb").write(data[:o] + v + data[o + bs:])
        out[k] = p
    return out


def _cli_refuses(exe, damaged_bams, tmp_path):
    good = os.path.join(str(tmp_path), "good")
    p = subprocess.run([exe, "-i", damaged_bams["good"], "-o", good], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    want = gzip.open(good + ".chr.stat.gz").read()
    assert want.startswith(b"#Chr") and want.count(b"\n") > 2
    for kind in ("wrong CRC", "invalid code", "maximal expansion"):
        prefix = os.path.join(str(tmp_path), kind.replace(" ", "_"))
        p = subprocess.run([exe, "-i", damaged_bams[kind], "-o", prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        err = p.stderr.decode()
        assert p.returncode not in (0, None) and p.returncode > 0, (kind, p.returncode, err[-400:])      # (an exit status, not a signal)
        assert "Error" in err, (kind, err[-400:])
        # no table at all — not a partial one, and not an empty gzip file a reader could take for a result
        left = [f for f in os.listdir(str(tmp_path)) if f.startswith(os.path.basename(prefix) + ".")]
        assert left == [], (kind, left)


def test_cli_refuses_a_damaged_member_on_the_host_decoder(damaged_bams, tmp_path):
    """The product's host code on the CPU oracle engine (tests/harness/pandepth_oracle_cli: the host BGZF reader inflates) on a BAM whose
    middle member has a wrong CRC-32, an invalid code, or is a maximal-expansion member: a non-zero exit status, a message, no table.
    (The reference binary, where oracle/_ref/pandepth_ref is built: on each of the three files it prints "Input data read done", exits
    with status 0 and leaves a chr.stat.gz computed from the records in front of the damaged member — a table that reads as complete.)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", HARNESS, "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    _cli_refuses(os.path.join(HARNESS, "pandepth_oracle_cli"), damaged_bams, tmp_path)


@pytest.mark.gpu
def test_cli_refuses_a_damaged_member_on_the_gpu_decoder(damaged_bams, tmp_path):
    """The executable of the GPU build (members inflated by the wave kernel on the device) on the same three files: a non-zero exit
    status, a message, no table, inside the time limit.  (The reference binary on these files: see the host test's docstring.)"""
    _cli_refuses(os.path.join(ROOT, "pandepth_amd", "pandepth"), damaged_bams, tmp_path)
