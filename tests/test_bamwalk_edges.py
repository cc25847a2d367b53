"""The reference the GPU tests of the record walk compare with (tests/bam_craft.py: a numpy walk written from the SAM specification)
against two independent CPU implementations, on the whole crafted corpus — every operation count around the wave-walked CIGARs'
threshold and step, first runs behind clips and gaps, CIGARs in the CG tag, records on every lane, segment and unit edge:
  * the oracle's per-base increments (oracle/pd_oracle.c: pdo_walk_records), fed the way test_gpu_bgzf.expected_depth feeds them;
  * the product's walk with its 64 lanes emulated on the host against the product's sequential reader (tests/harness/bamwalk_check),
    whose run counts must also be the reference's.
No GPU here; tests/test_gpu_bamwalk_edges.py runs the same files through the device."""
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as B
import pd_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = os.path.join(HERE, "harness")
FILES = ["alone", "packed", "layout", "few", "unsorted"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return B.build_corpus(tmp_path_factory.mktemp("edges"))      # (asserts that every named case is present)


@pytest.fixture(scope="module")
def walker():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(H, "bamwalk_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(H, "bamwalk_check.cpp"),
                    os.path.join(ROOT, "pandepth_amd", "libpandepth_host.a"), "-lz", "-ldl", "-o", exe], check=True)
    return exe


def test_writer_and_parser_agree_with_the_oracles_reader(corpus):
    """what the writer wrote is what two readers read: the record's own fields and CIGAR (the placeholder where the CIGAR is in CG)"""
    for name in FILES:
        f = corpus[name]
        r = O.read_alignments(f["path"])
        assert list(r.lens) == B.LENS and len(r.tid) == len(f["recs"])
        for k, mine in enumerate(f["recs"]):
            assert (r.tid[k], r.pos[k], r.flag[k], r.mapq[k]) == (mine["tid"], mine["pos"], mine["flag"], mine["mapq"])
            assert np.array_equal(np.array(r.cigars[k], dtype=np.uint32), mine["cigar"]), (name, k)
        blocks, inf = _scan(f["data"])
        assert blocks == f["blocks"] and inf == f["inf"]


def _scan(data):
    import struct
    import zlib
    blocks, o, uo, parts = [], 0, 0, []
    while o + 18 <= len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bs = struct.unpack_from("<H", data, o + 16)[0] + 1
        isize = struct.unpack_from("<I", data, o + bs - 4)[0]
        blocks.append((o + 12 + xlen, uo, bs - 12 - xlen - 8, isize))
        parts.append(zlib.decompress(data[o + 12 + xlen:o + bs - 8], -15))
        uo += isize; o += bs
    return blocks, b"".join(parts)


@pytest.mark.parametrize("flag_mask,min_mapq", B.FILTERS)
@pytest.mark.parametrize("name", FILES)
def test_reference_equals_oracle_walk(corpus, name, flag_mask, min_mapq):
    f = corpus[name]
    lens = f["lens"]
    dep, n_kept, _ = B.reference_depth(lens, f["recs"], flag_mask, min_mapq)
    sel = [r for r in f["recs"] if r["tid"] >= 0 and lens[r["tid"]] >= 2]
    tid = np.array([r["tid"] for r in sel], dtype=np.int32)
    pos = np.array([r["pos"] for r in sel], dtype=np.int32)
    flag = np.array([r["flag"] for r in sel], dtype=np.uint16)
    mapq = np.array([r["mapq"] for r in sel], dtype=np.uint8)
    cigs = [B.real_cigar(r) for r in sel]
    coff = np.zeros(len(sel) + 1, dtype=np.int64)
    coff[1:] = np.cumsum([c.size for c in cigs])
    cig = np.ascontiguousarray(np.concatenate(cigs + [np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
    off = O.contig_offsets(lens)
    d = np.zeros(int(off[-1]), dtype=np.uint32)
    got = O.lib().pdo_walk_records(len(tid), O._p(tid), O._p(pos), O._p(flag), O._p(mapq), O._p(coff), O._p(cig), flag_mask, min_mapq, O._p(d), O._p(off))
    assert got == n_kept
    for t, ln in enumerate(lens):
        if ln >= 2:
            assert np.array_equal(dep[t], d[off[t]:off[t] + ln]), t
    assert sum(int(x.sum(dtype=np.uint64)) for x in dep if x is not None) > 0


@pytest.mark.parametrize("opts", [[], ["-x", "0", "-q", "20"], ["-near", "1024"], ["-seg", "4", "-x", "0"], ["-seg", "256"]], ids=lambda o: "_".join(o) or "default")
def test_host_emulated_walk_on_the_crafted_files(corpus, walker, opts):
    """the product's walk (HostWave) = the product's sequential reader on every crafted file, and both count the reference's runs"""
    flag_mask = int(opts[opts.index("-x") + 1]) if "-x" in opts else 1796
    min_mapq = int(opts[opts.index("-q") + 1]) if "-q" in opts else 0
    p = subprocess.run([walker] + opts + [corpus[n]["path"] for n in FILES], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0, (out[-1500:], p.stderr.decode()[-400:])
    assert "DIFFERENT" not in out and out.count("identical") == 2 * len(FILES)
    for name in FILES:
        f = corpus[name]
        line = next(l for l in out.splitlines() if l.startswith(f["path"] + ":"))
        m = re.search(r": (\d+) records, .*first runs (\d+) \(expected \d+\) identical, other runs (\d+) \(expected \d+\) identical, flags 0,", line)
        assert m, line
        keep = [r for r in f["recs"] if B.kept(r, len(f["lens"]), flag_mask, min_mapq)]           # (the harness walks every contig, the 1-base one too)
        assert int(m.group(1)) == len(f["recs"])
        assert int(m.group(2)) + int(m.group(3)) == sum(B.runs_of(r)[0].size for r in keep), name
