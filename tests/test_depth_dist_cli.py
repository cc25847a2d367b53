"""-dist N on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli, which has no
histogram entry points, so the host reads the depth back and bins it) against an independent Python computation from the CPU
oracle's depth (oracle/pd_oracle.py replaying the same command line), plus the option's messages."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import pd_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = "#Chr\tDepth\tSites\tAtLeast\tAtLeast(%)\n"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


def run(cli, fixture, args, out):
    p = subprocess.run([cli] + args + ["-o", out, "-t", "2"], cwd=os.path.join(HERE, "golden", fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return p


def first_input(fixture, args):
    d = os.path.join(HERE, "golden", fixture)
    path = args[1]
    if path.endswith(".list"):
        path = [ln for ln in open(os.path.join(d, path)).read().splitlines() if ln][0]
    return O.read_alignments(os.path.join(d, path))


def oracle_cells(fixture, args):
    """the oracle's wrapped depth of every counted cell, per contig in table order: [(tid or None, uint32 array)] — every cell of
    the table's contigs in the whole-contig modes, the union of the regions with -g / -b"""
    cap = {}
    real_stat, real_sweep = O.stat_regions, O.sweep_windows

    def stat(depth, off, reg, min_dep):
        cap["depth"], cap["off"], cap["reg"] = depth.copy(), np.asarray(off), np.asarray(reg).reshape(-1, 3)
        return real_stat(depth, off, reg, min_dep)

    def sweep(dc, length, w, min_dep):
        cap.setdefault("contigs", []).append(np.array(dc[:int(length)], dtype=np.uint32))
        return real_sweep(dc, length, w, min_dep)

    O.stat_regions, O.sweep_windows = stat, sweep
    try:
        O.run(args, cwd=os.path.join(HERE, "golden", fixture))
    finally:
        O.stat_regions, O.sweep_windows = real_stat, real_sweep
    if "contigs" in cap:                                       # -w < 150: every contig's cells, in table order
        return [(None, x) for x in cap["contigs"]]
    out = []
    d, off, reg = cap["depth"], cap["off"], cap["reg"]
    whole = "-g" not in args and "-b" not in args
    lens = first_input(fixture, args).lens if whole else None
    for t in sorted(set(int(x) for x in reg[:, 0])):
        mask = np.zeros(int(off[t + 1] - off[t]), dtype=bool)
        if whole:
            mask[:int(lens[t])] = True
        for _, s, e in ([] if whole else reg[reg[:, 0] == t]):
            mask[max(int(s) - 1, 0):max(int(e), 0)] = True     # the union: a cell of overlapping regions counts once
        cells = d[off[t]:off[t + 1]][mask]
        if cells.size:
            out.append((t, cells))
    return out


def blocks_of(text):
    """the file's rows grouped by Chr, in order: [(name, [(label, sites, atleast, pct)])]"""
    lines = text.splitlines()
    assert lines[0] + "\n" == HEADER
    out = []
    for ln in lines[1:]:
        c = ln.split("\t")
        assert len(c) == 5, ln
        if not out or out[-1][0] != c[0]:
            out.append((c[0], []))
        out[-1][1].append((c[1], int(c[2]), int(c[3]), c[4]))
    return out


def expected_rows(cells, n):
    h = np.bincount(np.minimum(cells, n), minlength=n + 1)
    total, at, rows = int(h.sum()), int(h.sum()), []
    for k in range(n + 1):
        if h[k]:
            rows.append((">=%d" % n if k == n else str(k), int(h[k]), at, "%.2f" % (at * 100.0 / total)))
        at -= int(h[k])
    return rows


CASES = [
    ("f1", ["-i", "f1.bam"]),
    ("f1", ["-i", "f1.bam", "-d", "3"]),
    ("f1", ["-i", "f1.bam", "-w", "100"]),
    ("f1", ["-i", "f1.bam", "-w", "200"]),
    ("f1", ["-i", "f1.bam", "-g", "f1.gff"]),
    ("f1", ["-i", "f1.bam", "-g", "f1.gtf"]),
    ("f1", ["-i", "f1.bam", "-b", "f1.bed3"]),
    ("f1", ["-i", "f1.bam", "-b", "f1.bed4", "-d", "10"]),
    ("f1", ["-i", "f1.bam", "-a"]),
    ("f1", ["-i", "f1.bam", "-g", "f1.gff", "-a"]),
    ("f1", ["-i", "f1_3.list"]),
    ("f1", ["-i", "f1_3.list", "-b", "f1.bed4"]),
    ("f1", ["-i", "f1_unsorted.bam"]),
    ("f1", ["-i", "f1_noidx.bam", "-w", "100"]),
    ("f1", ["-i", "f1.bam", "-s"]),
    ("f2", ["-i", "f2.bam", "-b", "f2.bed4"]),
    ("f4", ["-i", "e.bam", "-b", "e.bed"]),
    ("f4", ["-i", "e.bam", "-g", "e.gff"]),
    ("f6", ["-i", "p.paf", "-w", "100"]),
    ("f6", ["-i", "p.list", "-g", "p.gff"]),
]


@pytest.mark.parametrize("n", [1, 7, 200])
@pytest.mark.parametrize("fixture,args", CASES, ids=lambda x: x if isinstance(x, str) else "_".join(x).replace("-", ""))
def test_dist_equals_oracle(cli, fixture, args, n, tmp_path):
    p = run(cli, fixture, args + ["-dist", str(n)], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    got = blocks_of(gzip.decompress((tmp_path / "o.dist.stat.gz").read_bytes()).decode())
    exp_cells = oracle_cells(fixture, args)
    names = O.read_alignments(os.path.join(HERE, "golden", fixture, args[1])).names if not args[1].endswith((".list", ".paf")) else None
    assert len(got) == len(exp_cells) + 1 and got[-1][0] == "*"
    for (name, rows), (t, cells) in zip(got, exp_cells):
        if t is not None and names is not None:
            assert name == names[t]
        assert rows == expected_rows(cells, n), name
    assert got[-1][1] == expected_rows(np.concatenate([c for _, c in exp_cells]), n)


@pytest.mark.parametrize("fixture,args", [c for c in CASES if not any(f in c[1] for f in ("-g", "-b", "-w"))],
                         ids=lambda x: x if isinstance(x, str) else "_".join(x).replace("-", ""))
def test_dist_rederives_the_chr_table(cli, fixture, args, tmp_path):
    """whole-genome mode with N above every depth: the Sites of depth >= -d add up to CoveredSite, depth x Sites to TotalDepth"""
    p = run(cli, fixture, args + ["-dist", "4096"], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    dist = blocks_of(gzip.decompress((tmp_path / "o.dist.stat.gz").read_bytes()).decode())
    chr_rows = [ln.split("\t") for ln in gzip.decompress((tmp_path / "o.chr.stat.gz").read_bytes()).decode().splitlines()
                if not ln.startswith("#")]
    min_dep = int(args[args.index("-d") + 1]) if "-d" in args else 1
    table = {r[0]: (int(r[1]), int(r[2]), int(r[3])) for r in chr_rows}
    assert set(table) == {name for name, _ in dist[:-1]}
    for name, rows in dist[:-1]:
        assert all(not lab.startswith(">=") for lab, *_ in rows)
        L, C, D = table[name]
        assert sum(s for _, s, _, _ in rows) == L
        assert sum(s for lab, s, _, _ in rows if int(lab) >= min_dep) == C
        assert sum(int(lab) * s for lab, s, _, _ in rows if int(lab) >= min_dep) == D     # (TotalDepth sums the depths >= -d)


def test_without_dist_no_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam"], str(tmp_path / "o"))
    assert p.returncode == 0
    assert sorted(os.listdir(tmp_path)) == ["o.chr.stat.gz"]


def test_dist_adds_exactly_one_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-a", "-dist", "3"], str(tmp_path / "o"))
    assert p.returncode == 0 and p.stdout.decode() == "INFO: Input data read done\n"
    assert sorted(os.listdir(tmp_path)) == ["o.SiteDepth.gz", "o.chr.stat.gz", "o.dist.stat.gz"]


@pytest.mark.parametrize("value", ["0", "4097", "abc", "-3", "1.5", ""])
def test_dist_out_of_range(cli, value, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-dist", value], str(tmp_path / "o"))
    assert p.returncode == 0
    assert "Error: -dist should be between 1 and 4096" in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_dist_missing_value(cli, tmp_path):
    p = subprocess.run([cli, "-i", "f1.bam", "-o", str(tmp_path / "o"), "-dist"], cwd=os.path.join(HERE, "golden", "f1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    assert "Error: Lack argument for [ -dist ]" in p.stderr.decode()
    assert os.listdir(tmp_path) == []
