"""-levels SPEC on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli, which has no
pd_depth_levels member, so the host reads the depth back and finds the runs itself) against an independent Python computation:
the CPU oracle's wrapped depth (oracle/pd_oracle.py replaying the same command line), the covered cells WITH their positions,
and numpy run-finding.  Plus the file's invariants, the chunked walk, and the option's messages."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import pd_oracle as O
from test_depth_dist_cli import CASES, first_input

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MESSAGE = "Error: -levels should be 'exact' or up to 64 ascending depths such as 0,1,5,15"
SPECS = ["exact", "0,1,5,15", "3", "1,2"]
IDS = lambda x: x if isinstance(x, str) else "_".join(x).replace("-", "")  # noqa: E731


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


def run(cli, fixture, args, out):
    return subprocess.run([cli] + args + ["-o", out, "-t", "2"], cwd=os.path.join(HERE, "golden", fixture),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def oracle_cells(fixture, args):
    """the oracle's wrapped depth of every counted cell with its position, per contig in table order:
    [(tid or None, positions int64 ascending, depth uint32)] — every cell of the table's contigs in the whole-contig and window
    modes, the union of the regions with -g / -b (the definition test_depth_dist_cli.oracle_cells uses, positions kept)"""
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
    if "contigs" in cap:
        return [(None, np.arange(x.size, dtype=np.int64), x) for x in cap["contigs"]]
    out = []
    d, off, reg = cap["depth"], cap["off"], cap["reg"]
    whole = "-g" not in args and "-b" not in args
    lens = first_input(fixture, args).lens if whole else None
    for t in sorted(set(int(x) for x in reg[:, 0])):
        mask = np.zeros(int(off[t + 1] - off[t]), dtype=bool)
        if whole:
            mask[:int(lens[t])] = True
        for _, s, e in ([] if whole else reg[reg[:, 0] == t]):
            mask[max(int(s) - 1, 0):max(int(e), 0)] = True
        pos = np.nonzero(mask)[0].astype(np.int64)
        if pos.size:
            out.append((t, pos, np.asarray(d[off[t]:off[t + 1]][mask], dtype=np.uint32)))
    return out


def edges_of(spec):
    return None if spec == "exact" else [int(x) for x in spec.split(",")]


def expected_rows(pos, depth, spec):
    """[(start, end, value text)]: maximal stretches of consecutive covered cells of one class"""
    edges = edges_of(spec)
    cls = depth.astype(np.int64) if edges is None else np.searchsorted(np.asarray(edges, dtype=np.int64), depth.astype(np.int64), side="right") - 1
    brk = np.ones(pos.size, dtype=bool)
    brk[1:] = (pos[1:] != pos[:-1] + 1) | (cls[1:] != cls[:-1])
    first = np.nonzero(brk)[0]
    last = np.append(first[1:], pos.size) - 1
    rows = []
    for a, b in zip(first, last):
        c = int(cls[a])
        if edges is None:
            rows.append((int(pos[a]), int(pos[b]) + 1, str(c)))
        elif c >= 0:
            rows.append((int(pos[a]), int(pos[b]) + 1, "%d:%s" % (edges[c], edges[c + 1] if c + 1 < len(edges) else "inf")))
    return rows


def parse(text):
    """the file's rows grouped by contig, in order: [(name, [(start, end, value text)])]"""
    assert text == "" or text.endswith("\n")
    out = []
    for ln in text.splitlines():
        c = ln.split("\t")
        assert len(c) == 4, ln
        if not out or out[-1][0] != c[0]:
            out.append((c[0], []))
        out[-1][1].append((int(c[1]), int(c[2]), c[3]))
    assert len({name for name, _ in out}) == len(out), "a contig's rows are not together"
    return out


def levels_text(tmp_path, stem="o"):
    return gzip.decompress((tmp_path / (stem + ".levels.bed.gz")).read_bytes()).decode()


def known_names(fixture, args):
    return None if args[1].endswith((".list", ".paf")) else O.read_alignments(os.path.join(HERE, "golden", fixture, args[1])).names


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("fixture,args", CASES, ids=IDS)
def test_levels_equal_oracle(cli, fixture, args, spec, tmp_path):
    p = run(cli, fixture, args + ["-levels", spec], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    text = levels_text(tmp_path)
    got = parse(text)
    cells = oracle_cells(fixture, args)
    names = known_names(fixture, args)
    exp = [(t, expected_rows(pos, d, spec)) for t, pos, d in cells]
    exp = [(t, rows) for t, rows in exp if rows]               # (a contig whose cells all lie below the first edge has no row)
    assert len(got) == len(exp)
    lines = []
    for (name, rows), (t, erows) in zip(got, exp):
        if t is not None and names is not None:
            assert name == names[t]
        assert rows == erows, name
        lines += ["%s\t%d\t%d\t%s\n" % (name, s, e, v) for s, e, v in erows]
    assert text == "".join(lines)                              # the whole decompressed text: nothing but these rows, this format


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("fixture,args", CASES, ids=IDS)
def test_levels_invariants(cli, fixture, args, spec, tmp_path):
    p = run(cli, fixture, args + ["-levels", spec], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    got = parse(levels_text(tmp_path))
    cells = oracle_cells(fixture, args)
    edges = edges_of(spec)
    for name, rows in got:
        for (s, e, v), nxt in zip(rows, rows[1:] + [None]):
            assert 0 <= s < e
            if nxt is not None:
                assert e <= nxt[0], "rows overlap or descend"
                assert not (e == nxt[0] and v == nxt[2]), "touching rows with one value: not maximal"
    # coverage of the covered cells: exact and edges starting at 0 tile them; with e_0 > 0 exactly the cells below e_0 are missing
    kept = [(t, pos, d) for t, pos, d in cells if edges is None or (d >= edges[0]).any()]
    assert len(got) == len(kept)
    for (name, rows), (t, pos, d) in zip(got, kept):
        covered = np.concatenate([np.arange(s, e, dtype=np.int64) for s, e, _ in rows])
        want = pos if edges is None else pos[d >= edges[0]]
        assert np.array_equal(covered, want), name
        if edges is None:                                       # expanding the rows reproduces depth x position
            values = np.concatenate([np.full(e - s, int(v), dtype=np.int64) for s, e, v in rows])
            assert np.array_equal(values, d.astype(np.int64)), name


@pytest.mark.parametrize("fixture,args", [c for c in CASES if not any(f in c[1] for f in ("-g", "-b", "-w"))], ids=IDS)
def test_exact_levels_rederive_the_chr_table(cli, fixture, args, tmp_path):
    p = run(cli, fixture, args + ["-levels", "exact"], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    got = parse(levels_text(tmp_path))
    chr_rows = [ln.split("\t") for ln in gzip.decompress((tmp_path / "o.chr.stat.gz").read_bytes()).decode().splitlines()
                if not ln.startswith("#")]
    min_dep = int(args[args.index("-d") + 1]) if "-d" in args else 1
    table = {r[0]: (int(r[1]), int(r[2]), int(r[3])) for r in chr_rows}
    assert set(table) == {name for name, _ in got}
    for name, rows in got:
        L, C, D = table[name]
        assert sum(e - s for s, e, _ in rows) == L
        assert sum(e - s for s, e, v in rows if int(v) >= min_dep) == C
        assert sum((e - s) * int(v) for s, e, v in rows if int(v) >= min_dep) == D


@pytest.mark.parametrize("fixture,args", [c for c in CASES if "-a" in c[1] and not any(f in c[1] for f in ("-g", "-b", "-w"))], ids=IDS)
def test_exact_levels_expand_to_the_site_file(cli, fixture, args, tmp_path):
    p = run(cli, fixture, args + ["-levels", "exact"], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    site = gzip.decompress((tmp_path / "o.SiteDepth.gz").read_bytes()).decode()
    lines = []
    for name, rows in parse(levels_text(tmp_path)):
        for s, e, v in rows:
            lines += ["%s\t%d\t%s\n" % (name, i, v) for i in range(s, e)]
    assert "".join(lines) == site


CHUNKED = [CASES[0], CASES[4], CASES[11]]                         # whole contigs, -g gff, a list with -b bed4


@pytest.mark.parametrize("spec", ["exact", "0,1,5,15"])
@pytest.mark.parametrize("fixture,args", CHUNKED, ids=IDS)
def test_chunked_walk_gives_the_same_text(cli, fixture, args, spec, tmp_path):
    assert run(cli, fixture, args + ["-levels", spec], str(tmp_path / "whole")).returncode == 0
    whole = levels_text(tmp_path, "whole")
    assert whole
    for chunk in ("7", "1000"):
        p = run(cli, fixture, args + ["-levels", spec, "-X", "levels_chunk=" + chunk], str(tmp_path / ("c" + chunk)))
        assert p.returncode == 0, p.stderr.decode()[-500:]
        assert levels_text(tmp_path, "c" + chunk) == whole, chunk


BAD_SPECS = ["", "1,1", "5,1", "0,1,5,3", "-1", "+1", "1,,2", "1,", ",1", "a", "1,2,x", "exact,1", "Exact", "1.5", "0x10", " 1", "2147483648",
             "99999999999", ",".join(str(k) for k in range(65))]


@pytest.mark.parametrize("value", BAD_SPECS, ids=lambda v: "spec[%s]" % v[:24])
def test_levels_malformed_spec(cli, value, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-levels", value], str(tmp_path / "o"))
    assert p.returncode == 0
    assert MESSAGE in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_levels_accepts_64_edges_and_the_largest_edge(cli, tmp_path):
    spec = ",".join(str(k) for k in range(63)) + ",2147483647"
    p = run(cli, "f1", ["-i", "f1.bam", "-levels", spec], str(tmp_path / "o"))
    assert p.returncode == 0 and MESSAGE not in p.stderr.decode()
    got = parse(levels_text(tmp_path))
    cells = oracle_cells("f1", ["-i", "f1.bam"])
    assert [rows for _, rows in got] == [expected_rows(pos, d, spec) for _, pos, d in cells]


def test_levels_missing_value(cli, tmp_path):
    p = subprocess.run([cli, "-i", "f1.bam", "-o", str(tmp_path / "o"), "-levels"], cwd=os.path.join(HERE, "golden", "f1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    assert "Error: Lack argument for [ -levels ]" in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_levels_adds_exactly_one_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-a"], str(tmp_path / "o"))
    assert p.returncode == 0
    before = sorted(os.listdir(tmp_path))
    assert before == ["o.SiteDepth.gz", "o.chr.stat.gz"]
    p = run(cli, "f1", ["-i", "f1.bam", "-a", "-levels", "0,1,5,15"], str(tmp_path / "o"))
    assert p.returncode == 0 and p.stdout.decode() == "INFO: Input data read done\n"
    assert sorted(os.listdir(tmp_path)) == sorted(before + ["o.levels.bed.gz"])


def test_levels_and_dist_together(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-dist", "5", "-levels", "exact"], str(tmp_path / "o"))
    assert p.returncode == 0 and p.stdout.decode() == "INFO: Input data read done\n"
    assert sorted(os.listdir(tmp_path)) == ["o.chr.stat.gz", "o.dist.stat.gz", "o.levels.bed.gz"]
    q = run(cli, "f1", ["-i", "f1.bam", "-levels", "exact"], str(tmp_path / "p"))
    assert q.returncode == 0
    assert levels_text(tmp_path, "o") == levels_text(tmp_path, "p")


def test_help_does_not_list_levels(cli):
    p = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"levels" not in p.stdout + p.stderr
