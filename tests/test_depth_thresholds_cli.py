"""-thresholds SPEC on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli, which has
no threshold entry points, so the host reads the depth back and counts) against rows computed here with numpy from the CPU
oracle's depth (oracle/pd_oracle.py replaying the same command line), plus the option's messages.  Exact integers throughout."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from test_depth_quantiles_cli import CASES, IDS, HERE, capture, cli, run, table_rows  # noqa: F401  (cli: the fixture)

MESSAGE = "Error: -thresholds should be 1 to 16 ascending depths, such as 1,10,20,30"
EXTRA_MARKS = (".quantile.", ".dist.", ".thresholds.")


def main_suffix(tmp):
    names = [f[2:] for f in os.listdir(tmp) if f.endswith(".stat.gz") and not any(m in f for m in EXTRA_MARKS)]
    assert len(names) == 1, names
    return names[0]


def expected(fixture, args, thr, head, rows):
    """[identity columns + Cells + GE...] for every row of the main table, from the oracle's depth"""
    cap = capture(fixture, args)
    tid_of = {}
    for t, n in enumerate(cap["names"]):
        tid_of.setdefault(n, t)
    n_id = 1 if head[1] != "Start" else (4 if head[3] in ("GeneID", "RegionID") else 3)
    out, multi = [], 0
    group, prev = -1, None
    for r in rows:
        t = tid_of[r[0]]
        ln = cap["lens"][t]
        if "contigs" in cap:                                   # -w < 150: the contigs' cells as the sweep saw them, in table order
            if r[0] != prev:
                group, prev = group + 1, r[0]
            cells = cap["contigs"][group][int(r[1]) - 1:int(r[2])]
        else:
            d = cap["depth"][cap["off"][t]:cap["off"][t] + ln]
            if n_id == 1:
                cells = d
            elif n_id == 3:
                cells = d[int(r[1]) - 1:int(r[2])]
            else:
                cds = cap["genes"][t][r[3]].cds
                multi += len(cds) > 1
                cells = np.concatenate([d[min(max(s - 1, 0), ln):min(max(e, 0), ln)] for s, e in cds])
        cells = np.asarray(cells, dtype=np.int64)
        out.append(r[:n_id] + [str(cells.size)] + [str(int((cells >= x).sum())) for x in thr])
    return out, multi


def check_case(cli, fixture, args, spec, tmp_path):
    thr = [int(x) for x in spec.split(",")]
    p = run(cli, fixture, args + ["-thresholds", spec], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    head, rows = table_rows(tmp_path, main_suffix(tmp_path))
    thead, trows = table_rows(tmp_path, "thresholds.stat.gz")
    exp, multi = expected(fixture, args, thr, head, rows)
    assert exp, "a table without rows checks nothing"
    n_id = len(exp[0]) - 1 - len(thr)
    assert thead == head[:n_id] + ["Cells"] + ["GE%d" % x for x in thr]
    assert len(trows) == len(rows)                            # one row per row of the table, in its order ...
    assert trows == exp                                       # ... with its identity columns, the cell count and the counts
    if 0 in thr:
        assert all(r[n_id] == r[n_id + 1 + thr.index(0)] for r in trows)          # GE0 == Cells
    return head, rows, exp, multi, n_id


@pytest.mark.parametrize("spec", ["1", "0,1,5,10,300"])
@pytest.mark.parametrize("fixture,args", CASES, ids=IDS)
def test_thresholds_equal_oracle(cli, fixture, args, spec, tmp_path):
    check_case(cli, fixture, args, spec, tmp_path)


@pytest.mark.parametrize("fixture,args", [CASES[0], CASES[1], CASES[7], CASES[2], CASES[4], CASES[6]], ids=IDS)
def test_ge_d_is_covered_site(cli, fixture, args, tmp_path):
    """GE<D> equals the main table's CoveredSite wherever Cells equals its Length: the default run (D = 1), -d 3 and -d 10"""
    D = int(args[args.index("-d") + 1]) if "-d" in args else 1
    head, rows, exp, _, n_id = check_case(cli, fixture, args, "0,%d,300" % D, tmp_path)
    li, ci = head.index("Length"), head.index("CoveredSite")
    same = [(r, e) for r, e in zip(rows, exp) if r[li] == e[n_id]]
    assert same, "no row has all its cells on the contig"
    for r, e in same:
        assert e[n_id + 2] == r[ci], (r, e)


def test_overlapping_entries_count_twice_and_overhang_clips(cli, tmp_path):
    """q_overlap.bed4 (written by hand): `ov` = chrA 100-200 + 150-250, `tail` = chrA 990-1100 on a 1001-base contig,
    `gone` = chrB 600-700 on a 500-base contig"""
    head, rows, exp, multi, n_id = check_case(cli, "f1", ["-i", "f1.bam", "-b", "q_overlap.bed4"], "0,1,5", tmp_path)
    assert multi == 1
    length = {r[3]: int(r[4]) for r in rows}
    cells = {r[3]: r[4:] for r in exp}
    assert int(cells["ov"][0]) == 101 + 101 == length["ov"]               # cells 150..200 are in the row twice
    assert int(cells["tail"][0]) == 12 < length["tail"] == 111
    assert cells["gone"] == ["0", "0", "0", "0"] and length["gone"] == 101


def test_sixteen_values_are_accepted(cli, tmp_path):
    check_case(cli, "f1", ["-i", "f1.bam", "-w", "200"], ",".join(str(x) for x in range(0, 48, 3)), tmp_path)


@pytest.mark.parametrize("value", ["", "abc", "5,5", "6,5", "-1", ",".join(str(x) for x in range(17)), "5,", ",5", "5 0", "2147483648"])
def test_bad_spec(cli, value, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-thresholds", value], str(tmp_path / "o"))
    assert p.returncode == 0
    assert MESSAGE in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_largest_value_is_accepted(cli, tmp_path):
    check_case(cli, "f1", ["-i", "f1.bam"], "1,2147483647", tmp_path)


def test_missing_value(cli, tmp_path):
    p = subprocess.run([cli, "-i", "f1.bam", "-o", str(tmp_path / "o"), "-thresholds"], cwd=os.path.join(HERE, "golden", "f1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    assert "Error: Lack argument for [ -thresholds ]" in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_without_the_option_no_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam"], str(tmp_path / "o"))
    assert p.returncode == 0
    assert sorted(os.listdir(tmp_path)) == ["o.chr.stat.gz"]
    p = run(cli, "f1", ["-i", "f1.bam", "-thresholds", "1"], str(tmp_path / "o"))
    assert p.returncode == 0
    assert sorted(os.listdir(tmp_path)) == ["o.chr.stat.gz", "o.thresholds.stat.gz"]


def test_adds_exactly_one_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-a", "-thresholds", "1,10"], str(tmp_path / "o"))
    assert p.returncode == 0 and p.stdout.decode() == "INFO: Input data read done\n"
    assert sorted(os.listdir(tmp_path)) == ["o.SiteDepth.gz", "o.chr.stat.gz", "o.thresholds.stat.gz"]


@pytest.mark.parametrize("fixture,args", [("f1", ["-i", "f1.bam"]), ("f1", ["-i", "f1.bam", "-w", "100"]), ("f1", ["-i", "f1.bam", "-g", "f1.gff", "-a"])], ids=IDS)
def test_together_with_the_other_extras(cli, fixture, args, tmp_path):
    """-dist 7 -levels 0,1 -quantile 50 -thresholds 1,10 in one run: every file is what it is alone, and the tables do not change"""
    def files(extra, sub):
        d = tmp_path / sub
        d.mkdir()
        p = run(cli, fixture, args + extra, str(d / "o"))
        assert p.returncode == 0, p.stderr.decode()[-500:]
        return {f: gzip.decompress((d / f).read_bytes()) for f in os.listdir(d)}
    plain = files([], "plain")
    every = files(["-dist", "7", "-levels", "0,1", "-quantile", "50", "-thresholds", "1,10"], "all")
    alone = {}
    for k, extra in enumerate((["-dist", "7"], ["-levels", "0,1"], ["-quantile", "50"], ["-thresholds", "1,10"])):
        got = files(extra, "alone%d" % k)
        assert {f: got[f] for f in plain} == plain
        alone.update({f: got[f] for f in got if f not in plain})
    assert sorted(alone) == ["o.dist.stat.gz", "o.levels.bed.gz", "o.quantile.stat.gz", "o.thresholds.stat.gz"]
    assert every == {**plain, **alone}


def test_empty_paf_writes_the_header_alone(cli, tmp_path):
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "e.paf").write_bytes(b"")
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([cli, "-i", "e.paf", "-thresholds", "1,10", "-o", str(out / "o"), "-t", "2"],
                       cwd=str(tmp_path / "in"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    text = {f: gzip.decompress((out / f).read_bytes()).decode() for f in os.listdir(out)}
    assert sorted(text) == ["o.chr.stat.gz", "o.thresholds.stat.gz"]
    assert text["o.thresholds.stat.gz"] == "#Chr\tCells\tGE1\tGE10\n"
