"""-quantile SPEC on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli, which has
no quantile entry points, so the host reads the depth back and selects with std::nth_element) against rows computed here with
numpy from the CPU oracle's depth (oracle/pd_oracle.py replaying the same command line), plus the option's messages."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import pd_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MESSAGE = "Error: -quantile should be 1 to 16 ascending percentages between 0 and 100, such as 25,50,75"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


def run(cli, fixture, args, out):
    return subprocess.run([cli] + args + ["-o", out, "-t", "2"], cwd=os.path.join(HERE, "golden", fixture),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def capture(fixture, args):
    """what the oracle had in hand while replaying the command line: names, lens, the region model, the wrapped depth"""
    cap = {}
    real_stat, real_sweep, real_run, real_parse = O.stat_regions, O.sweep_windows, O._run, O.parse_regions

    def stat(depth, off, reg, min_dep):
        cap["depth"], cap["off"] = depth.copy(), np.asarray(off)
        return real_stat(depth, off, reg, min_dep)

    def sweep(dc, length, w, min_dep):
        cap.setdefault("contigs", []).append(np.array(dc[:int(length)], dtype=np.uint32))
        return real_sweep(dc, length, w, min_dep)

    def _run(o, cwd, files, is_list, first, names, lens, *a, **k):
        cap["names"], cap["lens"] = list(names), [int(x) for x in lens]
        return real_run(o, cwd, files, is_list, first, names, lens, *a, **k)

    def parse(*a, **k):
        cap["genes"] = real_parse(*a, **k)
        return cap["genes"]

    O.stat_regions, O.sweep_windows, O._run, O.parse_regions = stat, sweep, _run, parse
    try:
        O.run(args, cwd=os.path.join(HERE, "golden", fixture))
    finally:
        O.stat_regions, O.sweep_windows, O._run, O.parse_regions = real_stat, real_sweep, real_run, real_parse
    return cap


def nearest_rank(cells, pct):
    """the issue's definition, on a sorted copy"""
    if cells.size == 0:
        return ["NA"] * len(pct)
    s = np.sort(cells)
    return [str(int(s[max(1, (p * cells.size + 99) // 100) - 1])) for p in pct]


def table_rows(tmp, suffix):
    lines = gzip.decompress((tmp / ("o." + suffix)).read_bytes()).decode().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:] if not ln.startswith("##")]


def main_suffix(tmp):
    names = [f[2:] for f in os.listdir(tmp) if f.endswith(".stat.gz") and ".quantile." not in f and ".dist." not in f]
    assert len(names) == 1, names
    return names[0]


def expected(fixture, args, pct, head, rows):
    """[identity columns + Cells + Q...] for every row of the main table, from the oracle's depth"""
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
        out.append(r[:n_id] + [str(cells.size)] + nearest_rank(cells, pct))
    return out, multi


# the cases of test_depth_dist_cli.py
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
IDS = lambda x: x if isinstance(x, str) else "_".join(x).replace("-", "")  # noqa: E731


def check_case(cli, fixture, args, spec, tmp_path):
    pct = [int(x) for x in spec.split(",")]
    p = run(cli, fixture, args + ["-quantile", spec], str(tmp_path / "o"))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    head, rows = table_rows(tmp_path, main_suffix(tmp_path))
    qhead, qrows = table_rows(tmp_path, "quantile.stat.gz")
    exp, multi = expected(fixture, args, pct, head, rows)
    n_id = len(exp[0]) - 1 - len(pct) if exp else None
    if exp:
        assert qhead == head[:n_id] + ["Cells"] + ["Q%d" % x for x in pct]
    assert len(qrows) == len(rows)                            # one row per row of the table, in its order ...
    assert qrows == exp                                       # ... with its identity columns, the cell count and the percentiles
    return exp, multi


@pytest.mark.parametrize("spec", ["50", "0,10,50,90,100"])
@pytest.mark.parametrize("fixture,args", CASES, ids=IDS)
def test_quantile_equals_oracle(cli, fixture, args, spec, tmp_path):
    exp, _ = check_case(cli, fixture, args, spec, tmp_path)
    assert exp, "a table without rows checks nothing"


def test_multi_entry_rows_are_covered(cli, tmp_path):
    """f1.gff's ids have several CDS entries: rows that are a union of entries are among the cases"""
    _, multi = check_case(cli, "f1", ["-i", "f1.bam", "-g", "f1.gff"], "50", tmp_path)
    assert multi > 0


def test_overlapping_entries_count_twice_and_overhang_clips(cli, tmp_path):
    """q_overlap.bed4 (written by hand): `ov` = chrA 100-200 + 150-250, `tail` = chrA 990-1100 on a 1001-base contig,
    `gone` = chrB 600-700 on a 500-base contig"""
    exp, multi = check_case(cli, "f1", ["-i", "f1.bam", "-b", "q_overlap.bed4"], "0,50,100", tmp_path)
    assert multi == 1
    head, rows = table_rows(tmp_path, "bed.stat.gz")
    length = {r[3]: int(r[4]) for r in rows}
    cells = {r[3]: r[4:] for r in exp}
    assert int(cells["ov"][0]) == 101 + 101 == length["ov"]               # cells 150..200 are in the row twice
    assert int(cells["tail"][0]) == 12 < length["tail"] == 111
    assert cells["gone"] == ["0", "NA", "NA", "NA"] and length["gone"] == 101


@pytest.mark.parametrize("value", ["", "abc", "101", "50,50", "60,50", "-1", ",".join(str(x) for x in range(17)), "50,", ",50", "5 0"])
def test_quantile_bad_spec(cli, value, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-quantile", value], str(tmp_path / "o"))
    assert p.returncode == 0
    assert MESSAGE in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_quantile_sixteen_values_are_accepted(cli, tmp_path):
    check_case(cli, "f1", ["-i", "f1.bam", "-w", "200"], ",".join(str(x) for x in range(0, 96, 6)), tmp_path)


def test_quantile_missing_value(cli, tmp_path):
    p = subprocess.run([cli, "-i", "f1.bam", "-o", str(tmp_path / "o"), "-quantile"], cwd=os.path.join(HERE, "golden", "f1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    assert "Error: Lack argument for [ -quantile ]" in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_without_quantile_no_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam"], str(tmp_path / "o"))
    assert p.returncode == 0
    assert sorted(os.listdir(tmp_path)) == ["o.chr.stat.gz"]


def test_quantile_adds_exactly_one_file(cli, tmp_path):
    p = run(cli, "f1", ["-i", "f1.bam", "-a", "-quantile", "50"], str(tmp_path / "o"))
    assert p.returncode == 0 and p.stdout.decode() == "INFO: Input data read done\n"
    assert sorted(os.listdir(tmp_path)) == ["o.SiteDepth.gz", "o.chr.stat.gz", "o.quantile.stat.gz"]


@pytest.mark.parametrize("fixture,args", [("f1", ["-i", "f1.bam"]), ("f1", ["-i", "f1.bam", "-w", "100"]), ("f1", ["-i", "f1.bam", "-g", "f1.gff", "-a"])], ids=IDS)
def test_together_with_dist_and_levels(cli, fixture, args, tmp_path):
    """-dist 7 -levels 0,1 -quantile 50 in one run: every file is what it is alone, and the tables do not change"""
    def files(extra, sub):
        d = tmp_path / sub
        d.mkdir()
        p = run(cli, fixture, args + extra, str(d / "o"))
        assert p.returncode == 0, p.stderr.decode()[-500:]
        return {f: gzip.decompress((d / f).read_bytes()) for f in os.listdir(d)}
    plain = files([], "plain")
    both = files(["-dist", "7", "-levels", "0,1", "-quantile", "50"], "all")
    alone = {}
    for k, extra in enumerate((["-dist", "7"], ["-levels", "0,1"], ["-quantile", "50"])):
        got = files(extra, "alone%d" % k)
        assert {f: got[f] for f in plain} == plain
        alone.update({f: got[f] for f in got if f not in plain})
    assert sorted(alone) == ["o.dist.stat.gz", "o.levels.bed.gz", "o.quantile.stat.gz"]
    assert both == {**plain, **alone}


def test_empty_paf_writes_every_extra_empty(cli, tmp_path):
    """a PAF without a single line has no targets: the main table is its header and last line, and every extra output is
    what it holds without rows — -dist and -quantile their header, -levels nothing"""
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "e.paf").write_bytes(b"")
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([cli, "-i", "e.paf", "-dist", "8", "-levels", "exact", "-quantile", "50", "-o", str(out / "o"), "-t", "2"],
                       cwd=str(tmp_path / "in"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    text = {f: gzip.decompress((out / f).read_bytes()).decode() for f in os.listdir(out)}
    assert sorted(text) == ["o.chr.stat.gz", "o.dist.stat.gz", "o.levels.bed.gz", "o.quantile.stat.gz"]
    main = text["o.chr.stat.gz"].splitlines()
    assert len(main) == 2 and main[0] == "#Chr\tLength\tCoveredSite\tTotalDepth\tCoverage(%)\tMeanDepth"
    assert main[1].startswith("##RegionLength: 0\tCoveredSite: 0\t")
    assert text["o.dist.stat.gz"] == "#Chr\tDepth\tSites\tAtLeast\tAtLeast(%)\n"
    assert text["o.levels.bed.gz"] == ""
    assert text["o.quantile.stat.gz"] == "#Chr\tCells\tQ50\n"
