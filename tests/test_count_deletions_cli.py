"""-del on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli) against the model of
tests/del_model.py — depth where deletions count as covered, taken per operation from the SAM text (or the PAF's cg:Z: strings).

BAM inputs run with `-X device_decode=0`: the harness's emulated decode session builds its walk configuration field by field and
cannot know the new flag (it keeps compiling and behaving as it did), so here the BAMs go through the host reader's emit_runs; the
device walk's own rule is tested in tests/test_bamwalk_del.py (64-lane emulation) and tests/test_gpu_count_deletions.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import del_model as DM
from test_depth_dist_cli import blocks_of, expected_rows
from test_depth_quantiles_cli import CASES, IDS, capture, nearest_rank

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# fixture -> (the SAM the model reads, [(input, extra arguments)]); inputs on one line of SAME must give identical files
INPUTS = {
    "f1": ("f1.sam", [("f1.sam", []), ("f1.bam", []), ("f1_unsorted.sam", []), ("f1_noidx.bam", ["-s"])]),
    "f5": ("c.sam", [("c.sam", []), ("c.bam", [])]),
    "f7": ("m.sam", [("m.sam", []), ("m.bam", []), ("m.cram", []), ("m_v31.cram", [])]),
}
SAME = [("f1", ["f1.sam", "f1.bam"]), ("f5", ["c.sam", "c.bam"]), ("f7", ["m.sam", "m.bam", "m.cram", "m_v31.cram"])]


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


def host_only(args):
    """BAM inputs: the host reader (see the module's docstring)"""
    return args + (["-X", "device_decode=0"] if any(a.endswith(".bam") or a.endswith(".list") for a in args) else [])


def run(cli, fixture, args, out_dir, check=True):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([cli] + host_only(args) + ["-o", os.path.join(out_dir, "o"), "-t", "2"], cwd=os.path.join(GOLDEN, fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-500:]
    return p, {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def text(files, suffix):
    (name,) = [f for f in files if f.endswith(suffix)]
    return gzip.decompress(files[name]).decode()


def rows_of(files, suffix):
    lines = text(files, suffix).splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:] if not ln.startswith("##")]


def main_table(files):
    (name,) = [f for f in files if f.endswith(".stat.gz") and not any(x in f for x in (".dist.", ".quantile.", ".thresholds."))]
    return name[2:]


_models = {}


def sam_model(fixture, sam=None):
    """(names, lens, depth with deletions, depth without) of a fixture's SAM, computed once"""
    sam = sam or INPUTS[fixture][0]
    if (fixture, sam) not in _models:
        names, lens, recs = DM.read_sam(os.path.join(GOLDEN, fixture, sam))
        with_d, without = DM.model(lens, recs)[0], DM.model(lens, recs, count_del=False)[0]
        _models[fixture, sam] = names, lens, with_d, without, recs
    return _models[fixture, sam]


def sites(files):
    """SiteDepth.gz -> {contig: depth by cell}; every contig's lines are its cells 0, 1, 2 ... in order"""
    out = {}
    for ln in text(files, "SiteDepth.gz").splitlines():
        n, i, d = ln.split("\t")
        out.setdefault(n, []).append((int(i), int(d)))
    for n, v in out.items():
        assert [i for i, _ in v] == list(range(len(v))), n
    return {n: np.array([d for _, d in v], dtype=np.uint32) for n, v in out.items()}


def same_sites(got, names, depth):
    """(compared array by array: a failing comparison of two long texts sends pytest into a diff that takes minutes)"""
    want = {n: d for n, d in zip(names, depth) if d is not None}
    return sorted(got) == sorted(want) and all(np.array_equal(got[n], want[n]) for n in want)


def stat(cells, min_dep):
    keep = cells[cells >= min_dep]
    return [str(keep.size), str(int(keep.sum(dtype=np.uint64)))]


def cover_total(head, rows):
    c = head.index("CoveredSite")
    return [r[c:c + 2] for r in rows]


# ---- 1. depth equals the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", sorted(INPUTS))
def test_site_depth_and_chr_table_equal_the_model(cli, fixture, tmp_path):
    names, lens, dep, plain, recs = sam_model(fixture)
    # not vacuous: the deletions change the depth of this fixture, and no cell reaches the 18-bit wrap
    assert DM.has_gaps(recs) and any(d is not None and not np.array_equal(d, p) for d, p in zip(dep, plain))
    assert max(int(d.max()) for d in dep if d is not None) < 1 << 18
    for inp, extra in INPUTS[fixture][1]:
        if inp.endswith(".sam") and inp != INPUTS[fixture][0]:
            n2, l2, d2, _, r2 = sam_model(fixture, inp)
            assert (n2, l2) == (names, lens) and DM.has_gaps(r2)
        else:
            d2 = dep
        _, out = run(cli, fixture, ["-i", inp, "-del", "-a"] + extra, str(tmp_path / (inp + ".a")))
        assert same_sites(sites(out), names, d2), inp
        for min_dep in (None, 3):
            _, out = run(cli, fixture, ["-i", inp, "-del"] + extra + (["-d", "3"] if min_dep else []), str(tmp_path / ("%s.d%s" % (inp, min_dep))))
            head, rows = rows_of(out, "chr.stat.gz")
            assert [r[0] for r in rows] == [n for n, d in zip(names, d2) if d is not None]
            assert cover_total(head, rows) == [stat(d, min_dep or 1) for d in d2 if d is not None], (inp, min_dep)


@pytest.mark.parametrize("fixture,inputs", SAME, ids=[s[0] for s in SAME])
@pytest.mark.parametrize("mode", [["-a"], ["-w", "100"]], ids=IDS)
def test_bam_cram_and_sam_give_identical_files(cli, fixture, inputs, mode, tmp_path):
    outs = [run(cli, fixture, ["-i", inp, "-del"] + mode, str(tmp_path / inp))[1] for inp in inputs]
    assert len(outs[0]) == (2 if mode == ["-a"] else 1) and all((o == outs[0]) is True for o in outs[1:])


# ---- 2. windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [100, 1000])
@pytest.mark.parametrize("fixture,inp", [("f1", "f1.bam"), ("f1", "f1.sam"), ("f7", "m.bam"), ("f7", "m.cram")])
def test_window_rows_are_sums_over_the_model(cli, fixture, inp, w, tmp_path):
    names, lens, dep, plain, _ = sam_model(fixture)
    _, out = run(cli, fixture, ["-i", inp, "-del", "-w", str(w)], str(tmp_path / "o"))
    head, rows = rows_of(out, "win.stat.gz")
    assert rows and head[:3] == ["#Chr", "Start", "End"]
    exp = [stat(dep[names.index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
    assert cover_total(head, rows) == exp
    assert exp != [stat(plain[names.index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
    seen = {n: sum(int(r[2]) - int(r[1]) + 1 for r in rows if r[0] == n) for n in {r[0] for r in rows}}
    assert all(lens[names.index(n)] - seen[n] in (0, 1) for n in seen)           # (the reference's sweep leaves out a last window of one base)


# ---- 3. regions ----------------------------------------------------------------------------------------------------
# (f4's targets sit on contig ends, where the reference's widened index fetch does not return every read that covers a target's cell —
# behaviour this option leaves alone: its CIGARs hold no D / N, and test_without_deletions_every_byte_stays compares those bytes)
REGION_CASES = [(f, a) for f, a in CASES if ("-g" in a or "-b" in a) and a[1].endswith(".bam") and f != "f4"]


def bam_model(fixture, bam):
    if (fixture, bam) not in _models:
        lens, recs = DM.read_bam(os.path.join(GOLDEN, fixture, bam))
        _models[fixture, bam] = lens, DM.model(lens, recs)[0], DM.model(lens, recs, count_del=False)[0]
    return _models[fixture, bam]


@pytest.mark.parametrize("fixture,args", REGION_CASES, ids=IDS)
def test_region_rows_are_sums_over_the_model(cli, fixture, args, tmp_path):
    """every row's CoveredSite / TotalDepth over the row's entries: a cell inside a target sees every read that covers it, so the
    whole file's model is the depth there (the region model — which cells a row has — is the oracle's parse of the annotation)"""
    assert len(REGION_CASES) >= 6 and sum(f == "f1" for f, _ in REGION_CASES) >= 5
    lens, dep, plain = bam_model(fixture, args[1])
    min_dep = int(args[args.index("-d") + 1]) if "-d" in args else 1
    cap = capture(fixture, args)
    assert cap["lens"] == lens
    _, out = run(cli, fixture, args + ["-del"], str(tmp_path / "o"))
    head, rows = rows_of(out, main_table(out))
    tid_of = {}
    for t, n in enumerate(cap["names"]):
        tid_of.setdefault(n, t)
    exp, exp_plain = [], []
    for r in rows:
        t = tid_of[r[0]]
        for d, dst in ((dep[t], exp), (plain[t], exp_plain)):
            if head[3] in ("GeneID", "RegionID"):
                cells = np.concatenate([d[min(max(s - 1, 0), lens[t]):min(max(e, 0), lens[t])] for s, e in cap["genes"][t][r[3]].cds])
            else:
                cells = d[int(r[1]) - 1:int(r[2])]
            dst.append(stat(cells, min_dep))
    assert rows and cover_total(head, rows) == exp
    if fixture == "f1":                                                           # (f2's CIGARs hold no D / N)
        assert exp != exp_plain


# ---- 4. the extras ---------------------------------------------------------------------------------------------------
def test_extras_are_computed_from_the_same_depth(cli, tmp_path):
    names, lens, dep, plain, _ = sam_model("f1")
    _, out = run(cli, "f1", ["-i", "f1.bam", "-del", "-thresholds", "1,5", "-quantile", "50", "-levels", "exact", "-dist", "8"], str(tmp_path / "o"))
    assert sorted(out) == ["o.chr.stat.gz", "o.dist.stat.gz", "o.levels.bed.gz", "o.quantile.stat.gz", "o.thresholds.stat.gz"]
    on = [(n, d) for n, d in zip(names, dep) if d is not None]
    _, rows = rows_of(out, "thresholds.stat.gz")
    assert rows == [[n, str(d.size), str(int((d >= 1).sum())), str(int((d >= 5).sum()))] for n, d in on]
    _, rows = rows_of(out, "quantile.stat.gz")
    assert rows == [[n, str(d.size)] + nearest_rank(d, [50]) for n, d in on]
    # every row — label, Sites, AtLeast, AtLeast(%) — of every contig's block and of the closing block over all of them
    assert blocks_of(text(out, "dist.stat.gz")) == [(n, expected_rows(d, 8)) for n, d in on] + [("*", expected_rows(np.concatenate([d for _, d in on]), 8))]
    levels = [ln.split("\t") for ln in text(out, "levels.bed.gz").splitlines() if not ln.startswith("#")]
    for n, d in on:
        cuts = np.flatnonzero(np.diff(d.astype(np.int64))) + 1
        beg, end = np.concatenate([[0], cuts]), np.concatenate([cuts, [d.size]])
        assert [r[1:4] for r in levels if r[0] == n] == [[str(b), str(e), str(int(d[b]))] for b, e in zip(beg.tolist(), end.tolist())]
    assert any(not np.array_equal(d, p) for d, p in zip(dep, plain) if d is not None)


# ---- 5. PAF ----------------------------------------------------------------------------------------------------------
def test_paf_cg_strings_count_deletions(cli, tmp_path):
    _, plain_out = run(cli, "f6", ["-i", "p.paf", "-a"], str(tmp_path / "plain"))
    _, out = run(cli, "f6", ["-i", "p.paf", "-del", "-a"], str(tmp_path / "del"))
    head, rows = rows_of(out, "chr.stat.gz")
    names, lens = [r[0] for r in rows], [int(r[1]) for r in rows]
    path = os.path.join(GOLDEN, "f6", "p.paf")
    dep, n_gap = DM.paf_model(path, names, lens)
    assert n_gap == 72
    assert same_sites(sites(out), names, dep)
    assert same_sites(sites(plain_out), names, DM.paf_model(path, names, lens, count_del=False)[0])
    assert not same_sites(sites(plain_out), names, dep)
    # lines without cg:Z: are unchanged: a file of those lines alone gives the same bytes with and without -del
    bare = tmp_path / "bare.paf"
    bare.write_text("".join(ln for ln in open(path) if "cg:Z:" not in ln))
    a = run(cli, "f6", ["-i", str(bare), "-a"], str(tmp_path / "bare_plain"))[1]
    b = run(cli, "f6", ["-i", str(bare), "-del", "-a"], str(tmp_path / "bare_del"))[1]
    assert (a == b) is True and len(a) == 2 and int(rows_of(a, "chr.stat.gz")[1][0][3]) > 0


# ---- 6. no deletions, no change ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp,args", [("e.sam", ["-a"]), ("e.bam", ["-a"]), ("e.bam", ["-w", "100"]), ("e.bam", ["-g", "e.gff"]), ("e_noidx.bam", ["-s", "-a"]),
                                      ("e_noidx.bam", ["-w", "1000"])], ids=IDS)
def test_without_deletions_every_byte_stays(cli, inp, args, tmp_path):
    _, _, recs = DM.read_sam(os.path.join(GOLDEN, "f4", "e.sam"))
    assert recs and not DM.has_gaps(recs)
    a = run(cli, "f4", ["-i", inp] + args, str(tmp_path / "plain"))[1]
    b = run(cli, "f4", ["-i", inp, "-del"] + args, str(tmp_path / "del"))[1]
    assert a and (a == b) is True                                                           # (the .gz bytes)


# ---- 7. option parsing -------------------------------------------------------------------------------------------------
def test_option_spellings(cli, tmp_path):
    one = run(cli, "f1", ["-i", "f1.sam", "-del"], str(tmp_path / "one"))[1]
    two = run(cli, "f1", ["-i", "f1.sam", "--del"], str(tmp_path / "two"))[1]
    plain = run(cli, "f1", ["-i", "f1.sam"], str(tmp_path / "plain"))[1]
    assert (one == two) is True and (one != plain) is True and list(one) == ["o.chr.stat.gz"]
    p, files = run(cli, "f1", ["-i", "f1.sam", "-dell"], str(tmp_path / "typo"), check=False)
    assert b"Error UnKnow argument -dell" in p.stderr and not files
    h = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-del" not in h.stdout + h.stderr and b"-a " in h.stdout + h.stderr
