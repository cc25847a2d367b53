"""-frag on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli) against the model of
tests/frag_model.py — a properly paired read with tlen > 0 counts as the one run [pos, pos + tlen), its mate as nothing.

BAM inputs run with `-X device_decode=0`, as in tests/test_count_deletions_cli.py: the harness's emulated decode session builds its
walk configuration field by field and cannot know the new flag, so here the BAMs go through the host reader's emit_runs; the device
walk's own rule is tested in tests/test_bamwalk_frag.py (64-lane emulation) and tests/test_gpu_fragment.py.  All comparisons exact."""
import os
import subprocess

import numpy as np
import pytest

import del_model as DM
import frag_model as FM
from test_count_deletions_cli import cover_total, rows_of, run, same_sites, sites, stat

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return FM.fragment_corpus(tmp_path_factory.mktemp("frag_cli"))


@pytest.fixture(scope="module")
def f7():
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f7", "m.sam"))
    dep = FM.model(lens, recs)[0]
    plain = DM.model(lens, FM.plain_records(recs), count_del=False)[0]
    return names, lens, recs, dep, plain


def on(names, dep):
    return [(n, d) for n, d in zip(names, dep) if d is not None]


# ---- 1. the golden pair file ----------------------------------------------------------------------------------------
def test_f7_site_depth_and_chr_table_equal_the_model(cli, f7, tmp_path):
    names, lens, recs, dep, plain = f7
    assert sum(1 for r in recs if FM.fragment_class(r) == 1) >= 100 and sum(1 for r in recs if FM.fragment_class(r) == 2) >= 100
    assert any(d is not None and not np.array_equal(d, p) for d, p in zip(dep, plain))            # (not vacuous)
    assert max(int(d.max()) for d in dep if d is not None) < 1 << 18
    outs = {}
    for inp in ("m.sam", "m.bam"):
        _, outs[inp] = run(cli, "f7", ["-i", inp, "-frag", "-a"], str(tmp_path / (inp + ".a")))
        assert same_sites(sites(outs[inp]), names, dep), inp
        head, rows = rows_of(outs[inp], "chr.stat.gz")
        assert [r[0] for r in rows] == [n for n, _ in on(names, dep)]
        assert cover_total(head, rows) == [stat(d, 1) for _, d in on(names, dep)], inp
        _, plain_out = run(cli, "f7", ["-i", inp, "-s", "-a"], str(tmp_path / (inp + ".plain")))
        assert same_sites(sites(plain_out), names, plain) and not same_sites(sites(plain_out), names, dep)
    assert len(outs["m.sam"]) == 2 and (outs["m.sam"] == outs["m.bam"]) is True


# ---- 2. pair flags without mate fields: nothing changes ----------------------------------------------------------------
F1_MODES = [[], ["-a"], ["-w", "100"], ["-g", "f1.gff"], ["-b", "f1.bed4"], ["-del", "-a"]]


@pytest.mark.parametrize("mode", F1_MODES, ids=["_".join(m).replace("-", "") or "chr" for m in F1_MODES])
@pytest.mark.parametrize("inp", ["f1.sam", "f1.bam"])
def test_f1_without_mate_fields_every_byte_stays(cli, inp, mode, tmp_path):
    """f1's reads carry pair flags, but RNEXT is '*' and tlen 0: no read is a fragment read.  The run it is compared with reads the
    input sequentially too (-s), which is what -frag makes of every run"""
    _, _, recs = FM.read_sam(os.path.join(GOLDEN, "f1", "f1.sam"))
    assert any(r[2] & 3 == 3 for r in recs) and all(r[5] == -1 and r[6] == 0 for r in recs)
    a = run(cli, "f1", ["-i", inp, "-s"] + mode, str(tmp_path / "plain"))[1]
    b = run(cli, "f1", ["-i", inp, "-frag"] + mode, str(tmp_path / "frag"))[1]
    assert a and (a == b) is True                                                           # (the .gz bytes)
    if inp == "f1.sam" or mode in ([], ["-a"], ["-w", "100"]):
        # the text input has no index to lose, and the whole-contig modes count the same reads with and without one
        c = run(cli, "f1", ["-i", inp] + mode, str(tmp_path / "indexed"))[1]
        assert {k: len(v) for k, v in c.items()} == {k: len(v) for k, v in b.items()} and sites_or_rows(c) == sites_or_rows(b)


def sites_or_rows(out):
    import gzip
    return {k: gzip.decompress(v) for k, v in out.items()}


# ---- 3. the fragment corpus, written at run time as SAM and BAM ---------------------------------------------------------------
VARIANTS = [("alone", [], dict()), ("del", ["-del"], dict(count_del=True)), ("fragmax", ["-fragmax", str(FM.FRAGMAX_CASE)], dict(frag_max=FM.FRAGMAX_CASE)),
            ("q20", ["-q", "20"], dict(min_mapq=20)), ("x0_q20", ["-x", "0", "-q", "20"], dict(flag_mask=0, min_mapq=20)),
            ("del_fragmax", ["-del", "-fragmax", str(FM.FRAGMAX_CASE)], dict(count_del=True, frag_max=FM.FRAGMAX_CASE))]
_cache = {}


def corpus_model(f, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _cache:
        _cache[key] = FM.model(f["lens"], f["model_recs"], **kw)[0]
        for d in _cache[key]:
            d.setflags(write=False)
    return _cache[key]


@pytest.mark.parametrize("name,args,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_corpus_site_depth_equals_the_model(cli, corpus, name, args, kw, tmp_path):
    f = corpus
    dep = corpus_model(f, **kw)
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f7", ["-i", inp, "-frag", "-a"] + args, str(tmp_path / os.path.basename(inp)))
        assert same_sites(sites(out), f["names"], dep), inp
        head, rows = rows_of(out, "chr.stat.gz")
        assert cover_total(head, rows) == [stat(d, 1) for d in dep]
        outs.append(out)
    assert (outs[0] == outs[1]) is True
    # each variant changes what the plain -frag run gives, and -frag changes what the run without it gives
    if kw:
        assert any(not np.array_equal(a, b) for a, b in zip(dep, corpus_model(f)))
    no_frag = {k: v for k, v in kw.items() if k != "frag_max"}
    assert any(not np.array_equal(a, b) for a, b in zip(dep, DM.model(f["lens"], FM.plain_records(f["model_recs"]), no_frag.get("flag_mask", 1796),
                                                                    no_frag.get("min_mapq", -1), no_frag.get("count_del", False))[0]))


def test_corpus_the_mate_that_decides(corpus):
    """the run belongs to the left mate's record: with -q 20 the pair whose LEFT mate is below the bound loses its fragment (the right
    mate stays silent), the pair whose RIGHT mate is below it keeps it"""
    f = corpus
    dep, q20 = corpus_model(f), corpus_model(f, min_mapq=20)
    at = {c: f["model_recs"][f["offs"].index(o)] for c, o in f["cases"].items()}
    lo, ro = at["left_low_mapq"], at["right_low_mapq"]
    mid_l, mid_r = lo[1] + 250, ro[1] + 250                                   # (inside the fragments, outside the four reads; the two fragments overlap here)
    assert dep[0][mid_l] == 2 and dep[0][mid_r] == 2 and q20[0][mid_l] == 1 and q20[0][mid_r] == 1
    assert q20[0][lo[1] + 5] == 0 and q20[0][ro[1] + 395] == 1               # (left pair: gone altogether; right pair: its fragment reaches its last cell)


@pytest.mark.parametrize("w", [100, 1000])
def test_corpus_window_rows_are_sums_over_the_model(cli, corpus, w, tmp_path):
    f = corpus
    dep = corpus_model(f)
    plain = DM.model(f["lens"], FM.plain_records(f["model_recs"]), count_del=False)[0]
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f7", ["-i", inp, "-frag", "-w", str(w)], str(tmp_path / os.path.basename(inp)))
        head, rows = rows_of(out, "win.stat.gz")
        assert rows and head[:3] == ["#Chr", "Start", "End"]
        exp = [stat(dep[f["names"].index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
        assert cover_total(head, rows) == exp
        assert exp != [stat(plain[f["names"].index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
        seen = {n: sum(int(r[2]) - int(r[1]) + 1 for r in rows if r[0] == n) for n in {r[0] for r in rows}}
        assert all(f["lens"][f["names"].index(n)] - seen[n] in (0, 1) for n in seen)
        outs.append(out)
    assert (outs[0] == outs[1]) is True


def test_corpus_targets_inside_fragments_only(cli, corpus, tmp_path):
    """BED targets that no read touches: they lie between the mates of pairs, some of them tens of thousands of cells behind the end of
    the left mate — a fetch of the reads that overlap the targets would return nothing, the sequential read counts the fragments"""
    f = corpus
    dep = corpus_model(f)
    plain = DM.model(f["lens"], FM.plain_records(f["model_recs"]), count_del=False)[0]
    spans = [("fa", 60210, 60290), ("fa", 63200, 63800), ("fb", 30000, 30100)]              # (1-based, inclusive)
    for n, s, e in spans:
        t = f["names"].index(n)
        assert int(plain[t][s - 1:e].max()) == 0 and int(dep[t][s - 1:e].min()) >= 1
        recs = [r for r in f["model_recs"] if r[0] == t and FM.fragment_class(r) == 1 and r[1] < s - 1 and r[1] + r[6] >= e]
        assert recs and all(r[1] + int((r[4] >> 4)[np.isin(r[4] & 0xf, (0, 2, 3, 7, 8))].sum()) < s - 1 for r in recs)                               # (the carrying reads end before the target begins)
    bed = tmp_path / "inside.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % x for x in spans))
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f7", ["-i", inp, "-frag", "-b", str(bed)], str(tmp_path / os.path.basename(inp)))
        head, rows = rows_of(out, "bed.stat.gz")
        assert sorted((r[0], int(r[1]), int(r[2])) for r in rows) == sorted(spans)
        assert cover_total(head, rows) == [stat(dep[f["names"].index(r[0])][int(r[1]) - 1:int(r[2])], 1) for r in rows]
        outs.append(out)
        _, without = run(cli, "f7", ["-i", inp, "-s", "-b", str(bed)], str(tmp_path / ("plain_" + os.path.basename(inp))))
        h2, r2 = rows_of(without, "bed.stat.gz")
        assert cover_total(h2, r2) == [["0", "0"]] * len(spans)
    assert (outs[0] == outs[1]) is True


# ---- 4. inputs without mate fields are refused -----------------------------------------------------------------------------
def test_cram_and_paf_are_refused(cli, tmp_path):
    lists = {}
    for name, lines in (("cram.list", ["m.bam", "m.cram"]), ("paf.list", [os.path.join(GOLDEN, "f6", "p.paf")] * 2)):
        lists[name] = tmp_path / name
        lists[name].write_text("".join(os.path.join(GOLDEN, "f7", ln) + "\n" if not os.path.isabs(ln) else ln + "\n" for ln in lines))
    unreadable = run(cli, "f7", ["-i", "no_such_file.bam"], str(tmp_path / "missing"), check=False)[0]
    assert unreadable.returncode != 0
    for k, (inp, what) in enumerate([("m.cram", "m.cram"), (os.path.join(GOLDEN, "f6", "p.paf"), "p.paf"), (str(lists["cram.list"]), "m.cram"),
                                     (str(lists["paf.list"]), "p.paf")]):
        p, files = run(cli, "f7", ["-i", inp, "-frag"], str(tmp_path / ("refused%d" % k)), check=False)
        err = p.stderr.decode()
        assert p.returncode == unreadable.returncode and "-frag" in err and what in err and not files, (inp, p.returncode, err)
        # the same input without the flag is read
        p, files = run(cli, "f7", ["-i", inp], str(tmp_path / ("read%d" % k)))
        assert files


# ---- 5. option parsing ---------------------------------------------------------------------------------------------------
def test_option_spellings_and_values(cli, tmp_path):
    one = run(cli, "f7", ["-i", "m.sam", "-frag"], str(tmp_path / "one"))[1]
    two = run(cli, "f7", ["-i", "m.sam", "--frag"], str(tmp_path / "two"))[1]
    plain = run(cli, "f7", ["-i", "m.sam"], str(tmp_path / "plain"))[1]
    assert (one == two) is True and (one != plain) is True and list(one) == ["o.chr.stat.gz"]
    top = run(cli, "f7", ["-i", "m.sam", "-frag", "-fragmax", "2147483647"], str(tmp_path / "top"))[1]
    assert (top == one) is True                                                  # (the default bound)
    low = run(cli, "f7", ["-i", "m.sam", "-frag", "--fragmax", "1"], str(tmp_path / "low"))[1]
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f7", "m.sam"))       # (all pairs but those with |tlen| = 1 are above the bound: two ordinary reads each)
    head, rows = rows_of(low, "chr.stat.gz")
    assert cover_total(head, rows) == [stat(d, 1) for d in FM.model(lens, recs, frag_max=1)[0] if d is not None] and (low != one) is True
    for k, bad in enumerate(["0", "2147483648", "-5", "12x", "", "1e3", "99999999999", "+7"]):
        p, files = run(cli, "f7", ["-i", "m.sam", "-frag", "-fragmax", bad], str(tmp_path / ("bad%d" % k)), check=False)
        assert b"-fragmax should be between 1 and 2147483647" in p.stderr and not files, bad
    p, files = run(cli, "f7", ["-i", "m.sam", "-fragmax", "500"], str(tmp_path / "alone"), check=False)
    assert b"-fragmax needs -frag" in p.stderr and not files
    p, files = run(cli, "f7", ["-i", "m.sam", "-fragg"], str(tmp_path / "typo"), check=False)
    assert b"Error UnKnow argument -fragg" in p.stderr and not files
    h = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-frag" not in h.stdout + h.stderr and b"-a " in h.stdout + h.stderr
