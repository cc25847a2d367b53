"""-alnstats on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli) against the model of
tests/alnstats_model.py.  The harness's engine table ends before the new member, so every input here is counted by the host readers
(read_bam_device gives a BAM back before anything is counted); the device pass has tests/test_alnstats_walk.py (64-lane emulation) and
tests/test_gpu_alnstats.py / tests/test_gpu_alnstats_cli.py.  All comparisons are of exact bytes or text."""
import gzip
import os
import subprocess

import pytest

import alnstats_model as AM
import bam_craft as B
import frag_model as FM
import recstats_model as RM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
STAT = "o.aln.stat.gz"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the records corpus of tests/recstats_model.py (a SAM and a BAM of the same records, pairs, CG tags, wave-walked CIGARs)"""
    return RM.corpus(tmp_path_factory.mktemp("alnstats_cli"))


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    return AM.edges_file(tmp_path_factory.mktemp("alnstats_cli_edges"))


def run(cli, fixture, args, out_dir, check=True):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([cli] + args + ["-o", os.path.join(out_dir, "o"), "-t", "2"], cwd=os.path.join(GOLDEN, fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-500:]
    return p, {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def stat_text(files):
    return gzip.decompress(files[STAT]).decode()


def model_text(n_ref, recs, w, flag_mask=1796, min_mapq=-1, times=1):
    m = AM.Model(n_ref, flag_mask, min_mapq, w)
    for _ in range(times):
        m.add_tuples(recs)
    return m.text()


def section(text, tag):
    return [ln.split("\t")[1:] for ln in text.splitlines() if ln.startswith(tag + "\t")]


# ---- 1. the corpora, written at run time ----------------------------------------------------------------------------------
VARIANTS = [("default", [], dict()), ("q20", ["-q", "20"], dict(min_mapq=20)), ("x0", ["-x", "0"], dict(flag_mask=0)),
            ("x0_q20", ["-x", "0", "-q", "20"], dict(flag_mask=0, min_mapq=20))]


@pytest.mark.parametrize("w", AM.WIDTHS)
@pytest.mark.parametrize("name,args,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_corpus_as_sam_and_bam(cli, corpus, name, args, kw, w, tmp_path):
    f = corpus
    want = model_text(len(f["lens"]), f["model_recs"], w, **kw)
    assert want == AM.Model(len(f["lens"]), kw.get("flag_mask", 1796), kw.get("min_mapq", -1), w).add_parsed(f["recs"]).text()     # (the CG rule, both ways)
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f1", ["-i", inp, "-alnstats", str(w)] + args, str(tmp_path / os.path.basename(inp)))
        assert stat_text(out) == want, inp
        outs.append(out)
    assert outs[0][STAT] == outs[1][STAT]                                         # (the .gz bytes)


@pytest.mark.parametrize("w", AM.WIDTHS)
@pytest.mark.parametrize("name,args,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_the_edges_file(cli, edges, name, args, kw, w, tmp_path):
    """operation codes 9 .. 15, lengths of 2^28 - 1, CG tags that count and that do not: through the host BAM reader"""
    f = edges
    m = AM.Model(len(f["lens"]), kw.get("flag_mask", 1796), kw.get("min_mapq", -1), w).add_parsed(f["recs"])
    _, out = run(cli, "f1", ["-i", f["path"], "-alnstats", str(w)] + args, str(tmp_path / "o"))
    text = stat_text(out)
    assert text == m.text()
    # the invariant: the ID rows add up to the OP rows of I and D
    ops = {r[0]: int(r[1]) for r in section(text, "OP")}
    ids = section(text, "ID")
    assert [r[0] for r in section(text, "OP")] == AM.OP_NAMES
    assert sum(int(r[1]) for r in ids) == ops["I"] > 0 and sum(int(r[2]) for r in ids) == ops["D"] > 0
    assert {"0", "1", "255", ">=256"} <= {r[0] for r in ids} and "256" not in {r[0] for r in ids}
    sn = {r[0]: r[1] for r in section(text, "SN")}
    assert sn["read_n50"] == ">=%d" % (8191 * w) and sn["bin_width"] == str(w) and sn["len_bins"] == "8192"
    assert section(text, "RL")[-1][1] == "inf" and section(text, "AL")[-1][1] == "inf"


def test_n50_against_a_sort(cli, corpus, tmp_path):
    """W = 1 below 8191 bases: read_n50 is the N50 of the primary reads' lengths"""
    f = corpus
    lengths = []
    for r in f["model_recs"]:
        m = AM.Model(len(f["lens"]), 1796, -1, 1)
        m.add(r[0], r[2], r[3], r[4])
        if m.s[AM.PRIMARY]:
            lengths.append(m.s[AM.READ_BASES])
    want = AM.sorted_n50(lengths)
    assert len(lengths) > 1000 and len(set(lengths)) > 5 and 0 < want < 8191
    sn = {r[0]: r[1] for r in section(stat_text(run(cli, "f1", ["-i", f["path"], "-alnstats", "1"], str(tmp_path / "w1"))[1]), "SN")}
    assert sn["read_n50"] == str(want) and sn["read_max"] == str(max(lengths)) and sn["read_bases"] == str(sum(lengths))
    assert sn["read_mean"] == "%.2f" % (sum(lengths) / len(lengths)) and sn["primary"] == str(len(lengths))
    sn100 = {r[0]: r[1] for r in section(stat_text(run(cli, "f1", ["-i", f["path"], "-alnstats", "100"], str(tmp_path / "w100"))[1]), "SN")}
    assert int(sn100["read_n50"]) == want // 100 * 100                            # (a bin's lower edge: a lower bound)


def test_nothing_aligned_prints_na(cli, tmp_path):
    sam = tmp_path / "none.sam"
    sam.write_text("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:1000\nr0\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\nr1\t0\tc\t5\t60\t*\t*\t0\t0\t*\t*\n")
    text = stat_text(run(cli, "f1", ["-i", str(sam), "-alnstats", "10"], str(tmp_path / "o"))[1])
    sn = {r[0]: r[1] for r in section(text, "SN")}
    assert (sn["records"], sn["aligned"], sn["primary"]) == ("2", "0", "0")
    assert (sn["read_mean"], sn["read_max"], sn["read_n50"], sn["aligned_mean"], sn["read_bases"]) == ("NA", "NA", "NA", "NA", "0")
    assert len(section(text, "OP")) == 10 and not section(text, "ID") and not section(text, "RL") and not section(text, "AF")
    assert text == AM.Model(1, 1796, -1, 10).add_tuples([(-1, -1, 4, 0, []), (0, 4, 0, 60, [])]).text()


# ---- 2. the goldens: every other output stays as it is ----------------------------------------------------------------------
GOLDENS = {"f1": ("f1.sam", "f1.bam", [[], ["-a"], ["-w", "100"], ["-g", "f1.gff", "-s"], ["-b", "f1.bed4", "-s"]]),
           "f7": ("m.sam", "m.bam", [[], ["-a"], ["-w", "100"], ["-g", "m.gff", "-s"], ["-b", "m.bed4", "-s"]])}
CASES = [(fx, k) for fx in sorted(GOLDENS) for k in range(5)]


@pytest.mark.parametrize("fixture,k", CASES, ids=["%s_%s" % (fx, "_".join(GOLDENS[fx][2][k]).replace("-", "").replace(".", "_") or "chr") for fx, k in CASES])
def test_goldens_every_other_output_stays(cli, fixture, k, tmp_path):
    sam, bam, modes = GOLDENS[fixture]
    mode = modes[k]
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, fixture, sam))
    want = model_text(len(lens), recs, 50)
    for inp in (sam, bam):
        p0, plain = run(cli, fixture, ["-i", inp] + mode, str(tmp_path / ("plain_" + inp)))
        p1, with_it = run(cli, fixture, ["-i", inp, "-alnstats", "50"] + mode, str(tmp_path / ("with_" + inp)))
        assert plain and STAT not in plain and sorted(with_it) == sorted(list(plain) + [STAT])
        assert all(with_it[f] == plain[f] for f in plain) and p0.stdout == p1.stdout
        assert stat_text(with_it) == want, (inp, mode)
    assert "SN\taligned\t0\n" not in want and "SN\trecords\t%d\n" % len(recs) in want


def test_with_the_other_record_options(cli, tmp_path):
    """-readstats, -rowreads, -del and -frag beside it: its numbers stay, and so do theirs"""
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f7", "m.sam"))
    want = model_text(len(lens), recs, 50)
    _, alone = run(cli, "f7", ["-i", "m.bam", "-alnstats", "50"], str(tmp_path / "alone"))
    _, others = run(cli, "f7", ["-i", "m.bam", "-readstats", "300", "-rowreads", "-del", "-frag"], str(tmp_path / "others"))
    _, both = run(cli, "f7", ["-i", "m.bam", "-alnstats", "50", "-readstats", "300", "-rowreads", "-del", "-frag"], str(tmp_path / "both"))
    assert stat_text(alone) == want == stat_text(both) and alone[STAT] == both[STAT]
    assert sorted(both) == sorted(list(others) + [STAT]) and all(both[f] == others[f] for f in others)


def test_option_spellings(cli, tmp_path):
    one = run(cli, "f7", ["-i", "m.sam", "-alnstats", "50"], str(tmp_path / "one"))[1]
    two = run(cli, "f7", ["-i", "m.sam", "--alnstats", "50"], str(tmp_path / "two"))[1]
    assert one == two and STAT in one
    h = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"alnstats" not in h.stdout + h.stderr and b"-a " in h.stdout + h.stderr


# ---- 3. a list: the sum, read_max the maximum --------------------------------------------------------------------------------
def test_a_list_gives_the_sum(cli, edges, tmp_path):
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f1", "f1.sam"))
    lst = tmp_path / "two.list"
    lst.write_text("".join(os.path.join(GOLDEN, "f1", x) + "\n" for x in ("f1.bam", "f1.sam")))
    _, out = run(cli, "f1", ["-i", str(lst), "-alnstats", "50"], str(tmp_path / "sum"))
    assert stat_text(out) == model_text(len(lens), recs, 50, times=2)
    _, plain = run(cli, "f1", ["-i", str(lst)], str(tmp_path / "plain"))
    assert all(out[f] == plain[f] for f in plain) and sorted(out) == sorted(list(plain) + [STAT])
    # read_max is a maximum, not a sum: the edges file twice
    lst2 = tmp_path / "edges.list"
    lst2.write_text((edges["path"] + "\n") * 2)
    m = AM.Model(len(edges["lens"]), 1796, -1, 100).add_parsed(edges["recs"]).add_parsed(edges["recs"])
    text = stat_text(run(cli, "f1", ["-i", str(lst2), "-alnstats", "100"], str(tmp_path / "twice"))[1])
    assert text == m.text() and "SN\tread_max\t%d\n" % m.s[AM.READ_MAX] in text


# ---- 4. the sorted stream that stops early ------------------------------------------------------------------------------------
def test_targets_that_end_before_the_file_does(cli, corpus, tmp_path):
    """BED targets on the first contig only, no index: read_sorted_stream's cursors all run off long before the input ends, and without
    the option it stops reading there.  With it every record is counted all the same, and the table is the one it was."""
    f = corpus
    bed = tmp_path / "early.bed"
    bed.write_text("fa\t100\t900\nfa\t2000\t2500\n")
    assert sum(1 for r in f["model_recs"] if r[0] != 0 or r[1] > 2600) > 1000
    want = model_text(len(f["lens"]), f["model_recs"], 100)
    for inp in (f["sam"], f["path"]):
        _, plain = run(cli, "f1", ["-i", inp, "-b", str(bed)], str(tmp_path / ("plain_" + os.path.basename(inp))))
        _, out = run(cli, "f1", ["-i", inp, "-b", str(bed), "-alnstats", "100"], str(tmp_path / ("with_" + os.path.basename(inp))))
        assert stat_text(out) == want, inp
        assert plain and all(out[k] == plain[k] for k in plain)


# ---- 5. refusals: nothing is written ---------------------------------------------------------------------------------------------
def test_refusals_leave_no_output(cli, tmp_path):
    lists = {}
    for name, lines in (("cram.list", ["m.bam", "m.cram"]), ("paf.list", [os.path.join(GOLDEN, "f6", "p.paf")] * 2)):
        lists[name] = tmp_path / name
        lists[name].write_text("".join((ln if os.path.isabs(ln) else os.path.join(GOLDEN, "f7", ln)) + "\n" for ln in lines))
    unreadable = run(cli, "f7", ["-i", "no_such_file.bam"], str(tmp_path / "missing"), check=False)[0]
    assert unreadable.returncode != 0
    cases = [(["-i", "m.cram"], "m.cram"), (["-i", os.path.join(GOLDEN, "f6", "p.paf")], "p.paf"), (["-i", str(lists["cram.list"])], "m.cram"),
             (["-i", str(lists["paf.list"])], "p.paf"), (["-i", "m.bam", "-g", "m.gff"], "m.bam"), (["-i", "m.bam", "-b", "m.bed4"], "m.bam")]
    for k, (args, what) in enumerate(cases):
        p, files = run(cli, "f7", args + ["-alnstats", "50"], str(tmp_path / ("refused%d" % k)), check=False)
        err = p.stderr.decode()
        assert p.returncode == unreadable.returncode and "-alnstats" in err and what in err and not files, (args, p.returncode, err)
        p, files = run(cli, "f7", args, str(tmp_path / ("read%d" % k)))               # (the same input without the option is read)
        assert files
    p, _ = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-alnstats", "50"], str(tmp_path / "msg"), check=False)
    assert p.stderr.decode().strip() == "Error: -alnstats with -g/-b needs -s (an index fetch reads only the targets' records): m.bam"
    for k, extra in enumerate((["-s"], ["-frag"])):                                    # sequential readings of the same targets are taken
        _, files = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-alnstats", "50"] + extra, str(tmp_path / ("seq%d" % k)))
        assert STAT in files


def test_bad_values_give_the_one_message(cli, tmp_path):
    msg = b"Error: -alnstats should be the width of a length bin, from 1 to 65536"
    for k, bad in enumerate(["0", "65537", "x", "", "-5", "1e3", "12x", "99999999999"]):
        p, files = run(cli, "f7", ["-i", "m.sam", "-alnstats", bad], str(tmp_path / ("bad%d" % k)), check=False)
        assert msg in p.stderr and not files, bad
    os.makedirs(str(tmp_path / "last"))
    p = subprocess.run([cli, "-i", "m.sam", "-o", str(tmp_path / "last" / "o"), "-alnstats"], cwd=os.path.join(GOLDEN, "f7"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert msg in p.stderr and not os.listdir(str(tmp_path / "last"))
    for ok in ("1", "65536"):
        assert STAT in run(cli, "f7", ["-i", "m.sam", "-alnstats", ok], str(tmp_path / ("ok" + ok)))[1]
