"""-readstats on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli) against the model of
tests/recstats_model.py.  The harness's engine table ends before the new member, so every input here is counted by the host readers
(read_bam_device gives a BAM back before anything is counted); the device pass has tests/test_recstats_walk.py (64-lane emulation)
and tests/test_gpu_recstats.py / tests/test_gpu_recstats_cli.py.  All comparisons are of exact bytes or text."""
import gzip
import os
import subprocess

import pytest

import frag_model as FM
import recstats_model as RM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
STAT = "o.reads.stat.gz"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return RM.corpus(tmp_path_factory.mktemp("recstats_cli"))


def run(cli, fixture, args, out_dir, check=True):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([cli] + args + ["-o", os.path.join(out_dir, "o"), "-t", "2"], cwd=os.path.join(GOLDEN, fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-500:]
    return p, {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def stat_text(files):
    return gzip.decompress(files[STAT]).decode()


def model_text(names, lens, recs, n, flag_mask=1796, min_mapq=-1, times=1):
    m = RM.Model(names, lens, flag_mask, min_mapq, n)
    for _ in range(times):
        m.add_all(recs)
    return m.text()


# ---- 1. the corpus, written at run time as SAM and BAM ------------------------------------------------------------------
VARIANTS = [("default", [], dict()), ("q20", ["-q", "20"], dict(min_mapq=20)), ("x0", ["-x", "0"], dict(flag_mask=0)),
            ("x0_q20", ["-x", "0", "-q", "20"], dict(flag_mask=0, min_mapq=20))]


@pytest.mark.parametrize("n", RM.BINS)
@pytest.mark.parametrize("name,args,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_corpus_as_sam_and_bam(cli, corpus, name, args, kw, n, tmp_path):
    f = corpus
    want = model_text(f["names"], f["lens"], f["model_recs"], n, **kw)
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f1", ["-i", inp, "-readstats", str(n)] + args, str(tmp_path / os.path.basename(inp)))
        assert stat_text(out) == want, inp
        outs.append(out)
    assert outs[0][STAT] == outs[1][STAT]                                         # (the .gz bytes)


def test_the_filters_move_the_classes(cli, corpus, tmp_path):
    """the SN and MQ lines the executable writes: -x 0 empties dropped_flag and widens the MQ rows, -q 20 fills dropped_mapq and leaves the MQ rows alone"""
    f = corpus
    sn, mq = {}, {}
    for name, args, _ in VARIANTS:
        lines = stat_text(run(cli, "f1", ["-i", f["sam"], "-readstats", "1000"] + args, str(tmp_path / name))[1]).splitlines()
        sn[name] = {ln.split("\t")[1]: ln.split("\t")[2] for ln in lines if ln.startswith("SN\t")}
        mq[name] = sum(int(ln.split("\t")[2]) for ln in lines if ln.startswith("MQ\t"))
    n = {k: {c: int(v[c]) for c in ("records", "unplaced", "dropped_flag", "dropped_mapq", "kept")} for k, v in sn.items()}
    assert n["default"]["dropped_flag"] > 0 == n["x0"]["dropped_flag"] and n["q20"]["dropped_mapq"] > 0 == n["default"]["dropped_mapq"]
    assert n["x0"]["kept"] > n["default"]["kept"] > n["q20"]["kept"] and len({v["records"] for v in n.values()}) == 1 == len({v["unplaced"] for v in n.values()})
    assert all(v["records"] == v["unplaced"] + v["dropped_flag"] + v["dropped_mapq"] + v["kept"] for v in n.values())
    assert mq["x0_q20"] == mq["x0"] > mq["q20"] == mq["default"]
    assert (sn["x0_q20"]["flag_mask"], sn["x0_q20"]["min_mapq"], sn["default"]["flag_mask"], sn["default"]["min_mapq"]) == ("0", "20", "1796", "-1")


# ---- 2. the goldens: every other output stays as it is ----------------------------------------------------------------------
GOLDENS = {"f1": ("f1.sam", "f1.bam", [[], ["-a"], ["-w", "100"], ["-g", "f1.gff", "-s"], ["-b", "f1.bed4", "-s"]]),
           "f7": ("m.sam", "m.bam", [[], ["-a"], ["-w", "100"], ["-g", "m.gff", "-s"], ["-b", "m.bed4", "-s"]])}
CASES = [(fx, k) for fx in sorted(GOLDENS) for k in range(5)]


@pytest.mark.parametrize("fixture,k", CASES, ids=["%s_%s" % (fx, "_".join(GOLDENS[fx][2][k]).replace("-", "").replace(".", "_") or "chr") for fx, k in CASES])
def test_goldens_every_other_output_stays(cli, fixture, k, tmp_path):
    sam, bam, modes = GOLDENS[fixture]
    mode = modes[k]
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, fixture, sam))
    want = model_text(names, lens, recs, 300)
    for inp in (sam, bam):
        p0, plain = run(cli, fixture, ["-i", inp] + mode, str(tmp_path / ("plain_" + inp)))
        p1, with_it = run(cli, fixture, ["-i", inp, "-readstats", "300"] + mode, str(tmp_path / ("with_" + inp)))
        assert plain and STAT not in plain and sorted(with_it) == sorted(list(plain) + [STAT])
        assert all(with_it[f] == plain[f] for f in plain) and p0.stdout == p1.stdout
        assert stat_text(with_it) == want, (inp, mode)
    assert "SN\tkept\t0\n" not in want and "SN\trecords\t%d\n" % len(recs) in want


def test_option_spellings(cli, tmp_path):
    one = run(cli, "f7", ["-i", "m.sam", "-readstats", "300"], str(tmp_path / "one"))[1]
    two = run(cli, "f7", ["-i", "m.sam", "--readstats", "300"], str(tmp_path / "two"))[1]
    assert one == two and STAT in one
    assert "IS\t" in stat_text(one) and "SN\tinsert_median\tNA" not in stat_text(one)       # (f7 has pairs with mate fields)
    h = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"readstats" not in h.stdout + h.stderr and b"-a " in h.stdout + h.stderr


# ---- 3. a list: the sum -----------------------------------------------------------------------------------------------------
def test_a_list_gives_the_sum(cli, tmp_path):
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, "f1", "f1.sam"))
    lst = tmp_path / "two.list"
    lst.write_text("".join(os.path.join(GOLDEN, "f1", x) + "\n" for x in ("f1.bam", "f1.sam")))
    _, out = run(cli, "f1", ["-i", str(lst), "-readstats", "300"], str(tmp_path / "sum"))
    assert stat_text(out) == model_text(names, lens, recs, 300, times=2)
    _, plain = run(cli, "f1", ["-i", str(lst)], str(tmp_path / "plain"))
    assert all(out[f] == plain[f] for f in plain) and sorted(out) == sorted(list(plain) + [STAT])


# ---- 4. the sorted stream that stops early ------------------------------------------------------------------------------------
def test_targets_that_end_before_the_file_does(cli, corpus, tmp_path):
    """BED targets on the first contig only, no index: read_sorted_stream's cursors all run off long before the input ends, and without
    the option it stops reading there.  With it every record is counted all the same, and the table is the one it was."""
    f = corpus
    bed = tmp_path / "early.bed"
    bed.write_text("fa\t100\t900\nfa\t2000\t2500\n")
    assert sum(1 for r in f["model_recs"] if r[0] != 0 or r[1] > 2600) > 1000
    want = model_text(f["names"], f["lens"], f["model_recs"], 1000)
    for inp in (f["sam"], f["path"]):
        _, plain = run(cli, "f1", ["-i", inp, "-b", str(bed)], str(tmp_path / ("plain_" + os.path.basename(inp))))
        _, out = run(cli, "f1", ["-i", inp, "-b", str(bed), "-readstats", "1000"], str(tmp_path / ("with_" + os.path.basename(inp))))
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
        p, files = run(cli, "f7", args + ["-readstats", "300"], str(tmp_path / ("refused%d" % k)), check=False)
        err = p.stderr.decode()
        assert p.returncode == unreadable.returncode and "-readstats" in err and what in err and not files, (args, p.returncode, err)
        p, files = run(cli, "f7", args, str(tmp_path / ("read%d" % k)))               # (the same input without the option is read)
        assert files
    p, _ = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-readstats", "300"], str(tmp_path / "msg"), check=False)
    assert p.stderr.decode().strip() == "Error: -readstats with -g/-b needs -s (an index fetch reads only the targets' records): m.bam"
    for k, extra in enumerate((["-s"], ["-frag"])):                                    # sequential readings of the same targets are taken
        _, files = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-readstats", "300"] + extra, str(tmp_path / ("seq%d" % k)))
        assert STAT in files


def test_bad_values_give_the_one_message(cli, tmp_path):
    msg = b"Error: -readstats should be the number of insert-size bins, from 1 to 65536"
    for k, bad in enumerate(["0", "65537", "x", "", "-5", "1e3", "12x", "99999999999"]):
        p, files = run(cli, "f7", ["-i", "m.sam", "-readstats", bad], str(tmp_path / ("bad%d" % k)), check=False)
        assert msg in p.stderr and not files, bad
    os.makedirs(str(tmp_path / "last"))
    p = subprocess.run([cli, "-i", "m.sam", "-o", str(tmp_path / "last" / "o"), "-readstats"], cwd=os.path.join(GOLDEN, "f7"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert msg in p.stderr and not os.listdir(str(tmp_path / "last"))
    for ok in ("1", "65536"):
        assert STAT in run(cli, "f7", ["-i", "m.sam", "-readstats", ok], str(tmp_path / ("ok" + ok)))[1]
