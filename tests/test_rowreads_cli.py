"""-rowreads on the CPU: the product's host code on the oracle-backed engine (tests/harness/pandepth_oracle_cli) against the model of
tests/rowreads_model.py.  The harness's engine table ends before the new members, so every input here is counted by the host readers
(read_bam_device gives a BAM back before anything is counted); the device pass has tests/test_rowreads_walk.py (64-lane emulation)
and tests/test_gpu_rowreads.py / tests/test_gpu_rowreads_cli.py.  All comparisons are of exact bytes or text."""
import gzip
import os
import subprocess

import pytest

import frag_model as FM
import rowreads_model as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
STAT = "o.rowreads.stat.gz"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pandepth_amd"), "libpandepth_host.a"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(HERE, "harness"), "pandepth_oracle_cli"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HERE, "harness", "pandepth_oracle_cli")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowreads_cli")
    f = RR.corpus(d)
    f["bed"], f["gff"] = RR.write_regions(d)
    return f


def run(cli, fixture, args, out_dir, check=True):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([cli] + args + ["-o", os.path.join(out_dir, "o"), "-t", "2"], cwd=os.path.join(GOLDEN, fixture),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-500:]
    return p, {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def stat_text(files, name=STAT):
    return gzip.decompress(files[name]).decode()


def table_of(mode_args, f):
    """(the model's row set, uniform w, the header's mode, the run's extra arguments) of a table family"""
    kind = mode_args[0] if mode_args else "chr"
    if kind == "chr":
        return RR.rows_chr(f["lens"]), 0, "chr", []
    if kind == "-w":
        w = int(mode_args[1])
        return RR.rows_windows(f["lens"], w), w, "w", ["-w", str(w)]
    rows = RR.rows_regions(f["names"], f["lens"], RR.REGIONS)
    return (rows, 0, "g", ["-g", f["gff"], "-s"]) if kind == "-g" else (rows, 0, "b", ["-b", f["bed"], "-s"])


def model_text(f, rows, w, mode, flag_mask=1796, min_mapq=-1, times=1):
    m = RR.Model(f["lens"], rows, flag_mask, min_mapq, uniform_w=w)
    for _ in range(times):
        m.add_all(f["model_recs"])
    return m.text(f["names"], mode)


# ---- 1. the corpus, written at run time as SAM and BAM ------------------------------------------------------------------
TABLES = [("chr", []), ("w1000", ["-w", "1000"]), ("w7", ["-w", "7"]), ("w150000", ["-w", "150000"]), ("gff", ["-g"]), ("bed4", ["-b"])]
FILTERS = [("default", [], dict()), ("x0_q20", ["-x", "0", "-q", "20"], dict(flag_mask=0, min_mapq=20))]


@pytest.mark.parametrize("fname,fargs,kw", FILTERS, ids=[v[0] for v in FILTERS])
@pytest.mark.parametrize("tname,targs", TABLES, ids=[t[0] for t in TABLES])
def test_corpus_as_sam_and_bam(cli, corpus, tname, targs, fname, fargs, kw, tmp_path):
    f = corpus
    rows, w, mode, extra = table_of(targs, f)
    want = model_text(f, rows, w, mode, **kw)
    assert want.count("\n") == len(rows) + 1 and len(rows) > 0
    outs = []
    for inp in (f["sam"], f["path"]):
        _, out = run(cli, "f1", ["-i", inp, "-rowreads"] + extra + fargs, str(tmp_path / os.path.basename(inp)))
        assert stat_text(out) == want, inp
        outs.append(out)
    assert outs[0][STAT] == outs[1][STAT]                                         # (the .gz bytes)


CT_INPUTS = ["m.sam", "m.bam", "corpus_inside"]


@pytest.mark.parametrize("args", [[], ["-q", "20"], ["-x", "0"], ["-x", "0", "-q", "20"]], ids=["default", "q20", "x0", "x0_q20"])
@pytest.mark.parametrize("inp", CT_INPUTS, ids=[i.replace(".", "_") for i in CT_INPUTS])
def test_whole_contig_rows_equal_readstats_contig_rows(cli, corpus, inp, args, tmp_path):
    """Records / Kept / MeanMapQ of the whole-contig file equal the CT rows of -readstats in the same run, as the text of the two files.
    The inputs hold no placed record that starts outside its contig (asserted from the SAM text), so a contig's CT row and its row here
    are over the same records: the golden f7 as SAM and BAM, and the corpus's SAM without its pos == -1 and pos >= len lines."""
    fixture = "f7"
    if inp == "corpus_inside":
        names, lens = corpus["names"], corpus["lens"]
        inp = str(tmp_path / "inside.sam")
        with open(inp, "w") as out:
            for ln in open(corpus["sam"]):
                c = ln.split("\t")
                if ln.startswith("@") or c[2] == "*" or 0 <= int(c[3]) - 1 < lens[names.index(c[2])]:
                    out.write(ln)
        names, lens, recs = FM.read_sam(inp)
        assert len(recs) > len(corpus["model_recs"]) - 20
    else:
        names, lens, recs = FM.read_sam(os.path.join(GOLDEN, fixture, "m.sam"))
    assert recs and all(0 <= r[1] < lens[r[0]] for r in recs if r[0] >= 0)
    _, out = run(cli, fixture, ["-i", inp, "-rowreads", "-readstats", "300"] + args, str(tmp_path / "both"))
    ct = {c[1]: c for c in (ln.split("\t") for ln in stat_text(out, "o.reads.stat.gz").splitlines()) if c[0] == "CT"}       # CT contig Length Records Kept MeanMapQ
    rows = [ln.split("\t") for ln in stat_text(out).splitlines()[1:]]                                                      # contig Records Passed MapQ0 Kept Forward MeanMapQ
    assert [r[0] for r in rows] == [n for n, ln in zip(names, lens) if ln >= 2]
    compared = 0
    for r in rows:
        c = ct[r[0]]
        assert (c[3], c[4], c[5]) == (r[1], r[4], r[6]), (r, c)                   # the three fields, byte for byte
        if int(r[4]) > 0:
            assert r[6] != "NA" and "." in r[6]
            compared += 1
    assert compared >= 2                                                           # (contigs with kept records: their MeanMapQ is a number in both files)


def test_window_rows_sum_to_the_contig(cli, corpus, tmp_path):
    f = corpus
    _, chrom = run(cli, "f1", ["-i", f["path"], "-rowreads"], str(tmp_path / "chr"))
    whole = {c[0]: [int(v) for v in c[1:6]] for c in (ln.split("\t") for ln in stat_text(chrom).splitlines()[1:])}
    for w in (7, 1000):
        _, out = run(cli, "f1", ["-i", f["path"], "-rowreads", "-w", str(w)], str(tmp_path / ("w%d" % w)))
        sums = {}
        for c in (ln.split("\t") for ln in stat_text(out).splitlines()[1:]):
            s = sums.setdefault(c[0], [0] * 5)
            for j in range(5):
                s[j] += int(c[3 + j])
        assert all((ln - 1) % w for ln in f["lens"] if ln >= 2)                 # (no contig ends in a window of one base, which the -w table leaves out)
        assert sums == whole, w
    assert sum(v[0] for v in whole.values()) == RR.started(f["lens"], f["model_recs"]) - 3      # (three records start on the one-base contig, which has no row)


# ---- 2. the goldens: every other output stays as it is ----------------------------------------------------------------------
GOLDENS = {"f1": ("f1.sam", "f1.bam", [[], ["-a"], ["-w", "100"], ["-g", "f1.gff", "-s"], ["-b", "f1.bed4", "-s"]]),
           "f7": ("m.sam", "m.bam", [[], ["-a"], ["-w", "100"], ["-g", "m.gff", "-s"], ["-b", "m.bed4", "-s"]])}
CASES = [(fx, k) for fx in sorted(GOLDENS) for k in range(5)]
COMMITTED = {("f1", 0): "chr", ("f1", 1): "chr_a", ("f1", 2): "w100", ("f1", 4): "bed4_s", ("f7", 0): "chr"}      # tests/golden/<fixture>/expected/<case>.*


@pytest.mark.parametrize("fixture,k", CASES, ids=["%s_%s" % (fx, "_".join(GOLDENS[fx][2][k]).replace("-", "").replace(".", "_") or "chr") for fx, k in CASES])
def test_goldens_every_other_output_stays(cli, fixture, k, tmp_path):
    sam, bam, modes = GOLDENS[fixture]
    mode = modes[k]
    names, lens, recs = FM.read_sam(os.path.join(GOLDEN, fixture, sam))
    texts = []
    for inp in (sam, bam):
        p0, plain = run(cli, fixture, ["-i", inp] + mode, str(tmp_path / ("plain_" + inp)))
        p1, with_it = run(cli, fixture, ["-i", inp, "-rowreads"] + mode, str(tmp_path / ("with_" + inp)))
        assert plain and STAT not in plain and sorted(with_it) == sorted(list(plain) + [STAT])
        assert all(with_it[f] == plain[f] for f in plain) and p0.stdout == p1.stdout
        texts.append(stat_text(with_it))
        if inp == bam and (fixture, k) in COMMITTED:                                        # the committed goldens of the other outputs, where this mode has one
            for name in plain:
                gold = os.path.join(GOLDEN, fixture, "expected", COMMITTED[(fixture, k)] + name[1:])
                assert open(gold, "rb").read() == with_it[name], name
    assert texts[0] == texts[1]
    if mode in ([], ["-a"], ["-w", "100"]):                                                 # (the rows of these tables need no region file to model)
        rows, w = (RR.rows_windows(lens, 100), 100) if mode == ["-w", "100"] else (RR.rows_chr(lens), 0)
        m = RR.Model(lens, rows, 1796, -1, uniform_w=w).add_all(recs)
        assert texts[0] == m.text(names, "w" if w else "chr") and m.counts[:, RR.RECORDS].sum() > 0
    else:
        body = [ln.split("\t") for ln in texts[0].splitlines()[1:]]
        assert body and sum(int(c[4]) for c in body) > 0


def test_option_spellings(cli, tmp_path):
    one = run(cli, "f7", ["-i", "m.sam", "-rowreads"], str(tmp_path / "one"))[1]
    two = run(cli, "f7", ["-i", "m.sam", "--rowreads"], str(tmp_path / "two"))[1]
    assert one == two and STAT in one
    assert stat_text(one).startswith("#Chr\tRecords\tPassed\tMapQ0\tKept\tForward\tMeanMapQ\n")
    h = subprocess.run([cli, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"rowreads" not in h.stdout + h.stderr and b"-a " in h.stdout + h.stderr


# ---- 3. a list: the sum -----------------------------------------------------------------------------------------------------
def test_a_list_gives_the_sum(cli, corpus, tmp_path):
    f = corpus
    lst = tmp_path / "two.list"
    lst.write_text(f["path"] + "\n" + f["sam"] + "\n")
    for k, targs in enumerate(([], ["-w", "1000"], ["-b"])):
        rows, w, mode, extra = table_of(targs, f)
        _, out = run(cli, "f1", ["-i", str(lst), "-rowreads"] + extra, str(tmp_path / ("sum%d" % k)))
        assert stat_text(out) == model_text(f, rows, w, mode, times=2)
        _, plain = run(cli, "f1", ["-i", str(lst)] + extra, str(tmp_path / ("plain%d" % k)))
        assert all(out[n] == plain[n] for n in plain) and sorted(out) == sorted(list(plain) + [STAT])


# ---- 4. the sorted stream that stops early ------------------------------------------------------------------------------------
def test_targets_that_end_before_the_file_does(cli, corpus, tmp_path):
    """BED targets on the first contig only, no index: read_sorted_stream's cursors all run off long before the input ends, and without
    the option it stops reading there.  With it every record is read all the same — the rows are the targets', so what shows is that the
    table and the rows are right and, with -readstats beside it, that the whole file was counted."""
    f = corpus
    bed = tmp_path / "early.bed"
    bed.write_text("fa\t100\t900\tearly_a\nfa\t2000\t2500\tearly_b\n")
    regions = [("fa", 100, 900, "early_a"), ("fa", 2000, 2500, "early_b")]
    rows = RR.rows_regions(f["names"], f["lens"], regions)
    want = RR.Model(f["lens"], rows).add_all(f["model_recs"]).text(f["names"], "b")
    assert sum(1 for r in f["model_recs"] if r[0] != 0 or r[1] > 2600) > 1000
    for inp in (f["sam"], f["path"]):
        _, plain = run(cli, "f1", ["-i", inp, "-b", str(bed)], str(tmp_path / ("plain_" + os.path.basename(inp))))
        _, out = run(cli, "f1", ["-i", inp, "-b", str(bed), "-rowreads"], str(tmp_path / ("with_" + os.path.basename(inp))))
        assert stat_text(out) == want, inp
        assert plain and all(out[k] == plain[k] for k in plain)
        _, both = run(cli, "f1", ["-i", inp, "-b", str(bed), "-rowreads", "-readstats", "300"], str(tmp_path / ("both_" + os.path.basename(inp))))
        assert both[STAT] == out[STAT] and "SN\trecords\t%d\n" % len(f["model_recs"]) in stat_text(both, "o.reads.stat.gz")


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
        p, files = run(cli, "f7", args + ["-rowreads"], str(tmp_path / ("refused%d" % k)), check=False)
        err = p.stderr.decode()
        assert p.returncode == unreadable.returncode and "-rowreads" in err and what in err and not files, (args, p.returncode, err)
        p, files = run(cli, "f7", args, str(tmp_path / ("read%d" % k)))               # (the same input without the option is read)
        assert files
    p, _ = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-rowreads"], str(tmp_path / "msg"), check=False)
    assert p.stderr.decode().strip() == "Error: -rowreads with -g/-b needs -s (an index fetch reads only the targets' records): m.bam"
    for k, extra in enumerate((["-s"], ["-frag"])):                                    # sequential readings of the same targets are taken
        _, files = run(cli, "f7", ["-i", "m.bam", "-g", "m.gff", "-rowreads"] + extra, str(tmp_path / ("seq%d" % k)))
        assert STAT in files


def test_bad_usage(cli, tmp_path):
    p, files = run(cli, "f7", ["-i", "m.sam", "-rowreads", "5"], str(tmp_path / "value"), check=False)
    assert b"Command option error" in p.stderr and not files
    p, files = run(cli, "f7", ["-i", "m.sam", "-rowreads", "-rowreads"], str(tmp_path / "twice"), check=False)
    assert b"Error: -rowreads takes no value and is given once" in p.stderr and not files
    p, files = run(cli, "f7", ["-i", "m.sam", "-rowreads", "--rowreads"], str(tmp_path / "twice2"), check=False)
    assert b"Error: -rowreads takes no value and is given once" in p.stderr and not files
    assert STAT in run(cli, "f7", ["-i", "m.sam", "-rowreads"], str(tmp_path / "ok"))[1]
