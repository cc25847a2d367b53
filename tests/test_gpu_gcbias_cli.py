"""-gcbias W on the MI355X: the `pandepth` executable on the golden fixtures f5 and f7 in the four modes.  The file binned on the
device (pd_depth_gc_bias) is the file tests/gcbias_model.py writes from the CPU oracle's depth, and the file the host fallback
writes (-X gcbias_device=0); the other outputs are those of the run without the option.  A crafted input as BAM (decoded on the
device) and as SAM (decoded on the host) gives one file."""
import gzip
import os
import re
import subprocess

import pytest

import bam_craft as B
import gcbias_model as M
from test_gcbias_cli import CONTIGS, CW, F5, F7, FASTA, IDS, READS, model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "pandepth_amd", "pandepth")

CASES = [(F5, ["-i", "c.bam", "-r", "c.fa"], 7), (F5, ["-i", "c.bam", "-r", "c.fa.gz", "-w", "100"], 7), (F5, ["-i", "c.bam", "-r", "c.fa", "-w", "200"], 1),
         (F5, ["-i", "c.bam", "-r", "c.fa", "-g", "c.gff"], 7), (F5, ["-i", "c.bam", "-r", "c.fa", "-b", "c.bed4"], 7), (F5, ["-i", "c.list", "-r", "c.fa"], 3),
         (F7, ["-i", "m.cram", "-r", "m.fa"], 100), (F7, ["-i", "m.cram", "-r", "m.fa", "-w", "100"], 100), (F7, ["-i", "m.bam", "-r", "m.fa", "-w", "200"], 1000),
         (F7, ["-i", "m.cram", "-r", "m.fa", "-g", "m.gff"], 7), (F7, ["-i", "m.bam", "-r", "m.fa", "-b", "m.bed4"], 7)]


def run(cwd, args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    p = subprocess.run([CLI] + args + ["-o", os.path.join(out_dir, "o"), "-t", "4"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    return {f: gzip.decompress(open(os.path.join(out_dir, f), "rb").read()).decode() for f in os.listdir(out_dir)}


@pytest.mark.parametrize("cwd,args,W", CASES, ids=["%s_W%d" % (IDS(a[1:2] + a[3:]), w) for _, a, w in CASES])
def test_device_file_equals_model_and_host_file(cwd, args, W, tmp_path):
    assert os.access(CLI, os.X_OK), "pandepth binary not built (make -C pandepth_amd)"
    plain = run(cwd, args, str(tmp_path / "plain"))
    dev = run(cwd, args + ["-gcbias", str(W)], str(tmp_path / "dev"))
    host = run(cwd, args + ["-gcbias", str(W), "-X", "gcbias_device=0"], str(tmp_path / "host"))
    small = run(cwd, args + ["-gcbias", str(W), "-X", "gcbias_piece_cells=%d,gcbias_wave_max=%d" % (3 * W + 1, 0 if W < 100 else 2 ** 20)], str(tmp_path / "small"))
    assert sorted(dev) == sorted(list(plain) + ["o.gcbias.stat.gz"])
    assert {f: dev[f] for f in plain} == plain                                  # nothing else changes
    (win, tot, skipped), _ = model(cwd, args, W)
    assert int((win > 0).sum()) >= 2, "windows in fewer than two bins check nothing"
    assert dev["o.gcbias.stat.gz"] == M.text(W, win, tot, skipped)
    assert host["o.gcbias.stat.gz"] == dev["o.gcbias.stat.gz"] == small["o.gcbias.stat.gz"]


def test_device_decode_and_host_decode_give_one_file(tmp_path):
    """the crafted contigs of test_gcbias_cli.py as a BAM, whose records the device decodes, and as the SAM the host parses"""
    names, lens = [c[0] for c in CONTIGS], [c[1] for c in CONTIGS]
    tid = {n: k for k, n in enumerate(names)}
    recs = [(tid[n], pos - 1, 0, 60, b"r%d" % k, [(("MIDNSHP=X".index(op)), int(ln)) for ln, op in re.findall(r"(\d+)([MIDNSHP=X])", cig)], 0, b"")
            for k, (n, pos, cig) in enumerate(READS)]
    recs = [r[:6] + (B.qlen(r[5]),) + r[7:] for r in recs]
    B.write_bam(str(tmp_path / "x.bam"), names, lens, recs)
    sam = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    sam += "".join("r%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % (k, n, pos, cig) for k, (n, pos, cig) in enumerate(READS))
    (tmp_path / "x.sam").write_text(sam)
    (tmp_path / "x.fa").write_text(FASTA)
    bam = run(str(tmp_path), ["-i", "x.bam", "-r", "x.fa", "-gcbias", str(CW)], str(tmp_path / "bam"))
    sam_out = run(str(tmp_path), ["-i", "x.sam", "-r", "x.fa", "-gcbias", str(CW)], str(tmp_path / "sam"))
    (win, tot, skipped), _ = model(str(tmp_path), ["-i", "x.sam", "-r", "x.fa"], CW)
    assert win[50] == 9 and win[100] == 6 and win[88] == 1 and win[0] == 4 and skipped == 10          # (test_gcbias_cli.py: test_crafted_contigs)
    assert bam["o.gcbias.stat.gz"] == sam_out["o.gcbias.stat.gz"] == M.text(CW, win, tot, skipped)
    assert bam["o.chr.stat.gz"] == sam_out["o.chr.stat.gz"]
