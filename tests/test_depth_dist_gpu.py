"""GPU parity tests of the depth distribution (pd_scan_depth_histogram / pd_depth_histogram, the -dist table): the HIP
histogram kernels against numpy.bincount of the CPU oracle's depth (oracle/pd_oracle.c), exact for every bin."""
import numpy as np
import pytest

import pd_oracle as O
import pandepth_amd as pda

pytestmark = pytest.mark.gpu

PD_EINVAL, PD_ESTATE = -1, -4           # include/pandepth_amd.h

LENS = [700001, 250000, 50001, 1, 8192, 8191, 16384, 3, 100000]
N_BINS = [2, 3, 64, 4097]


def rand_intervals(rng, lens, n, max_len=300):
    tid = rng.integers(0, len(lens), n).astype(np.int32)
    L = np.asarray(lens, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L + 40)).astype(np.int64) - 5
    end = beg + rng.integers(0, max_len, n)
    return np.stack([tid, beg.astype(np.int32), end.astype(np.int32)], axis=1).astype(np.int32)


def sort_iv(iv):
    return iv[np.lexsort((iv[:, 1], iv[:, 0]))]


def clip(iv, lens):
    L = np.asarray(lens, dtype=np.int64)[iv[:, 0]]
    out = iv.copy()
    out[:, 1] = np.clip(iv[:, 1], 0, L)
    out[:, 2] = np.clip(iv[:, 2], 0, L)
    return out[out[:, 1] < out[:, 2]]


def oracle_depth(lens, iv, wrap18):
    return O.depth_from_intervals(lens, clip(iv, lens), wrap18)


def hist_ref(lens, d, off, n_bins, regs=None):
    """(n_contigs, n_bins) uint64: whole contigs, or the cells [first-1, second) of the regions (clipped to the contig)"""
    h = np.zeros((len(lens), n_bins), dtype=np.uint64)
    spans = [(t, 0, ln) for t, ln in enumerate(lens)] if regs is None else \
        [(int(t), max(int(f) - 1, 0), min(int(s), lens[int(t)])) for t, f, s in regs]
    for t, b, e in spans:
        if b < e:
            x = d[off[t] + b:off[t] + e]
            h[t] += np.bincount(np.minimum(x, n_bins - 1), minlength=n_bins).astype(np.uint64)
    return h


def sample(seed, pile=True):
    """random runs on LENS plus a 300 000-read pile in contig 0 (depth above 2^18: wraps in 18-bit cells)"""
    rng = np.random.default_rng(seed)
    iv = rand_intervals(rng, LENS, 120000)
    if pile:
        iv = np.concatenate([iv, np.tile(np.array([[0, 20000, 20100]], dtype=np.int32), (300000, 1)),
                             np.tile(np.array([[1, 8180, 8300]], dtype=np.int32), (500, 1))])
    return iv


@pytest.mark.parametrize("wrap", [0, 18])
def test_fused_and_scanned_equal_oracle(wrap):
    iv = sample(11 + wrap)
    d, off = oracle_depth(LENS, iv, wrap == 18)
    with pda.Engine(LENS) as e:
        e.push_intervals(iv, pda.PD_PUSH_DEFAULT)
        fused = {}
        for nb in N_BINS:
            fused[nb] = e.scan_depth_histogram(nb, wrap)
            assert fused[nb].shape == (len(LENS), nb) and fused[nb].dtype == np.uint64
            assert np.array_equal(fused[nb], hist_ref(LENS, d, off, nb)), nb
        # the fused call leaves the context accumulating: the window statistics and pd_scan still see the same sample
        woff, cover, tot = e.scan_reduce_windows(10000, 1, wrap)
        assert int(tot.sum()) == int(d.astype(np.uint64).sum())
        e.scan(wrap)
        for nb in N_BINS:
            assert np.array_equal(e.depth_histogram(nb), fused[nb]), nb
        # the piles land in the last bin for every n_bins below their depth
        assert fused[64][0, 63] >= 100 and fused[2][1, 1] >= 120


def test_sorted_batches_and_repeat_calls_are_bit_identical():
    rng = np.random.default_rng(5)
    iv = sort_iv(clip(rand_intervals(rng, LENS, 200000), LENS))
    d, off = oracle_depth(LENS, iv, False)
    ref = hist_ref(LENS, d, off, 257)
    with pda.Engine(LENS) as e:
        e.push_intervals(iv, pda.PD_PUSH_SORTED)
        a = e.scan_depth_histogram(257)
        b = e.scan_depth_histogram(257)
        assert np.array_equal(a, ref) and np.array_equal(b, ref)
        e.scan(0)
        assert np.array_equal(e.depth_histogram(257), ref)
        assert np.array_equal(e.depth_histogram(257), ref)


def _split_streams(rng, lens, n, max_len=300):
    """the sorted first-run stream and a nearly sorted second-run stream (test_gpu_engine's direct-window samples)"""
    first = sort_iv(rand_intervals(rng, lens, n, max_len=max_len))
    k = rng.random(first.shape[0]) < 0.2
    gap = rng.integers(1, 400, int(k.sum())).astype(np.int32)
    other = first[k].copy()
    other[:, 1] = first[k][:, 2] + gap
    other[:, 2] = other[:, 1] + rng.integers(1, max_len, other.shape[0]).astype(np.int32)
    return first, other


def windows_ref(lens, d, off, w, min_dep):
    cov, tot = [], []
    for t, ln in enumerate(lens):
        x = d[off[t]:off[t] + ln].astype(np.uint64)
        for s in range(0, ln, w):
            seg = x[s:min(s + w, ln)]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


@pytest.mark.parametrize("wrap", [0, 18])
@pytest.mark.parametrize("before", [False, True])
def test_deferred_sample(wrap, before):
    """pd_keep_deferred: the histogram materialises the deferred sample; the window calls before and after agree with the oracle"""
    rng = np.random.default_rng(300 + wrap)
    first, other = _split_streams(rng, LENS, 80000)
    pile = np.tile(np.array([[0, 8190, 8200]], dtype=np.int32), (1000, 1))
    first = sort_iv(np.concatenate([first, pile]))
    d, off = oracle_depth(LENS, np.concatenate([first, other]), wrap == 18)
    cov_ref, tot_ref = windows_ref(LENS, d, off, 10000, 1)
    with pda.Engine(LENS) as e:
        e.keep_deferred(True)
        e.push_intervals(first, pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE)
        e.push_intervals(other, pda.PD_PUSH_SORTED | pda.PD_PUSH_MORE | pda.PD_PUSH_DISORDER(800))
        if before:                                   # the direct window path READS the sample; it stays deferred
            _, cover, tot = e.scan_reduce_windows(10000, 1, wrap)
            assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref)
        h = e.scan_depth_histogram(64, wrap)
        assert np.array_equal(h, hist_ref(LENS, d, off, 64))
        _, cover, tot = e.scan_reduce_windows(10000, 1, wrap)
        assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref)
        assert np.array_equal(e.scan_depth_histogram(64, wrap), h)
        e.scan(wrap)
        for t in (0, 1, len(LENS) - 1):
            assert np.array_equal(e.read_depth(t, 0, LENS[t]), d[off[t]:off[t] + LENS[t]]), t


REGIONS = np.array([
    [0, 1, 100], [0, 101, 8200],                     # touching but disjoint, the second across a tile edge
    [0, 8300, 8300], [0, 8302, 8302],                # single cells
    [0, 16380, 40000],                               # longer than one piece, across several tile edges
    [0, 40001, 40001],                               # touches the one before
    [1, 8190, 8195], [1, 200000, 250000],            # across a tile edge; ends at the contig's end
    [2, 50001, 50001],                               # the contig's last cell
    [3, 1, 1],                                       # a contig of one cell
    [5, 8000, 9000],                                 # past the end of an 8191-cell contig: clipped
    [7, 1, 3],
    [8, 5, 4],                                       # empty (no cells)
    [8, 10, 99990],
], dtype=np.int32)


@pytest.mark.parametrize("nb", N_BINS)
def test_regions_equal_oracle(nb):
    iv = sample(23)
    d, off = oracle_depth(LENS, iv, True)
    with pda.Engine(LENS) as e:
        e.push_intervals(iv, pda.PD_PUSH_DEFAULT)
        e.scan(18)
        got = e.depth_histogram(nb, REGIONS)
        assert np.array_equal(got, hist_ref(LENS, d, off, nb, REGIONS))
        # one region per contig over the whole contig = the whole-contig call
        whole = np.array([[t, 1, ln] for t, ln in enumerate(LENS)], dtype=np.int32)
        assert np.array_equal(e.depth_histogram(nb, whole), e.depth_histogram(nb))


def test_errors():
    iv = sample(3, pile=False)
    with pda.Engine(LENS) as e:
        e.push_intervals(iv)
        for nb in (0, 1, 4098):
            with pytest.raises(pda.PdError) as x:
                e.scan_depth_histogram(nb)
            assert x.value.code == PD_EINVAL
        with pytest.raises(pda.PdError) as x:              # before pd_scan
            e.depth_histogram(16)
        assert x.value.code == PD_ESTATE
        e.scan(0)
        with pytest.raises(pda.PdError) as x:              # after pd_scan
            e.scan_depth_histogram(16)
        assert x.value.code == PD_ESTATE
        for nb in (1, 4098):
            with pytest.raises(pda.PdError) as x:
                e.depth_histogram(nb)
            assert x.value.code == PD_EINVAL
        bad = [
            [[1, 1, 10], [0, 1, 10]],                      # contigs out of order
            [[0, 50, 60], [0, 10, 20]],                    # starts out of order
            [[0, 10, 20], [0, 20, 30]],                    # overlap by one cell
            [[0, 10, 100], [0, 20, 30]],                   # contained
            [[len(LENS), 1, 10]],                          # contig id out of range
        ]
        for r in bad:
            with pytest.raises(pda.PdError) as x:
                e.depth_histogram(16, np.array(r, dtype=np.int32))
            assert x.value.code == PD_EINVAL, r
        assert e.depth_histogram(16).sum() == sum(LENS)    # the context is still usable


def test_empty_context():
    with pda.Engine(LENS) as e:
        for nb in (2, 4097):
            h = e.scan_depth_histogram(nb)
            assert np.array_equal(h[:, 0], np.array(LENS, dtype=np.uint64)) and int(h[:, 1:].sum()) == 0
        e.scan(0)
        h = e.depth_histogram(300)
        assert np.array_equal(h[:, 0], np.array(LENS, dtype=np.uint64)) and int(h[:, 1:].sum()) == 0


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_lds_variants_agree(variant):
    """the measured LDS forms of the kernels (per-wave / per-workgroup counters, folded or not) give the same bits"""
    iv = sample(41)
    d, off = oracle_depth(LENS, iv, False)
    with pda.Engine(LENS) as e:
        e.set_param("hist_variant", variant)
        e.push_intervals(iv)
        assert np.array_equal(e.scan_depth_histogram(101), hist_ref(LENS, d, off, 101))
        e.scan(0)
        assert np.array_equal(e.depth_histogram(101), hist_ref(LENS, d, off, 101))
        assert np.array_equal(e.depth_histogram(101, REGIONS), hist_ref(LENS, d, off, 101, REGIONS))


def test_multi_tile_flush_50mb_30x():
    """one 50 Mb contig at ~30x (tools/synth.py, seeded) and a short one behind it: every workgroup covers a run of tiles
    and flushes its bins once per contig"""
    import torch
    from tools import synth
    lens = [50_000_000, 12345]
    dev = torch.device("cuda", 0)
    first, other = synth.gen_runs_torch(lens, 10_000_000, dev, seed=7)
    f, o = first.cpu().numpy(), other.cpu().numpy()
    d, off = O.depth_from_intervals(lens, np.concatenate([f, o]))
    for nb in (64, 4097):
        ref = hist_ref(lens, d, off, nb)
        with pda.Engine(np.array(lens, dtype=np.uint32)) as e:
            e.push_intervals_device(first.data_ptr(), f.shape[0], pda.PD_PUSH_SORTED)
            e.push_intervals_device(other.data_ptr(), o.shape[0], pda.PD_PUSH_SORTED | pda.PD_PUSH_DISORDER(synth.MAX_SPAN))
            h = e.scan_depth_histogram(nb)
            assert np.array_equal(h, ref), nb
            e.scan(0)
            assert np.array_equal(e.depth_histogram(nb), ref), nb
            regs = np.array([[0, 1 + k, k + 3_000_000] for k in range(0, 50_000_000, 5_000_000)], dtype=np.int32)
            assert np.array_equal(e.depth_histogram(nb, regs), hist_ref(lens, d, off, nb, regs)), nb
    assert int(ref[0, 20:40].sum()) > 10_000_000            # the sample really sits around 30x
