"""A compact sample keeps its runs as two planes of 32-bit words — lo = (begin & 0xFFFF) | (length << 16), hi = the two high halves — and
the direct kernels (k_direct_c8, statistics and export forms, and the compact branch of the int-window kernel) read lo alone, with 16-bit
arithmetic relative to the tile.  Here: the places where 16 bits wrap (the tiles whose first flat cell is 57344, 65536 and 131072), for
buckets of 512 and of 4096 cells (the widest pd_set_param("lmax") accepts), through every "direct_un" code; and runs whose begin or length needs the hi plane, through the paths
that put a whole run together again.  Own contig tables, a numpy difference array as the oracle."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda

gpu = pytest.mark.gpu

TILE = 8192
LENS = [17 * TILE + 100, 3 * TILE]                       # contig 0: tiles 0 .. 17 (flat = local), contig 1 behind it
SEAM_TILES = (7, 8, 16)                                  # first flat cells 57344 (p0 + TILE = 2^16), 65536 and 131072 (p0 = 0 mod 2^16)
WS = (8192, 10000)
MODES = tuple((md, wrap) for md in (0, 1, 3) for wrap in (0, 18))
# every code pd_set_param("direct_un") selects a k_direct_c8 instantiation with (anything else: the default's)
UN_CODES = (0, 502, 504, 508, 602, 604, 702, 802, 804, 801, 708, 803, 703, 704, 1803, 1703, 1704, 1802, 1708,
            5704, 5702, 5802, 5706, 5708, 5608, 9704, 9708, 9608)


def oracle_depth(lens, iv):
    """per-contig depth of runs clipped to their contig (difference array)"""
    out = []
    iv = iv.astype(np.int64)
    for t, ln in enumerate(lens):
        x = iv[iv[:, 0] == t]
        b, e = np.clip(x[:, 1], 0, ln), np.clip(x[:, 2], 0, ln)
        ok = b < e
        diff = np.zeros(ln + 1, dtype=np.int64)
        np.add.at(diff, b[ok], 1)
        np.subtract.at(diff, e[ok], 1)
        out.append(np.cumsum(diff[:ln]))
    return out


def oracle_windows(depth, w, min_dep, wrap):
    cov, tot = [], []
    for d in depth:
        x = (d & ((1 << wrap) - 1) if wrap else d).astype(np.uint64)
        for s in range(0, x.size, w):
            seg = x[s:s + w]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


def sort_iv(iv):
    return iv[np.lexsort((iv[:, 1], iv[:, 0]))]


@functools.lru_cache(maxsize=None)
def seam_sample(bucket):
    """(sorted, other, depth) for buckets of `bucket` cells: no run is longer than a bucket"""
    rng = np.random.default_rng(bucket)
    seams = []
    for T in SEAM_TILES:
        p0 = T * TILE
        for e in (p0 - 1, p0, p0 + 1):                   # begin in the look-back bucket, end one before / at / one past the tile's first cell
            for b in (p0 - bucket, p0 - bucket + 1, p0 - bucket // 2, p0 - 2, p0 - 1):
                if b < e and e - b <= bucket: seams.append([0, b, e])
        seams.append([0, p0 - bucket, p0])               # a whole bucket long, ending at the seam
        for z in (p0 - 1, p0, p0 + TILE - 1): seams.append([0, z, z])        # runs without cells
        for b in (p0 + TILE - bucket, p0 + TILE - 1, p0 + TILE - bucket // 3): seams.append([0, b, p0 + TILE])   # ending exactly at the tile's end
        seams += [[0, p0, p0 + 1], [0, p0, p0 + bucket], [0, p0 + TILE - 1, p0 + TILE + 1], [0, p0 + 4095, p0 + 4097]]
    seams = np.array(seams, dtype=np.int32)
    n = 6000                                             # a few hundred runs per tile around them, some clipped at the contigs' ends
    tid = rng.choice(2, n, p=np.asarray(LENS) / sum(LENS))
    beg = (rng.random(n) * (np.asarray(LENS)[tid] + 40)).astype(np.int64) - 5
    end = beg + rng.integers(0, min(bucket, 300), n)
    rand = np.stack([tid, beg, end], axis=1).astype(np.int32)
    pile = np.tile(np.array([[0, 8 * TILE + 100, 8 * TILE + 200]], dtype=np.int32), (20000, 1))      # 40 000-fold with the other array's: tile 8, p0 = 65536
    first = sort_iv(np.concatenate([seams, rand[:4000], pile]))
    other = np.concatenate([seams, rand[4000:], pile])
    other = other[rng.permutation(other.shape[0])]
    depth = oracle_depth(LENS, np.concatenate([first, other]))
    return first, other, depth


@functools.lru_cache(maxsize=None)
def seam_windows(bucket, w, md, wrap):
    return oracle_windows(seam_sample(bucket)[2], w, md, wrap)


def test_seam_samples_are_what_they_claim():
    for bucket in (512, 4096):
        first, other, depth = seam_sample(bucket)
        for iv in (first, other):
            L = np.asarray(LENS)[iv[:, 0]]
            assert int((np.clip(iv[:, 2], 0, L) - np.clip(iv[:, 1], 0, L)).max()) == bucket
        assert int(depth[0][8 * TILE + 150]) >= 40000 and int(depth[0][8 * TILE - 1]) >= 2 * 5
        flat = first[first[:, 0] == 0]
        for T in SEAM_TILES:
            assert ((flat[:, 1] < T * TILE) & (flat[:, 2] == T * TILE + 1)).any() and ((flat[:, 1] == flat[:, 2]) & (flat[:, 1] == T * TILE)).any()


def _device(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@gpu
@pytest.mark.parametrize("bucket", [512, 4096])
@pytest.mark.parametrize("un", UN_CODES)
def test_sixteen_bit_seams_on_the_direct_path(un, bucket):
    first, other, _ = seam_sample(bucket)
    ft, ot = _device(first, other)
    with pda.Engine(LENS) as e:
        e.set_param("lmax", bucket)
        e.keep_deferred(True)
        e.set_param("direct_un", un)
        runs = e.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        for w in WS:
            for md, wrap in MODES:
                e.reset()
                e.push_runs(runs, pda.PD_PUSH_MORE)
                _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                ref = seam_windows(bucket, w, md, wrap)
                assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (w, md, wrap)
        e.reset()
        e.runs_destroy(runs)


@gpu
@pytest.mark.parametrize("bucket", [512, 4096])
def test_sixteen_bit_seams_in_the_export_form(bucket):
    """pd_export_i4 of the compact sample equals the export of the arrays: image and exception set"""
    import torch
    dev = torch.device("cuda", 0)
    first, other, _ = seam_sample(bucket)
    ft, ot = _device(first, other)
    B = 8192

    def export(e):
        n_cells, _ = e.device_layout()
        img = torch.zeros(n_cells // 2, dtype=torch.uint8, device=dev)
        exc = torch.zeros((B, 2), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.export_i4(img.data_ptr(), exc.data_ptr(), B, cnt.data_ptr())
        e.synchronize()
        return img, exc[:int(cnt.item())].cpu().numpy()

    with pda.Engine(LENS) as ea, pda.Engine(LENS) as ed:
        ea.push_intervals(first, pda.PD_PUSH_SORTED)
        ea.push_intervals(other, pda.PD_PUSH_DEFAULT)
        img_a, exc_a = export(ea)
        ed.set_param("lmax", bucket)
        ed.keep_deferred(True)
        runs = ed.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        ed.push_runs(runs, pda.PD_PUSH_MORE)
        img_d, exc_d = export(ed)
        assert torch.equal(img_a, img_d)
        key = lambda x: sorted(map(tuple, x.tolist()))
        assert key(exc_a) == key(exc_d) and len(exc_a) >= 2
        ed.reset()
        ed.runs_destroy(runs)


LONG_LENS = [300000]


@functools.lru_cache(maxsize=None)
def long_sample():
    long_runs = np.array([[0, b, b + n] for b in (65535, 65536, 131071) for n in (65535, 65536, 65537, 200003)], dtype=np.int32)
    rng = np.random.default_rng(9)
    beg = rng.integers(0, LONG_LENS[0], 3000)
    rand = np.stack([np.zeros(3000, dtype=np.int64), beg, beg + rng.integers(0, 300, 3000)], axis=1).astype(np.int32)
    first = sort_iv(np.concatenate([long_runs, rand[:2000]]))
    other = np.concatenate([rand[2000:], long_runs])
    return first, other, oracle_depth(LONG_LENS, np.concatenate([first, other]))


@gpu
def test_both_planes_survive():
    """begins and lengths of 2^16 and more: whatever puts a whole run together again (the sample is expanded) sees all 32 + 32 bits"""
    first, other, depth = long_sample()
    ft, ot = _device(first, other)
    with pda.Engine(LONG_LENS) as e:
        e.keep_deferred(True)
        runs = e.runs_create(ft.data_ptr(), ft.shape[0], ot.data_ptr(), ot.shape[0])
        e.push_runs(runs, pda.PD_PUSH_MORE)
        e.scan(0)
        assert np.array_equal(e.read_depth(0, 0, LONG_LENS[0]), depth[0])
        for w, md, wrap in ((100, 1, 0), (100, 0, 0), (8192, 1, 0), (10000, 3, 0), (10000000, 1, 18)):
            e.reset()
            e.push_runs(runs, pda.PD_PUSH_MORE)
            _, cover, tot = e.scan_reduce_windows(w, md, wrap)
            ref = oracle_windows(depth, w, md, wrap)
            assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (w, md, wrap)
        e.reset()
        e.runs_destroy(runs)
