"""k_direct_c8 reads one descriptor record per tile (TileDesc, written by k_c8_tile_desc when a compact sample is finished) instead of
chasing the bucket starts and the contig table: the descriptors of a contig's first tile (no look-back), of its last, partial tile, of
neighbours in different contigs, of empty and of pile-up tiles, for every bucket width, walked by one workgroup, by two and by the default
grid — against a numpy difference-array reference and against the arrays path of the same engine."""
import functools

import numpy as np
import pytest

import pandepth_amd as pda

gpu = pytest.mark.gpu

TILE = 8192
# 3 tiles + 5 cells, exactly one tile, 8191 cells, one cell, 2 tiles: nine tiles, every contig's first tile next to another contig's last
LENS = [3 * TILE + 5, TILE, TILE - 1, 1, 2 * TILE]
MAXLEN = 200                                             # no run longer than the narrowest bucket (256 cells): the sample stays compact for every lmax
WS = (8192, 10000, 10000000)
MODES = ((1, 0), (0, 0), (3, 18), (2, 0))               # (min_dep, wrap)


def sort_iv(iv):
    return iv[np.lexsort((iv[:, 1], iv[:, 0]))]


def rand_runs(rng, n, max_len=MAXLEN):
    tid = rng.choice(len(LENS), n, p=np.asarray(LENS) / sum(LENS))          # even coverage: a contig's share is its length
    L = np.asarray(LENS, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L + 40)).astype(np.int64) - 5          # some start before cell 0, some end past the contig
    end = beg + rng.integers(0, max_len, n)
    return np.stack([tid, beg, end], axis=1).astype(np.int32)


def later_runs(rng, first, frac=0.2):
    k = rng.random(first.shape[0]) < frac
    other = first[k].copy()
    other[:, 1] = first[k][:, 2] + rng.integers(1, 400, int(k.sum())).astype(np.int32)
    other[:, 2] = other[:, 1] + rng.integers(1, MAXLEN, other.shape[0]).astype(np.int32)
    return other[rng.permutation(other.shape[0])]                  # the second array may come in any order


def layers(tid, a, b, k, hole=None):
    """[a, b) of a contig covered by exactly k layers of abutting runs of <= 128 cells (every layer cut at other places); `hole`: one
    cell that the first layer leaves out."""
    out = []
    for j in range(k):
        x = a
        nxt = a + (37 * j) % 128 + 1
        while x < b:
            y = min(nxt, b)
            if j == 0 and hole is not None and x <= hole < y:
                out += [[tid, x, hole], [tid, hole + 1, y]]
            else:
                out.append([tid, x, y])
            x, nxt = y, y + 128
    return np.array(out, dtype=np.int32)


L0 = LENS[0]
EDGES = np.array([[0, -5, 40], [0, -1, 1], [0, 0, 0], [0, 8000, 8192], [0, 8192, 8192], [0, 8192, 8392], [0, 8191, 8193], [0, 16383, 16384],
                  [0, 16128, 16384], [0, 3996, 4096], [0, 4096, 4200], [0, 462, 512], [0, 256, 300], [0, 12288, 12300], [0, 12200, 12288],
                  [0, L0 - 10, L0 + 7], [0, L0 - 1, L0], [0, L0, L0 + 3], [0, L0 + 5, L0 + 9], [0, 24576, 24581], [0, 24570, 24578],
                  [1, -3, 190], [1, 100, 100], [1, 90, 80], [1, 8000, 8192], [1, 8100, 8300], [1, 0, 1], [2, 0, 191], [2, 8100, 8191],
                  [2, 8190, 8400], [2, 8191, 8200], [3, 0, 1], [3, -2, 5], [3, 1, 4], [4, 0, 3], [4, 7992, 8192], [4, 8192, 8448],
                  [4, 16128, 16384], [4, 16300, 16500], [4, 16383, 16384]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def sample(name):
    """(sorted first runs, later runs in any order) — either may be empty"""
    rng = np.random.default_rng(sum(map(ord, name)))
    none = np.zeros((0, 3), dtype=np.int32)
    if name in ("dense", "dense_hole"):                  # ~50x: no cell of an interior tile is uncovered
        first = rand_runs(rng, 30000)
        other = later_runs(rng, first)
        if name == "dense_hole":                         # ... but 300 cells inside one quarter of an interior tile (contig 0, tile 1)
            lo, hi = TILE + 1024 + 300, TILE + 1024 + 600
            keep = lambda iv: iv[~((iv[:, 0] == 0) & (iv[:, 1] < hi) & (iv[:, 2] > lo))]
            first, other = keep(first), keep(other)
        return sort_iv(first), other
    if name == "sparse":                                 # most tiles hold cells of depth zero
        first = rand_runs(rng, 250)
        return sort_iv(first), later_runs(rng, first)
    if name == "min_depth":                              # tiles whose least depth is exactly 1, 2, 3 and tiles where ONE cell has one less
        parts = [layers(1, 0, TILE, 1), layers(0, 0, TILE, 1, hole=5000),
                 layers(4, 0, TILE, 2), layers(4, TILE, 2 * TILE, 2, hole=TILE + 1),
                 layers(0, TILE, 2 * TILE, 3), layers(0, 2 * TILE, 3 * TILE, 3, hole=3 * TILE - 1)]
        first = np.concatenate(parts)
        return sort_iv(first), none
    if name == "later_only":                             # no sorted stream at all
        return none, rand_runs(rng, 6000)
    if name == "gaps":                                   # empty tiles between populated ones (tiles 1, 3 of contig 0, contigs 1 and 3, tile 0 of contig 4)
        first = rand_runs(rng, 6000)
        t = first[:, 1] // TILE
        keep = ((first[:, 0] == 0) & ((t == 0) | (t == 2)) & (first[:, 1] % TILE < 7000) & (first[:, 1] >= 0)) | ((first[:, 0] == 2) & (first[:, 1] < 7000)) | \
               ((first[:, 0] == 4) & (first[:, 1] >= TILE + 600))
        first = first[keep]
        other = later_runs(rng, first)
        return sort_iv(first), other[other[:, 1] % TILE < 7600]
    if name == "pile":                                   # 40 000 runs in one tile (the int-window kernel's), ordinary tiles behind it
        first = np.concatenate([rand_runs(rng, 5000), np.tile(np.array([[0, 9000, 9100]], dtype=np.int32), (40000, 1))])
        return sort_iv(first), later_runs(rng, first, 0.05)
    if name == "edges":                                  # ends on tile and bucket edges (256, 512, 4096 cells), runs clipped at both ends of a contig
        first = np.concatenate([rand_runs(rng, 3000), EDGES, np.tile(np.array([[4, 8190, 8200]], dtype=np.int32), (300, 1))])
        return sort_iv(first), np.concatenate([later_runs(rng, first), EDGES[::3]])
    raise KeyError(name)


SAMPLES = ("dense", "dense_hole", "sparse", "min_depth", "later_only", "gaps", "pile", "edges")


@functools.lru_cache(maxsize=None)
def depth_ref(name):
    """per-contig depth from a difference array (runs clipped to their contig)"""
    first, other = sample(name)
    iv = np.concatenate([first, other]).astype(np.int64)
    out = []
    for t, ln in enumerate(LENS):
        x = iv[iv[:, 0] == t]
        b, e = np.clip(x[:, 1], 0, ln), np.clip(x[:, 2], 0, ln)
        ok = b < e
        diff = np.zeros(ln + 1, dtype=np.int64)
        np.add.at(diff, b[ok], 1)
        np.subtract.at(diff, e[ok], 1)
        out.append(np.cumsum(diff[:ln]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def windows_ref(name, w, min_dep, wrap):
    cov, tot = [], []
    for d in depth_ref(name):
        x = (d & ((1 << wrap) - 1) if wrap else d).astype(np.uint64)
        for s in range(0, x.size, w):
            seg = x[s:s + w]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


def _device(first, other):
    import torch
    dev = torch.device("cuda", 0)
    return torch.from_numpy(np.ascontiguousarray(first)).to(dev), torch.from_numpy(np.ascontiguousarray(other)).to(dev)


def _create(e, ft, ot):
    return e.runs_create(ft.data_ptr() if ft.shape[0] else 0, ft.shape[0], ot.data_ptr() if ot.shape[0] else 0, ot.shape[0])


def test_reference_samples_are_what_they_claim():
    """the properties the samples are chosen for, checked on the numpy reference (no engine involved)"""
    d = depth_ref("dense")
    assert all(int(x[100:-100].min()) >= 3 for x in d if x.size > TILE) and 35 <= np.concatenate(d).mean() <= 65
    h = depth_ref("dense_hole")[0]
    assert int(h[TILE + 1324:TILE + 1624].max()) == 0 and int(h[TILE + 2048:2 * TILE].min()) >= 3 and int(h[TILE:TILE + 1024].min()) >= 3
    assert sum(int((x == 0).any()) for x in depth_ref("sparse")) >= 4
    m = depth_ref("min_depth")
    assert (int(m[1].min()), int(m[4][:TILE].min()), int(m[0][TILE:2 * TILE].min())) == (1, 2, 3)
    assert (int(m[0][:TILE].min()), int((m[0][:TILE] == 0).sum())) == (0, 1)
    assert (int(m[4][TILE:].min()), int((m[4][TILE:] == 1).sum())) == (1, 1)
    assert (int(m[0][2 * TILE:3 * TILE].min()), int((m[0][2 * TILE:3 * TILE] == 2).sum())) == (2, 1)
    g = depth_ref("gaps")
    assert int(g[0][:TILE].max()) > 0 and int(g[0][TILE:2 * TILE].max()) == 0 and int(g[0][2 * TILE:3 * TILE].max()) > 0 and int(g[0][3 * TILE:].max()) == 0
    assert int(g[1].max()) == 0 and int(g[2].max()) > 0 and int(g[4][:TILE].max()) == 0 and int(g[4][TILE:].max()) > 0
    assert int(depth_ref("pile")[0][9050]) >= 40000
    assert sample("later_only")[0].shape[0] == 0
    for name in SAMPLES:
        f, o = sample(name)
        for iv in (f, o):
            if iv.shape[0]:
                L = np.asarray(LENS)[iv[:, 0]]
                assert int((np.clip(iv[:, 2], 0, L) - np.clip(iv[:, 1], 0, L)).max()) <= 256, name


@gpu
@pytest.mark.parametrize("lmax", [256, 512, 4096])
@pytest.mark.parametrize("name", SAMPLES)
def test_descriptor_walk_equals_reference_and_arrays(name, lmax):
    """Every (grid, w, min_dep, wrap) on a compact sample made with buckets of 256, 512 and 4096 cells (bshift 5, 4, 1).  grid_tiles = 1:
    ONE workgroup follows the descriptor chain across contig borders, through empty tiles, past the pile-up tile, with no next tile at
    the end."""
    first, other = sample(name)
    ft, ot = _device(first, other)
    with pda.Engine(LENS) as e:
        e.set_param("lmax", lmax)
        arrays = {}
        for w in WS:                                     # the arrays path of the same engine
            for md, wrap in MODES:
                e.reset()
                if first.shape[0]: e.push_intervals(first, pda.PD_PUSH_SORTED)
                if other.shape[0]: e.push_intervals(other, pda.PD_PUSH_DEFAULT)
                _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                ref = windows_ref(name, w, md, wrap)
                assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), ("arrays", w, md, wrap)
                arrays[(w, md, wrap)] = (cover.copy(), tot.copy())
        e.reset()
        e.keep_deferred(True)
        runs = _create(e, ft, ot)
        for grid in (1, 2, 0):
            e.set_param("grid_tiles", grid)
            for w in WS:
                for md, wrap in MODES:
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                    ref = windows_ref(name, w, md, wrap)
                    assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (grid, w, md, wrap)
                    assert np.array_equal(cover, arrays[(w, md, wrap)][0]) and np.array_equal(tot, arrays[(w, md, wrap)][1]), (grid, w, md, wrap)
        e.reset()
        e.runs_destroy(runs)


@gpu
@pytest.mark.parametrize("un", [502, 704, 802, 1803, 5704, 5802])
def test_descriptor_walk_in_the_other_instantiations(un):
    """the plain, the joined-tail and the 16-byte-load forms read the same table"""
    for name in ("edges", "pile"):
        first, other = sample(name)
        ft, ot = _device(first, other)
        with pda.Engine(LENS) as e:
            e.keep_deferred(True)
            e.set_param("direct_un", un)
            runs = _create(e, ft, ot)
            for grid in (1, 0):
                e.set_param("grid_tiles", grid)
                for w, (md, wrap) in zip(WS, MODES):
                    e.reset()
                    e.push_runs(runs, pda.PD_PUSH_MORE)
                    _, cover, tot = e.scan_reduce_windows(w, md, wrap)
                    ref = windows_ref(name, w, md, wrap)
                    assert np.array_equal(cover, ref[0]) and np.array_equal(tot, ref[1]), (name, grid, w, md, wrap)
            e.reset()
            e.runs_destroy(runs)


@gpu
@pytest.mark.parametrize("name", ["edges", "pile", "gaps"])
@pytest.mark.parametrize("grid", [1, 0])
def test_export_through_the_descriptors_equals_export_of_the_arrays(name, grid):
    """pd_export_i4 of the compact sample (k_direct_c8's export instantiation) equals the export of the arrays: image and exception set"""
    import torch
    dev = torch.device("cuda", 0)
    first, other = sample(name)
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
        ed.keep_deferred(True)
        ed.set_param("grid_tiles", grid)
        runs = _create(ed, ft, ot)
        ed.push_runs(runs, pda.PD_PUSH_MORE)
        img_d, exc_d = export(ed)
        assert torch.equal(img_a, img_d)
        key = lambda x: sorted(map(tuple, x.tolist()))
        assert key(exc_a) == key(exc_d)
        if name != "gaps": assert len(exc_a) >= 2
        ed.reset()
        ed.runs_destroy(runs)
