"""numpy model of the 4-bit image path of the sliced sum (pd_export_i4 -> pd_slice_sweep_i4 -> pd_gather_windows), and a
generator of crafted images for tests/test_gpu_sliced_edges.py.

Everything is int64 on the host; nothing here touches a GPU.  The flat cell space is the engine's: contig t owns a
slot of roundup(len_t + 1, 8192) cells, the slots follow each other, a tile is 8192 cells and belongs to exactly one contig.

pd_slice_sweep_i4 is a pure function of the buffers it is given — the parts (one nibble d + 8 per cell), the tile sums and the
exception blocks — so a test needs no reads to put the kernels into a chosen state: the generator below builds the PARTS first
(so that chosen tiles stay free of exceptions and reach the packed kernels) from a target depth profile that is never negative,
which is what the kernels assume of their input.
"""
import numpy as np

TILE = 8192
GENOME = [70001, 50001, 1, 8192, 8191, 16384, 3, 30000, 60000]      # 36 tiles; contig 0: eight whole tiles and a ragged ninth
EXC_DTYPE = np.dtype([("cell", "<u8"), ("value", "<i4"), ("pad", "<i4")])            # pd_exc
PART_DTYPE = np.dtype([("c0", "<u4"), ("c1", "<u4"), ("s0", "<u8"), ("s1", "<u8")])   # TilePart, PD_TILE_PARTIAL_BYTES = 24
assert EXC_DTYPE.itemsize == 16 and PART_DTYPE.itemsize == 24


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def layout(lens):
    """(slot offsets in cells, n_cells, contig of every tile)"""
    lens = np.asarray(lens, dtype=np.int64)
    slot = (lens + 1 + TILE - 1) // TILE * TILE
    off = np.concatenate([[0], np.cumsum(slot)]).astype(np.int64)
    tile_contig = np.repeat(np.arange(lens.size), slot // TILE)
    return off[:-1], int(off[-1]), tile_contig


def window_offsets(lens, w):
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate([[0], np.cumsum((lens + w - 1) // w)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the image: d + 8 per cell, cell 2k in the low nibble of byte k
# ---------------------------------------------------------------------------------------------------------------------
def pack_nibbles(nib):
    nib = np.asarray(nib)
    assert nib.shape[-1] % 2 == 0 and nib.min() >= 0 and nib.max() <= 15
    nib = nib.astype(np.uint8)
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8)


def pack_i4(d):
    d = np.asarray(d, dtype=np.int64)
    assert d.min() >= -8 and d.max() <= 7
    return pack_nibbles(d + 8)


def unpack_i4(img):
    img = np.asarray(img, dtype=np.uint8)
    d = np.empty(img.shape[:-1] + (img.shape[-1] * 2,), dtype=np.int64)
    d[..., 0::2] = (img & 15).astype(np.int64) - 8
    d[..., 1::2] = (img >> 4).astype(np.int64) - 8
    return d


def clip_or_zero(D, lo=-8, hi=7):
    """what an export writes into its image: the difference, or 0 where it travels as an exception"""
    D = np.asarray(D, dtype=np.int64)
    return np.where((D < lo) | (D > hi), 0, D)


def exception_set(D, lo=-8, hi=7):
    D = np.asarray(D, dtype=np.int64)
    c = np.nonzero((D < lo) | (D > hi))[0]
    return sorted(zip(c.tolist(), D[c].tolist()))


def diff_from_intervals(lens, iv):
    """difference arrays of the flat cell space: +1 at a run's begin, -1 at its end, runs clipped to [0, len]"""
    off, n_cells, _ = layout(lens)
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 3)
    L = np.asarray(lens, dtype=np.int64)[iv[:, 0]]
    b, e = np.clip(iv[:, 1], 0, L), np.clip(iv[:, 2], 0, L)
    keep = b < e
    D = np.zeros(n_cells, dtype=np.int64)
    np.add.at(D, off[iv[keep, 0]] + b[keep], 1)
    np.add.at(D, off[iv[keep, 0]] + e[keep], -1)
    return D


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
def summed_increments(parts, exc_blocks, exc_counts, tile_first, tile_count):
    """D of the cells of the tiles [tile_first, tile_first + tile_count): sum over the parts of (nibble - 8), plus the exceptions
    whose cell lies in the range, at most min(count_j, exc_stride) of block j (a negative count: none; no counts: none)"""
    parts = np.asarray(parts, dtype=np.uint8)
    parts = parts.reshape(parts.shape[0], -1)
    assert parts.shape[1] == tile_count * (TILE // 2)
    D = np.zeros(parts.shape[1] * 2, dtype=np.int64)
    for row in parts:
        D += unpack_i4(row)
    if exc_blocks is not None and exc_counts is not None:
        exc_blocks = np.asarray(exc_blocks, dtype=EXC_DTYPE).reshape(parts.shape[0], -1)
        c_lo, c_hi = tile_first * TILE, (tile_first + tile_count) * TILE
        for j in range(parts.shape[0]):
            n = min(max(int(exc_counts[j]), 0), exc_blocks.shape[1])
            e = exc_blocks[j, :n]
            m = (e["cell"] >= c_lo) & (e["cell"] < c_hi)
            np.add.at(D, (e["cell"][m] - np.uint64(c_lo)).astype(np.int64), e["value"][m].astype(np.int64))
    return D


def wrap_mask(wrap_bits):
    return 0xFFFFFFFF if wrap_bits in (0, 32) else (1 << wrap_bits) - 1


def sweep_ref(parts, exc_blocks, exc_counts, lens, tile_first, tile_count, w, min_dep, wrap_bits, tile_sums=None):
    """The TilePart of every tile of the range.  parts: (n_parts, tile_count * 4096) bytes, the images of the range; tile_sums: the
    int32 sums of ALL tiles of the buffer (the prefix before the range comes from them; not needed when tile_first == 0)."""
    D = summed_increments(parts, exc_blocks, exc_counts, tile_first, tile_count)
    return sweep_increments(D, lens, tile_first, tile_count, w, min_dep, wrap_bits, tile_sums)


def sweep_increments(D, lens, tile_first, tile_count, w, min_dep, wrap_bits, tile_sums=None):
    """sweep_ref's second half: from the summed increments of the range to its TileParts"""
    off, n_cells, tile_contig = layout(lens)
    lens = np.asarray(lens, dtype=np.int64)
    before = 0
    if tile_first:
        before = int(np.asarray(tile_sums, dtype=np.int64)[:tile_first].sum())
    depth = (before + np.cumsum(D)) & 0xFFFFFFFF & wrap_mask(wrap_bits)
    depth = depth.reshape(tile_count, TILE)
    t = np.arange(tile_first, tile_first + tile_count)
    ctg = tile_contig[t]
    local0 = t * TILE - off[ctg]
    clen = lens[ctg]
    nb = (local0 // w + 1) * w - local0
    pos = np.arange(TILE, dtype=np.int64)[None, :]
    ok = (local0[:, None] + pos < clen[:, None]) & (depth >= min_dep)
    first = pos < nb[:, None]
    out = np.zeros(tile_count, dtype=PART_DTYPE)
    out["c0"] = (ok & first).sum(axis=1)
    out["c1"] = (ok & ~first).sum(axis=1)
    out["s0"] = np.where(ok & first, depth, 0).sum(axis=1)
    out["s1"] = np.where(ok & ~first, depth, 0).sum(axis=1)
    return out


def fold_windows(partials, lens, w):
    """pd_gather_windows: (c0, s0) of a tile go to the window its first cell lies in, (c1, s1) to the next one"""
    off, n_cells, tile_contig = layout(lens)
    lens = np.asarray(lens, dtype=np.int64)
    partials = np.asarray(partials, dtype=PART_DTYPE)
    assert partials.size == n_cells // TILE
    woff = window_offsets(lens, w)
    cover = np.zeros(int(woff[-1]), dtype=np.int64)
    tot = np.zeros(int(woff[-1]), dtype=np.uint64)
    for t in range(partials.size):
        c = int(tile_contig[t])
        local0 = t * TILE - int(off[c])
        p = partials[t]
        if local0 >= lens[c]:
            assert int(p["c0"]) == 0 and int(p["c1"]) == 0 and int(p["s0"]) == 0 and int(p["s1"]) == 0
            continue
        k = int(woff[c]) + local0 // w
        cover[k] += int(p["c0"]); tot[k] += p["s0"]
        if k + 1 < int(woff[c + 1]):
            cover[k + 1] += int(p["c1"]); tot[k + 1] += p["s1"]
        else:
            assert int(p["c1"]) == 0 and int(p["s1"]) == 0
    return cover.astype(np.uint32), tot


def windows_from_depth(depth, lens, w, min_dep):
    """the same windows straight from the cells (no tiles, no partials)"""
    off, n_cells, _ = layout(lens)
    cov, tot = [], []
    for c, ln in enumerate(lens):
        x = np.asarray(depth[off[c]:off[c] + ln], dtype=np.int64)
        for s in range(0, ln, w):
            seg = x[s:min(s + w, ln)]
            m = seg >= min_dep
            cov.append(int(m.sum())); tot.append(int(seg[m].sum()))
    return np.array(cov, dtype=np.uint32), np.array(tot, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def nonneg_walk(steps):
    """depth of the walk `steps`, lifted wherever it would go below zero; an increment only ever moves towards zero by that, so
    increments that were in [-8n, 7n] still are"""
    depth = np.cumsum(np.asarray(steps, dtype=np.int64))
    return depth - np.minimum.accumulate(np.minimum(depth, 0))


def split_parts(D, n, rng):
    """n nibble planes (values 0..15) whose (nibble - 8) add up to D per cell; D in [-8n, 7n]"""
    D = np.asarray(D, dtype=np.int64)
    assert D.min() >= -8 * n and D.max() <= 7 * n, (int(D.min()), int(D.max()), n)
    q, r = np.divmod(D + 8 * n, n)
    rot = rng.integers(0, n, D.size)
    j = np.arange(n)[:, None]
    nib = q[None, :] + (((j + rot[None, :]) % n) < r[None, :])
    for _ in range(2):                                              # pairwise zero-sum perturbations, clipped to the nibble range
        perm = rng.permutation(n)
        for i in range(0, n - 1, 2):
            a, b = nib[perm[i]], nib[perm[i + 1]]
            d = np.clip(rng.integers(-4, 5, D.size), np.maximum(-a, b - 15), np.minimum(15 - a, b))
            nib[perm[i]] = a + d
            nib[perm[i + 1]] = b - d
    assert nib.min() >= 0 and nib.max() <= 15 and np.array_equal(nib.sum(axis=0) - 8 * n, D)
    return nib.astype(np.uint8)


class Case:
    """One crafted input of pd_slice_sweep_i4 over the whole buffer of GENOME.

    T: the depth of every cell WITHOUT the exceptions (never negative); exc: [(part, cell, value)], whose running sum is never
    negative either, so that the input is valid with the exceptions and (dev_exc_counts = NULL) without them.  The parts are
    made from diff(T); the exceptions come on top.  counts / blocks may be overridden to craft count edges.
    props: what the case promises about itself (tests/test_i4_model.py holds it to that):
       free_tiles   tiles that hold no exception
       bracket      (tiles, lo, hi): the depth over those tiles has exactly this minimum and maximum
       values       depths that occur in the bracket's tiles
       saturated    cells with every part at nibble 15 exist, and cells with every part at 0
       exact        {cell: depth}
    """

    def __init__(self, name, n_parts, T, exc=(), seed=0, exc_stride=16, counts=None, junk=None, **props):
        self.name, self.n_parts, self.props, self.exc_stride = name, n_parts, props, exc_stride
        self.lens = GENOME
        off, self.n_cells, self.tile_contig = layout(GENOME)
        self.n_tiles = self.n_cells // TILE
        T = np.asarray(T, dtype=np.int64)
        assert T.size == self.n_cells and T.min() >= 0
        rng = np.random.default_rng(seed)
        self.nib = split_parts(np.diff(T, prepend=0), n_parts, rng)
        self.parts = pack_nibbles(self.nib)                          # (n_parts, n_cells / 2) bytes
        self.blocks = np.zeros((n_parts, exc_stride), dtype=EXC_DTYPE)
        fill = np.zeros(n_parts, dtype=np.int64)
        for (j, cell, value) in exc:
            self.blocks[j, fill[j]] = (cell, value, 0)
            fill[j] += 1
        self.counts = fill.astype(np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
        for (j, k, cell, value) in (junk or ()):                     # entries beyond a block's count: must never be read
            assert k >= fill[j]
            self.blocks[j, k] = (cell, value, 0)
        self.with_exceptions = True
        self._inc = {}
        self._derive()

    def _derive(self):
        blocks, counts = (self.blocks, self.counts) if self.with_exceptions else (None, None)
        self.D = summed_increments(self.parts, blocks, counts, 0, self.n_tiles)
        self.depth = np.cumsum(self.D)
        self.tile_sums = self.D.reshape(-1, TILE).sum(axis=1).astype(np.int32)

    def without_exceptions(self):
        """the same parts handed over with dev_exc_counts = NULL: tile sums and depth of the parts alone"""
        import copy
        c = copy.copy(self)
        c.name, c.with_exceptions = self.name + "-null", False
        c._derive()
        return c

    def exception_tiles(self):
        if not self.with_exceptions:
            return set()
        out = set()
        for j in range(self.n_parts):
            n = min(max(int(self.counts[j]), 0), self.exc_stride)
            cells = self.blocks[j, :n]["cell"]
            out |= set((cells[cells < self.n_cells] // TILE).tolist())
        return out

    def ref(self, tile_first, tile_count, w, min_dep, wrap_bits):
        """sweep_ref of a range of this case (the summed increments of a range are kept: they do not depend on w, min_dep, wrap_bits)"""
        key = (tile_first, tile_count, self.with_exceptions)
        if key not in self._inc:
            b = (TILE // 2)
            blocks, counts = (self.blocks, self.counts) if self.with_exceptions else (None, None)
            self._inc[key] = summed_increments(self.parts[:, tile_first * b:(tile_first + tile_count) * b], blocks, counts, tile_first, tile_count)
        return sweep_increments(self._inc[key], self.lens, tile_first, tile_count, w, min_dep, wrap_bits, self.tile_sums)


N_CELLS = layout(GENOME)[1]
N_TILES = N_CELLS // TILE


def _sparse_steps(n, rng, size=N_CELLS):
    u = rng.random(size)
    steps = np.where(u < 0.02, rng.integers(-8 * n, 7 * n + 1, size), 0)
    steps = np.where((u >= 0.02) & (u < 0.0225), rng.integers(0, 7 * n + 1, size), steps)
    off, _, _ = layout(GENOME)
    steps[off[1] + 20000:off[2]] = 0                                # long stretches of depth 0: the end of contig 1 ...
    steps[off[5]:off[6]] = 0                                        # ... and all of contig 5
    return steps.astype(np.int64)


def sparse_case(n, seed=1):
    rng = np.random.default_rng(1000 + seed * 64 + n)
    T = nonneg_walk(_sparse_steps(n, rng))
    return Case("sparse-%d" % n, n, T, seed=seed, free_tiles=tuple(range(N_TILES)), mode="sparse")


SAT_STARTS = (100, 2048 - 8, 4096 + 31, 8192 * 2 - 20, 8192 * 3 + 2048 * 3 - 64, 8192 * 5 + 17, 8192 * 9 + 1000, 8192 * 20 + 8191 - 300)


def saturated_case(n, seed=2):
    """stretches where every part is +7 (nibble 15: a byte of the packed sums reaches 15 * n_parts), then every part -8 (nibble 0);
    8k cells up and 7k cells down return to the level they started from"""
    rng = np.random.default_rng(2000 + seed * 64 + n)
    steps = _sparse_steps(n, rng)
    for i, s in enumerate(SAT_STARTS):
        k = (1, 4, 8, 32)[i % 4]
        steps[s:s + 8 * k] = 7 * n
        steps[s + 8 * k:s + 15 * k] = -8 * n
    T = nonneg_walk(steps)
    return Case("saturated-%d" % n, n, T, seed=seed, free_tiles=tuple(range(N_TILES)), saturated=True, mode="saturated")


def _lifted(base, exc_part=0, lift_cell=TILE + 3000, drop_cell=7 * TILE + 100):
    """exceptions that lift the depth by `base` at a cell of tile 1 and drop it again in tile 7: the tiles 2..6 between them reach
    any height without an exception of their own"""
    return [(exc_part, lift_cell, base), (exc_part, drop_cell, -base)]


PLATEAU_TILES = (2, 3, 4, 5, 6)


def plateau_case(n, h, amp=3, seed=3, extra_exc=(), name=None):
    """depth 0, then h +- amp from a cell of tile 1 to a cell of tile 7 (every value of the bracket occurs), then 0 again"""
    rng = np.random.default_rng(3000 + seed * 64 + n + h)
    lift, drop = TILE + 3000, 7 * TILE + 100
    T = np.zeros(N_CELLS, dtype=np.int64)
    u = rng.integers(0, amp + 1, drop - lift + 1)
    u[:2] = 0
    u[-2:] = 0
    u[5 * TILE:5 * TILE + 2 * amp + 2] = np.arange(2 * amp + 2) // 2   # (in tile 6) every value, whatever the draw
    r = u[:-1] + u[1:]                                               # 0 .. 2 amp, neighbours differ by at most amp: one part can carry it
    T[lift:drop] = r                                                 # the parts' share: 0 .. 2 amp; the exceptions add h - amp
    exc = _lifted(h - amp, 0, lift, drop) + list(extra_exc)
    free = tuple(t for t in range(N_TILES) if t not in {1, 7} | {c // TILE for (_, c, _) in extra_exc})
    return Case(name or "plateau-%d-%d" % (h, n), n, T, exc, seed=seed, free_tiles=free, bracket=(PLATEAU_TILES if not extra_exc else (2, 4), h - amp, h + amp),
                values=tuple(range(h - amp, h + amp + 1)), mode="plateau")


def climb_case(n, seed=4, base=59000, top=61000):
    """depth `base` over the tiles 2..6; in quarter q of tile 2 + q the parts climb through 60 000 to `top` and come down again, so the
    packed kernel has finished q quarters of that tile when it meets a depth it must hand over"""
    T = np.zeros(N_CELLS, dtype=np.int64)
    lift, drop = TILE + 3000, 7 * TILE + 100
    exact = {}
    for q in range(4):
        s = (2 + q) * TILE + q * 2048 + 700
        up = np.minimum(np.arange(1, 2048) * 7 * n, top - base)
        n_up = int(np.argmax(up == top - base)) + 1
        T[s:s + n_up] = up[:n_up]
        T[s + n_up:s + n_up + 100] = top - base
        down = np.maximum(top - base - np.arange(1, 2048) * 8 * n, 0)
        n_dn = int(np.argmax(down == 0)) + 1
        T[s + n_up + 100:s + n_up + 100 + n_dn] = down[:n_dn]
        assert 700 + n_up + 100 + n_dn < 2048                       # inside the quarter
        exact[s - 1] = base
        exact[s + n_up + 50] = top
        exact[(2 + q) * TILE + q * 2048 + 2047] = base
    return Case("climb-%d" % n, n, T, _lifted(base, 0, lift, drop), seed=seed, free_tiles=tuple(t for t in range(N_TILES) if t not in (1, 7)),
                bracket=((2, 3, 4, 5), base, top), exact=exact, mode="climb")


ZERO_TILES = {1: 0, 2: 15, 3: 16, 4: 31}                            # tile -> the cell of a lane's 32 that touches zero


def touch_zero_cells():
    return [t * TILE + q * 2048 + lane * 32 + k for t, k in ZERO_TILES.items() for q in (0, 3) for lane in (0, 63)]


NEAR_LANE = 5 * TILE + 2048 + 17 * 32                               # first cell of a lane that starts at depth 2 and only comes down to 1


def touch_zero_case(n, seed=5):
    """depth 1 over the tiles 1..5, and exactly 0 at single cells — cell 0, 15, 16, 31 of a lane's 32 (both halves of the 16 + 16 packed
    walk), in the lanes 0 and 63 of the quarters 0 and 3: each such lane starts at depth b0 = 1 and its negative differences sum to 1.
    In tile 5 a lane starts at depth 2 and its negative differences sum to 1 (b0 == neg + 1): no cell of it is zero."""
    T = np.zeros(N_CELLS, dtype=np.int64)
    T[TILE - 1:6 * TILE] = 1                                        # (from the cell before tile 1: the tile's carry is 1)
    exact = {}
    for c in touch_zero_cells():
        T[c] = 0
        exact[c] = 0
        exact[c + 1] = 1
        if c > TILE:
            exact[c - 1] = 1
    T[NEAR_LANE - 1:NEAR_LANE + 32] = 2
    T[NEAR_LANE + 9] = 1
    exact.update({NEAR_LANE - 1: 2, NEAR_LANE + 9: 1, NEAR_LANE + 8: 2, NEAR_LANE + 10: 2, NEAR_LANE + 32: 1})
    return Case("touch-zero-%d" % n, n, T, seed=seed, free_tiles=tuple(range(N_TILES)), bracket=((1, 2, 3, 4, 5), 0, 2), exact=exact, mode="touch-zero")


SLICES3 = ((0, 12), (12, 12), (24, 12))


def exceptions_case(seed=6):
    """three parts over a sparse background: one cell named by all three parts, values +-1 and +-300 000, the first and last cell of every
    slice's first and last tile (= one cell outside the neighbouring slice on each side), cells >= n_cells"""
    n = 3
    rng = np.random.default_rng(6000 + seed)
    T = nonneg_walk(_sparse_steps(n, rng))
    exc = []
    same = 3 * TILE + 4097
    exc += [(0, same, 300000), (1, same, 1), (2, same, -1), (1, same + 700, -300000)]
    exc += [(2, 5 * TILE + 11, 1), (2, 5 * TILE + 12, -1)]
    for k, (t0, tc) in enumerate(SLICES3):
        j = k % n
        exc += [(j, t0 * TILE, 1), (j, t0 * TILE + TILE - 1, -1), (j, (t0 + tc - 1) * TILE, 2), (j, (t0 + tc) * TILE - 1, -2)]
    exc += [(0, N_CELLS, 7), (1, N_CELLS + 5, -9), (2, 1 << 40, 1000)]
    tiles = {c // TILE for (_, c, _) in exc if c < N_CELLS}
    return Case("exceptions", n, T, exc, seed=seed, exc_stride=16, free_tiles=tuple(t for t in range(N_TILES) if t not in tiles),
                exact={same - 1: int(T[same - 1]), same: int(T[same]) + 300000, same + 700: int(T[same + 700])}, mode="exceptions")


def exception_counts_case(seed=7):
    """exc_counts[j] negative (the block is ignored although it holds entries) and larger than exc_stride (clamped: the block is full)"""
    n = 3
    rng = np.random.default_rng(7000 + seed)
    T = nonneg_walk(_sparse_steps(n, rng))
    stride = 8
    exc = [(0, 2 * TILE + 5, 9), (0, 2 * TILE + 900, -9)]
    exc += [(2, 4 * TILE + 100 * i, 20 if i % 2 == 0 else -20) for i in range(stride)]           # block 2 is full, every entry counts
    junk = [(1, i, 6 * TILE + 50 + i, 1000) for i in range(stride)]                              # block 1: entries, and a count of -3
    junk += [(0, 2 + i, 8 * TILE + i, -5000) for i in range(stride - 2)]                         # block 0: entries behind its count of 2
    return Case("exception-counts", n, T, exc, seed=seed, exc_stride=stride, counts=[2, -3, stride + 100], junk=junk,
                free_tiles=tuple(t for t in range(N_TILES) if t not in (2, 4)), mode="exceptions")


def flagged_between_plateaus_case(n=2, seed=8):
    """tiles 2..6 at 61 000 (the packed kernel hands them over), tile 3 with an exception of its own (the workgroup form with the LDS
    patch): the three forms are neighbours; tile 8 and later are ordinary packed tiles"""
    extra = [(1, 3 * TILE + 2048 + 77, 1), (1, 3 * TILE + 2048 + 78, -1)]
    return plateau_case(n, 61000, 3, seed, extra_exc=extra, name="flagged-between-plateaus")


def every_tile_flagged_case(seed=9):
    n = 2
    rng = np.random.default_rng(9000 + seed)
    T = nonneg_walk(_sparse_steps(n, rng))
    exc = []
    for t in range(N_TILES):
        exc += [(t % n, t * TILE + 5 + t, 1 + t), (t % n, t * TILE + 9 + 2 * t, -1 - t)]
    return Case("every-tile-flagged", n, T, exc, seed=seed, exc_stride=64, free_tiles=(), mode="full-lists")


def every_tile_slow_case(seed=10):
    """16 parts climb to 61 000 inside the first quarter of tile 0 and the depth stays there to the end of the buffer: the packed kernel hands
    over every tile it starts (the others — a contig's end, a window boundary — are never started); no exceptions"""
    n = 16
    rng = np.random.default_rng(10000 + seed)
    T = np.zeros(N_CELLS, dtype=np.int64)
    T[:] = 61000 + rng.integers(0, 7, N_CELLS)
    up = np.minimum(np.arange(1, 1001) * 7 * n, 61000)
    T[:1000] = up
    return Case("every-tile-slow", n, T, seed=seed, free_tiles=tuple(range(N_TILES)), bracket=(tuple(range(1, N_TILES)), 61000, 61006), mode="full-lists")


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_sliced_edges.py, by name; tests/test_i4_model.py checks what each promises
# ---------------------------------------------------------------------------------------------------------------------
PART_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33)
GATE_HEIGHTS = (59990, 60000, 60010, 63500, 65530, 65536, 70000)
# +- 5: 262 140 .. 262 150 and 65 530 .. 65 540 (whose lanes all start at 60 000 or more: every tile is handed over), and 40 000, between
# 2^15 and the gate: the one height at which the packed kernels themselves would have to wrap for wrap_bits = 15, and so must not be used
WRAP_HEIGHTS = (262145, 65535, 40000)

_cache = {}


def case(kind, *args):
    key = (kind,) + args
    if key not in _cache:
        _cache[key] = BUILDERS[kind](*args)
    return _cache[key]


BUILDERS = {
    "sparse": sparse_case,
    "saturated": saturated_case,
    "plateau": lambda n, h: plateau_case(n, h, 3),
    "wrap": lambda n, h: plateau_case(n, h, 5),
    "climb": climb_case,
    "touch-zero": touch_zero_case,
    "exceptions": exceptions_case,
    "exception-counts": exception_counts_case,
    "flagged-between-plateaus": flagged_between_plateaus_case,
    "every-tile-flagged": every_tile_flagged_case,
    "every-tile-slow": every_tile_slow_case,
}


def all_case_keys():
    keys = [(m, n) for n in PART_COUNTS for m in ("sparse", "saturated")]
    keys += [("plateau", n, h) for n in (1, 16) for h in GATE_HEIGHTS]
    keys += [("climb", n) for n in (1, 16)]
    keys += [("wrap", n, h) for n in (1, 16) for h in WRAP_HEIGHTS]
    keys += [("touch-zero", n) for n in (1, 16)]
    keys += [("exceptions",), ("exception-counts",), ("flagged-between-plateaus",), ("every-tile-flagged",), ("every-tile-slow",)]
    return keys


# ---------------------------------------------------------------------------------------------------------------------
# the export side: a sample of reads stacked so that chosen cells have chosen differences
# ---------------------------------------------------------------------------------------------------------------------
EDGE_VALUES = (-10, -9, -8, -7, 7, 8, 9)
# in-tile positions: first / last cell of the tile, of a wave's 2048-cell span, of a lane's 4-cell group
EDGE_POS = (0, 8191, 4096, 6143, 1200, 2003)
READ_LEN = 40


def stacked_reads(values=EDGE_VALUES, positions=EDGE_POS, first_tile=1, contig=0):
    """value i lives in tile first_tile + i of `contig`: |v| reads beginning (v > 0) or ending (v < 0) on each of the positions.
    Returns (runs (tid, beg, end), {cell of the contig: v})."""
    iv, want = [], {}
    for i, v in enumerate(values):
        for p in positions:
            c = (first_tile + i) * TILE + p
            run = (contig, c, c + READ_LEN) if v > 0 else (contig, c - READ_LEN, c)
            iv += [run] * abs(v)
            want[c] = v
    return np.array(iv, dtype=np.int32), want


def export_sample(seed=11):
    """the stacked reads over a light random background that leaves whole contigs (and so half-tiles) unwritten"""
    rng = np.random.default_rng(seed)
    iv, want = stacked_reads()
    n = 3000
    tid = rng.choice([1, 7], n).astype(np.int64)                    # contigs 2..6 and 8 stay untouched, contig 0 has the stacks alone
    L = np.asarray(GENOME, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L // 2)).astype(np.int64) - 5           # ... and the second half of the contigs 1 and 7
    bg = np.stack([tid, beg, beg + rng.integers(0, 300, n)], axis=1).astype(np.int32)
    allv = np.concatenate([iv, bg])
    order = np.lexsort((allv[:, 1], allv[:, 0]))
    return allv[order], want
