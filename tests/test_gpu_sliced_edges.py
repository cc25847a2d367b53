"""The 4-bit image kernels of the sliced sum at their arithmetic edges (k_export_i4, k_export_i8 / k_import_i8, k_add_i4,
k_flag_exception_tiles, k_sweep_i4<PATCH>, k_sweep_i4_wave, k_sweep_i4_fast) against the numpy model in tests/i4_model.py.

pd_slice_sweep_i4 is a pure function of the device buffers it is handed, so the sweep cases craft the images directly: part
counts up to and beyond the 16 that fit a packed byte, every part at nibble 15 or 0 in the same cell, depths on both sides of
the packed kernels' 60 000 gate and of the 2^16 / 2^18 wraps, depth exactly zero at chosen cells of a lane, exceptions at the
edges of a slice and with bad counts, and slices whose flagged / handed-over lists are full.  Every comparison is exact: the
24-byte partials of every tile, then the windows pd_gather_windows makes of them.  tests/test_i4_model.py (CPU) checks that the
inputs have the properties named here.
"""
import numpy as np
import pytest

import i4_model as M
import pandepth_amd as pda

gpu = pytest.mark.gpu
TILE = M.TILE
WHOLE = ((0, M.N_TILES),)
FILL = 0xCD                                                         # partials are pre-filled: a tile nobody wrote shows


class Rig:
    """one context over M.GENOME, and the device copies of the case being swept"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.e = pda.Engine(M.GENOME)
        n_cells, n_sums = self.e.device_layout()
        off, n_model, _ = M.layout(M.GENOME)
        assert n_cells == n_model == M.N_CELLS and n_sums >= M.N_TILES
        assert np.array_equal(self.e.device_buffer()[2].astype(np.int64), off)
        self.n_sums = n_sums
        self.partials = torch.zeros(M.N_TILES * 24, dtype=torch.uint8, device=self.dev)
        self.loaded = None

    def close(self):
        self.e.close()

    def load(self, c):
        if self.loaded is c:
            return
        t = self.torch
        self.parts = t.from_numpy(np.ascontiguousarray(c.parts)).to(self.dev)
        self.blocks = t.from_numpy(np.ascontiguousarray(c.blocks).view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.counts = t.from_numpy(np.ascontiguousarray(c.counts, dtype=np.int32)).to(self.dev)
        sums = np.zeros(self.n_sums, dtype=np.int32)
        sums[:M.N_TILES] = c.tile_sums
        self.sums = t.from_numpy(sums).to(self.dev)
        t.cuda.synchronize()
        self.loaded = c

    def sweep(self, c, slices, w, min_dep, wrap_bits, exc=True, counts=True):
        """pd_slice_sweep_i4 over each slice into one partials buffer -> (TileParts of all tiles, windows of pd_gather_windows)"""
        self.load(c)
        self.partials.fill_(FILL)
        self.torch.cuda.synchronize()                               # the engine works on ITS stream
        stride = M.N_CELLS // 2
        for t0, tc in slices:
            self.e.slice_sweep_i4(self.parts.data_ptr() + t0 * (TILE // 2), c.n_parts, stride, t0, tc, self.sums.data_ptr(),
                                  self.blocks.data_ptr() if exc else 0, c.exc_stride, self.counts.data_ptr() if counts else 0,
                                  w, min_dep, wrap_bits, self.partials.data_ptr() + t0 * 24)
        self.e.synchronize()
        got = self.partials.cpu().numpy().view(M.PART_DTYPE).copy()
        woff, cover, tot = self.e.gather_windows(self.partials.data_ptr(), w)
        return got, woff, cover, tot


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    try:
        yield r
    finally:
        r.e.set_param("sweep_i4_fast", 1)
        r.close()


def _same_partials(got, ref, what):
    if np.array_equal(got, ref):
        return
    bad = np.nonzero(got != ref)[0]
    t = int(bad[0])
    raise AssertionError("%s: %d tiles differ, first tile %d: got %s, expected %s" % (what, bad.size, t, got[t], ref[t]))


def check(rig, c, w, min_dep, wrap_bits, slicings=(WHOLE, M.SLICES3), exc=True, counts=True):
    """both sweeps (sweep_i4_fast 1 and 0), one slice and three: partials and windows exactly equal to the model's"""
    ref = c.ref(0, M.N_TILES, w, min_dep, wrap_bits)
    cov_ref, tot_ref = M.fold_windows(ref, M.GENOME, w)
    cov_d, tot_d = M.windows_from_depth(c.depth & M.wrap_mask(wrap_bits), M.GENOME, w, min_dep)
    assert np.array_equal(cov_ref, cov_d) and np.array_equal(tot_ref, tot_d)
    try:
        for fast in (1, 0):
            rig.e.set_param("sweep_i4_fast", fast)                 # process-wide
            for slices in slicings:
                what = "%s w=%d min_dep=%d wrap=%d fast=%d slices=%d" % (c.name, w, min_dep, wrap_bits, fast, len(slices))
                ref_s = ref if len(slices) == 1 else np.concatenate([c.ref(t0, tc, w, min_dep, wrap_bits) for t0, tc in slices])
                got, woff, cover, tot = rig.sweep(c, slices, w, min_dep, wrap_bits, exc, counts)
                _same_partials(got, ref_s, what)
                assert np.array_equal(woff, M.window_offsets(M.GENOME, w)), what
                assert np.array_equal(cover, cov_ref) and np.array_equal(tot, tot_ref), what
    finally:
        rig.e.set_param("sweep_i4_fast", 1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. part counts: the bytes of the packed sums at their limit (16 parts at nibble 15: 240), the chunks of 16 beyond
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["sparse", "saturated"])
@pytest.mark.parametrize("n_parts", M.PART_COUNTS)
def test_part_counts(rig, n_parts, mode):
    c = M.case(mode, n_parts)
    for w in (8192, 10000, 8192 * 3, 10000000):
        for min_dep in (0, 1, 2):
            for wrap_bits in (0, 18):
                check(rig, c, w, min_dep, wrap_bits)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the depth gate of the packed kernels: a lane that starts at 60 000 or more is not theirs
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_parts", [1, 16])
@pytest.mark.parametrize("h", M.GATE_HEIGHTS)
def test_depth_gate_plateaus(rig, h, n_parts):
    c = M.case("plateau", n_parts, h)
    for w in (10000000, 8192 * 3):
        for min_dep in (0, 1, 2):
            for wrap_bits in (0, 16, 18):
                check(rig, c, w, min_dep, wrap_bits)


@gpu
@pytest.mark.parametrize("n_parts", [1, 16])
def test_climb_through_the_gate_in_each_quarter(rig, n_parts):
    """the packed kernel has finished 0, 1, 2, 3 quarters of a tile when it meets the depth it must hand over"""
    c = M.case("climb", n_parts)
    for w in (10000000, 8192 * 3):
        for min_dep in (0, 1, 2):
            for wrap_bits in (0, 16, 18):
                check(rig, c, w, min_dep, wrap_bits)


# ---------------------------------------------------------------------------------------------------------------------
# 3. wraps: both sides of `wrap_mask >= 0xFFFF`, depths that straddle 2^18 and 2^16
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_parts", [1, 16])
@pytest.mark.parametrize("h", M.WRAP_HEIGHTS)
def test_wrap(rig, h, n_parts):
    c = M.case("wrap", n_parts, h)
    for w in (10000000, 10000):
        for wrap_bits in (0, 15, 16, 18):
            for min_dep in (0, 1, 2):                               # 2: the per-cell path
                check(rig, c, w, min_dep, wrap_bits)


# ---------------------------------------------------------------------------------------------------------------------
# 4. depth exactly zero at single cells of a lane: the sad_u8 shortcut (b0 <= neg) and both halves of the packed walk
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_parts", [1, 16])
def test_touch_zero(rig, n_parts):
    c = M.case("touch-zero", n_parts)
    ref = c.ref(0, M.N_TILES, 10000000, 1, 0)
    for t, k in M.ZERO_TILES.items():
        assert int(ref[t]["c0"]) == TILE - 4                        # two lanes in each of two quarters lose one cell
    assert int(ref[5]["c0"]) == TILE
    for w in (10000000, 8192):
        for min_dep in (1, 0, 2):
            for wrap_bits in (0, 18):
                check(rig, c, w, min_dep, wrap_bits)


# ---------------------------------------------------------------------------------------------------------------------
# 5. exceptions
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["exceptions", "exception-counts", "flagged-between-plateaus"])
def test_exceptions(rig, name):
    c = M.case(name)
    for w in (10000000, 10000):
        for min_dep in (0, 1, 2):
            for wrap_bits in (0, 18):
                check(rig, c, w, min_dep, wrap_bits)


@gpu
def test_exceptions_without_counts_are_not_read(rig):
    """dev_exc_counts = NULL (with or without a block pointer): the parts alone"""
    c = M.case("exceptions").without_exceptions()
    for min_dep in (0, 1):
        check(rig, c, 10000, min_dep, 18, counts=False)
        check(rig, c, 10000000, min_dep, 0, exc=False, counts=False)


# ---------------------------------------------------------------------------------------------------------------------
# 6. full scratch lists behind the flags: every tile of a whole-buffer slice flagged, every tile handed over
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,w", [("every-tile-flagged", 10000), ("every-tile-flagged", 8193), ("every-tile-slow", 8193), ("every-tile-slow", 10000000)])
def test_full_lists(rig, name, w):
    c = M.case(name)
    for min_dep in (0, 1):
        for wrap_bits in (0, 18):
            check(rig, c, w, min_dep, wrap_bits, slicings=(WHOLE,))


# ---------------------------------------------------------------------------------------------------------------------
# the export side
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _export_i4(e, cap, with_block=True):
    """(image bytes, the whole exception buffer as entries incl. GUARD entries behind the block, count)"""
    import torch
    dev = torch.device("cuda", 0)
    n_cells, _ = e.device_layout()
    img = torch.full((n_cells // 2,), 0x5A, dtype=torch.uint8, device=dev)
    exc = torch.full(((cap + GUARD) * 16,), 0xA5, dtype=torch.uint8, device=dev)
    cnt = torch.full((1,), 0x7777, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.export_i4(img.data_ptr(), exc.data_ptr() if with_block else 0, cap, cnt.data_ptr())
    e.synchronize()
    return img.cpu().numpy(), exc.cpu().numpy().view(M.EXC_DTYPE).copy(), int(cnt.item())


def _sample_engine(iv, direct):
    e = pda.Engine(M.GENOME)
    e.keep_deferred(bool(direct))
    e.profile(True)
    e.push_intervals(iv, pda.PD_PUSH_SORTED | (pda.PD_PUSH_MORE if direct else 0))
    return e


def _entries(block):
    return sorted((int(x["cell"]), int(x["value"])) for x in block)


@gpu
@pytest.mark.parametrize("direct", [0, 1], ids=["arrays", "direct"])
def test_export_i4_byte_for_byte(direct):
    """differences of exactly -10 .. -7 and 7 .. 9 at the first and last cell of a tile, of a wave's 2048 cells and of a lane's 4:
    the image is pack_i4(the difference, or 0 where it is an exception), the exceptions are exactly the cells outside [-8, 7]"""
    iv, want = M.export_sample()
    D = M.diff_from_intervals(M.GENOME, iv)
    for cell, v in want.items():
        assert int(D[cell]) == v
    image = M.pack_i4(M.clip_or_zero(D))
    exc_ref = M.exception_set(D)
    with _sample_engine(iv, direct) as e:
        img, block, n = _export_i4(e, 1024)
        if direct:
            assert e.profile_get("direct_export")[1] == 1 and e.profile_get("export_i4")[1] == 0      # the image came from the tile windows
        assert n == len(exc_ref)
        assert np.array_equal(img, image), "image differs at bytes %s" % np.nonzero(img != image)[0][:8]
        untouched = np.add.reduceat(np.abs(D), np.arange(0, D.size, TILE // 2)) == 0                 # half-tiles nothing was ever written to
        assert untouched.sum() >= 10 and np.all(img.reshape(-1, TILE // 4)[untouched] == 0x88)
        assert _entries(block[:n]) == exc_ref
        assert np.all(block[:n]["pad"] == 0)
        assert np.all(block[n:].view(np.uint8) == 0xA5)


@gpu
@pytest.mark.parametrize("direct", [0, 1], ids=["arrays", "direct"])
def test_export_i4_capacity(direct):
    """one entry too few: the count is the full number, exactly `cap` genuine entries are written, nothing behind the block; no block at
    all: the image alone"""
    iv, _ = M.export_sample()
    D = M.diff_from_intervals(M.GENOME, iv)
    image = M.pack_i4(M.clip_or_zero(D))
    exc_ref = M.exception_set(D)
    cap = len(exc_ref) - 1
    with _sample_engine(iv, direct) as e:
        img, block, n = _export_i4(e, cap)
        assert n == len(exc_ref)
        got = _entries(block[:cap])
        assert len(set(got)) == cap and set(got) <= set(exc_ref)
        assert np.all(block[cap:].view(np.uint8) == 0xA5)
        assert np.array_equal(img, image)
    with _sample_engine(iv, direct) as e:
        img, block, n = _export_i4(e, 0, with_block=False)
        assert n == len(exc_ref) and np.array_equal(img, image)
        assert np.all(block.view(np.uint8) == 0xA5)


def _i8_sample(thr):
    iv, want = M.stacked_reads(values=(-(thr + 1), -thr, thr, thr + 1), positions=(0, 8191, 16 * 40, 16 * 90 + 15))
    rng = np.random.default_rng(thr)
    n = 2000
    beg = rng.integers(0, M.GENOME[1] // 2, n)
    bg = np.stack([np.ones(n, dtype=np.int64), beg, beg + rng.integers(1, 300, n)], axis=1).astype(np.int32)
    allv = np.concatenate([iv, bg])
    return allv[np.lexsort((allv[:, 1], allv[:, 0]))], want


@gpu
@pytest.mark.parametrize("world,thr", [(2, 63), (8, 15)])
def test_export_i8_at_the_threshold(world, thr):
    """differences of exactly +-thr and +-(thr + 1) at the edges of the kernel's 16-cell groups: bytes are d + thr, the exceptions are
    exactly the cells beyond the threshold"""
    import torch
    dev = torch.device("cuda", 0)
    assert thr == 127 // world
    iv, want = _i8_sample(thr)
    D = M.diff_from_intervals(M.GENOME, iv)
    for cell, v in want.items():
        assert int(D[cell]) == v
    assert {c % 16 for c in want} == {0, 15}
    exc_ref = M.exception_set(D, -thr, thr)
    cap = 256
    with pda.Engine(M.GENOME) as e:
        e.push_intervals(iv, pda.PD_PUSH_SORTED)
        i8 = torch.full((M.N_CELLS,), 0x5A, dtype=torch.uint8, device=dev)
        exc = torch.full(((cap + GUARD) * 16,), 0xA5, dtype=torch.uint8, device=dev)
        cnt = torch.full((1,), 0x7777, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.export_i8(thr, i8.data_ptr(), exc.data_ptr(), cap, cnt.data_ptr())
        e.synchronize()
        n = int(cnt.item())
        block = exc.cpu().numpy().view(M.EXC_DTYPE)
        assert n == len(exc_ref) and _entries(block[:n]) == exc_ref
        assert np.all(block[n:].view(np.uint8) == 0xA5)
        assert np.array_equal(i8.cpu().numpy().astype(np.int64), M.clip_or_zero(D, -thr, thr) + thr)


@gpu
@pytest.mark.parametrize("world,thr", [(2, 63), (8, 15)])
def test_import_i8_of_bytes_at_their_maximum(world, thr):
    """the sum of `world` images whose every byte is 2 * thr (no carry leaves a byte: 2 * thr * world <= 254), and a random one:
    cell = byte - world * thr, plus the exceptions"""
    import torch
    from tools import multi_torch as multi
    dev = torch.device("cuda", 0)
    top = 2 * thr * world
    assert top <= 254
    rng = np.random.default_rng(world)
    exc = np.zeros(3, dtype=M.EXC_DTYPE)
    exc[0], exc[1], exc[2] = (0, 1000, 0), (M.N_CELLS - 1, -1000, 0), (12345, 300000, 0)
    add = np.zeros(M.N_CELLS, dtype=np.int64)
    add[[0, M.N_CELLS - 1, 12345]] = [1000, -1000, 300000]
    for kind in ("maximum", "random"):
        with pda.Engine(M.GENOME) as e:
            if kind == "maximum":                                    # summed the way the collective does it: as int32 WORDS
                img = np.full(M.N_CELLS, top, dtype=np.uint8)
                one = torch.full((M.N_CELLS // 4,), 2 * thr * 0x01010101, dtype=torch.int32, device=dev)
                total = torch.zeros_like(one)
                for _ in range(world):
                    total += one
            else:
                img = rng.integers(0, top + 1, M.N_CELLS).astype(np.uint8)
                total = torch.from_numpy(img.view(np.int32).copy()).to(dev)
            assert np.array_equal(total.cpu().numpy().view(np.uint8), img)
            x = torch.from_numpy(exc.view(np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            e.import_i8(total.data_ptr(), world * thr, x.data_ptr(), 3)
            e.synchronize()
            cells = multi.buffer_view(e, dev)[:M.N_CELLS].cpu().numpy().astype(np.int64)
            assert np.array_equal(cells, img.astype(np.int64) - world * thr + add)


@gpu
def test_accumulate_from_packed_at_the_nibble_edges():
    """the source holds differences of exactly -10 .. -7 and 7 .. 9 (k_export_i4 -> k_add_i4 + exceptions): the destination cell by cell
    against the int32 transport and against the sum of the two difference arrays"""
    import torch
    from tools import multi_torch as multi
    dev = torch.device("cuda", 0)
    src_iv, want = M.export_sample()
    rng = np.random.default_rng(91)
    n = 20000
    tid = rng.integers(0, len(M.GENOME), n)
    L = np.asarray(M.GENOME, dtype=np.int64)[tid]
    beg = (rng.random(n) * (L + 40)).astype(np.int64) - 5
    dst_iv = np.stack([tid, beg, beg + rng.integers(0, 300, n)], axis=1).astype(np.int32)
    dst_iv = np.concatenate([dst_iv, np.tile(np.array([[0, 2 * TILE - 40, 2 * TILE]], dtype=np.int32), (9, 1))])   # -9 in the source meets -9 here
    D = M.diff_from_intervals(M.GENOME, src_iv) + M.diff_from_intervals(M.GENOME, dst_iv)
    assert int(D[2 * TILE]) == -18
    got = {}
    for packed in (1, 0):
        with pda.Engine(M.GENOME) as dst, pda.Engine(M.GENOME) as src:
            dst.set_param("accumulate_packed", packed)
            dst.profile(True)
            dst.push_intervals(dst_iv)
            src.push_intervals(src_iv, pda.PD_PUSH_SORTED)
            dst.accumulate_from(src)
            view = multi.buffer_view(dst, dev).cpu().numpy().astype(np.int64)
            got[packed] = view
            assert np.array_equal(view[:M.N_CELLS], D), "packed=%d: cells %s" % (packed, np.nonzero(view[:M.N_CELLS] != D)[0][:8])
            assert np.array_equal(view[M.N_CELLS:M.N_CELLS + M.N_TILES], D.reshape(-1, TILE).sum(axis=1))
    assert np.array_equal(got[1], got[0])
