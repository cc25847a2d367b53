"""CPU tests of tests/i4_model.py: the inputs that tests/test_gpu_sliced_edges.py feeds to the 4-bit image kernels have the
properties each case relies on, and the model's sweep agrees with the per-base oracle on a real sample."""
import numpy as np
import pytest

import i4_model as M

TILE = M.TILE


def test_layout_of_the_test_genome():
    off, n_cells, tile_contig = M.layout(M.GENOME)
    assert n_cells == 36 * TILE and tile_contig.size == 36
    for ln in (8192, 8191, 16384, 1, 3):
        assert ln in M.GENOME
    slots = np.diff(np.concatenate([off, [n_cells]]))
    assert slots[M.GENOME.index(8192)] == 2 * TILE              # len + 1 cells: a whole tile past the contig's end
    assert slots[M.GENOME.index(8191)] == TILE
    assert M.GENOME[0] % TILE not in (0, TILE - 1) and M.GENOME[0] > 3 * TILE      # several tiles and a ragged end


def test_pack_and_unpack():
    rng = np.random.default_rng(1)
    d = rng.integers(-8, 8, (3, 64))
    img = M.pack_i4(d)
    assert img.shape == (3, 32) and np.array_equal(M.unpack_i4(img), d)
    assert M.pack_i4([-8, 7])[0] == 0xF0 and M.pack_i4([0, 0])[0] == 0x88 and M.pack_i4([1, -1])[0] == 0x79
    with pytest.raises(AssertionError):
        M.pack_i4([8, 0])


def test_split_parts_edges():
    rng = np.random.default_rng(2)
    for n in (1, 2, 16, 33):
        D = np.array([-8 * n, 7 * n, 0, -1, 1, -8 * n + 1, 7 * n - 1] * 5)
        nib = M.split_parts(D, n, rng)
        assert nib.shape == (n, D.size)
        assert np.all(nib[:, 0] == 0) and np.all(nib[:, 1] == 15)
    with pytest.raises(AssertionError):
        M.split_parts(np.array([8]), 1, rng)


def test_nonneg_walk_keeps_increments_in_range():
    rng = np.random.default_rng(3)
    steps = rng.integers(-8, 8, 5000)
    T = M.nonneg_walk(steps)
    inc = np.diff(T, prepend=0)
    assert T.min() == 0 and inc.min() >= -8 and inc.max() <= 7


@pytest.mark.parametrize("key", M.all_case_keys(), ids=lambda k: "-".join(map(str, k)))
def test_case_has_the_properties_it_promises(key):
    c = M.case(*key)
    variants = [c] + ([c.without_exceptions()] if key == ("exceptions",) else [])
    for v in variants:
        assert v.nib.shape == (v.n_parts, M.N_CELLS) and v.nib.min() >= 0 and v.nib.max() <= 15
        assert np.array_equal(M.unpack_i4(v.parts), v.nib.astype(np.int64) - 8)
        assert v.depth.min() >= 0                                 # "a depth is never negative"
        assert v.depth.max() < 2 ** 31
        assert np.array_equal(np.cumsum(v.tile_sums.astype(np.int64)), v.depth[TILE - 1::TILE])
    p = c.props
    exc_tiles = c.exception_tiles()
    assert not (set(p["free_tiles"]) & exc_tiles)
    assert set(p["free_tiles"]) | exc_tiles == set(range(M.N_TILES))
    if p.get("saturated"):
        assert np.any(np.all(c.nib == 15, axis=0)) and np.any(np.all(c.nib == 0, axis=0))
        hi = np.nonzero(np.all(c.nib == 15, axis=0))[0]
        assert np.any(hi % 32 == 31) and np.any(hi % 32 == 0) and np.any(hi % 2048 == 2047) and np.any(hi % TILE == TILE - 1)
    if "bracket" in p:
        tiles, lo, hi = p["bracket"]
        assert set(tiles) <= set(p["free_tiles"])
        x = c.depth.reshape(-1, TILE)[list(tiles)]
        assert int(x.min()) == lo and int(x.max()) == hi
        for v in p.get("values", ()):
            assert np.any(x == v)
        if p["mode"] == "plateau":                                # held across at least three whole tiles
            assert len(tiles) >= 2 and all(np.all((c.depth.reshape(-1, TILE)[t] >= lo) & (c.depth.reshape(-1, TILE)[t] <= hi)) for t in tiles)
    for cell, d in p.get("exact", {}).items():
        assert int(c.depth[cell]) == d, (cell, int(c.depth[cell]), d)


def test_gate_cases_sit_on_the_sides_they_name():
    for n in (1, 16):
        for h in M.GATE_HEIGHTS:
            c = M.case("plateau", n, h)
            lane_first = c.depth.reshape(-1, 32)[:, -1]           # the depth before the first cell of the next lane
            b0 = lane_first[2 * 256 - 1:5 * 256 - 1]              # lanes of the tiles 2..4
            assert (b0.max() < 60000) == (h == 59990)
            assert (b0.min() >= 60000) == (h >= 60010)
        c = M.case("climb", n)
        for q in range(4):
            t = 2 + q
            b0 = np.concatenate([[c.depth[t * TILE - 1]], c.depth[t * TILE + 31:(t + 1) * TILE - 1:32]]).reshape(4, 64)
            over = (b0 >= 60000).any(axis=1)
            assert list(over) == [k == q for k in range(4)]       # the quarters before q are done when the tile is handed over
    c = M.case("wrap", 1, 262145)
    x = c.depth.reshape(-1, TILE)[[2, 3, 4]]
    assert np.any(x == 2 ** 18) and np.any(x == 2 ** 18 - 1) and int(x.min()) == 262140 and int(x.max()) == 262150
    x = M.case("wrap", 16, 65535).depth.reshape(-1, TILE)[[2, 3, 4]]
    assert np.any(x == 2 ** 16) and np.any(x == 2 ** 16 - 1) and int(x.min()) == 65530 and int(x.max()) == 65540
    x = M.case("plateau", 1, 65536).depth.reshape(-1, TILE)[[2, 3, 4]]
    assert np.any(x == 2 ** 16)


def test_touch_zero_lanes():
    for n in (1, 16):
        c = M.case("touch-zero", n)
        D = c.D
        cells = M.touch_zero_cells()
        assert len(cells) == 16 and {x % 32 for x in cells} == {0, 15, 16, 31}
        assert {(x % TILE) // 2048 for x in cells} == {0, 3} and {(x % 2048) // 32 for x in cells} == {0, 63}
        for x in cells:
            lane0 = x - x % 32
            b0 = int(c.depth[lane0 - 1])
            neg = int(-D[lane0:lane0 + 32][D[lane0:lane0 + 32] < 0].sum())
            assert b0 == 1 and neg == 1                           # b0 <= neg holds with equality
            assert int((c.depth[lane0:lane0 + 32] == 0).sum()) == 1
            q0 = lane0 - lane0 % 2048                             # no other lane of the wave's quarter decides the branch: b0 < neg nowhere
            for l in range(q0, q0 + 2048, 32):
                assert int(c.depth[l - 1]) >= int(-D[l:l + 32][D[l:l + 32] < 0].sum())
        lane0 = M.NEAR_LANE
        assert int(c.depth[lane0 - 1]) == 2 and int(-D[lane0:lane0 + 32][D[lane0:lane0 + 32] < 0].sum()) == 1
        assert c.depth[lane0:lane0 + 32].min() == 1


def test_exception_cases():
    c = M.case("exceptions")
    used = [(j, int(e["cell"]), int(e["value"])) for j in range(3) for e in c.blocks[j, :c.counts[j]]]
    cells = [x[1] for x in used]
    assert max(cells.count(x) for x in cells) == 3
    assert {1, -1, 300000, -300000} <= {x[2] for x in used}
    assert sum(1 for x in cells if x >= M.N_CELLS) == 3
    for t0, tc in M.SLICES3:
        for cell in (t0 * TILE, t0 * TILE + TILE - 1, (t0 + tc - 1) * TILE, (t0 + tc) * TILE - 1):
            assert cell in cells
    assert int(c.depth.max()) >= 300000 and int(c.without_exceptions().depth.max()) < 300000
    k = M.case("exception-counts")
    assert k.counts[1] < 0 and k.counts[2] > k.exc_stride and np.all(k.blocks[1]["value"] == 1000) and np.all(k.blocks[2]["value"] != 0)
    assert int(np.abs(k.D).max()) < 1000                          # nothing behind a count was added
    f = M.case("every-tile-flagged")
    assert f.exception_tiles() == set(range(M.N_TILES))
    s = M.case("every-tile-slow")
    assert s.depth[1000:].min() >= 61000 and not s.exception_tiles()
    b = M.case("flagged-between-plateaus")
    assert b.exception_tiles() == {1, 3, 7} and b.depth.reshape(-1, TILE)[[2, 3, 4]].min() >= 60997


def test_fold_equals_windows_straight_from_the_cells():
    for key in (("saturated", 2), ("exceptions",), ("plateau", 1, 70000)):
        c = M.case(*key)
        for w, min_dep, wrap in ((8192, 1, 0), (10000, 0, 18), (8193, 2, 16), (3 * 8192, 1, 15), (10000000, 1, 0)):
            whole = c.ref(0, M.N_TILES, w, min_dep, wrap)
            pieces = np.concatenate([c.ref(t0, tc, w, min_dep, wrap) for t0, tc in M.SLICES3])
            assert np.array_equal(whole, pieces)
            cov, tot = M.fold_windows(whole, M.GENOME, w)
            cov2, tot2 = M.windows_from_depth(c.depth & M.wrap_mask(wrap), M.GENOME, w, min_dep)
            assert np.array_equal(cov, cov2) and np.array_equal(tot, tot2)


def test_stacked_reads_give_the_differences_they_name():
    iv, want = M.export_sample()
    D = M.diff_from_intervals(M.GENOME, iv)
    assert set(want.values()) == set(M.EDGE_VALUES)
    for cell, v in want.items():
        assert int(D[cell]) == v
    pos = {c % TILE for c in want}
    assert {0, TILE - 1} <= pos and any(p % 2048 == 0 and p for p in pos) and any(p % 2048 == 2047 and p != TILE - 1 for p in pos)
    assert any(p % 4 == 0 and p % 2048 for p in pos) and any(p % 4 == 3 and p % 2048 != 2047 for p in pos)
    assert len(M.exception_set(D)) >= 4 * len(M.EDGE_POS)
    touched = np.add.reduceat(np.abs(D), np.arange(0, D.size, TILE // 2)) > 0
    assert (~touched).sum() >= 10                                 # never-written half-tiles


def test_sweep_ref_reproduces_windows_ref_on_a_real_sample():
    """the model against the per-base oracle (oracle/pd_oracle.c) and test_gpu_engine.py's own window reference"""
    import test_gpu_engine as G
    rng = np.random.default_rng(77)
    lens = G.LENS
    iv = np.concatenate([G.rand_intervals(rng, lens, 30000), np.tile(np.array([[1, 700, 900]], dtype=np.int32), (300, 1)),
                         np.tile(np.array([[0, 8190, 8200]], dtype=np.int32), (40, 1))])
    d, off = G.oracle_depth(lens, iv, True)
    D = M.diff_from_intervals(lens, iv)
    img = M.pack_i4(M.clip_or_zero(D))[None, :]
    exc = M.exception_set(D)
    assert len(exc) >= 4
    blocks = np.zeros((1, len(exc) + 3), dtype=M.EXC_DTYPE)
    for k, (cell, v) in enumerate(exc):
        blocks[0, k] = (cell, v, 0)
    n_tiles = D.size // TILE
    sums = D.reshape(-1, TILE).sum(axis=1)
    for w, min_dep in ((10000, 1), (8192, 3), (10000000, 1), (250000, 2)):
        parts = np.concatenate([M.sweep_ref(img[:, t0 * 4096:(t0 + tc) * 4096], blocks, [len(exc)], lens, t0, tc, w, min_dep, 18, sums)
                                for t0, tc in ((0, 50), (50, n_tiles - 50))])
        cov, tot = M.fold_windows(parts, lens, w)
        cov_ref, tot_ref = G.windows_ref(lens, d, off, w, min_dep)
        assert np.array_equal(cov, cov_ref) and np.array_equal(tot, tot_ref)
