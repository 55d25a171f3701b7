"""GPU tests of the frontier extension (dspmap_build_frontiers, its accessors and device buffers, dspmap_debug_set_known): exact parity --
zero differing integers -- with the numpy restatement (tests/frontier_ref.py), fed with the ages the known-space layer hands out
(DSPMap.known_age) and the layers of the cast grid as set (DSPMap.set_cast_grid).  The shapes, at 0.15 m with six horizons so that t selects
among layers that differ: 66 x 12 x 8 (two words per row, a ragged last word, the known/unknown border across the words), 16 x 16 x 6 (one
word), 3 x 3 x 3 (one partial wave) and 130 x 40 x 24 (2 880 word items and 124 800 cells: the ordered compaction's tile holds 256 items,
so the scan of the cells spans 12 workgroups and that of the blocks up to 488).

The scene: four accepted frames of the scaled wall cloud (update counter 4), a cast grid whose layer j is frontier_ref.scene(shape,
seed = 5 + j)'s occupancy, and the ages of frontier_ref.scene(shape) written cell by cell through dspmap_debug_set_known.  Before it
compares, every parity test asserts on the RESTATEMENT's output that the scene is not degenerate."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import frontier_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
RES = 0.15
WIDE, CUBE, TINY, BIG = (66, 12, 8), (16, 16, 6), (3, 3, 3), (130, 40, 24)
SHAPES = [WIDE, CUBE, TINY, BIG]
IDS = ["66x12x8", "16x16x6", "3x3x3", "130x40x24"]
S2 = float(np.sqrt(0.5))
QUATS = {"identity": (1.0, 0.0, 0.0, 0.0), "yaw90": (S2, 0.0, 0.0, S2), "yaw180": (0.0, 0.0, 0.0, 1.0)}
WALL_DIST = {WIDE: 4.0, CUBE: 0.9, TINY: 0.6, BIG: 4.0}
MAX_AGE = 2
T_BETWEEN, T_PAST = 0.1, 5.0                     # between the horizons 0.05 and 0.2; past the last (2.0)
TIMES = {-1.0: 0, 0.0: 1, T_BETWEEN: 2, T_PAST: 6}   # t -> the layer it selects
MOVED = (7.31, -2.2, 0.4)                        # a position whose window base is off zero on all three axes of WIDE, TINY and BIG


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cloud(dist, seed=3):
    return (common.wall_cloud(seed, n_side=40) * F(dist / 3.0)).astype(F)


def _map(dsp, shape, seed=7, **kw):
    return dsp.DSPMap(dsp.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12, seed=seed, **kw))


def _layers(shape, L):
    return np.stack([R.scene(shape, seed=5 + j)[0] for j in range(L)])


def _frames(dsp, shape, integrate=False):
    """four accepted frames of the scaled wall cloud (test_gpu_view's attitudes; integrate: its integrations, after frames 0, 1 and 3)"""
    m = _map(dsp, shape)
    pts = _cloud(WALL_DIST[shape])
    for f, quat in enumerate((QUATS["yaw90"], QUATS["yaw180"], QUATS["identity"], QUATS["identity"])):
        assert m.update(pts, (0.0, 0.0, 0.0), f / 30.0, quat) == 1
        if integrate and f != 2:
            m.integrate_known()
    return m


def _scene(dsp, shape):
    m = _frames(dsp, shape)
    lay = _layers(shape, m.T + 1)
    m.build_cast_grid(0.5, 0)
    m.set_cast_grid(R.pack(lay))
    m.set_known(R.scene(shape)[1])
    return m, lay


def _read(m):
    """everything a build gives, through the host accessors"""
    return m.frontier_grid(), m.frontier_cells(), m.frontier_blocks(), m.frontier_counts()


def _want(occ, age, max_age, mu, block):
    fr, u, free = R.frontier(occ, age, max_age, mu)
    return R.pack(fr), R.cells(fr), R.blocks(fr, u, block), (int(fr.sum()), None, int(free.sum()))


def _same(got, want, tag):
    grid, cells, blocks, counts = got
    wgrid, wcells, wblocks, wcounts = want
    assert grid.dtype == np.uint64 and grid.shape == wgrid.shape, tag
    bad = np.flatnonzero(grid != wgrid)
    assert bad.size == 0, (tag, "grid", bad.size, bad[:5])
    assert cells.dtype == np.int32 and cells.shape == wcells.shape, (tag, "cells", cells.shape, wcells.shape)
    bad = np.flatnonzero(cells != wcells)
    assert bad.size == 0, (tag, "cells", bad.size, bad[:5], cells[bad[:5]], wcells[bad[:5]])
    assert blocks.dtype == R.BLOCK_DTYPE and blocks.shape == wblocks.shape, (tag, "blocks", blocks.shape, wblocks.shape)
    for f in R.BLOCK_DTYPE.names:
        bad = np.flatnonzero(blocks[f] != wblocks[f])
        assert bad.size == 0, (tag, f, bad.size, bad[:5], blocks[bad[:5]], wblocks[bad[:5]])
    assert counts == (wcounts[0], len(wblocks), wcounts[2]), (tag, counts)


def _non_degenerate(shape, lay, age):
    """the conditions of the scene, on the restatement (layer 0, max_age = 2)"""
    nx = shape[0]
    both = False
    for mu in (1, 2, 4, 6):
        fr = R.frontier(lay[0], age, MAX_AGE, mu)[0]
        if mu != 6:
            assert fr.any(), (shape, mu)
            if nx > 64:
                assert fr[:, :, 63].sum() >= 5 and fr[:, :, 64].sum() >= 5, (shape, mu)
        words = R.pack(fr)
        both |= bool((words == 0).any() and (words != 0).any())
    assert both, shape                                                                # an empty and a non-empty word item
    if nx > 64:
        assert (age[:, 0::2, 63] >= 0).any() and (age[:, 0::2, 64] < 0).all() and (age[:, 1::2, 64] >= 0).any()   # the border crosses the word
    assert (age == 3).any() and (age == -1).any() and ((age >= 0) & (age <= MAX_AGE)).any()


def _device_copy(dsp, ptr, shape, typestr="<i4"):
    return torch.as_tensor(dsp.capi._DeviceSpan(ptr, shape, typestr), device="cuda").cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_frontiers_match_the_restatement(dsp, shape):
    """grid, cells, blocks and counts for every min_unknown x block x t; host accessors, device buffers and torch tensors agree; a
    small cap copies a prefix; a repeated build gives identical bytes"""
    m, lay = _scene(dsp, shape)
    age = m.known_age()
    assert np.array_equal(age, R.scene(shape)[1])                                     # set_known wrote what it was given
    _non_degenerate(shape, lay, age)
    nx, ny, nz = shape
    W = (nx + 63) // 64
    total = 0
    for t, layer in TIMES.items():
        for mu in (1, 2, 4, 6):
            fr, u, free = R.frontier(lay[layer], age, MAX_AGE, mu)
            wgrid, wcells, n_free = R.pack(fr), R.cells(fr), int(free.sum())
            for block in (1, 4, 5, 32):
                m.build_frontiers(t=t, max_age=MAX_AGE, min_unknown=mu, block=block)
                got = _read(m)
                _same(got, (wgrid, wcells, R.blocks(fr, u, block), (wcells.size, None, n_free)), (shape, t, mu, block))
                total += wcells.size
            # (block = 32 is the last build) the device side of the same snapshot
            n, k = got[3][0], got[3][1]
            assert np.array_equal(m.frontier_cells(device="cuda").cpu().numpy(), got[1])
            tb = m.frontier_blocks(device="cuda")
            assert tb.dtype == torch.int32 and tuple(tb.shape) == (k, 6)
            assert np.array_equal(tb.cpu().numpy(), got[2].view(np.int32).reshape(k, 6))
            L = m.L
            assert np.array_equal(_device_copy(dsp, L.dspmap_frontier_grid_device(m.h), (nz, ny, W), "<i8").view(np.uint64), got[0])
            assert tuple(_device_copy(dsp, L.dspmap_frontier_counts_device(m.h), (3,), "<i8")) == got[3]
            if n:
                assert np.array_equal(_device_copy(dsp, L.dspmap_frontier_cells_device(m.h), (n,)), got[1])
            # cap < n: a prefix, and still n
            cap, cnt = n // 2, C.c_int(-1)
            part = np.full(n + 1, -7, np.int32)
            assert L.dspmap_get_frontier_cells(m.h, cap, _p(part), C.byref(cnt)) == 1 and cnt.value == n
            assert np.array_equal(part[:cap], got[1][:cap]) and (part[cap:] == -7).all()
            capb, partb = k // 2, np.full(k + 1, -7, R.BLOCK_DTYPE)
            assert L.dspmap_get_frontier_blocks(m.h, capb, _p(partb), C.byref(cnt)) == 1 and cnt.value == k
            assert np.array_equal(partb[:capb], got[2][:capb]) and (partb["count"][capb:] == -7).all()
            np.testing.assert_array_equal(m.frontier_block_centers(), R.centers(got[2], shape, RES))
    assert total > 0
    # order does not depend on atomic arrival: the same build again gives the same bytes, also after another one in between
    m.build_frontiers(t=T_BETWEEN, max_age=MAX_AGE, min_unknown=1, block=4)
    first = _read(m)
    m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=2, block=1)
    for _ in range(2):
        m.build_frontiers(t=T_BETWEEN, max_age=MAX_AGE, min_unknown=1, block=4)
        again = _read(m)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    # the block sums added per cell instead of per (wave, block): integer sums, the same bytes
    m.set_param(dsp.capi.P_FRONTIER_MERGE, 0)
    for block in (1, 5, 32):
        m.build_frontiers(t=T_BETWEEN, max_age=MAX_AGE, min_unknown=1, block=block)
        _same(_read(m), _want(lay[2], age, MAX_AGE, 1, block), (shape, "per-cell atomics", block))
    m.set_param(dsp.capi.P_FRONTIER_MERGE, 1)
    # max_age decides: 0 knows only the newest stamps, 3 knows every stamped cell
    for max_age in (0, 3):
        m.build_frontiers(t=-1.0, max_age=max_age, min_unknown=1, block=4)
        _same(_read(m), _want(lay[0], age, max_age, 1, 4), (shape, "max_age", max_age))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, TINY, BIG], ids=["66x12x8", "3x3x3", "130x40x24"])
def test_frontiers_in_a_moved_window(dsp, shape):
    """the window base off zero on all three axes: a neighbour lookup that forgets the wrap of a toroidal axis fails only here"""
    from tests import known_ref as K
    m, lay = _scene(dsp, shape)
    m.set_current_position(*MOVED)
    k0, _ = K.window(m.cfg, MOVED)
    assert all(k % n != 0 for k, n in zip(k0, shape)), k0
    age = R.scene(shape)[1]
    m.set_known(age)
    assert np.array_equal(m.known_age(), age)                                         # through the slot mapping and back
    _non_degenerate(shape, lay, age)
    for t, mu, block in ((-1.0, 1, 4), (0.0, 2, 5), (T_PAST, 4, 1), (T_BETWEEN, 1, 32)):
        m.build_frontiers(t=t, max_age=MAX_AGE, min_unknown=mu, block=block)
        _same(_read(m), _want(lay[TIMES[t]], age, MAX_AGE, mu, block), (shape, "moved", t, mu, block))
    # a step of one cell along x: the cells that entered the window are unknown, the others keep their ages one voxel further
    step = (MOVED[0] + RES, MOVED[1], MOVED[2])
    m.set_current_position(*step)
    assert K.window(m.cfg, step)[0][0] == k0[0] + 1
    moved = np.full_like(age, -1)
    moved[:, :, :-1] = age[:, :, 1:]
    assert np.array_equal(m.known_age(), moved)
    m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=1, block=4)
    _same(_read(m), _want(lay[0], moved, MAX_AGE, 1, 4), (shape, "stepped"))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE], ids=["66x12x8", "16x16x6"])
def test_frontiers_of_a_real_layer_and_a_masked_grid(dsp, shape):
    """the layer three real integrations leave (ages -1, 0, 2, 3), no set_known; and the grid masked with the same max_age, whose frontier
    set is that of the unmasked grid: a known cell keeps its bit, and unknown is decided by age alone"""
    m = _frames(dsp, shape, integrate=True)
    lay = _layers(shape, m.T + 1)
    m.build_cast_grid(0.5, 0)
    m.set_cast_grid(R.pack(lay))
    age = m.known_age()
    assert set(np.unique(age)) >= {-1, 0} and ((age >= 0) & (age <= MAX_AGE)).any() and (age > MAX_AGE).any()
    assert R.frontier(lay[0], age, MAX_AGE, 1)[0].sum() >= 10                         # the restatement finds a frontier
    plain = {}
    for t, mu, block in ((-1.0, 1, 4), (T_BETWEEN, 2, 5), (T_PAST, 1, 1)):
        m.build_frontiers(t=t, max_age=MAX_AGE, min_unknown=mu, block=block)
        plain[t] = _read(m)
        _same(plain[t], _want(lay[TIMES[t]], age, MAX_AGE, mu, block), (shape, "real", t, mu, block))
    m.mask_cast_grid(MAX_AGE)
    masked = m.cast_grid()
    unknown = (age < 0) | (age > MAX_AGE)
    assert np.array_equal(masked, R.pack(lay | unknown)) and not np.array_equal(masked, R.pack(lay))
    for t, mu, block in ((-1.0, 1, 4), (T_BETWEEN, 2, 5), (T_PAST, 1, 1)):
        m.build_frontiers(t=t, max_age=MAX_AGE, min_unknown=mu, block=block)
        got = _read(m)
        _same(got, _want((lay | unknown)[TIMES[t]], age, MAX_AGE, mu, block), (shape, "masked", t, mu, block))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], plain[t][:3])) and got[3] == plain[t][3]
    m.close()


def _stale(m):
    L = m.L
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    cnt, n = (C.c_longlong * 3)(), C.c_int(0)
    words = np.zeros((m.cfg.nz, m.cfg.ny, (m.cfg.nx + 63) // 64), np.uint64)
    buf = np.zeros(64, R.BLOCK_DTYPE)
    assert L.dspmap_frontier_counts(m.h, cnt) == E_STATE and b"dspmap_build_frontiers" in err()
    assert L.dspmap_get_frontier_grid(m.h, _p(words)) == E_STATE and b"dspmap_build_frontiers" in err()
    assert L.dspmap_get_frontier_cells(m.h, 64, _p(buf), C.byref(n)) == E_STATE and b"dspmap_build_frontiers" in err()
    assert L.dspmap_get_frontier_blocks(m.h, 64, _p(buf), C.byref(n)) == E_STATE and b"dspmap_build_frontiers" in err()
    for fn in (L.dspmap_frontier_grid_device, L.dspmap_frontier_cells_device, L.dspmap_frontier_blocks_device, L.dspmap_frontier_counts_device):
        assert not fn(m.h)
    return True


def _fresh(m):
    L = m.L
    assert all(fn(m.h) for fn in (L.dspmap_frontier_grid_device, L.dspmap_frontier_cells_device, L.dspmap_frontier_blocks_device,
                                  L.dspmap_frontier_counts_device))
    return m.frontier_counts()


def test_frontier_life_cycle(dsp):
    m, lay = _scene(dsp, CUBE)
    age = R.scene(CUBE)[1]
    build = lambda: m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=1, block=4)   # noqa: E731
    assert _stale(m)                                                                  # never built
    build()
    want = _want(lay[0], age, MAX_AGE, 1, 4)
    assert _fresh(m) == (want[3][0], len(want[2]), want[3][2])
    pts = _cloud(WALL_DIST[CUBE])
    grid = R.pack(lay)
    triggers = [("build_cast_grid", lambda: (m.build_cast_grid(0.5, 0), m.set_cast_grid(grid))),
                ("mask_cast_grid", lambda: (m.mask_cast_grid(MAX_AGE), m.set_cast_grid(grid))),
                ("set_cast_grid", lambda: m.set_cast_grid(grid)),
                ("known_integrate", lambda: (m.integrate_known(), m.set_known(age))),
                ("known_reset", lambda: (m.reset_known(), m.set_known(age))),
                ("set_known", lambda: m.set_known(age)),
                ("set_current_position", lambda: m.set_current_position(0.0, 0.0, 0.0))]
    for name, fn in triggers:
        fn()
        assert _stale(m), name
        build()
        _same(_read(m), want, name)                                                   # (every trigger restored the scene)
    # a smaller block after a larger one: the block buffers grow
    m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=1, block=32)
    _same(_read(m), _want(lay[0], age, MAX_AGE, 1, 32), "block 32")
    m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=1, block=1)
    _same(_read(m), _want(lay[0], age, MAX_AGE, 1, 1), "block 1 after 32")
    # what makes the cast grid stale: a frame
    assert m.update(pts, (0.0, 0.0, 0.0), 0.2, QUATS["identity"]) == 1
    assert _stale(m)
    L = m.L
    assert L.dspmap_build_frontiers(m.h, -1.0, MAX_AGE, 1, 4, 0) == E_STATE and b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
    # a grid, but a layer without an integration since its reset
    m.build_cast_grid(0.5, 0)
    m.reset_known()
    assert L.dspmap_build_frontiers(m.h, -1.0, MAX_AGE, 1, 4, 0) == E_STATE and b"dspmap_known_integrate" in L.dspmap_last_error(m.h)
    # set_known's range follows the counter (5 now)
    bad = age.copy()
    bad[0, 0, 0] = 5
    assert L.dspmap_debug_set_known(m.h, _p(bad)) == -1 and b"outside" in L.dspmap_last_error(m.h)
    bad[0, 0, 0] = -2
    assert L.dspmap_debug_set_known(m.h, _p(bad)) == -1
    bad[0, 0, 0] = 4
    m.set_known(bad)
    assert np.array_equal(m.known_age(), bad)
    m.close()
    fresh = _map(dsp, CUBE)                                                           # a grid needs no frame; the layer's hook does
    fresh.build_cast_grid(0.5, 0)
    assert fresh.L.dspmap_debug_set_known(fresh.h, _p(age)) == E_STATE and b"no frame" in fresh.L.dspmap_last_error(fresh.h)
    assert fresh.L.dspmap_build_frontiers(fresh.h, -1.0, MAX_AGE, 1, 4, 0) == E_STATE and b"dspmap_known_integrate" in fresh.L.dspmap_last_error(fresh.h)
    fresh.close()


def test_frontier_build_is_read_only(dsp):
    """twins: one builds frontiers between the frames, the other never does; map, grid, layer, counters and the next frame are the same"""
    twins = []
    for _ in range(2):
        m = _map(dsp, CUBE, seed=99)
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        twins.append(m)
    a, b = twins
    pts = [_cloud(0.6, seed=s) for s in range(5)]
    found = 0
    for f in range(4):
        cur = (0.03 * f, -0.02 * f, 0.0)
        for m in (a, b):
            assert m.update(pts[f], cur, f / 30.0, QUATS[("identity", "yaw90", "yaw180")[f % 3]]) == 1
            m.integrate_known(max_range=0.8)
            m.build_cast_grid(0.05, 1)
        state = (a.results(), b.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors())   # (getFutureStatus is a consuming readout: the twin's is the "before")
        ca = a.counters()
        for t, mu, block in ((-1.0, 1, 4), (T_BETWEEN, 2, 1), (T_PAST, 1, 32)):
            a.build_frontiers(t=t, max_age=MAX_AGE, min_unknown=mu, block=block)
            got = _read(a)
            _same(got, _want(CR_unpack(state[2][TIMES[t]], CUBE[0]), state[3], MAX_AGE, mu, block), ("twin", f, t))
            found += got[3][0]
        after = (a.results(), a.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors())
        for x, y in zip(state[:4], after[:4]):
            assert np.array_equal(x, y)
        assert state[4] == after[4]
        cb = a.counters()
        ca.pop("update_ms"), cb.pop("update_ms")
        assert ca == cb
        assert a.cast_grid_ptr() is not None                                          # nothing else went stale
    assert found > 0
    for m in (a, b):
        assert m.update(pts[4], (0.1, 0.0, 0.0), 0.2, QUATS["identity"]) == 1
    assert np.array_equal(a.results(), b.results()) and (a.results()[:, 0] > 0).any()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    ca, cb = a.counters(), b.counters()
    ca.pop("update_ms"), cb.pop("update_ms")
    assert ca == cb and a.cursors() == b.cursors()
    assert np.array_equal(a.known_age(), b.known_age())
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    a.close(), b.close()


def CR_unpack(words, nx):
    """uint64 [nz, ny, W] -> bool [nz, ny, nx]"""
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :nx].astype(bool)
