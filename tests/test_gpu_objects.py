"""GPU tests of the objects extension (dspmap_build_objects, its accessors, device buffers and queries): exact parity -- zero differing
integers in records (per field), label grid and counts -- with the numpy restatement (tests/objects_ref.py), fed with the layers of the
cast grid as set (DSPMap.set_cast_grid) and the result grid as read back (DSPMap.results), which is the feature's input.  The shapes, at
0.15 m with six horizons and 12 particles per voxel: 66 x 12 x 8 (two words per row, a ragged last word, components across the word edge),
16 x 16 x 6 (one word), 3 x 3 x 3 (one partial wave) and 130 x 40 x 24 (2 880 word items, 124 800 cells: the compaction spans 488 tiles).

The scene: layer j of the grid is objects_ref.scene(shape, seed = 11 + j) -- a serpentine in plane 0 that the smallest index has to
travel, an empty plane, random planes above.  Mass and velocity come from two handles: four accepted frames of the scaled wall cloud, and
a handle seeded with moving particles (seed_uniform with vmax > 0, then occupancy_resample) whose velocities are not zero.  Before it
compares, every parity test asserts on the RESTATEMENT's output that the scene is not degenerate.  No test provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import objects_ref as R
from tests.test_gpu_frontier import BIG, CUBE, IDS, MOVED, QUATS, RES, SHAPES, TINY, WALL_DIST, WIDE, CR_unpack, _cloud, _device_copy, _frames, _map, _p
from tests.test_objects_cpu import lab_of

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
T_BETWEEN, T_PAST = 0.1, 5.0
TIMES = {-1.0: 0, T_BETWEEN: 2, T_PAST: 6}      # t -> the layer it selects
MAX_AGE = 2


def _layers(shape, L):
    return np.stack([R.scene(shape, seed=11 + j) for j in range(L)])


def _with_grid(m, shape):
    lay = _layers(shape, m.T + 1)
    m.build_cast_grid(0.5, 0)
    m.set_cast_grid(R.pack(lay))
    return m, lay


def _scene(dsp, shape):
    """the four wall-cloud frames, then the grid"""
    return _with_grid(_frames(dsp, shape), shape)


def _moving(dsp, shape):
    """a handle whose voxels hold moving particles, then the grid"""
    m = _map(dsp, shape, seed=99)
    m.set_tables(*common.tables(5))
    m.seed_uniform(2, 0.01, 17, vmax=0.8)
    m.occupancy_resample()
    return _with_grid(m, shape)


def _read(m):
    """everything a build gives, through the host accessors"""
    return m.objects(), m.object_labels(), m.object_counts()


def _same(got, want, tag):
    rec, grid, counts = got
    wrec, wgrid, wcounts = want
    print(tag, "counts", counts, "records", len(rec))
    assert counts == wcounts, (tag, counts, wcounts)
    assert rec.dtype == R.OBJECT_DTYPE and rec.shape == wrec.shape, (tag, rec.shape, wrec.shape)
    for f in R.OBJECT_DTYPE.names:
        diff = rec[f] != wrec[f]
        bad = np.flatnonzero(diff.any(1) if diff.ndim > 1 else diff)
        assert bad.size == 0, (tag, f, bad.size, bad[:5], rec[bad[:5]], wrec[bad[:5]])
    assert grid.dtype == np.int32 and grid.shape == wgrid.shape, tag
    bad = np.flatnonzero(grid != wgrid)
    assert bad.size == 0, (tag, "label grid", bad.size, bad[:5], grid.ravel()[bad[:5]], wgrid.ravel()[bad[:5]])


def _want(shape, layer, occ, res, conn, min_cells, max_objects=1 << 20):
    """the restatement; the components of the scene's own layers are computed once per session (tests.test_objects_cpu.lab_of)"""
    lab = lab_of(shape, conn, 11 + layer) if layer is not None else None
    return R.objects(occ, res, conn, min_cells, max_objects, lab=lab)


def _non_degenerate(shape, lay, res, moving):
    """the conditions of the scene, on the restatement"""
    nx = shape[0]
    q = R.contributions(res)
    for layer in TIMES.values():
        occ = lay[layer]
        s6, s26 = R.summary(lab_of(shape, 6, 11 + layer)), R.summary(lab_of(shape, 26, 11 + layer))
        assert s6[0] >= 2 and s26[0] >= 2, (shape, layer)                         # at least two components
        if shape != TINY:                                                         # (27 cells hold neither singles nor two partitions)
            assert s6[2] > 0 and s26[2] > 0 and 0 < s6[3] < s6[0] and 0 < s26[3] < s26[0], (shape, layer)   # singles, filtered at min_cells = 4
            assert s6[0] > s26[0], (shape, layer)                                 # the 6- and 26-partitions differ
        if nx > 64:
            both = occ[:, :, 63] & occ[:, :, 64]
            l6 = lab_of(shape, 6, 11 + layer)
            assert both.sum() >= 5 and (l6[:, :, 63][both] == l6[:, :, 64][both]).all(), (shape, layer)   # a component crosses x = 63 | 64
        on = q[occ.ravel()]
        if moving or shape != TINY:                                               # (the frames' wall lies outside a 0.45 m map)
            assert (on[:, 0] > 0).any(), (shape, layer)                           # some set cell adds mass
        if moving:
            assert (on[:, 1:] != 0).any(), (shape, layer)                         # ... and momentum


@pytest.mark.parametrize("handle", ["frames", "moving"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_objects_match_the_restatement(dsp, shape, handle):
    """records, label grid and counts for connectivity x min_cells x t; the device buffers equal the host copies; a small cap copies a
    prefix; a repeated build gives identical bytes"""
    m, lay = (_moving if handle == "moving" else _scene)(dsp, shape)
    res = m.results()
    assert np.array_equal(CR_unpack(m.cast_grid(), shape[0]), lay)                    # set_cast_grid wrote what it was given
    print(shape, handle, "cells with mass", int((res[:, 0] > 0).sum()), "with velocity", int((res[:, 1:] != 0).any(1).sum()), "max mass", float(res[:, 0].max()))
    _non_degenerate(shape, lay, res, handle == "moving")
    nx, ny, nz = shape
    V = nx * ny * nz
    L = m.L
    for t, layer in TIMES.items():
        for conn in (6, 26):
            for min_cells in (1, 4):
                m.build_objects(t=t, connectivity=conn, min_cells=min_cells, max_objects=V)
                got = _read(m)
                _same(got, _want(shape, layer, lay[layer], res, conn, min_cells), (shape, handle, t, conn, min_cells))
            # (min_cells = 4 is the last build) the device side of the same snapshot
            rec, grid, counts = got
            k = len(rec)
            tr = m.objects(device="cuda")
            assert tr.dtype == torch.int32 and tuple(tr.shape) == (k, 22)
            assert np.array_equal(tr.cpu().numpy(), rec.view(np.int32).reshape(k, 22))
            assert np.array_equal(m.object_labels(device="cuda").cpu().numpy(), grid)
            assert tuple(_device_copy(dsp, L.dspmap_object_counts_device(m.h), (4,), "<i8")) == counts + (0,)   # (the fault word is 0)
            assert np.array_equal(_device_copy(dsp, L.dspmap_object_labels_device(m.h), (nz, ny, nx)), grid)
            if k:
                assert np.array_equal(_device_copy(dsp, L.dspmap_objects_device(m.h), (k, 22)), rec.view(np.int32).reshape(k, 22))
            # cap < k: a prefix, and still k
            cap, cnt = k // 2, C.c_int(-1)
            part = np.full(k + 1, -7, R.OBJECT_DTYPE)
            assert L.dspmap_get_objects(m.h, cap, _p(part), C.byref(cnt)) == 1 and cnt.value == k
            assert np.array_equal(part[:cap], rec[:cap]) and (part["count"][cap:] == -7).all()
            # what a planner takes from the records
            for a, b in zip(m.object_states(rec), R.states(rec, shape, RES)):
                np.testing.assert_array_equal(a, b)
    # sums do not depend on atomic arrival: the same build again gives the same bytes, also after another one in between
    m.build_objects(t=T_BETWEEN, connectivity=26, min_cells=1, max_objects=V)
    first = _read(m)
    m.build_objects(t=-1.0, connectivity=6, min_cells=4, max_objects=V)
    for _ in range(2):
        m.build_objects(t=T_BETWEEN, connectivity=26, min_cells=1, max_objects=V)
        again = _read(m)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:2], again[:2])) and first[2] == again[2]
    m.close()


PADDED = (18, 14, 6)      # 4 x 4 x 4 cubes padded on all three axes


def _moving_stored(dsp, shape, tiling):
    """_moving under a chosen storage order (DSPMAP_P_TILING: 1 = 4 x 4 x 4 cubes, 0 = runs in index order), read back after the first use"""
    m = _map(dsp, shape, seed=99)
    m.set_param(dsp.capi.P_TILING, tiling)
    m.set_tables(*common.tables(5))
    m.seed_uniform(2, 0.01, 17, vmax=0.8)
    m.occupancy_resample()
    assert int(m.get_param(dsp.capi.P_TILING)) == tiling
    return _with_grid(m, shape)


@pytest.mark.parametrize("shape", [WIDE, PADDED], ids=["66x12x8", "18x14x6"])
def test_objects_under_cube_storage(dsp, shape):
    """k_objects_accumulate reads mass and momentum through lv_of_true: records, label grid and counts under cube storage equal the
    restatement fed with that handle's results(), and the records equal, byte for byte, those of a twin in index order"""
    (cubes, lay), (runs, lay_r) = _moving_stored(dsp, shape, 1), _moving_stored(dsp, shape, 0)
    res = cubes.results()
    assert np.array_equal(res, runs.results()) and np.array_equal(lay, lay_r)
    assert np.array_equal(CR_unpack(cubes.cast_grid(), shape[0]), lay)
    _non_degenerate(shape, lay, res, True)
    V = shape[0] * shape[1] * shape[2]
    for t, layer in TIMES.items():
        for conn in (6, 26):
            for min_cells in (1, 4):
                got = []
                for m in (cubes, runs):
                    m.build_objects(t=t, connectivity=conn, min_cells=min_cells, max_objects=V)
                    got.append(_read(m))
                want = _want(shape, layer, lay[layer], res, conn, min_cells)
                assert len(want[0]) > 0 and (want[0]["mass_q"] > 0).any() and (want[0]["mom_q"] != 0).any()   # records that carry mass and momentum
                _same(got[0], want, (shape, "cubes", t, conn, min_cells))
                assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes() and got[0][2] == got[1][2]
    assert int(cubes.get_param(dsp.capi.P_TILING)) == 1 and int(runs.get_param(dsp.capi.P_TILING)) == 0
    cubes.close(), runs.close()


@pytest.mark.parametrize("shape", [WIDE, BIG], ids=["66x12x8", "130x40x24"])
def test_max_objects_cuts_the_list_not_the_counts_or_the_grid(dsp, shape):
    m, lay = _moving(dsp, shape)
    res = m.results()
    for conn, min_cells, cap in ((6, 1, 7), (26, 1, 5), (6, 4, 1), (26, 4, 3)):
        full = _want(shape, 0, lay[0], res, conn, min_cells)
        assert full[2][0] > cap                                                        # the restatement finds more than the cap
        m.build_objects(t=-1.0, connectivity=conn, min_cells=min_cells, max_objects=cap)
        got = _read(m)
        _same(got, _want(shape, 0, lay[0], res, conn, min_cells, cap), (shape, "cap", conn, min_cells, cap))
        assert len(got[0]) == cap and got[2] == full[2] and got[1].max() == full[2][0] - 1 >= cap   # ordinals past the cap stay in the grid
        assert np.array_equal(got[0], full[0][:cap])
    # a larger max_objects after a smaller one: the record buffer grows
    m.build_objects(t=-1.0, connectivity=6, min_cells=1, max_objects=1 << 20)
    _same(_read(m), _want(shape, 0, lay[0], res, 6, 1), (shape, "grown"))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE], ids=["66x12x8", "16x16x6"])
def test_objects_of_an_inflated_and_a_masked_grid(dsp, shape):
    """the grid a build leaves (inflated by one voxel), then the same grid masked with the known-space layer: labelled as they are"""
    m = _frames(dsp, shape, integrate=True)
    res = m.results()
    mass = res[:, 0]
    assert (mass > 0).sum() >= 10
    m.build_cast_grid(float(np.quantile(mass[mass > 0], 0.7)), 1)                      # the heaviest 30 % of the voxels that hold mass, inflated
    seen = {}
    for name in ("inflated", "masked"):
        if name == "masked":
            m.mask_cast_grid(MAX_AGE)
        occ = CR_unpack(m.cast_grid(), shape[0])
        seen[name] = occ
        assert occ[0].any() and not occ[0].all(), name
        for t, layer in TIMES.items():
            for conn, min_cells in ((6, 1), (26, 2)):
                m.build_objects(t=t, connectivity=conn, min_cells=min_cells, max_objects=4096)
                _same(_read(m), _want(shape, None, occ[layer], res, conn, min_cells, 4096), (shape, name, t, conn, min_cells))
    assert not np.array_equal(seen["inflated"], seen["masked"])
    m.close()


@pytest.mark.parametrize("shape", [WIDE, TINY, BIG], ids=["66x12x8", "3x3x3", "130x40x24"])
def test_empty_and_full_layers(dsp, shape):
    m, lay = _moving(dsp, shape)
    res = m.results()
    lay = lay.copy()
    lay[0] = False
    lay[1] = True
    m.set_cast_grid(R.pack(lay))
    nx, ny, nz = shape
    V = nx * ny * nz
    for conn in (6, 26):
        m.build_objects(t=-1.0, connectivity=conn, min_cells=1, max_objects=16)
        rec, grid, counts = _read(m)
        assert counts == (0, 0, 0) and len(rec) == 0 and (grid == -1).all()
        assert tuple(m.objects(device="cuda").shape) == (0, 22)
        lab = R.components(lay[1], conn)
        assert (lab == 0).all()
        for min_cells in (1, V, V + 1):
            m.build_objects(t=0.0, connectivity=conn, min_cells=min_cells, max_objects=16)
            got = _read(m)
            _same(got, R.objects(lay[1], res, conn, min_cells, 16, lab=lab), (shape, "full", conn, min_cells))
            assert got[2] == (int(min_cells <= V), 1, V)
        rec = R.objects(lay[1], res, conn, 1, lab=lab)[0]
        assert rec["count"][0] == V and rec["label"][0] == 0 and rec["sum_x"][0] == ny * nz * nx * (nx - 1) // 2 and rec["mass_q"][0] > 0
    m.close()


def _samples(m, shape, seed):
    """samples inside, on voxel faces, outside the map and with NaN coordinates, float32 [n, 4]"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    half = np.array([nx, ny, nz], np.float64) * RES / 2.0
    q = np.zeros((400, 4), F)
    q[:, :3] = rng.uniform(-half * 1.15, half * 1.15, (400, 3))
    for i in range(100):                                   # on voxel faces: a lattice plane per axis in turn
        ax = i % 3
        q[i, ax] = F(-half[ax] + RES * rng.integers(0, (nx, ny, nz)[ax] + 1))
    q[100:110, 0] = np.nan
    q[110:115, 2] = np.nan
    q[:, 3] = rng.uniform(-1.0, 3.0, 400)                  # t is ignored
    return q


def _want_query(m, q, grid, cur=None):
    out = np.full(len(q), -1, np.int32)
    flat = grid.ravel()
    for i, s in enumerate(q):
        p = s[:3] if cur is None else (s[:3] - np.asarray(cur, F)).astype(F)   # fl(q - current position) per axis
        if np.isnan(p).any():
            continue
        ok, idx = m.getPointVoxelsIndexPublic(float(p[0]), float(p[1]), float(p[2]))
        if ok:
            out[i] = flat[idx]
    return out


@pytest.mark.parametrize("shape", [WIDE, TINY], ids=["66x12x8", "3x3x3"])
def test_query_objects(dsp, shape):
    m, lay = _moving(dsp, shape)
    m.build_objects(t=-1.0, connectivity=26, min_cells=1, max_objects=3)
    grid = m.object_labels()
    assert grid.max() >= 3 or shape == TINY                                            # ordinals past max_objects are answered too
    q = _samples(m, shape, 3)
    want = _want_query(m, q, grid)
    assert (want >= 0).any() and (want == -1).any()
    assert np.array_equal(m.query_objects(q), want)
    qd = torch.as_tensor(q, device="cuda")
    got = m.query_objects(qd)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    # world frame: the samples are taken relative to the current position, which a build does not depend on
    m.set_current_position(*MOVED)
    assert m.L.dspmap_object_labels_device(m.h)
    qw = q.copy()
    qw[:, :3] += np.asarray(MOVED, F)
    want_w = _want_query(m, qw, grid, MOVED)
    assert (want_w >= 0).any()
    assert np.array_equal(m.query_objects(qw, world=True), want_w)
    assert np.array_equal(m.query_objects(torch.as_tensor(qw, device="cuda"), world=True).cpu().numpy(), want_w)
    assert np.array_equal(m.query_objects(q), want)                                    # the map frame does not move
    assert m.query_objects(np.zeros((0, 4), F)).shape == (0,)
    m.close()


OTHERS = ["dspmap_distance_field_device", "dspmap_cast_grid_device", "dspmap_reach_fields_device", "dspmap_reach_timeline_device",
          "dspmap_forecast_device", "dspmap_frontier_grid_device"]
MINE = ["dspmap_objects_device", "dspmap_object_labels_device", "dspmap_object_counts_device"]
SRC = np.array([[0.0, 0.0, 0.0, 0]], np.float64)


def _gone(m):
    L = m.L
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    cnt, n = (C.c_longlong * 3)(), C.c_int(0)
    buf = np.zeros(8, R.OBJECT_DTYPE)
    grid = np.zeros(m.cfg.nx * m.cfg.ny * m.cfg.nz, np.int32)
    q = np.zeros((2, 4), F)
    out = np.zeros(2, np.int32)
    assert L.dspmap_object_counts(m.h, cnt) == E_STATE and b"dspmap_build_objects" in err()
    assert L.dspmap_get_objects(m.h, 8, _p(buf), C.byref(n)) == E_STATE and b"dspmap_build_objects" in err()
    assert L.dspmap_get_object_labels(m.h, _p(grid)) == E_STATE and b"dspmap_build_objects" in err()
    assert L.dspmap_query_objects(m.h, 2, _p(q), 0, _p(out)) == E_STATE and b"dspmap_build_objects" in err()
    assert not any(getattr(L, fn)(m.h) for fn in MINE)
    return True


def test_object_life_cycle(dsp):
    """stale after everything that changes the map or the grid, untouched by the other layers' builds, the known-space calls and the
    position; and a build of objects takes none of the other six snapshots away"""
    from tests import frontier_ref as FR
    m, lay = _scene(dsp, CUBE)
    res = [m.results()]
    grid, age = R.pack(lay), FR.scene(CUBE)[1]
    pts = _cloud(WALL_DIST[CUBE])
    build = lambda: m.build_objects(t=-1.0, connectivity=26, min_cells=1, max_objects=64)   # noqa: E731
    want = lambda: _want(CUBE, 0, lay[0], res[0], 26, 1, 64)                          # noqa: E731
    assert _gone(m)                                                                  # never built
    build()
    _same(_read(m), want(), "first")
    frame = [4]

    def update():
        assert m.update(pts, (0.0, 0.0, 0.0), frame[0] / 30.0, QUATS["identity"]) == 1
        frame[0] += 1
    regrid = lambda: (m.build_cast_grid(0.5, 0), m.set_cast_grid(grid))              # noqa: E731
    stale = [("update", update, True), ("seed_uniform", lambda: m.seed_uniform(2), True), ("clear_state", m.clear_state, True),
             ("build_cast_grid", lambda: m.build_cast_grid(0.5, 0), False), ("mask_cast_grid", lambda: (m.set_known(age), m.mask_cast_grid(MAX_AGE)), False),
             ("set_cast_grid", lambda: m.set_cast_grid(grid), False)]
    for name, fn, map_changed in stale:
        fn()
        assert _gone(m), name
        if map_changed:                                                              # the grid went with the map
            assert m.L.dspmap_build_objects(m.h, -1.0, 26, 1, 64, 0) == E_STATE and b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h), name
            res[0] = m.results()
        regrid()
        build()
        _same(_read(m), want(), name)
    # the other snapshots, built around a valid build of objects
    m.set_known(age)
    m.build_distance_field(0.5, 8)
    m.build_reach_timeline(SRC, max_steps=16)
    m.build_forecast([0.1, 0.4])
    m.build_frontiers(max_age=MAX_AGE)
    assert all(getattr(m.L, fn)(m.h) for fn in OTHERS + MINE)
    first = _read(m)
    keep = [("build_reach_fields", lambda: m.build_reach_fields(SRC, max_steps=16)), ("build_reach_timeline", lambda: m.build_reach_timeline(SRC, max_steps=16)),
            ("build_distance_field", lambda: m.build_distance_field(0.5, 8)), ("build_forecast", lambda: m.build_forecast([0.1, 0.4])),
            ("build_frontiers", lambda: m.build_frontiers(max_age=MAX_AGE)), ("integrate_known", m.integrate_known),
            ("reset_known", m.reset_known), ("set_known", lambda: m.set_known(age)),
            ("set_current_position", lambda: m.set_current_position(0.3, -0.15, 0.0))]
    for name, fn in keep:
        fn()
        assert all(getattr(m.L, f)(m.h) for f in MINE), name
        again = _read(m)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:2], again[:2])) and first[2] == again[2], name
    # a build of objects takes none of the other six away
    m.set_current_position(0.0, 0.0, 0.0)
    m.set_known(age)
    m.build_reach_timeline(SRC, max_steps=16)
    m.build_frontiers(max_age=MAX_AGE)
    assert all(getattr(m.L, fn)(m.h) for fn in OTHERS)
    build()
    assert all(getattr(m.L, fn)(m.h) for fn in OTHERS + MINE)
    m.close()


def test_object_build_is_read_only(dsp):
    """twins: one builds objects between the frames, the other never does; results, future status, cast grid, counters and the next frame
    are the same"""
    twins = []
    for _ in range(2):
        m = _map(dsp, CUBE, seed=99)
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        twins.append(m)
    a, b = twins
    pts = [_cloud(0.6, seed=s) for s in range(4)]
    found = 0
    for f in range(3):
        cur = (0.03 * f, -0.02 * f, 0.0)
        for m in (a, b):
            assert m.update(pts[f], cur, f / 30.0, QUATS[("identity", "yaw90", "yaw180")[f % 3]]) == 1
            m.build_cast_grid(0.05, 1)
        state = (a.results(), b.getFutureStatus(), a.cast_grid(), a.cursors())   # (getFutureStatus is a consuming readout: the twin's is the "before")
        ca = a.counters()
        for t, conn, min_cells in ((-1.0, 26, 1), (T_BETWEEN, 6, 2), (T_PAST, 26, 4)):
            a.build_objects(t=t, connectivity=conn, min_cells=min_cells, max_objects=256)
            got = _read(a)
            _same(got, R.objects(CR_unpack(state[2][TIMES[t]], CUBE[0]), state[0], conn, min_cells, 256), ("twin", f, t))
            found += got[2][0]
        after = (a.results(), a.getFutureStatus(), a.cast_grid(), a.cursors())
        for x, y in zip(state[:3], after[:3]):
            assert np.array_equal(x, y)
        assert state[3] == after[3]
        cb = a.counters()
        ca.pop("update_ms"), cb.pop("update_ms")
        assert ca == cb
        assert a.cast_grid_ptr() is not None
    assert found > 0
    for m in (a, b):
        assert m.update(pts[3], (0.1, 0.0, 0.0), 0.2, QUATS["identity"]) == 1
    assert np.array_equal(a.results(), b.results()) and (a.results()[:, 0] > 0).any()
    ca, cb = a.counters(), b.counters()
    ca.pop("update_ms"), cb.pop("update_ms")
    assert ca == cb and a.cursors() == b.cursors()
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    a.close(), b.close()
