"""GPU tests of the occupancy forecast at caller-chosen times (dspmap_build_forecast, the accessors, dspmap_query_forecast*): bit parity of
every layer with the numpy restatement (tests/forecast_ref.py) of export_state() taken after the build, over both storage orders; bit
parity with the frame's own rollout where the two contracts coincide; hand-built edges; the snapshot's life cycle and read-only
behaviour; host == device == restatement for the point query."""
import importlib

import numpy as np
import pytest
import torch

from tests import common
from tests import forecast_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
SMALL = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
TINY = dict(nx=16, ny=16, nz=6, res=0.15, ppv=12)
TIMES = [0.0, 0.05, 0.13, 0.5, 1.0, 2.0, 3.5]


def _scene_frames(dsp, kw, n, seed=1234):
    scene = importlib.import_module("dsp-map_amd.scene")
    sc = scene.CorridorScene(kw["nx"] * kw["res"], kw["ny"] * kw["res"], kw["nz"] * kw["res"], seed=seed, device="cuda")
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        out = [sc.frame(f / 30.0) + (f / 30.0,) for f in range(n)]
    finally:
        torch.use_deterministic_algorithms(was)
    torch.cuda.synchronize()
    return out


def _run(m, frames, each=None):
    for f, (pts, pos, quat, t) in enumerate(frames):
        if f:
            m.clearOccupancyMapPrediction()   # (once per frame, :429-438; not after the last one: its future status is read)
        assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        if each:
            each(m)
    return np.array(frames[-1][1], F)


@pytest.fixture(scope="module")
def frames8(dsp):
    return _scene_frames(dsp, SMALL, 8)


def _scene_map(dsp, frames, tiling, **cfg_kw):
    kw = dict(SMALL)
    kw.update(cfg_kw)
    m = dsp.DSPMap(dsp.make_config(seed=1234, **kw))
    m.set_param(dsp.capi.P_TILING, tiling)
    m.seed_uniform(2, 0.01, 99, vmax=0.0 if cfg_kw.get("static_model") else 1.0)
    cur = _run(m, frames)
    assert int(m.get_param(dsp.capi.P_TILING)) == tiling
    return m, cur


def _check_against_export(m, times):
    """forecast() of a build at `times` == the restatement of export_state() taken afterwards, bit for bit; returns (layers, sums, dropped)"""
    m.build_forecast(times)
    assert m.forecast_ptr() is not None and np.array_equal(m.forecast_times(), np.asarray(times, F))
    got = m.forecast()
    voxel, slot, rec = m.export_state()
    want, acc, dropped = R.layers(m.cfg, voxel, rec, times)
    assert got.dtype == F and got.shape == want.shape == (len(times), m.V)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])
    for j in (0, len(times) - 1):
        assert np.array_equal(m.forecast(j), got[j])
    return got, acc, dropped


def test_forecast_bit_parity_after_real_frames(dsp, frames8):
    by_tiling = []
    for tiling in (0, 1):
        m, _ = _scene_map(dsp, frames8, tiling)
        got, acc, dropped = _check_against_export(m, TIMES)
        assert dropped == 0
        # not vacuous: the layers differ, and particles have left the map by the last one
        assert (got[0] != got[-1]).sum() > 1000
        assert acc[-1].sum() < acc[0].sum()
        m.build_forecast(TIMES)
        assert np.array_equal(m.forecast().view(np.uint32), got.view(np.uint32))          # a second build: the same bytes
        res = m.results()
        mass = res[:, 0]
        err = np.abs(got[0] - mass)
        print("t = 0 against results(): max |diff| %.3g, max mass %.3g" % (err.max(), mass.max()))
        assert (err <= 1e-5 * np.maximum(1.0, mass)).all()
        # newborn inclusion: mass the frame's own future status leaves out (consuming readout last).  The 8 scene frames were enough.
        fut = m.getFutureStatus()
        only_new = (mass > 0) & (fut[:, 0] == 0)
        print("voxels with mass but no future status at horizon 0: %d" % only_new.sum())
        assert only_new.sum() >= 1 and (got[0][only_new] > 0).all()
        by_tiling.append(got)
        m.close()
    assert np.array_equal(by_tiling[0].view(np.uint32), by_tiling[1].view(np.uint32))       # both storage orders: the same bytes


def test_forecast_static_model_scene(dsp, frames8):
    """dsp_static.h's motion model: every particle static, every tile's velocity rows skipped; all layers equal"""
    m, _ = _scene_map(dsp, frames8, 0, static_model=1)
    got, acc, dropped = _check_against_export(m, TIMES)
    assert dropped == 0 and (got == got[0]).all() and (got[0] > 0).sum() > 1000
    assert not m.tile_moving().any()
    m.set_param(dsp.capi.P_STATIC_TILE_SKIP, 0)          # every velocity row fetched after all: the same bytes
    m.build_forecast(TIMES)
    assert np.array_equal(m.forecast().view(np.uint32), got.view(np.uint32))
    m.close()


def _rollout_input(cfg, seed=5):
    """<= 4 particles per voxel in about 60 % of the voxels, flag 1, |v| in 0.2 .. 1.5 on at least one axis, weights in [0.002, 0.5]"""
    rng = np.random.default_rng(seed)
    res, (nx, ny, nz), (hx, hy, hz) = R.dims(cfg)
    vox, slots, recs = [], [], []
    for v in range(nx * ny * nz):
        if rng.random() >= 0.6:
            continue
        k = int(rng.integers(1, 5))
        iz, iy, ix = v // (nx * ny), (v // nx) % ny, v % nx
        for s in range(k):
            vel = rng.uniform(0.2, 1.5, 2) * rng.choice([-1.0, 1.0], 2)
            if rng.random() < 0.3:
                vel[int(rng.integers(0, 2))] = 0.0
            p = [(ix + rng.uniform(0.1, 0.9)) * float(res) - float(hx), (iy + rng.uniform(0.1, 0.9)) * float(res) - float(hy),
                 (iz + rng.uniform(0.1, 0.9)) * float(res) - float(hz)]
            vox.append(v)
            slots.append(s)
            recs.append([1.0, vel[0], vel[1], 0.0] + p + [rng.uniform(0.002, 0.5)])
    return np.array(vox, np.int32), np.array(slots, np.int32), np.array(recs, F)


@pytest.mark.parametrize("tiling", [0, 1])
def test_forecast_equals_frame_rollout(dsp, tiling):
    """no cull (weights >= 1e-3), no resampling (fewer than five particles per voxel), no newborn, no static particle: the frame's future
    status and the forecast at the configured horizons are the same sums of the same quanta"""
    cfg = dsp.make_config(seed=7, **TINY)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, tiling)
    voxel, slot, rec = _rollout_input(cfg)
    horizons = [cfg.prediction_future_time[k] for k in range(cfg.prediction_times)]
    assert len(horizons) == 6 and R.layers(cfg, voxel, rec, horizons)[2] == 0
    m.clear_state()
    m.import_state(voxel, rec, slot)
    m.clearOccupancyMapPrediction()
    m.occupancy_resample()
    m.build_forecast(horizons)
    got = m.forecast()
    v2, s2, r2 = m.export_state()
    assert np.array_equal(v2, voxel) and np.array_equal(s2, slot) and np.array_equal(r2[:, 1:], rec[:, 1:])   # the stage changed nothing
    fut = m.getFutureStatus()              # the consuming readout last
    assert int(m.get_param(dsp.capi.P_TILING)) == tiling
    for j in range(6):
        assert np.array_equal(got[j].view(np.uint32), np.ascontiguousarray(fut[:, j]).view(np.uint32)), j
    assert (got[0] != got[-1]).sum() > 200 and got[0].sum() > got[-1].sum() > 0
    m.close()


def _edge_input(cfg, slots):
    """hand-built particles: (voxel, slot, rec8, voxel of the five awkward weights alone, the edge float's expected drops per build)"""
    res, (nx, ny, nz), (hx, hy, hz) = R.dims(cfg)
    rng = np.random.default_rng(3)
    r = float(res)
    g = lambda x, y, z: (z * ny + y) * nx + x   # noqa: E731
    centre = lambda x, y, z: [(x + 0.5) * r - float(hx), (y + 0.5) * r - float(hy), (z + 0.5) * r - float(hz)]   # noqa: E731
    items = []   # (voxel, [flag, vx, vy, vz, px, py, pz, w])

    def put(v, vx, vy, p, w, flag=1.0):
        items.append((v, [flag, vx, vy, 0.0] + list(p) + [w]))

    # one particle through each x / y face between t = 0.05 and t = 0.13
    for (x, y, vx, vy, px, py) in ((nx - 1, 5, 1.0, 0.0, float(hx) - 0.06, None), (0, 6, -1.0, 0.0, -float(hx) + 0.06, None),
                                   (7, ny - 1, 0.0, 1.0, None, float(hy) - 0.06), (8, 0, 0.0, -1.0, None, -float(hy) + 0.06)):
        p = centre(x, y, 2)
        p[0] = p[0] if px is None else px
        p[1] = p[1] if py is None else py
        put(g(x, y, 2), vx, vy, p, 0.25)
    # exactly on a voxel face, moving along it and static
    face = float(F(F(5) * res) - hx)
    put(g(5, 3, 1), 0.0, 0.3, [face, centre(5, 3, 1)[1], centre(5, 3, 1)[2]], 0.125)
    put(g(5, 3, 1), 0.0, 0.0, [face, centre(5, 3, 1)[1], centre(5, 3, 1)[2]], 0.0625)
    put(g(4, 3, 1), 0.3, 0.0, [face, centre(4, 3, 1)[1], centre(4, 3, 1)[2]], 0.03125, flag=15.0)     # a newborn counts
    # static next to moving in one voxel / one tile
    put(g(2, 2, 3), 0.0, 0.0, centre(2, 2, 3), 0.5)
    put(g(2, 2, 3), 0.7, -0.4, centre(2, 2, 3), 0.25)
    put(g(3, 2, 3), -0.9, 0.0, centre(3, 2, 3), 0.125)
    # the awkward weights, static in a voxel of their own and moving from another: quanta 0, 2, 0, 0, 0
    alone = g(nx - 3, ny - 3, nz - 1)
    for w in (2.0 ** -25, 3 * 2.0 ** -25, 0.0, -0.25, np.nan):
        put(alone, 0.0, 0.0, centre(nx - 3, ny - 3, nz - 1), w)
        put(g(9, 9, 4), 0.5, 0.5, centre(9, 9, 4), w)
    # non-finite velocities and positions (an import can hold them): a NaN fx or fy is outside the map; the static one stays where it is stored
    c = centre(10, 4, 4)
    put(g(10, 4, 4), np.nan, 0.2, c, 0.25)
    put(g(10, 4, 4), np.inf, 0.0, c, 0.25)
    put(g(10, 4, 4), 0.3, np.nan, c, 0.25)
    put(g(10, 4, 4), 0.3, 0.0, [np.inf, c[1], c[2]], 0.25)
    put(g(10, 4, 4), 0.0, 0.0, [np.nan, c[1], c[2]], 0.125)
    # the one float just below half_x, stored in the last voxel of a row, moving outwards
    edge = np.nextafter(hx, F(0))
    put(g(nx - 1, 10, 0), 1.0, 0.0, [float(edge), centre(0, 10, 0)[1], centre(0, 10, 0)[2]], 0.25)
    edge_drops = 1 if int(F(F(edge + hx) / res)) == nx else 0
    # one voxel filled to its last slot (the second occupancy word where slots > 64)
    for s in range(slots):
        mv = s % 3 != 0
        put(g(6, 11, 5), 0.4 * mv * (1 if s % 2 else -1), 0.8 * mv, [c + rng.uniform(-0.4, 0.4) * r for c in centre(6, 11, 5)], rng.uniform(0.002, 0.1))
    # a sprinkle over the rest of the map
    for v in rng.choice(nx * ny * nz, nx * ny * nz // 3, replace=False):
        if v in (alone, g(6, 11, 5), g(nx - 1, 10, 0)):
            continue
        iz, iy, ix = v // (nx * ny), (v // nx) % ny, v % nx
        for _ in range(int(rng.integers(1, 4))):
            mv = rng.random() < 0.6
            put(int(v), rng.uniform(-1.5, 1.5) * mv, rng.uniform(-1.5, 1.5) * mv, [c + rng.uniform(-0.45, 0.45) * r for c in centre(ix, iy, iz)],
                rng.uniform(0.002, 0.5))
    used = {}
    vox, slot, rec = [], [], []
    for v, rr in items:
        s = used.get(v, 0)
        if s >= slots:
            continue
        used[v] = s + 1
        vox.append(v)
        slot.append(s)
        rec.append(rr)
    assert used[g(6, 11, 5)] == slots
    return np.array(vox, np.int32), np.array(slot, np.int32), np.array(rec, F), alone, edge_drops


@pytest.mark.parametrize("name,kw,tiling", [("runs", TINY, 0), ("cubes", TINY, 1), ("cubes_padded", dict(TINY, nx=18, ny=14), 1),
                                            ("runs_two_words", dict(TINY, ppv=33), 0), ("cubes_two_words", dict(TINY, ppv=33), 1)])
def test_forecast_hand_built_edges(dsp, name, kw, tiling):
    cfg = dsp.make_config(seed=3, **kw)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, tiling)
    assert m.slots == 2 * kw["ppv"]
    voxel, slot, rec, alone, edge_drops = _edge_input(cfg, m.slots)
    assert edge_drops == (1 if kw["nx"] == 16 else 0)
    m.clear_state()
    m.import_state(voxel, rec, slot)
    assert int(m.get_param(dsp.capi.P_TILING)) == tiling
    builds = {}
    for skip in (1, 0):
        m.set_param(dsp.capi.P_STATIC_TILE_SKIP, skip)
        for times in (TIMES, [0.3], list(np.arange(64, dtype=F) * F(0.04))):
            got, acc, dropped = _check_against_export(m, times)
            assert dropped == edge_drops * sum(1 for t in times if t == 0.0), (times[:3], dropped)
            key = len(times)
            if key in builds:
                assert np.array_equal(builds[key].view(np.uint32), got.view(np.uint32)), (skip, key)       # tile skip 0 and 1: the same bytes
            builds[key] = got
    got = builds[len(TIMES)]
    nx, ny = cfg.nx, cfg.ny
    assert got[0, alone] == F(2.0 ** -23) and (got[:, alone] >= F(2.0 ** -23)).all()   # quanta 0 + 2 + 0 + 0 + 0 (later layers: plus arrivals)
    last = (10 * nx) + nx - 1                                            # voxel (nx - 1, 10, 0): the edge float's own
    assert (voxel == last).sum() == 1 and got[0, last] == (0 if edge_drops else F(0.25))    # the dropped particle adds nothing at t = 0
    # through the four faces, on the device and alone in the map: each in its border voxel at t = 0 and 0.05, gone from t = 0.13 on
    m.clear_state()
    m.import_state(voxel[:4], rec[:4], slot[:4])
    m.build_forecast(TIMES)
    four = m.forecast()
    border = [(2 * ny + 5) * nx + nx - 1, (2 * ny + 6) * nx, (2 * ny + ny - 1) * nx + 7, (2 * ny) * nx + 8]
    assert voxel[:4].tolist() == border
    for j in (0, 1):
        assert (four[j, border] == F(0.25)).all() and four[j].sum() == 1.0
    assert not four[2:].any()
    # the non-finite ones alone: only the static one is ever counted, in the voxel it is stored in
    odd = np.flatnonzero(voxel == (4 * ny + 4) * nx + 10)[:5]
    assert len(odd) == 5 and not np.isfinite(rec[odd][:, [1, 2, 4]]).all(1).any()
    m.clear_state()
    m.import_state(voxel[odd], rec[odd], slot[odd])
    m.build_forecast(TIMES)
    lone = m.forecast()
    assert (lone[:, (4 * ny + 4) * nx + 10] == F(0.125)).all() and (lone.sum(1) == F(0.125)).all()
    m.close()


def test_forecast_static_tile_after_zero_motion_predict(dsp):
    """a tile whose particles are all static has tile_moving 0 after a prediction: its velocity rows are not fetched, the layers are the same"""
    cfg = dsp.make_config(seed=3, **TINY)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 0)
    res, (nx, ny, nz), (hx, hy, hz) = R.dims(cfg)
    rng = np.random.default_rng(9)
    vox, rec = [], []
    for v in list(range(0, 64)) + list(range(640, 700)):        # tile 0: static only; tile 10: mixed
        iz, iy, ix = v // (nx * ny), (v // nx) % ny, v % nx
        for k in range(3):
            mv = v >= 640 and k > 0
            vox.append(v)
            rec.append([1.0, 0.8 * mv, -0.6 * mv, 0.0, (ix + 0.5) * float(res) - float(hx), (iy + 0.5) * float(res) - float(hy),
                        (iz + 0.5) * float(res) - float(hz), rng.uniform(0.01, 0.3)])
    m.clear_state()
    m.set_tables(np.zeros(1000, F), np.zeros(1000, F))          # no prediction noise: the particles stay where they were put
    m.import_state(np.array(vox, np.int32), np.array(rec, F))
    m.predict(0.0, 0.0, 0.0, 0.0)
    tm = m.tile_moving()
    assert tm[0] == 0 and tm[10] == 1
    got, acc, dropped = _check_against_export(m, TIMES)
    assert dropped == 0 and (got[:, :64] > 0).all() and (got[:, :64] == got[0, :64]).all() and (got[0] != got[3]).any()
    # the same tile WITH its velocity rows (DSPMAP_P_STATIC_TILE_SKIP 0 reads the zeros tile_moving 0 promises): the same bytes
    m.set_param(dsp.capi.P_STATIC_TILE_SKIP, 0)
    m.build_forecast(TIMES)
    assert np.array_equal(m.forecast().view(np.uint32), got.view(np.uint32)) and m.tile_moving()[0] == 0
    m.close()


def _counters(m):
    c = m.counters()
    c.pop("update_ms", None)
    return c


def _assert_stale(dsp, m, q):
    L = m.L
    assert m.forecast_ptr() is None
    out = np.zeros(m.V, F)
    vals = np.zeros(len(q), F)
    t = np.zeros(64, F)
    for rc in (L.dspmap_get_forecast(m.h, 0, out.ctypes.data), L.dspmap_query_forecast(m.h, len(q), q.ctypes.data, 0, 1.0, vals.ctypes.data)):
        assert rc == E_STATE and b"dspmap_build_forecast" in L.dspmap_last_error(m.h)
    assert L.dspmap_forecast_times(m.h, t.ctypes.data, 64) == E_STATE
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_forecast"):
        m.query_forecast(qd)


def test_forecast_life_cycle_and_read_only(dsp, tmp_path):
    frames = _scene_frames(dsp, SMALL, 7, seed=77)
    maps = []
    for _ in range(2):
        m = dsp.DSPMap(dsp.make_config(seed=99, **SMALL))
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        maps.append(m)
    a, b = maps
    q = np.array([[0.1, 0.2, 0.3, 0.07], [0.0, 0.0, 0.0, 9.0]], F)
    _run(a, frames[:6], each=lambda m: m.build_forecast(TIMES))
    _run(b, frames[:6])
    assert a.forecast_ptr() is not None and b.forecast_ptr() is None
    lay = a.forecast()
    vals = a.query_forecast(q, lerp=True)
    # valid through the readouts, a clear of the prediction and the occupancy readout; and nothing of the map differs
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
    assert a.forecast_ptr() is not None
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and fa.any()
    assert a.forecast_ptr() is not None
    ea, eb = a.export_state(), b.export_state()
    for x, y in zip(ea, eb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert _counters(a) == _counters(b)
    a.clearOccupancyMapPrediction()
    a.getOccupancyMap(0.5)
    assert a.forecast_ptr() is not None
    assert np.array_equal(a.forecast().view(np.uint32), lay.view(np.uint32)) and np.array_equal(a.query_forecast(q, lerp=True), vals)
    # a smaller build after a larger one, and a larger one again
    a.build_forecast([0.25])
    assert a.forecast_times().tolist() == [0.25] and a.forecast().shape == (1, a.V)
    a.build_forecast(list(np.arange(10, dtype=F) * F(0.1)))
    assert len(a.forecast_times()) == 10 and np.array_equal(a.forecast(0).view(np.uint32), lay[0].view(np.uint32))
    with pytest.raises(dsp.capi.DSPMapError):
        a.forecast(10)
    # stale after everything that computes a frame or replaces state
    ckpt = tmp_path / "state.ckpt"
    a.save_checkpoint(ckpt)
    pts, pos, quat, t = frames[6]
    voxel, slot, rec = ea
    steps = (("update_device", lambda: a.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat)),
             ("import_state", lambda: a.import_state(voxel[:1], rec[:1])),
             ("clear_state", a.clear_state),
             ("seed_uniform", lambda: a.seed_uniform(1, 0.01, 5, vmax=0.5)),
             ("stage_predict", lambda: a.predict(0.0, 0.0, 0.0, 0.03)),
             ("load_checkpoint", lambda: a.load_checkpoint(ckpt)))
    for name, step in steps:
        a.build_forecast(TIMES)
        assert a.forecast_ptr() is not None, name
        step()
        _assert_stale(dsp, a, q)
    a.build_forecast(TIMES)
    assert a.forecast_ptr() is not None
    for m in maps:
        m.close()
    # a sharded handle holds part of the map
    s = dsp.DSPMap(dsp.make_config(seed=1, z_lo=0, z_hi=3, **TINY))
    s.seed_uniform(1, 0.01, 5)
    t = np.array(TIMES, F)
    assert s.L.dspmap_build_forecast(s.h, len(t), t.ctypes.data, 0) == E_STATE and b"slab" in s.L.dspmap_last_error(s.h)
    assert s.forecast_ptr() is None
    s.close()


def _samples(cfg, times, n, seed):
    """n samples over 1.1 x the map box: uniform points, voxel centres, voxel faces, NaN; every class of t"""
    rng = np.random.default_rng(seed)
    hx, hy, hz = common.half_extent(cfg)
    half = np.array([hx, hy, hz], F)
    res = F(cfg.voxel_resolution)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    p = (rng.uniform(-1.1, 1.1, (n, 3)) * half).astype(F)
    idx = rng.integers(0, nn, (n, 3))
    corr = (-half + res * F(0.5)).astype(F)
    centres = (idx.astype(F) * res + corr).astype(F)
    a, b = n // 5, 2 * (n // 5)
    p[:a] = centres[:a]                                                     # lattice centres
    faces = centres[a:b].copy()
    ax = rng.integers(0, 3, b - a)
    faces[np.arange(b - a), ax] = (faces[np.arange(b - a), ax] + res * F(0.5)).astype(F)   # a voxel face
    p[a:b] = faces
    times = np.asarray(times, F)
    mids = ((times[:-1] + times[1:]) * F(0.5)).astype(F)
    below = np.array([times[0] * F(0.5), np.nextafter(times[0], F(-1))], F)
    above = np.array([times[-1] + F(1), np.nextafter(times[-1], F(np.inf)), np.inf], F)
    tclass = np.concatenate([[-1.0, -0.0, 0.0], below, above, times, mids]).astype(F)
    t = tclass[rng.integers(0, len(tclass), n)]
    between = rng.random(n) < 0.4
    t[between] = rng.uniform(float(times[0]), float(times[-1]), between.sum()).astype(F)     # anywhere between the knots
    q = np.concatenate([p, t[:, None]], 1).astype(F)
    nan = rng.random((n, 4)) < 0.003
    q[nan] = np.nan
    return q


def test_forecast_query_parity(dsp, frames8):
    m, cur = _scene_map(dsp, frames8, 0)
    assert np.abs(cur).max() > 0
    times = TIMES[1:]
    m.build_forecast(TIMES)
    m.build_forecast(times)                       # (a smaller build after a larger one)
    lay = m.forecast()
    cfg = m.cfg
    q = _samples(cfg, times, 20000, 7)
    plain = {}
    for lerp in (False, True):
        for world in (False, True):
            qq = q.copy()
            if world:
                qq[:, :3] = (qq[:, :3] + cur[None, :]).astype(F)
            host = m.query_forecast(qq, world=world, lerp=lerp, outside=0.75)
            qd = torch.from_numpy(np.concatenate([qq, qq], 1)).cuda()[:, :4]   # a non-contiguous view: the binding's temporary
            torch.cuda.synchronize()   # (the copy ran on torch's stream, the query runs on the handle's)
            dev = m.query_forecast(qd, world=world, lerp=lerp, outside=0.75)
            m.sync()
            want = R.query(cfg, lay, times, qq, world=world, lerp=lerp, cur_pos=cur, outside=0.75)
            assert np.array_equal(host.view(np.uint32), dev.cpu().numpy().view(np.uint32)), (lerp, world)
            bad = np.flatnonzero(host.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (lerp, world, bad.size, bad[:5], qq[bad[:5]], host[bad[:5]], want[bad[:5]])
            if lerp:
                assert (host != plain[world]).sum() >= 1000            # the flag is exercised
            else:
                plain[world] = host
    out = plain[False]
    assert (out == F(0.75)).sum() > 1000 and ((out != F(0.75)) & (out > 0)).sum() > 5000
    m.close()
