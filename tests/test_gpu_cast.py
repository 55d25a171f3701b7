"""GPU tests of the segment casts (dspmap_build_cast_grid, dspmap_get_cast_grid, dspmap_cast_segments*): bit parity -- zero mismatching
words, zero mismatching output fields -- with the numpy restatement (tests/cast_ref.py) fed with what the map hands out AFTER the
build, over storage orders, thresholds, inflation radii and awkward shapes; the device entry point enqueued right behind the frame;
read-only behaviour, the pending clear, snapshot validity and staleness."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cast_ref as R
from tests import common
from tests import distance_ref as D
from tests import query_ref as Q
from tests.test_gpu_query import B, _run, _scene_frames

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
SMALL = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)


def _median_threshold(m):
    mass = m.results()[:, 0]
    assert (mass > 0).any()
    return float(np.median(mass[mass > 0]))


def _build_all(m, combos):
    """the grids of every (threshold, inflate) of combos, each read back right after its build"""
    out = []
    for thr, r in combos:
        m.build_cast_grid(thr, r)
        assert m.cast_grid_ptr() is not None
        out.append(m.cast_grid())
    return out


def _check_grids(m, cfg, combos, got):
    """word parity of got[i] with the restatement of combos[i] over results() / getFutureStatus() read now; returns (res, fut, raw layers by threshold)"""
    res, fut = m.results(), m.getFutureStatus()
    raw = {}
    W = (cfg.nx + 63) // 64
    for (thr, r), g in zip(combos, got):
        if thr not in raw:
            raw[thr] = D.occupancy_layers(cfg, res, fut, thr)
        want = R.pack(R.inflate(raw[thr], r))
        assert g.dtype == np.uint64 and g.shape == want.shape == (cfg.prediction_times + 1, cfg.nz, cfg.ny, W)
        bad = np.flatnonzero(g != want)
        assert bad.size == 0, (thr, r, bad.size, bad[:5], g.ravel()[bad[:5]], want.ravel()[bad[:5]])
        if cfg.nx & 63:
            assert not (g[..., -1] >> np.uint64(cfg.nx & 63)).any()      # pad bits at x >= nx
    return res, fut, raw


@pytest.mark.parametrize("variant", ["runs", "cubes", "static"])
def test_cast_grid_bit_parity(dsp, variant):
    kw = dict(B)
    if variant == "static":
        kw.update(static_model=1)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    if variant in ("runs", "cubes"):
        m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=0.0 if variant == "static" else 1.0)
    _run(m, _scene_frames(dsp, kw, 12))
    if variant in ("runs", "cubes"):
        assert int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    med = _median_threshold(m)
    combos = [(thr, r) for thr in (0.2, med, 0.0, 1e9) for r in (0, 1, 3, 8)]
    got = _build_all(m, combos)
    res, fut, raw = _check_grids(m, cfg, combos, got)
    # the input is not degenerate: both classes at the median threshold, an empty and a dense case, inflation that changes something
    occ0 = res[:, 0] > F(med)
    assert occ0.sum() >= 1000 and (~occ0).sum() >= 1000
    assert not got[combos.index((1e9, 8))].any() and raw[0.0][0].sum() > 10000
    a, b = got[combos.index((med, 0))], got[combos.index((med, 3))]
    assert (a & ~b).sum() == 0 and (b != a).sum() > 1000
    if variant != "static":
        assert (a[1] != a[-1]).any()      # the horizons differ: moving mass
    m.close()


@pytest.mark.parametrize("shape", ["50x37x23", "132x40x12", "8x8x1", "t0"])
def test_cast_grid_awkward_shapes(dsp, shape):
    kw = {"50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),        # no multiple of 64 anywhere
          "132x40x12": dict(nx=132, ny=40, nz=12, res=0.15, ppv=9),        # three words per row: carries across two word boundaries
          "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=())}[shape]
    cfg = dsp.make_config(seed=77, **kw)
    m = dsp.DSPMap(cfg)
    m.seed_uniform(2, 0.01, 5, vmax=1.0)
    if shape == "8x8x1":     # (a map smaller than the scene's sensor range: a hand-made cloud inside it)
        pts = torch.tensor([[0.3, 0.1, 0.0], [0.3, -0.2, 0.02], [0.45, 0.3, -0.03]], dtype=torch.float32, device="cuda")
        for f in range(4):
            assert m.update_device(pts.data_ptr(), 3, (0.0, 0.0, 0.0), f / 30.0, (1.0, 0.0, 0.0, 0.0)) == 1
    else:
        _run(m, _scene_frames(dsp, kw, 8, seed=31))
    assert m.T == (0 if shape == "t0" else 6)
    med = _median_threshold(m)
    combos = [(med, r) for r in (0, 1, 3, 8)] + [(0.0, 2), (1e9, 8)]
    got = _build_all(m, combos)
    # a few casts on each shape too (T = 0: every time reads layer 0) -- before the readouts below, which consume the future status
    seg = _segments(cfg, 3000, 11)
    m.build_cast_grid(med, 1)
    hits = m.cast_segments(seg)
    res, fut, raw = _check_grids(m, cfg, combos, got)
    occ0 = res[:, 0] > F(med)
    assert (~occ0).any() and (occ0.any() or shape == "8x8x1")      # (64 voxels may all hold the same mass; the dense and the empty case remain)
    assert got[0].shape[0] == m.T + 1
    if shape == "132x40x12":      # the inflation did carry across both word boundaries somewhere
        a, b = got[0], got[2]
        assert ((b & ~a)[..., 0] >> np.uint64(61)).any() and ((b & ~a)[..., 1] & np.uint64(7)).any()
        assert ((b & ~a)[..., 1] >> np.uint64(61)).any() and ((b & ~a)[..., 2] & np.uint64(7)).any()
    want = R.cast(cfg, R.inflate(raw[med], 1), seg)
    _assert_same_hits(hits, want, seg, shape)
    if shape == "t0":
        assert (hits["layer"][hits["status"] == R.HIT] == 0).all() and (hits["status"] == R.HIT).any()
    m.close()


def _segments(cfg, n, seed):
    """n segments {ax, ay, az, ta, bx, by, bz, tb}: random pairs inside the map, rays from the centre to beyond the map, axis-aligned and
    exactly diagonal ones through voxel corners (coordinates that are multiples of res), zero-length ones, starts outside, NaN and inf
    entries; times: ta < 0, ta = tb inside each horizon, ta < tb spanning all horizons, tb < ta"""
    rng = np.random.default_rng(seed)
    half = np.array(common.half_extent(cfg), F)
    res = F(cfg.voxel_resolution)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    a = (rng.uniform(-0.98, 0.98, (n, 3)) * half).astype(F)
    b = (rng.uniform(-0.98, 0.98, (n, 3)) * half).astype(F)
    kind = rng.integers(0, 8, n)
    ray = kind == 1                                                    # from the map centre to beyond the map
    a[ray] = (rng.uniform(-0.5, 0.5, (ray.sum(), 3)) * res).astype(F)
    direction = rng.standard_normal((ray.sum(), 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    b[ray] = (direction * rng.uniform(1.8, 3.0, (ray.sum(), 1)) * half.max()).astype(F)
    lat = (kind == 2) | (kind == 3)                                    # through voxel corners: integer multiples of res
    ka = np.stack([rng.integers(-(k // 2) + 1, max(k // 2, -(k // 2) + 2), lat.sum()) for k in nn], 1)
    steps = rng.integers(-12, 13, (lat.sum(), 1))
    dirs = np.where((kind[lat] == 2)[:, None], np.eye(3, dtype=np.int64)[rng.integers(0, 3, lat.sum())],
                    rng.choice([-1, 1], (lat.sum(), 3)))               # one axis, or an exact diagonal
    a[lat] = (ka.astype(F) * res).astype(F)
    b[lat] = ((ka + steps * dirs).astype(F) * res).astype(F)
    zero = kind == 4
    b[zero] = a[zero]
    outside = kind == 5                                                # starts outside the map (some exactly on its faces)
    ax = rng.integers(0, 3, outside.sum())
    a[outside, ax] = (rng.choice([-1.0, 1.0], outside.sum()) * rng.choice([1.0, 1.0, 1.05, 1.7], outside.sum()) * half[ax]).astype(F)
    seg = np.empty((n, 8), F)
    seg[:, 0:3], seg[:, 4:7] = a, b
    T = cfg.prediction_times
    pred = np.array([cfg.prediction_future_time[k] for k in range(T)], F)
    tk = rng.integers(0, 4, n)
    inside_h = np.concatenate([[0.0], (pred[:-1] + pred[1:]) * F(0.5), pred]).astype(F) if T else np.array([0.0, 1.0], F)
    t_end = F(pred[-1] + F(0.2)) if T else F(1.0)
    same = inside_h[rng.integers(0, len(inside_h), n)]
    seg[:, 3] = np.where(tk == 0, F(-1.0), np.where(tk == 1, same, np.where(tk == 2, F(0.0), t_end)))
    seg[:, 7] = np.where(tk == 0, rng.uniform(-1, 3, n).astype(F), np.where(tk == 1, same, np.where(tk == 2, t_end, F(0.0))))
    bad = rng.random((n, 8)) < 0.002
    seg[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), bad.sum())
    return seg


def _assert_same_hits(got, want, seg, tag):
    for k in ("s", "voxel", "layer", "status"):
        g, w = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (tag, k, bad.size, bad[:5], seg[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_cast_bit_parity(dsp, variant):
    kw = dict(B)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    assert np.abs(cur).max() > 0 and int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    thr = _median_threshold(m)
    seg = _segments(cfg, 24000, 7)
    runs = []
    for r in (0, 2):
        m.build_cast_grid(thr, r)
        for world in (False, True):
            ss = seg.copy()
            if world:
                ss[:, 0:3] = (ss[:, 0:3] + cur[None, :]).astype(F)
                ss[:, 4:7] = (ss[:, 4:7] + cur[None, :]).astype(F)
            runs.append((r, world, ss, m.cast_segments(ss, world=world)))
    res, fut = m.results(), m.getFutureStatus()
    raw = D.occupancy_layers(cfg, res, fut, thr)
    T, pred = cfg.prediction_times, np.array([cfg.prediction_future_time[k] for k in range(cfg.prediction_times)], F)
    for r, world, ss, got in runs:
        want = R.cast(cfg, R.inflate(raw, r), ss, world=world, cur_pos=cur)
        assert len(got) >= 20000
        _assert_same_hits(got, want, ss, (variant, r, world))
        st = got["status"]
        assert set(st.tolist()) == {R.FREE, R.HIT, R.LEFT_MAP, R.START_OUTSIDE, R.INVALID}
        hit = st == R.HIT
        assert (hit & (got["s"] == 0)).any() and (hit & (got["s"] > 0)).any()
        with np.errstate(invalid="ignore"):
            timed = hit & ~(ss[:, 3] < 0)
            la, lb = Q.horizons(pred, ss[:, 3]) + 1, Q.horizons(pred, ss[:, 7]) + 1
        between = timed & (got["layer"] != la) & (got["layer"] != lb)
        assert between.any() and (got["layer"][hit & (ss[:, 3] < 0)] == 0).all()
    assert not np.array_equal(runs[0][3], runs[2][3])      # the inflation changes answers
    m.close()


def _twins(dsp, kw, n=2):
    maps = []
    for _ in range(n):
        m = dsp.DSPMap(dsp.make_config(seed=99, **kw))
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        maps.append(m)
    return maps


def test_cast_device_entry_point_stream_ordered_behind_frame(dsp):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    (m,) = _twins(dsp, kw, 1)
    seg = _segments(m.cfg, 20000, 13)
    sd = torch.from_numpy(np.concatenate([seg, seg], 1)).cuda()[:, :8]      # a non-contiguous view: the binding's temporary
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    keys = ("s", "voxel", "layer", "status")
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(0.05, 1)                                       # no synchronisation between the frame, the build and the cast
            outs.append(m.cast_segments(sd, world=True))
        st.synchronize()
        after = m.cast_segments(sd, world=True)
        st.synchronize()
        host = m.cast_segments(seg, world=True)
        res, fut = m.results(), m.getFutureStatus()
    for k in keys:
        assert torch.equal(outs[-1][k], after[k]), k
        assert after[k].cpu().numpy().tobytes() == np.ascontiguousarray(host[k]).tobytes(), k
    assert not all(torch.equal(outs[0][k], outs[-1][k]) for k in keys)
    want = R.cast(m.cfg, R.layers(m.cfg, res, fut, 0.05, 1), seg, world=True, cur_pos=np.array(frames[-1][1], F))
    _assert_same_hits(host, want, seg, "device")
    assert (host["status"] == R.HIT).sum() > 100
    m.close()


def test_cast_is_read_only(dsp):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 10, seed=77)
    a, b = _twins(dsp, kw)
    seg = _segments(a.cfg, 4000, 3)
    for pts, pos, quat, t in frames[:4]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    a.build_cast_grid(0.1, 2)
    a.cast_segments(seg)
    grid = a.cast_grid()
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra, rb)
    fa, fb = a.getFutureStatus(), b.getFutureStatus()      # the future status after a build is the one of the twin that never built
    assert np.array_equal(fa, fb) and (fa != 0).any()
    assert np.array_equal(grid, R.pack(R.layers(a.cfg, ra, fa, 0.1, 2)))
    # more frames, one twin building and casting behind every frame (no readout in between: nothing arms a clear on either)
    for pts, pos, quat, t in frames[4:]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        a.build_cast_grid(0.1, 1)
        a.cast_segments(seg, world=True)
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.results(), b.results())
    assert np.array_equal(a.getFutureStatus(), b.getFutureStatus())
    assert b.cast_grid_ptr() is None      # a handle that never built a grid has none
    a.close(); b.close()


def test_cast_snapshot_validity_and_staleness(dsp):
    kw = dict(SMALL)
    (m,) = _twins(dsp, kw, 1)
    frames = _scene_frames(dsp, kw, 7, seed=31)
    _run(m, frames[:6])
    thr = _median_threshold(m)
    seg = _segments(m.cfg, 2000, 3)
    m.build_cast_grid(thr, 1)
    snap, ptr, h0 = m.cast_grid(), m.cast_grid_ptr(), m.cast_segments(seg)
    assert snap[1:].any()
    # the snapshot survives readouts and the clear ...
    m.getOccupancyMapWithFutureStatus(0.1)
    m.clearOccupancyMapPrediction()
    m.results(); m.query_occupancy(seg[:, :4])
    assert m.cast_grid_ptr() == ptr and np.array_equal(m.cast_grid(), snap)
    assert m.cast_segments(seg).tobytes() == h0.tobytes()
    # ... and a rebuild sees horizons that read 0 everywhere: empty layers 1 .. T; the current mass is unchanged
    m.build_cast_grid(thr, 1)
    after = m.cast_grid()
    assert np.array_equal(after[0], snap[0]) and not after[1:].any()
    m.build_cast_grid(-1.0, 0)      # 0 > -1: every voxel of a cleared layer is occupied
    full = m.cast_grid()
    assert (full[1:, :, :, 0] == np.uint64((1 << 40) - 1)).all()
    # a new frame makes it stale; so does every other call that replaces state
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    assert m.cast_grid_ptr() is None
    out = np.zeros(snap[0].size, np.uint64)
    hit = np.zeros(len(seg), R.HIT_DTYPE)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert m.L.dspmap_get_cast_grid(m.h, 0, p(out)) == E_STATE
    assert b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    assert m.L.dspmap_cast_segments(m.h, len(seg), p(seg), 0, p(hit)) == E_STATE
    sd = torch.from_numpy(seg).cuda()
    with pytest.raises(dsp.capi.DSPMapError):
        m.cast_segments(sd)
    voxel, slot, rec = m.export_state()
    for stale in (m.clear_state, lambda: m.import_state(voxel, rec, slot), lambda: m.seed_uniform(1, 0.01, 3)):
        m.build_cast_grid(0.1, 0)
        assert m.cast_grid_ptr() is not None
        stale()
        assert m.cast_grid_ptr() is None
        assert m.L.dspmap_cast_segments(m.h, len(seg), p(seg), 0, p(hit)) == E_STATE
    m.build_cast_grid(0.1, 2)      # and a rebuild is valid again, in the same buffer
    assert m.cast_grid_ptr() == ptr and m.cast_grid().shape == snap.shape
    m.close()
