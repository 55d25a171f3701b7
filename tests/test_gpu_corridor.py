"""GPU tests of the free boxes grown in the cast grid (dspmap_grow_boxes*): bit parity -- zero mismatches in all eight integers of every
box -- with the numpy restatement (tests/corridor_ref.py) fed with the grid the map hands out AFTER the build (m.cast_grid()), over
storage orders, inflation radii, limits, both flags and awkward shapes; the restatement's three algorithm-blind checkers run on the
device's output; the device entry point enqueued right behind the frame and the build; read-only behaviour and the grid's life cycle."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import corridor_ref as R
from tests.test_gpu_cast import SMALL, _median_threshold, _twins
from tests.test_gpu_query import _run, _scene_frames

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
GROWS = ((0, 0, 0), (1, 1, 1), (8, 8, 4), (64, 64, 64))


def _seeds(cfg, n, seed):
    """n seeds {ax, ay, az, ta, bx, by, bz, tb}: random pairs at most 1.5 m apart, zero-length ones, end points on voxel faces (multiples
    of res), seeds touching each face of the map (an end point in the outermost cell), one end outside the map, NaN and inf entries;
    times as tests/test_gpu_cast._segments: ta < 0, ta = tb inside each horizon, ta < tb spanning all horizons, tb < ta"""
    rng = np.random.default_rng(seed)
    half = np.array(common.half_extent(cfg), F)
    res = F(cfg.voxel_resolution)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    a = (rng.uniform(-0.98, 0.98, (n, 3)) * half).astype(F)
    step = rng.standard_normal((n, 3))
    step *= rng.uniform(0.0, 1.5, (n, 1)) / np.linalg.norm(step, axis=1, keepdims=True)
    b = np.clip(a + step, -0.985 * half, 0.985 * half).astype(F)          # (clipping only shortens a pair)
    kind = rng.integers(0, 8, n)
    zero = kind == 2
    b[zero] = a[zero]
    lat = kind == 3                                                       # on voxel faces: integer multiples of res
    ka = np.stack([rng.integers(-(k // 2) + 1, max(k // 2, -(k // 2) + 2), lat.sum()) for k in nn], 1)
    kb = ka + rng.integers(-4, 5, (lat.sum(), 3))
    a[lat] = (ka.astype(F) * res).astype(F)
    b[lat] = (kb.astype(F) * res).astype(F)
    touch = np.flatnonzero(kind == 4)                                     # an end point in the outermost cell of a face, every face in turn
    face = np.arange(touch.size) % 6
    a[touch, face >> 1] = (np.where(face & 1, 1.0, -1.0) * (half[face >> 1] - res * rng.uniform(0.01, 0.99, touch.size))).astype(F)
    b[touch] = np.clip(a[touch] + step[touch] * 0.3, -0.985 * half, 0.985 * half).astype(F)
    b[touch, face >> 1] = a[touch, face >> 1]
    outside = np.flatnonzero(kind == 5)                                   # one end outside the map (some exactly on its faces), either end
    ax = rng.integers(0, 3, outside.size)
    val = (rng.choice([-1.0, 1.0], outside.size) * rng.choice([1.0, 1.0, 1.05, 1.7], outside.size) * half[ax]).astype(F)
    first = rng.random(outside.size) < 0.5
    a[outside[first], ax[first]] = val[first]
    b[outside[~first], ax[~first]] = val[~first]
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


def _ints(boxes):
    return np.ascontiguousarray(boxes).view(np.int32).reshape(-1, 8)


def _assert_same_boxes(got, want, seg, tag):
    assert got.dtype == want.dtype == R.BOX_DTYPE and got.shape == want.shape
    bad = np.flatnonzero((_ints(got) != _ints(want)).any(1))
    assert bad.size == 0, (tag, bad.size, bad[:5], seg[bad[:5]], got[bad[:5]], want[bad[:5]])


def _causes(boxes):
    """[n, 6] cause per face"""
    return (boxes["stop"][:, None] >> (2 * np.arange(6, dtype=np.uint32))[None, :]) & np.uint32(3)


def _grid_cells(m):
    """the bool cells [L, nz, ny, nx] of the grid the map holds now"""
    return R.unpack(m.cast_grid(), m.cfg.nx)


def _shift(seg, cur):
    ss = seg.copy()
    ss[:, 0:3] = (ss[:, 0:3] + cur[None, :]).astype(F)
    ss[:, 4:7] = (ss[:, 4:7] + cur[None, :]).astype(F)
    return ss


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_corridor_bit_parity(dsp, variant):
    kw = dict(SMALL)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    assert np.abs(cur).max() > 0 and int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    thr = _median_threshold(m)
    seg = _seeds(cfg, 6000, 7)
    world_seg = _shift(seg, cur)
    statuses, causes, all_six, checked = set(), set(), 0, 0
    answers = {}
    for r in (0, 2):
        m.build_cast_grid(thr, r)
        lay = _grid_cells(m)                                              # read after the build: what the kernel grows in
        assert lay.any() and not lay.all()
        for grow in GROWS:
            for world in (False, True):
                for wc in (False, True):
                    ss = world_seg if world else seg
                    got = m.grow_boxes(ss, grow, world=world, with_current=wc)
                    want = R.grow(cfg, lay, ss, grow, world=world, with_current=wc, cur_pos=cur)
                    _assert_same_boxes(got, want, ss, (variant, r, grow, world, wc))
                    # the input is not degenerate -- conditions on the restatement's own output
                    ok = want["status"] == R.OK
                    statuses |= set(want["status"].tolist())
                    causes |= set(_causes(want)[ok].ravel().tolist())
                    slo, shi = R.seed_cells(cfg, ss, world, cur)[2:]
                    all_six += int((ok & (want["lo"] < slo).all(1) & (want["hi"] > shi).all(1)).sum())     # extended on all six faces
                    if grow in ((1, 1, 1), (8, 8, 4)) and world == wc:     # the independent checkers on the DEVICE's output
                        assert R.check_contains_seed(cfg, ss, got, world=world, cur_pos=cur) > 3000
                        checked += R.check_free(cfg, lay, ss, got, with_current=wc)
                        seen = R.check_causes(cfg, lay, ss, got, grow, with_current=wc, world=world, cur_pos=cur)
                        assert seen[R.OBSTACLE] >= 1 and seen[R.LIMIT] >= 1
                    answers[(r, grow, world, wc)] = got
    assert statuses == {R.OK, R.SEED_BLOCKED, R.SEED_OUTSIDE, R.INVALID}
    assert causes == {R.OBSTACLE, R.EDGE, R.LIMIT}
    assert all_six >= 1 and checked >= 1
    # the arguments change answers: the limit, the inflation, the extra layer
    assert not np.array_equal(answers[(0, (1, 1, 1), False, False)], answers[(0, (8, 8, 4), False, False)])
    assert not np.array_equal(answers[(0, (8, 8, 4), False, False)], answers[(2, (8, 8, 4), False, False)])
    assert not np.array_equal(answers[(0, (8, 8, 4), False, False)], answers[(0, (8, 8, 4), False, True)])
    m.close()


@pytest.mark.parametrize("shape", ["132x40x12", "50x37x23", "8x8x1", "t0"])
def test_corridor_awkward_shapes(dsp, shape):
    kw = {"50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),        # no multiple of 64 anywhere
          "132x40x12": dict(nx=132, ny=40, nz=12, res=0.15, ppv=9),        # three words per row: boxes across two word boundaries
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
    seg = _seeds(cfg, 3000, 11)
    grow = (64, 64, 64)
    for thr, r in ((_median_threshold(m), 1), (1e9, 0)):
        m.build_cast_grid(thr, r)
        lay = _grid_cells(m)
        for wc in (False, True):
            got = m.grow_boxes(seg, grow, with_current=wc)
            _assert_same_boxes(got, R.grow(cfg, lay, seg, grow, with_current=wc), seg, (shape, thr, wc))
        assert (got["status"] == R.OK).any()
        if thr == 1e9 and shape == "132x40x12":      # an empty grid: boxes that span two and three words of a row
            ok = got[got["status"] == R.OK]
            assert not lay.any()
            for edge in (64, 128):
                assert ((ok["lo"][:, 0] < edge) & (edge <= ok["hi"][:, 0])).any(), edge
            assert ((ok["lo"][:, 0] < 64) & (128 <= ok["hi"][:, 0])).any()
            mid = m.grow_boxes(seg, (20, 3, 3))       # and boxes that start and end inside the words on either side of a boundary
            _assert_same_boxes(mid, R.grow(cfg, lay, seg, (20, 3, 3)), seg, (shape, "mid"))
            ok = mid[mid["status"] == R.OK]
            for edge in (64, 128):
                assert ((ok["lo"][:, 0] < edge) & (edge <= ok["hi"][:, 0]) & (ok["lo"][:, 0] > 0) & (ok["hi"][:, 0] < 131)).any(), edge
    m.close()


def test_corridor_empty_and_dense_grids(dsp):
    kw = dict(SMALL)
    (m,) = _twins(dsp, kw, 1)
    _run(m, _scene_frames(dsp, kw, 6, seed=31))
    cfg = m.cfg
    seg = _seeds(cfg, 4000, 5)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    valid, inside, slo, shi = R.seed_cells(cfg, seg)
    # threshold 1e9: nothing is set, every valid inside seed gives the whole map clipped by the limit, every cause is EDGE or LIMIT
    m.build_cast_grid(1e9, 2)
    lay = _grid_cells(m)
    assert not lay.any()
    for grow in GROWS:
        got = m.grow_boxes(seg, grow, with_current=True)
        _assert_same_boxes(got, R.grow(cfg, lay, seg, grow, with_current=True), seg, ("empty", grow))
        assert ((got["status"] == R.OK) == inside).all() and inside.sum() > 2000
        g = np.array(grow)
        assert (got["lo"][inside] == np.maximum(slo[inside] - g, 0)).all() and (got["hi"][inside] == np.minimum(shi[inside] + g, nn - 1)).all()
        c = _causes(got)[inside]
        lo_edge = (slo[inside] - g <= 0)                                   # c = -1 is met before, or together with, the limit
        hi_edge = (shi[inside] + g >= nn - 1)
        assert (c[:, 0::2] == np.where(lo_edge, R.EDGE, R.LIMIT)).all() and (c[:, 1::2] == np.where(hi_edge, R.EDGE, R.LIMIT)).all()
        assert (got["status"][valid & ~inside] == R.SEED_OUTSIDE).all() and (got["status"][~valid] == R.INVALID).all()
        assert (~valid).sum() >= 10 and (valid & ~inside).sum() >= 200
    # threshold 0.0: wherever a particle lives; many seeds are blocked
    m.build_cast_grid(0.0, 0)
    lay = _grid_cells(m)
    got = m.grow_boxes(seg, (8, 8, 4))
    want = R.grow(cfg, lay, seg, (8, 8, 4))
    _assert_same_boxes(got, want, seg, "dense")
    assert (want["status"] == R.SEED_BLOCKED).sum() > 500      # (every voxel that holds a particle is set)
    R.check_free(cfg, lay, seg, got)
    R.check_causes(cfg, lay, seg, got, (8, 8, 4))
    m.close()


def test_corridor_device_entry_point_stream_ordered_behind_frame(dsp):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    (m,) = _twins(dsp, kw, 1)
    seg = _seeds(m.cfg, 6000, 13)
    sd = torch.from_numpy(np.concatenate([seg, seg], 1)).cuda()[:, :8]      # a non-contiguous view: the binding's temporary
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    keys = ("lo", "hi", "status", "stop")
    grow = (8, 8, 4)
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(0.05, 1)                                       # no synchronisation between the frame, the build and the boxes
            outs.append(m.grow_boxes(sd, grow, world=True, with_current=True))
        st.synchronize()
        after = m.grow_boxes(sd, grow, world=True, with_current=True)
        st.synchronize()
        host = m.grow_boxes(seg, grow, world=True, with_current=True)
        lay = _grid_cells(m)
    for k in keys:
        assert after[k].dtype == torch.int32 and torch.equal(outs[-1][k], after[k]), k
    dev = np.concatenate([after["lo"].cpu().numpy(), after["hi"].cpu().numpy(), after["status"].cpu().numpy()[:, None],
                          after["stop"].cpu().numpy()[:, None]], 1)
    assert np.array_equal(dev, _ints(host))
    assert not all(torch.equal(outs[0][k], outs[-1][k]) for k in keys)
    cur = np.array(frames[-1][1], F)
    want = R.grow(m.cfg, lay, seg, grow, world=True, with_current=True, cur_pos=cur)
    _assert_same_boxes(host, want, seg, "device")
    assert (host["status"] == R.OK).sum() > 100 and (_causes(host)[host["status"] == R.OK] == R.OBSTACLE).any()
    lo_m, hi_m = m.box_bounds(after)                                         # the dict form, and boxes that hold their seeds in metres
    lo_h, hi_h = m.box_bounds(host)
    assert np.array_equal(lo_m, lo_h, equal_nan=True) and np.array_equal(hi_m, hi_h, equal_nan=True)
    ok = host["status"] == R.OK
    for p in (seg[ok, 0:3] - cur[None, :], seg[ok, 4:7] - cur[None, :]):
        assert (lo_h[ok] <= p + 1e-4).all() and (p - 1e-4 <= hi_h[ok]).all()
    m.close()


def test_corridor_is_read_only_and_follows_the_grid(dsp):
    kw = dict(SMALL)
    m, twin = _twins(dsp, kw)
    frames = _scene_frames(dsp, kw, 7, seed=31)
    for x in (m, twin):
        _run(x, frames[:6])
    thr = _median_threshold(m)
    seg = _seeds(m.cfg, 2000, 3)
    sd = torch.from_numpy(seg).cuda()
    for x in (m, twin):
        x.build_cast_grid(thr, 1)
    grid, ptr = m.cast_grid(), m.cast_grid_ptr()
    b0 = m.grow_boxes(seg, (8, 8, 4))                                        # the twin builds the same grid and never grows a box
    m.grow_boxes(sd, (64, 64, 64), world=True, with_current=True)
    torch.cuda.synchronize()
    # the grid's words are identical before and after a call and the grid is still valid ...
    assert m.cast_grid_ptr() == ptr and np.array_equal(m.cast_grid(), grid) and np.array_equal(twin.cast_grid(), grid)
    assert m.grow_boxes(seg, (8, 8, 4)).tobytes() == b0.tobytes()
    _assert_same_boxes(b0, R.grow(m.cfg, R.unpack(grid, m.cfg.nx), seg, (8, 8, 4)), seg, "read-only")
    # ... and so is what the map hands out (getFutureStatus is a consuming readout: the twin's is the "before")
    assert np.array_equal(m.results(), twin.results())
    fut = m.getFutureStatus()
    assert np.array_equal(fut, twin.getFutureStatus()) and (fut != 0).any()
    for x, y in zip(m.export_state(), twin.export_state()):
        assert np.array_equal(x, y)
    twin.close()
    # the next frame makes the grid stale: E_STATE naming the build, on both entry points
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    box = np.zeros(len(seg), R.BOX_DTYPE)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    g = (C.c_int * 3)(8, 8, 4)
    assert m.L.dspmap_grow_boxes(m.h, len(seg), p(seg), g, 0, p(box)) == E_STATE
    assert b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    assert not box.view(np.int32).any()
    with pytest.raises(dsp.capi.DSPMapError):
        m.grow_boxes(sd, (8, 8, 4))
    # ... and a rebuild makes the call work again
    m.build_cast_grid(thr, 1)
    again = m.grow_boxes(seg, (8, 8, 4))
    _assert_same_boxes(again, R.grow(m.cfg, _grid_cells(m), seg, (8, 8, 4)), seg, "rebuilt")
    assert again.tobytes() != b0.tobytes()
    m.close()
