"""CPU tests of the point / trajectory queries (dspmap_query_occupancy*, dspmap_trajectory_risk*): the entry points are exported
and bound, argument errors are DSPMAP_E_ARG before any device is touched, a valid call needs a device, and known answers of the
numpy restatement (tests/query_ref.py) that the GPU tests hold the kernels to."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import query_ref as Q

E_ARG, E_DEVICE, E_STATE = -1, -2, -3
NAMES = ("dspmap_query_occupancy", "dspmap_query_occupancy_device", "dspmap_trajectory_risk", "dspmap_trajectory_risk_device")
F = np.float32


def test_query_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    assert dsp.capi.RISK_DTYPE.itemsize == 16


def _bufs(dsp, n):
    return np.zeros((n, 4), F), np.zeros(n, F), np.zeros(n, dsp.capi.RISK_DTYPE)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_query_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    q, out, rk = _bufs(dsp, 8)
    rmax = float(F(8) * F(0.15))
    for fn in (L.dspmap_query_occupancy, L.dspmap_query_occupancy_device):
        assert fn(None, 4, _p(q), 0.0, 0, 1.0, _p(out)) == E_ARG
        assert fn(h, -1, _p(q), 0.0, 0, 1.0, _p(out)) == E_ARG
        assert fn(h, 4, None, 0.0, 0, 1.0, _p(out)) == E_ARG
        assert fn(h, 4, _p(q), 0.0, 0, 1.0, None) == E_ARG
        for r in (-0.01, float(np.nextafter(F(rmax), F(10))), float("nan"), float("inf")):
            assert fn(h, 4, _p(q), r, 0, 1.0, _p(out)) == E_ARG, r
        assert fn(h, 4, _p(q), 0.0, 2, 1.0, _p(out)) == E_ARG
        assert fn(h, 4, _p(q), 0.0, 0, float("nan"), _p(out)) == E_ARG
    assert b"radius" in L.dspmap_last_error(h) or b"outside" in L.dspmap_last_error(h)
    for fn in (L.dspmap_trajectory_risk, L.dspmap_trajectory_risk_device):
        assert fn(None, 2, 4, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, -1, 4, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, 2, 0, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, 2, -3, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, 2, 4, None, 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, 2, 4, _p(q), 0.0, 0, 1.0, 0.5, None) == E_ARG
        assert fn(h, 2, 4, _p(q), rmax * 2, 0, 1.0, 0.5, _p(rk)) == E_ARG
        assert fn(h, 1 << 16, 1 << 16, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_ARG   # 2^32 samples: size overflow
    assert b"INT_MAX" in L.dspmap_last_error(h)
    m.close()


def test_query_risk_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    q, out, rk = _bufs(dsp, 8)
    for fn in (L.dspmap_trajectory_risk, L.dspmap_trajectory_risk_device):
        assert fn(m.h, 2, 4, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == E_STATE
    m.close()


def test_query_valid_call_needs_device(dsp):
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    q, out, rk = _bufs(dsp, 8)
    want = 1 if torch.cuda.is_available() else E_DEVICE   # (no CPU fallback: without a device every valid call fails)
    assert L.dspmap_query_occupancy(m.h, 8, _p(q), 0.3, 1, 1.0, _p(out)) == want
    assert L.dspmap_trajectory_risk(m.h, 2, 4, _p(q), 0.0, 0, 1.0, 0.5, _p(rk)) == want
    if want == E_DEVICE:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError):
            m.query_occupancy(q)
        with pytest.raises(dsp.capi.DSPMapError):
            m.trajectory_risk(q.reshape(2, 4, 4))
    m.close()


# ---- known answers of the restatement on a hand-built 4 x 4 x 4 grid at 0.5 m (half = 1 m, centres -0.75, -0.25, 0.25, 0.75)
PRED = (0.05, 0.2, 0.5, 1.0, 1.5, 2.0)


@pytest.fixture(scope="module")
def grid(dsp):
    cfg = dsp.make_config(nx=4, ny=4, nz=4, res=0.5, pred_times=PRED)
    V = 64
    res = np.zeros((V, 4), F)
    res[:, 0] = np.arange(V) + 1                              # current mass of voxel v: v + 1
    fut = (100 * (np.arange(6)[None, :] + 1) + np.arange(V)[:, None]).astype(F)   # horizon k of voxel v: 100 (k + 1) + v
    return cfg, res, fut


def vox(x, y, z):
    return (z * 4 + y) * 4 + x


def one(grid, x, y, z, t, **kw):
    cfg, res, fut = grid
    v, f = Q.query(cfg, res, fut, np.array([[x, y, z, t]], F), **kw)
    return float(v[0]), bool(f[0])


def test_query_ref_own_voxel_and_faces(grid):
    assert one(grid, 0.25, 0.25, 0.25, -1) == (vox(2, 2, 2) + 1, False)
    assert one(grid, 0.0, -0.25, -0.25, -1) == (vox(2, 1, 1) + 1, False)    # x on the face between voxels 1 and 2: (0 + 1) / 0.5 = 2
    assert one(grid, -0.5, -0.5, -0.5, -1) == (vox(1, 1, 1) + 1, False)      # a corner of four voxels
    assert one(grid, -1.0, 0.0, 0.0, -1, outside=7.0) == (7.0, True)         # |x| == half: outside (:1118-1125)
    assert one(grid, 0.999, 0.999, 0.999, -1) == (vox(3, 3, 3) + 1, False)


def test_query_ref_horizons(grid):
    v = vox(2, 2, 2)
    assert one(grid, 0.25, 0.25, 0.25, -0.5)[0] == v + 1
    assert one(grid, 0.25, 0.25, 0.25, 0.0)[0] == 100 + v                   # t = 0: the first horizon
    assert one(grid, 0.25, 0.25, 0.25, 0.2)[0] == 200 + v                   # exactly on horizon 1
    assert one(grid, 0.25, 0.25, 0.25, 0.3)[0] == 300 + v                   # between 0.2 and 0.5: the next one up
    assert one(grid, 0.25, 0.25, 0.25, 2.0)[0] == 600 + v                   # the last horizon
    assert one(grid, 0.25, 0.25, 0.25, 5.0)[0] == 600 + v                   # past the last: clamped
    assert one(grid, 0.25, 0.25, 0.25, float("inf"))[0] == 600 + v
    assert list(Q.horizons(np.array([], F), np.array([-1, 0, 3], F))) == [-1, -1, -1]   # T == 0: the current mass


def test_query_ref_radius_on_centre_distance(grid):
    # the six face neighbours of voxel (2, 2, 2) are exactly 0.5 m away: d2 = 0.25 = fl(r * r) -> inside; diagonals (0.707 m) are not
    assert one(grid, 0.25, 0.25, 0.25, -1, radius=0.5)[0] == vox(2, 2, 3) + 1
    assert one(grid, 0.25, 0.25, 0.25, -1, radius=float(np.nextafter(F(0.5), F(0))))[0] == vox(2, 2, 2) + 1
    assert one(grid, 0.25, 0.25, 0.25, -1, radius=0.71)[0] == vox(2, 3, 3) + 1   # the largest of the 12 edge neighbours
    # the corner voxel (3, 3, 3): its +x / +y / +z neighbours are outside the map and contribute `outside`
    assert one(grid, 0.75, 0.75, 0.75, 0.2, radius=0.5, outside=1000.0) == (1000.0, False)
    assert one(grid, 0.75, 0.75, 0.75, 0.2, radius=0.49, outside=1000.0) == (200 + vox(3, 3, 3), False)


def test_query_ref_outside_nan_and_world(grid):
    # a point outside the map reads `outside`, raised by the map voxels within r
    assert one(grid, 1.1, 0.75, 0.75, -1, radius=0.3, outside=0.5) == (0.5, True)             # (3,3,3) centre 0.35 m away
    assert one(grid, 1.1, 0.75, 0.75, -1, radius=0.4, outside=0.5) == (vox(3, 3, 3) + 1, True)
    assert one(grid, 50.0, 0.0, 0.0, 1.0, radius=0.4, outside=0.5) == (0.5, True)
    for s in ((np.nan, 0, 0, -1), (0, np.nan, 0, 1), (0, 0, np.nan, 1), (0.25, 0.25, 0.25, np.nan)):
        assert one(grid, *s, radius=0.5, outside=3.0) == (3.0, True)
    # world frame: p = fl(q - cur_pos)
    assert one(grid, 10.25, -4.75, 1.25, -1, world=True, cur_pos=(10.0, -5.0, 1.0)) == (vox(2, 2, 2) + 1, False)
    assert one(grid, 10.25, -4.75, 1.25, -1, world=False, outside=2.0) == (2.0, True)


def test_query_ref_risk(grid):
    cfg, res, fut = grid
    tr = np.array([[[-0.75, -0.75, -0.75, -1], [-0.25, -0.75, -0.75, -1], [0.25, -0.75, -0.75, -1], [1.25, -0.75, -0.75, -1]],
                   [[0.0, 0.0, 5.0, -1], [0.0, 0.0, np.nan, 0.5], [-0.25, -0.25, -0.25, 0.05], [0.1, 0.1, 0.1, -1]]], F)
    v, f = Q.query(cfg, res, fut, tr.reshape(-1, 4), outside=2.5)
    assert list(v) == [1, 2, 3, 2.5, 2.5, 2.5, 100 + vox(1, 1, 1), vox(2, 2, 2) + 1]
    s, mx, first, nout = Q.risk(v, f, 4, threshold=2.0)
    assert list(s) == [F(8.5), F(F(F(2.5 + 2.5) + 121) + 43)]
    assert list(mx) == [3, 121] and list(first) == [2, 0] and list(nout) == [1, 2]
