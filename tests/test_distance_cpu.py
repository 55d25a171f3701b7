"""CPU tests of the distance fields (dspmap_build_distance_field, dspmap_get_distance_field, dspmap_query_distance*): the entry points
are exported and bound, argument errors are DSPMAP_E_ARG before any device is touched, a slab handle and a missing field are
DSPMAP_E_STATE, a valid build needs a device, and known answers of the numpy restatement (tests/distance_ref.py) that the GPU tests
hold the kernels to, with its two routes to the squared distance checked against each other."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import distance_ref as D

E_ARG, E_DEVICE, E_STATE = -1, -2, -3
NAMES = ("dspmap_build_distance_field", "dspmap_distance_field_device", "dspmap_get_distance_field", "dspmap_query_distance",
         "dspmap_query_distance_device")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_distance_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    assert dsp.capi.DIST_OUTSIDE_OCCUPIED == 1
    for meth in ("build_distance_field", "distance_field", "distance_field_ptr", "query_distance"):
        assert callable(getattr(dsp.DSPMap, meth))


def test_distance_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    assert L.dspmap_build_distance_field(None, 0.5, 20, 0) == E_ARG
    assert L.dspmap_build_distance_field(h, float("nan"), 20, 0) == E_ARG
    assert b"NaN" in L.dspmap_last_error(h)
    for r in (0, -1, 65, 1 << 20):
        assert L.dspmap_build_distance_field(h, 0.5, r, 0) == E_ARG, r
    assert b"max_voxels" in L.dspmap_last_error(h)
    for fl in (2, 3, -1):
        assert L.dspmap_build_distance_field(h, 0.5, 20, fl) == E_ARG, fl
    assert b"flags" in L.dspmap_last_error(h)
    out = np.zeros(20 * 20 * 10, F)
    assert L.dspmap_get_distance_field(None, 0, _p(out)) == E_ARG
    assert L.dspmap_get_distance_field(h, 0, None) == E_ARG
    for layer in (-1, 7, 100):       # T = 6: layers 0 .. 6
        assert L.dspmap_get_distance_field(h, layer, _p(out)) == E_ARG, layer
    assert L.dspmap_distance_field_device(None) is None
    q, dist, grad = np.zeros((8, 4), F), np.zeros(8, F), np.zeros((8, 3), F)
    for fn in (L.dspmap_query_distance, L.dspmap_query_distance_device):
        assert fn(None, 4, _p(q), 0, 0.0, _p(dist), _p(grad)) == E_ARG
        assert fn(h, -1, _p(q), 0, 0.0, _p(dist), _p(grad)) == E_ARG
        assert fn(h, 4, None, 0, 0.0, _p(dist), _p(grad)) == E_ARG
        assert fn(h, 4, _p(q), 0, 0.0, None, _p(grad)) == E_ARG
        assert fn(h, 4, _p(q), 2, 0.0, _p(dist), _p(grad)) == E_ARG
        assert fn(h, 4, _p(q), 0, float("nan"), _p(dist), _p(grad)) == E_ARG
    m.close()


def test_distance_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    assert L.dspmap_build_distance_field(m.h, 0.5, 20, 0) == E_STATE
    assert b"slab" in L.dspmap_last_error(m.h)
    assert L.dspmap_build_distance_field(m.h, float("nan"), 20, 0) == E_ARG     # the argument checks come first
    m.close()


def test_distance_read_before_build_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    out = np.zeros(20 * 20 * 10, F)
    q, dist, grad = np.zeros((8, 4), F), np.zeros(8, F), np.zeros((8, 3), F)
    assert L.dspmap_get_distance_field(m.h, 0, _p(out)) == E_STATE
    assert b"dspmap_build_distance_field" in L.dspmap_last_error(m.h)
    assert L.dspmap_query_distance(m.h, 8, _p(q), 0, 0.0, _p(dist), _p(grad)) == E_STATE
    assert L.dspmap_query_distance_device(m.h, 8, _p(q), 0, 0.0, _p(dist), None) == E_STATE
    assert L.dspmap_distance_field_device(m.h) is None and m.distance_field_ptr() is None
    with pytest.raises(dsp.capi.DSPMapError):
        m.distance_field(0)
    with pytest.raises(dsp.capi.DSPMapError):
        m.query_distance(q)
    m.close()


def test_distance_valid_build_needs_device(dsp):
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    want = 1 if torch.cuda.is_available() else E_DEVICE   # (no CPU fallback: without a device every valid call fails)
    assert L.dspmap_build_distance_field(m.h, 0.5, 20, 1) == want
    if want == E_DEVICE:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError):
            m.build_distance_field(0.5, 20)
        assert m.distance_field_ptr() is None
    m.close()


# ---- known answers of the restatement on a hand-built 4 x 4 x 4 grid at 0.5 m (half = 1 m, centres -0.75, -0.25, 0.25, 0.75)
RES = F(0.5)


def _occ(*voxels):
    o = np.zeros((4, 4, 4), bool)          # [z, y, x]
    for x, y, z in voxels:
        o[z, y, x] = True
    return o


def test_distance_ref_single_voxel():
    d2 = D.d2_separable(_occ((1, 2, 3)))
    assert np.array_equal(d2, D.d2_brute(_occ((1, 2, 3))))
    assert d2[3, 2, 1] == 0 and d2[3, 2, 0] == 1 and d2[0, 0, 3] == 4 + 4 + 9
    v = D.value(d2, 64, RES)
    assert v.dtype == F and v[3, 2, 1] == 0 and v[3, 2, 3] == F(1.0) and v[3, 3, 2] == F(np.sqrt(F(2))) * RES
    assert v[0, 0, 3] == F(np.sqrt(F(17))) * RES


def test_distance_ref_exact_tie_at_r_squared():
    d2 = D.d2_separable(_occ((0, 0, 0)))
    assert d2[2, 2, 1] == 9 and d2[0, 0, 3] == 9                      # (1, 2, 2) and (3, 0, 0): both exactly 3 voxels away
    v3, v2 = D.value(d2, 3, RES), D.value(d2, 2, RES)
    assert v3[2, 2, 1] == F(1.5) and v3[0, 0, 3] == F(1.5)            # D2 == R^2: the clamp changes nothing
    assert v3[3, 3, 3] == F(1.5) and d2[3, 3, 3] == 27               # further away: truncated to R * res
    assert v3[2, 2, 0] == F(np.sqrt(F(8))) * RES                      # just inside
    assert v2[2, 2, 1] == F(1.0) and v2[0, 0, 1] == F(0.5) and v2[0, 0, 2] == F(1.0)


def test_distance_ref_empty_layer_reads_r_times_res():
    d2 = D.d2_separable(_occ())
    assert (d2 == D.INF).all() and np.array_equal(d2, D.d2_brute(_occ()))
    for R in (1, 20, 64):
        assert (D.value(d2, R, RES) == F(R) * RES).all()
    cfg_like = type("Cfg", (), dict(nx=4, ny=4, nz=4, voxel_resolution=0.5, prediction_times=2))
    res = np.zeros((64, 4), F)
    fut = np.zeros((64, 2), F)
    fut[5, 1] = 1.0
    fld = D.field(cfg_like, res, fut, 0.5, 7)
    assert fld.shape == (3, 4, 4, 4) and (fld[0] == F(3.5)).all() and (fld[1] == F(3.5)).all()
    assert fld[2, 0, 1, 1] == 0 and fld[2, 0, 1, 2] == F(0.5)        # voxel 5 = (x 1, y 1, z 0)
    assert (D.field(cfg_like, res, fut, 1.0, 7)[2] == F(3.5)).all()   # the comparison is strict (:394)


def test_distance_ref_outside_occupied_faces():
    e = D.outside_d2((4, 4, 4))
    assert e[0, 0, 0] == 1 and e[1, 1, 1] == 4 and e[2, 2, 2] == 4 and e[3, 1, 1] == 1 and e[1, 2, 3] == 1
    v = D.value(D.d2_separable(_occ()), 64, RES, outside_occupied=True)
    assert v[0, 2, 2] == F(0.5) and v[1, 1, 1] == F(1.0) and v[2, 1, 2] == F(1.0) and v[2, 3, 2] == F(0.5)
    e = D.outside_d2((1, 5, 6))                                        # a one-layer map: both z faces are one step away
    assert (e == 1).all()
    e = D.outside_d2((9, 9, 9))
    assert e[4, 4, 4] == 25 and e[4, 4, 5] == 16
    # an occupied voxel nearer than the face wins, and the other way round
    v = D.value(D.d2_separable(_occ((1, 1, 1))), 64, RES, outside_occupied=True)
    assert v[1, 1, 1] == 0 and v[2, 2, 2] == F(np.sqrt(F(3))) * RES and v[2, 2, 3] == F(0.5)


def test_distance_ref_query_and_one_sided_gradients(dsp):
    cfg = dsp.make_config(nx=4, ny=4, nz=4, res=0.5, pred_times=(0.1, 0.5))
    fld = np.zeros((3, 4, 4, 4), F)
    fld[0] = (np.arange(4)[None, None, :] * 1.0 + np.arange(4)[None, :, None] * 10.0 + np.arange(4)[:, None, None] * 100.0).astype(F)
    fld[1] = fld[0] * F(2)
    fld[2] = (np.arange(4)[None, None, :] ** 2).astype(F) * np.ones((4, 4, 1), F)
    q = np.array([[-0.25, 0.25, 0.25, -1.0],     # voxel (1, 2, 2), layer 0: central differences over 2 * res = 1 m
                  [-0.75, 0.75, -0.75, -1.0],    # (0, 3, 0): one-sided at three faces, over res = 0.5 m
                  [-0.25, 0.25, 0.25, 0.05],     # layer 1
                  [0.75, 0.25, 0.25, 0.3],       # (3, 2, 2) layer 2: x one-sided (9 - 4) / 0.5
                  [0.25, 0.25, 0.25, 9.0],       # (2, 2, 2) layer 2 (clamped horizon): (9 - 1) / 1
                  [1.5, 0.0, 0.0, -1.0],         # outside
                  [np.nan, 0.0, 0.0, -1.0]], F)
    dist, grad = D.query(cfg, fld, q, outside=7.0)
    assert list(dist) == [221.0, 30.0, 442.0, 9.0, 4.0, 7.0, 7.0]
    assert grad[0].tolist() == [2.0, 20.0, 200.0]
    assert grad[1].tolist() == [2.0, 20.0, 200.0]
    assert grad[2].tolist() == [4.0, 40.0, 400.0]
    assert grad[3].tolist() == [10.0, 0.0, 0.0]
    assert grad[4].tolist() == [8.0, 0.0, 0.0]
    assert grad[5].tolist() == [0.0, 0.0, 0.0] and grad[6].tolist() == [0.0, 0.0, 0.0]
    dw, gw = D.query(cfg, fld, q + np.array([10.0, -5.0, 1.0, 0.0], F), world=True, cur_pos=(10.0, -5.0, 1.0), outside=7.0)
    assert np.array_equal(dw, dist) and np.array_equal(gw, grad)
    flat = dsp.make_config(nx=4, ny=4, nz=1, res=0.5, pred_times=())      # n == 1 along z: no z gradient; T == 0: always layer 0
    d1, g1 = D.query(flat, fld[:1, :1], np.array([[-0.25, 0.25, 0.0, 3.0]], F))
    assert d1[0] == 21.0 and g1[0].tolist() == [2.0, 20.0, 0.0]


def test_distance_ref_brute_force_equals_separable():
    rng = np.random.default_rng(2024)
    try:
        from scipy import ndimage
    except Exception:  # noqa: BLE001
        ndimage = None
    n_cases = 0
    for case in range(24):
        shape = tuple(int(v) for v in rng.integers(1, 12, 3))
        if case < 3:
            shape = [(1, 9, 13), (11, 1, 7), (5, 12, 1)][case]
        density = [0.0, 0.002, 0.02, 0.2, 0.9, 1.0][case % 6]
        occ = rng.random(shape) < density
        if case % 6 == 1:
            occ.flat[rng.integers(0, occ.size)] = True
        a, b = D.d2_brute(occ), D.d2_separable(occ)
        assert np.array_equal(a, b), (case, shape)
        assert (b[occ] == 0).all() and ((b == D.INF).all() if not occ.any() else (b < D.INF).all())
        if ndimage is not None and occ.any():
            edt = ndimage.distance_transform_edt(~occ)
            assert np.array_equal(np.rint(edt * edt).astype(np.int64), b), (case, shape)
        for R in (1, 3, 64):
            for oo in (False, True):
                v = D.value(b, R, 0.15, oo)
                assert v.dtype == F and v.max() <= F(R) * F(0.15) and (v[occ] == 0).all()
        n_cases += 1
    assert n_cases >= 20


def test_dropin_class_offers_distance_fields(dsp, tmp_path):
    """include/dsp_dynamic.h: buildDistanceField / getDistanceField / queryDistance type-check and forward to the C ABI"""
    src = tmp_path / "df.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n    dspmap_query s[2] = {};\n    float d[2], g[6], f[8];\n'
                   "    int a = my_map.buildDistanceField();\n    int b = my_map.buildDistanceField(0.5f, 64, true);\n"
                   "    int c = my_map.getDistanceField(0, f);\n    int e = my_map.queryDistance(2, s, d);\n"
                   "    int h = my_map.queryDistance(2, s, d, g, true, -1.f);\n    return a + b + c + e + h;\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for fn in ("dspmap_build_distance_field(h_", "dspmap_get_distance_field(h_", "dspmap_query_distance(h_"):
        assert fn in hdr, fn
