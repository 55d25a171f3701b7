"""CPU tests of the known-space layer (dspmap_known_integrate and the calls next to it): the numpy restatement (tests/known_ref.py) that
the GPU tests hold the kernels to gives the answers worked by hand -- the window table, the cells a moving window resets, what a flat
wall hides --, the entry points are exported and bound, every argument error is DSPMAP_E_ARG with a text before any device is touched, a
valid call needs a device, and the drop-in class offers the new members."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import known_ref as K

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_known_integrate", "dspmap_known_reset", "dspmap_get_known", "dspmap_query_known", "dspmap_query_known_device",
         "dspmap_mask_cast_grid", "dspmap_known_stats", "dspmap_get_view")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = F(0.15)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the window
def test_window_table_known_answers():
    """k0 and o for cur at 0, at -0.01, at exactly res / 2 and at -4 res, for n = 66 (even) and n = 3 (odd); worked by hand from
    g = cur / res - n / 2, k0 = floor(g + 0.5), o = (k0 + 0.5) res - cur"""
    r = float(RES)
    c = float(F(-0.01))
    table = {
        (0.0, 66): (-33, -32.5 * r), (0.0, 3): (-1, -0.5 * r),
        (c, 66): (-33, -32.5 * r - c), (c, 3): (-2, -1.5 * r - c),                  # g = -33.07 / -1.57: the odd map's window has moved on
        (r / 2, 66): (-32, -32.0 * r), (r / 2, 3): (-1, -1.0 * r),                  # g + 0.5 is the integer -32 / a half: floor keeps it
        (-4 * r, 66): (-37, -32.5 * r), (-4 * r, 3): (-5, -0.5 * r),                # a whole number of cells: the offsets of cur = 0
    }
    for (cur, n), (k0, o) in table.items():
        got = K.window_axis(cur, RES, n)
        assert got[0] == k0 and got[1] == F(o) and got[1].dtype == F, (cur, n, got)
    # the voxel's centre lies in its lattice cell, and o is that cell's centre seen from the sensor -- over a sweep through negative coordinates
    for n in (3, 16, 66):
        for cur in np.linspace(-3.0, 3.0, 241).astype(F):
            k0, o = K.window_axis(cur, RES, n)
            centre = float(cur) + (0.5 - n / 2.0) * r                               # voxel 0, world frame
            assert k0 * r <= centre < (k0 + 1) * r, (n, cur)
            assert abs(float(o) - ((k0 + 0.5) * r - float(cur))) <= 1e-6


def test_window_shift_resets_exactly_the_entering_cells(dsp):
    """a shift by 1, n - 1, n and n + 3 cells along x (and a diagonal one) keeps the stamps of the cells that stay, where they now are, and
    nothing else"""
    cfg = dsp.make_config(nx=7, ny=5, nz=3, res=0.15)
    n = 7
    q = 0.25 * float(RES)                                                           # (a quarter cell off the lattice: float rounding of the positions decides nothing)
    for shift, kept in ((1, 6), (n - 1, 1), (n, 0), (n + 3, 0), (-2, 5), (-n, 0)):
        lay = K.Layer(cfg)
        lay.sync((q, q, q))
        lay.stamp[:] = np.arange(1, 7 * 5 * 3 + 1).reshape(3, 5, 7)
        before = lay.stamp.copy()
        ages = lay.ages((q + shift * float(RES), q, q), 1000)
        assert lay.k0[0] == K.window_axis(q, RES, n)[0] + shift
        known = ages >= 0
        assert known.sum() == kept * 5 * 3, shift
        if shift > 0:
            assert known[:, :, :kept].all() and np.array_equal(lay.stamp[:, :, :kept], before[:, :, shift:shift + kept])
        else:
            assert known[:, :, n - kept:].all() and np.array_equal(lay.stamp[:, :, n - kept:], before[:, :, :kept])
    lay = K.Layer(cfg)
    lay.sync((q, q, q))
    lay.stamp[:] = 5
    ages = lay.ages((q + 2 * float(RES), q - float(RES), q + float(RES)), 9)        # +2 in x, -1 in y, +1 in z
    want = np.full((3, 5, 7), -1)
    want[:2, 1:, :5] = 4
    assert np.array_equal(ages, want)
    lay.sync((q, q, q))                                                             # and back: what left is gone
    assert (lay.stamp != 0).sum() == 2 * 4 * 5 and (lay.stamp[1:, :4, 2:] == 5).all()


# ---- the view
def _flat_wall(dist=2.0):
    y, z = np.meshgrid(np.linspace(-2.5, 2.5, 201), np.linspace(-1.2, 1.2, 97))
    return np.stack([np.full(y.size, dist), y.ravel(), z.ravel()], 1).astype(F)


def test_flat_wall_known_answers(dsp):
    cfg = dsp.make_config(nx=40, ny=40, nz=24, res=0.15)
    cur = (0.0, 0.0, 0.0)
    px, py, pz = K.centres(cfg, cur)
    assert px[26] == F(F(26 * RES) + F(-19.5 * float(RES))) and abs(px[26] - 0.975) < 1e-6 and abs(pz[12] - 0.075) < 1e-6
    ph, pv, ml = K.bin_cloud(cfg, _flat_wall())
    assert ph.shape == (29, 3) and pv.shape == (17, 3) and ml.shape == (28 * 16,)
    assert (ml > 0).all() and ml.min() >= 2.0 and ml.max() < 2.0 / np.cos(np.radians(42)) / np.cos(np.radians(24)) + 0.1
    seen, occluded, beyond, outside = K.classify(cfg, cur, ph, pv, ml)
    assert ((seen.astype(int) + occluded + beyond + outside) == 1).all() and not beyond.any()
    assert seen[12, 20, 26]                                                         # 1 m in front of the sensor
    assert occluded[12, 20, 36] and not seen[12, 20, 36]                            # 2.475 m: behind the wall by more than the 0.3 m margin
    assert seen[12, 20, 34] and abs(px[34] - 2.175) < 1e-6                          # 2.175 m: behind the wall, inside the margin
    assert outside[12, 20, 13] and outside[23, 20, 22] and outside[12, 39, 22]      # behind, above and beside the wedge
    assert seen.sum() > 1000 and occluded.sum() > 1000 and outside.sum() > 1000
    # the restated bisection and the reference's linear scan name the same pyramid
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, (1500, 3)).astype(F)
    b = K.pyramid_of(ph, pv, pts[:, 0], pts[:, 1], pts[:, 2])
    assert (b >= 0).sum() > 60 and b.max() < 28 * 16
    assert b.tolist() == [K.pyramid_of_linear(ph, pv, *p) for p in pts]
    # no return anywhere: every cell of the wedge is seen through, up to max_range
    empty = np.full(28 * 16, -1, F)
    s_inf, o_inf, b_inf, out_inf = K.classify(cfg, cur, ph, pv, empty)
    assert np.array_equal(s_inf, ~outside) and not o_inf.any() and not b_inf.any()
    s15, o15, b15, _ = K.classify(cfg, cur, ph, pv, empty, max_range=1.5)
    z, y, x = np.meshgrid(pz, py, px, indexing="ij")
    dist = np.sqrt(x.astype(np.float64) ** 2 + y ** 2 + z ** 2)
    assert not o15.any() and s15.sum() > 100 and b15.sum() > 100
    assert np.array_equal(s15[np.abs(dist - 1.5) > 1e-4], (~outside & (dist <= 1.5))[np.abs(dist - 1.5) > 1e-4])
    # a range that cuts in front of the wall beats the occlusion test only where the wall does not
    s1, o1, b1, _ = K.classify(cfg, cur, ph, pv, ml, max_range=1.0)
    assert np.array_equal(o1, occluded) and s1[12, 20, 26] and b1[12, 20, 28] and not s1[12, 20, 28]
    # a yaw of 90 degrees turns the wedge towards +y
    phr, pvr, mlr = K.bin_cloud(cfg, _flat_wall(), (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)))
    sr = K.classify(cfg, cur, phr, pvr, mlr)[0]
    assert sr[12, 26, 20] and not sr[12, 20, 26] and not sr[12, 36, 20]


def test_layer_stamps_ages_and_queries(dsp):
    cfg = dsp.make_config(nx=16, ny=16, nz=6, res=0.15)
    ph, pv, ml = K.bin_cloud(cfg, _flat_wall(0.6))
    lay = K.Layer(cfg)
    assert (lay.ages((0, 0, 0), 1) == -1).all()
    seen = lay.integrate((0, 0, 0), ph, pv, ml, 1)
    a1 = lay.ages((0, 0, 0), 1)
    assert 20 < seen.sum() < 16 * 16 * 6 and np.array_equal(a1 == 0, seen) and np.array_equal(a1 == -1, ~seen)
    lay.integrate((0, 0, 0), ph, pv, ml, 1)
    assert np.array_equal(lay.ages((0, 0, 0), 1), a1)                                # twice is once
    a4 = lay.ages((0, 0, 0), 4)
    assert np.array_equal(a4, np.where(seen, 3, -1))
    assert K.stats(a4, 2) == (0, 0) and K.stats(a4, 3) == (int(seen.sum()), 0) and K.stats(a1, 0) == (int(seen.sum()), int(seen.sum()))
    assert np.array_equal(K.unknown(a4, 2), np.ones_like(seen)) and np.array_equal(K.unknown(a4, 3), ~seen)
    # queries: centres, a face (the upper cell owns it), outside, NaN; t ignored
    res = float(RES)
    c = lambda x, y, z: (-8 * res + (x + 0.5) * res, -8 * res + (y + 0.5) * res, -3 * res + (z + 0.5) * res)   # noqa: E731
    zi, yi, xi = np.argwhere(seen)[0]
    q = np.array([c(xi, yi, zi) + (0.0,), c(xi, yi, zi) + (np.nan,), c(0, 0, 0) + (1.0,), (8 * res, 0, 0, 0), (np.nan, 0, 0, 0),
                  (-8 * res + (xi + 1) * res, c(xi, yi, zi)[1], c(xi, yi, zi)[2], 0.0)], F)
    got = K.query(cfg, a4, q)
    assert got.tolist()[:5] == [3, 3, int(a4[0, 0, 0]), -1, -1] and got[5] == a4[zi, yi, min(xi + 1, 15)]
    cur = np.array([3.0, -2.0, 0.5], F)
    qw = q.copy()
    qw[:, :3] = (qw[:, :3] + cur).astype(F)
    assert np.array_equal(K.query(cfg, a4, qw, world=True, cur_pos=cur)[[0, 1, 3, 4]], got[[0, 1, 3, 4]])
    lay.reset()
    assert (lay.ages((0, 0, 0), 4) == -1).all()


# ---- the library without a device
def test_known_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    for meth in ("integrate_known", "reset_known", "known_age", "query_known", "mask_cast_grid", "known_stats", "view"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert "int %s(dspmap_t* m" % n in hdr, n
    assert '"dspmap_known.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()


def test_known_argument_errors_without_a_device(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    assert L.dspmap_known_integrate(None, 5.0, 0) == E_ARG
    for r in (float("nan"), 0.0, -0.0, -1.0, -float("inf")):
        assert L.dspmap_known_integrate(h, r, 0) == E_ARG and b"max_range" in err(), r
    for fl in (1, 2, -1):
        assert L.dspmap_known_integrate(h, 5.0, fl) == E_ARG and b"flags" in err(), fl
    assert L.dspmap_known_reset(None) == E_ARG
    ages = np.zeros(m.V, np.int32)
    assert L.dspmap_get_known(None, _p(ages)) == E_ARG
    assert L.dspmap_get_known(h, None) == E_ARG and b"NULL" in err()
    q, out = np.zeros((4, 4), F), np.zeros(4, np.int32)
    for fn in (L.dspmap_query_known, L.dspmap_query_known_device):
        assert fn(None, 4, _p(q), 0, _p(out)) == E_ARG
        assert fn(h, -1, _p(q), 0, _p(out)) == E_ARG and b"negative" in err()
        assert fn(h, 4, None, 0, _p(out)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(q), 0, None) == E_ARG and b"NULL" in err()
        for fl in (2, 4, -1):
            assert fn(h, 4, _p(q), fl, _p(out)) == E_ARG and b"flags" in err(), fl
    assert L.dspmap_mask_cast_grid(None, 0, 0) == E_ARG
    for age in (-1, -1000):
        assert L.dspmap_mask_cast_grid(h, age, 0) == E_ARG and b"max_age" in err()
    for fl in (1, -1):
        assert L.dspmap_mask_cast_grid(h, 0, fl) == E_ARG and b"flags" in err()
    assert L.dspmap_mask_cast_grid(h, 0, 0) == E_STATE and b"dspmap_build_cast_grid" in err()    # valid arguments: the missing grid decides
    st = (C.c_longlong * 2)()
    assert L.dspmap_known_stats(None, 0, C.cast(st, C.c_void_p)) == E_ARG
    assert L.dspmap_known_stats(h, -1, C.cast(st, C.c_void_p)) == E_ARG and b"max_age" in err()
    assert L.dspmap_known_stats(h, 0, None) == E_ARG and b"NULL" in err()
    assert L.dspmap_get_view(None, None, None, None) == E_ARG
    with pytest.raises(ValueError):
        m.query_known(np.zeros((3, 5), F))
    for call in (lambda: m.integrate_known(-1.0), lambda: m.mask_cast_grid(-1), lambda: m.known_stats(-2)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_known_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    assert L.dspmap_known_integrate(m.h, 5.0, 0) == E_STATE and b"slab" in err()
    assert L.dspmap_known_integrate(m.h, -5.0, 0) == E_ARG                           # the argument checks come first
    ages = np.zeros(m.V, np.int32)
    assert L.dspmap_get_known(m.h, _p(ages)) == E_STATE and b"slab" in err()
    st = (C.c_longlong * 2)()
    assert L.dspmap_known_stats(m.h, 0, C.cast(st, C.c_void_p)) == E_STATE and b"slab" in err()
    q, out = np.zeros((1, 4), F), np.zeros(1, np.int32)
    assert L.dspmap_query_known(m.h, 1, _p(q), 0, _p(out)) == E_STATE and b"slab" in err()
    m.close()


def test_known_valid_calls_need_a_device(dsp):
    """a valid call without a usable device is DSPMAP_E_DEVICE (no CPU fallback)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    ages, st = np.zeros(m.V, np.int32), (C.c_longlong * 2)()
    q, out = np.zeros((4, 4), F), np.zeros(4, np.int32)
    ph = np.zeros((29, 3), F)
    for r in (5.0, float("inf")):
        assert L.dspmap_known_integrate(h, r, 0) == E_DEVICE and b"no HIP device" in err()
    assert L.dspmap_known_reset(h) == E_DEVICE
    assert L.dspmap_get_known(h, _p(ages)) == E_DEVICE
    assert L.dspmap_query_known(h, 4, _p(q), 1, _p(out)) == E_DEVICE and L.dspmap_query_known_device(h, 4, _p(q), 0, _p(out)) == E_DEVICE
    assert L.dspmap_known_stats(h, 3, C.cast(st, C.c_void_p)) == E_DEVICE
    assert L.dspmap_get_view(h, _p(ph), None, None) == E_DEVICE and b"no HIP device" in err()
    for call in (m.integrate_known, m.known_age, m.view, lambda: m.query_known(q), lambda: m.known_stats(0)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_dropin_class_offers_known_space_members(tmp_path):
    """include/dsp_dynamic.h: integrateKnownSpace, getKnownAge, queryKnown and maskCastGridUnknown type-check and forward to the C ABI"""
    src = tmp_path / "known.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    dspmap_query q[2] = {{0.f, 0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, -1.f}};\n"
                   "    std::vector<int> ages(1000);\n    int out[2];\n"
                   "    int a = my_map.integrateKnownSpace() + my_map.integrateKnownSpace(6.5f);\n"
                   "    int b = my_map.getKnownAge(ages.data());\n"
                   "    int c = my_map.queryKnown(2, q, out) + my_map.queryKnown(2, q, out, true);\n"
                   "    int d = my_map.maskCastGridUnknown(3);\n"
                   "    return a + b + c + d + ages[0] + out[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_known_integrate(h_", "dspmap_get_known(h_", "dspmap_query_known(h_", "dspmap_mask_cast_grid(h_"):
        assert call in hdr, call
