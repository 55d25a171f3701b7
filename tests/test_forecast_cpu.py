"""CPU tests of the occupancy forecast at caller-chosen times (dspmap_build_forecast, the accessors, dspmap_query_forecast*): the entry
points are exported and bound, argument errors are DSPMAP_E_ARG with a text before any device is touched, a slab handle and a missing
snapshot are DSPMAP_E_STATE, a valid build needs a device, the drop-in class offers the new members, and the numpy restatement
(tests/forecast_ref.py) that the GPU tests hold the kernels to agrees with a plain per-particle loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import forecast_ref as R

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_build_forecast", "dspmap_forecast_device", "dspmap_forecast_times", "dspmap_get_forecast", "dspmap_query_forecast",
         "dspmap_query_forecast_device")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_forecast_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    cap = dsp.capi
    assert (cap.FORECAST_MAX_TIMES, cap.FORECAST_LERP, cap.QUERY_WORLD) == (64, 2, 1) == (R.MAX_TIMES, R.LERP, 1)
    for meth in ("build_forecast", "forecast", "forecast_times", "forecast_ptr", "query_forecast"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for line in ("#define DSPMAP_FORECAST_MAX_TIMES 64", "#define DSPMAP_FORECAST_LERP 2"):
        assert line in hdr, line
    assert '"dspmap_forecast.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()


def test_forecast_build_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    fn = L.dspmap_build_forecast
    t3 = np.array([0.0, 0.5, 1.0], F)
    t65 = np.arange(65, dtype=F)
    assert fn(None, 3, _p(t3), 0) == E_ARG
    for n in (0, -1, 65, 1 << 20):
        assert fn(h, n, _p(t65), 0) == E_ARG and b"n_times" in err(), n
    assert fn(h, 3, None, 0) == E_ARG and b"NULL" in err()
    for bad in (float("nan"), float("inf"), -float("inf"), -0.5):
        for at in (0, 1, 2):
            t = t3.copy()
            t[at] = bad
            assert fn(h, 3, _p(t), 0) == E_ARG and b"times[" in err(), (bad, at)
    for t in ([0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 1.0, 0.5], [2.0, 1.0, 3.0]):
        assert fn(h, 3, _p(np.array(t, F)), 0) == E_ARG and b"not greater" in err(), t
    for fl in (1, 2, 4, -1):
        assert fn(h, 3, _p(t3), fl) == E_ARG and b"flags" in err(), fl
    with pytest.raises(dsp.capi.DSPMapError):
        m.build_forecast([])
    with pytest.raises(dsp.capi.DSPMapError):
        m.build_forecast([1.0, 0.5])
    m.close()
    # a request that reaches 2^31 cells: 64 layers of a 512 x 512 x 128 map are exactly 2^31 (the handle alone allocates nothing)
    big = dsp.DSPMap(dsp.make_config(nx=512, ny=512, nz=128, res=0.15, z_lo=0, z_hi=64))
    assert fn(big.h, 64, _p(t65), 0) == E_ARG and b"2^31" in L.dspmap_last_error(big.h)
    assert fn(big.h, 63, _p(t65), 0) == E_STATE and b"slab" in L.dspmap_last_error(big.h)   # below the bound: the state decides
    big.close()


def test_forecast_accessor_and_query_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    q, out = np.zeros((4, 4), F), np.zeros(4, F)
    for fn in (L.dspmap_query_forecast, L.dspmap_query_forecast_device):
        assert fn(None, 4, _p(q), 0, 1.0, _p(out)) == E_ARG
        assert fn(h, -1, _p(q), 0, 1.0, _p(out)) == E_ARG and b"negative" in err()
        assert fn(h, 4, None, 0, 1.0, _p(out)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(q), 0, 1.0, None) == E_ARG and b"NULL" in err()
        for fl in (4, 8, 7, -1):
            assert fn(h, 4, _p(q), fl, 1.0, _p(out)) == E_ARG and b"flags" in err(), fl
        assert fn(h, 4, _p(q), 0, float("nan"), _p(out)) == E_ARG and b"outside_value" in err()
        for fl in (0, 1, 2, 3):     # valid argument lists: the missing snapshot decides
            assert fn(h, 4, _p(q), fl, 1.0, _p(out)) == E_STATE and b"dspmap_build_forecast" in err(), fl
        assert fn(h, 0, None, 0, 1.0, None) == E_STATE and b"dspmap_build_forecast" in err()
    lay = np.zeros(m.V, F)
    assert L.dspmap_get_forecast(None, 0, _p(lay)) == E_ARG
    assert L.dspmap_get_forecast(h, 0, None) == E_ARG and b"NULL" in err()
    for layer in (-1, 64):
        assert L.dspmap_get_forecast(h, layer, _p(lay)) == E_ARG and b"layer" in err()
    assert L.dspmap_get_forecast(h, 0, _p(lay)) == E_STATE and b"dspmap_build_forecast" in err()
    t = np.zeros(64, F)
    assert L.dspmap_forecast_times(None, _p(t), 64) == E_ARG
    assert L.dspmap_forecast_times(h, None, 64) == E_ARG and b"NULL" in err()
    assert L.dspmap_forecast_times(h, _p(t), 64) == E_STATE and L.dspmap_forecast_times(h, None, 0) == E_STATE
    assert L.dspmap_forecast_device(h) is None and L.dspmap_forecast_device(None) is None and m.forecast_ptr() is None
    with pytest.raises(ValueError):
        m.query_forecast(np.zeros((3, 5), F))
    for call in (lambda: m.forecast(0), lambda: m.forecast(), m.forecast_times, lambda: m.query_forecast(q)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_forecast_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    t = np.array([0.0, 0.5], F)
    assert L.dspmap_build_forecast(m.h, 2, _p(t), 0) == E_STATE and b"slab" in L.dspmap_last_error(m.h)
    assert L.dspmap_build_forecast(m.h, 2, _p(t), 1) == E_ARG               # the argument checks come first
    m.close()


def test_forecast_valid_build_needs_device(dsp):
    """a valid call without a usable device is DSPMAP_E_DEVICE (no CPU fallback)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    for t in ([0.0], [0.05, 0.1, 2.0], np.arange(64) * 0.05):
        t = np.array(t, F)
        assert L.dspmap_build_forecast(m.h, len(t), _p(t), 0) == E_DEVICE and b"no HIP device" in L.dspmap_last_error(m.h)
    with pytest.raises(dsp.capi.DSPMapError):
        m.build_forecast([0.0, 1.0])
    assert m.forecast_ptr() is None
    m.close()


def test_dropin_class_offers_forecast_members(tmp_path):
    """include/dsp_dynamic.h: buildForecast, getForecast and queryForecast type-check and forward to the C ABI"""
    src = tmp_path / "forecast.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    float times[DSPMAP_FORECAST_MAX_TIMES] = {0.f, 0.05f, 0.1f};\n"
                   "    dspmap_query q[2] = {{0.f, 0.f, 0.f, 0.07f}, {1.f, 0.f, 0.f, -1.f}};\n"
                   "    std::vector<float> v(1000);\n    float out[2];\n"
                   "    int a = my_map.buildForecast(3, times);\n"
                   "    int b = my_map.getForecast(2, v.data());\n"
                   "    int c = my_map.queryForecast(2, q, out) + my_map.queryForecast(2, q, out, true, true, 0.5f);\n"
                   "    return a + b + c + (int)(v[0] + out[0]);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    assert "dspmap_build_forecast(h_" in hdr and "dspmap_get_forecast(h_" in hdr and "dspmap_query_forecast(h_" in hdr
    assert "DSPMAP_FORECAST_LERP" in hdr


# ---- the restatement against a plain per-particle loop
def _hand_made(cfg, n, seed):
    """n particles in random voxels of cfg: positions inside their voxels, a third static, weights with the awkward cases mixed in"""
    rng = np.random.default_rng(seed)
    res, (nx, ny, nz), (hx, hy, hz) = R.dims(cfg)
    ix, iy, iz = rng.integers(0, nx, n), rng.integers(0, ny, n), rng.integers(0, nz, n)
    rec = np.zeros((n, 8), F)
    rec[:, 0] = 1.0
    rec[:, 4] = (ix + rng.uniform(0.05, 0.95, n)) * float(res) - float(hx)
    rec[:, 5] = (iy + rng.uniform(0.05, 0.95, n)) * float(res) - float(hy)
    rec[:, 6] = (iz + rng.uniform(0.05, 0.95, n)) * float(res) - float(hz)
    mv = rng.random(n) > 0.33
    rec[:, 1] = rng.uniform(-1.5, 1.5, n) * mv
    rec[:, 2] = rng.uniform(-1.5, 1.5, n) * mv * (rng.random(n) > 0.2)
    rec[:, 7] = rng.uniform(0.002, 0.5, n)
    rec[:10, 7] = [2.0 ** -25, 3 * 2.0 ** -25, 0.0, -0.25, np.nan, 2.0 ** -24, 1.0, 5 * 2.0 ** -25, 7 * 2.0 ** -25, 1e-3]
    rec[10:16, 1] = [np.nan, np.inf, -np.inf, 0.0, 0.3, 0.0]               # non-finite velocities and positions: a NaN fx or fy is outside the map,
    rec[10:16, 2] = [0.2, 0.0, np.nan, np.nan, 0.0, 0.0]                   # a static particle stays in the voxel it is stored in whatever its position
    rec[14:16, 4] = [np.inf, np.nan]
    return ((iz * ny + iy) * nx + ix).astype(np.int32), rec


def test_forecast_ref_quanta_known_answers():
    w = np.array([2.0 ** -25, 3 * 2.0 ** -25, 0.0, -0.25, np.nan, 5 * 2.0 ** -25, 7 * 2.0 ** -25, 1.0, 2.0 ** -24], F)
    assert R.quanta(w).tolist() == [0, 2, 0, 0, 0, 2, 4, 1 << 24, 1]          # ties to even
    assert R.value(np.array([0, 1, 1 << 24, (1 << 25) + 1])).tolist() == [0.0, 2.0 ** -24, 1.0, 2.0]


def test_forecast_ref_equals_per_particle_loop(dsp):
    cfg = dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12)
    voxel, rec = _hand_made(cfg, 300, 11)
    times = np.array([0.0, 0.05, 0.13, 0.5, 1.0, 2.0, 3.5], F)
    lay, acc, dropped = R.layers(cfg, voxel, rec, times)
    want, dropped_loop = R.layers_loop(cfg, voxel, rec, times)
    assert lay.dtype == F and lay.shape == (7, 16 * 16 * 6) and np.array_equal(lay, want) and dropped == dropped_loop == 0
    q = R.quanta(rec[:, 7])
    static = (rec[:, 1] == 0) & (rec[:, 2] == 0)
    counted = static | np.isfinite(rec[:, [1, 2, 4, 5]]).all(1)               # (a moving particle with a non-finite v or p is outside at every t)
    assert (~counted).sum() == 5 and q[~counted].sum() > 0
    assert acc[0].sum() == q[counted].sum() and acc[-1].sum() < acc[0].sum()  # t = 0 keeps everything else; particles leave the map later
    assert (lay[0] != lay[-1]).sum() > 50
    assert 50 < static.sum() < 250
    only_static, _, _ = R.layers(cfg, voxel[static], rec[static], times)
    assert (only_static == only_static[0]).all() and only_static[0].sum() > 0


def test_forecast_ref_edge_float_is_dropped(dsp):
    """the one float just below half_x whose quotient rounds up to nx: on nx = 16 and 40 at 0.15 m, never on 14, 18, 66 or 132"""
    for nx, hit in ((16, True), (40, True), (14, False), (18, False), (66, False), (132, False)):
        cfg = dsp.make_config(nx=nx, ny=16, nz=6, res=0.15, ppv=12)
        res, _, (hx, hy, hz) = R.dims(cfg)
        edge = np.nextafter(hx, F(0))
        assert (int(F(F(edge + hx) / res)) == nx) == hit, nx
        assert int(F(F(np.nextafter(edge, F(0)) + hx) / res)) == nx - 1
        rec = np.zeros((1, 8), F)
        rec[0] = [1.0, 1.0, 0.0, 0.0, edge, 0.0, 0.0, 0.25]
        voxel = np.array([(3 * 16 + 8) * nx + nx - 1], np.int32)
        lay, acc, dropped = R.layers(cfg, voxel, rec, [0.0, 0.5])
        assert dropped == (1 if hit else 0) and acc[1].sum() == 0 and acc[0].sum() == (0 if hit else 1 << 22)


def test_forecast_ref_query_layer_choice_and_lerp(dsp):
    cfg = dsp.make_config(nx=8, ny=6, nz=5, res=0.5)
    times = np.array([0.1, 0.5, 1.0], F)
    lay = np.zeros((3, 8 * 6 * 5), F)
    g = (2 * 6 + 3) * 8 + 4
    lay[:, g] = [1.0, 2.0, 4.0]
    c = (-2.0 + 0.5 * 4 + 0.25, -1.5 + 0.5 * 3 + 0.25, -1.25 + 0.5 * 2 + 0.25)
    ts = [-1.0, 0.0, 0.1, 0.3, 0.5, 0.75, 1.0, 9.0, np.inf, np.nan]
    q = np.array([c + (t,) for t in ts] + [(9.0, 0.0, 0.0, 0.3), (np.nan, 0.0, 0.0, 0.3)], F)
    assert R.layer_index(times, np.array(ts[:-1], F)).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert R.query(cfg, lay, times, q, outside=0.75).tolist() == [1, 1, 1, 2, 2, 4, 4, 4, 4, 0.75, 0.75, 0.75]
    got = R.query(cfg, lay, times, q, lerp=True, outside=0.75)
    u = F(F(F(0.3) - F(0.1)) / F(F(0.5) - F(0.1)))
    assert got.tolist() == [1, 1, 1, float(F(1) + F(u * F(1))), 2, 3, 4, 4, 4, 0.75, 0.75, 0.75]
    cur = np.array([8.0, -4.0, 2.0], F)
    qw = q.copy()
    qw[:, :3] += cur
    assert np.array_equal(R.query(cfg, lay, times, qw, world=True, lerp=True, cur_pos=cur, outside=0.75), got)
    one = R.query(cfg, lay[:1], times[:1], q, lerp=True, outside=0.75)
    assert one.tolist() == [1] * 9 + [0.75] * 3
