"""CPU tests of the viewpoint scores (dspmap_score_views and the calls next to it): the central direction of every pyramid lies in its own
pyramid, the numpy restatement (tests/view_ref.py) that the GPU tests hold the kernel to gives the answers worked by hand on a
16 x 16 x 6 map -- an empty grid, a full wall, everything known, nothing known, the precedence of the statuses --, the entry points are
exported and bound, every argument error is DSPMAP_E_ARG with a text before any device is touched, a valid call needs a device, and the
drop-in class offers the new members."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cast_ref as CR
from tests import known_ref as K
from tests import view_ref as V

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_score_views", "dspmap_score_views_device", "dspmap_view_rays", "dspmap_debug_view_cells")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2 = float(np.sqrt(0.5))
QUATS = ((1.0, 0.0, 0.0, 0.0), (S2, 0.0, 0.0, S2), (0.9799247, 0.0868241, 0.1736482, 0.0))
INF = float("inf")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _view(pos, quat=QUATS[0], max_range=INF, t=-1.0):
    return np.array(tuple(pos) + tuple(quat) + (max_range, t), F)


# ---- the rays
@pytest.mark.parametrize("kw", [dict(), dict(angle=1, neighbor_n=2)], ids=["3deg_28x16", "1deg_84x48_5x5"])
def test_central_direction_lies_in_its_own_pyramid(dsp, kw):
    cfg = dsp.make_config(**kw)
    nh, nv = K.pyramid_counts(cfg)
    d0 = V.directions0(cfg)
    assert d0.shape == (nh * nv, 3) and d0.dtype == F and np.allclose(np.linalg.norm(d0.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (d0[:, 0] > 0.5).all()
    # the table is symmetric: pyramid (h, v) mirrors (nh - 1 - h, nv - 1 - v), and the first pyramid looks up and to the -y side
    g = d0.reshape(nh, nv, 3)
    assert np.array_equal(g[::-1, ::-1, 1:], -g[:, :, 1:]) and g[0, 0, 1] < 0 < g[0, 0, 2]
    for quat in QUATS:
        ph, pv = K.plane_normals(cfg, quat)
        d = V.directions(cfg, quat)
        b = K.pyramid_of(ph, pv, d[:, 0], d[:, 1], d[:, 2])
        assert np.array_equal(b, np.arange(nh * nv)), (kw, quat, np.flatnonzero(b != np.arange(nh * nv))[:5])
        far = (d * F(7.3)).astype(F)                                   # ... and so does every point of the ray
        assert np.array_equal(K.pyramid_of(ph, pv, far[:, 0], far[:, 1], far[:, 2]), np.arange(nh * nv))


# ---- answers worked by hand
def _small(dsp):
    cfg = dsp.make_config(nx=16, ny=16, nz=6, res=0.15)
    lay = np.zeros((cfg.prediction_times + 1, 6, 16, 16), bool)
    return cfg, lay


POS = (-0.5, 0.02, 0.01)


def _wedge(cfg, pos, quat=QUATS[0]):
    """the cells of the wedge and their distances, without the restatement's score()"""
    ph, pv = K.plane_normals(cfg, quat)
    cx, cy, cz = V.centres(cfg)
    z, y, x = np.meshgrid((cz - F(pos[2])).astype(F), (cy - F(pos[1])).astype(F), (cx - F(pos[0])).astype(F), indexing="ij")
    b = K.pyramid_of(ph, pv, x, y, z)
    return b, np.sqrt(x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2 + z.astype(np.float64) ** 2)


def test_empty_grid_sees_the_whole_wedge(dsp):
    cfg, lay = _small(dsp)
    cx = V.centres(cfg)[0]
    assert cx[0] == F(-1.125) and abs(float(cx[12]) - 0.675) < 1e-6       # -half + res / 2 = -1.2 + 0.075
    ages = np.full((6, 16, 16), -1, np.int32)
    b, dist = _wedge(cfg, POS)
    n_wedge = int((b >= 0).sum())
    assert 200 < n_wedge < 16 * 16 * 6 - 200
    s = V.score(cfg, lay, ages, _view(POS)[None], 0, V.host_rays(cfg))
    assert s.dtype == V.SCORE_DTYPE and s.tolist() == [(n_wedge, n_wedge, 0, V.OK)]   # nothing known: every seen cell is unknown
    ages[:] = 0
    assert V.score(cfg, lay, ages, _view(POS)[None], 0, V.host_rays(cfg)).tolist() == [(n_wedge, 0, 0, V.OK)]   # everything known
    ages[:] = 3
    assert V.score(cfg, lay, ages, _view(POS)[None], 2, V.host_rays(cfg))["n_unknown"][0] == n_wedge            # ... but too long ago
    assert V.score(cfg, lay, ages, _view(POS)[None], 3, V.host_rays(cfg))["n_unknown"][0] == 0
    # a range: exactly the wedge cells within it (no centre lies within 1e-4 of 0.9 m of this position: checked, not assumed)
    assert not ((b >= 0) & (np.abs(dist - 0.9) < 1e-4)).any()
    s9 = V.score(cfg, lay, ages, _view(POS, max_range=0.9)[None], 3, V.host_rays(cfg))
    assert s9["n_seen"][0] == int(((b >= 0) & (dist <= 0.9)).sum()) and 20 < s9["n_seen"][0] < n_wedge - 20
    # world frame: the same view seen from a map whose sensor stands at cur
    cur = np.array([3.0, -2.0, 0.5], F)
    vw = _view(POS)
    vw[:3] = (vw[:3] + cur).astype(F)
    back = (vw[:3] - cur).astype(F)
    sw = V.score(cfg, lay, ages, vw[None], 3, V.host_rays(cfg), world=True, cur_pos=cur)
    assert sw.tolist() == V.score(cfg, lay, ages, _view(back)[None], 3, V.host_rays(cfg)).tolist() and sw["n_seen"][0] > 200


def test_full_wall_hides_what_lies_behind_it(dsp):
    cfg, lay = _small(dsp)
    lay[:, :, :, 12] = True                                               # the plane x = 12 in every layer
    ages = np.full((6, 16, 16), -1, np.int32)
    ages[:, :, :8] = 0                                                    # the near half is known
    rays = V.host_rays(cfg)
    view = _view(POS)
    s, info = V.score(cfg, lay, ages, view[None], 0, rays, details=True)
    d = info[0]
    # the rays, cast here once more: n_returns is the number of hits, and a hit's return is the distance to the centre of its voxel
    dirs = rays(QUATS[0])[2]
    reach = F(F(0.15) * F(16 + 16 + 6))
    seg = np.zeros((len(dirs), 8), F)
    seg[:, 0:3], seg[:, 4:7], seg[:, 3], seg[:, 7] = np.array(POS, F), (np.array(POS, F) + (dirs * reach).astype(F)).astype(F), -1, -1
    hits = CR.cast(cfg, lay, seg)
    hit = hits["status"] == CR.HIT
    assert s["n_returns"][0] == hit.sum() and 30 < hit.sum() < len(dirs) and set(hits["status"].tolist()) == {CR.HIT, CR.LEFT_MAP}
    assert (hits["voxel"][hit] % 16 == 12).all()                          # every hit is a cell of the wall
    assert np.array_equal(d["ml"] > 0, hit) and (d["ml"][~hit] == -1).all()
    ahead = 14 * 16 + 7                                                   # 1.5 degrees to +y and up: wall cell (12, 8, 3)
    assert abs(float(dirs[ahead, 1]) - np.tan(np.radians(1.5)) * float(dirs[ahead, 0])) < 1e-6 and dirs[ahead, 2] > 0
    assert hits["voxel"][ahead] == (3 * 16 + 8) * 16 + 12
    assert abs(float(d["ml"][ahead]) - np.sqrt((0.675 + 0.5) ** 2 + (0.075 - 0.02) ** 2 + (0.075 - 0.01) ** 2)) < 1e-6
    # no cell farther than its pyramid's return plus the margin is seen; cells in front of the wall are
    b, dist = _wedge(cfg, POS)
    mlb = d["ml"][np.maximum(b, 0)].astype(np.float64)
    behind = (b >= 0) & (mlb > 0) & (dist > mlb + 0.3 + 1e-5)
    assert behind.sum() >= 20 and not d["seen"][behind].any() and d["occluded"][behind].all()
    front = (b >= 0) & (np.arange(16)[None, None, :] < 12)
    assert front.sum() > 100 and d["seen"][front].all()
    assert d["seen"][3, 8, 12] and d["seen"][3, 8, 13] and not d["seen"][3, 8, 15]   # the wall itself, 0.15 m behind it (inside the margin), 0.45 m
    assert s["n_seen"][0] == d["seen"].sum() == (b >= 0).sum() - d["occluded"].sum() and not d["beyond"].any()
    assert s["n_unknown"][0] == (d["seen"] & (ages < 0)).sum() and 0 < s["n_unknown"][0] < s["n_seen"][0]
    # the wall only in layer 1 + k(0.1) = 2: t = 0.1 sees it, t = -1 and t = 1.2 do not; t = +inf reads the last layer
    lay[:] = False
    lay[2, :, :, 12] = True
    lay[cfg.prediction_times, :, :, 14] = True
    for t, want in ((-1.0, 0), (0.1, int(hit.sum())), (0.2, int(hit.sum())), (1.2, 0)):
        assert V.score(cfg, lay, ages, _view(POS, t=t)[None], 0, rays)["n_returns"][0] == want, t
    assert V.layer_of(cfg, 0.1) == 2 and V.layer_of(cfg, INF) == cfg.prediction_times and V.layer_of(cfg, -INF) == 0
    s_inf = V.score(cfg, lay, ages, _view(POS, t=INF)[None], 0, rays)
    assert s_inf["status"][0] == V.OK and s_inf["n_returns"][0] > 30


def test_status_precedence(dsp):
    """INVALID over OUTSIDE over BLOCKED"""
    cfg, lay = _small(dsp)
    lay[:] = True                                                         # every cell is blocked in every layer
    ages = np.zeros((6, 16, 16), np.int32)
    nan = float("nan")
    views = np.stack([
        _view(POS),                                                       # blocked
        _view((5.0, 0.0, 0.0)),                                           # outside (and nothing to be blocked in)
        _view((1.2, 0.0, 0.0)),                                           # on the upper face: outside
        _view((-1.2, 0.0, 0.0)),                                          # on the lower face: outside
        _view((5.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 0.0)),                # outside AND a zero quaternion: invalid
        _view(POS, quat=(nan, 0.0, 0.0, 0.0)), _view(POS, quat=(1.0, INF, 0.0, 0.0)),
        _view((nan, 0.0, 0.0)), _view((0.0, -INF, 0.0)),
        _view(POS, max_range=0.0), _view(POS, max_range=-1.0), _view(POS, max_range=nan), _view(POS, t=nan),
        _view(POS, quat=(1e-30, 0.0, 0.0, 0.0)),                          # the squared norm underflows to zero
    ])
    s = V.score(cfg, lay, ages, views, 0, V.host_rays(cfg))
    assert s["status"].tolist() == [V.BLOCKED] + [V.OUTSIDE] * 3 + [V.INVALID] * 10
    assert not s["n_seen"].any() and not s["n_unknown"].any() and not s["n_returns"].any()
    lay[:] = False
    s = V.score(cfg, lay, ages, views[:2], 0, V.host_rays(cfg))
    assert s["status"].tolist() == [V.OK, V.OUTSIDE] and s["n_seen"][0] > 0
    assert (V.OK, V.BLOCKED, V.OUTSIDE, V.INVALID) == (dsp.capi.VIEW_OK, dsp.capi.VIEW_BLOCKED, dsp.capi.VIEW_OUTSIDE, dsp.capi.VIEW_INVALID)
    assert V.SCORE_DTYPE == dsp.capi.VIEW_SCORE_DTYPE and dsp.capi.VIEW_DTYPE.itemsize == 36 and dsp.capi.VIEW_SCORE_DTYPE.itemsize == 16


# ---- the library without a device
def test_view_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert "int %s(dspmap_t* m" % n in hdr, n
    for meth in ("score_views", "view_rays", "view_cells"):
        assert callable(getattr(dsp.DSPMap, meth))
    assert "DSPMAP_VIEW_OK = 0, DSPMAP_VIEW_BLOCKED = 1, DSPMAP_VIEW_OUTSIDE = 3, DSPMAP_VIEW_INVALID = 4" in hdr
    assert '"dspmap_view.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()
    blob = open(dsp.capi.LIB_PATH, "rb").read()
    assert b"k_view_score" in blob and b"k_view_rays" in blob
    # the cast walk is ONE device function in a shared header: k_cast holds no copy of the loop
    cast = open(os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_cast.hip")).read()
    view = open(os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_view.hip")).read()
    assert "cast_walk(" in cast and "cast_walk(" in view and "__fadd_rn(tm, tdx)" not in cast + view


def test_view_argument_errors_without_a_device(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    views, out = np.zeros((4, 9), F), np.zeros(4, dsp.capi.VIEW_SCORE_DTYPE)
    for fn in (L.dspmap_score_views, L.dspmap_score_views_device):
        assert fn(None, 4, _p(views), 0, 0, _p(out)) == E_ARG
        assert fn(h, -1, _p(views), 0, 0, _p(out)) == E_ARG and b"negative" in err()
        assert fn(h, 4, None, 0, 0, _p(out)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(views), 0, 0, None) == E_ARG and b"NULL" in err()
        for age in (-1, -1000):
            assert fn(h, 4, _p(views), age, 0, _p(out)) == E_ARG and b"max_age" in err()
        for fl in (2, 4, 3, -1):
            assert fn(h, 4, _p(views), 0, fl, _p(out)) == E_ARG and b"flags" in err(), fl
        for n, fl in ((4, 0), (4, 1), (0, 0)):                            # valid arguments: the missing grid decides, also for n = 0
            assert fn(h, n, _p(views), 3, fl, _p(out)) == E_STATE and b"dspmap_build_cast_grid" in err()
    quat, ph = np.array([1, 0, 0, 0], F), np.zeros((29, 3), F)
    assert L.dspmap_view_rays(None, _p(quat), _p(ph), None, None) == E_ARG
    assert L.dspmap_view_rays(h, None, _p(ph), None, None) == E_ARG and b"NULL quaternion" in err()
    words = np.zeros((10, 20, 1), np.uint64)
    assert L.dspmap_debug_view_cells(None, _p(views), 0, _p(words), None) == E_ARG
    assert L.dspmap_debug_view_cells(h, None, 0, _p(words), None) == E_ARG and b"NULL" in err()
    assert L.dspmap_debug_view_cells(h, _p(views), 0, None, None) == E_ARG and b"NULL" in err()
    assert L.dspmap_debug_view_cells(h, _p(views), 2, _p(words), None) == E_ARG and b"flags" in err()
    assert L.dspmap_debug_view_cells(h, _p(views), 1, _p(words), None) == E_STATE and b"dspmap_build_cast_grid" in err()
    assert not out.view(np.int32).any() and not words.any()               # nothing was written
    for bad in (np.zeros((3, 8), F), np.zeros(9, F)[:8]):
        with pytest.raises(ValueError):
            m.score_views(bad, 0)
    with pytest.raises(ValueError):
        m.view_rays((1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        m.view_cells(np.zeros((2, 9), F))
    for call in (lambda: m.score_views(views, -1), lambda: m.score_views(views, 0), lambda: m.view_cells(views[0])):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_view_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    views, out = np.zeros((2, 9), F), np.zeros(2, dsp.capi.VIEW_SCORE_DTYPE)
    for fn in (L.dspmap_score_views, L.dspmap_score_views_device):
        assert fn(m.h, 2, _p(views), 0, 0, _p(out)) == E_STATE and b"slab" in err()
        assert fn(m.h, 2, _p(views), -1, 0, _p(out)) == E_ARG                # the argument checks come first
    quat = np.array([1, 0, 0, 0], F)
    assert L.dspmap_view_rays(m.h, _p(quat), None, None, None) == E_STATE and b"slab" in err()
    m.close()


def test_view_valid_calls_need_a_device(dsp):
    """a valid call without a usable device is DSPMAP_E_DEVICE (no CPU fallback); the scoring calls need a grid, which needs one too"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    quat, ph, pv, dirs = np.array([1, 0, 0, 0], F), np.zeros((29, 3), F), np.zeros((17, 3), F), np.zeros((448, 3), F)
    assert L.dspmap_view_rays(m.h, _p(quat), _p(ph), _p(pv), _p(dirs)) == E_DEVICE and b"no HIP device" in err()
    assert L.dspmap_view_rays(m.h, _p(quat), None, None, None) == E_DEVICE
    assert L.dspmap_build_cast_grid(m.h, 0.1, 0, 0) == E_DEVICE
    with pytest.raises(dsp.capi.DSPMapError, match="no HIP device"):
        m.view_rays(quat)
    m.close()


def test_dropin_class_offers_view_members(tmp_path):
    """include/dsp_dynamic.h: scoreViews and viewRays type-check and forward to the C ABI"""
    src = tmp_path / "view.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    dspmap_view v[2] = {{0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 3.f, -1.f}, {1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, INFINITY, 0.5f}};\n"
                   "    dspmap_view_score s[2];\n    const float q[4] = {1.f, 0.f, 0.f, 0.f};\n"
                   "    std::vector<float> ph(29 * 3), pv(17 * 3), dirs(448 * 3);\n"
                   "    int a = my_map.scoreViews(2, v, 30, s) + my_map.scoreViews(2, v, 0, s, true);\n"
                   "    int b = my_map.viewRays(q, ph.data(), pv.data(), dirs.data()) + my_map.viewRays(q, nullptr, nullptr, nullptr);\n"
                   "    static_assert(sizeof(dspmap_view) == 36 && sizeof(dspmap_view_score) == 16, \"layout\");\n"
                   "    return a + b + s[0].n_seen + s[0].n_unknown + s[1].n_returns + (s[1].status == DSPMAP_VIEW_OK);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_score_views(h_", "dspmap_view_rays(h_"):
        assert call in hdr, call
