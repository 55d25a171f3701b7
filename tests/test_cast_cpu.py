"""CPU tests of the segment casts (dspmap_build_cast_grid, dspmap_get_cast_grid, dspmap_cast_segments*): the entry points are exported
and bound, argument errors are DSPMAP_E_ARG before any device is touched, a slab handle and a missing grid are DSPMAP_E_STATE, a valid
build needs a device, and known answers of the numpy restatement (tests/cast_ref.py) that the GPU tests hold the kernels to, with its
two routes to the inflation checked against each other."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cast_ref as R

E_ARG, E_DEVICE, E_STATE = -1, -2, -3
NAMES = ("dspmap_build_cast_grid", "dspmap_cast_grid_device", "dspmap_get_cast_grid", "dspmap_cast_segments", "dspmap_cast_segments_device")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_cast_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    cap = dsp.capi
    assert (cap.CAST_FREE, cap.CAST_HIT, cap.CAST_LEFT_MAP, cap.CAST_START_OUTSIDE, cap.CAST_INVALID) == (0, 1, 2, 3, 4)
    assert cap.CAST_MAX_INFLATE == 8
    assert cap.SEGMENT_DTYPE.itemsize == 32 and cap.SEGMENT_DTYPE.names == ("ax", "ay", "az", "ta", "bx", "by", "bz", "tb")
    assert cap.HIT_DTYPE.itemsize == 16 and cap.HIT_DTYPE == R.HIT_DTYPE
    for meth in ("build_cast_grid", "cast_grid", "cast_grid_ptr", "cast_segments"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    assert "#define DSPMAP_CAST_MAX_INFLATE 8" in hdr
    assert "DSPMAP_CAST_FREE = 0, DSPMAP_CAST_HIT = 1, DSPMAP_CAST_LEFT_MAP = 2, DSPMAP_CAST_START_OUTSIDE = 3, DSPMAP_CAST_INVALID = 4" in hdr


def test_cast_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    assert L.dspmap_build_cast_grid(None, 0.5, 0, 0) == E_ARG
    assert L.dspmap_build_cast_grid(h, float("nan"), 0, 0) == E_ARG
    assert b"NaN" in L.dspmap_last_error(h)
    for r in (-1, 9, 1 << 20):
        assert L.dspmap_build_cast_grid(h, 0.5, r, 0) == E_ARG, r
        assert b"inflate_voxels" in L.dspmap_last_error(h)
    for fl in (1, 2, -1):
        assert L.dspmap_build_cast_grid(h, 0.5, 0, fl) == E_ARG, fl
        assert b"flags" in L.dspmap_last_error(h)
    out = np.zeros(20 * 10, np.uint64)
    assert L.dspmap_get_cast_grid(None, 0, _p(out)) == E_ARG
    assert L.dspmap_get_cast_grid(h, 0, None) == E_ARG
    for layer in (-1, 7, 100):       # T = 6: layers 0 .. 6
        assert L.dspmap_get_cast_grid(h, layer, _p(out)) == E_ARG, layer
    assert L.dspmap_cast_grid_device(None) is None
    seg, hit = np.zeros((8, 8), F), np.zeros(8, R.HIT_DTYPE)
    for fn in (L.dspmap_cast_segments, L.dspmap_cast_segments_device):
        assert fn(None, 4, _p(seg), 0, _p(hit)) == E_ARG
        assert fn(h, -1, _p(seg), 0, _p(hit)) == E_ARG
        assert b"negative" in L.dspmap_last_error(h)
        assert fn(h, 4, None, 0, _p(hit)) == E_ARG
        assert b"NULL" in L.dspmap_last_error(h)
        assert fn(h, 4, _p(seg), 0, None) == E_ARG
        for fl in (2, 3, -2):
            assert fn(h, 4, _p(seg), fl, _p(hit)) == E_ARG, fl
            assert b"flags" in L.dspmap_last_error(h)
    m.close()


def test_cast_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    assert L.dspmap_build_cast_grid(m.h, 0.5, 2, 0) == E_STATE
    assert b"slab" in L.dspmap_last_error(m.h)
    assert L.dspmap_build_cast_grid(m.h, float("nan"), 2, 0) == E_ARG     # the argument checks come first
    assert L.dspmap_build_cast_grid(m.h, 0.5, 9, 0) == E_ARG
    assert L.dspmap_build_cast_grid(m.h, 0.5, 2, 1) == E_ARG
    m.close()


def test_cast_before_build_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    out = np.zeros(20 * 10, np.uint64)
    seg, hit = np.zeros((8, 8), F), np.zeros(8, R.HIT_DTYPE)
    assert L.dspmap_get_cast_grid(m.h, 0, _p(out)) == E_STATE
    assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
    for fn in (L.dspmap_cast_segments, L.dspmap_cast_segments_device):
        assert fn(m.h, 8, _p(seg), 0, _p(hit)) == E_STATE
        assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
        assert fn(m.h, 0, None, 1, None) == E_STATE                      # n == 0 is a valid argument list: the state decides
        assert fn(m.h, 8, _p(seg), 2, _p(hit)) == E_ARG                  # ... and the argument checks come first
    assert L.dspmap_cast_grid_device(m.h) is None and m.cast_grid_ptr() is None
    with pytest.raises(dsp.capi.DSPMapError):
        m.cast_grid(0)
    with pytest.raises(dsp.capi.DSPMapError):
        m.cast_segments(seg)
    with pytest.raises(ValueError):
        m.cast_segments(np.zeros((8, 4), F))
    m.close()


def test_cast_valid_build_needs_device(dsp):
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    want = 1 if torch.cuda.is_available() else E_DEVICE   # (no CPU fallback: without a device every valid call fails)
    assert L.dspmap_build_cast_grid(m.h, 0.5, 8, 0) == want
    if want == E_DEVICE:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError):
            m.build_cast_grid(0.5)
        assert m.cast_grid_ptr() is None
    m.close()


def test_dropin_class_offers_casts(dsp, tmp_path):
    """include/dsp_dynamic.h: buildCastGrid / castSegments type-check and forward to the C ABI"""
    src = tmp_path / "cast.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n    dspmap_segment s[2] = {};\n    dspmap_cast_hit h[2];\n'
                   "    static_assert(sizeof(dspmap_segment) == 32 && sizeof(dspmap_cast_hit) == 16, \"layout\");\n"
                   "    int a = my_map.buildCastGrid();\n    int b = my_map.buildCastGrid(0.5f, DSPMAP_CAST_MAX_INFLATE);\n"
                   "    int c = my_map.castSegments(2, s, h);\n    int e = my_map.castSegments(2, s, h, true);\n"
                   "    return a + b + c + e + (h[0].status == DSPMAP_CAST_HIT ? h[0].voxel + h[0].layer + (int)h[0].s : 0);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for fn in ("dspmap_build_cast_grid(h_", "dspmap_cast_segments(h_"):
        assert fn in hdr, fn


# ---- known answers of the restatement on a hand-built 4 x 4 x 4 grid at 0.5 m with T = 2 (half = 1 m: cell i spans [-1 + i / 2, -0.5 + i / 2),
# centres -0.75, -0.25, 0.25, 0.75; horizon 0 holds t in [0, 0.1], horizon 1 everything later)
@pytest.fixture(scope="module")
def cfg(dsp):
    return dsp.make_config(nx=4, ny=4, nz=4, res=0.5, pred_times=(0.1, 0.5))


def _lay(*cells):
    """bool [3, 4, 4, 4] with the given (layer, x, y, z) set"""
    o = np.zeros((3, 4, 4, 4), bool)
    for l, x, y, z in cells:
        o[l, z, y, x] = True
    return o


def _g(x, y, z):
    return (z * 4 + y) * 4 + x


def _one(cfg, lay, a, b, ta=-1.0, tb=-1.0, **kw):
    r = R.cast(cfg, lay, np.array([[a[0], a[1], a[2], ta, b[0], b[1], b[2], tb]], F), **kw)[0]
    return (r["s"], int(r["voxel"]), int(r["layer"]), int(r["status"]))


def test_cast_ref_axis_aligned_hit_and_occupied_start(cfg):
    lay = _lay((0, 3, 1, 1))
    # u runs 0.5 -> 4.5 along x (d = 4): faces at s = 0.125, 0.375, 0.625; b lies outside the map
    assert _one(cfg, lay, (-0.75, -0.25, -0.25), (1.25, -0.25, -0.25)) == (F(0.625), _g(3, 1, 1), 0, R.HIT)
    # u runs 0.5 -> 3.5 (d = 3): every operation rounded on its own
    s3 = F(F(F(0.5) / F(3)) + F(F(1) / F(3)))
    s3 = F(s3 + F(F(1) / F(3)))
    assert _one(cfg, lay, (-0.75, -0.25, -0.25), (0.75, -0.25, -0.25)) == (s3, _g(3, 1, 1), 0, R.HIT)
    # the same walk backwards from inside the occupied cell: s = 0, whatever follows
    assert _one(cfg, lay, (0.75, -0.25, -0.25), (-0.75, -0.25, -0.25)) == (F(0), _g(3, 1, 1), 0, R.HIT)
    assert _one(cfg, lay, (0.75, -0.25, -0.25), (0.75, -0.25, -0.25)) == (F(0), _g(3, 1, 1), 0, R.HIT)
    # one row beside it: free all the way, ending inside a free cell
    assert _one(cfg, lay, (-0.75, 0.25, -0.25), (0.75, 0.25, -0.25)) == (F(1), -1, -1, R.FREE)
    assert _one(cfg, lay, (-0.75, -0.25, -0.25), (0.25, -0.25, -0.25)) == (F(1), -1, -1, R.FREE)      # stops one cell short


def test_cast_ref_diagonal_ties_go_x_then_y_then_z(cfg):
    a, b = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)       # corner (1, 1, 1) -> corner (3, 3, 3): all three tMax are 0.5, then 1.0
    # visited: (1,1,1) s 0 | (2,1,1) (2,2,1) (2,2,2) s 0.5 | (3,2,2) (3,3,2) (3,3,3) s 1
    for cell, s in (((1, 1, 1), 0.0), ((2, 1, 1), 0.5), ((2, 2, 1), 0.5), ((2, 2, 2), 0.5), ((3, 2, 2), 1.0), ((3, 3, 2), 1.0), ((3, 3, 3), 1.0)):
        assert _one(cfg, _lay((0,) + cell), a, b) == (F(s), _g(*cell), 0, R.HIT), cell
    for cell in ((1, 2, 1), (1, 1, 2), (1, 2, 2), (2, 1, 2), (3, 1, 1), (2, 3, 3), (3, 2, 3)):      # the other orders' cells are never entered
        assert _one(cfg, _lay((0,) + cell), a, b) == (F(1), -1, -1, R.FREE), cell
    assert _one(cfg, _lay((0, 2, 2, 1), (0, 2, 1, 1)), a, b)[1] == _g(2, 1, 1)                      # the first of two
    # backwards the same rule: x first
    assert _one(cfg, _lay((0, 1, 2, 2)), (0.25, 0.25, 0.25), (-0.75, -0.75, -0.75)) == (F(0.25), _g(1, 2, 2), 0, R.HIT)


def test_cast_ref_leaves_through_each_face(cfg):
    lay = _lay()
    a = (0.25, -0.25, 0.25)                          # cell (2, 1, 2)
    for axis, sign, last in ((0, 1, (3, 1, 2)), (0, -1, (0, 1, 2)), (1, 1, (2, 3, 2)), (1, -1, (2, 0, 2)), (2, 1, (2, 1, 3)), (2, -1, (2, 1, 0))):
        b = list(a)
        b[axis] += sign * 5.0
        s, voxel, layer, status = _one(cfg, lay, a, b)
        assert (voxel, layer, status) == (_g(*last), -1, R.LEFT_MAP), (axis, sign)
        want = (1.0 - a[axis]) / 5.0 if sign > 0 else (a[axis] + 1.0) / 5.0      # where the face at +-1 m is crossed
        assert abs(float(s) - want) < 1e-6
    # an occupied cell on the way wins over the face
    assert _one(cfg, _lay((0, 3, 1, 2)), a, (5.25, -0.25, 0.25))[3] == R.HIT
    # a == b tests the start cell only
    assert _one(cfg, _lay((0, 3, 1, 2)), a, a) == (F(1), -1, -1, R.FREE)


def test_cast_ref_start_outside_and_invalid(cfg):
    lay = _lay((0, 0, 0, 0), (0, 3, 3, 3))
    out = (F(0), -1, -1, R.START_OUTSIDE)
    for a in ((1.5, 0, 0), (0, -1.5, 0), (0, 0, 7.0), (1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, 0, -1.0), (3e38, 0, 0)):   # +-half itself is outside (:1576)
        assert _one(cfg, lay, a, (0.0, 0.0, 0.0)) == out, a
    # the last float below half is inside for dspmap_point_voxel_index, but fl(p + half) rounds up to 2 * half: trunc(u) == n
    assert _one(cfg, lay, (np.nextafter(F(1), F(0)), 0, 0), (0.0, 0.0, 0.0)) == out
    assert _one(cfg, lay, (0.9999, 0, 0), (0.0, 0.0, 0.0))[3] == R.FREE
    bad = (F(0), -1, -1, R.INVALID)
    for v in (np.nan, np.inf, -np.inf):
        for j in range(3):
            a, b = [0.1, 0.1, 0.1], [0.3, 0.3, 0.3]
            a[j] = v
            assert _one(cfg, lay, a, b) == bad and _one(cfg, lay, b, a) == bad, (v, j)
    assert _one(cfg, lay, (0.1, 0.1, 0.1), (0.3, 0.3, 0.3), ta=np.nan) == bad
    assert _one(cfg, lay, (0.1, 0.1, 0.1), (0.3, 0.3, 0.3), ta=0.0, tb=np.nan) == bad
    assert _one(cfg, lay, (0.1, 0.1, 0.1), (0.3, 0.3, 0.3), ta=0.0, tb=np.inf)[3] == R.FREE       # an infinite time is a time
    assert _one(cfg, lay, (1.5, 0, 0), (np.nan, 0, 0)) == bad                                    # validity comes first


def test_cast_ref_world_frame_equals_map_frame(cfg):
    rng = np.random.default_rng(5)
    lay = np.zeros((3, 4, 4, 4), bool)
    lay[:, rng.integers(0, 4, 12), rng.integers(0, 4, 12), rng.integers(0, 4, 12)] = True
    seg = rng.uniform(-1.2, 1.2, (400, 8)).astype(F)
    seg[:, 3], seg[:, 7] = rng.uniform(-0.1, 0.6, 400), rng.uniform(-0.1, 0.6, 400)
    cur = np.array([8.0, -4.0, 2.0], F)              # shifts that keep every coordinate exact in fp32 at these magnitudes ...
    seg[:, [0, 1, 2, 4, 5, 6]] = np.round(seg[:, [0, 1, 2, 4, 5, 6]] * 1024) / 1024   # ... for coordinates on a 2^-10 lattice
    shifted = seg.copy()
    shifted[:, 0:3] += cur
    shifted[:, 4:7] += cur
    want = R.cast(cfg, lay, seg)
    got = R.cast(cfg, lay, shifted, world=True, cur_pos=cur)
    assert want.tobytes() == got.tobytes()
    assert set(want["status"]) == {R.FREE, R.HIT, R.LEFT_MAP, R.START_OUTSIDE}
    assert R.cast(cfg, lay, shifted, world=False).tobytes() != want.tobytes()


def test_cast_ref_space_time(cfg):
    a, b = (-0.75, -0.25, -0.25), (0.75, -0.25, -0.25)       # u 0.5 -> 3.5: cell 2 is entered at s ~ 0.5 and left at s ~ 0.83
    s1 = F(F(0.5) / F(3))
    s2 = F(s1 + F(F(1) / F(3)))
    lay = _lay((2, 2, 1, 1))                                 # free in layer 1 (horizon 0), occupied in layer 2 (horizon 1)
    # ta < 0 reads layer 0 whatever tb is
    for tb in (-1.0, 0.0, 0.3, 5.0, np.inf):
        assert _one(cfg, lay, a, b, ta=-0.5, tb=tb) == (F(1), -1, -1, R.FREE), tb
        assert _one(cfg, _lay((0, 2, 1, 1)), a, b, ta=-0.5, tb=tb) == (s2, _g(2, 1, 1), 0, R.HIT), tb
    # entry at t ~ 0.08 (horizon 0), exit at t ~ 0.133 (horizon 1): both layers are tested, the second one holds the voxel
    assert _one(cfg, lay, a, b, ta=0.0, tb=0.16) == (s2, _g(2, 1, 1), 2, R.HIT)
    # the whole segment at one time inside horizon 0: layer 1 only
    assert _one(cfg, lay, a, b, ta=0.05, tb=0.05) == (F(1), -1, -1, R.FREE)
    assert _one(cfg, lay, a, b, ta=0.3, tb=0.3) == (s2, _g(2, 1, 1), 2, R.HIT)
    # layer 0 is not tested at t >= 0
    assert _one(cfg, _lay((0, 2, 1, 1)), a, b, ta=0.0, tb=0.16) == (F(1), -1, -1, R.FREE)
    # both layers set: the lower one is reported (ascending order)
    assert _one(cfg, _lay((1, 2, 1, 1), (2, 2, 1, 1)), a, b, ta=0.0, tb=0.16) == (s2, _g(2, 1, 1), 1, R.HIT)
    # reversed times test the same set: cell 1 is entered at t ~ 0.133 (horizon 1) and left at t = 0.08 (horizon 0)
    assert _one(cfg, _lay((2, 1, 1, 1)), a, b, ta=0.16, tb=0.0) == (s1, _g(1, 1, 1), 2, R.HIT)
    assert _one(cfg, _lay((1, 1, 1, 1)), a, b, ta=0.16, tb=0.0) == (s1, _g(1, 1, 1), 1, R.HIT)
    assert _one(cfg, _lay((1, 1, 1, 1), (2, 1, 1, 1)), a, b, ta=0.16, tb=0.0) == (s1, _g(1, 1, 1), 1, R.HIT)
    assert _one(cfg, _lay((2, 2, 1, 1)), a, b, ta=0.16, tb=0.0) == (F(1), -1, -1, R.FREE)            # cell 2 lies in horizon 0 then
    # a time spanning every horizon passes layer by layer
    assert _one(cfg, _lay((2, 3, 1, 1)), a, b, ta=0.0, tb=0.4)[2] == 2


def test_cast_ref_t0_reads_layer_0(dsp):
    flat = dsp.make_config(nx=4, ny=4, nz=1, res=0.5, pred_times=())
    lay = np.zeros((1, 1, 4, 4), bool)
    lay[0, 0, 1, 3] = True
    r = R.cast(flat, lay, np.array([[-0.75, -0.25, 0.0, 3.0, 1.25, -0.25, 0.0, 9.0]], F))[0]
    assert (r["s"], r["voxel"], r["layer"], r["status"]) == (F(0.625), 7, 0, R.HIT)


def test_cast_ref_inflation_known_answers():
    o = np.zeros((4, 4, 4), bool)
    o[1, 2, 0] = True                                # (x 0, y 2, z 1): the cube is clipped at the x = 0 face
    got = R.inflate(o, 1)
    want = np.zeros_like(o)
    want[0:3, 1:4, 0:2] = True
    assert np.array_equal(got, want) and got.sum() == 18
    o[:] = False
    o[2, 1, 2] = True
    assert R.inflate(o, 1).sum() == 27 and np.array_equal(R.inflate(o, 0), o)
    assert R.inflate(o, 8).all() and R.inflate(o, 2).all()      # r = 8 on a 4 x 4 x 4 grid: everything iff anything
    assert not R.inflate(np.zeros((4, 4, 4), bool), 8).any()
    lay = np.zeros((3, 4, 4, 4), bool)               # layers do not leak into each other
    lay[1, 0, 0, 0] = True
    inf = R.inflate(lay, 8)
    assert inf[1].all() and not inf[0].any() and not inf[2].any()


def test_cast_ref_pack_layout():
    lay = np.zeros((2, 3, 70), bool)
    lay[0, 0, 0] = lay[0, 1, 63] = lay[1, 2, 64] = lay[1, 0, 69] = True
    w = R.pack(lay)
    assert w.shape == (2, 3, 2) and w.dtype == np.uint64
    assert w[0, 0, 0] == 1 and w[0, 1, 0] == 1 << 63 and w[1, 2, 1] == 1 and w[1, 0, 1] == 1 << 5
    assert w.sum() == 1 + (1 << 63) + 1 + 32
    assert (R.pack(np.ones((5, 70), bool))[:, 1] == (1 << 6) - 1).all()      # bits at x >= nx are 0


def test_cast_ref_inflation_brute_force_equals_shifted_or():
    rng = np.random.default_rng(2025)
    n_cases = 0
    for case in range(24):
        shape = tuple(int(v) for v in rng.integers(1, 13, 3))
        if case < 4:
            shape = [(9, 13, 1), (1, 1, 70), (12, 1, 7), (1, 5, 12)][case]      # nx = 1; one 70-wide row (two words); flat ones
        density = [0.0, 0.004, 0.03, 0.2, 0.9, 1.0][case % 6]
        occ = rng.random(shape) < density
        if case % 6 == 1:
            occ.flat[rng.integers(0, occ.size)] = True
        for r in (0, 1, 2, 3, 8):
            a, b = R.inflate_brute(occ, r), R.inflate(occ, r)
            assert np.array_equal(a, b), (case, shape, r)
            assert (b | ~occ).all() and b.any() == occ.any()
            if r >= max(shape) - 1:
                assert b.all() == occ.any()
            words = R.pack(b)
            assert words.shape == shape[:2] + ((shape[2] + 63) // 64,)
            back = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(shape[:2] + (-1,))
            assert np.array_equal(back[..., :shape[2]], b) and not back[..., shape[2]:].any()
        n_cases += 1
    assert n_cases >= 20
