"""CPU tests of the free boxes grown in the cast grid (dspmap_grow_boxes*): the entry points are exported and bound, argument errors are
DSPMAP_E_ARG before any device is touched, a slab handle and a missing grid are DSPMAP_E_STATE, a valid call needs a device, the drop-in
class offers growBoxes, box_bounds' arithmetic, and known answers of the numpy restatement (tests/corridor_ref.py) that the GPU tests hold
the kernel to -- with its three algorithm-blind checkers run over random grids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import corridor_ref as R

E_ARG, E_DEVICE, E_STATE = -1, -2, -3
NAMES = ("dspmap_grow_boxes", "dspmap_grow_boxes_device")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, O, LIM = R.EDGE, R.OBSTACLE, R.LIMIT


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _g(*v):
    return (C.c_int * 3)(*v)


def test_corridor_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    cap = dsp.capi
    assert (cap.BOX_OK, cap.BOX_SEED_BLOCKED, cap.BOX_SEED_OUTSIDE, cap.BOX_INVALID) == (0, 1, 3, 4) == (R.OK, R.SEED_BLOCKED, R.SEED_OUTSIDE, R.INVALID)
    assert (cap.BOX_STOP_OBSTACLE, cap.BOX_STOP_EDGE, cap.BOX_STOP_LIMIT) == (1, 2, 3) == (R.OBSTACLE, R.EDGE, R.LIMIT)
    assert cap.BOX_MAX_GROW == 64 == R.MAX_GROW and cap.BOX_WITH_CURRENT == 2 and cap.QUERY_WORLD == 1
    assert cap.BOX_DTYPE.itemsize == 32 and cap.BOX_DTYPE == R.BOX_DTYPE and cap.BOX_DTYPE.names == ("lo", "hi", "status", "stop")
    for meth in ("grow_boxes", "box_bounds"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    assert "#define DSPMAP_BOX_MAX_GROW 64" in hdr and "#define DSPMAP_BOX_WITH_CURRENT 2" in hdr
    assert "DSPMAP_BOX_OK = 0, DSPMAP_BOX_SEED_BLOCKED = 1, DSPMAP_BOX_SEED_OUTSIDE = 3, DSPMAP_BOX_INVALID = 4" in hdr
    assert "DSPMAP_BOX_STOP_OBSTACLE = 1, DSPMAP_BOX_STOP_EDGE = 2, DSPMAP_BOX_STOP_LIMIT = 3" in hdr
    assert '"dspmap_corridor.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()


def test_corridor_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    seed, box = np.zeros((8, 8), F), np.zeros(8, R.BOX_DTYPE)
    for fn in (L.dspmap_grow_boxes, L.dspmap_grow_boxes_device):
        assert fn(None, 4, _p(seed), _g(1, 1, 1), 0, _p(box)) == E_ARG
        assert fn(h, -1, _p(seed), _g(1, 1, 1), 0, _p(box)) == E_ARG
        assert b"negative" in L.dspmap_last_error(h)
        assert fn(h, 4, None, _g(1, 1, 1), 0, _p(box)) == E_ARG
        assert b"NULL" in L.dspmap_last_error(h)
        assert fn(h, 4, _p(seed), _g(1, 1, 1), 0, None) == E_ARG
        assert b"NULL" in L.dspmap_last_error(h)
        assert fn(h, 4, _p(seed), None, 0, _p(box)) == E_ARG
        assert b"max_grow" in L.dspmap_last_error(h)
        assert fn(h, 0, None, None, 0, None) == E_ARG                       # max_grow is needed whatever n is
        for bad in ((-1, 0, 0), (0, 65, 0), (0, 0, 1 << 20), (64, 64, -64)):
            assert fn(h, 4, _p(seed), _g(*bad), 0, _p(box)) == E_ARG, bad
            assert b"max_grow" in L.dspmap_last_error(h)
        for fl in (4, 7, 8, -1, -4):
            assert fn(h, 4, _p(seed), _g(1, 1, 1), fl, _p(box)) == E_ARG, fl
            assert b"flags" in L.dspmap_last_error(h)
    with pytest.raises(ValueError):
        m.grow_boxes(np.zeros((8, 4), F), (1, 1, 1))
    with pytest.raises(dsp.capi.DSPMapError):
        m.grow_boxes(seed, (1, 1, 65))
    m.close()


def test_corridor_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    seed, box = np.zeros((8, 8), F), np.zeros(8, R.BOX_DTYPE)
    for fn in (L.dspmap_grow_boxes, L.dspmap_grow_boxes_device):
        assert fn(m.h, 8, _p(seed), _g(1, 1, 1), 0, _p(box)) == E_STATE
        assert b"slab" in L.dspmap_last_error(m.h)
        assert fn(m.h, 8, _p(seed), _g(1, 1, 65), 0, _p(box)) == E_ARG       # the argument checks come first
        assert fn(m.h, 8, _p(seed), _g(1, 1, 1), 4, _p(box)) == E_ARG
    m.close()


def test_corridor_before_build_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    seed, box = np.zeros((8, 8), F), np.zeros(8, R.BOX_DTYPE)
    for fn in (L.dspmap_grow_boxes, L.dspmap_grow_boxes_device):
        for fl in (0, 1, 2, 3):
            assert fn(m.h, 8, _p(seed), _g(8, 8, 4), fl, _p(box)) == E_STATE
            assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
        assert fn(m.h, 0, None, _g(0, 0, 0), 0, None) == E_STATE               # n == 0 is a valid argument list: the state decides
        assert fn(m.h, 8, _p(seed), _g(8, 8, 4), 4, _p(box)) == E_ARG          # ... and the argument checks come first
    with pytest.raises(dsp.capi.DSPMapError):
        m.grow_boxes(seed, (8, 8, 4))
    m.close()


def test_corridor_valid_call_needs_device(dsp):
    """a valid call is a grid and a batch: without a device the grid's build is DSPMAP_E_DEVICE and the batch finds no grid (no CPU fallback)"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    seed, box = np.zeros((8, 8), F), np.zeros(8, R.BOX_DTYPE)
    have = torch.cuda.is_available()
    assert L.dspmap_build_cast_grid(m.h, 0.5, 0, 0) == (0 if have else E_DEVICE)
    if not have:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
    rc = L.dspmap_grow_boxes(m.h, 8, _p(seed), _g(1, 1, 1), 0, _p(box))
    assert rc == (0 if have else E_STATE)
    if have:
        assert (box["status"] == R.OK).all()      # an empty map: (0, 0, 0) lies in a free cell
    else:
        assert (box["status"] == 0).all() and (box["hi"] == 0).all()      # nothing was written
        with pytest.raises(dsp.capi.DSPMapError):
            m.grow_boxes(seed, (1, 1, 1))
    m.close()


def test_dropin_class_offers_grow_boxes(dsp, tmp_path):
    """include/dsp_dynamic.h: growBoxes type-checks and forwards to the C ABI"""
    src = tmp_path / "corridor.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n    dspmap_segment s[2] = {};\n    dspmap_box b[2];\n'
                   "    static_assert(sizeof(dspmap_box) == 32 && sizeof(dspmap_segment) == 32, \"layout\");\n"
                   "    const int grow[3] = {8, 8, DSPMAP_BOX_MAX_GROW};\n"
                   "    int a = my_map.buildCastGrid(0.2f, 2);\n    int c = my_map.growBoxes(2, s, grow, b);\n"
                   "    int e = my_map.growBoxes(2, s, grow, b, true, true);\n"
                   "    unsigned cause = (b[0].stop >> 2) & 3u;\n"
                   "    return a + c + e + (b[0].status == DSPMAP_BOX_OK && cause == DSPMAP_BOX_STOP_OBSTACLE ? b[0].lo[0] + b[0].hi[2] : 0);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    assert "dspmap_grow_boxes(h_" in hdr and "DSPMAP_BOX_WITH_CURRENT" in hdr


def test_box_bounds_known_answers(dsp):
    m = dsp.DSPMap(dsp.make_config(nx=8, ny=6, nz=5, res=0.5))                # half = (2, 1.5, 1.25)
    b = np.zeros(3, dsp.capi.BOX_DTYPE)
    b["lo"], b["hi"] = [(1, 2, 0), (0, 0, 0), (-1, -1, -1)], [(6, 2, 2), (7, 5, 4), (-1, -1, -1)]
    b["status"] = [R.OK, R.SEED_BLOCKED, R.SEED_OUTSIDE]
    lo, hi = m.box_bounds(b)
    assert lo.dtype == hi.dtype == F and lo.shape == hi.shape == (3, 3)
    assert lo[0].tolist() == [-1.5, -0.5, -1.25] and hi[0].tolist() == [1.5, 0.0, 0.25]
    assert lo[1].tolist() == [-2.0, -1.5, -1.25] and hi[1].tolist() == [2.0, 1.5, 1.25]      # the whole map: -half .. +half
    assert np.isnan(lo[2]).all() and np.isnan(hi[2]).all()
    lo2, hi2 = m.box_bounds({"lo": b["lo"], "hi": b["hi"]})                    # the dict form of the device call
    assert np.array_equal(lo, lo2, equal_nan=True) and np.array_equal(hi, hi2, equal_nan=True)
    m.close()
    m = dsp.DSPMap(dsp.make_config(nx=66, ny=66, nz=40, res=0.15))             # every operation rounded to fp32 on its own
    b = np.zeros(1, dsp.capi.BOX_DTYPE)
    b["lo"], b["hi"] = [(7, 31, 3)], [(41, 33, 39)]
    lo, hi = m.box_bounds(b)
    res = F(0.15)
    half = [F(F(res * F(n)) * F(0.5)) for n in (66, 66, 40)]
    for a in range(3):
        assert lo[0, a] == F(F(F(b["lo"][0, a]) * res) + (-half[a])) and hi[0, a] == F(F(F(b["hi"][0, a] + 1) * res) + (-half[a]))
    assert hi[0, 2] == half[2] and (hi > lo).all()
    m.close()


# ---- known answers of the restatement on a hand-built 8 x 6 x 5 grid at 0.5 m with T = 3 (half = (2, 1.5, 1.25); cell i of an axis has its
# centre at -half + 0.5 i + 0.25; horizon 0 holds t in [0, 0.1], horizon 1 (0.1, 0.5], horizon 2 everything later)
N = (8, 6, 5)


@pytest.fixture(scope="module")
def cfg(dsp):
    return dsp.make_config(nx=8, ny=6, nz=5, res=0.5, pred_times=(0.1, 0.5, 1.0))


def _lay(*cells, L=4):
    """bool [L, 5, 6, 8] with the given (layer, x, y, z) set"""
    o = np.zeros((L, 5, 6, 8), bool)
    for l, x, y, z in cells:
        o[l, z, y, x] = True
    return o


def _c(x, y, z):
    return (-2.0 + 0.5 * x + 0.25, -1.5 + 0.5 * y + 0.25, -1.25 + 0.5 * z + 0.25)


def _pt(v):
    """a tuple of three ints is a cell (its centre is meant), anything else a point"""
    return _c(*v) if all(isinstance(k, int) for k in v) else v


def _one(cfg, lay, a, b, grow, ta=-1.0, tb=-1.0, **kw):
    """(lo, hi, status, (cause of face 0 .. 5)) of the seed from the centre of cell a to the centre of cell b"""
    pa, pb = _pt(a), _pt(b)
    r = R.grow(cfg, lay, np.array([[pa[0], pa[1], pa[2], ta, pb[0], pb[1], pb[2], tb]], F), grow, **kw)[0]
    return tuple(r["lo"].tolist()), tuple(r["hi"].tolist()), int(r["status"]), tuple((int(r["stop"]) >> (2 * f)) & 3 for f in range(6))


NONE6 = (0,) * 6


def test_corridor_ref_free_map_gives_the_whole_map(cfg):
    assert _one(cfg, _lay(), (3, 2, 1), (3, 2, 1), (64, 64, 64)) == ((0, 0, 0), (7, 5, 4), R.OK, (E,) * 6)
    assert _one(cfg, _lay(), (0, 0, 0), (7, 5, 4), (0, 0, 0)) == ((0, 0, 0), (7, 5, 4), R.OK, (E,) * 6)      # the seed box is the map: edge before limit
    assert _one(cfg, _lay(), (6, 1, 4), (2, 4, 0), (7, 7, 7)) == ((0, 0, 0), (7, 5, 4), R.OK, (E,) * 6)


def test_corridor_ref_limit_gives_exact_extents(cfg):
    assert _one(cfg, _lay(), (3, 2, 2), (4, 2, 2), (2, 0, 1)) == ((1, 2, 1), (6, 2, 3), R.OK, (LIM,) * 6)
    assert _one(cfg, _lay(), (4, 2, 2), (3, 2, 2), (2, 0, 1)) == ((1, 2, 1), (6, 2, 3), R.OK, (LIM,) * 6)    # the seed's direction does not matter
    assert _one(cfg, _lay(), (3, 2, 2), (3, 2, 2), (0, 0, 0)) == ((3, 2, 2), (3, 2, 2), R.OK, (LIM,) * 6)
    # the limit is measured from the SEED box on each side, and the edge wins where both apply
    assert _one(cfg, _lay(), (1, 2, 2), (5, 2, 2), (1, 1, 1)) == ((0, 1, 1), (6, 3, 3), R.OK, (E, LIM, LIM, LIM, LIM, LIM))
    assert _one(cfg, _lay(), (1, 2, 2), (5, 2, 2), (2, 3, 1)) == ((0, 0, 1), (7, 5, 3), R.OK, (E, E, E, E, LIM, LIM))


def test_corridor_ref_obstacle_and_round_robin_order(cfg):
    # one blocked voxel next to the seed on +x: that face stops at once, the others run to the edges
    assert _one(cfg, _lay((0, 4, 2, 2)), (3, 2, 2), (3, 2, 2), (64, 64, 64)) == ((0, 0, 0), (3, 5, 4), R.OK, (E, O, E, E, E, E))
    # a blocked voxel diagonally off the seed, at (+1, +1): +x (face 1) is visited before +y (face 3), takes the column x = 4 while the box
    # is still one row high, and the voxel then lies in +y's slab
    lay = _lay((0, 4, 3, 2))
    assert _one(cfg, lay, (3, 2, 2), (3, 2, 2), (64, 64, 64)) == ((0, 0, 0), (7, 2, 4), R.OK, (E, E, E, O, E, E))
    # visited y first the same seed gives the other box: the order is part of the definition
    assert _one(cfg, lay, (3, 2, 2), (3, 2, 2), (64, 64, 64), order=(2, 3, 0, 1, 4, 5)) == ((0, 0, 0), (3, 5, 4), R.OK, (E, O, E, E, E, E))
    # extensions made earlier in the same round count: -x (face 0) widens the box to x = 2 before +y looks at its slab
    assert _one(cfg, _lay((0, 2, 3, 2)), (3, 2, 2), (3, 2, 2), (1, 1, 0)) == ((2, 1, 2), (4, 2, 2), R.OK, (LIM, LIM, LIM, O, LIM, LIM))
    # an obstacle met in a later round: two free columns, then the voxel
    assert _one(cfg, _lay((0, 6, 2, 2)), (3, 2, 2), (3, 2, 2), (64, 0, 0)) == ((0, 2, 2), (5, 2, 2), R.OK, (E, O, LIM, LIM, LIM, LIM))
    # ... which the limit reaches first if it is smaller
    assert _one(cfg, _lay((0, 6, 2, 2)), (3, 2, 2), (3, 2, 2), (2, 0, 0)) == ((1, 2, 2), (5, 2, 2), R.OK, (LIM, LIM, LIM, LIM, LIM, LIM))


def test_corridor_ref_blocked_outside_and_invalid_seeds(cfg):
    lay = _lay((0, 4, 2, 2))
    # blocked: the seed box itself is reported, nothing is grown -- also when only a cell BETWEEN the end points' cells is set
    assert _one(cfg, lay, (4, 2, 2), (4, 2, 2), (8, 8, 4)) == ((4, 2, 2), (4, 2, 2), R.SEED_BLOCKED, NONE6)
    assert _one(cfg, lay, (5, 1, 2), (3, 3, 2), (8, 8, 4)) == ((3, 1, 2), (5, 3, 2), R.SEED_BLOCKED, NONE6)
    assert _one(cfg, lay, (5, 1, 3), (3, 3, 3), (8, 8, 4))[2] == R.OK
    none = ((-1, -1, -1), (-1, -1, -1), R.SEED_OUTSIDE, NONE6)
    inside = _c(3, 2, 2)
    for p in ((2.5, 0, 0), (0, -1.6, 0), (0, 0, 7.0), (2.0, 0, 0), (-2.0, 0, 0), (0, 1.5, 0), (0, 0, -1.25), (3e38, 0, 0)):   # +-half itself is outside
        assert _one(cfg, lay, p, inside, (8, 8, 4)) == none, p
        assert _one(cfg, lay, inside, p, (8, 8, 4)) == none, p                 # BOTH end points must be inside
    # the last float below half is inside for dspmap_point_voxel_index, but fl(p + half) rounds up to 2 * half: trunc(u) == n
    assert _one(cfg, lay, inside, (np.nextafter(F(2), F(0)), 0.0, 0.0), (8, 8, 4)) == none
    assert _one(cfg, lay, inside, (1.9999, 0.0, 0.0), (8, 8, 4))[2] == R.SEED_BLOCKED      # (x 3 .. 7 holds the voxel)
    bad = ((-1, -1, -1), (-1, -1, -1), R.INVALID, NONE6)
    for v in (np.nan, np.inf, -np.inf):
        for j in range(3):
            p = list(inside)
            p[j] = v
            assert _one(cfg, lay, p, inside, (8, 8, 4)) == bad and _one(cfg, lay, inside, p, (8, 8, 4)) == bad, (v, j)
    assert _one(cfg, lay, inside, inside, (8, 8, 4), ta=np.nan) == bad
    assert _one(cfg, lay, inside, inside, (8, 8, 4), ta=0.0, tb=np.nan) == bad
    assert _one(cfg, lay, inside, inside, (8, 8, 4), ta=0.0, tb=np.inf)[2] == R.OK          # an infinite time is a time
    assert _one(cfg, lay, (2.5, 0, 0), (np.nan, 0, 0), (8, 8, 4)) == bad                    # validity comes first


def test_corridor_ref_time_rules(cfg, dsp):
    cell = (3, 2, 2)
    grow = (1, 1, 1)

    def status(lay, ta, tb, **kw):
        return _one(cfg, lay, cell, cell, grow, ta=ta, tb=tb, **kw)[2]

    # a voxel set only in horizon 1 (layer 2) blocks a seed whose k(ta) .. k(tb) contains 1, and no other; k: 0.05 -> 0, 0.3 -> 1, 0.8 -> 2
    lay = _lay((2,) + cell)
    want = {(0.05, 0.05): R.OK, (0.3, 0.3): R.SEED_BLOCKED, (0.8, 0.8): R.OK, (0.05, 0.3): R.SEED_BLOCKED, (0.3, 0.8): R.SEED_BLOCKED,
            (0.05, 0.8): R.SEED_BLOCKED,                                       # between the two ends' horizons
            (0.8, 0.05): R.SEED_BLOCKED, (0.3, 0.05): R.SEED_BLOCKED, (0.8, 0.3): R.SEED_BLOCKED,   # tb < ta tests the same set
            (0.1, 0.1): R.OK, (0.5, 0.5): R.SEED_BLOCKED, (0.0, 0.0): R.OK, (5.0, 9.0): R.OK, (0.6, np.inf): R.OK,
            (0.05, -1.0): R.OK,                                                # a negative tb selects layer 0: layers 0 .. 1
            (0.3, -1.0): R.SEED_BLOCKED}                                       # ... layers 0 .. 2
    for (ta, tb), st in want.items():
        assert status(lay, ta, tb) == st, (ta, tb)
    # ta < 0 reads layer 0 whatever tb is
    for tb in (-1.0, 0.0, 0.3, 5.0, np.inf):
        assert status(lay, -0.5, tb) == R.OK, tb
        assert status(_lay((0,) + cell), -0.5, tb) == R.SEED_BLOCKED, tb
    # layer 0 is not tested at t >= 0 -- unless WITH_CURRENT adds it
    cur = _lay((0,) + cell)
    for ta, tb in ((0.05, 0.05), (0.3, 0.8), (0.8, 0.05)):
        assert status(cur, ta, tb) == R.OK and status(cur, ta, tb, with_current=True) == R.SEED_BLOCKED
        assert status(lay, ta, tb, with_current=True) == want[(ta, tb)]        # ... and adds nothing else
    assert status(cur, -1.0, -1.0, with_current=True) == R.SEED_BLOCKED
    # the tested layers also decide the growth: the voxel of horizon 1 beside the seed stops +x only for the seeds that test it
    beside = _lay((2, 4, 2, 2))
    assert _one(cfg, beside, cell, cell, grow, ta=0.05, tb=0.05) == ((2, 1, 1), (4, 3, 3), R.OK, (LIM,) * 6)
    assert _one(cfg, beside, cell, cell, grow, ta=0.05, tb=0.8) == ((2, 1, 1), (3, 3, 3), R.OK, (LIM, O, LIM, LIM, LIM, LIM))
    # T == 0 reads layer 0 for every time
    flat = dsp.make_config(nx=8, ny=6, nz=5, res=0.5, pred_times=())
    for ta, tb in ((-1.0, -1.0), (0.0, 0.0), (3.0, 9.0), (9.0, -3.0)):
        for wc in (False, True):
            assert _one(flat, _lay((0,) + cell, L=1), cell, cell, grow, ta=ta, tb=tb, with_current=wc)[2] == R.SEED_BLOCKED
            assert _one(flat, _lay(L=1), cell, cell, grow, ta=ta, tb=tb, with_current=wc) == ((2, 1, 1), (4, 3, 3), R.OK, (LIM,) * 6)


def _random_case(cfg, density, n, seed):
    rng = np.random.default_rng(seed)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    T = cfg.prediction_times
    lay = rng.random((T + 1, cfg.nz, cfg.ny, cfg.nx)) < density
    res = F(cfg.voxel_resolution)
    half = (nn.astype(F) * res * F(0.5)).astype(F)
    a = (rng.uniform(-1.05, 1.05, (n, 3)) * half).astype(F)
    b = (a + rng.uniform(-3, 3, (n, 3)) * res).astype(F)
    lat = rng.random(n) < 0.2                                                  # on voxel faces: multiples of res
    a[lat] = (np.round(a[lat] / res) * res).astype(F)
    seg = np.empty((n, 8), F)
    seg[:, 0:3], seg[:, 4:7] = a, b
    seg[:, 3], seg[:, 7] = rng.uniform(-0.3, 1.3, n), rng.uniform(-0.3, 1.3, n)
    bad = rng.random((n, 8)) < 0.003
    seg[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), bad.sum())
    return lay, seg


def test_corridor_ref_world_frame_equals_map_frame(cfg):
    lay, seg = _random_case(cfg, 0.05, 600, 5)
    cur = np.array([8.0, -4.0, 2.0], F)              # shifts that keep every coordinate exact in fp32 at these magnitudes ...
    seg[:, [0, 1, 2, 4, 5, 6]] = np.round(seg[:, [0, 1, 2, 4, 5, 6]] * 1024) / 1024   # ... for coordinates on a 2^-10 lattice
    shifted = seg.copy()
    shifted[:, 0:3] += cur
    shifted[:, 4:7] += cur
    want = R.grow(cfg, lay, seg, (2, 2, 1))
    got = R.grow(cfg, lay, shifted, (2, 2, 1), world=True, cur_pos=cur)
    assert want.tobytes() == got.tobytes()
    assert set(want["status"].tolist()) == {R.OK, R.SEED_BLOCKED, R.SEED_OUTSIDE, R.INVALID}
    assert R.grow(cfg, lay, shifted, (2, 2, 1), world=False).tobytes() != want.tobytes()


@pytest.mark.parametrize("density", [0.01, 0.1, 0.4])
def test_corridor_ref_passes_the_independent_checkers(dsp, density):
    big = dsp.make_config(nx=21, ny=17, nz=9, res=0.2, pred_times=(0.1, 0.5, 1.0))
    lay, seg = _random_case(big, density, 2000, int(density * 100))
    seen_all = {R.OBSTACLE: 0, R.EDGE: 0, R.LIMIT: 0}
    n_ok = 0
    for grow, wc in (((5, 5, 3), False), ((64, 64, 64), True), ((0, 1, 0), False)):
        boxes = R.grow(big, lay, seg, grow, with_current=wc)
        assert R.check_contains_seed(big, seg, boxes) > 1000
        n_ok += R.check_free(big, lay, seg, boxes, with_current=wc)
        for k, v in R.check_causes(big, lay, seg, boxes, grow, with_current=wc).items():
            seen_all[k] += v
        assert set(boxes["status"].tolist()) >= {R.SEED_BLOCKED, R.SEED_OUTSIDE, R.INVALID}
    assert n_ok >= (300 if density < 0.2 else 1) and all(v > 0 for v in seen_all.values()), (n_ok, seen_all)
