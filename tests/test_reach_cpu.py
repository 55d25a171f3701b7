"""CPU tests of the arrival-time fields grown through the cast grid (dspmap_build_reach_fields*, dspmap_reach_paths*, the accessors and the
dspmap_debug_set_cast_grid hook): the entry points are exported and bound, argument errors are DSPMAP_E_ARG with a text before any device
is touched, a slab handle and a missing grid / snapshot are DSPMAP_E_STATE, a valid build needs a device, the drop-in class offers the new
members, and known answers of the numpy restatement (tests/reach_ref.py) that the GPU tests hold the kernels to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import reach_ref as R

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_build_reach_fields", "dspmap_build_reach_fields_device", "dspmap_reach_fields_device", "dspmap_get_reach_field",
         "dspmap_reach_paths", "dspmap_reach_paths_device", "dspmap_debug_reach_storage", "dspmap_debug_set_cast_grid")
F = np.float32
U = R.UNREACHED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_reach_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    cap = dsp.capi
    assert (cap.REACH_MAX_FIELDS, cap.REACH_MAX_STEPS, cap.REACH_UNREACHED) == (64, 4096, 65535) == (R.MAX_FIELDS, R.MAX_STEPS, R.UNREACHED)
    assert (cap.QUERY_WORLD, cap.REACH_WITH_CURRENT, cap.REACH_DEVICE_SETS) == (1, 2, 4)
    assert cap.REACH_POINT_DTYPE.itemsize == 16 and cap.REACH_POINT_DTYPE == R.POINT_DTYPE
    for meth in ("build_reach_fields", "reach_field", "reach_fields_ptr", "reach_paths", "set_cast_grid", "reach_storage"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for line in ("#define DSPMAP_REACH_MAX_FIELDS 64", "#define DSPMAP_REACH_MAX_STEPS 4096", "#define DSPMAP_REACH_UNREACHED 65535",
                 "#define DSPMAP_REACH_WITH_CURRENT 2", "#define DSPMAP_REACH_DEVICE_SETS 4"):
        assert line in hdr, line
    assert '"dspmap_reach.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()


def _build_fns(L):
    return (L.dspmap_build_reach_fields, L.dspmap_build_reach_fields_device)


def test_reach_build_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    src = np.zeros(4, R.POINT_DTYPE)
    for fn in _build_fns(L):
        assert fn(None, 1, 4, _p(src), 0.0, 0.1, 16, 0) == E_ARG
        for nf in (0, -1, 65, 1 << 20):
            assert fn(h, nf, 4, _p(src), 0.0, 0.1, 16, 0) == E_ARG and b"n_fields" in err(), nf
        assert fn(h, 1, -1, _p(src), 0.0, 0.1, 16, 0) == E_ARG and b"negative" in err()
        assert fn(h, 1, 4, None, 0.0, 0.1, 16, 0) == E_ARG and b"NULL" in err()
        assert fn(h, 1, 4, _p(src), float("nan"), 0.1, 16, 0) == E_ARG and b"t_start" in err()
        for dt in (float("nan"), -0.1, float("inf"), -float("inf")):
            assert fn(h, 1, 4, _p(src), 0.0, dt, 16, 0) == E_ARG and b"step_seconds" in err(), dt
        for ms in (0, -1, 4097, 1 << 20):
            assert fn(h, 1, 4, _p(src), 0.0, 0.1, ms, 0) == E_ARG and b"max_steps" in err(), ms
        for fl in (8, 16, 15, -1, -8):
            assert fn(h, 1, 4, _p(src), 0.0, 0.1, 16, fl) == E_ARG and b"flags" in err(), fl
        # valid argument lists reach the state check: infinite and negative start times, a zero step, no sources, every flag
        for args in ((1, 4, _p(src), float("inf"), 0.0, 1, 0), (64, 0, None, -float("inf"), 0.0, 4096, 7), (3, 4, _p(src), -1.0, 2.5, 7, 4)):
            assert fn(h, *args) == E_STATE and b"dspmap_build_cast_grid" in err(), args
    m.close()
    # a request whose buffers exceed 2^31 cells: 64 fields of a 512 x 512 x 160 map (the handle alone allocates nothing)
    big = dsp.DSPMap(dsp.make_config(nx=512, ny=512, nz=160, res=0.15))
    for fn in _build_fns(L):
        assert fn(big.h, 64, 0, None, 0.0, 0.1, 16, 0) == E_ARG and b"2^31" in L.dspmap_last_error(big.h)
        assert fn(big.h, 51, 0, None, 0.0, 0.1, 16, 0) == E_STATE         # 51 * V = 2^31 - 2^25: the state decides
    big.close()


def test_reach_paths_and_accessor_argument_errors(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    st, steps, cells = np.zeros(4, R.POINT_DTYPE), np.zeros(4, np.int32), np.zeros((4, 8), np.int32)
    for fn in (L.dspmap_reach_paths, L.dspmap_reach_paths_device):
        assert fn(None, 4, _p(st), 8, 0, _p(steps), _p(cells)) == E_ARG
        assert fn(h, -1, _p(st), 8, 0, _p(steps), _p(cells)) == E_ARG and b"negative" in err()
        for ml in (-1, 4098, 1 << 20):
            assert fn(h, 4, _p(st), ml, 0, _p(steps), _p(cells)) == E_ARG and b"max_len" in err(), ml
        assert fn(h, 4, None, 8, 0, _p(steps), _p(cells)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(st), 8, 0, None, _p(cells)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(st), 8, 0, _p(steps), None) == E_ARG and b"cells_out" in err()
        for fl in (2, 4, 3, -1):
            assert fn(h, 4, _p(st), 8, fl, _p(steps), _p(cells)) == E_ARG and b"flags" in err(), fl
        assert fn(h, 1 << 20, _p(st), 4097, 0, _p(steps), _p(cells)) == E_ARG and b"2^31" in err()
        # valid argument lists: the missing snapshot decides (cells_out may be NULL when max_len is 0; max_len 4097 is the longest path)
        for args in ((4, _p(st), 0, 0, _p(steps), None), (4, _p(st), 4097, 1, _p(steps), _p(cells)), (0, None, 8, 0, None, None)):
            assert fn(h, *args) == E_STATE and b"dspmap_build_reach_fields" in err(), args
    out = np.zeros(m.V, np.uint16)
    assert L.dspmap_get_reach_field(None, 0, _p(out)) == E_ARG
    assert L.dspmap_get_reach_field(h, 0, None) == E_ARG and b"NULL" in err()
    for f in (-1, 64):
        assert L.dspmap_get_reach_field(h, f, _p(out)) == E_ARG and b"field" in err()
    assert L.dspmap_get_reach_field(h, 0, _p(out)) == E_STATE and b"dspmap_build_reach_fields" in err()
    assert not out.any()
    assert L.dspmap_reach_fields_device(h) is None and L.dspmap_reach_fields_device(None) is None and m.reach_fields_ptr() is None
    two = (C.c_longlong * 2)(7, 7)
    assert L.dspmap_debug_reach_storage(None, two) == E_ARG and L.dspmap_debug_reach_storage(h, None) == E_ARG
    assert L.dspmap_debug_reach_storage(h, two) == OK and tuple(two) == (0, 0) == m.reach_storage()      # nothing was ever built
    # the hook: NULL and a bit at x >= nx are argument errors, a missing grid a state error
    words = np.zeros((m.T + 1, 10, 20, 1), np.uint64)
    assert L.dspmap_debug_set_cast_grid(None, _p(words)) == E_ARG
    assert L.dspmap_debug_set_cast_grid(h, None) == E_ARG and b"NULL" in err()
    bad = words.copy()
    bad[m.T, 9, 19, 0] = np.uint64(1) << np.uint64(20)
    assert L.dspmap_debug_set_cast_grid(h, _p(bad)) == E_ARG and b"x >= nx" in err()
    bad[m.T, 9, 19, 0] = np.uint64(1) << np.uint64(19)
    assert L.dspmap_debug_set_cast_grid(h, _p(bad)) == E_STATE and b"dspmap_build_cast_grid" in err()
    with pytest.raises(ValueError):
        m.set_cast_grid(words[1:])
    with pytest.raises(ValueError):
        m.build_reach_fields(np.zeros((3, 5), F))
    with pytest.raises(ValueError):
        m.reach_field()
    with pytest.raises(dsp.capi.DSPMapError):
        m.build_reach_fields(np.zeros((3, 4), F), n_fields=65)
    with pytest.raises(dsp.capi.DSPMapError):
        m.reach_paths(st, 8)
    m.close()


def test_reach_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    src, steps, cells = np.zeros(4, R.POINT_DTYPE), np.zeros(4, np.int32), np.zeros((4, 8), np.int32)
    for fn in _build_fns(L):
        assert fn(m.h, 1, 4, _p(src), 0.0, 0.1, 16, 0) == E_STATE and b"slab" in L.dspmap_last_error(m.h)
        assert fn(m.h, 1, 4, _p(src), 0.0, 0.1, 0, 0) == E_ARG               # the argument checks come first
    for fn in (L.dspmap_reach_paths, L.dspmap_reach_paths_device):
        assert fn(m.h, 4, _p(src), 8, 0, _p(steps), _p(cells)) == E_STATE and b"slab" in L.dspmap_last_error(m.h)
        assert fn(m.h, 4, _p(src), 8, 2, _p(steps), _p(cells)) == E_ARG
    out = np.zeros(20 * 20 * 10, np.uint16)
    assert L.dspmap_get_reach_field(m.h, 0, _p(out)) == E_STATE and b"slab" in L.dspmap_last_error(m.h)
    words = np.zeros((m.T + 1, 10, 20, 1), np.uint64)
    assert L.dspmap_debug_set_cast_grid(m.h, _p(words)) == E_STATE and b"slab" in L.dspmap_last_error(m.h)
    m.close()


def test_reach_valid_build_needs_device(dsp):
    """a valid call is a grid and a build: without a device the grid's build is DSPMAP_E_DEVICE and the fields find no grid (no CPU fallback)"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    have = torch.cuda.is_available()
    assert L.dspmap_build_cast_grid(m.h, 0.5, 0, 0) == (OK if have else E_DEVICE)
    if not have:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
    src = R.points([(0.0, 0.0, 0.0, 0)])
    rc = L.dspmap_build_reach_fields(m.h, 1, 1, _p(src), -1.0, 0.0, 5, 0)
    assert rc == (OK if have else E_STATE)
    if have:
        val = m.reach_field(0)
        assert val[5, 10, 10] == 0 and (val != U).sum() == (R.fields(m.cfg, np.zeros((m.T + 1, 10, 20, 20), bool), src, 1, max_steps=5) != U).sum()
    else:
        assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError):
            m.build_reach_fields(src)
        with pytest.raises(dsp.capi.DSPMapError):
            m.reach_field(0)
        assert m.reach_fields_ptr() is None
    m.close()


def test_dropin_class_offers_reach_members(dsp, tmp_path):
    """include/dsp_dynamic.h: buildReachFields, getReachField and reachPaths type-check and forward to the C ABI"""
    src = tmp_path / "reach.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n    dspmap_reach_point s[2] = {{0.f, 0.f, 0.f, 0}, {1.f, 0.f, 0.f, 1}};\n'
                   "    static_assert(sizeof(dspmap_reach_point) == 16, \"layout\");\n"
                   "    std::vector<unsigned short> v(1000);\n    int steps[2], cells[2 * (DSPMAP_REACH_MAX_STEPS + 1)];\n"
                   "    int a = my_map.buildCastGrid(0.2f, 2);\n"
                   "    int b = my_map.buildReachFields(2, 2, s, -1.f, 0.f, DSPMAP_REACH_MAX_STEPS);\n"
                   "    int c = my_map.buildReachFields(DSPMAP_REACH_MAX_FIELDS, 2, s, 0.f, 0.1f, 64, true, true);\n"
                   "    int d = my_map.getReachField(1, v.data());\n"
                   "    int e = my_map.reachPaths(2, s, DSPMAP_REACH_MAX_STEPS + 1, steps, cells) + my_map.reachPaths(2, s, 0, steps, nullptr, true);\n"
                   "    return a + b + c + d + e + (v[0] == DSPMAP_REACH_UNREACHED ? steps[0] + cells[0] : 0);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    assert "dspmap_build_reach_fields(h_" in hdr and "dspmap_get_reach_field(h_" in hdr and "dspmap_reach_paths(h_" in hdr
    assert "DSPMAP_REACH_WITH_CURRENT" in hdr


# ---- known answers of the restatement on hand-made grids.  Maps at 0.5 m: cell i of an axis of n cells has its centre at
# -0.25 n + 0.5 i + 0.25
def _centre(cfg, x, y, z):
    return (-0.25 * cfg.nx + 0.5 * x + 0.25, -0.25 * cfg.ny + 0.5 * y + 0.25, -0.25 * cfg.nz + 0.5 * z + 0.25)


def _src(cfg, *cells):
    """sources at the centres of cells (x, y, z) or (x, y, z, field)"""
    return R.points([_centre(cfg, *c[:3]) + ((c[3] if len(c) > 3 else 0),) for c in cells])


def _manhattan(cfg, cells):
    z, y, x = np.meshgrid(np.arange(cfg.nz), np.arange(cfg.ny), np.arange(cfg.nx), indexing="ij")
    return np.min([np.abs(x - c[0]) + np.abs(y - c[1]) + np.abs(z - c[2]) for c in cells], 0)


@pytest.fixture(scope="module")
def box(dsp):
    return dsp.make_config(nx=8, ny=6, nz=5, res=0.5, pred_times=(0.1, 0.5, 1.0))


@pytest.fixture(scope="module")
def corridor(dsp):
    return dsp.make_config(nx=8, ny=1, nz=1, res=0.5, pred_times=(0.5, 1.0))


def _empty(cfg):
    return np.zeros((cfg.prediction_times + 1, cfg.nz, cfg.ny, cfg.nx), bool)


def test_reach_ref_pack_round_trip():
    rng = np.random.default_rng(3)
    for nx in (1, 8, 63, 64, 65, 132):
        cells = rng.random((2, 3, 4, nx)) < 0.4
        words = R.pack(cells)
        assert words.shape == (2, 3, 4, (nx + 63) // 64) and words.dtype == np.uint64
        assert np.array_equal(R.unpack(words, nx), cells)
        assert int(words[0, 0, 0, 0]) & 1 == int(cells[0, 0, 0, 0])          # bit x & 63 of word x >> 6
        if nx > 64:
            assert (int(words[1, 2, 3, 1]) >> 0) & 1 == int(cells[1, 2, 3, 64])


def test_reach_ref_empty_grid_is_manhattan_distance_cut_at_max_steps(box):
    srcs = ((1, 1, 1), (6, 4, 3))
    want = _manhattan(box, srcs)
    for kw in (dict(), dict(t_start=0.0, step_seconds=0.2), dict(t_start=3.0, step_seconds=0.0, with_current=True)):
        val = R.fields(box, _empty(box), _src(box, *srcs), 1, max_steps=64, **kw)[0]
        assert np.array_equal(val, want), kw
    cut = R.fields(box, _empty(box), _src(box, *srcs), 1, max_steps=3)[0]
    assert np.array_equal(cut, np.where(want <= 3, want, U)) and (cut == U).any() and (cut == 3).any()
    # fields are independent: field 1 is grown from its own source only, field 2 has none
    three = R.fields(box, _empty(box), _src(box, (1, 1, 1, 0), (6, 4, 3, 1)), 3, max_steps=64)
    assert np.array_equal(three[0], _manhattan(box, srcs[:1])) and np.array_equal(three[1], _manhattan(box, srcs[1:])) and (three[2] == U).all()


def test_reach_ref_wall_with_one_hole(box):
    lay = _empty(box)
    lay[0, :, :, 4] = True              # a wall across the map at x = 4 ...
    lay[0, 3, 5, 4] = False             # ... with one hole at (4, 5, 3)
    val = R.fields(box, lay, _src(box, (1, 0, 0)), 1, max_steps=64)[0]
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(8), indexing="ij")
    near = np.abs(x - 1) + y + z
    through = (3 + 5 + 3) + np.abs(x - 4) + np.abs(y - 5) + np.abs(z - 3)
    want = np.where(x < 4, near, through)
    want[lay[0]] = U
    assert np.array_equal(val, want) and val[3, 5, 4] == 11 and val[0, 0, 7] == 11 + 3 + 5 + 3
    R.check_free(box, lay, val[None])
    R.check_predecessors(box, lay, val[None], _src(box, (1, 0, 0)))
    # closed, the far side is never reached
    lay[0, 3, 5, 4] = True
    shut = R.fields(box, lay, _src(box, (1, 0, 0)), 1, max_steps=64)[0]
    assert (shut[:, :, 4:] == U).all() and np.array_equal(shut[:, :, :4], near[:, :, :4])


SCHED = dict(t_start=0.0, step_seconds=0.25, max_steps=64)    # steps 0, 1, 2 test layer 1 (t <= 0.5), step 3 onwards layer 2


def test_reach_ref_corridor_with_a_changing_layer(corridor):
    assert R.schedule(corridor, 0.0, 0.25, 6).tolist() == [1, 1, 1, 2, 2, 2, 2] and not R.time_invariant(corridor, 0.0, 0.25, 6)
    assert R.time_invariant(corridor, 0.0, 0.25, 2) and R.time_invariant(corridor, -1.0, 0.25, 64) and R.time_invariant(corridor, 0.75, 9.0, 64)
    lay = _empty(corridor)
    lay[1, 0, 0, 2] = True
    val = R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, **SCHED)[0]
    assert val[0, 0].tolist() == [0, 1, 3, 4, 5, 6, 7, 8]                    # the front waits in front of cell 2 until the layer changes
    R.check_free(corridor, lay, val[None], **SCHED)
    R.check_predecessors(corridor, lay, val[None], _src(corridor, (0, 0, 0)), **SCHED)
    # the static answers on either layer
    assert R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, t_start=0.0, max_steps=64)[0, 0, 0].tolist() == [0, 1, U, U, U, U, U, U]
    assert R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, t_start=0.75, max_steps=64)[0, 0, 0].tolist() == list(range(8))
    assert R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, t_start=-1.0, step_seconds=0.25, max_steps=64)[0, 0, 0].tolist() == list(range(8))
    # max_steps cuts a scheduled field too
    assert R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, t_start=0.0, step_seconds=0.25, max_steps=5)[0, 0, 0].tolist() == [0, 1, 3, 4, 5, U, U, U]


def test_reach_ref_reached_cells_are_removed(corridor):
    lay = _empty(corridor)
    lay[1, 0, 0, 2] = True
    lay[2, 0, 0, 0:2] = True
    val, sets = R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, return_sets=True, **SCHED)
    assert val[0, 0, 0].tolist() == [0, 1, 3, 4, 5, 6, 7, 8]                 # first arrivals stay; the front goes on from cell 2
    assert sets[2][0, 0, 0].tolist() == [True, True] + [False] * 6
    assert sets[3][0, 0, 0].tolist() == [False, False, True] + [False] * 5   # cells 0 and 1 are removed at step 3
    assert sets[5][0, 0, 0].tolist() == [False, False, True, True, True, False, False, False]
    R.check_free(corridor, lay, val, **SCHED)
    R.check_predecessors(corridor, lay, val, _src(corridor, (0, 0, 0)), **SCHED)


def test_reach_ref_dead_front_reaches_nothing_afterwards(corridor):
    lay = _empty(corridor)
    lay[1, 0, 0, 2] = True
    lay[2, 0, 0, 0:3] = True            # at step 3 every reached cell and every candidate is blocked: R_3 is empty
    val, sets = R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, return_sets=True, **SCHED)
    assert val[0, 0, 0].tolist() == [0, 1, U, U, U, U, U, U] and not sets[3].any()
    assert not lay[2, 0, 0, 3:].any()   # ... although cells 3 .. 7 are free from then on
    # a blocked source never starts
    lay = _empty(corridor)
    lay[1, 0, 0, 0] = True
    assert (R.fields(corridor, lay, _src(corridor, (0, 0, 0)), 1, **SCHED) == U).all()


def test_reach_ref_with_current_changes_an_answer(corridor):
    lay = _empty(corridor)
    lay[0, 0, 0, 4] = True              # only the current layer holds an obstacle
    src = _src(corridor, (0, 0, 0))
    assert R.fields(corridor, lay, src, 1, **SCHED)[0, 0, 0].tolist() == list(range(8))
    assert R.fields(corridor, lay, src, 1, with_current=True, **SCHED)[0, 0, 0].tolist() == [0, 1, 2, 3, U, U, U, U]
    assert R.fields(corridor, lay, src, 1, t_start=-1.0, max_steps=64)[0, 0, 0].tolist() == [0, 1, 2, 3, U, U, U, U]
    lay[0, 0, 0, 4] = False
    lay[1, 0, 0, 4] = True              # ... and WITH_CURRENT adds nothing else
    for wc in (False, True):
        assert R.fields(corridor, lay, src, 1, with_current=wc, **SCHED)[0, 0, 0].tolist() == list(range(8))   # cell 4 is met at step 4: layer 2


def test_reach_ref_path_order_decides_between_equal_neighbours(box):
    lay = _empty(box)
    src = _src(box, (2, 2, 2))
    val = R.fields(box, lay, src, 1, max_steps=64)
    start = _src(box, (4, 4, 3))        # value 5; -x (3, 4, 3), -y (4, 3, 3) and -z (4, 4, 2) all have value 4: -x is first in the order
    steps, cells = R.paths(box, val, start, 8)
    g = lambda x, y, z: (z * 6 + y) * 8 + x   # noqa: E731
    assert steps.tolist() == [5]
    assert cells[0].tolist() == [g(4, 4, 3), g(3, 4, 3), g(2, 4, 3), g(2, 3, 3), g(2, 2, 3), g(2, 2, 2), -1, -1]
    assert R.check_paths(box, val, start, steps, cells) == 1
    # from the other side +x comes before -y, and -y before -z
    steps, cells = R.paths(box, val, _src(box, (0, 4, 3)), 8)
    assert cells[0].tolist() == [g(0, 4, 3), g(1, 4, 3), g(2, 4, 3), g(2, 3, 3), g(2, 2, 3), g(2, 2, 2), -1, -1]
    # max_len cuts a path; max_len 0 gives the steps alone
    steps, cells = R.paths(box, val, start, 3)
    assert steps.tolist() == [5] and cells[0].tolist() == [g(4, 4, 3), g(3, 4, 3), g(2, 4, 3)] and R.check_paths(box, val, start, steps, cells) == 0
    steps, cells = R.paths(box, val, start, 0)
    assert steps.tolist() == [5] and cells.shape == (1, 0)
    # unreached, outside, invalid
    lay[0, 0, 0, 0] = True
    val = R.fields(box, lay, src, 1, max_steps=64)
    bad = R.points([_centre(box, 0, 0, 0) + (0,), (2.5, 0.0, 0.0, 0), (np.nan, 0.0, 0.0, 0), _centre(box, 1, 1, 1) + (1,), _centre(box, 1, 1, 1) + (-1,),
                    (9.0, 0.0, 0.0, 7)])
    steps, cells = R.paths(box, val, bad, 4)
    assert steps.tolist() == [-1, -2, -3, -3, -3, -3] and (cells == -1).all()
    R.check_paths(box, val, bad, steps, cells)


def test_reach_ref_ignored_sources(box):
    good = _src(box, (3, 2, 2))
    want = R.fields(box, _empty(box), good, 2, max_steps=64)
    inside = _centre(box, 5, 5, 4)
    junk = R.points([(2.5, 0.0, 0.0, 0), (0.0, -1.5, 0.0, 0), (2.0, 0.0, 0.0, 0), (0.0, 0.0, 7.0, 1),          # outside the map (+-half itself is outside)
                     (float(np.nextafter(F(2), F(0))), 0.0, 0.0, 0),                                        # trunc(u) == nx
                     (np.nan, 0.0, 0.0, 0), (0.0, np.inf, 0.0, 1), (0.0, 0.0, -np.inf, 0),                  # non-finite
                     inside + (2,), inside + (-1,), inside + (64,), inside + (1 << 30,)])                   # a field outside [0, n_fields)
    got = R.fields(box, _empty(box), np.concatenate([junk[:6], good, junk[6:]]), 2, max_steps=64)
    assert np.array_equal(got, want) and (want[1] == U).all() and want[0, 2, 2, 3] == 0
    assert R.fields(box, _empty(box), np.concatenate([good, R.points([inside + (1,)])]), 2, max_steps=64)[1, 4, 5, 5] == 0    # ... a valid field counts
    assert (R.fields(box, _empty(box), junk, 2, max_steps=64) == U).all() and (R.fields(box, _empty(box), junk[:0], 1, max_steps=4) == U).all()


def test_reach_ref_world_frame_equals_map_frame_shifted(box):
    rng = np.random.default_rng(5)
    lay = rng.random((4, 5, 6, 8)) < 0.15
    n = 40
    src = np.zeros(n, R.POINT_DTYPE)
    half = np.array([2.0, 1.5, 1.25])
    p = np.round(rng.uniform(-1.05, 1.05, (n, 3)) * half * 1024) / 1024          # a 2^-10 lattice: the shift below is exact in fp32
    src["x"], src["y"], src["z"], src["field"] = p[:, 0], p[:, 1], p[:, 2], rng.integers(-1, 4, n)
    cur = np.array([8.0, -4.0, 2.0], F)
    shifted = src.copy()
    shifted["x"] += cur[0]
    shifted["y"] += cur[1]
    shifted["z"] += cur[2]
    kw = dict(t_start=0.05, step_seconds=0.1, max_steps=40)
    want = R.fields(box, lay, src, 3, **kw)
    assert np.array_equal(R.fields(box, lay, shifted, 3, world=True, cur_pos=cur, **kw), want)
    assert not np.array_equal(R.fields(box, lay, shifted, 3, **kw), want) and (want != U).any() and (want == U).any()
    static = R.fields(box, lay, src, 3, t_start=-1.0, max_steps=40)
    s1, c1 = R.paths(box, static, src, 12)
    s2, c2 = R.paths(box, static, shifted, 12, world=True, cur_pos=cur)
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2) and set(s1.tolist()) >= {0, -2, -3}


@pytest.mark.parametrize("density", [0.05, 0.3, 0.6])
def test_reach_ref_passes_the_independent_checkers(dsp, density):
    cfg = dsp.make_config(nx=21, ny=17, nz=9, res=0.2, pred_times=(0.1, 0.5, 1.0))
    rng = np.random.default_rng(int(density * 100))
    lay = rng.random((4, 9, 17, 21)) < density
    n = 30
    src = np.zeros(n, R.POINT_DTYPE)
    p = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([2.1, 1.7, 0.9])
    src["x"], src["y"], src["z"], src["field"] = p[:, 0], p[:, 1], p[:, 2], rng.integers(0, 4, n)
    reached = moved = 0
    for kw in (dict(t_start=-1.0), dict(t_start=0.0, step_seconds=0.08), dict(t_start=0.3, step_seconds=0.0, with_current=True),
               dict(t_start=0.0, step_seconds=0.3, with_current=True, max_steps=6)):
        kw.setdefault("max_steps", 80)
        val = R.fields(cfg, lay, src, 4, **kw)
        reached += R.check_free(cfg, lay, val, **kw)
        moved += R.check_predecessors(cfg, lay, val, src, **kw)
        if R.time_invariant(cfg, kw["t_start"], kw.get("step_seconds", 0.0), kw["max_steps"]):
            steps, cells = R.paths(cfg, val, src, 90)
            assert R.check_paths(cfg, val, src, steps, cells) == (steps >= 0).sum()
    assert reached > 100 and moved > 50
