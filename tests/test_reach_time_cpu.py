"""CPU tests of the space-time paths (dspmap_build_reach_timeline*, dspmap_reach_timeline_paths*, dspmap_get_reach_sets,
dspmap_reach_last_steps, dspmap_reach_timeline_device): the entry points are exported and bound, argument errors -- the cap on the kept
sets among them -- are DSPMAP_E_ARG with a text before any device is touched, a slab handle and a missing grid / timeline are
DSPMAP_E_STATE, the drop-in class offers the new members, and known answers of the numpy restatement (tests/reach_time_ref.py) that the GPU
tests hold the kernels to, with a checker that is shown to reject what it must."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import reach_ref as R
from tests import reach_time_ref as TR

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_build_reach_timeline", "dspmap_build_reach_timeline_device", "dspmap_reach_timeline_device", "dspmap_reach_last_steps",
         "dspmap_get_reach_sets", "dspmap_reach_timeline_paths", "dspmap_reach_timeline_paths_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_timeline_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
    assert dsp.capi.REACH_TIMELINE_MAX_BYTES == 1 << 30
    for meth in ("build_reach_timeline", "reach_sets", "reach_last_steps", "reach_timeline_ptr", "reach_timeline_paths"):
        assert callable(getattr(dsp.DSPMap, meth))
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    assert "#define DSPMAP_REACH_TIMELINE_MAX_BYTES (1ull << 30)" in hdr
    for n in NAMES:
        assert n + "(dspmap_t* m" in hdr, n


def test_timeline_build_argument_errors_and_cap(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(**TR.SCENE_CFG))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    src = np.zeros(4, R.POINT_DTYPE)
    for fn in (L.dspmap_build_reach_timeline, L.dspmap_build_reach_timeline_device):
        assert fn(None, 1, 4, _p(src), 0.0, 0.1, 16, 0) == E_ARG
        for nf in (0, -1, 65, 1 << 20):
            assert fn(h, nf, 4, _p(src), 0.0, 0.1, 16, 0) == E_ARG and b"n_fields" in err(), nf
        assert fn(h, 1, -1, _p(src), 0.0, 0.1, 16, 0) == E_ARG and b"negative" in err()
        assert fn(h, 1, 4, None, 0.0, 0.1, 16, 0) == E_ARG and b"NULL" in err()
        assert fn(h, 1, 4, _p(src), float("nan"), 0.1, 16, 0) == E_ARG and b"t_start" in err()
        for dt in (float("nan"), -0.1, float("inf")):
            assert fn(h, 1, 4, _p(src), 0.0, dt, 16, 0) == E_ARG and b"step_seconds" in err(), dt
        for ms in (0, -1, 4097):
            assert fn(h, 1, 4, _p(src), 0.0, 0.1, ms, 0) == E_ARG and b"max_steps" in err(), ms
        for fl in (8, 16, 15, -1):
            assert fn(h, 1, 4, _p(src), 0.0, 0.1, 16, fl) == E_ARG and b"flags" in err(), fl
        # the cap: 64 fields x 4097 steps x 960 words x 8 bytes = 2.0 GB on 40 x 40 x 24; the text names both numbers
        assert 64 * 4097 * 960 * 8 == 2013757440 > 1 << 30
        assert fn(h, 64, 4, _p(src), 0.0, 0.1, 4096, 0) == E_ARG and b"2013757440" in err() and b"1073741824" in err()
        # ... the largest requests below it, and every flag, reach the state check: 1 field x 4097 rows, 64 fields x 2184 rows
        assert 64 * 2184 * 960 * 8 <= 1 << 30 < 64 * 2185 * 960 * 8
        assert fn(h, 64, 4, _p(src), 0.0, 0.1, 2184, 0) == E_ARG and b"DSPMAP_REACH_TIMELINE_MAX_BYTES" in err()
        for args in ((1, 4, _p(src), float("inf"), 0.0, 4096, 0), (64, 0, None, -1.0, 0.0, 2183, 7), (3, 4, _p(src), -1.0, 2.5, 7, 4)):
            assert fn(h, *args) == E_STATE and b"dspmap_build_cast_grid" in err(), args
    # the plain build has no cap
    assert L.dspmap_build_reach_fields(h, 64, 4, _p(src), 0.0, 0.1, 4096, 0) == E_STATE
    m.close()
    slab = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    for fn in (L.dspmap_build_reach_timeline, L.dspmap_build_reach_timeline_device):
        assert fn(slab.h, 1, 4, _p(src), 0.0, 0.1, 16, 0) == E_STATE and b"slab" in L.dspmap_last_error(slab.h)
        assert fn(slab.h, 1, 4, _p(src), 0.0, 0.1, 0, 0) == E_ARG
    slab.close()


def test_timeline_accessor_and_paths_argument_errors_and_state(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    st, steps, cells = np.zeros(4, R.POINT_DTYPE), np.zeros(4, np.int32), np.zeros((4, 8), np.int32)
    for fn in (L.dspmap_reach_timeline_paths, L.dspmap_reach_timeline_paths_device):
        assert fn(None, 4, _p(st), 8, 0, _p(steps), _p(cells)) == E_ARG
        assert fn(h, -1, _p(st), 8, 0, _p(steps), _p(cells)) == E_ARG and b"negative" in err()
        for ml in (-1, 4098):
            assert fn(h, 4, _p(st), ml, 0, _p(steps), _p(cells)) == E_ARG and b"max_len" in err(), ml
        assert fn(h, 4, None, 8, 0, _p(steps), _p(cells)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(st), 8, 0, None, _p(cells)) == E_ARG and b"NULL" in err()
        assert fn(h, 4, _p(st), 8, 0, _p(steps), None) == E_ARG and b"cells_out" in err()
        for fl in (2, 4, 3, -1):
            assert fn(h, 4, _p(st), 8, fl, _p(steps), _p(cells)) == E_ARG and b"flags" in err(), fl
        for args in ((4, _p(st), 0, 0, _p(steps), None), (4, _p(st), 4097, 1, _p(steps), _p(cells)), (0, None, 8, 0, None, None)):
            assert fn(h, *args) == E_STATE and b"dspmap_build_reach_timeline" in err(), args
    words = np.zeros((2, 10, 20, 1), np.uint64)
    assert L.dspmap_get_reach_sets(None, 0, 0, 1, _p(words)) == E_ARG
    for f in (-1, 64):
        assert L.dspmap_get_reach_sets(h, f, 0, 1, _p(words)) == E_ARG and b"field" in err()
    assert L.dspmap_get_reach_sets(h, 0, -1, 1, _p(words)) == E_ARG and b"first_step" in err()
    assert L.dspmap_get_reach_sets(h, 0, 0, -1, _p(words)) == E_ARG and b"n_steps" in err()
    assert L.dspmap_get_reach_sets(h, 0, 4096, 2, _p(words)) == E_ARG and L.dspmap_get_reach_sets(h, 0, 4098, 0, _p(words)) == E_ARG
    assert L.dspmap_get_reach_sets(h, 0, 0, 2, None) == E_ARG and b"NULL" in err()
    for args in ((0, 0, 2, _p(words)), (63, 4096, 1, _p(words)), (0, 4097, 0, None)):
        assert L.dspmap_get_reach_sets(h, *args) == E_STATE and b"dspmap_build_reach_timeline" in err(), args
    last = np.zeros(64, np.int32)
    assert L.dspmap_reach_last_steps(None, _p(last)) == E_ARG
    assert L.dspmap_reach_last_steps(h, None) == E_ARG and b"NULL" in err()
    assert L.dspmap_reach_last_steps(h, _p(last)) == E_STATE and b"dspmap_build_reach_timeline" in err()
    assert not words.any() and not last.any() and not steps.any()
    assert L.dspmap_reach_timeline_device(h) is None and L.dspmap_reach_timeline_device(None) is None and m.reach_timeline_ptr() is None
    for call in (lambda: m.reach_timeline_paths(st, 8), lambda: m.reach_sets(0), lambda: m.reach_last_steps(1),
                 lambda: m.build_reach_timeline(np.zeros((3, 4), np.float32), n_fields=65)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    with pytest.raises(ValueError):
        m.build_reach_timeline(np.zeros((3, 5), np.float32))
    m.close()
    slab = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15, z_lo=0, z_hi=5))
    assert L.dspmap_reach_timeline_paths(slab.h, 4, _p(st), 8, 0, _p(steps), _p(cells)) == E_STATE and b"slab" in L.dspmap_last_error(slab.h)
    assert L.dspmap_get_reach_sets(slab.h, 0, 0, 2, _p(words)) == E_STATE and b"slab" in L.dspmap_last_error(slab.h)
    assert L.dspmap_reach_last_steps(slab.h, _p(last)) == E_STATE and b"slab" in L.dspmap_last_error(slab.h)
    slab.close()


def test_timeline_valid_build_needs_device(dsp):
    """a valid call is a grid and a build: without a device the grid's build is DSPMAP_E_DEVICE and the timeline finds no grid"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    have = torch.cuda.is_available()
    assert L.dspmap_build_cast_grid(m.h, 0.5, 0, 0) == (OK if have else E_DEVICE)
    src = R.points([(0.0, 0.0, 0.0, 0)])
    rc = L.dspmap_build_reach_timeline(m.h, 1, 1, _p(src), -1.0, 0.0, 5, 0)
    assert rc == (OK if have else E_STATE)
    if have:
        assert m.reach_last_steps(1).tolist() == [5] and m.reach_timeline_ptr() is not None
    else:
        assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h) and m.reach_timeline_ptr() is None
    m.close()


def test_dropin_class_offers_timeline_members(dsp, tmp_path):
    """include/dsp_dynamic.h: buildReachTimeline, getReachSets and reachTimelinePaths type-check and forward to the C ABI"""
    src = tmp_path / "reach_time.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n    dspmap_reach_point s[2] = {{0.f, 0.f, 0.f, 0}, {1.f, 0.f, 0.f, 1}};\n'
                   "    static_assert(DSPMAP_REACH_TIMELINE_MAX_BYTES == 1073741824ull, \"cap\");\n"
                   "    std::vector<unsigned long long> w(3 * 1000);\n    int steps[2], cells[2 * 65];\n"
                   "    int a = my_map.buildCastGrid(0.2f, 2);\n"
                   "    int b = my_map.buildReachTimeline(2, 2, s, 0.f, 0.1f, 64);\n"
                   "    int c = my_map.buildReachTimeline(2, 2, s, 0.f, 0.1f, 64, true, true);\n"
                   "    int d = my_map.getReachSets(1, 0, 3, w.data());\n"
                   "    int e = my_map.reachTimelinePaths(2, s, 65, steps, cells) + my_map.reachTimelinePaths(2, s, 0, steps, nullptr, true);\n"
                   "    return a + b + c + d + e + steps[0] + cells[0] + (int)w[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    assert "dspmap_build_reach_timeline(h_" in hdr and "dspmap_get_reach_sets(h_" in hdr and "dspmap_reach_timeline_paths(h_" in hdr


# ---- known answers of the restatement
@pytest.fixture(scope="module")
def cfg(dsp):
    c = dsp.make_config(**TR.SCENE_CFG)
    assert c.prediction_times == 6
    return c


@pytest.fixture(scope="module")
def door(cfg):
    lay, src, nf, starts, sched = TR.opening_door_scene(cfg)
    val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **sched)
    return lay, src, nf, starts, sched, val, sets


def test_timeline_ref_opening_door(cfg, door):
    lay, src, nf, starts, sched, val, sets = door
    layers = R.schedule(cfg, **sched)
    assert layers[9:12].tolist() == [2, 2, 3] and not R.time_invariant(cfg, **sched)
    assert val[0, 5, 10, 20] == 11 and val[0, 5, 10, 25] == 16 and val[0, 5, 10, 19] == 4
    steps, cells = TR.timeline_paths(cfg, val, sets, starts, 160)
    assert steps.tolist()[:4] == [16, 11, 0, 4]
    g = cells[0, :17]
    assert (g % 40).tolist() == [25, 24, 23, 22, 21, 20, 19, 19, 19, 19, 19, 19, 19, 18, 17, 16, 15]      # six waits before the door
    assert ((g // 40) % 40 == 10).all() and (g // 1600 == 5).all() and (cells[0, 17:] == -1).all()
    done, waits = TR.check_timeline_paths(cfg, lay, src, nf, starts, steps, cells, **sched)
    assert done == (steps >= 0).sum() == len(starts) and waits >= 1
    # first arrivals alone do not give this path: the cell before the door has value 4, its successor on the path value 11
    assert val[0, 5, 10, 19] != val[0, 5, 10, 20] - 1
    # sets behind the early exit repeat the last one, and max_len cuts the row, not the steps
    assert len(sets) - 1 < sched["max_steps"] and TR.set_at(sets, 150) is sets[-1] and TR.set_at(sets, 3) is sets[3]
    for ml in (0, 1, 16, 17):
        s, c = TR.timeline_paths(cfg, val, sets, starts[:1], ml)
        assert s.tolist() == [16] and c.shape == (1, ml) and np.array_equal(c[0], g[:ml])
        TR.check_timeline_paths(cfg, lay, src, nf, starts[:1], s, c, val=val, **sched)


def test_timeline_ref_checker_rejects_bad_paths(cfg, door):
    lay, src, nf, starts, sched, val, sets = door
    steps, cells = TR.timeline_paths(cfg, val, sets, starts[:1], 20)
    chk = lambda s, c: TR.check_timeline_paths(cfg, lay, src, nf, starts[:1], s, c, val=val, **sched)   # noqa: E731
    assert chk(steps, cells) == (1, 1)
    jump = cells.copy()
    jump[0, 3] += 2                                   # (22, 10, 5) -> (24, 10, 5): two cells from both neighbours on the path
    with pytest.raises(AssertionError, match="jump"):
        chk(steps, jump)
    early = cells.copy()
    early[0, 6:12] = cells[0, 5]                      # waits IN the door instead of before it: the door is shut at steps 10 .. 5
    early[0, 12] = cells[0, 6]
    with pytest.raises(AssertionError, match="blocked"):
        chk(steps, early)
    off = cells.copy()
    off[0, 16] = cells[0, 15]                         # stays one cell short of the source
    with pytest.raises(AssertionError, match="source"):
        chk(steps, off)
    with pytest.raises(AssertionError):
        chk(steps + 1, cells)                         # a wrong value
    tail = cells.copy()
    tail[0, 18] = 0
    with pytest.raises(AssertionError):
        chk(steps, tail)                              # something behind the end
    other = cells.copy()
    other[0, 0] = cells[0, 1]
    with pytest.raises(AssertionError):
        chk(steps, other)                             # not the start's cell


def test_timeline_ref_equals_descent_on_time_invariant_builds(cfg):
    lay, src, nf, starts, _ = TR.invariant_scene(cfg)
    reached = 0
    for sched in (TR.STATIC, TR.FROZEN):
        assert R.time_invariant(cfg, **sched)
        val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **sched)
        assert all((b | ~a).all() for a, b in zip(sets[:-1], sets[1:]))       # monotone: R_{n-1} is a subset of R_n
        got, want = TR.timeline_paths(cfg, val, sets, starts, 210), R.paths(cfg, val, starts, 210)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        done, waits = TR.check_timeline_paths(cfg, lay, src, nf, starts, *got, val=val, **sched)
        assert waits == 0 and done == (got[0] >= 0).sum()
        reached = int((got[0] >= 0).sum())
    assert reached >= 150


def test_timeline_ref_changing_clutter(cfg):
    lay, src, nf, starts, sched = TR.changing_clutter_scene(cfg)
    assert all((lay[l] != lay[l + 1]).any() for l in range(6)) and set(R.schedule(cfg, **sched).tolist()) == set(range(1, 7))
    val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **sched)
    assert not all((b | ~a).all() for a, b in zip(sets[:-1], sets[1:]))       # cells are removed: the sets are not monotone
    steps, cells = TR.timeline_paths(cfg, val, sets, starts, 130)
    done, waits = TR.check_timeline_paths(cfg, lay, src, nf, starts, steps, cells, **sched)
    print("reached", int((steps >= 0).sum()), "complete", done, "with a wait", waits, "longest", int(steps.max()))
    assert (steps >= 0).sum() >= 100 and waits >= 10 and done == (steps >= 0).sum()
    assert set(np.unique(steps[steps < 0]).tolist()) == {-1, -2, -3}
