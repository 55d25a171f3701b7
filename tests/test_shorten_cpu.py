"""CPU tests of the shortened paths (dspmap_shorten_paths*): the entry points are exported, bound and built from their own kernel file; the
rule is well-posed on the test configurations (every voxel centre lies in its own voxel, and the restatement's vertices are
dspmap_voxel_center's bits); and hand-worked answers of the numpy restatement (tests/shorten_ref.py) that the GPU tests hold the kernel
to, on the empty 40 x 40 x 24 grid with T = 6 and on small scenes in it, with a checker that is shown to reject what it must."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import reach_ref as R
from tests import reach_time_ref as TR
from tests import shorten_ref as S

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dspmap_shorten_paths", "dspmap_shorten_paths_device")
SMALL = dict(TR.SCENE_CFG)                       # SMALL of tests/test_gpu_cast.py without its particle count: 40 x 40 x 24 at 0.15 m, T = 6
SHAPES = [SMALL, dict(nx=64, ny=6, nz=3, res=0.15), dict(nx=65, ny=6, nz=3, res=0.15), dict(nx=132, ny=40, nz=12, res=0.15),
          dict(nx=50, ny=37, nz=23, res=0.15)]


def test_shorten_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert n + "(dspmap_t* m" in hdr, n
    assert "#define DSPMAP_SHORTEN_MAX_WINDOW 64" in hdr and dsp.capi.SHORTEN_MAX_WINDOW == S.MAX_WINDOW == 64
    assert "compressing waits out of a path" not in hdr
    assert dsp.capi.PATH_INFO_DTYPE == S.INFO_DTYPE and S.INFO_DTYPE.itemsize == 16
    assert callable(dsp.DSPMap.shorten_paths)
    assert "shortenPaths" in open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    assert '"dspmap_shorten.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()
    assert b"k_shorten" in open(dsp.capi.LIB_PATH, "rb").read()
    src = open(os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_shorten.hip")).read()
    assert "cast_walk(" in src and '#include "dspmap_cast_walk.h"' in src      # the walk is called, not restated


@pytest.mark.parametrize("kw", SHAPES, ids=lambda kw: "%dx%dx%d" % (kw["nx"], kw["ny"], kw["nz"]))
def test_every_voxel_centre_lies_in_its_own_voxel(dsp, kw):
    """without this the rule is ill-posed: a vertex would be cast from another cell than the path's"""
    m = dsp.DSPMap(dsp.make_config(**kw))
    cfg, L = m.cfg, m.L
    V = cfg.nx * cfg.ny * cfg.nz
    x, y, z, idx = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    got = np.zeros((V, 3), F)
    for i in range(V):
        L.dspmap_voxel_center(m.h, i, C.byref(x), C.byref(y), C.byref(z))
        got[i] = (x.value, y.value, z.value)
        assert L.dspmap_point_voxel_index(m.h, x, y, z, C.byref(idx)) == 1 and idx.value == i, i
    cells = np.arange(V, dtype=np.int32)[:, None]
    want = S.vertices(cfg, np.zeros(V, np.int32), cells, np.zeros(V, np.int64), -1.0, 0.0)
    assert np.array_equal(got.view(np.uint32), want[:, :3].view(np.uint32)) and (want[:, 3] == -1.0).all()
    m.close()


def _cfg(dsp):
    c = dsp.make_config(**SMALL)
    assert (c.nx, c.ny, c.nz, c.prediction_times) == (40, 40, 24, 6)
    return c


def _empty(cfg):
    return np.zeros((cfg.prediction_times + 1, cfg.nz, cfg.ny, cfg.nx), bool)


def _g(cfg, x, y, z):
    return (z * cfg.ny + y) * cfg.nx + x


def _rows(cfg, paths, max_len):
    """cells [n, max_len] of lists of (x, y, z), padded with -1; steps = cells - 1, a wavefront path's first arrival"""
    cells = np.full((len(paths), max_len), -1, np.int32)
    for i, p in enumerate(paths):
        cells[i, :len(p)] = [_g(cfg, *c) for c in p]
    return np.array([len(p) - 1 for p in paths], np.int32), cells


def _ends(info, end, i=0):
    return end[i, :info["n_segments"][i]].tolist()


def test_straight_path_staircase_and_window(dsp):
    cfg = _cfg(dsp)
    lay = _empty(cfg)
    straight = [(5 + j, 10, 5) for j in range(30)]
    stairs = [(5 + (j + 1) // 2, 5 + j // 2, 7) for j in range(31)]          # +x, +y, +x, ...: 31 cells from (5, 5) to (20, 20)
    assert stairs[0] == (5, 5, 7) and stairs[1] == (6, 5, 7) and stairs[2] == (6, 6, 7) and stairs[-1] == (20, 20, 7)
    steps, cells = _rows(cfg, [straight, stairs], 40)
    info, seg, end = S.shorten(cfg, lay, steps, cells)
    assert info["n_cells"].tolist() == [30, 31] and info["n_segments"].tolist() == [1, 1] and not info["n_blocked"].any()
    assert _ends(info, end, 0) == [29] and _ends(info, end, 1) == [30] and seg.shape == (2, 39, 8) and not info["truncated"].any()
    res, hx, hy, hz = 0.15, 3.0, 3.0, 1.8
    assert np.allclose(seg[0, 0], [-hx + 5.5 * res, -hy + 10.5 * res, -hz + 5.5 * res, -1, -hx + 34.5 * res, -hy + 10.5 * res, -hz + 5.5 * res, -1])
    assert S.check(cfg, lay, steps, cells, info, seg, end) == (2, 0, 0, 30)
    info, seg, end = S.shorten(cfg, lay, steps, cells, window=8)
    assert _ends(info, end, 0) == [8, 16, 24, 29] and _ends(info, end, 1) == [8, 16, 24, 30]
    assert S.check(cfg, lay, steps, cells, info, seg, end, window=8) == (8, 0, 0, 8)
    info, seg, end = S.shorten(cfg, lay, steps, cells, window=1)
    assert _ends(info, end, 0) == list(range(1, 30))
    # with times: the empty grid is empty in every layer, the vertices carry the steps' times
    info, seg, end = S.shorten(cfg, lay, steps, cells, t_start=0.25, step_seconds=0.05)
    assert _ends(info, end, 0) == [29] and seg[0, 0, 3] == F(F(0.25) + F(F(29) * F(0.05))) and seg[0, 0, 7] == F(0.25)
    S.check(cfg, lay, steps, cells, info, seg, end, t_start=0.25, step_seconds=0.05)


def test_l_around_a_wall_corner(dsp):
    """a wall at x = 20 for y <= 18; the path runs up x = 18 from y = 10 to y = 22 (positions 0 .. 12) and then along y = 22 to x = 25
    (positions 13 .. 19).  From (18, 10) the segment to (20, 22) enters the column x = 20 at y = 19.5, above the wall: free.  The one to
    (21, 22) enters it at y = 16.5: blocked, and so is every later one.  From (20, 22) the rest is a straight line."""
    cfg = _cfg(dsp)
    lay = _empty(cfg)
    lay[:, :, :19, 20] = True
    path = [(18, 10 + j, 5) for j in range(13)] + [(19 + j, 22, 5) for j in range(7)]
    assert len(path) == 20 and path[14] == (20, 22, 5)
    steps, cells = _rows(cfg, [path], 20)
    info, seg, end = S.shorten(cfg, lay, steps, cells)
    assert _ends(info, end) == [14, 19] and info["n_blocked"][0] == 0
    assert S.check(cfg, lay, steps, cells, info, seg, end) == (2, 0, 0, 14)
    info, seg, end = S.shorten(cfg, lay, steps, cells, window=10)             # (18, 20) sees all of the row y = 22
    assert _ends(info, end) == [10, 19]


def test_opening_door_a_segment_spans_the_waits(dsp):
    """the timeline's path from (25, 10, 5) waits at x = 19 for steps 10 .. 4 (positions 6 .. 12).  Worked with t = 0.019 n and the door
    cell (20, 10, 5) open in the layers >= 3 (t > 0.2, steps >= 11): from position 0 (step 16) the segment to the door cell itself (position
    5, step 11) leaves it at t = 0.209: free; the one to position 6 leaves it at t = 0.1995: layer 2, shut, and so every later one.  From
    the door at step 11 to x = 19 at step 10 the door cell is tested from t = 0.209 to 0.1995: layers 3 and 2, blocked -- the adjacent
    step across a change of layer that n_blocked reports.  From position 6 everything is free: one segment over all the waits."""
    cfg = _cfg(dsp)
    lay, src, nf, starts, sched = TR.opening_door_scene(cfg)
    val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **sched)
    starts = np.concatenate([starts[:4], TR.at(cfg, (20, 30, 5))])          # (the last one: a wall cell, never reached)
    steps, cells = TR.timeline_paths(cfg, val, sets, starts, 40)
    assert steps.tolist() == [16, 11, 0, 4, -1]
    assert (cells[0, :17] % 40).tolist() == [25, 24, 23, 22, 21, 20, 19, 19, 19, 19, 19, 19, 19, 18, 17, 16, 15]
    ts = dict(t_start=sched["t_start"], step_seconds=sched["step_seconds"])
    info, seg, end = S.shorten(cfg, lay, steps, cells, **ts)
    assert info["n_cells"].tolist() == [17, 12, 1, 5, 0]
    assert _ends(info, end, 0) == [5, 6, 16] and info["n_blocked"].tolist() == [1, 1, 0, 0, 0]
    assert _ends(info, end, 1) == [1, 11] and _ends(info, end, 3) == [4] and not info["n_segments"][[2, 4]].any()
    assert seg[0, 2, 3] == F(F(0.019) * F(10)) and seg[0, 2, 7] == 0          # the spanning segment: from step 10 to step 0
    assert S.check(cfg, lay, steps, cells, info, seg, end, **ts)[:3] == (6, 2, 0)
    # statically (layer 0, where the door is shut) the same cells are cut at the wall
    info0, seg0, end0 = S.shorten(cfg, lay, steps, cells)
    assert _ends(info0, end0, 0) == [4, 5, 6, 16] and info0["n_blocked"][0] == 2
    S.check(cfg, lay, steps, cells, info0, seg0, end0)


def test_blocked_adjacent_cast_is_reported(dsp):
    """two cells, a caller-made path: (10, 10, 5) at step 1 (t = 0.1, layer 2) and (11, 10, 5) at step 0 (t = 0, layer 1), the second
    one occupied in the layers 1 and 2"""
    cfg = _cfg(dsp)
    lay = _empty(cfg)
    lay[1:3, 5, 10, 11] = True
    steps, cells = _rows(cfg, [[(10, 10, 5), (11, 10, 5)]], 4)
    info, seg, end = S.shorten(cfg, lay, steps, cells, t_start=0.0, step_seconds=0.1)
    assert info.tolist() == [(2, 1, 1, 0)] and end.tolist() == [[1, -1, -1]]
    assert S.check(cfg, lay, steps, cells, info, seg, end, t_start=0.0, step_seconds=0.1) == (1, 1, 0, 1)
    info, seg, end = S.shorten(cfg, lay, steps, cells)                        # layer 0 is empty
    assert info.tolist() == [(2, 1, 0, 0)]


def test_max_seg_edges_and_path_ends(dsp):
    cfg = _cfg(dsp)
    lay = _empty(cfg)
    V = cfg.nx * cfg.ny * cfg.nz
    straight = [(5 + j, 10, 5) for j in range(30)]
    steps, cells = _rows(cfg, [straight], 30)
    for max_seg, want in ((0, (30, 0, 0, 1)), (1, (30, 1, 0, 1)), (3, (30, 3, 0, 1)), (4, (30, 4, 0, 0)), (5, (30, 4, 0, 0))):
        info, seg, end = S.shorten(cfg, lay, steps, cells, window=8, max_seg=max_seg)
        assert info.tolist() == [want] and end.shape == (1, max_seg) and end[0].tolist() == ([8, 16, 24, 29] + [-1])[:max_seg], max_seg
        S.check(cfg, lay, steps, cells, info, seg, end, window=8)
    # what ends a path: steps < 0 (no cells at all), the first -1, the first index outside [0, V), max_len
    rows = np.full((7, 12), -1, np.int32)
    line = np.array([_g(cfg, 5 + j, 10, 5) for j in range(12)], np.int32)
    rows[:] = line
    rows[1, 5:] = -1
    rows[2, 7] = V
    rows[3, 3] = -7
    rows[4, 0] = -1
    rows[5, 1] = 2**31 - 1
    steps = np.array([-1, 11, 11, 11, 11, 11, 11], np.int32)
    info, seg, end = S.shorten(cfg, lay, steps, rows)
    assert info["n_cells"].tolist() == [0, 5, 7, 3, 0, 1, 12] and info["n_segments"].tolist() == [0, 1, 1, 1, 0, 0, 1]
    assert end[:, 0].tolist() == [-1, 4, 6, 2, -1, -1, 11] and (end[:, 1:] == -1).all() and not seg[[0, 4, 5]].any()
    S.check(cfg, lay, steps, rows, info, seg, end)
    # waits and jumps are legal in a caller-made path; a step count smaller than the path clamps the steps at 0
    path = [(5, 5, 5), (5, 5, 5), (9, 7, 5), (9, 7, 5), (2, 30, 20)]
    st, ce = _rows(cfg, [path], 6)
    st[0] = 2
    info, seg, end = S.shorten(cfg, lay, st, ce, t_start=0.0, step_seconds=0.5)
    assert info.tolist() == [(5, 1, 0, 0)] and seg[0, 0, 3] == 1.0 and seg[0, 0, 7] == 0.0
    S.check(cfg, lay, st, ce, info, seg, end, t_start=0.0, step_seconds=0.5)


def test_time_invariant_result_does_not_depend_on_step_seconds(dsp):
    cfg = _cfg(dsp)
    lay, src, nf, starts, _ = TR.invariant_scene(cfg)
    val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **TR.FROZEN)
    steps, cells = TR.timeline_paths(cfg, val, sets, starts[:60], 60)
    a = S.shorten(cfg, lay, steps, cells, t_start=0.3, step_seconds=0.0, window=16)
    b = S.shorten(cfg, lay, steps, cells, t_start=-1.0, step_seconds=0.7, window=16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1][..., :3], b[1][..., :3])
    assert a[0]["n_segments"].sum() > 60 and not a[0]["n_blocked"].any()
    S.check(cfg, lay, steps, cells, *a, t_start=0.3, step_seconds=0.0, window=16)


def test_the_checker_rejects_what_it_must(dsp):
    cfg = _cfg(dsp)
    lay = _empty(cfg)
    lay[:, :, :19, 20] = True
    path = [(18, 10 + j, 5) for j in range(13)] + [(19 + j, 22, 5) for j in range(7)]
    steps, cells = _rows(cfg, [path], 20)
    info, seg, end = S.shorten(cfg, lay, steps, cells)

    def rejects(i2, s2, e2, **kw):
        with pytest.raises(AssertionError):
            S.check(cfg, lay, steps, cells, i2, s2, e2, **kw)

    S.check(cfg, lay, steps, cells, info, seg, end)
    rejects(info, seg, end, window=8)                                         # a segment longer than the window
    e2 = end.copy(); e2[0, 5] = 0
    rejects(info, seg, e2)                                                    # padding
    s2 = seg.copy(); s2[0, 7, 3] = -0.0
    rejects(info, s2, end)                                                    # ... bit for bit
    i2 = info.copy(); i2["n_cells"] = 19
    rejects(i2, seg, end)
    i2 = info.copy(); i2["n_blocked"] = 1
    rejects(i2, seg, end)
    i2 = info.copy(); i2["truncated"] = 1
    rejects(i2, seg, end)
    # a shortcut through the wall: one segment from the first to the last cell, counted as unblocked
    i2 = info.copy(); i2["n_segments"] = 1
    e2 = np.full_like(end, -1); e2[0, 0] = 19
    s2 = np.zeros_like(seg); s2[0, 0, :4] = seg[0, 0, :4]; s2[0, 0, 4:] = seg[0, 1, 4:]
    rejects(i2, s2, e2)
    s2 = seg.copy(); s2[0, 0, 4] += F(0.01)                                   # a vertex off the path
    rejects(info, s2, end)


def test_dropin_class_offers_shorten_paths(dsp, tmp_path):
    """include/dsp_dynamic.h: shortenPaths type-checks and forwards to the C ABI"""
    src = tmp_path / "shorten.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n    int steps[2] = {3, -1}, cells[8] = {0, 1, 2, 3, -1, -1, -1, -1}, ends[6];\n'
                   "    dspmap_path_info info[2];\n    dspmap_segment seg[6];\n    dspmap_cast_hit hit[6];\n"
                   "    static_assert(sizeof(dspmap_path_info) == 16 && sizeof(dspmap_segment) == 32, \"layout\");\n"
                   "    int a = my_map.buildCastGrid(0.2f, 1);\n"
                   "    int c = my_map.shortenPaths(2, 4, steps, cells, 0.f, 0.1f, DSPMAP_SHORTEN_MAX_WINDOW, 3, info, seg, ends);\n"
                   "    int e = my_map.castSegments(6, seg, hit);\n"
                   "    return a + c + e + info[0].n_cells + info[0].n_segments + info[0].n_blocked + info[0].truncated + ends[0];\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert "dspmap_shorten_paths(h_" in open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
