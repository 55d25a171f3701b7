"""GPU tests of the arrival-time fields grown through the cast grid (dspmap_build_reach_fields*, dspmap_reach_paths*): bit parity -- zero
mismatches in every uint16 of every field and in every int of every path -- with the numpy restatement (tests/reach_ref.py) fed with the
grid the map hands out AFTER the build or after set_cast_grid (m.cast_grid()), over storage orders, inflation radii, field counts,
schedules, both flags and both homes of the wave sets; hand-made mazes, closing doors and extinguished fronts; awkward shapes; a shape
whose sets do not fit in LDS; the device entry points enqueued right behind the frame and the build; read-only behaviour and the
snapshot's life cycle.  The restatement's checkers run on the DEVICE's output."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import reach_ref as R
from tests.test_gpu_cast import SMALL, _median_threshold, _twins
from tests.test_gpu_query import _run, _scene_frames

pytestmark = pytest.mark.gpu
F = np.float32
U = R.UNREACHED
OK, E_STATE = 1, -3


def _sources(cfg, n, n_fields, seed):
    """n points {x, y, z, field}: random ones inside the map, some just outside, some on its faces, NaN and inf entries, fields from
    -1 to n_fields (both ends invalid); the first n_fields points are inside and name each field once"""
    rng = np.random.default_rng(seed)
    half = np.array(common.half_extent(cfg), F)
    p = (rng.uniform(-1.04, 1.04, (n, 3)) * half).astype(F)
    p[:n_fields] = (rng.uniform(-0.9, 0.9, (min(n, n_fields), 3)) * half).astype(F)
    face = rng.random(n) < 0.05
    face[:n_fields] = False
    p[face, 0] = np.where(rng.random(face.sum()) < 0.5, half[0], -half[0])
    bad = rng.random((n, 3)) < 0.01
    bad[:n_fields] = False
    p[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), bad.sum())
    out = np.zeros(n, R.POINT_DTYPE)
    out["x"], out["y"], out["z"] = p[:, 0], p[:, 1], p[:, 2]
    out["field"] = rng.integers(-1, n_fields + 1, n)
    out["field"][:n_fields] = np.arange(min(n, n_fields))
    return out


def _shift(pts, cur):
    s = pts.copy()
    for k, a in enumerate("xyz"):
        s[a] = (s[a] + cur[k]).astype(F)
    return s


def _grid_cells(m):
    """the bool cells [L, nz, ny, nx] of the grid the map holds now"""
    return R.unpack(m.cast_grid(), m.cfg.nx)


def _assert_same_fields(got, want, tag):
    assert got.dtype == want.dtype == np.uint16 and got.shape == want.shape, tag
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


def _assert_same_paths(got, want, tag):
    for g, w, name in zip(got, want, ("steps", "cells")):
        g = np.asarray(g)
        assert g.dtype == np.int32 and g.shape == w.shape, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (tag, name, bad.shape[0], bad[:5])


def _manhattan_to_sources(cfg, src, n_fields):
    """int [n_fields, nz, ny, nx]: the Manhattan distance to the nearest valid source cell of the field (a large number without one)"""
    finite, inside, ijk = R.point_cells(cfg, src)
    z, y, x = np.meshgrid(np.arange(cfg.nz), np.arange(cfg.ny), np.arange(cfg.nx), indexing="ij")
    out = np.full((n_fields, cfg.nz, cfg.ny, cfg.nx), 1 << 20, np.int64)
    for i in np.flatnonzero(inside & (src["field"] >= 0) & (src["field"] < n_fields)):
        f = src["field"][i]
        out[f] = np.minimum(out[f], np.abs(x - ijk[i, 0]) + np.abs(y - ijk[i, 1]) + np.abs(z - ijk[i, 2]))
    return out


def _blank_map(dsp, kw, seed=5):
    """a map that never saw a frame, with a valid (empty) cast grid for set_cast_grid to replace"""
    m = dsp.DSPMap(dsp.make_config(seed=seed, **kw))
    m.build_cast_grid(1e9, 0)
    return m


def _centre(cfg, x, y, z):
    res = cfg.voxel_resolution
    return (-0.5 * res * cfg.nx + res * (x + 0.5), -0.5 * res * cfg.ny + res * (y + 0.5), -0.5 * res * cfg.nz + res * (z + 0.5))


def _at(cfg, *cells):
    """sources / starts at the centres of cells (x, y, z[, field])"""
    return R.points([_centre(cfg, *c[:3]) + ((c[3] if len(c) > 3 else 0),) for c in cells])


# the schedules of the scene tests: static on the current layer; step_seconds = 0 inside a predicted layer (time-invariant); one that spans
# all horizons (0 .. 2.4 s over 2.0 s of predictions: the tested layer changes five times, then stays)
STATIC = dict(t_start=-1.0, step_seconds=0.0, max_steps=200)
FROZEN = dict(t_start=0.3, step_seconds=0.0, max_steps=200)
SPAN = dict(t_start=0.0, step_seconds=0.02, max_steps=120)
CUT = dict(t_start=-1.0, step_seconds=0.0, max_steps=17)


def _free_sources(cfg, lay, n_fields, seed, per_field=2):
    """sources for a scene grid: per field `per_field` centres of cells that are free in every layer (so that no schedule blocks a field at
    step 0), followed by the mixed bag of _sources (valid extras, points outside, NaN, fields out of range)"""
    rng = np.random.default_rng(seed)
    cand = np.argwhere(~lay.any(0))                                           # (z, y, x)
    assert len(cand) >= 50, "the grid leaves no cell free in every layer"
    pick = cand[rng.integers(0, len(cand), n_fields * per_field)]
    mine = _at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k % n_fields) for k, c in enumerate(pick)])
    return np.concatenate([mine, _sources(cfg, 6 * n_fields + 5, n_fields, seed + 1)])


def _scene_threshold(m):
    """a threshold at which inflation by 2 still leaves room: the first quantile of the positive masses for which at least 3 % of the
    cells are free in every layer of the grid inflated by 2 (the last candidate otherwise: the test's own conditions then say what is wrong)"""
    mass = m.results()[:, 0]
    assert (mass > 0).any()
    for q in (0.5, 0.8, 0.95, 0.99, 0.999):
        thr = float(np.quantile(mass[mass > 0], q))
        m.build_cast_grid(thr, 2)
        lay = _grid_cells(m)
        free = float((~lay.any(0)).mean())
        print("threshold quantile", q, thr, "occupied per layer", lay.mean((1, 2, 3)).round(3).tolist(), "free in every layer", round(free, 4))
        if free >= 0.03:
            break
    return thr


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_reach_bit_parity_on_scene_grids(dsp, variant):
    kw = dict(SMALL)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    assert np.abs(cur).max() > 0 and int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    thr = _scene_threshold(m)
    assert R.schedule(cfg, **SPAN).tolist()[0] == 1 and set(R.schedule(cfg, **SPAN).tolist()) == set(range(1, m.T + 1))
    assert R.time_invariant(cfg, **STATIC) and R.time_invariant(cfg, **FROZEN) and not R.time_invariant(cfg, **SPAN)
    # (n_fields, schedule, world, with_current, device_sets): every field count, schedule and flag, LDS against device sets on equal input
    combos = ((1, STATIC, False, False, False), (1, STATIC, False, False, True), (3, SPAN, False, False, False), (3, SPAN, False, False, True),
              (3, SPAN, True, True, False), (3, FROZEN, True, False, False), (3, FROZEN, False, True, True), (1, CUT, False, False, False),
              (64, STATIC, True, False, False), (64, SPAN, False, True, True))
    answers = {}
    detour = differs = far = complete = 0
    for r in (0, 2):
        m.build_cast_grid(thr, r)
        lay = _grid_cells(m)                                                  # read after the build: what the kernel grows in
        assert lay.any() and not lay.all() and (lay[1] != lay[m.T]).any() and (lay[0] != lay[1]).any()      # the layers differ
        src = {nf: _free_sources(cfg, lay, nf, 7 + nf) for nf in (1, 3, 64)}
        for nf, sched, world, wc, dev in combos:
            if nf == 64 and r == 0:                                           # (64 fields on one of the two grids)
                continue
            s = _shift(src[nf], cur) if world else src[nf]
            m.build_reach_fields(s, nf, world=world, with_current=wc, device_sets=dev, **sched)
            assert m.reach_storage() == ((0, nf) if dev else (nf, 0))
            got = m.reach_field(None, nf)
            key = (r, nf, sched["t_start"], sched["max_steps"], world, wc)
            if key in answers:                                                # the other home of the wave sets: the same words
                want = answers[key]
            else:
                want = answers[key] = R.fields(cfg, lay, s, nf, world=world, with_current=wc, cur_pos=cur, **sched)
            _assert_same_fields(got, want, (variant, r, nf, sched, world, wc, dev))
            # the input is not degenerate -- conditions on the restatement's own output
            assert (want == U).any() and all((w == 0).any() for w in want), "unreached cells exist, and every field starts"
            far += int(((want != U) & (want > 3)).sum())
            if sched is STATIC and not world:
                man = _manhattan_to_sources(cfg, s, nf)
                detour += int(((want != U) & (want > man)).sum())             # a value above the Manhattan distance: the front went round
            if nf <= 3 and not dev:                                           # the independent checkers on the DEVICE's output
                assert R.check_free(cfg, lay, got, with_current=wc, **sched) >= nf
                R.check_predecessors(cfg, lay, got, s, world=world, with_current=wc, cur_pos=cur, **sched)
            if R.time_invariant(cfg, **sched) and not dev:
                starts = _free_sources(cfg, lay, nf, 99, per_field=40 if nf <= 3 else 2)
                starts = np.concatenate([starts, R.points([(1000.0, 0.0, 0.0, 0), (np.nan, 0.0, 0.0, 0), (0.0, 0.0, 0.0, -1)])])
                starts = _shift(starts, cur) if world else starts
                steps, cells = m.reach_paths(starts, 150, world=world)
                _assert_same_paths((steps, cells), R.paths(cfg, want, starts, 150, world=world, cur_pos=cur), (variant, r, nf, sched))
                complete += R.check_paths(cfg, got, starts, steps, cells, world=world, cur_pos=cur)
                assert set(np.unique(steps[steps < 0]).tolist()) >= {-2, -3}
        a, b = answers[(r, 3, 0.0, 120, False, False)], R.fields(cfg, lay, src[3], 3, **dict(STATIC, max_steps=120))
        differs += int((a != b).sum())                                        # the schedule changes answers
    print("reached beyond 3 steps", far, "above Manhattan", detour, "static != scheduled", differs, "complete paths", complete)
    assert far >= 100 and detour >= 1 and differs >= 1 and complete >= 10
    cutv, full = answers[(2, 1, -1.0, 17, False, False)], answers[(2, 1, -1.0, 200, False, False)]
    assert np.array_equal(cutv, np.where(full <= 17, full, U)) and (cutv == 17).any() == (full == 17).any()
    m.close()


def _serpentine(cfg):
    """bool [nz, ny, nx]: everything blocked but the plane z = 0, where the even rows are free lanes and the odd rows walls with one gap, at
    x = nx - 1 and x = 0 in turn: one path through all lanes"""
    b = np.ones((cfg.nz, cfg.ny, cfg.nx), bool)
    b[0, 0::2, :] = False
    for k, y in enumerate(range(1, cfg.ny - 1, 2)):
        b[0, y, cfg.nx - 1 if k % 2 == 0 else 0] = False
    return b


def test_reach_serpentine_maze_of_more_than_700_steps(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    maze = _serpentine(cfg)
    lay = np.repeat(maze[None], m.T + 1, 0)
    m.set_cast_grid(R.pack(lay))
    assert np.array_equal(_grid_cells(m), lay) and m.cast_grid_ptr() is not None
    lanes = cfg.ny // 2
    far = (cfg.nx - 1 if lanes % 2 == 1 else 0, 2 * (lanes - 1), 0)
    length = lanes * (cfg.nx - 1) + 2 * (lanes - 1)
    assert length > 700
    src = _at(cfg, (0, 0, 0), (far[0], far[1], far[2], 1))                    # field 0 from the near end, field 1 from the far end
    for max_steps, dev in ((length + 50, False), (500, True), (length, False), (length - 1, True)):
        m.build_reach_fields(src, 2, max_steps=max_steps, device_sets=dev)
        got = m.reach_field(None, 2)
        want = R.fields(cfg, lay, src, 2, max_steps=max_steps)
        _assert_same_fields(got, want, ("maze", max_steps, dev))
        end = int(got[0][far[2], far[1], far[0]])
        assert end == (length if max_steps >= length else U) and (got[0] != U).sum() == min(max_steps, length) + 1
        assert got[1][0, 0, 0] == end and got[0].max() == U
        starts = _at(cfg, far, (0, 0, 0, 1), (5, 1, 0), (3, 3, 3))            # the far end, the near end down field 1, two walled-in cells
        steps, cells = m.reach_paths(starts, length + 1)
        _assert_same_paths((steps, cells), R.paths(cfg, want, starts, length + 1), ("maze paths", max_steps))
        assert steps.tolist() == ([length, length, -1, -1] if max_steps >= length else [-1, -1, -1, -1])
        if max_steps >= length:
            assert R.check_paths(cfg, got, starts, steps, cells) == 2
            g0 = lambda c: (c[2] * cfg.ny + c[1]) * cfg.nx + c[0]   # noqa: E731
            assert cells[0, 0] == g0(far) and cells[0, length] == 0 and cells[1, 0] == 0 and cells[1, length] == g0(far)
            short = m.reach_paths(starts, 100)                                # max_len cuts the path, not the steps
            assert short[0].tolist() == steps.tolist() and np.array_equal(short[1][:2], cells[:2, :100])
    R.check_free(cfg, lay, got, max_steps=length - 1)
    R.check_predecessors(cfg, lay, got, src, max_steps=length - 1)
    m.close()


def test_reach_door_that_closes_at_horizon_2(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay = np.zeros((m.T + 1, cfg.nz, cfg.ny, cfg.nx), bool)
    lay[:, :, :, 20] = True                       # a wall at x = 20 in every layer ...
    door = (20, 10, 5)
    lay[:3, door[2], door[1], door[0]] = False    # ... with a door that is open now and at horizons 0 and 1, closed from horizon 2 on
    m.set_cast_grid(R.pack(lay))
    sched = dict(t_start=0.0, step_seconds=0.019, max_steps=150)              # horizon 2 (layer 3) from step 11 on: t_10 = 0.19, t_11 = 0.209 > 0.2
    assert R.schedule(cfg, **sched).tolist()[9:12] == [2, 2, 3]
    src = _at(cfg, (15, 10, 5, 0), (5, 10, 5, 1), (20, 10, 5, 2))             # 5 steps from the door, 15 steps from it, inside it
    m.build_reach_fields(src, 3, **sched)
    got = m.reach_field(None, 3)
    _assert_same_fields(got, R.fields(cfg, lay, src, 3, **sched), "door")
    assert got[0][5, 10, 20] == 5 and got[0][5, 10, 39] == 24 and (got[0][:, :, 21:] != U).all()      # through in time: the far side fills
    assert (got[1][:, :, 20:] == U).all() and (got[1][:, :, :20] != U).all()                          # too late: never through
    assert got[2][5, 10, 20] == 0 and got[2][5, 10, 0] == 20                  # the door cell itself is removed at step 11; both sides were left before
    R.check_free(cfg, lay, got, **sched)
    R.check_predecessors(cfg, lay, got, src, **sched)
    # the same door seen statically: open on layer 0, shut on the last horizon
    for t0, through in ((-1.0, True), (5.0, False)):
        m.build_reach_fields(src[:2], 2, t_start=t0, max_steps=150)
        st = m.reach_field(None, 2)
        _assert_same_fields(st, R.fields(cfg, lay, src[:2], 2, t_start=t0, max_steps=150), ("door static", t0))
        assert bool((st[1][:, :, 21:] != U).any()) == through
    m.close()


def test_reach_front_extinguished_at_step_3(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay = np.zeros((m.T + 1, cfg.nz, cfg.ny, cfg.nx), bool)
    lay[2] = True                                 # horizon 1 blocks every cell; before and after it the map is free
    m.set_cast_grid(R.pack(lay))
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=4096)              # t_3 = 0.06 > 0.05: step 3 is the first in layer 2
    assert R.schedule(cfg, **sched).tolist()[:4] == [1, 1, 1, 2] and R.schedule(cfg, **sched)[-1] == m.T
    src = _sources(cfg, 40, 4, 3)
    for dev in (False, True):
        m.build_reach_fields(src, 4, device_sets=dev, **sched)
        got = m.reach_field(None, 4)
        _assert_same_fields(got, R.fields(cfg, lay, src, 4, **sched), ("extinguished", dev))
        assert set(np.unique(got).tolist()) == {0, 1, 2, U}                   # nothing is reached once the front is gone, free as the map is
    with pytest.raises(dsp.capi.DSPMapError, match="time-invariant"):
        m.reach_paths(src, 8)
    m.close()


SHAPES = {"132x40x12": dict(nx=132, ny=40, nz=12, res=0.15, ppv=9),           # three words per row: fronts across both word boundaries
          "50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),            # no multiple of 64 anywhere
          "64x6x3": dict(nx=64, ny=6, nz=3, res=0.15, ppv=12),                # the word edge exactly ...
          "65x6x3": dict(nx=65, ny=6, nz=3, res=0.15, ppv=12),                # ... and one bit past it
          "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=())}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reach_awkward_shapes(dsp, shape):
    kw = SHAPES[shape]
    cfg = dsp.make_config(seed=77, **kw)
    m = dsp.DSPMap(cfg)
    scene = shape in ("132x40x12", "50x37x23", "t0")
    if scene:
        m.seed_uniform(2, 0.01, 5, vmax=1.0)
        _run(m, _scene_frames(dsp, kw, 8, seed=31))
    assert m.T == (0 if shape == "t0" else 6)
    src = _sources(cfg, 30, 3, 11)
    sched = dict(t_start=0.0, step_seconds=0.03, max_steps=250)
    rng = np.random.default_rng(4)
    grids = [("median", 1), (1e9, 0), (0.0, 0)] if scene else [(1e9, 0), ("random", 0)]
    for thr, r in grids:
        m.build_cast_grid(_median_threshold(m) if thr == "median" else (1e9 if thr == "random" else thr), r)
        if thr == "random":                      # a map too small for the scene: hand-made layers, a different one per horizon
            m.set_cast_grid(R.pack(rng.random((m.T + 1, cfg.nz, cfg.ny, cfg.nx)) < 0.25))
        lay = _grid_cells(m)
        assert lay.any() == (thr != 1e9)
        for wc, kws in ((False, sched), (True, sched), (False, dict(t_start=-1.0, max_steps=250))):
            m.build_reach_fields(src, 3, with_current=wc, **kws)
            got = m.reach_field(None, 3)
            _assert_same_fields(got, R.fields(cfg, lay, src, 3, with_current=wc, **kws), (shape, thr, wc, kws))
            R.check_free(cfg, lay, got, with_current=wc, **kws)
            R.check_predecessors(cfg, lay, got, src, with_current=wc, **kws)
        steps, cells = m.reach_paths(src, 64)                                 # (the last build is static)
        _assert_same_paths((steps, cells), R.paths(cfg, got, src, 64), (shape, thr))
        R.check_paths(cfg, got, src, steps, cells)
        if thr == 1e9:                           # an empty grid: the Manhattan distance, across every word boundary of a row
            man = _manhattan_to_sources(cfg, src, 3)
            assert np.array_equal(got.astype(np.int64), np.where(man <= 250, man, U))
            if cfg.nx > 64:
                one = _at(cfg, (3, 2, 0))
                m.build_reach_fields(one, 1, max_steps=250)
                row = m.reach_field(0)[0, 2]
                assert row.tolist() == [abs(x - 3) for x in range(cfg.nx)]
                one = _at(cfg, (cfg.nx - 1, 2, 0))
                m.build_reach_fields(one, 1, max_steps=250)
                assert m.reach_field(0)[0, 2].tolist() == [cfg.nx - 1 - x for x in range(cfg.nx)]
        if thr == 0.0:
            assert lay[0].mean() > 0.05                                       # dense: wherever a particle lives
    m.close()


def test_reach_sets_that_do_not_fit_in_lds(dsp):
    """the two wave sets take 2 * nz * ny * W * 8 bytes of the 160 KiB - 256 B a workgroup is given: 8 x 128 x 80 needs 163 840 bytes, the
    smallest multiple of 128 rows above the budget of 10 224 words per set"""
    kw = dict(nx=8, ny=128, nz=80, res=0.15, ppv=9)
    assert 2 * 8 * 128 * 80 > 160 * 1024 - 256 >= 2 * 8 * 128 * 79
    m = _blank_map(dsp, kw)
    cfg = m.cfg
    rng = np.random.default_rng(8)
    lay = rng.random((m.T + 1, cfg.nz, cfg.ny, cfg.nx)) < 0.3
    lay[0] = lay[1]
    m.set_cast_grid(R.pack(lay))                                              # filled with set_cast_grid alone: no frame ever ran
    src = _sources(cfg, 40, 2, 5)
    for kws in (dict(t_start=-1.0, max_steps=400), dict(t_start=0.0, step_seconds=0.02, max_steps=300, with_current=True)):
        m.build_reach_fields(src, 2, **kws)
        assert m.reach_storage() == (0, 2)
        got = m.reach_field(None, 2)
        _assert_same_fields(got, R.fields(cfg, lay, src, 2, **kws), ("device sets", kws))
        assert (got != U).sum() > 10000 and (got == U).any()
        R.check_free(cfg, lay, got, **kws)
        R.check_predecessors(cfg, lay, got, src, **kws)
    m.close()
    small = _blank_map(dsp, dict(SMALL))
    small.build_reach_fields(_sources(small.cfg, 10, 5, 1), 5, max_steps=10)
    assert small.reach_storage() == (5, 0)
    small.build_reach_fields(_sources(small.cfg, 10, 5, 1), 5, max_steps=10, device_sets=True)
    assert small.reach_storage() == (0, 5)
    small.close()


def test_reach_device_entry_points_stream_ordered_behind_frame(dsp):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    (m,) = _twins(dsp, kw, 1)
    cfg = m.cfg
    cur = np.array(frames[-1][1], F)
    src = _shift(_sources(cfg, 400, 4, 13), cur)
    starts = _shift(_sources(cfg, 500, 4, 14), cur)
    wide = torch.from_numpy(np.concatenate([src.view(np.int32).reshape(-1, 4)] * 2, 1)).cuda()
    sd = wide[:, :4]                                                          # a non-contiguous view: the binding's temporary
    td = torch.from_numpy(starts.view(np.int32).reshape(-1, 4).copy()).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(0.05, 1)                                        # no synchronisation between the frame, the builds and the paths
            m.build_reach_fields(sd, 4, world=True, with_current=True, max_steps=120)
            outs.append(m.reach_paths(td, 130, world=True))
        st.synchronize()
        ptr = m.reach_fields_ptr()
        assert ptr is not None
        dev_fields = m.reach_field(None, 4)                                   # what the device entry point left behind the last frame
        lay = _grid_cells(m)
        m.build_reach_fields(src, 4, world=True, with_current=True, max_steps=120)      # the host variant on the same grid
        host_fields = m.reach_field(None, 4)
        host_paths = m.reach_paths(starts, 130, world=True)
        after = m.reach_paths(td, 130, world=True)
        st.synchronize()
    assert np.array_equal(dev_fields, host_fields)
    want = R.fields(cfg, lay, src, 4, world=True, with_current=True, cur_pos=cur, max_steps=120)
    _assert_same_fields(host_fields, want, "device entry")
    for k in range(2):
        assert outs[-1][k].dtype == torch.int32 and torch.equal(outs[-1][k], after[k])
        assert np.array_equal(after[k].cpu().numpy(), host_paths[k])
    assert not all(torch.equal(outs[0][k], outs[-1][k]) for k in range(2))
    _assert_same_paths(host_paths, R.paths(cfg, want, starts, 130, world=True, cur_pos=cur), "device paths")
    assert R.check_paths(cfg, host_fields, starts, host_paths[0], host_paths[1], world=True, cur_pos=cur) >= 1
    m.close()


def test_reach_is_read_only_and_follows_the_grid(dsp):
    kw = dict(SMALL)
    m, twin = _twins(dsp, kw)
    frames = _scene_frames(dsp, kw, 7, seed=31)
    for x in (m, twin):
        _run(x, frames[:6])
    thr = _median_threshold(m)
    cfg = m.cfg
    src, starts = _sources(cfg, 400, 3, 3), _sources(cfg, 300, 3, 4)
    for x in (m, twin):
        x.build_cast_grid(thr, 1)
    assert m.reach_fields_ptr() is None
    grid, ptr = m.cast_grid(), m.cast_grid_ptr()
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=120)
    m.build_reach_fields(src, 3, **sched)                                     # the twin builds the same grid and never grows a field
    scheduled = m.reach_field(None, 3)
    with pytest.raises(dsp.capi.DSPMapError, match="time-invariant"):         # a scheduled build has no paths
        m.reach_paths(starts, 50)
    steps, cells = np.zeros(len(starts), np.int32), np.zeros((len(starts), 50), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert m.L.dspmap_reach_paths(m.h, len(starts), p(starts), 50, 0, p(steps), p(cells)) == E_STATE and not steps.any() and not cells.any()
    m.build_reach_fields(torch.from_numpy(src.view(np.int32).reshape(-1, 4).copy()).cuda(), 3, max_steps=120, with_current=True, device_sets=True)
    torch.cuda.synchronize()
    static = m.reach_field(None, 3)
    paths0 = m.reach_paths(starts, 50)
    # the grid's words are identical before and after the builds and the paths, and the grid is still valid ...
    assert m.cast_grid_ptr() == ptr and np.array_equal(m.cast_grid(), grid) and np.array_equal(twin.cast_grid(), grid)
    lay = R.unpack(grid, cfg.nx)
    _assert_same_fields(scheduled, R.fields(cfg, lay, src, 3, **sched), "read-only scheduled")
    _assert_same_fields(static, R.fields(cfg, lay, src, 3, max_steps=120), "read-only static")
    R.check_free(cfg, lay, scheduled, **sched)
    R.check_predecessors(cfg, lay, scheduled, src, **sched)
    assert R.check_paths(cfg, static, starts, *paths0) >= 1
    # ... and so is what the map hands out (getFutureStatus is a consuming readout: the twin's is the "before")
    assert np.array_equal(m.results(), twin.results())
    fut = m.getFutureStatus()
    assert np.array_equal(fut, twin.getFutureStatus()) and (fut != 0).any()
    for x, y in zip(m.export_state(), twin.export_state()):
        assert np.array_equal(x, y)
    twin.close()
    out = np.zeros(m.V, np.uint16)

    def stale():
        assert m.reach_fields_ptr() is None
        assert m.L.dspmap_get_reach_field(m.h, 0, p(out)) == E_STATE and b"dspmap_build_reach_fields" in m.L.dspmap_last_error(m.h)
        assert m.L.dspmap_reach_paths(m.h, len(starts), p(starts), 50, 0, p(steps), p(cells)) == E_STATE
        assert b"dspmap_build_reach_fields" in m.L.dspmap_last_error(m.h) and not out.any() and not steps.any()

    # a rebuild of the grid makes the snapshot stale, and a build of the fields makes it valid again
    m.build_cast_grid(thr, 1)
    stale()
    m.build_reach_fields(src, 3, max_steps=120)
    assert m.reach_fields_ptr() is not None and np.array_equal(m.reach_field(None, 3), static)
    # ... so does set_cast_grid (the grid stays valid)
    m.set_cast_grid(grid)
    stale()
    assert m.cast_grid_ptr() == ptr
    m.build_reach_fields(src, 3, max_steps=120)
    assert np.array_equal(m.reach_field(None, 3), static)
    with pytest.raises(dsp.capi.DSPMapError):
        m.reach_field(3)                                                      # a field the last build did not grow
    # ... and so does the next frame, which takes the grid with it
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    stale()
    assert m.L.dspmap_build_reach_fields(m.h, 3, len(src), p(src), -1.0, 0.0, 120, 0) == E_STATE
    assert b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    m.build_cast_grid(thr, 1)
    stale()
    m.build_reach_fields(src, 3, max_steps=120)
    again = m.reach_field(None, 3)
    _assert_same_fields(again, R.fields(cfg, _grid_cells(m), src, 3, max_steps=120), "rebuilt")
    assert (again != static).any()
    m.close()
