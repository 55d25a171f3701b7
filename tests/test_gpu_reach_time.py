"""GPU tests of the space-time paths (dspmap_build_reach_timeline*, dspmap_get_reach_sets, dspmap_reach_last_steps,
dspmap_reach_timeline_paths*): bit parity -- zero mismatches in every word of every kept set, every uint16 of every field and every int of
every path -- with the numpy restatement (tests/reach_ref.py, tests/reach_time_ref.py) on hand-made grids fed by set_cast_grid: a door that
opens, time-invariant clutter (where the paths also equal dspmap_reach_paths), clutter that changes with every layer, a door that closes,
a front that is extinguished, shapes where the word logic can break, a shape whose sets do not fit in LDS; with and without
DSPMAP_REACH_WITH_CURRENT and with the wave sets in LDS and in device memory; max_len's edges; the device entry points enqueued right
behind a frame and the grid's build; read-only behaviour and the timeline's life cycle.  The restatement's checker runs on the DEVICE's
output."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reach_ref as R
from tests import reach_time_ref as TR
from tests.test_gpu_cast import SMALL, _median_threshold, _twins
from tests.test_gpu_query import _run, _scene_frames
from tests.test_gpu_reach import _assert_same_fields, _assert_same_paths, _blank_map, _grid_cells, _shift, _sources

pytestmark = pytest.mark.gpu
F = np.float32
U = R.UNREACHED
OK, E_STATE = 1, -3


def _expected_last(cfg, sets, sched):
    """per field, from the restatement's sets and the two exits the header states: the first step n >= 1 whose set is empty, or equals
    the one before while the layer never changes again; the list's last step otherwise.  (The restatement's own loop ends when EVERY
    field has stopped, so its length is the largest of these.)"""
    layers = R.schedule(cfg, sched["t_start"], sched.get("step_seconds", 0.0), sched["max_steps"])
    out = []
    for f in range(sets[0].shape[0]):
        last = len(sets) - 1
        for n in range(1, len(sets)):
            if not sets[n][f].any() or (np.array_equal(sets[n][f], sets[n - 1][f]) and (layers[n:] == layers[n]).all()):
                last = n
                break
        out.append(last)
    assert max(out) == len(sets) - 1
    return out


def _assert_same_sets(m, sets, nf, max_steps, tag, first=0):
    """reach_sets of every step first .. max_steps of every field against the restatement's, clamped past the early exit"""
    for f in range(nf):
        got = m.reach_sets(f, first, max_steps + 1 - first)
        want = R.pack(np.stack([TR.set_at(sets, n)[f] for n in range(first, max_steps + 1)]))
        assert got.dtype == np.uint64 and got.shape == want.shape, (tag, f)
        bad = np.argwhere(got != want)
        assert bad.shape[0] == 0, (tag, f, bad.shape[0], bad[:5])


def _timeline_case(m, lay, src, nf, starts, sched, max_len, wc=False, dev=False, tag="", sets_upto=None):
    """one timeline build held against the restatement: fields, last steps, sets (every step, or with sets_upto the steps 0 .. sets_upto
    and the last 3), paths, and the checker on the device's paths.  Returns (val, sets, steps, cells, complete, with a wait)."""
    cfg = m.cfg
    m.build_reach_fields(src, nf, with_current=wc, device_sets=dev, **sched)
    plain = m.reach_field(None, nf)
    assert m.reach_timeline_ptr() is None
    m.build_reach_timeline(src, nf, with_current=wc, device_sets=dev, **sched)
    assert m.reach_timeline_ptr() is not None and m.reach_fields_ptr() is not None
    val, sets = R.fields(cfg, lay, src, nf, with_current=wc, return_sets=True, **sched)
    got = m.reach_field(None, nf)
    _assert_same_fields(got, val, (tag, "fields"))
    assert np.array_equal(got, plain), (tag, "the plain build's fields")
    want_last = _expected_last(cfg, sets, sched)
    assert m.reach_last_steps(nf).tolist() == want_last, (tag, "last")
    if nf == 1:
        assert want_last == [len(sets) - 1]
    if sets_upto is None:
        _assert_same_sets(m, sets, nf, sched["max_steps"], tag)
    else:
        _assert_same_sets(m, sets, nf, sets_upto, tag)
        _assert_same_sets(m, sets, nf, sched["max_steps"], tag, sched["max_steps"] - 2)
    steps, cells = m.reach_timeline_paths(starts, max_len)
    _assert_same_paths((steps, cells), TR.timeline_paths(cfg, val, sets, starts, max_len), (tag, "paths"))
    done, waits = TR.check_timeline_paths(cfg, lay, src, nf, starts, steps, cells, with_current=wc, val=val, **sched)
    if R.time_invariant(cfg, sched["t_start"], sched.get("step_seconds", 0.0), sched["max_steps"]):
        _assert_same_paths((steps, cells), m.reach_paths(starts, max_len), (tag, "reach_paths"))
        assert waits == 0
    else:
        with pytest.raises(_error(), match="time-invariant"):
            m.reach_paths(starts, max_len)
    return val, sets, steps, cells, done, waits


def _error():
    import dsp_map_amd
    return dsp_map_amd.capi.DSPMapError


FLAG_COMBOS = ((False, False), (False, True), (True, False), (True, True))      # (with_current, device_sets)


@pytest.mark.parametrize("scene", ["door", "invariant", "clutter"])
def test_timeline_sets_fields_and_paths_bit_for_bit(dsp, scene):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    assert (cfg.nx, cfg.ny, cfg.nz, m.T) == (40, 40, 24, 6)
    if scene == "door":
        lay, src, nf, starts, sched = TR.opening_door_scene(cfg)
        scheds = [sched]
    elif scene == "invariant":
        lay, src, nf, starts, _ = TR.invariant_scene(cfg)
        scheds = [TR.STATIC, TR.FROZEN]
    else:
        lay, src, nf, starts, sched = TR.changing_clutter_scene(cfg)
        scheds = [sched]
    m.set_cast_grid(R.pack(lay))
    assert np.array_equal(_grid_cells(m), lay)
    for sched in scheds:
        for wc, dev in FLAG_COMBOS:
            val, sets, steps, cells, done, waits = _timeline_case(m, lay, src, nf, starts, sched, sched["max_steps"] + 1, wc, dev,
                                                                  (scene, sched["t_start"], wc, dev))
            assert m.reach_storage() == ((0, nf) if dev else (nf, 0))
            assert done == (steps >= 0).sum()
            if scene == "door" and not wc:
                assert steps.tolist()[:4] == [16, 11, 0, 4]
                assert (cells[0, :17] % 40).tolist() == [25, 24, 23, 22, 21, 20, 19, 19, 19, 19, 19, 19, 19, 18, 17, 16, 15]
            if scene == "door" and wc:                # layer 0 holds the door shut: with it the far side is never reached
                assert steps.tolist()[:4] == [-1, -1, 0, 4]
            if scene == "invariant":
                assert (steps >= 0).sum() >= 150
            if scene == "clutter" and not wc:
                assert (steps >= 0).sum() >= 100 and waits >= 10
    m.close()


def test_timeline_door_that_closes_at_horizon_2(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay = np.zeros((m.T + 1, cfg.nz, cfg.ny, cfg.nx), bool)
    lay[:, :, :, 20] = True
    lay[:3, 5, 10, 20] = False                    # open now and at horizons 0 and 1, closed from horizon 2 (step 11) on
    m.set_cast_grid(R.pack(lay))
    src = TR.at(cfg, (15, 10, 5, 0), (5, 10, 5, 1), (20, 10, 5, 2))
    starts = TR.at(cfg, (39, 10, 5, 0), (30, 30, 20, 0), (39, 10, 5, 1), (25, 10, 5, 1), (0, 10, 5, 2), (10, 10, 5, 0))
    val, sets, steps, cells, done, waits = _timeline_case(m, lay, src, 3, starts, TR.DOOR, 151, tag="closing door")
    door = (5 * cfg.ny + 10) * cfg.nx + 20
    for i in (0, 1):                              # field 0's far-side starts: through the door, at a step at which it is open
        v = int(steps[i])
        assert v > 10 and door in cells[i].tolist()
        assert v - cells[i].tolist().index(door) <= 10
    assert steps.tolist()[2:4] == [-1, -1] and (cells[2:4] == -1).all()      # field 1 comes too late: its far side is never reached
    assert steps[4] == 20 and steps[5] == 5 and done == 4
    m.close()


def test_timeline_front_extinguished_at_step_3(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay = np.zeros((m.T + 1, cfg.nz, cfg.ny, cfg.nx), bool)
    lay[2] = True                                 # horizon 1 blocks every cell; step 3 is the first in layer 2
    m.set_cast_grid(R.pack(lay))
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=4096)
    src = _sources(cfg, 40, 4, 3)
    near = np.argwhere(R.fields(cfg, lay, src, 4, **sched) <= 2)[::7]           # (field, z, y, x) of cells the front came to in time
    assert len(near) >= 12
    starts = np.concatenate([TR.at(cfg, *[(int(c[3]), int(c[2]), int(c[1]), int(c[0])) for c in near]), _sources(cfg, 300, 4, 9)])
    for dev in (False, True):
        val, sets, steps, cells, done, waits = _timeline_case(m, lay, src, 4, starts, sched, 8, dev=dev, tag=("extinguished", dev), sets_upto=8)
        assert len(sets) == 4 and not sets[3].any()
        assert m.reach_last_steps(4).tolist() == [3, 3, 3, 3]
        for f in range(4):
            assert not m.reach_sets(f, 3, 4094).any() and m.reach_sets(f, 2, 1).any()     # empty from step 3 to step 4096
        assert set(np.unique(steps).tolist()) == {-3, -2, -1, 0, 1, 2}                 # paths exist for the values 0 .. 2 only
    m.close()


SHAPES = {"65x6x3": dict(nx=65, ny=6, nz=3, res=0.15, ppv=12),
          "64x6x3": dict(nx=64, ny=6, nz=3, res=0.15, ppv=12),
          "132x40x12": dict(nx=132, ny=40, nz=12, res=0.15, ppv=9),
          "50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),
          "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=()),
          "8x128x80": dict(nx=8, ny=128, nz=80, res=0.15, ppv=9)}            # 163 840 bytes of sets: more than a workgroup's LDS
SHAPE_SCHED = dict(t_start=0.0, step_seconds=0.03, max_steps=100)              # 0 .. 3.0 s over 2.0 s of predictions: every layer, then the last


def _shape_scene(cfg, T):
    """a layer-dependent random clutter, three fields from cells free in every layer plus a mixed bag of sources, mixed starts"""
    rng = np.random.default_rng(4)
    lay = rng.random((T + 1, cfg.nz, cfg.ny, cfg.nx)) < 0.12
    free = np.argwhere(~lay.any(0))
    pick = free[rng.integers(0, len(free), 3)]
    src = np.concatenate([TR.at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k) for k, c in enumerate(pick)]), _sources(cfg, 20, 3, 11)])
    return lay, src, _sources(cfg, 150, 3, 12)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_timeline_awkward_shapes(dsp, shape):
    m = _blank_map(dsp, SHAPES[shape], seed=77)
    cfg = m.cfg
    assert m.T == (0 if shape == "t0" else 6)
    lay, src, starts = _shape_scene(cfg, m.T)
    if m.T:
        assert set(R.schedule(cfg, **SHAPE_SCHED).tolist()) == set(range(1, 7)) and (lay[1] != lay[m.T]).any()
    m.set_cast_grid(R.pack(lay))
    reached = 0
    for wc, dev in ((False, False), (True, True)):
        val, sets, steps, cells, done, waits = _timeline_case(m, lay, src, 3, starts, SHAPE_SCHED, 101, wc, dev, (shape, wc, dev))
        fits = 2 * 8 * cfg.nz * cfg.ny * ((cfg.nx + 63) // 64) <= 160 * 1024 - 256
        assert fits == (shape != "8x128x80")
        assert m.reach_storage() == ((3, 0) if fits and not dev else (0, 3))
        assert done == (steps >= 0).sum()
        reached += int((steps >= 0).sum())
    assert reached >= 10
    m.close()


def test_timeline_max_len_edges_and_truncated_rows(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay, src, nf, starts, sched = TR.changing_clutter_scene(cfg)
    m.set_cast_grid(R.pack(lay))
    m.build_reach_timeline(src, nf, **sched)
    val, sets = R.fields(cfg, lay, src, nf, return_sets=True, **sched)
    full = TR.timeline_paths(cfg, val, sets, starts, 121)
    v = int(np.median(full[0][full[0] > 0]))
    assert (full[0] > v).any() and (full[0] == v).any() and (full[0] < v).any()
    for max_len in (0, 1, v, v + 1, 121):
        steps, cells = m.reach_timeline_paths(starts, max_len)
        assert cells.shape == (len(starts), max_len)
        _assert_same_paths((steps, cells), (full[0], full[1][:, :max_len]), ("max_len", max_len))
        TR.check_timeline_paths(cfg, lay, src, nf, starts, steps, cells, val=val, **sched)
        longer = full[0] >= max_len                                           # truncated rows are full; the steps are not cut
        assert (cells[longer] >= 0).all() and np.array_equal(steps, full[0])
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    steps = np.zeros(len(starts), np.int32)
    assert m.L.dspmap_reach_timeline_paths(m.h, len(starts), p(starts), 0, 0, p(steps), None) == OK and np.array_equal(steps, full[0])
    assert m.L.dspmap_reach_timeline_paths(m.h, 0, None, 8, 0, None, None) == OK
    # dspmap_get_reach_sets: windows, and the argument errors that need a build
    one = m.reach_sets(2, 7, 3)
    assert np.array_equal(one, R.pack(np.stack([TR.set_at(sets, n)[2] for n in (7, 8, 9)])))
    assert np.array_equal(m.reach_sets(1, 120, 1), R.pack(TR.set_at(sets, 120)[1][None])) and m.reach_sets(0, 121, 0).shape[0] == 0
    assert np.array_equal(m.reach_sets(2, 118), R.pack(np.stack([TR.set_at(sets, n)[2] for n in (118, 119, 120)])))      # n_steps=None: the rest
    for bad in ((4, 0, 1), (0, 120, 2), (0, 121, 1), (0, 0, 122)):
        with pytest.raises(dsp.capi.DSPMapError):
            m.reach_sets(*bad)
    m.close()


def test_timeline_device_entry_points_stream_ordered_behind_frame(dsp):
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
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=120)
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(0.05, 1)                                        # no synchronisation between the frame, the builds and the paths
            m.build_reach_timeline(sd, 4, world=True, with_current=True, **sched)
            outs.append(m.reach_timeline_paths(td, 125, world=True))
        st.synchronize()
        assert m.reach_timeline_ptr() is not None
        dev_fields, dev_last = m.reach_field(None, 4), m.reach_last_steps(4)
        dev_sets = m.reach_sets(1, 0, 121)
        lay = _grid_cells(m)
        m.build_reach_timeline(src, 4, world=True, with_current=True, **sched)          # the host variant on the same grid
        host_fields, host_last = m.reach_field(None, 4), m.reach_last_steps(4)
        host_sets = m.reach_sets(1, 0, 121)
        host_paths = m.reach_timeline_paths(starts, 125, world=True)
        after = m.reach_timeline_paths(td, 125, world=True)
        st.synchronize()
    assert np.array_equal(dev_fields, host_fields) and np.array_equal(dev_last, host_last) and np.array_equal(dev_sets, host_sets)
    val, sets = R.fields(cfg, lay, src, 4, world=True, with_current=True, cur_pos=cur, return_sets=True, **sched)
    _assert_same_fields(host_fields, val, "device entry")
    assert not R.time_invariant(cfg, **sched)
    for k in range(2):
        assert outs[-1][k].dtype == torch.int32 and torch.equal(outs[-1][k], after[k])
        assert np.array_equal(after[k].cpu().numpy(), host_paths[k])
    assert not all(torch.equal(outs[0][k], outs[-1][k]) for k in range(2))
    _assert_same_paths(host_paths, TR.timeline_paths(cfg, val, sets, starts, 125, world=True, cur_pos=cur), "device paths")
    done, waits = TR.check_timeline_paths(cfg, lay, src, 4, starts, *host_paths, world=True, with_current=True, cur_pos=cur, val=val, **sched)
    assert done >= 1
    m.close()


def test_timeline_is_read_only_and_follows_the_fields(dsp):
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
    assert m.reach_timeline_ptr() is None
    grid, ptr = m.cast_grid(), m.cast_grid_ptr()
    lay = R.unpack(grid, cfg.nx)
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=120)
    # the twin builds the same grid and never builds a timeline: the map's results and the future grid are the same bits
    val, sets, steps, cells, done, waits = _timeline_case(m, lay, src, 3, starts, sched, 121, tag="read-only")
    assert m.cast_grid_ptr() == ptr and np.array_equal(m.cast_grid(), grid) and np.array_equal(twin.cast_grid(), grid)
    assert np.array_equal(m.results(), twin.results())
    fut = m.getFutureStatus()
    assert np.array_equal(fut, twin.getFutureStatus()) and (fut != 0).any()
    for x, y in zip(m.export_state(), twin.export_state()):
        assert np.array_equal(x, y)
    twin.close()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    words, last = np.zeros((1, cfg.nz, cfg.ny, 1), np.uint64), np.zeros(64, np.int32)
    so, co = np.zeros(len(starts), np.int32), np.zeros((len(starts), 20), np.int32)

    def stale():
        err = lambda: m.L.dspmap_last_error(m.h)   # noqa: E731
        assert m.reach_timeline_ptr() is None
        assert m.L.dspmap_get_reach_sets(m.h, 0, 0, 1, p(words)) == E_STATE and b"dspmap_build_reach_timeline" in err()
        assert m.L.dspmap_reach_last_steps(m.h, p(last)) == E_STATE and b"dspmap_build_reach_timeline" in err()
        assert m.L.dspmap_reach_timeline_paths(m.h, len(starts), p(starts), 20, 0, p(so), p(co)) == E_STATE
        assert b"dspmap_build_reach_timeline" in err() and not words.any() and not last.any() and not so.any() and not co.any()

    def fresh(same_grid):
        """a new build makes the timeline valid again, in the grid as it is now (getFutureStatus above was a consuming readout: a grid
        rebuilt from the map has other predicted layers than the one the first build saw)"""
        m.build_reach_timeline(src, 3, **sched)
        assert m.reach_timeline_ptr() is not None
        got = m.reach_timeline_paths(starts, 121)
        if same_grid:
            _assert_same_paths(got, (steps, cells), "rebuilt")
        else:
            v2, s2 = R.fields(cfg, _grid_cells(m), src, 3, return_sets=True, **sched)
            _assert_same_paths(got, TR.timeline_paths(cfg, v2, s2, starts, 121), "rebuilt in the new grid")

    # a plain build replaces the fields the timeline belongs to (the fields themselves stay readable)
    m.build_reach_fields(src, 3, **sched)
    stale()
    assert m.reach_fields_ptr() is not None and np.array_equal(m.reach_field(None, 3), val)
    fresh(True)
    m.build_cast_grid(thr, 1)
    stale()
    fresh(False)
    m.set_cast_grid(grid)
    stale()
    fresh(True)
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    stale()
    assert m.L.dspmap_build_reach_timeline(m.h, 3, len(src), p(src), 0.0, 0.02, 120, 0) == E_STATE
    assert b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    m.close()
