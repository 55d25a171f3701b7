"""GPU tests of the clearance-weighted cost-to-go fields (dspmap_build_cost_fields*, dspmap_cost_paths*): bit parity -- zero mismatches in
every uint16 of the fields, every weight byte and every int of the paths -- with the numpy restatement tests/cost_ref.py, which is always
fed with what the map hands back (cast_grid(), distance_field(), cost_weights()); the header's known answer; the n_bands == 0 identity with
the static arrival fields; max_cost cuts; levels that stay empty in front of a heavy cell; a real scene with the chain paths -> shorten ->
casts; the device entry points behind a frame; and the life cycle of the snapshot."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cast_ref as CR
from tests import cost_ref as K
from tests import reach_ref as R
from tests.test_gpu_cast import SMALL, _median_threshold, _twins
from tests.test_gpu_query import _run, _scene_frames
from tests.test_gpu_reach import SHAPES, _at, _blank_map, _grid_cells, _scene_threshold, _shift, _sources

pytestmark = pytest.mark.gpu
F = np.float32
U = K.UNREACHED
OK, E_STATE = 1, -3
BANDS = {1: [(0.5, 3)],                                        # weights {1, 4}
         3: [(0.3, 1), (0.6, 2), (0.8, 1)],                    # nested: {1, 2, 4, 5}
         4: [(0.2, 1), (0.4, 2), (0.6, 1), (0.8, 3)]}          # a total of exactly 8: {1, 4, 5, 7, 8}
OCCUR = {1: {1, 4}, 3: {1, 2, 4, 5}, 4: {1, 4, 5, 7, 8}}


def _cost_map(dsp, kw, lay, dist, seed=5):
    """a map that never saw a frame whose cast grid and distance field are the caller's: bool [L, nz, ny, nx] and float32 of that shape"""
    m = _blank_map(dsp, kw, seed)
    m.set_cast_grid(R.pack(lay))
    m.build_distance_field(1e9, 4)
    m.set_distance_field(dist)
    return m


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


def _parity(m, src, nf, t, bands, max_cost, world, cur, starts, max_len, tag):
    """one build and its paths against the restatement, fed with what the map hands back; the checkers on the device's output.
    Returns (fields, weights, cost, cells) of the device"""
    cfg = m.cfg
    l = K.layer_of(cfg, t)
    lay, dist = _grid_cells(m)[l], m.distance_field(l)
    m.build_cost_fields(src, nf, t=t, bands=bands, max_cost=max_cost, world=world)
    assert m.cost_fields_ptr() is not None
    w, got = m.cost_weights(), m.cost_field(None, nf)
    _same(w, K.weights(lay, dist, bands), (tag, "weights"))
    want = K.fields(cfg, w, src, nf, max_cost=max_cost, world=world, cur_pos=cur)
    _same(got, want, (tag, "fields"))
    K.check_fields(cfg, w, got, src, max_cost=max_cost, world=world, cur_pos=cur)
    cost, cells = m.cost_paths(starts, max_len, world=world)
    wc, wp = K.paths(cfg, want, w, starts, max_len, world=world, cur_pos=cur)
    _same(cost, wc, (tag, "cost"))
    _same(cells, wp, (tag, "cells"))
    K.check_paths(cfg, got, w, starts, cost, cells, world=world, cur_pos=cur)
    return got, w, cost, cells


def test_cost_known_answer_10x3x1(dsp):
    """the header's example, int for int: fields, weights and the path that leaves the penalised row"""
    kw = dict(nx=10, ny=3, nz=1, res=0.15, ppv=12)
    cfg = dsp.make_config(seed=5, **kw)
    L = cfg.prediction_times + 1
    dist = np.full((L, 1, 3, 10), 1.0, F)
    dist[:, 0, 0] = 0.05
    m = _cost_map(dsp, kw, np.zeros((L, 1, 3, 10), bool), dist)
    src, start = _at(cfg, (0, 0, 0)), _at(cfg, (9, 0, 0))
    m.build_cost_fields(src, bands=[(0.1, 4)], max_cost=100)
    val, w = m.cost_field(0), m.cost_weights()
    assert w.dtype == np.uint8 and w[0].tolist() == [[5] * 10, [1] * 10, [1] * 10]
    assert val.dtype == np.uint16 and val[0].tolist() == [[0, 5, 8, 9, 10, 11, 12, 13, 14, 15], list(range(1, 11)), list(range(2, 12))]
    cost, cells = m.cost_paths(start, 16)
    assert cost.tolist() == [15] and cells[0].tolist() == [9, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 0, -1, -1, -1, -1]
    m.build_cost_fields(src, max_cost=100)                                    # unweighted: 9 at (9, 0, 0), the path stays in row 0
    assert m.cost_weights()[0].tolist() == [[1] * 10] * 3 and m.cost_field(0)[0, 0].tolist() == list(range(10))
    cost, cells = m.cost_paths(start, 16)
    assert cost.tolist() == [9] and cells[0, :10].tolist() == list(range(9, -1, -1)) and (cells[0, 10:] == -1).all()
    m.close()


def test_cost_without_bands_is_the_static_reach_field(dsp):
    """bands=(): uint16 for uint16 the static arrival fields of the same grid with max_steps = max_cost, and the same paths"""
    kw = dict(SMALL)
    m = _blank_map(dsp, kw)
    cfg = m.cfg
    rng = np.random.default_rng(21)
    lay = rng.random((m.T + 1, cfg.nz, cfg.ny, cfg.nx)) < 0.3
    m.set_cast_grid(R.pack(lay))                                              # (no distance field at all: none is needed without bands)
    assert m.distance_field_ptr() is None
    src, starts = _sources(cfg, 40, 3, 5), _sources(cfg, 300, 3, 6)
    for t, max_cost in ((-1.0, 300), (0.3, 300), (2.0, 11)):
        m.build_reach_fields(src, 3, t_start=t, step_seconds=0.0, max_steps=max_cost)
        m.build_cost_fields(src, 3, t=t, max_cost=max_cost)
        reach, cost = m.reach_field(None, 3), m.cost_field(None, 3)           # (neither build touches the other's snapshot)
        _same(cost, reach, ("identity", t))
        assert (cost != U).sum() > 1000 and (cost == U).any() and (max_cost > 11 or (cost == 11).any())
        a, b = m.cost_paths(starts, 80), m.reach_paths(starts, 80)
        _same(a[0], b[0], ("identity cost", t))
        _same(a[1], b[1], ("identity cells", t))
        assert np.array_equal(m.cost_weights() == 0, lay[K.layer_of(cfg, t)])
    m.close()


def _maze_inputs(cfg, T, seed):
    """a different random grid and a different random clearance per layer"""
    rng = np.random.default_rng(seed)
    shape = (T + 1, cfg.nz, cfg.ny, cfg.nx)
    return rng.random(shape) < 0.25, rng.random(shape).astype(F)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cost_random_mazes(dsp, shape):
    kw = SHAPES[shape]
    cfg = dsp.make_config(seed=5, **kw)
    T = cfg.prediction_times
    assert T == (0 if shape == "t0" else 6)
    lay, dist = _maze_inputs(cfg, T, 17)
    m = _cost_map(dsp, kw, lay, dist)
    small = cfg.nx * cfg.ny * cfg.nz <= 2000
    cur = np.array([0.3, -0.2, 0.1], F)
    # (bands, fields, t, world): 1, 3 and 4 bands; 1, 5 and 64 fields (64 where the restatement stays quick); t from the current layer to
    # the last horizon and beyond it; the world frame after a position change
    combos = [(1, 1, -1.0, False), (3, 5, 0.3, True), (4, 64 if small else 5, 2.0, False), (3, 1, 7.5, True)]
    for nb, nf, t, world in combos:
        if world:
            m.set_current_position(*[float(v) for v in cur])                  # (makes nothing of the cost fields' inputs stale)
        src = _sources(cfg, 12 * nf + 140, nf, 100 + nf)
        starts = _sources(cfg, 150, nf, 200 + nf)
        if world:
            src, starts = _shift(src, cur), _shift(starts, cur)
        pos = cur if world else np.zeros(3, F)
        got, w, cost, cells = _parity(m, src, nf, t, BANDS[nb], K.MAX_COST, world, pos, starts, 70, (shape, nb, nf, t, world))
        # not vacuous: every intended weight occurs, the sources include blocked, outside, non-finite and wrong-field ones, every field
        # with a free source reaches some other cell, and the weights change the answer
        assert set(np.unique(w).tolist()) == OCCUR[nb] | {0}, (shape, nb, np.unique(w))
        finite, inside, ijk = R.point_cells(cfg, src, world, pos)
        assert (~finite).any() and (finite & ~inside).any() and ((src["field"] < 0) | (src["field"] >= nf)).any()
        ok = inside & (src["field"] >= 0) & (src["field"] < nf)
        assert (w[ijk[ok, 2], ijk[ok, 1], ijk[ok, 0]] == 0).any(), "no source in a blocked cell"
        has = (got == 0).any((1, 2, 3))
        assert has.any() and ((got != U) & (got > 0)).any((1, 2, 3))[has].all()
        plain = K.fields(cfg, (w > 0).astype(np.uint8), src, nf, world=world, cur_pos=pos)
        assert (plain != got).any() and (got[got != U] >= plain[got != U]).all()
        assert {-1, -2, -3} <= set(np.unique(cost[cost < 0]).tolist()) and (cost > 0).any()
    m.close()


def test_cost_max_cost_cuts(dsp):
    kw = SHAPES["50x37x23"]
    cfg = dsp.make_config(seed=5, **kw)
    lay, dist = _maze_inputs(cfg, cfg.prediction_times, 3)
    m = _cost_map(dsp, kw, lay, dist)
    src, starts = _sources(cfg, 30, 2, 8), _sources(cfg, 100, 2, 9)
    full = _parity(m, src, 2, -1.0, BANDS[3], K.MAX_COST, False, np.zeros(3, F), starts, 40, "uncut")[0]
    assert full[full != U].max() > 17
    for max_cost in (17, 1):
        cut = _parity(m, src, 2, -1.0, BANDS[3], max_cost, False, np.zeros(3, F), starts, 40, ("cut", max_cost))[0]
        _same(cut, np.where(full <= max_cost, full, U).astype(np.uint16), ("cut of the full field", max_cost))
        assert (cut == max_cost).any() and (cut == U).any()
    m.close()


def test_cost_empty_levels_in_front_of_a_heavy_cell(dsp):
    """a wall of weight 8 across a plain of weight 1: once the plain in front of the wall is settled, levels stay empty before the wall's
    first cell settles, and the front goes on behind it; in a corridor one cell wide whose cells all weigh 8, SEVEN levels in a row are
    empty between any two settled ones, and the front still arrives at its end; a field with no free source is all UNREACHED"""
    kw = dict(nx=70, ny=5, nz=2, res=0.15, ppv=12)
    cfg = dsp.make_config(seed=5, **kw)
    L = cfg.prediction_times + 1
    lay = np.zeros((L, 2, 5, 70), bool)
    dist = np.full((L, 2, 5, 70), 1.0, F)
    dist[:, :, :, 20] = 0.05                                                  # the wall: the whole plane x = 20
    dist[:, :, :, 50:] = 0.05                                                 # ... and everything from x = 50 on,
    lay[:, :, :, 50:] = True
    lay[:, 0, 0, 50:] = False                                                 # of which only the row y = 0, z = 0 is free: the corridor
    lay[:, 1, 2, 3] = True                                                    # field 2's only source lies in a blocked cell
    m = _cost_map(dsp, kw, lay, dist)
    src = _at(cfg, (0, 0, 0, 0), (69, 0, 0, 1), (3, 2, 1, 2))
    starts = _at(cfg, (69, 0, 0, 0), (0, 0, 0, 1), (10, 2, 1, 2), (60, 0, 0, 0))
    got, w, cost, cells = _parity(m, src, 3, -1.0, [(0.1, 7)], K.MAX_COST, False, np.zeros(3, F), starts, 90, "gaps")
    assert set(np.unique(w).tolist()) == {0, 1, 8}
    present = set(np.unique(got[0][got[0] != U]).tolist())
    # field 0: the plain up to x = 19 ends at 19 + 4 + 1 = 24, the wall's first cell settles at 19 + 8 = 27, and between 24 and 27 ...
    assert got[0, 0, 0, 19] == 19 and got[0, 0, 0, 20] == 27 and got[0, 1, 4, 19] == 24
    # ... the levels 25 and 26 are empty.  The plain behind the wall ends at (49, 4, 1) = 61; the corridor goes 64, 72, 80, ... to 216
    assert not {25, 26} & present and got[0, 0, 0, 49] == 56 and got[0, 1, 4, 49] == 61
    assert got[0, 0, 0, 50:].tolist() == [64 + 8 * k for k in range(20)]
    assert not (set(range(62, 217)) - set(range(64, 217, 8))) & present       # seven empty levels between any two of them
    assert (got[2] == U).all() and cost.tolist() == [216, int(got[1, 0, 0, 0]), -1, int(got[0, 0, 0, 60])]
    assert (cells[0] >= 0).sum() == 20 + 29 + 1 + 20 and (cells[2] == -1).all()
    # field 1 starts at the corridor's end: its first step already costs 8, and the levels 1 .. 7 are empty
    f1 = set(np.unique(got[1][got[1] != U]).tolist())
    assert {0, 8, 152, 153} <= f1 and not (set(range(1, 152)) - set(range(8, 152, 8))) & f1
    m.close()


def _mean_clearance(dist, cells):
    ok = cells >= 0
    return float(dist.reshape(-1)[cells[ok]].mean()), float(dist.reshape(-1)[cells[ok]].min()), int(ok.sum())


def test_cost_on_a_real_scene(dsp):
    kw = dict(SMALL)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    thr = _scene_threshold(m)
    m.build_distance_field(thr, 8)
    bands = [(0.45, 3), (0.75, 2), (1.05, 1)]                                 # metres: 3, 5 and 7 voxels of 0.15 m
    used = complete = 0
    for r in (0, 2):
        m.build_cast_grid(thr, r)
        assert m.distance_field_ptr() is not None                            # (the grid's build leaves the distance field alone)
        for t, world in ((-1.0, False), (0.3, True)):
            l = K.layer_of(cfg, t)
            lay, dist = _grid_cells(m)[l], m.distance_field(l)
            free = np.argwhere(~lay)
            rng = np.random.default_rng(5 + r)
            pick = free[rng.integers(0, len(free), 2 + 120)]
            pts = _at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k % 2) for k, c in enumerate(pick)])
            src, starts = pts[:2], np.concatenate([pts[2:], _sources(cfg, 30, 2, 4)])
            if world:
                src, starts = _shift(src, cur), _shift(starts, cur)
            pos = cur if world else np.zeros(3, F)
            got, w, cost, cells = _parity(m, src, 2, t, bands, K.MAX_COST, world, pos, starts, 200, ("scene", r, t))
            assert len(set(np.unique(w).tolist()) - {0}) >= 2, np.unique(w)
            # the chain: weighted paths -> line-of-sight waypoints -> casts, all in the grid the paths were found in
            ts = dict(t_start=t, step_seconds=0.0)
            info, seg, end = m.shorten_paths(cost, cells, window=64, **ts)
            assert info["n_blocked"].sum() == 0
            hits = m.cast_segments(seg.reshape(-1, 8))
            live = (np.arange(end.shape[1])[None, :] < info["n_segments"][:, None]).reshape(-1)
            assert live.any() and (hits["status"][live] == CR.FREE).all()
            used += int(live.sum())
            # the point of the weights: along the weighted paths the clearance is no smaller than along the unweighted ones
            m.build_cost_fields(src, 2, t=t, world=world)
            plain_cost, plain_cells = m.cost_paths(starts, 200, world=world)
            both = (cost >= 0) & (plain_cost >= 0) & (cells[:, -1] < 0) & (plain_cells[:, -1] < 0)       # complete in both builds
            assert both.sum() >= 20 and (plain_cost[both] <= cost[both]).all()
            a, b = _mean_clearance(dist, cells[both]), _mean_clearance(dist, plain_cells[both])
            print("inflate", r, "t", t, "mean / min F / cells along weighted paths", a, "unweighted", b)
            assert a[0] >= b[0], ("mean clearance along weighted paths %r below that along unweighted paths %r" % (a, b), r, t)
            complete += int(both.sum())
    assert used >= 100 and complete >= 80
    m.close()


def test_cost_device_entry_points_stream_ordered_behind_frame(dsp):
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
    bands = [(0.3, 2), (0.6, 1)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(0.05, 1)                                        # no synchronisation between the frame, the builds and the paths
            m.build_distance_field(0.05, 6)
            m.build_cost_fields(sd, 4, t=0.2, bands=bands, max_cost=400, world=True)
            outs.append(m.cost_paths(td, 130, world=True))
        st.synchronize()
        assert m.cost_fields_ptr() is not None
        dev_fields, dev_w = m.cost_field(None, 4), m.cost_weights()           # what the device entry point left behind the last frame
        l = K.layer_of(cfg, 0.2)
        lay, dist = _grid_cells(m)[l], m.distance_field(l)
        m.build_cost_fields(src, 4, t=0.2, bands=bands, max_cost=400, world=True)       # the host variant on the same snapshots
        host_fields, host_w = m.cost_field(None, 4), m.cost_weights()
        host_paths = m.cost_paths(starts, 130, world=True)
        after = m.cost_paths(td, 130, world=True)
        st.synchronize()
    assert np.array_equal(dev_fields, host_fields) and np.array_equal(dev_w, host_w)
    _same(host_w, K.weights(lay, dist, bands), "device entry weights")
    want = K.fields(cfg, host_w, src, 4, max_cost=400, world=True, cur_pos=cur)
    _same(host_fields, want, "device entry")
    assert ((want != U) & (want > 0)).sum() > 1000 and len(np.unique(host_w)) >= 3
    for k in range(2):
        assert outs[-1][k].dtype == torch.int32 and torch.equal(outs[-1][k], after[k])
        assert np.array_equal(after[k].cpu().numpy(), host_paths[k])
    assert not all(torch.equal(outs[0][k], outs[-1][k]) for k in range(2))
    wc, wp = K.paths(cfg, want, host_w, starts, 130, world=True, cur_pos=cur)
    _same(host_paths[0], wc, "device cost")
    _same(host_paths[1], wp, "device cells")
    assert K.check_paths(cfg, host_fields, host_w, starts, host_paths[0], host_paths[1], world=True, cur_pos=cur) >= 1
    m.close()


def test_cost_life_cycle_and_read_only(dsp):
    kw = dict(SMALL)
    m, twin = _twins(dsp, kw)
    frames = _scene_frames(dsp, kw, 8, seed=31)
    for x in (m, twin):
        _run(x, frames[:6])
    thr = _median_threshold(m)
    cfg = m.cfg
    src, starts = _sources(cfg, 400, 3, 3), _sources(cfg, 300, 3, 4)
    bands = [(0.3, 2), (0.6, 1)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    cb = m._cost_bands(bands)
    out, cost, cells = np.zeros(m.V, np.uint16), np.zeros(len(starts), np.int32), np.zeros((len(starts), 50), np.int32)

    def build_raw(n_bands=True):
        b = cb if n_bands else m._cost_bands(())
        return m.L.dspmap_build_cost_fields(m.h, 3, len(src), p(src), -1.0, C.addressof(b), 500, 0)

    for x in (m, twin):
        x.build_cast_grid(thr, 1)
    assert m.cost_fields_ptr() is None
    # bands need the distance field, a build without bands does not
    assert build_raw() == E_STATE and b"dspmap_build_distance_field" in m.L.dspmap_last_error(m.h) and m.cost_fields_ptr() is None
    assert build_raw(False) == OK and m.cost_fields_ptr() is not None
    for x in (m, twin):
        x.build_distance_field(thr, 6)
    m.build_reach_fields(src, 3, max_steps=120)
    grid, field, reach, res = m.cast_grid(), m.distance_field(), m.reach_field(None, 3), m.results()
    ptrs = (m.cast_grid_ptr(), m.distance_field_ptr(), m.reach_fields_ptr())

    def fresh():
        """whatever is stale is built again, then the cost fields"""
        if m.cast_grid_ptr() is None:
            m.build_cast_grid(thr, 1)
        if m.distance_field_ptr() is None:
            m.build_distance_field(thr, 6)
        m.build_cost_fields(src, 3, bands=bands, max_cost=500)
        assert m.cost_fields_ptr() is not None and m.L.dspmap_cost_weights_device(m.h) is not None

    def stale(tag):
        assert m.cost_fields_ptr() is None and m.L.dspmap_cost_weights_device(m.h) is None, tag
        for rc in (m.L.dspmap_get_cost_field(m.h, 0, p(out)), m.L.dspmap_get_cost_weights(m.h, p(out)),
                   m.L.dspmap_cost_paths(m.h, len(starts), p(starts), 50, 0, p(cost), p(cells))):
            assert rc == E_STATE and b"dspmap_build_cost_fields" in m.L.dspmap_last_error(m.h), tag
        assert not out.any() and not cost.any() and not cells.any(), tag

    fresh()
    first = m.cost_field(None, 3)
    paths0 = m.cost_paths(starts, 50)
    # read-only: the grid, the distance field, the arrival fields and the map are bit-identical before and after, and still valid
    assert (m.cast_grid_ptr(), m.distance_field_ptr(), m.reach_fields_ptr()) == ptrs
    assert np.array_equal(m.cast_grid(), grid) and m.distance_field().tobytes() == field.tobytes() and np.array_equal(m.reach_field(None, 3), reach)
    assert np.array_equal(m.results(), res) and np.array_equal(m.results(), twin.results())
    fut = m.getFutureStatus()
    assert np.array_equal(fut, twin.getFutureStatus()) and (fut != 0).any()
    for x, y in zip(m.export_state(), twin.export_state()):
        assert np.array_equal(x, y)
    twin.close()
    w = m.cost_weights()
    _same(first, K.fields(cfg, w, src, 3, max_cost=500), "life cycle")
    _same(w, K.weights(R.unpack(grid, cfg.nx)[0], field[0], bands), "life cycle weights")
    assert K.check_paths(cfg, first, w, starts, *paths0) >= 1
    # NOT stale after a readout, a reach build or a clear of the future status
    m.results(); m.cast_grid(); m.distance_field(); m.cost_field(0); m.cost_weights()
    m.build_reach_fields(src, 3, max_steps=60)
    m.clearOccupancyMapPrediction()
    assert m.cost_fields_ptr() is not None and np.array_equal(m.cost_field(None, 3), first)
    with pytest.raises(dsp.capi.DSPMapError):
        m.cost_field(3)                                                       # a field the last build did not grow
    # stale after each of these, one by one; a build makes it valid again
    m.build_cast_grid(thr, 1)
    stale("build_cast_grid")
    fresh()
    m.set_cast_grid(grid)
    stale("set_cast_grid")
    fresh()
    assert np.array_equal(m.cost_field(None, 3), first)
    m.set_known(np.zeros((cfg.nz, cfg.ny, cfg.nx), np.int32))
    assert m.cost_fields_ptr() is not None                                    # (the known-space layer alone changes nothing here)
    m.mask_cast_grid(1000)
    stale("mask_cast_grid")
    fresh()
    m.build_distance_field(thr, 6)
    stale("build_distance_field")
    fresh()
    m.set_distance_field(field)
    stale("set_distance_field")
    assert m.distance_field_ptr() == ptrs[1]                                  # (the field stays valid)
    fresh()
    m.build_cost_fields(src, 3, max_cost=500)                                 # without bands ...
    m.set_distance_field(field)
    stale("set_distance_field without bands")                                 # ... the same rule
    fresh()
    # a new cost build replaces the snapshot: the old fields are gone
    m.build_cost_fields(src[:50], 1, bands=bands, max_cost=9)
    assert (m.cost_field(0) != first[0]).any()
    with pytest.raises(dsp.capi.DSPMapError):
        m.cost_field(1)
    # a build that fails its state check after the rebuild flag would have been cleared leaves the snapshot alone
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    stale("update")
    assert build_raw() == E_STATE and b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    fresh()
    assert (m.cost_field(None, 3) != first).any()
    m.clear_state()
    stale("clear_state")
    m.close()
