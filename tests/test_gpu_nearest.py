"""GPU tests of the nearest-obstacle fields (dspmap_build_nearest_field, dspmap_get_nearest_field, dspmap_query_nearest*): exact parity --
integer equality of the indices, bit patterns of the floats -- with the numpy restatement (tests/nearest_ref.py) fed with what the map
hands out AFTER the build, over storage orders, thresholds, radii and both modes; hand-made cast grids whose ties, truncation edges, word
boundaries and padding bits the tie rule and the three passes have to get right; the point queries through the host and the device path;
read-only behaviour, snapshot validity and staleness (with the extra dependency of a snapshot built from the cast grid), and stream order
behind the frame."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import distance_ref as D
from tests import nearest_ref as N
from tests.test_gpu_distance import _bits, _median_threshold, _twins
from tests.test_gpu_query import B, _run, _samples, _scene_frames

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
RADII = (1, 4, 20, 64)
SMALL = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)


def _same(got_near, got_dist, want_near, want_dist, what):
    assert got_near.dtype == np.int32 and got_near.shape == want_near.shape and got_dist.shape == want_dist.shape, what
    bad = np.flatnonzero(got_near.ravel() != want_near.ravel())
    assert bad.size == 0, (what, "near", bad.size, bad[:5], got_near.ravel()[bad[:5]], want_near.ravel()[bad[:5]])
    bad = np.flatnonzero(_bits(got_dist).ravel() != _bits(want_dist).ravel())
    assert bad.size == 0, (what, "dist", bad.size, bad[:5], got_dist.ravel()[bad[:5]], want_dist.ravel()[bad[:5]])


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_nearest_field_parity_on_real_frames(dsp, variant):
    cfg = dsp.make_config(seed=1234, **B)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    _run(m, _scene_frames(dsp, B, 12))
    assert int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    med = _median_threshold(m)
    res_m = F(cfg.voxel_resolution)
    got = {}
    for thr in (0.2, med, 0.0, 1e9):
        for R in RADII:
            for signed in (False, True):
                m.build_nearest_field(thr, R, signed=signed)
                assert m.nearest_field_ptr() is not None and m.nearest_distance_ptr() is not None
                got[thr, R, signed] = (m.nearest_field(), m.nearest_distance())
            m.build_distance_field(thr, R)
            got[thr, R, "df"] = m.distance_field()
    res, fut = m.results(), m.getFutureStatus()      # read after the builds: they changed nothing
    for thr in (0.2, med, 0.0, 1e9):
        occ = D.occupancy_layers(cfg, res, fut, thr)
        for signed in (False, True):
            d2, near = N.pairs_untruncated(occ, signed)
            for R in RADII:
                td2, tnear = N.truncate(d2, near, R)
                _same(*got[thr, R, signed], tnear, N.value(td2, occ, R, res_m, signed), (variant, thr, R, signed))
            if thr == med:
                # the input is not degenerate: both classes, cells without a target and cells exactly R away at R = 4, and under SIGNED
                # occupied cells with a free target
                assert occ[0].sum() >= 1000 and (~occ[0]).sum() >= 1000
                t4, n4 = N.truncate(d2, near, 4)
                assert (n4[~occ] == -1).any() and (t4[~occ] == 16).any() and ((t4 > 0) & (t4 < 16)).any()
                if signed:
                    hit = occ & (n4 >= 0)
                    assert hit.sum() >= 1000 and not occ.reshape(len(occ), -1)[np.nonzero(hit)[0], n4[hit]].any()
                else:
                    assert (near[occ] == np.nonzero(occ.reshape(len(occ), -1))[1]).all()
        for R in RADII:      # without a flag the distances are the distance field's, bit for bit
            assert np.array_equal(_bits(got[thr, R, False][1]), _bits(got[thr, R, "df"])), (thr, R)
    assert (got[1e9, 20, True][0] == -1).all() and (got[1e9, 20, True][1] == F(20) * res_m).all()
    assert (got[0.0, 20, True][1][0] < 0).sum() > 10000
    m.close()


SHAPES = {"50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),        # no multiple of 64 anywhere, padding bits in the only word
          "132x132x60": dict(nx=132, ny=132, nz=60, res=0.15, ppv=9),      # rows of three words
          "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=())}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_nearest_ties_and_edges_in_hand_made_grids(dsp, shape):
    kw = SHAPES[shape]
    cfg = dsp.make_config(seed=77, **kw)
    m = dsp.DSPMap(cfg)
    dims = (cfg.nz, cfg.ny, cfg.nx)
    L = m.T + 1
    assert L == (1 if shape == "t0" else 7)
    big = shape == "132x132x60"
    radii = (64,) if big else (5, 64)
    scenes = N.tie_scenes(dims, 64)
    if big:      # only what needs three-word rows: the reach of R = 64 across word boundaries, the last columns, one random layer
        scenes = [s for s in scenes if s[0].startswith(("edge_", "last_")) or s[0] == "random_0.02"]
        assert {"edge_x63", "edge_x64", "edge_x127"} <= {s[0] for s in scenes}
    if shape == "t0":      # one layer per build: a selection that still has every kind
        keep = ("pair_x_2", "pair_y_1", "pair_z_3", "xy_5_+1+1", "xy_5_-1-1", "yz_5_+1-1", "xz_5_-1+1", "345_xyz_+1", "345_xyz_-1",
                "345_xy_mixed_+1", "345_zx_-1", "edge_x0", "edge_ymid", "last_columns", "all_set", "all_clear", "random_0.02", "random_0.98")
        scenes = [s for s in scenes if s[0] in keep]
        assert len(scenes) == len(keep)
    m.build_cast_grid(0.5, 0)
    for r0 in range(0, len(scenes), L):
        grp = [scenes[(r0 + k) % len(scenes)] for k in range(L)]      # every layer another pattern
        occ = np.stack([g for _, g, _ in grp])
        names = [n for n, _, _ in grp]
        for R in radii:
            for signed in (False, True):
                m.set_cast_grid(N.bits_of(occ))
                assert m.nearest_field_ptr() is None
                m.build_nearest_field(float("nan"), R, signed=signed, from_cast_grid=True)      # (the threshold is not read)
                near, dist = m.nearest_field(), m.nearest_distance()
                wn, wd = N.layers(occ, R, F(cfg.voxel_resolution), signed)
                _same(near, dist, wn, wd, (shape, names, R, signed))
                for l, (name, g, cell) in enumerate(grp):      # (that these cells have several minimisers: tests/test_nearest_cpu.py)
                    assert cell is None or (near[l][cell] >= 0 and g.ravel()[near[l][cell]]), name
    # spot checks in words, beside the parity: exactly R cells away is a target, R + 1 is none; the padding bits are no free targets
    one = np.zeros((L,) + dims, bool)
    one[:, 0, 0, 0] = True
    R = min(5, cfg.nx - 2)
    m.set_cast_grid(N.bits_of(one))
    m.build_nearest_field(0.0, R, from_cast_grid=True)
    near = m.nearest_field()
    assert (near[:, 0, 0, R] == 0).all() and (near[:, 0, 0, R + 1] == -1).all()
    if cfg.ny > R + 1:
        assert (near[:, 0, R, 0] == 0).all() and (near[:, 0, R + 1, 0] == -1).all()
    full = np.ones((L,) + dims, bool)
    m.set_cast_grid(N.bits_of(full))
    m.build_nearest_field(0.0, 64, signed=True, from_cast_grid=True)
    assert (m.nearest_field() == -1).all() and (m.nearest_distance() == -(F(64) * F(cfg.voxel_resolution))).all()
    m.close()


def _query_same(got, want, what):
    for name in N.NEAREST_DTYPE.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(w), -1).any(1))
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_nearest_query_parity(dsp, variant):
    cfg = dsp.make_config(seed=1234, **SMALL)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, SMALL, 8, seed=31))
    assert np.abs(cur).max() > 0
    thr = _median_threshold(m)
    q = _samples(cfg, 4096, 7)
    assert len({float(t) for t in q[:, 3] if t == t}) >= 8      # every layer is selected by some t
    runs = []
    for R, signed, from_grid in ((3, False, False), (20, True, False), (3, True, True)):
        if from_grid:
            m.build_cast_grid(thr, 1)
            grid = m.cast_grid()
        m.build_nearest_field(thr, R, signed=signed, from_cast_grid=from_grid)
        near, dist = m.nearest_field(), m.nearest_distance()
        for world in (False, True):
            qq = q.copy()
            if world:
                qq[:, :3] = (qq[:, :3] + cur[None, :]).astype(F)
            host = m.query_nearest(qq, world=world, outside=-2.5)
            qd = torch.from_numpy(np.concatenate([qq, qq], 1)).cuda()[:, :4]   # a non-contiguous view: the binding's temporary
            torch.cuda.synchronize()
            dev = m.query_nearest(qd, world=world, outside=-2.5)
            m.sync()
            runs.append((R, signed, grid if from_grid else None, near, dist, world, qq, host, {k: v.cpu().numpy() for k, v in dev.items()}))
    res, fut = m.results(), m.getFutureStatus()
    for R, signed, grid, near, dist, world, qq, host, dev in runs:
        if grid is None:
            occ = D.occupancy_layers(cfg, res, fut, thr)
        else:
            occ = ((grid[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(grid.shape[:3] + (-1,))[..., :cfg.nx]
        wn, wd = N.layers(occ, R, F(cfg.voxel_resolution), signed)
        _same(near, dist, wn, wd, (variant, R, signed, grid is not None))
        want = N.query(cfg, wn, wd, occ, res, qq, world=world, cur_pos=cur, outside=-2.5)
        _query_same(host, want, ("host", R, signed, world))
        _query_same(dev, want, ("device", R, signed, world))
        inside = want["dist"] != F(-2.5)
        own_occ = inside & ((want["dist"] < 0) if signed else (want["dist"] == 0))
        assert 500 < inside.sum() < len(qq) and own_occ.sum() > 20 and (inside & ~own_occ).sum() > 200
        assert (want["voxel"][~inside] == -1).all() and not want["offset"][~inside].any() and not want["velocity"][~inside].any()
        if R == 3:
            assert (inside & (want["voxel"] == -1)).sum() > 20      # cells without a target within R
        assert (want["velocity"][inside & (qq[:, 3] >= 0)] == 0).all()
        assert (want["offset"] != 0).any(0).all()
        if R == 20:      # velocities of free cells' targets and of occupied own cells, in the current layer
            cur_layer = inside & (qq[:, 3] < 0)
            assert (want["velocity"][cur_layer & own_occ] != 0).any() and (want["velocity"][cur_layer & ~own_occ] != 0).any()
    m.close()


def test_nearest_build_is_read_only_and_follows_the_life_cycle(dsp, tmp_path):
    frames = _scene_frames(dsp, SMALL, 14, seed=77)
    a, b = _twins(dsp, SMALL)
    for pts, pos, quat, t in frames[:4]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    # the future status after a build is the one of the twin that never built; distance field and cast grid of the handle are untouched
    a.build_distance_field(0.1, 20)
    a.build_cast_grid(0.1, 1)
    df, cg = a.distance_field(), a.cast_grid()
    a.build_nearest_field(0.1, 20, signed=True)
    a.build_nearest_field(0.1, 20, signed=True, from_cast_grid=True)
    near, dist = a.nearest_field(), a.nearest_distance()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    assert a.distance_field_ptr() is not None and a.cast_grid_ptr() is not None
    assert np.array_equal(_bits(a.distance_field()), _bits(df)) and np.array_equal(a.cast_grid(), cg)
    occ = ((cg[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(cg.shape[:3] + (-1,))[..., :a.cfg.nx]
    _same(near, dist, *N.layers(occ, 20, F(0.15), True), "from the inflated grid")
    for pts, pos, quat, t in frames[4:]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        a.build_nearest_field(0.1, 8, signed=True)
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.results(), b.results())
    assert np.array_equal(a.getFutureStatus(), b.getFutureStatus())
    assert b.nearest_field_ptr() is None and b.nearest_distance_ptr() is None      # a handle that never built has none
    b.close()
    # the snapshot survives readouts and the clear; every call that computes a frame or replaces state makes it stale
    m = a
    snap = m.nearest_field()
    ptr = m.nearest_field_ptr()
    q = _samples(m.cfg, 500, 3)
    m.getOccupancyMapWithFutureStatus(0.1)
    m.clearOccupancyMapPrediction()
    m.results(); m.query_occupancy(q)
    assert m.nearest_field_ptr() == ptr and np.array_equal(m.nearest_field(), snap)
    voxel, slot, rec = m.export_state()
    ck = str(tmp_path / "ck.bin")
    m.save_checkpoint(ck)
    pts, pos, quat, t = frames[-1]
    t_next = [t]

    def update():
        t_next[0] += 1 / 30.0
        assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t_next[0], quat) == 1
    # the four stages are one frame in its order, behind the binning of its cloud, on a handle of their own that runs no other frame
    (st,) = _twins(dsp, SMALL, 1)
    st.bin_points(common.wall_cloud(2, n_side=30, dist=1.6, half_w=1.2, half_h=0.7))
    stale_calls = [(m, "update_device", update), (m, "clear_state", m.clear_state), (m, "import_state", lambda: m.import_state(voxel, rec, slot)),
                   (m, "load_checkpoint", lambda: m.load_checkpoint(ck)), (m, "seed_uniform", lambda: m.seed_uniform(1, 0.01, 3)),
                   (st, "stage_predict", lambda: st.predict(0.0, 0.0, 0.0, 0.0)), (st, "stage_update", st.map_update),
                   (st, "stage_birth", st.add_newborn), (st, "stage_resample", st.occupancy_resample)]
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)   # noqa: E731
    out_n, out_q = np.zeros(m.V, np.int32), np.zeros(len(q), N.NEAREST_DTYPE)
    for k, (h, name, call) in enumerate(stale_calls):
        from_grid = bool(k & 1)      # either source: the map carries both
        if from_grid:
            h.build_cast_grid(0.1, 0)
        h.build_nearest_field(0.1, 4, from_cast_grid=from_grid)
        assert h.nearest_field_ptr() is not None and h.nearest_distance_ptr() is not None, name
        call()
        assert h.nearest_field_ptr() is None and h.nearest_distance_ptr() is None, name
        assert h.L.dspmap_get_nearest_field(h.h, 0, p(out_n), None) == E_STATE and b"dspmap_build_nearest_field" in h.L.dspmap_last_error(h.h)
        assert h.L.dspmap_query_nearest(h.h, len(q), p(q), 0, 0.0, p(out_q)) == E_STATE and b"dspmap_build_nearest_field" in h.L.dspmap_last_error(h.h)
    st.close()
    with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_nearest_field"):
        m.query_nearest(torch.from_numpy(q).cuda())
    # the cast grid carries only the snapshot that was built from it
    update()
    m.integrate_known()
    m.build_cast_grid(0.1, 0)
    words = m.cast_grid()
    grid_calls = [("build_cast_grid", lambda: m.build_cast_grid(0.1, 1)), ("mask_cast_grid", lambda: m.mask_cast_grid(2)),
                  ("set_cast_grid", lambda: m.set_cast_grid(words))]
    for name, call in grid_calls:
        m.build_nearest_field(0.1, 4, signed=True, from_cast_grid=True)
        assert m.nearest_field_ptr() == ptr
        call()
        assert m.nearest_field_ptr() is None and m.cast_grid_ptr() is not None, name
        m.build_nearest_field(0.1, 4, signed=True)
        mass_sourced = m.nearest_field()
        call()
        assert m.nearest_field_ptr() == ptr and np.array_equal(m.nearest_field(), mass_sourced), name
    m.build_nearest_field(0.1, 4, from_cast_grid=True)
    m.build_distance_field(0.1, 4)      # another layer's build takes nothing away
    assert m.nearest_field_ptr() == ptr and m.nearest_field().shape == snap.shape
    m.close()


def test_nearest_build_stream_ordered_behind_frame(dsp):
    frames = _scene_frames(dsp, SMALL, 6, seed=31)
    fields = []
    for sync_first in (False, True):
        (m,) = _twins(dsp, SMALL, 1)
        st = torch.cuda.Stream()
        m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
        with torch.cuda.stream(st):
            for pts, pos, quat, t in frames:
                assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
                if sync_first:
                    st.synchronize()
                m.build_nearest_field(0.1, 20, signed=True)      # directly behind the frame
            fields.append((m.nearest_field(), m.nearest_distance()))
            res, fut = m.results(), m.getFutureStatus()
        wn, wd, occ = N.field(m.cfg, res, fut, 0.1, 20, True)
        _same(*fields[-1], wn, wd, sync_first)
        m.close()
    assert np.array_equal(fields[0][0], fields[1][0]) and np.array_equal(_bits(fields[0][1]), _bits(fields[1][1]))
    assert (fields[0][1] > 0).any() and (fields[0][1] < 0).any() and (fields[0][0] >= 0).any()
