"""GPU tests of the distance fields (dspmap_build_distance_field, dspmap_get_distance_field, dspmap_query_distance*): bit parity --
zero mismatching cells -- with the numpy restatement (tests/distance_ref.py) fed with what the map hands out AFTER the build, over
storage orders, thresholds, radii, the outside-occupied flag and awkward shapes; read-only behaviour, the pending clear, snapshot
validity and staleness, stream order behind the frame, and the point queries with their gradients."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import distance_ref as D
from tests.test_gpu_query import B, _run, _samples, _scene_frames

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
RADII = (1, 4, 20, 64)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _median_threshold(m):
    mass = m.results()[:, 0]
    assert (mass > 0).any()
    return float(np.median(mass[mass > 0]))


def _build_all(m, combos):
    """the fields of every (threshold, R, outside_occupied) of combos, each read back right after its build"""
    out = []
    for thr, R, oo in combos:
        m.build_distance_field(thr, R, outside_occupied=oo)
        assert m.distance_field_ptr() is not None
        out.append(m.distance_field())
    return out


def _check_fields(m, cfg, combos, got):
    """bit parity of got[i] with the restatement of combos[i] over results() / getFutureStatus() read now; returns (res, fut, d2 by threshold)"""
    res, fut = m.results(), m.getFutureStatus()
    d2 = {}
    for (thr, R, oo), g in zip(combos, got):
        if thr not in d2:
            d2[thr] = D.d2_layers(D.occupancy_layers(cfg, res, fut, thr))
        want = D.field(cfg, res, fut, thr, R, oo, d2=d2[thr])
        assert g.shape == want.shape == (cfg.prediction_times + 1, cfg.nz, cfg.ny, cfg.nx)
        bad = np.flatnonzero(_bits(g) != _bits(want))
        assert bad.size == 0, (thr, R, oo, bad.size, bad[:5], g.ravel()[bad[:5]], want.ravel()[bad[:5]])
    return res, fut, d2


@pytest.mark.parametrize("variant", ["runs", "cubes", "static"])
def test_distance_field_bit_parity(dsp, variant):
    kw = dict(B)
    if variant == "static":
        kw.update(static_model=1)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    if variant in ("runs", "cubes"):
        m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=0.0 if variant == "static" else 1.0)
    _run(m, _scene_frames(dsp, kw, 12))
    if variant in ("runs", "cubes"):
        assert int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    med = _median_threshold(m)
    combos = [(thr, R, oo) for thr in (0.2, med, 0.0, 1e9) for R in RADII for oo in (False, True)]
    got = _build_all(m, combos)
    res, fut, d2 = _check_fields(m, cfg, combos, got)
    # the input is not degenerate: both classes at the median threshold, truncated and untruncated cells at R = 4, an empty and a dense case
    occ0 = res[:, 0] > F(med)
    assert occ0.sum() >= 1000 and (~occ0).sum() >= 1000
    assert (d2[med] > 16).any() and (d2[med] <= 16).any() and ((d2[med] > 0) & (d2[med] < 16)).any()
    assert (d2[1e9] == D.INF).all() and (d2[0.0][0] == 0).sum() > 10000
    empty = got[combos.index((1e9, 20, False))]
    assert (empty == F(20) * F(cfg.voxel_resolution)).all()
    assert not np.array_equal(got[combos.index((med, 20, False))], got[combos.index((med, 20, True))])
    m.close()


@pytest.mark.parametrize("shape", ["50x37x23", "132x132x60", "8x8x1", "t0"])
def test_distance_field_awkward_shapes(dsp, shape):
    kw = {"50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),        # no multiple of 64 anywhere
          "132x132x60": dict(nx=132, ny=132, nz=60, res=0.15, ppv=9),      # rows longer than two ballot words
          "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=())}[shape]
    cfg = dsp.make_config(seed=77, **kw)
    m = dsp.DSPMap(cfg)
    m.seed_uniform(2, 0.01, 5, vmax=1.0)
    if shape == "8x8x1":     # (a map smaller than the scene's sensor range: a hand-made cloud inside it)
        pts = torch.tensor([[0.3, 0.1, 0.0], [0.3, -0.2, 0.02], [0.45, 0.3, -0.03]], dtype=torch.float32, device="cuda")
        for f in range(4):
            assert m.update_device(pts.data_ptr(), 3, (0.0, 0.0, 0.0), f / 30.0, (1.0, 0.0, 0.0, 0.0)) == 1
    else:
        _run(m, _scene_frames(dsp, kw, 6 if shape == "132x132x60" else 8, seed=31))
    assert m.T == (0 if shape == "t0" else 6)
    med = _median_threshold(m)
    combos = [(med, R, oo) for R in ((4, 64) if shape == "132x132x60" else RADII) for oo in (False, True)] + [(0.0, 20, False), (1e9, 64, True)]
    got = _build_all(m, combos)
    res, fut, d2 = _check_fields(m, cfg, combos, got)
    occ0 = res[:, 0] > F(med)
    assert (~occ0).any() and (occ0.any() or shape == "8x8x1")      # (64 voxels may all hold the same mass; the dense and the empty case remain)
    assert got[0].shape[0] == m.T + 1
    m.close()


def _twins(dsp, kw, n=2):
    maps = []
    for _ in range(n):
        m = dsp.DSPMap(dsp.make_config(seed=99, **kw))
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        maps.append(m)
    return maps


def test_distance_build_is_read_only(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    frames = _scene_frames(dsp, kw, 14, seed=77)
    a, b = _twins(dsp, kw)
    for pts, pos, quat, t in frames[:4]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    # the future status after a build is the one of the twin that never built
    a.build_distance_field(0.1, 20, outside_occupied=True)
    fld = a.distance_field()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    assert np.array_equal(_bits(fld), _bits(D.field(a.cfg, a.results(), fa, 0.1, 20, True)))
    # ten more frames, one twin building a field behind every frame (no readout in between: nothing arms a clear on either)
    for pts, pos, quat, t in frames[4:]:
        for m in (a, b):
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        a.build_distance_field(0.1, 8)
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.results(), b.results())
    assert np.array_equal(a.getFutureStatus(), b.getFutureStatus())
    assert b.distance_field_ptr() is None      # a handle that never built a field has none
    a.close(); b.close()


def test_distance_pending_clear_reads_empty_layers(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    (m,) = _twins(dsp, kw, 1)
    _run(m, _scene_frames(dsp, kw, 6, seed=31))
    thr = _median_threshold(m)
    m.build_distance_field(thr, 20)
    before = m.distance_field()
    assert (before[1:] != F(20) * F(0.15)).any()
    m.clearOccupancyMapPrediction()
    # the snapshot survives the clear ...
    assert m.distance_field_ptr() is not None and np.array_equal(m.distance_field(), before)
    # ... and a rebuild sees horizons that read 0 everywhere: empty layers; the current mass is unchanged
    m.build_distance_field(thr, 20)
    after = m.distance_field()
    assert np.array_equal(after[0], before[0])
    assert (after[1:] == F(20) * F(0.15)).all()
    m.build_distance_field(-1.0, 20)      # 0 > -1: every voxel of a cleared layer is occupied
    assert (m.distance_field()[1:] == 0).all()
    m.close()


def test_distance_snapshot_validity_and_staleness(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    (m,) = _twins(dsp, kw, 1)
    frames = _scene_frames(dsp, kw, 7, seed=31)
    _run(m, frames[:6])
    m.build_distance_field(0.1, 20)
    snap = m.distance_field()
    ptr = m.distance_field_ptr()
    q = _samples(m.cfg, 2000, 3)
    d0, g0 = m.query_distance(q)
    m.getOccupancyMapWithFutureStatus(0.1)
    m.clearOccupancyMapPrediction()
    m.results(); m.query_occupancy(q)
    assert m.distance_field_ptr() == ptr and np.array_equal(m.distance_field(), snap)
    d1, g1 = m.query_distance(q)
    assert np.array_equal(_bits(d0), _bits(d1)) and np.array_equal(_bits(g0), _bits(g1))
    pts, pos, quat, t = frames[6]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    assert m.distance_field_ptr() is None
    out = np.zeros(m.V, F)
    dist, grad = np.zeros(len(q), F), np.zeros((len(q), 3), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert m.L.dspmap_get_distance_field(m.h, 0, p(out)) == E_STATE
    assert b"changed" in m.L.dspmap_last_error(m.h)
    assert m.L.dspmap_query_distance(m.h, len(q), p(q), 0, 0.0, p(dist), p(grad)) == E_STATE
    qd = torch.from_numpy(q).cuda()
    with pytest.raises(dsp.capi.DSPMapError):
        m.query_distance(qd)
    # every other call that computes a frame or replaces state does the same
    voxel, slot, rec = m.export_state()
    for stale in (lambda: m.seed_uniform(1, 0.01, 3), m.clear_state, lambda: m.import_state(voxel, rec, slot)):
        m.build_distance_field(0.1, 4)
        assert m.distance_field_ptr() is not None
        stale()
        assert m.distance_field_ptr() is None
    m.build_distance_field(0.1, 20)      # and a rebuild is valid again
    assert m.distance_field_ptr() == ptr and m.distance_field().shape == snap.shape
    m.close()


def test_distance_build_stream_ordered_behind_frame(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    fields = []
    for sync_first in (False, True):
        (m,) = _twins(dsp, kw, 1)
        st = torch.cuda.Stream()
        m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
        with torch.cuda.stream(st):
            for pts, pos, quat, t in frames:
                assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
                if sync_first:
                    st.synchronize()
                m.build_distance_field(0.1, 20, outside_occupied=True)      # directly behind the frame
            fields.append(m.distance_field())
            res, fut = m.results(), m.getFutureStatus()
        assert np.array_equal(_bits(fields[-1]), _bits(D.field(m.cfg, res, fut, 0.1, 20, True)))
        m.close()
    assert np.array_equal(_bits(fields[0]), _bits(fields[1]))
    assert (fields[0] > 0).any() and (fields[0] == 0).any()


@pytest.mark.parametrize("variant", ["runs", "cubes"])
def test_distance_query_bit_parity(dsp, variant):
    kw = dict(B)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    assert np.abs(cur).max() > 0
    thr = _median_threshold(m)
    m.build_distance_field(thr, 20, outside_occupied=(variant == "cubes"))
    fld = m.distance_field()
    q = _samples(cfg, 50000, 7)
    runs = []
    for world in (False, True):
        qq = q.copy()
        if world:
            qq[:, :3] = (qq[:, :3] + cur[None, :]).astype(F)
        hd, hg = m.query_distance(qq, world=world, outside=-2.5)
        h_only = m.query_distance(qq, world=world, outside=-2.5, grad=False)
        qd = torch.from_numpy(np.concatenate([qq, qq], 1)).cuda()[:, :4]   # a non-contiguous view: the binding's temporary
        torch.cuda.synchronize()
        dd, dg = m.query_distance(qd, world=world, outside=-2.5)
        d_only = m.query_distance(qd, world=world, outside=-2.5, grad=False)
        m.sync()
        runs.append((world, qq, hd, hg, h_only, dd.cpu().numpy(), dg.cpu().numpy(), d_only.cpu().numpy()))
    res, fut = m.results(), m.getFutureStatus()
    want_fld = D.field(cfg, res, fut, thr, 20, variant == "cubes")
    assert np.array_equal(_bits(fld), _bits(want_fld))
    for world, qq, hd, hg, h_only, dd, dg, d_only in runs:
        wd, wg = D.query(cfg, want_fld, qq, world=world, cur_pos=cur, outside=-2.5)
        for name, got, want in (("host dist", hd, wd), ("host grad", hg, wg), ("host dist only", h_only, wd), ("device dist", dd, wd),
                                ("device grad", dg, wg), ("device dist only", d_only, wd)):
            bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(qq), -1).any(1))
            assert bad.size == 0, (name, world, bad.size, bad[:5], qq[bad[:5]], got[bad[:5]], want[bad[:5]])
        inside = wd != F(-2.5)
        assert 1000 < inside.sum() < len(qq) and (wg[inside] != 0).any() and (wg[~inside] == 0).all()
    assert (np.abs(wg).max(0) > 0).all()      # every axis has a gradient somewhere
    m.close()
