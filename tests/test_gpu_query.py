"""GPU tests of the point / trajectory queries (dspmap_query_occupancy*, dspmap_trajectory_risk*): bit parity of the host and device
entry points with the numpy restatement (tests/query_ref.py) over what the map hands out, read-only behaviour, the per-trajectory
risk (also past one 32-sample chunk and one 256-trajectory block of k_risk_reduce, at radius 0, with an infinite outside value, at a
threshold that occurs, and across regrowth of the handle's scratch), slab handles merged with max, and stream order behind the frame."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import common
from tests import query_ref as Q

pytestmark = pytest.mark.gpu
F = np.float32
B = dict(nx=66, ny=66, nz=40, res=0.15, ppv=24)


def _scene_frames(dsp, kw, n, seed=1234):
    scene = importlib.import_module("dsp-map_amd.scene")
    sc = scene.CorridorScene(kw["nx"] * kw["res"], kw["ny"] * kw["res"], kw["nz"] * kw["res"], seed=seed, device="cuda")
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        out = [sc.frame(f / 30.0) + (f / 30.0,) for f in range(n)]
    finally:
        torch.use_deterministic_algorithms(was)
    torch.cuda.synchronize()
    return out


def _run(m, frames):
    for f, (pts, pos, quat, t) in enumerate(frames):
        if f:
            m.clearOccupancyMapPrediction()   # (once per frame, :429-438; not after the last one: its future status is queried)
        assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
    return np.array(frames[-1][1], F)


def _samples(cfg, n, seed):
    """n samples over 1.1 x the map box: uniform points, voxel centres, voxel faces, NaN; every class of t"""
    rng = np.random.default_rng(seed)
    hx, hy, hz = common.half_extent(cfg)
    half = np.array([hx, hy, hz], F)
    res = F(cfg.voxel_resolution)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    p = (rng.uniform(-1.1, 1.1, (n, 3)) * half).astype(F)
    idx = rng.integers(0, nn, (n, 3))
    corr = (-half + res * F(0.5)).astype(F)
    centres = (idx.astype(F) * res + corr).astype(F)
    a, b = n // 5, 2 * (n // 5)
    p[:a] = centres[:a]                                                     # lattice centres
    faces = centres[a:b].copy()
    ax = rng.integers(0, 3, b - a)
    faces[np.arange(b - a), ax] = (faces[np.arange(b - a), ax] + res * F(0.5)).astype(F)   # a voxel face
    p[a:b] = faces
    pred = np.array([cfg.prediction_future_time[k] for k in range(cfg.prediction_times)], F)
    mids = ((pred[:-1] + pred[1:]) * F(0.5)).astype(F)
    tclass = np.concatenate([[-1.0, -0.0, 0.0, 5.0, np.inf], pred, mids]).astype(F)
    t = tclass[rng.integers(0, len(tclass), n)]
    q = np.concatenate([p, t[:, None]], 1).astype(F)
    nan = rng.random((n, 4)) < 0.003
    q[nan] = np.nan
    return q


def _check_parity(m, cfg, cur_pos, q, radii, world_too=True):
    """host == device == restatement over results() / getFutureStatus() read afterwards, for every radius (and the world flag)"""
    runs = []
    for r in radii:
        sub = q if r <= 0.31 else q[:4000]   # (the widest radius: fewer samples, the restatement's box is 21^3)
        for world in ((False, True) if world_too else (False,)):
            qq = sub.copy()
            if world:
                qq[:, :3] = (qq[:, :3] + cur_pos[None, :]).astype(F)
            host = m.query_occupancy(qq, radius=r, world=world, outside=0.75)
            qd = torch.from_numpy(np.concatenate([qq, qq], 1)).cuda()[:, :4]   # a non-contiguous view: the binding's temporary
            torch.cuda.synchronize()   # (the copy ran on torch's stream, the query runs on the handle's)
            dev = m.query_occupancy(qd, radius=r, world=world, outside=0.75)
            m.sync()
            runs.append((r, world, qq, host, dev.cpu().numpy()))
    res, fut = m.results(), m.getFutureStatus()
    for r, world, qq, host, dev in runs:
        want, _ = Q.query(cfg, res, fut, qq, radius=r, world=world, cur_pos=cur_pos, outside=0.75)
        assert np.array_equal(host, dev), (r, world)
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (r, world, bad[:5], qq[bad[:5]], host[bad[:5]], want[bad[:5]])
    return res, fut


@pytest.mark.parametrize("variant", ["runs", "cubes", "nb2_angle1", "static"])
def test_query_bit_parity(dsp, variant):
    kw = dict(B)
    if variant == "nb2_angle1":
        kw.update(neighbor_n=2, angle=1)
    if variant == "static":
        kw.update(static_model=1)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    if variant in ("runs", "cubes"):
        m.set_param(dsp.capi.P_TILING, 1 if variant == "cubes" else 0)
    m.seed_uniform(2, 0.01, 99, vmax=0.0 if variant == "static" else 1.0)
    cur = _run(m, _scene_frames(dsp, kw, 12))
    if variant in ("runs", "cubes"):
        assert int(m.get_param(dsp.capi.P_TILING)) == (1 if variant == "cubes" else 0)
    assert np.abs(cur).max() > 0
    q = _samples(cfg, 50000, 7)
    res_f = float(F(cfg.voxel_resolution))
    radii = [0.0, float(F(0.5) * F(res_f)), res_f, 0.3, float(F(8) * F(res_f))]
    res, fut = _check_parity(m, cfg, cur, q, radii)
    assert (res[:, 0] > 0).sum() > 10000
    if variant != "static":
        assert (fut[:, 0] != fut[:, -1]).sum() > 100     # the horizons differ: moving mass
    m.close()


def _all_queries(m, q, traj):
    qd, td = torch.from_numpy(q).cuda(), torch.from_numpy(traj).cuda()
    torch.cuda.synchronize()
    a = m.query_occupancy(q, radius=0.3)
    b = m.query_occupancy(qd, radius=0.3, world=True)
    c = m.trajectory_risk(traj, radius=0.15)
    d = m.trajectory_risk(td)
    m.sync()
    return a, b, c, d


def test_query_is_read_only(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    frames = _scene_frames(dsp, kw, 10, seed=77)
    maps = []
    for _ in range(2):
        m = dsp.DSPMap(dsp.make_config(seed=99, **kw))
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        maps.append(m)
    a, b = maps
    cfg = a.cfg
    q = _samples(cfg, 4000, 3)
    traj = _samples(cfg, 64 * 16, 4).reshape(64, 16, 4)
    for pts, pos, quat, t in frames:
        for m in maps:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        _all_queries(a, q, traj)
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    # within one frame: a query before getFutureStatus matches the grid it returns; afterwards t >= 0 reads 0, t < 0 is unchanged
    cur = np.array(frames[-1][1], F)
    before = a.query_occupancy(q, radius=0.3)
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra, rb)
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb)
    want, _ = Q.query(cfg, ra, fa, q, radius=0.3, cur_pos=cur, outside=1.0)
    assert np.array_equal(before, want)
    after = a.query_occupancy(q, radius=0.3)
    tneg = np.nan_to_num(q[:, 3], nan=-1.0) < 0
    nan = np.isnan(q).any(1)
    zero, _ = Q.query(cfg, ra, np.zeros_like(fa), q, radius=0.3, outside=1.0)
    assert np.array_equal(after, zero)
    assert np.array_equal(after[tneg & ~nan], before[tneg & ~nan])
    assert (fa != 0).any() and not np.array_equal(after, before)
    for m in maps:
        m.close()


def test_trajectory_risk(dsp):
    kw = dict(B)
    cfg = dsp.make_config(seed=1234, **kw)
    m = dsp.DSPMap(cfg)
    m.seed_uniform(2, 0.01, 99, vmax=1.0)
    cur = _run(m, _scene_frames(dsp, kw, 8))
    rng = np.random.default_rng(11)
    K, S = 1024, 24
    hx, hy, hz = common.half_extent(cfg)
    start = (rng.uniform(-0.9, 0.9, (K, 3)) * np.array([hx, hy, hz])).astype(F)
    vel = rng.uniform(-1.5, 1.5, (K, 3)).astype(F)
    ts = np.linspace(-0.1, 2.2, S).astype(F)
    traj = np.empty((K, S, 4), F)
    traj[:, :, :3] = (start[:, None, :] + vel[:, None, :] * ts[None, :, None]).astype(F)   # straight lines, some leave the map
    traj[:, :, 3] = ts[None, :]
    traj[:7, 5, 0] = np.nan
    got = [m.trajectory_risk(traj, radius=0.3, outside=2.0, threshold=0.05) for _ in range(2)]
    td = torch.from_numpy(traj).cuda()
    torch.cuda.synchronize()
    dev = m.trajectory_risk(td, radius=0.3, outside=2.0, threshold=0.05)
    m.sync()
    assert got[0].tobytes() == got[1].tobytes()
    for k in ("sum", "max", "first_over", "n_outside"):
        d = dev[k].cpu().numpy()
        assert d.tobytes() == np.ascontiguousarray(got[0][k]).tobytes(), k
    vals, flags = Q.query(cfg, m.results(), m.getFutureStatus(), traj.reshape(-1, 4), radius=0.3, cur_pos=cur, outside=2.0)
    s, mx, first, nout = Q.risk(vals, flags, S, threshold=0.05)
    assert s.tobytes() == got[0]["sum"].tobytes()
    assert np.array_equal(mx, got[0]["max"]) and np.array_equal(first, got[0]["first_over"]) and np.array_equal(nout, got[0]["n_outside"])
    assert 50 < (nout > 0).sum() < K and (first >= 0).sum() > 50
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# k_risk_reduce past one chunk of RISK_CHUNK = 32 samples and one block of 256 trajectories, and k_query<false, true> (radius 0 with flags).
# One map (40 x 40 x 24, 12 particles per voxel, seeded with moving particles, eight frames of the corridor scene) and one pool of
# RISK_POOL samples whose values the restatement computes ONCE per radius; every case's trajectories are rows of pool indices, so its
# reference is a gather.  The first rows are designed from the restatement's values (LOW: inside, value <= threshold at radius 0.3 and
# so at radius 0; HIGH: inside, own voxel > threshold, so over at both radii; OUT: flagged) so that first_over falls where k_risk_reduce
# can go wrong: at the last sample, never, in chunk 0, at 31 | 32 | 33, at 63 | 64 | 65 and beyond, and n_outside is 0 and n_samples.
RISK_KW = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
RISK_POOL = 600 * 100
RISK_OUTSIDE = 0.75
RISK_RADII = [0.0, 0.3]
RISK_S, RISK_K = [1, 31, 32, 33, 64, 65, 100], [1, 255, 256, 257, 600]
RISK_SHAPES = sorted(set([(k, s) for s in RISK_S for k in (257, 1)] + [(k, s) for k in RISK_K for s in (33, 100)]))
# row -> the designed first_over (S - 1: the last sample; None: all LOW; "out": all OUT); a design applies where its row and sample exist
RISK_DESIGN = ["last", None, "out", 32, 0, 31, 33, 64, 65, 63, 70, 5]


def _risk_map(dsp, frames):
    m = dsp.DSPMap(dsp.make_config(seed=99, **RISK_KW))
    m.set_tables(*common.tables(5))
    m.seed_uniform(2, 0.01, 17, vmax=0.8)
    return m, _run(m, frames)


def _future_in_place(dsp, m):
    """the [V, T] future status without the readout's side effect (dspmap_future_device: no clear is armed)"""
    ptr = m.L.dspmap_future_device(m.h)
    assert ptr
    fut = torch.as_tensor(dsp.capi._DeviceSpan(ptr, (m.V, m.T), "<f4"), device="cuda")
    m.sync()
    return fut.cpu().numpy()


class _Risk:
    pass


@pytest.fixture(scope="module")
def risk(dsp):
    """the handle, what it hands out, the pool and the restatement's values of the pool at both radii"""
    r = _Risk()
    r.frames = _scene_frames(dsp, RISK_KW, 8, seed=77)
    r.m, r.cur = _risk_map(dsp, r.frames)
    twin, _ = _risk_map(dsp, r.frames)
    m, cfg = r.m, r.m.cfg
    r.res, r.fut = m.results(), _future_in_place(dsp, m)
    assert np.array_equal(r.res, twin.results()) and np.array_equal(r.fut, twin.getFutureStatus())   # the in-place view IS what the readout gives
    twin.close()
    mass = r.res[:, 0]
    assert (mass > 0.2).any() and len(np.unique(mass)) > 50 and (r.fut[:, 0] != r.fut[:, -1]).sum() > 100   # masses and horizons non-trivial
    r.pool = _samples(cfg, RISK_POOL, 4)
    r.vals, r.flags = {}, None
    for rad in RISK_RADII:
        v, f = Q.query(cfg, r.res, r.fut, r.pool, radius=rad, cur_pos=r.cur, outside=RISK_OUTSIDE)
        assert r.flags is None or np.array_equal(f, r.flags)
        r.vals[rad], r.flags = v, f
    v0, v3, inside = r.vals[0.0], r.vals[0.3], ~r.flags
    assert (v3[inside] >= v0[inside]).all()
    r.thr = float(np.quantile(v3[inside], 0.5))                          # half of the inside samples are LOW at radius 0.3: non-empty by construction
    assert r.thr < RISK_OUTSIDE                                          # a flagged sample is over the threshold
    r.low = np.flatnonzero(inside & (v3 <= F(r.thr)))
    r.high = np.flatnonzero(inside & (v0 > F(r.thr)))
    r.out = np.flatnonzero(r.flags)
    assert len(r.low) > 1000 and len(r.high) >= 20 and len(r.out) > 1000
    yield r
    r.m.close()


def _risk_rows(r, K, S, seed=0):
    """[K, S] pool indices: consecutive pool samples, the first rows overwritten by the designs that fit"""
    rng = np.random.default_rng(1000 * K + S + seed)
    src = np.arange(K * S).reshape(K, S)
    designed = {}
    for row, what in enumerate(RISK_DESIGN[:K]):
        f = S - 1 if what == "last" else what
        if what == "out":
            src[row] = rng.choice(r.out, S)
        elif f is None:
            src[row] = rng.choice(r.low, S)
        elif f < S:
            src[row, :f] = rng.choice(r.low, f)
            src[row, f] = rng.choice(r.high)
        else:
            continue
        designed[row] = what
    return src, designed


def _risk_want(r, src, radius, threshold):
    S = src.shape[1]
    return Q.risk(r.vals[radius][src.ravel()], r.flags[src.ravel()], S, threshold=threshold)


def _risk_covered(K, S, designed, first, nout):
    """the coverage conditions, on the restatement's output"""
    for row, what in designed.items():
        if what == "out":
            assert nout[row] == S and first[row] == 0, (row, what)
        elif what is None:
            assert nout[row] == 0 and first[row] == -1, (row, what)
        else:
            assert first[row] == (S - 1 if what == "last" else what), (row, what, first[row])
    if K >= len(RISK_DESIGN):
        assert (first == -1).any() and ((first >= 0) & (first <= 31)).any() and (nout == S).any() and (nout == 0).any()
        if S > 32:
            assert (first == 32).any()
        if S > 33:
            assert (first > 32).any()
        if S > 65:
            assert (first > 64).any()


def _risk_both(m, traj, **kw):
    """host and device entry points: identical bytes; returns the host's records"""
    host = m.trajectory_risk(traj, **kw)
    td = torch.from_numpy(traj).cuda()
    torch.cuda.synchronize()
    dev = m.trajectory_risk(td, **kw)
    m.sync()
    for k in ("sum", "max", "first_over", "n_outside"):
        assert dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(host[k]).tobytes(), k
    return host


def _risk_same(got, want, tag):
    s, mx, first, nout = want
    assert got["sum"].tobytes() == s.tobytes(), (tag, "sum", np.flatnonzero(got["sum"].view(np.uint32) != s.view(np.uint32))[:5])
    assert np.array_equal(mx, got["max"]), (tag, "max", np.flatnonzero(mx != got["max"])[:5])
    assert np.array_equal(first, got["first_over"]), (tag, "first_over", np.flatnonzero(first != got["first_over"])[:5])
    assert np.array_equal(nout, got["n_outside"]), (tag, "n_outside", np.flatnonzero(nout != got["n_outside"])[:5])


@pytest.mark.parametrize("radius", RISK_RADII)
@pytest.mark.parametrize("K,S", RISK_SHAPES, ids=["%dx%d" % ks for ks in RISK_SHAPES])
def test_trajectory_risk_chunks_and_blocks(dsp, risk, K, S, radius):
    r = risk
    src, designed = _risk_rows(r, K, S)
    want = _risk_want(r, src, radius, r.thr)
    _risk_covered(K, S, designed, want[2], want[3])
    traj = np.ascontiguousarray(r.pool[src])
    got = _risk_both(r.m, traj, radius=radius, outside=RISK_OUTSIDE, threshold=r.thr)
    _risk_same(got, want, (K, S, radius))
    assert np.array_equal(r.m.results(), r.res) and np.array_equal(_future_in_place(dsp, r.m), r.fut)   # what the reference was computed from


@pytest.mark.parametrize("radius", RISK_RADII)
def test_trajectory_risk_threshold_is_strict(dsp, risk, radius):
    """a threshold equal to a value that occurs: that sample is not over"""
    r = risk
    K, S = 257, 33
    src, _ = _risk_rows(r, K, S)
    v = r.vals[radius][src.ravel()].reshape(K, S)
    vals, counts = np.unique(v[(v > 0) & (v < F(RISK_OUTSIDE))], return_counts=True)
    thr = float(vals[counts.argmax()])                                   # the most frequent positive value of these trajectories
    want = _risk_want(r, src, radius, thr)
    ge = v >= F(thr)
    first_ge = np.where(ge.any(1), ge.argmax(1), -1)
    assert (first_ge != want[2]).sum() >= 5                              # trajectories that a >= in place of > would answer differently
    got = _risk_both(r.m, np.ascontiguousarray(r.pool[src]), radius=radius, outside=RISK_OUTSIDE, threshold=thr)
    _risk_same(got, want, ("strict", radius))


@pytest.mark.parametrize("radius", RISK_RADII)
def test_trajectory_risk_outside_infinite(dsp, risk, radius):
    """outside = +inf: sum and max are inf where a sample lies outside; first_over is the first such sample unless one is over earlier"""
    r = risk
    K, S = 257, 33
    src, _ = _risk_rows(r, K, S)
    traj = np.ascontiguousarray(r.pool[src])
    vals, flags = Q.query(r.m.cfg, r.res, r.fut, traj.reshape(-1, 4), radius=radius, cur_pos=r.cur, outside=np.inf)
    want = Q.risk(vals, flags, S, threshold=r.thr)
    s, mx, first, nout = want
    fl = flags.reshape(K, S)
    has = fl.any(1)
    assert has.sum() > 20 and (~has).sum() >= 1
    assert np.isinf(s[has]).all() and np.isinf(mx[has]).all() and (s[has] > 0).all()
    if radius == 0.0:
        assert np.isfinite(s[~has]).all()                                # (with a radius, a lattice point outside the map reads inf too)
    first_out = fl.argmax(1)
    assert (first[has] <= first_out[has]).all() and (first[has] == first_out[has]).any() and (first[has] < first_out[has]).any()
    got = _risk_both(r.m, traj, radius=radius, outside=float("inf"), threshold=r.thr)
    _risk_same(got, want, ("inf", radius))


def test_trajectory_risk_scratch_regrows(dsp, risk):
    """a fresh handle: a small K x S, a large one, the small one again through the device entry point (which regrows the handle's scratch),
    then the same through the host entry point"""
    r = risk
    m, _ = _risk_map(dsp, r.frames)
    assert np.array_equal(m.results(), r.res) and np.array_equal(_future_in_place(dsp, m), r.fut)   # the fixture's state: its values hold here
    shapes = [(3, 5), (600, 100), (3, 5), (257, 65), (1, 1)]
    for device in (True, False):
        for K, S in shapes:
            src, _ = _risk_rows(r, K, S, seed=7)
            traj = np.ascontiguousarray(r.pool[src])
            want = _risk_want(r, src, 0.3, r.thr)
            if device:
                td = torch.from_numpy(traj).cuda()
                torch.cuda.synchronize()
                d = m.trajectory_risk(td, radius=0.3, outside=RISK_OUTSIDE, threshold=r.thr)
                m.sync()
                got = {k: d[k].cpu().numpy() for k in d}
            else:
                got = m.trajectory_risk(traj, radius=0.3, outside=RISK_OUTSIDE, threshold=r.thr)
            _risk_same(got, want, ("regrow", device, K, S))
    m.close()


def _slab_stream(n_frames, seed=5):
    rng = np.random.default_rng(seed)
    ys, zs = np.meshgrid(np.linspace(-2.0, 2.0, 41), np.linspace(-1.0, 1.0, 21))
    base = np.stack([np.full(ys.size, 2.2) + 0.2 * np.sin(2 * ys.ravel()), ys.ravel(), zs.ravel()], 1).astype(np.float32)
    for f in range(n_frames):
        t = f / 30.0
        yield base + rng.normal(0, 0.005, base.shape).astype(np.float32), (0.4 * t, 0.0, 0.1 * np.sin(5 * t)), t, (1.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("world", [2, 4])
def test_query_slabs_merge_with_max(dsp, world):
    sharded = __import__("dsp-map_amd.sharded", fromlist=["CppGroup"])
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    tables = common.tables(3)
    grp = sharded.CppGroup(dsp, kw, world)
    for m in grp.maps:
        m.set_tables(*tables)
    full = dsp.DSPMap(dsp.make_config(**kw))
    full.set_tables(*tables)
    for f, (pts, pos, t, q) in enumerate(_slab_stream(6)):
        d = torch.from_numpy(pts).cuda()
        assert grp.update(d, pos, t, q) == 1
        assert full.update_device(d.data_ptr(), len(pts), pos, t, q) == 1
        grp.sync()
        if f < 5:
            for m in grp.maps + [full]:
                m.clearOccupancyMapPrediction()
    cfg = full.cfg
    qs = _samples(cfg, 20000, 21)
    for r in (0.0, 0.3):
        for w in (False, True):
            parts = [m.query_occupancy(qs, radius=r, world=w) for m in grp.maps]
            want = full.query_occupancy(qs, radius=r, world=w)
            assert np.array_equal(np.maximum.reduce(parts), want), (r, w)
            assert all((p == -np.inf).any() for p in parts)     # samples with nothing on a slab
    res, fut = full.results(), full.getFutureStatus()
    assert np.array_equal(full.query_occupancy(qs, radius=0.3), Q.query(cfg, res, np.zeros_like(fut), qs, radius=0.3)[0])
    L = grp.maps[0].L
    rk = np.zeros(2, dsp.capi.RISK_DTYPE)
    tr = np.ascontiguousarray(qs[:8])
    assert L.dspmap_trajectory_risk(grp.maps[0].h, 2, 4, tr.ctypes.data_as(C.c_void_p), 0.0, 0, 1.0, 0.5, rk.ctypes.data_as(C.c_void_p)) == -3
    grp.close(); full.close()


def test_query_stream_ordered_behind_frame(dsp):
    kw = dict(nx=40, ny=40, nz=24, res=0.15, ppv=12)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    m = dsp.DSPMap(dsp.make_config(seed=5, **kw))
    m.set_tables(*common.tables(9))
    m.seed_uniform(2, 0.01, 3, vmax=1.0)
    q = torch.from_numpy(_samples(m.cfg, 20000, 13)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            outs.append(m.query_occupancy(q, radius=0.3))          # no synchronisation between the frame and the query
            outs.append(m.trajectory_risk(q.view(-1, 20, 4), radius=0.15)["sum"])
        st.synchronize()
        after = m.query_occupancy(q, radius=0.3)
        after_r = m.trajectory_risk(q.view(-1, 20, 4), radius=0.15)["sum"]
        st.synchronize()
    assert torch.equal(outs[-2], after) and torch.equal(outs[-1], after_r)
    assert not torch.equal(outs[0], outs[-2])
    m.close()
