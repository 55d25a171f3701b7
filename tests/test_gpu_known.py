"""GPU tests of the known-space layer (dspmap_known_integrate, dspmap_get_known, dspmap_query_known*, dspmap_mask_cast_grid,
dspmap_known_stats, dspmap_get_view): exact parity -- zero differing cells -- with the numpy restatement (tests/known_ref.py) fed with the
planes and farthest returns the map hands out (DSPMap.view()), over one frame at three attitudes, two sensor ranges and an empty cloud,
ego motion across lattice boundaries and through negative coordinates, window jumps, ageing, resets, the queries, the mask in the cast grid
and what casts, boxes and arrival fields make of it, and read-only behaviour.  The shapes are 66 x 12 x 8 (two words per row, a ragged
last word, a wrap in x inside a word), 16 x 16 x 6 and 3 x 3 x 3 (odd, a single partial wave) at 0.15 m.

The cloud is common.wall_cloud scaled about the sensor so that the wall lies inside these small maps (SCENES: the wall's distance in
metres and the sensor position, chosen on the CPU from the restatement so that every class of cell occurs).  Before it compares, every
parity test asserts on the RESTATEMENT's output that the scene is not degenerate."""
import numpy as np
import pytest
import torch

from tests import cast_ref as CR
from tests import common
from tests import corridor_ref as BR
from tests import known_ref as K
from tests import reach_ref as RR
from tests.test_gpu_cast import _assert_same_hits, _segments
from tests.test_gpu_corridor import _assert_same_boxes, _seeds
from tests.test_gpu_reach import _assert_same_fields, _free_sources

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
RES = 0.15
WIDE, CUBE, TINY = (66, 12, 8), (16, 16, 6), (3, 3, 3)
S2 = float(np.sqrt(0.5))
QUATS = {"identity": (1.0, 0.0, 0.0, 0.0), "yaw90": (S2, 0.0, 0.0, S2), "pitch_roll": (0.9799247, 0.0868241, 0.1736482, 0.0)}
# (wall distance, sensor position, fewest cells per class {seen, occluded, outside the wedge}).  WIDE at yaw90 looks along the 12-voxel
# axis: the wedge holds ~140 cells of the map in all, the wall at 0.46 m splits them; the sensor sits 7 cm off the lattice so that a row more
# of cells lies in front of it
SCENES = {
    (WIDE, "identity"): (2.0, (0.0, 0.0, 0.0), 50), (WIDE, "yaw90"): (0.46, (0.02, -0.07, 0.01), 50), (WIDE, "pitch_roll"): (2.0, (0.0, 0.0, 0.0), 50),
    (CUBE, "identity"): (0.6, (0.0, 0.0, 0.0), 30), (CUBE, "yaw90"): (0.6, (0.0, 0.0, 0.0), 30), (CUBE, "pitch_roll"): (0.6, (0.0, 0.0, 0.0), 30),
    (TINY, "identity"): (0.6, (0.0, 0.0, 0.0), 1), (TINY, "yaw90"): (0.6, (0.0, 0.0, 0.0), 1), (TINY, "pitch_roll"): (0.6, (0.0, 0.0, 0.0), 1),
}


def _cloud(dist, seed=3):
    return (common.wall_cloud(seed, n_side=40) * F(dist / 3.0)).astype(F)


def _map(dsp, shape, seed=7, **kw):
    return dsp.DSPMap(dsp.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12, seed=seed, **kw))


def _counter(dsp, m):
    return int(m.get_param(dsp.capi.P_UPDATE_COUNTER))


def _ref_integrate(dsp, lay, m, cur, max_range=np.inf):
    """the restatement's integration of the frame the map ran last, from the map's own planes and farthest returns"""
    ph, pv, ml = m.view()
    return lay.integrate(cur, ph, pv, ml, _counter(dsp, m), float(m.get_param(dsp.capi.P_OCCLUSION_MARGIN)), max_range)


def _same(got, want, tag):
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape, tag
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (tag, bad.shape[0], bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


@pytest.mark.parametrize("att", ["identity", "yaw90", "pitch_roll"])
@pytest.mark.parametrize("shape", [WIDE, CUBE, TINY], ids=["66x12x8", "16x16x6", "3x3x3"])
def test_known_one_frame(dsp, orc, shape, att):
    dist, pos, least = SCENES[(shape, att)]
    quat, pts = QUATS[att], _cloud(dist)
    m = _map(dsp, shape)
    assert (m.known_age() == -1).all() and m.known_stats(0) == (0, 0)           # before any integration, and nothing allocated for it
    assert m.update(pts, pos, 0.0, quat) == 1
    ph, pv, ml = m.view()
    o = orc.Oracle(orc.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12))
    o.bin_points(pts, quat)
    assert np.array_equal(ml.ravel(), o.obs_max_length) and (ml > 0).sum() > 100
    o.close()
    cfg, cur = m.cfg, np.array(pos, F)
    margin = float(m.get_param(dsp.capi.P_OCCLUSION_MARGIN))
    for max_range in (np.inf, 1.5):
        seen, occluded, beyond, outside = K.classify(cfg, cur, ph, pv, ml, margin, max_range)
        print(shape, att, max_range, "seen", seen.sum(), "occluded", occluded.sum(), "beyond", beyond.sum(), "outside", outside.sum())
        assert min(seen.sum(), outside.sum()) >= least                                # the scene is not degenerate
        assert occluded.sum() >= least or shape == TINY                               # (3 x 3 x 3 ends inside the occlusion margin of any wall)
        if (shape, att) == (WIDE, "identity") and max_range == 1.5:
            assert beyond.sum() >= 50
        lay = K.Layer(cfg)
        _ref_integrate(dsp, lay, m, cur, max_range)
        m.reset_known()
        m.integrate_known(max_range)
        got = m.known_age()
        _same(got, lay.ages(cur, 1), (shape, att, max_range))
        assert set(np.unique(got).tolist()) == {-1, 0}
        assert m.known_stats(0) == K.stats(got, 0) == (int(seen.sum()), int(seen.sum()))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE], ids=["66x12x8", "16x16x6"])
def test_known_empty_cloud(dsp, shape):
    """no return in any pyramid: the whole wedge is seen through, up to max_range"""
    m = _map(dsp, shape)
    assert m.update(np.zeros((0, 3), F), (0.0, 0.0, 0.0), 0.0, QUATS["identity"]) == 1
    ph, pv, ml = m.view()
    assert (ml == -1).all()
    cur = np.zeros(3, F)
    for max_range in (np.inf, 0.7):
        seen, occluded, beyond, outside = K.classify(m.cfg, cur, ph, pv, ml, 0.3, max_range)
        assert not occluded.any() and seen.sum() >= 30 and outside.sum() >= 30 and (beyond.sum() >= 30 or max_range == np.inf)
        lay = K.Layer(m.cfg)
        _ref_integrate(dsp, lay, m, cur, max_range)
        m.reset_known()
        m.integrate_known(max_range)
        _same(m.known_age(), lay.ages(cur, 1), (shape, max_range))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE, TINY], ids=["66x12x8", "16x16x6", "3x3x3"])
def test_known_ego_motion(dsp, shape):
    """twelve frames of 4 cm steps in -x and +y across lattice boundaries and through negative world coordinates, integrated one by one;
    then window moves without a frame: out and back, by exactly n cells, by n + 3 cells -- each followed by a read with no integration in
    between (the read itself has to move the window)"""
    dist = SCENES[(shape, "identity")][0]
    m = _map(dsp, shape)
    cfg, lay = m.cfg, K.Layer(m.cfg)
    pts = _cloud(dist)
    windows, seen_total = set(), 0
    for f in range(12):
        cur = np.array([0.1 - 0.04 * f, -0.2 + 0.04 * f, 0.05], F)
        att = ("identity", "pitch_roll")[f % 2]
        assert m.update(pts, cur, f / 30.0, QUATS[att]) == 1
        seen_total += int(_ref_integrate(dsp, lay, m, cur).sum())
        m.integrate_known()
        got = m.known_age()
        _same(got, lay.ages(cur, f + 1), (shape, f))
        windows.add(lay.k0)
    assert len(windows) >= 4 and min(k[0] for k in windows) < max(k[0] for k in windows) and cur[0] < 0 < cur[1]
    ages = lay.ages(cur, 12)
    assert seen_total > 12 and len(np.unique(ages)) >= (3 if shape != TINY else 2)    # cells seen in different frames, cells never seen
    n = np.array(shape)
    r = float(F(RES))

    def at(cells):
        p = (cur.astype(np.float64) + np.array(cells, np.float64) * r).astype(F)
        m.set_current_position(float(p[0]), float(p[1]), float(p[2]))
        return p

    # 5 cells out along y (min(5, n - 1) on the tiny map) and back: what left the window is forgotten
    k = min(5, shape[1] - 1)
    p = at((0, k, 0))
    assert m.known_stats(100) == K.stats(lay.ages(p, 12), 100)                        # the first read after the move is the stats call
    _same(m.known_age(), lay.ages(p, 12), (shape, "out"))
    p = at((0, 0, 0))
    back = lay.ages(p, 12)
    _same(m.known_age(), back, (shape, "back"))
    assert (back[:, :k, :] == -1).all() and np.array_equal(back[:, k:, :], ages[:, k:, :])
    assert (ages[:, :k, :] >= 0).any() and ((back >= 0).any() or shape == TINY)       # something was there to forget, something stayed
    # a query as the first read after a diagonal move
    p = at((-1, 1, 1))
    want = lay.ages(p, 12)
    z, y, x = np.meshgrid(*[(np.arange(n[a]) + 0.5) * r - n[a] * r / 2 for a in (2, 1, 0)], indexing="ij")
    q = np.stack([x, y, z, np.zeros_like(x)], -1).reshape(-1, 4).astype(F)
    assert np.array_equal(m.query_known(q).reshape(want.shape), want)
    # exactly n cells, then n + 3 cells: every slot now belongs to another cell -- nothing is known
    ph, pv, ml = m.view()
    for axis, extra in ((0, 0), (1, 3), (2, 0)):
        m.integrate_known()                                                           # something to forget: the last frame's view, at this window
        lay.integrate(p, ph, pv, ml, 12)
        _same(m.known_age(), lay.ages(p, 12), (shape, "before the jump", axis))
        assert (lay.ages(p, 12) >= 0).any() or shape == TINY                          # (27 cells: this window may hold none of the wedge)
        step = [0, 0, 0]
        step[axis] = int(n[axis]) + extra
        cur = p
        p = at(step)
        got = m.known_age()
        _same(got, lay.ages(p, 12), (shape, "jump", axis, extra))
        assert (got == -1).all()
    m.close()


def test_known_ageing_rejected_frames_and_resets(dsp):
    m = _map(dsp, CUBE)
    pts, cur = _cloud(0.6), np.zeros(3, F)
    lay = K.Layer(m.cfg)
    assert m.update(pts, cur, 0.0, QUATS["identity"]) == 1
    _ref_integrate(dsp, lay, m, cur)
    m.integrate_known()
    a1 = m.known_age()
    _same(a1, lay.ages(cur, 1), "first")
    assert (a1 == 0).sum() >= 30
    m.integrate_known()                                                               # twice is once
    assert np.array_equal(m.known_age(), a1)
    for f in (1, 2, 3):                                                               # frames without an integration: every age + 1
        assert m.update(pts, cur, f / 30.0, QUATS["yaw90"]) == 1
        assert np.array_equal(m.known_age(), np.where(a1 >= 0, a1 + f, -1))
    assert _counter(dsp, m) == 4
    view = m.view()
    assert m.update(pts, cur, -5.0, QUATS["pitch_roll"]) == 0                         # dt < 0: rejected
    assert m.update(pts, cur, 50.0, QUATS["pitch_roll"]) == 0                         # dt > 10 s: rejected
    assert _counter(dsp, m) == 4 and all(np.array_equal(a, b) for a, b in zip(view, m.view()))
    assert np.array_equal(m.known_age(), np.where(a1 >= 0, a1 + 3, -1))
    _ref_integrate(dsp, lay, m, cur)                                                  # the yaw90 view of frame 4 on top
    m.integrate_known()
    a4 = m.known_age()
    _same(a4, lay.ages(cur, 4), "fourth")
    assert set(np.unique(a4).tolist()) == {-1, 0, 3}
    assert m.known_stats(0) == K.stats(a4, 0) and m.known_stats(3) == K.stats(a4, 3) and m.known_stats(2)[0] < m.known_stats(3)[0]
    m.reset_known()
    assert (m.known_age() == -1).all() and m.known_stats(1000) == (0, 0)
    m.integrate_known()
    assert np.array_equal(m.known_age() == 0, a4 == 0)
    m.clear_state()
    assert (m.known_age() == -1).all()
    m.close()
    fresh = _map(dsp, CUBE)                                                           # no accepted frame: nothing to integrate
    assert fresh.L.dspmap_known_integrate(fresh.h, 5.0, 0) == E_STATE and b"dspmap_update" in fresh.L.dspmap_last_error(fresh.h)
    fresh.close()


def test_known_queries(dsp):
    m = _map(dsp, WIDE)
    cfg, cur = m.cfg, np.array([0.31, -0.12, 0.02], F)
    pts = _cloud(2.0)
    assert m.update(pts, cur, 0.0, QUATS["identity"]) == 1
    m.integrate_known()
    assert m.update(pts, cur, 0.1, QUATS["pitch_roll"]) == 1
    assert m.update(pts, cur, 0.2, QUATS["pitch_roll"]) == 1
    m.integrate_known()
    ages = m.known_age()
    assert set(np.unique(ages).tolist()) == {-1, 0, 2}
    res = F(RES)
    half = np.array(common.half_extent(cfg), F)
    n = np.array(WIDE)
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    idx = np.stack([x, y, z], -1).reshape(-1, 3)
    centres = ((idx.astype(F) * res).astype(F) + (-half + res * F(0.5)).astype(F)).astype(F)       # dspmap_voxel_center
    t = np.resize(np.array([0.0, -1.0, np.nan, 7.0], F), len(centres))                              # t is ignored, NaN included
    qc = np.concatenate([centres, t[:, None]], 1).astype(F)
    assert np.array_equal(m.query_known(qc).reshape(ages.shape), ages)
    rng = np.random.default_rng(5)
    faces = centres[rng.integers(0, len(centres), 600)].copy()
    ax = rng.integers(0, 3, 600)
    faces[np.arange(600), ax] = (faces[np.arange(600), ax] + res * F(0.5) * rng.choice([-1, 1], 600).astype(F)).astype(F)
    outside = (rng.uniform(-1.3, 1.3, (600, 3)) * half).astype(F)
    outside[:6] = np.array([[half[0], 0, 0], [-half[0], 0, 0], [0, half[1], 0], [0, 0, -half[2]], [1e30, 0, 0], [np.inf, 0, 0]], F)
    nan = centres[:6].copy()
    nan[np.arange(6), np.arange(6) % 3] = np.nan
    q = np.concatenate([np.concatenate([faces, outside, nan]), np.zeros((1206, 1), F)], 1).astype(F)
    want = K.query(cfg, ages, q)
    got = m.query_known(q)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want[:600] >= 0).sum() > 20 and (want[600:1200] == -1).sum() > 100 and (want[600:1200] >= 0).sum() > 5 and (want[1200:] == -1).all()
    qw = q.copy()
    qw[:, :3] = (qw[:, :3] + cur[None, :]).astype(F)
    want_w = K.query(cfg, ages, qw, world=True, cur_pos=cur)
    assert np.array_equal(m.query_known(qw, world=True), want_w) and (want_w >= 0).sum() > 20
    for world, qq, w in ((False, q, want), (True, qw, want_w)):
        qd = torch.from_numpy(np.concatenate([qq, qq], 1)).cuda()[:, :4]                # a non-contiguous view: the binding's temporary
        torch.cuda.synchronize()
        dev = m.query_known(qd, world=world)
        m.sync()
        assert dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), w)
    m.close()
    blank = _map(dsp, CUBE)                                                            # never integrated: nothing is known, on both routes
    qd = torch.zeros((5, 4), dtype=torch.float32, device="cuda")
    assert (blank.query_known(np.zeros((5, 4), F)) == -1).all()
    dev = blank.query_known(qd)
    blank.sync()
    assert (dev.cpu().numpy() == -1).all()
    blank.close()


def _aged_scene(dsp, shape, dist):
    """five frames of the wall cloud, integrated after the first, the second and the fifth (three attitudes): ages 0, 3, 4 and -1"""
    m = _map(dsp, shape)
    cur = np.array([0.05, -0.03, 0.0], F)
    pts = _cloud(dist)
    for f, att in enumerate(("identity", "yaw90", "identity", "identity", "pitch_roll")):
        assert m.update(pts, cur, f / 30.0, QUATS[att]) == 1
        if f in (0, 1, 4):
            m.integrate_known()
    return m, cur


@pytest.mark.parametrize("inflate", [0, 2])
def test_known_mask_in_cast_grid(dsp, inflate):
    m, cur = _aged_scene(dsp, WIDE, 2.0)
    cfg, L = m.cfg, m.T + 1
    ages = m.known_age()
    assert set(np.unique(ages).tolist()) == {-1, 0, 3, 4}
    mass = m.results()[:, 0]
    thr = float(np.median(mass[mass > 0]))
    seg = _segments(cfg, 3000, 7)
    seeds = _seeds(cfg, 1500, 9)
    layers = {}
    for max_age in (0, 3):
        m.build_cast_grid(thr, inflate)
        old = m.cast_grid()
        src = _free_sources(cfg, RR.unpack(old, cfg.nx) | K.unknown(ages, max_age)[None], 2, 11)
        m.build_reach_fields(src, 2, t_start=-1.0, step_seconds=0.0, max_steps=200)
        assert m.reach_fields_ptr() is not None
        m.mask_cast_grid(max_age)
        assert m.reach_fields_ptr() is None                                           # grown in the grid as it was: stale
        with pytest.raises(dsp.capi.DSPMapError):
            m.reach_field(0)
        new = m.cast_grid()
        unknown = K.unknown(ages, max_age)
        want = old | CR.pack(unknown)[None]
        assert new.shape == want.shape == (L, WIDE[2], WIDE[1], 2)
        bad = np.flatnonzero(new != want)
        assert bad.size == 0, (max_age, bad.size, bad[:5])
        assert not (new[..., -1] >> np.uint64(WIDE[0] & 63)).any()                   # bits at x >= nx stay 0
        assert 100 < unknown.sum() < unknown.size - 100 and (new != old).any() and (old != 0).any()
        lay = RR.unpack(new, cfg.nx)
        layers[max_age] = lay
        assert np.array_equal(lay, RR.unpack(old, cfg.nx) | unknown[None])           # unknown space is not inflated
        for world in (False, True):
            ss = seg.copy()
            if world:
                ss[:, 0:3], ss[:, 4:7] = (ss[:, 0:3] + cur[None, :]).astype(F), (ss[:, 4:7] + cur[None, :]).astype(F)
            got = m.cast_segments(ss, world=world)
            _assert_same_hits(got, CR.cast(cfg, lay, ss, world=world, cur_pos=cur), ss, (max_age, world))
        assert {CR.FREE, CR.HIT} <= set(got["status"].tolist())
        gotb = m.grow_boxes(seeds, (8, 8, 4))
        wantb = BR.grow(cfg, lay, seeds, (8, 8, 4))
        _assert_same_boxes(gotb, wantb, seeds, max_age)
        assert {BR.OK, BR.SEED_BLOCKED} <= set(wantb["status"].tolist())
        m.build_reach_fields(src, 2, t_start=-1.0, step_seconds=0.0, max_steps=200)
        wantf = RR.fields(cfg, lay, src, 2, t_start=-1.0, step_seconds=0.0, max_steps=200)
        _assert_same_fields(m.reach_field(None, 2), wantf, max_age)
        assert (wantf == RR.UNREACHED).any() and (wantf[wantf != RR.UNREACHED] > 3).any()
        assert (wantf[:, unknown] == RR.UNREACHED).all()                              # no front enters unknown space
    assert (layers[0] != layers[3]).any()                                             # the age limit changes the grid
    # a second mask with a wider limit adds nothing; the life cycle
    m.mask_cast_grid(1000)
    assert np.array_equal(RR.unpack(m.cast_grid(), cfg.nx), layers[3] | (ages < 0)[None])
    assert m.update(_cloud(2.0), cur, 1.0, QUATS["identity"]) == 1                    # the grid is stale now
    assert m.L.dspmap_mask_cast_grid(m.h, 0, 0) == E_STATE and b"dspmap_build_cast_grid" in m.L.dspmap_last_error(m.h)
    m.build_cast_grid(thr, inflate)
    m.reset_known()
    assert m.L.dspmap_mask_cast_grid(m.h, 0, 0) == E_STATE and b"dspmap_known_integrate" in m.L.dspmap_last_error(m.h)
    m.close()
    fresh = _map(dsp, CUBE)
    assert fresh.update(_cloud(0.6), (0.0, 0.0, 0.0), 0.0, QUATS["identity"]) == 1
    fresh.build_cast_grid(0.1, 0)
    assert fresh.L.dspmap_mask_cast_grid(fresh.h, 0, 0) == E_STATE and b"dspmap_known_integrate" in fresh.L.dspmap_last_error(fresh.h)
    fresh.close()


def test_known_is_read_only(dsp):
    """twins fed the same frames: one interleaves every known-space call, the other none; results, future status, counters and the
    exported particles stay bit-identical"""
    maps = []
    for _ in range(2):
        m = _map(dsp, CUBE, seed=99)
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        maps.append(m)
    a, b = maps
    pts = [_cloud(0.6, seed=s) for s in range(6)]
    q = np.concatenate([(np.random.default_rng(1).uniform(-1, 1, (200, 3)) * np.array(common.half_extent(a.cfg))), np.zeros((200, 1))], 1).astype(F)
    for f in range(6):
        cur = (0.03 * f, -0.02 * f, 0.0)
        for m in (a, b):
            assert m.update(pts[f], cur, f / 30.0, QUATS[("identity", "yaw90", "pitch_roll")[f % 3]]) == 1
        if f >= 3:
            a.integrate_known(2.0 if f == 4 else float("inf"))
            a.known_age(), a.query_known(q, world=True), a.known_stats(1), a.view()
            a.build_cast_grid(0.05, 1)
            a.mask_cast_grid(1)
            a.cast_segments(_segments(a.cfg, 200, 3))
        if f == 2:
            assert np.array_equal(a.results(), b.results())
    assert (a.known_age() >= 0).sum() >= 30
    assert np.array_equal(a.results(), b.results()) and (a.results()[:, 0] > 0).any()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    ca, cb = a.counters(), b.counters()
    ca.pop("update_ms"), cb.pop("update_ms")
    assert ca == cb
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    assert b.cast_grid_ptr() is None and (b.known_age() == -1).all()
    a.close(), b.close()
