"""GPU tests of the viewpoint scores (dspmap_score_views*, dspmap_view_rays, dspmap_debug_view_cells): exact parity -- zero differing
integers -- with the numpy restatement (tests/view_ref.py), fed with the planes and ray directions the device makes of every attitude
(DSPMap.view_rays), the layers of the cast grid as set (DSPMap.set_cast_grid) and the ages the known-space layer hands out
(DSPMap.known_age).  The shapes are those of test_gpu_known.py at 0.15 m: 66 x 12 x 8 (two words per row, a ragged last word),
16 x 16 x 6 (one word) and 3 x 3 x 3 (a single partial wave); the configuration has six horizons, so that t selects among layers that
differ.

The scene: four frames of the scaled wall cloud, integrated after the first (yaw 90 degrees), the second (yaw 180) and the fourth
(identity), so that about half the window is known, the ages are -1, 0, 2 and 3, and max_age = 2 decides something; then the cast grid is REPLACED by layers made on the host -- a wall at 0.8 nx with
random holes, different in every layer.  Before it compares, every parity test asserts on the RESTATEMENT's output that the scene is not
degenerate."""
import numpy as np
import pytest
import torch

from tests import cast_ref as CR
from tests import common
from tests import known_ref as K
from tests import view_ref as V

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
RES = 0.15
WIDE, CUBE, TINY = (66, 12, 8), (16, 16, 6), (3, 3, 3)
SHAPES = [WIDE, CUBE, TINY]
IDS = ["66x12x8", "16x16x6", "3x3x3"]
S2 = float(np.sqrt(0.5))
QUATS = {"identity": (1.0, 0.0, 0.0, 0.0), "yaw90": (S2, 0.0, 0.0, S2), "pitch_roll": (0.9799247, 0.0868241, 0.1736482, 0.0)}
# the attitudes of the candidate views: the three above, two of them scaled (the rotation divides by the squared norm), a yaw of 180 degrees
VIEW_QUATS = [QUATS["identity"], QUATS["yaw90"], QUATS["pitch_roll"], (2.0, 0.0, 0.0, 0.0), tuple(0.5 * c for c in QUATS["pitch_roll"]),
              (0.0, 0.0, 0.0, 1.0), (0.9914449, 0.0, 0.0, -0.1305262)]
WALL_DIST = {WIDE: 4.0, CUBE: 0.9, TINY: 0.6}
YAW180 = (0.0, 0.0, 0.0, 1.0)
MAX_AGE = 2
INF = float("inf")
T_BETWEEN, T_PAST = 0.1, 5.0                                                          # between the horizons 0.05 and 0.2; past the last (2.0)


def _cloud(dist, seed=3):
    return (common.wall_cloud(seed, n_side=40) * F(dist / 3.0)).astype(F)


def _map(dsp, shape, seed=7, **kw):
    return dsp.DSPMap(dsp.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12, seed=seed, **kw))


def _layers(shape, L, seed=5):
    """bool [L, nz, ny, nx]: a wall at x = floor(0.8 nx) with random holes, different per layer; row y = 0 of the wall has no holes"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    lay = np.zeros((L, nz, ny, nx), bool)
    xw = int(0.8 * nx)
    lay[:, :, :, xw] = rng.random((L, nz, ny)) > 0.3
    lay[:, :, 0, xw] = True
    return lay


def _set_grid(m, lay):
    m.build_cast_grid(0.5, 0)
    m.set_cast_grid(CR.pack(lay))


def _scene(dsp, shape, cur=(0.0, 0.0, 0.0)):
    m = _map(dsp, shape)
    pts = _cloud(WALL_DIST[shape])
    for f, quat in enumerate((QUATS["yaw90"], YAW180, QUATS["identity"], QUATS["identity"])):
        assert m.update(pts, cur, f / 30.0, quat) == 1
        if f != 2:
            m.integrate_known()
    lay = _layers(shape, m.T + 1)
    _set_grid(m, lay)
    return m, lay


def _views(cfg, shape, n_ok=140, seed=11):
    """[n, 9] views in the map frame: n_ok candidates inside the map (a fifth of them on voxel faces) over every attitude, range and t
    of the lists above, then views outside the map, invalid ones and views whose own cell is a wall cell without holes"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    half = np.array(common.half_extent(cfg), np.float64)
    res = float(F(RES))
    xw = int(0.8 * nx)
    pos = rng.uniform(-0.97, 0.97, (n_ok, 3)) * half
    pos[: n_ok // 2, 0] = rng.uniform(-0.97 * half[0], -half[0] + xw * res - 0.01, n_ok // 2)   # half of them in front of the wall
    pos[0] = (-0.5 if shape != TINY else -0.1, 0.02, 0.01)
    k = n_ok // 5                                                                     # on a face: centre + res / 2 along one axis
    idx = np.stack([rng.integers(0, nx, k), rng.integers(0, ny, k), rng.integers(0, nz, k)], 1)
    face = (idx + 0.5) * res - half
    face[np.arange(k), rng.integers(0, 3, k)] += 0.5 * res
    pos[-k:] = face
    v = np.zeros((n_ok, 9), np.float64)
    v[:, 0:3] = pos
    v[:, 3:7] = np.array(VIEW_QUATS)[np.arange(n_ok) % len(VIEW_QUATS)]
    v[:, 7] = np.array([INF, 0.9, 0.2, INF])[(np.arange(n_ok) // 2) % 4]
    v[:, 8] = np.array([-1.0, 0.0, T_BETWEEN, T_PAST, -1.0])[(np.arange(n_ok) // 3) % 5]
    out = rng.uniform(1.02, 1.4, (12, 3)) * half * rng.choice([-1, 1], (12, 3))
    out[:4] = [[half[0], 0, 0], [-half[0], 0, 0], [0, half[1], 0], [0, 0, -half[2]]]
    vo = np.tile(v[:1], (12, 1))
    vo[:, 0:3] = out
    nan = float("nan")
    vi = np.tile(v[:1], (10, 1))
    vi[0, 0], vi[1, 2], vi[2, 1] = nan, INF, -INF
    vi[3, 3], vi[4, 5] = nan, INF
    vi[5, 3:7] = 0.0
    vi[6, 3:7] = (1e-30, 0.0, 0.0, 0.0)
    vi[7, 7], vi[8, 7], vi[9, 8] = 0.0, nan, nan
    vi[7, 0] = 9.0                                                                    # invalid AND outside
    vb = np.tile(v[:1], (8, 1))                                                       # the wall's row y = 0: set in every layer
    vb[:, 0] = (xw + 0.5) * res - half[0] + rng.uniform(-0.4, 0.4, 8) * res
    vb[:, 1] = 0.5 * res - half[1]
    vb[:, 2] = (rng.integers(0, nz, 8) + 0.5) * res - half[2]
    vb[:, 8] = np.array([-1.0, 0.0, T_BETWEEN, T_PAST])[np.arange(8) % 4]
    return np.concatenate([v, vo, vi, vb]).astype(F)


def _device_rays(m):
    cache = {}

    def rays(quat):
        if quat not in cache:
            cache[quat] = m.view_rays(quat)
        return cache[quat]
    return rays


def _margin(dsp, m):
    return float(m.get_param(dsp.capi.P_OCCLUSION_MARGIN))


def _same_scores(got, want, views, tag):
    assert got.dtype == want.dtype == V.SCORE_DTYPE and got.shape == want.shape, tag
    for f in ("status", "n_returns", "n_seen", "n_unknown"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (tag, f, bad.size, bad[:5], got[bad[:5]], want[bad[:5]], views[bad[:5]])


def _from_device(raw):
    out = np.zeros(raw.shape[0], V.SCORE_DTYPE)
    out.view(np.int32).reshape(-1, 4)[:] = raw.cpu().numpy()
    return out


def _not_degenerate(shape, want, info, NP):
    st = want["status"]
    ok = st == V.OK
    print(shape, "OK", ok.sum(), "BLOCKED", (st == V.BLOCKED).sum(), "OUTSIDE", (st == V.OUTSIDE).sum(), "INVALID", (st == V.INVALID).sum(),
          "returns", want["n_returns"][ok].min(), want["n_returns"][ok].max(), "seen", want["n_seen"][ok].max())
    if shape == TINY:
        assert ok.sum() >= 1 and (st == V.BLOCKED).sum() >= 1
        return
    mixed = ok & (0 < want["n_unknown"]) & (want["n_unknown"] < want["n_seen"]) & (0 < want["n_returns"]) & (want["n_returns"] < NP)
    assert mixed.sum() >= 20, mixed.sum()
    for s in (V.OUTSIDE, V.INVALID, V.BLOCKED):
        assert (st == s).sum() >= 5, s
    assert max(d["occluded"].sum() for d in info.values()) >= 30 and max(d["beyond"].sum() for d in info.values()) >= 30
    rays = np.concatenate([d["ray_status"] for d in info.values()])
    assert {CR.HIT, CR.FREE, CR.LEFT_MAP} <= set(rays.tolist())


@pytest.mark.parametrize("att", ["identity", "yaw90", "pitch_roll"])
def test_view_rays_against_a_real_frame(dsp, att):
    """the planes view_rays makes of an attitude are those of a frame taken with it, bit for bit; every direction lies in its own pyramid"""
    m = _map(dsp, CUBE)
    fresh = _map(dsp, CUBE)
    ph0, pv0, dirs0 = fresh.view_rays(QUATS[att])                                     # before any frame: the call needs none
    assert m.update(_cloud(0.6), (0.0, 0.0, 0.0), 0.0, QUATS[att]) == 1
    ph, pv, _ = m.view()
    rh, rv, dirs = m.view_rays(QUATS[att])
    for a, b in ((rh, ph), (rv, pv), (ph0, ph), (pv0, pv), (dirs0, dirs)):
        assert a.dtype == b.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    other = m.view_rays(QUATS["identity" if att != "identity" else "yaw90"])          # another attitude: the frame's planes stay
    assert not np.array_equal(other[0], rh) and all(np.array_equal(a, b) for a, b in zip(m.view()[:2], (ph, pv)))
    assert dirs.shape == (m.NP, 3)
    assert np.array_equal(K.pyramid_of(rh, rv, dirs[:, 0], dirs[:, 1], dirs[:, 2]), np.arange(m.NP))
    assert np.abs(dirs.astype(np.float64) - V.directions(m.cfg, QUATS[att])).max() <= 1e-6
    ident = m.view_rays(QUATS["identity"])[2] if att != "identity" else dirs
    assert np.abs(ident - V.directions0(m.cfg)).max() <= 6e-8                         # the table itself: float64 on the host, rounded once (an ulp: two libms)
    m.close(), fresh.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_view_scores_match_the_restatement(dsp, shape):
    m, lay = _scene(dsp, shape)
    cfg = m.cfg
    ages = m.known_age()
    assert set(np.unique(ages).tolist()) <= {-1, 0, 2, 3} and (shape == TINY or len(np.unique(ages)) == 4)
    assert shape == TINY or 0.25 < (~K.unknown(ages, MAX_AGE)).mean() < 0.8            # roughly half the window is known
    views = _views(cfg, shape)
    rays = _device_rays(m)
    margin = _margin(dsp, m)
    want, info = V.score(cfg, lay, ages, views, MAX_AGE, rays, margin, details=True)
    _not_degenerate(shape, want, info, m.NP)
    got = m.score_views(views, MAX_AGE)
    _same_scores(got, want, views, (shape, "host"))
    dev = m.score_views(torch.from_numpy(np.concatenate([views, views], 1)).cuda()[:, :9], MAX_AGE)   # a non-contiguous view: the binding's temporary
    m.sync()
    assert dev.dtype == torch.int32 and tuple(dev.shape) == (len(views), 4)
    _same_scores(_from_device(dev), want, views, (shape, "device"))
    # any chunking gives the same integers
    for chunks in (1, 3, 64):
        m.set_param(dsp.capi.P_VIEW_CHUNKS, chunks)
        _same_scores(m.score_views(views, MAX_AGE), want, views, (shape, "chunks", chunks))
    m.set_param(dsp.capi.P_VIEW_CHUNKS, 0)
    # another age limit: the same seen sets, other unknown counts
    want0 = V.score(cfg, lay, ages, views, 3, rays, margin)
    _same_scores(m.score_views(views, 3), want0, views, (shape, "max_age 3"))
    assert shape == TINY or (want0["n_unknown"] < want["n_unknown"]).any()
    # world frame: the same candidates, given in world coordinates (the sensor stands at the origin here: subtracting it changes no bit)
    _same_scores(m.score_views(views, MAX_AGE, world=True), want, views, (shape, "world at origin"))
    # cell by cell: the seen set and the farthest returns of OK views, the ones with the most to get wrong first
    ok = sorted(info, key=lambda i: -int(info[i]["occluded"].sum()) - int(info[i]["beyond"].sum()))
    some = ok[:6] + ok[-4:] if shape != TINY else ok[:3]
    assert len(set(some)) >= (8 if shape != TINY else 1)
    for i in set(some):
        words, ml = m.view_cells(views[i])
        wantw = CR.pack(info[i]["seen"])
        assert words.shape == wantw.shape and np.array_equal(words, wantw), (shape, i, np.argwhere(words != wantw)[:5])
        assert np.array_equal(ml.view(np.uint32), info[i]["ml"].view(np.uint32)), (shape, i, np.flatnonzero(ml != info[i]["ml"])[:5])
    bad = int(np.flatnonzero(want["status"] != V.OK)[0])                              # a view that is not OK: nothing seen, no return
    words, ml = m.view_cells(views[bad])
    assert not words.any() and (ml == -1).all()
    m.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_view_scores_in_a_masked_grid(dsp, shape):
    """after dspmap_mask_cast_grid the rays stop at unknown space: the conservative gain"""
    m, lay = _scene(dsp, shape)
    cfg = m.cfg
    ages = m.known_age()
    views = _views(cfg, shape, n_ok=100)
    rays = _device_rays(m)
    margin = _margin(dsp, m)
    before = m.score_views(views, MAX_AGE)
    _same_scores(before, V.score(cfg, lay, ages, views, MAX_AGE, rays, margin), views, (shape, "unmasked"))
    m.mask_cast_grid(MAX_AGE)
    masked = lay | K.unknown(ages, MAX_AGE)[None]
    assert np.array_equal(m.cast_grid(), CR.pack(masked)) and (masked != lay).any()
    want = V.score(cfg, lay=masked, ages=ages, views=views, max_age=MAX_AGE, rays=rays, occl_margin=margin)
    after = m.score_views(views, MAX_AGE)
    _same_scores(after, want, views, (shape, "masked"))
    both = (before["status"] == V.OK) & (after["status"] == V.OK)
    assert (want["status"] == V.BLOCKED).sum() > (before["status"] == V.BLOCKED).sum()    # a candidate in unknown space is blocked now
    if shape != TINY:
        assert both.sum() >= 10 and (after["n_unknown"][both] < before["n_unknown"][both]).any()
        assert (after["n_returns"][both] >= before["n_returns"][both]).all()          # more set bits: every ray that hit still hits
    m.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_view_scores_after_ego_motion(dsp, shape):
    """the window moves by a frame 0.2 m away; candidates given in world coordinates are scored against the moved layer"""
    m, lay = _scene(dsp, shape)
    cfg = m.cfg
    before = m.known_age()
    cur = np.array([0.2, -0.05, 0.0], F)
    assert m.update(_cloud(WALL_DIST[shape]), cur, 0.5, QUATS["pitch_roll"]) == 1
    m.integrate_known()
    lay = _layers(shape, m.T + 1, seed=6)
    _set_grid(m, lay)
    ages = m.known_age()
    assert not np.array_equal(ages, before) and (shape == TINY or len(np.unique(ages)) >= 3)
    views = _views(cfg, shape, n_ok=100, seed=13)
    world = views.copy()
    world[:, 0:3] = (world[:, 0:3] + cur[None, :]).astype(F)
    rays = _device_rays(m)
    want = V.score(cfg, lay, ages, world, MAX_AGE, rays, _margin(dsp, m), world=True, cur_pos=cur)
    st = want["status"]
    assert (st == V.OK).sum() >= (20 if shape != TINY else 1) and (st == V.INVALID).sum() >= 5 and (st == V.OUTSIDE).sum() >= 5
    _same_scores(m.score_views(world, MAX_AGE, world=True), want, world, (shape, "world"))
    dev = m.score_views(torch.from_numpy(world).cuda(), MAX_AGE, world=True)
    m.sync()
    _same_scores(_from_device(dev), want, world, (shape, "world, device"))
    # the same numbers in the map frame mean other places
    want_map = V.score(cfg, lay, ages, world, MAX_AGE, rays, _margin(dsp, m))
    _same_scores(m.score_views(world, MAX_AGE), want_map, world, (shape, "map frame"))
    assert shape == TINY or (want_map["n_seen"] != want["n_seen"]).any()
    m.close()


def test_view_life_cycle_and_read_only(dsp):
    twins = []
    for _ in range(2):
        m = _map(dsp, CUBE, seed=99)
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        twins.append(m)
    a, b = twins
    pts = [_cloud(0.6, seed=s) for s in range(5)]
    views = _views(a.cfg, CUBE, n_ok=60)
    dviews = torch.from_numpy(views).cuda()
    L = a.L
    err = lambda: L.dspmap_last_error(a.h)   # noqa: E731
    out = np.zeros(len(views), dsp.capi.VIEW_SCORE_DTYPE)
    ptr = lambda x: x.ctypes.data_as(__import__("ctypes").c_void_p)   # noqa: E731
    for f in range(4):
        cur = (0.03 * f, -0.02 * f, 0.0)
        for m in (a, b):
            assert m.update(pts[f], cur, f / 30.0, QUATS[("identity", "yaw90", "pitch_roll")[f % 3]]) == 1
        a.integrate_known()
        # stale grid (the frame above): the call names the build
        assert L.dspmap_score_views(a.h, len(views), ptr(views), MAX_AGE, 0, ptr(out)) == E_STATE and b"dspmap_build_cast_grid" in err()
        assert L.dspmap_score_views(a.h, 0, None, MAX_AGE, 0, None) == E_STATE
        a.build_cast_grid(0.05, 1)
        state = (a.results(), b.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors(), a.view())   # (getFutureStatus is a consuming readout: the twin's is the "before")
        ca = a.counters()
        s1 = a.score_views(views, MAX_AGE, world=True)
        s2 = a.score_views(dviews, MAX_AGE, world=True)
        a.view_rays(QUATS["yaw90"]), a.view_cells(views[0])
        # n = 0: OK, nothing touched
        assert L.dspmap_score_views(a.h, 0, None, MAX_AGE, 0, None) == 1 and L.dspmap_score_views_device(a.h, 0, None, MAX_AGE, 0, None) == 1
        assert a.score_views(np.zeros((0, 9), F), MAX_AGE).shape == (0,)
        a.sync()
        assert np.array_equal(_from_device(s2), s1) and (s1["status"] == V.OK).sum() >= 10 and s1["n_seen"].max() > 30
        assert np.array_equal(a.score_views(views, MAX_AGE, world=True), s1)          # twice is the same
        after = (a.results(), a.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors(), a.view())
        for x, y in zip(state[:4], after[:4]):
            assert np.array_equal(x, y)
        assert state[4] == after[4] and all(np.array_equal(x, y) for x, y in zip(state[5], after[5]))
        cb = a.counters()
        ca.pop("update_ms"), cb.pop("update_ms")
        assert ca == cb
        assert a.cast_grid_ptr() is not None                                          # nothing went stale
    # a following frame equals that of the twin that never scored
    for m in (a, b):
        assert m.update(pts[4], (0.1, 0.0, 0.0), 0.2, QUATS["identity"]) == 1
    assert np.array_equal(a.results(), b.results()) and (a.results()[:, 0] > 0).any()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    ca, cb = a.counters(), b.counters()
    ca.pop("update_ms"), cb.pop("update_ms")
    assert ca == cb and a.cursors() == b.cursors()
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    # the layer without an integration since its last reset: the call names the integration
    a.build_cast_grid(0.05, 0)
    a.reset_known()
    assert L.dspmap_score_views(a.h, len(views), ptr(views), MAX_AGE, 0, ptr(out)) == E_STATE and b"dspmap_known_integrate" in err()
    assert L.dspmap_score_views_device(a.h, len(views), dviews.data_ptr(), MAX_AGE, 0, ptr(out)) == E_STATE and b"dspmap_known_integrate" in err()
    b.build_cast_grid(0.05, 0)                                                        # a grid, but never an integration
    assert b.L.dspmap_score_views(b.h, len(views), ptr(views), MAX_AGE, 0, ptr(out)) == E_STATE and b"dspmap_known_integrate" in b.L.dspmap_last_error(b.h)
    assert not out.view(np.int32).any()
    a.close(), b.close()
    slab = _map(dsp, CUBE, z_lo=0, z_hi=3)                                            # a sharded handle
    assert slab.L.dspmap_score_views(slab.h, len(views), ptr(views), MAX_AGE, 0, ptr(out)) == E_STATE and b"slab" in slab.L.dspmap_last_error(slab.h)
    slab.close()
