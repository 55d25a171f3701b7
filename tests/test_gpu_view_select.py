"""GPU tests of the joint gain of views (dspmap_score_view_sets*, dspmap_select_views*): exact parity -- zero differing integers -- with
the numpy restatement (tests/view_select_ref.py), fed like tests/test_gpu_view.py: the planes and ray directions the device makes of
every attitude (DSPMap.view_rays), the layers of the cast grid as set (DSPMap.set_cast_grid) and the ages the known-space layer hands
out (DSPMap.known_age).  The shapes at 0.15 m: 66 x 12 x 8 (a second word with two bits), 65 x 5 x 4 (a second word with ONE bit),
16 x 16 x 6 (one partial word) and 3 x 3 x 3 (a map smaller than a wave); one test runs 130 x 20 x 10, whose layer of 600 words makes
the set, gain and cover kernels work in several workgroups per mask.  The ages are set (DSPMap.set_known, the scene whose
non-degeneracy tests/test_view_select_cpu.py asserts) in one parametrisation and made by real frames and integrate_known in the other
(the scene of test_gpu_view.py).  The candidates are test_gpu_view's: 60 inside the map over every attitude, range and layer, 12
outside, 10 invalid, 8 blocked, and the first 10 once more at the end."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cast_ref as CR
from tests import common
from tests import known_ref as K
from tests import test_gpu_view as G
from tests import view_ref as V
from tests import view_select_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
E_STATE = -3
WIDE, CUBE, NARROW, TINY = (66, 12, 8), (16, 16, 6), (65, 5, 4), (3, 3, 3)
SHAPES = [WIDE, CUBE, NARROW, TINY]
IDS = ["66x12x8", "16x16x6", "65x5x4", "3x3x3"]
WALL_DIST = dict(G.WALL_DIST)
WALL_DIST[NARROW] = 4.0
LONG = (130, 20, 10)                                                      # 600 words per layer: more than one pass of a chunk
WALL_DIST[LONG] = 4.0
MAX_AGE = R.SCENE_MAX_AGE


def _scene(dsp, shape, known):
    """known "set": six frames (the counter the ages 0 .. 5 need), then the ages of the CPU guards; "frames": test_gpu_view's scene, four
    frames integrated after the first, second and fourth.  Then the grid replaced by the wall with holes."""
    m = G._map(dsp, shape)
    pts = G._cloud(WALL_DIST[shape])
    quats = (G.QUATS["yaw90"], G.YAW180, G.QUATS["identity"], G.QUATS["identity"]) + ((G.QUATS["identity"],) * 2 if known == "set" else ())
    for f, quat in enumerate(quats):
        assert m.update(pts, (0.0, 0.0, 0.0), f / 30.0, quat) == 1
        if known == "frames" and f != 2:
            m.integrate_known()
    if known == "set":
        m.set_known(R.scene_ages(shape))
    lay = G._layers(shape, m.T + 1)
    G._set_grid(m, lay)
    return m, lay


def _reference(dsp, m, lay, views, max_age=MAX_AGE, **kw):
    return R.seen_sets(m.cfg, lay, m.known_age(), views, max_age, G._device_rays(m), G._margin(dsp, m), **kw)


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    for f in got.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, (tag, f, len(bad), bad[:5].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def _np(raw, dtype):
    a = raw.cpu().numpy()
    out = np.zeros(a.shape[:-1], dtype)
    out.view(np.int32).reshape(a.shape)[...] = a
    return out


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


@pytest.mark.parametrize("known", ["set", "frames"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_view_sets_match_the_restatement(dsp, shape, known):
    m, lay = _scene(dsp, shape, known)
    views = R.scene_views(m.cfg, shape)
    scores, S, unknown = _reference(dsp, m, lay, views)
    assert (scores["status"] == V.OK).sum() >= (20 if shape != TINY else 1) and (shape == TINY or 0 < unknown.mean() < 1)
    alone = m.score_views(views, MAX_AGE)
    _same(alone, scores, (shape, "score_views"))
    # sets of one view: the view's own score, and scores_out is score_views field for field
    one, sc = m.score_view_sets(views[:, None, :], MAX_AGE, scores=True)
    _same(sc[:, 0], alone, (shape, "scores_out"))
    assert np.array_equal(one["n_seen"], alone["n_seen"]) and np.array_equal(one["n_unknown"], alone["n_unknown"])
    assert np.array_equal(one["n_ok"], (alone["status"] == V.OK).astype(np.int32)) and not one["reserved"].any()
    # sets of 4 and of 7: attitudes, ranges and layers mix, members are OUTSIDE, INVALID and BLOCKED, the last set has no OK view
    for size, n_sets in ((4, 48), (7, 30)):
        sets, idx = R.scene_sets(views, size, n_sets)
        want = R.sets_from(scores[idx.ravel()], S[idx.ravel()], unknown, n_sets, size)
        st = scores["status"][idx]
        assert want["n_ok"][-1] == 0 and want["n_seen"][-1] == 0 and {V.OUTSIDE, V.INVALID, V.BLOCKED} <= set(st.ravel().tolist())
        assert shape == TINY or len(np.unique(views[idx][st == V.OK][:, 8])) >= 3      # several layers among the OK members
        if shape in (WIDE, CUBE):
            assert ((want["n_seen"] > scores["n_seen"][idx].max(1)) & (want["n_seen"] < scores["n_seen"][idx].sum(1))).sum() >= 10
        got, sc = m.score_view_sets(sets, MAX_AGE, scores=True)
        _same(got, want, (shape, known, size, "host"))
        _same(sc, scores[idx], (shape, known, size, "host scores"))
        _same(m.score_view_sets(sets, MAX_AGE), want, (shape, known, size, "host, no scores"))
        dev, dsc = m.score_view_sets(_cuda(sets), MAX_AGE, scores=True)
        dev2 = m.score_view_sets(_cuda(sets), MAX_AGE)
        m.sync()
        assert dev.dtype == torch.int32 and tuple(dev.shape) == (n_sets, 4) and tuple(dsc.shape) == (n_sets, size, 4)
        _same(_np(dev, R.SET_SCORE_DTYPE), want, (shape, known, size, "device"))
        _same(_np(dsc, V.SCORE_DTYPE), scores[idx], (shape, known, size, "device scores"))
        _same(_np(dev2, R.SET_SCORE_DTYPE), want, (shape, known, size, "device, no scores"))
    # another age limit: the same seen sets, other unknown counts
    sets, idx = R.scene_sets(views, 4, 48)
    want3 = R.sets_from(scores[idx.ravel()], S[idx.ravel()], K.unknown(m.known_age(), 3), 48, 4)
    _same(m.score_view_sets(sets, 3), want3, (shape, known, "max_age 3"))
    assert m.score_view_sets(np.zeros((0, 4, 9), F), MAX_AGE).shape == (0,)
    m.close()


@pytest.mark.parametrize("known", ["set", "frames"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_view_selection_matches_the_restatement(dsp, shape, known):
    m, lay = _scene(dsp, shape, known)
    views = R.scene_views(m.cfg, shape)
    scores, S, unknown = _reference(dsp, m, lay, views)
    dviews = _cuda(views)
    base = R.greedy_from(S, unknown, 0, 16, 1)
    rounds = int((base["view"] >= 0).sum())
    print(shape, known, "rounds", rounds, base["view"].tolist(), base["gain"].tolist())
    assert (rounds >= 1 or shape == TINY) and (known != "set" or shape not in (WIDE, CUBE) or rounds >= 8)
    stop = int(base["gain"][min(2, rounds - 1)])                          # a min_gain that ends the rounds after a few
    cases = [dict(k=16), dict(k=16, n_fixed=5), dict(k=16, min_gain=stop + 1), dict(k=64), dict(k=0), dict(k=3, n_fixed=len(views)),
             dict(k=5, n_fixed=90, min_gain=1)]                            # (the last: only the duplicates are candidates)
    for kw in cases:
        want = R.greedy_from(S, unknown, kw.get("n_fixed", 0), kw["k"], kw.get("min_gain", 1))
        got, sc = m.select_views(views, kw["k"], MAX_AGE, n_fixed=kw.get("n_fixed", 0), min_gain=kw.get("min_gain", 1), scores=True)
        _same(got, want, (shape, known, kw, "host"))
        _same(sc, scores, (shape, known, kw, "host scores"))
        dev = m.select_views(dviews, kw["k"], MAX_AGE, n_fixed=kw.get("n_fixed", 0), min_gain=kw.get("min_gain", 1))
        m.sync()
        assert dev.dtype == torch.int32 and tuple(dev.shape) == (kw["k"], 4)
        _same(_np(dev, R.PICK_DTYPE), want, (shape, known, kw, "device"))
        real = want["view"][want["view"] >= 0]
        assert len(set(real.tolist())) == len(real) and (real >= kw.get("n_fixed", 0)).all()
        if kw.get("n_fixed", 0) == 0:
            assert not (set(real.tolist()) & set(range(90, 100)))         # a duplicate is never picked behind its original
    want64 = R.greedy_from(S, unknown, 0, 64, 1)
    assert (want64["view"] >= 0).sum() < 64 and want64["view"][-1] == -1  # fewer useful views than k
    assert (R.greedy_from(S, unknown, 0, 16, stop + 1)["view"] >= 0).sum() <= 3
    if shape in (WIDE, CUBE) and known == "set":
        assert R.greedy_from(S, unknown, 5, 16, 1)["view"].tolist() != base["view"].tolist()   # committed views change the choice
    dsel, dsc = m.select_views(dviews, 16, MAX_AGE, scores=True)
    m.sync()
    _same(_np(dsel, R.PICK_DTYPE), base, (shape, known, "device with scores"))
    _same(_np(dsc, V.SCORE_DTYPE), scores, (shape, known, "device scores"))
    # no views at all: k empty picks, nothing covered
    empty = m.select_views(np.zeros((0, 9), F), 3, MAX_AGE)
    assert empty["view"].tolist() == [-1] * 3 and not empty["gain"].any() and not empty["covered"].any()
    assert m.select_views(np.zeros((0, 9), F), 0, MAX_AGE).shape == (0,)
    m.close()


@pytest.mark.parametrize("shape", [WIDE, TINY], ids=["66x12x8", "3x3x3"])
def test_results_do_not_depend_on_the_launch_or_on_the_scratch(dsp, shape):
    m, lay = _scene(dsp, shape, "set")
    views = R.scene_views(m.cfg, shape)
    sets, _ = R.scene_sets(views, 7, 30)
    want_sets, want_sc = m.score_view_sets(sets, MAX_AGE, scores=True)
    want_sel = m.select_views(views, 16, MAX_AGE, n_fixed=5)
    assert want_sets["n_seen"].any() and (want_sel["view"] >= 0).any()
    for chunks in (1, 64, 3):
        m.set_param(dsp.capi.P_VIEW_CHUNKS, chunks)
        got, sc = m.score_view_sets(sets, MAX_AGE, scores=True)
        assert got.tobytes() == want_sets.tobytes() and sc.tobytes() == want_sc.tobytes(), chunks
        assert m.select_views(views, 16, MAX_AGE, n_fixed=5).tobytes() == want_sel.tobytes(), chunks
    m.set_param(dsp.capi.P_VIEW_CHUNKS, 0)
    # a dirty scratch: a larger batch first (its masks, gains and grids stay behind), then smaller ones
    big = np.concatenate([views[::-1], views, views])
    m.select_views(big, 64, MAX_AGE, n_fixed=3)
    m.score_view_sets(big.reshape(30, 10, 9), MAX_AGE)
    small = views[10:40]
    scores, S, unknown = _reference(dsp, m, lay, small)
    _same(m.select_views(small, 8, MAX_AGE, n_fixed=2), R.greedy_from(S, unknown, 2, 8, 1), (shape, "small after large"))
    _same(m.score_view_sets(small.reshape(10, 3, 9), MAX_AGE), R.sets_from(scores, S, unknown, 10, 3), (shape, "small sets after large"))
    assert m.select_views(views, 16, MAX_AGE, n_fixed=5).tobytes() == want_sel.tobytes()
    assert m.score_view_sets(sets, MAX_AGE).tobytes() == want_sets.tobytes()
    m.close()


def test_many_words_many_chunks_and_many_candidates_match_the_restatement(dsp):
    """130 x 20 x 10: a layer of 600 words, so the set and gain kernels really split a mask over two or three workgroups (256 words
    per pass of a chunk) and the cover kernel runs three; every forced chunk count -- also 64, far more than the layer has words for
    -- against the RESTATEMENT, not against another launch.  Then 300 views: more candidates than the pick kernel has threads, every
    gain three times, so that the smallest index has to win across its strides."""
    m, lay = _scene(dsp, LONG, "set")
    views = R.scene_views(m.cfg, LONG)
    scores, S, unknown = _reference(dsp, m, lay, views)
    nx, ny, nz = LONG
    word = ((np.arange(nz)[:, None, None] * ny + np.arange(ny)[None, :, None]) * 3 + (np.arange(nx) >> 6)[None, None, :])
    assert word.max() == 599
    want_sel = R.greedy_from(S, unknown, 5, 16, 1)
    picked = want_sel["view"][want_sel["view"] >= 0]
    assert len(picked) >= 8
    for i in picked[:3]:                                                  # the first picks' gains come from all three passes of a chunk
        assert set((word[S[i] & unknown] // 256).tolist()) == {0, 1, 2}, i
    wants = {}
    for size, n_sets in ((4, 48), (7, 30)):
        sets, idx = R.scene_sets(views, size, n_sets)
        wants[size] = (sets, R.sets_from(scores[idx.ravel()], S[idx.ravel()], unknown, n_sets, size), scores[idx])
        assert (wants[size][1]["n_unknown"] > 0).sum() >= 20
    big = np.concatenate([views[::-1], views, views])
    S_big = np.concatenate([S[::-1], S, S])
    want_big = R.greedy_from(S_big, unknown, 3, 16, 1)
    real = want_big["view"][want_big["view"] >= 0]
    assert len(real) >= 8 and (real < 100).all()                         # every gain ties with its copies at 199 - i and 299 - i: the first wins
    late = big.copy()
    late[:200, 7] = 0.0                                                   # the first two copies INVALID: every pick lies in 200 .. 299
    want_late = R.greedy_from(np.concatenate([np.zeros_like(S), np.zeros_like(S), S]), unknown, 3, 16, 1)
    real = want_late["view"][want_late["view"] >= 0]
    assert len(real) >= 8 and (real >= 200).all() and (real < 256).any() and (real >= 256).any()
    dbig = _cuda(big)
    for chunks in (0, 1, 2, 3, 64):
        m.set_param(dsp.capi.P_VIEW_CHUNKS, chunks)
        for size, (sets, want, want_sc) in wants.items():
            got, sc = m.score_view_sets(sets, MAX_AGE, scores=True)
            _same(got, want, ("chunks", chunks, "sets of", size))
            _same(sc, want_sc, ("chunks", chunks, "scores of sets of", size))
        got, sc = m.select_views(views, 16, MAX_AGE, n_fixed=5, scores=True)
        _same(got, want_sel, ("chunks", chunks, "selection"))
        _same(sc, scores, ("chunks", chunks, "selection scores"))
        _same(m.select_views(big, 16, MAX_AGE, n_fixed=3), want_big, ("chunks", chunks, "300 views"))
        dev = m.select_views(dbig, 16, MAX_AGE, n_fixed=3)
        m.sync()
        _same(_np(dev, R.PICK_DTYPE), want_big, ("chunks", chunks, "300 views, device"))
        _same(m.select_views(late, 16, MAX_AGE, n_fixed=3), want_late, ("chunks", chunks, "300 views, the last 100 valid"))
    m.set_param(dsp.capi.P_VIEW_CHUNKS, 0)
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE], ids=["66x12x8", "16x16x6"])
def test_view_selection_in_a_masked_grid(dsp, shape):
    """after dspmap_mask_cast_grid the rays stop at unknown space: the conservative joint gain"""
    m, lay = _scene(dsp, shape, "frames")
    views = R.scene_views(m.cfg, shape)
    before = m.select_views(views, 16, MAX_AGE)
    m.mask_cast_grid(MAX_AGE)
    masked = lay | K.unknown(m.known_age(), MAX_AGE)[None]
    assert np.array_equal(m.cast_grid(), CR.pack(masked)) and (masked != lay).any()
    scores, S, unknown = _reference(dsp, m, masked, views)
    want = R.greedy_from(S, unknown, 0, 16, 1)
    got, sc = m.select_views(views, 16, MAX_AGE, scores=True)
    _same(got, want, (shape, "masked"))
    _same(sc, scores, (shape, "masked scores"))
    assert (want["view"] >= 0).any() and want.tobytes() != before.tobytes()
    sets, idx = R.scene_sets(views, 4, 48)
    _same(m.score_view_sets(sets, MAX_AGE), R.sets_from(scores[idx.ravel()], S[idx.ravel()], unknown, 48, 4), (shape, "masked sets"))
    m.close()


@pytest.mark.parametrize("shape", [WIDE, CUBE, TINY], ids=["66x12x8", "16x16x6", "3x3x3"])
def test_view_selection_after_ego_motion(dsp, shape):
    """the window moves by a frame 0.2 m away -- a non-integer number of voxels --; candidates given in world coordinates are scored
    against the moved layer"""
    m, lay = _scene(dsp, shape, "frames")
    cur = np.array([0.2, -0.05, 0.0], F)
    before = m.known_age()
    assert m.update(G._cloud(WALL_DIST[shape]), cur, 0.5, G.QUATS["pitch_roll"]) == 1
    m.integrate_known()
    lay = G._layers(shape, m.T + 1, seed=6)
    G._set_grid(m, lay)
    assert not np.array_equal(m.known_age(), before)
    views = R.scene_views(m.cfg, shape)
    world = views.copy()
    world[:, 0:3] = (world[:, 0:3] + cur[None, :]).astype(F)
    scores, S, unknown = _reference(dsp, m, lay, world, world=True, cur_pos=cur)
    assert (scores["status"] == V.OK).sum() >= (10 if shape != TINY else 1)
    want = R.greedy_from(S, unknown, 3, 16, 1)
    got, sc = m.select_views(world, 16, MAX_AGE, n_fixed=3, world=True, scores=True)
    _same(got, want, (shape, "world"))
    _same(sc, scores, (shape, "world scores"))
    dev = m.select_views(_cuda(world), 16, MAX_AGE, n_fixed=3, world=True)
    sets, idx = R.scene_sets(world, 4, 48)
    dsets = m.score_view_sets(_cuda(sets), MAX_AGE, world=True)
    m.sync()
    _same(_np(dev, R.PICK_DTYPE), want, (shape, "world, device"))
    _same(_np(dsets, R.SET_SCORE_DTYPE), R.sets_from(scores[idx.ravel()], S[idx.ravel()], unknown, 48, 4), (shape, "world sets, device"))
    # the same numbers in the map frame mean other places
    ms, mS, _ = _reference(dsp, m, lay, world)
    _same(m.select_views(world, 16, MAX_AGE, n_fixed=3), R.greedy_from(mS, unknown, 3, 16, 1), (shape, "map frame"))
    assert shape == TINY or (ms["n_seen"] != scores["n_seen"]).any()
    m.close()


def test_view_select_life_cycle_and_read_only(dsp):
    twins = []
    for _ in range(2):
        m = G._map(dsp, CUBE, seed=99)
        m.set_tables(*common.tables(5))
        m.seed_uniform(2, 0.01, 17, vmax=0.8)
        twins.append(m)
    a, b = twins
    pts = [G._cloud(0.6, seed=s) for s in range(5)]
    views = R.scene_views(a.cfg, CUBE)
    dviews = _cuda(views)
    sets, _ = R.scene_sets(views, 4, 48)
    L = a.L
    err = lambda: L.dspmap_last_error(a.h)   # noqa: E731
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    out, picks = np.zeros(48, R.SET_SCORE_DTYPE), np.zeros(16, R.PICK_DTYPE)
    src = np.array([[-0.5, 0.0, 0.0, 0.0]], F)
    for f in range(3):
        cur = (0.03 * f, -0.02 * f, 0.0)
        for m in (a, b):
            assert m.update(pts[f], cur, f / 30.0, G.QUATS[("identity", "yaw90", "pitch_roll")[f % 3]]) == 1
        a.integrate_known()
        # stale grid (the frame above): the calls name the build, also without views
        assert L.dspmap_score_view_sets(a.h, 48, 4, ptr(sets), MAX_AGE, 0, ptr(out), None) == E_STATE and b"dspmap_build_cast_grid" in err()
        assert L.dspmap_select_views(a.h, len(views), ptr(views), 0, MAX_AGE, 0, 16, 1, ptr(picks), None) == E_STATE and b"dspmap_build_cast_grid" in err()
        assert L.dspmap_select_views_device(a.h, 0, None, 0, MAX_AGE, 0, 0, 1, None, None) == E_STATE
        a.build_cast_grid(0.05, 1)
        a.build_frontiers(max_age=MAX_AGE)
        a.build_objects()
        a.build_reach_fields(src, max_steps=8)
        state = (a.results(), b.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors(), a.view())
        layers = (a.frontier_counts(), a.frontier_grid(), a.objects(), a.reach_field(0))
        alone, cells = a.score_views(views, MAX_AGE, world=True), a.view_cells(views[0])
        ca = a.counters()
        s1 = a.score_view_sets(sets, MAX_AGE, world=True)
        p1 = a.select_views(views, 16, MAX_AGE, n_fixed=2, world=True)
        s2 = a.score_view_sets(_cuda(sets), MAX_AGE, world=True)
        p2 = a.select_views(dviews, 16, MAX_AGE, n_fixed=2, world=True)
        # nothing to do: OK, nothing touched
        assert L.dspmap_score_view_sets(a.h, 0, 4, None, MAX_AGE, 0, None, None) == 1 and L.dspmap_score_view_sets_device(a.h, 0, 0, None, MAX_AGE, 0, None, None) == 1
        assert L.dspmap_select_views(a.h, 0, None, 0, MAX_AGE, 0, 0, 1, None, None) == 1 and L.dspmap_select_views_device(a.h, 0, None, 0, MAX_AGE, 0, 0, 1, None, None) == 1
        a.sync()
        assert np.array_equal(_np(s2, R.SET_SCORE_DTYPE), s1) and np.array_equal(_np(p2, R.PICK_DTYPE), p1)
        assert s1["n_seen"].max() > 30 and s1["n_unknown"].any() and (p1["view"] >= 2).any()
        assert np.array_equal(a.select_views(views, 16, MAX_AGE, n_fixed=2, world=True), p1)   # twice is the same
        # read-only: the map, the grid, the layer, the frame's view -- and every snapshot is still valid and unchanged
        after = (a.results(), a.getFutureStatus(), a.cast_grid(), a.known_age(), a.cursors(), a.view())
        for x, y in zip(state[:4], after[:4]):
            assert np.array_equal(x, y)
        assert state[4] == after[4] and all(np.array_equal(x, y) for x, y in zip(state[5], after[5]))
        cb = a.counters()
        ca.pop("update_ms"), cb.pop("update_ms")
        assert ca == cb
        assert a.cast_grid_ptr() is not None and a.reach_fields_ptr() is not None
        again = (a.frontier_counts(), a.frontier_grid(), a.objects(), a.reach_field(0))
        assert layers[0] == again[0] and all(np.array_equal(x, y) for x, y in zip(layers[1:], again[1:]))
        assert np.array_equal(a.score_views(views, MAX_AGE, world=True), alone)
        assert all(np.array_equal(x, y) for x, y in zip(a.view_cells(views[0]), cells))
    # a following frame equals that of the twin that never called
    for m in (a, b):
        assert m.update(pts[4], (0.1, 0.0, 0.0), 0.2, G.QUATS["identity"]) == 1
    assert np.array_equal(a.results(), b.results()) and (a.results()[:, 0] > 0).any()
    fa, fb = a.getFutureStatus(), b.getFutureStatus()
    assert np.array_equal(fa, fb) and (fa != 0).any()
    ca, cb = a.counters(), b.counters()
    ca.pop("update_ms"), cb.pop("update_ms")
    assert ca == cb and a.cursors() == b.cursors()
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    # the layer without an integration since its last reset: the calls name the integration
    a.build_cast_grid(0.05, 0)
    a.reset_known()
    assert L.dspmap_score_view_sets(a.h, 48, 4, ptr(sets), MAX_AGE, 0, ptr(out), None) == E_STATE and b"dspmap_known_integrate" in err()
    assert L.dspmap_select_views(a.h, len(views), ptr(views), 0, MAX_AGE, 0, 16, 1, ptr(picks), None) == E_STATE and b"dspmap_known_integrate" in err()
    assert L.dspmap_select_views_device(a.h, len(views), dviews.data_ptr(), 0, MAX_AGE, 0, 16, 1, ptr(picks), None) == E_STATE and b"dspmap_known_integrate" in err()
    b.build_cast_grid(0.05, 0)                                            # a grid, but never an integration
    assert b.L.dspmap_score_view_sets_device(b.h, 48, 4, dviews.data_ptr(), MAX_AGE, 0, ptr(out), None) == E_STATE
    assert b"dspmap_known_integrate" in b.L.dspmap_last_error(b.h)
    assert not out.view(np.int32).any() and not picks.view(np.int32).any()
    a.close(), b.close()
