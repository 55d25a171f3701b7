"""How a frame is queued (DSPMAP_P_USE_GRAPH; run with `-m gpu` on an MI355X): by default a small map's single-chain frames go out as plain
launches with their parameter block in the pinned ring (what the value 2 asks for everywhere), everything else as a replayed graph (what
3 forces); 0 copies the parameter block.  Nothing a map computes may depend on which of the four queued its frames.  (The file's name is
the plan's: a pre-packed launch list was to issue those launches; it did not lower their host time and was left out, LOG.md.)"""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import config_edges as E

pytestmark = pytest.mark.gpu

CFGS = {
    "20x20x8": dict(nx=20, ny=20, nz=8, res=0.15, ppv=24),
    "24x20x12": dict(nx=24, ny=20, nz=12, res=0.15, ppv=24),
    "slots66": dict(E.EDGES["slots66"]["cfg"]),      # two occupancy words: k_predict<2>, k_place<2>, k_resample_wg<2>
}
N_FRAMES = 40
CHECK_AT = (9, 19, 29, 39)
AUTO, RING, GRAPH, PLAIN = 1, 2, 3, 0      # RING: plain launches + parameter ring; PLAIN: plain launches + copied parameters


def _stream(dsp, cfg, seed=3, n_frames=N_FRAMES, identity=False):
    """tests/common.py's wall (through config_edges.observation_cloud: inside this map's box, plus the fan) with per-frame noise and a moving,
    turning sensor; frame 7 has no point at all, frame 12 exactly as many points as the handle's buffers hold after the first frame
    (dspmap_ensure_point_cap: n + n / 2 + 1024 -- the captured grids are sized for that number, the plain launches' for the frame's cloud)"""
    base = E.observation_cloud(dsp.make_config(**cfg))
    rng = np.random.default_rng(seed)
    n0 = len(base)
    cap = n0 + n0 // 2 + 1024
    assert cap <= 6144                                   # (the device estimator takes it)
    frames = []
    for f in range(n_frames):
        t = f / 30.0
        if f == 7:
            pts = np.zeros((0, 3), np.float32)
        elif f == 12:
            pts = base[np.arange(cap) % n0]
        else:
            pts = base
        pts = (pts + rng.normal(0, 0.004, pts.shape)).astype(np.float32)
        pos = (0.3 * t, -0.2 * t, 0.05 * np.sin(5 * t))
        quat = (1.0, 0.0, 0.0, 0.0) if identity else common.EX_QUATS[(f // 4) % 3]
        frames.append((pts, pos, quat, t))
    return frames


def _birth_cloud(dsp, pts, pos, rng):
    """a caller-supplied tagged birth cloud for the frame's points: most static, some with a velocity, some marked unknown"""
    src = np.zeros(len(pts), dsp.VPOINT_DTYPE)
    src["x"] = pts[:, 0] + np.float32(pos[0]); src["y"] = pts[:, 1] + np.float32(pos[1]); src["z"] = pts[:, 2] + np.float32(pos[2])
    k = min(80, len(src))
    if k:
        dyn = rng.choice(len(src), k, replace=False)
        src["intensity"][dyn] = rng.uniform(0.1, 1.0, k)
        src["nx"][dyn] = rng.uniform(-1, 1, k); src["ny"][dyn] = rng.uniform(-1, 1, k)
        src["nx"][dyn[:k // 3]] = -10000; src["ny"][dyn[:k // 3]] = -10000; src["nz"][dyn[:k // 3]] = -10000
    return src


def _make(dsp, cfg, est, mode, tables, sweep_alt=None):
    m = dsp.DSPMap(dsp.make_config(**cfg))
    m.set_tables(*tables)
    m.L.dspmap_init_device(m.h)
    if est:
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, est)
    if sweep_alt is not None:
        m.set_param(dsp.capi.P_SWEEP_ALTERNATE, sweep_alt)
    if mode is not None:
        m.set_param(dsp.capi.P_USE_GRAPH, mode)
        assert m.get_param(dsp.capi.P_USE_GRAPH) == mode
    return m


def _feed(dsp, torch, m, feed, frame, keep, rng_seed):
    pts, pos, quat, t = frame
    n = len(pts)
    if feed == "host":
        assert m.update(pts, pos, t, quat) == 1
        return
    d_pts = torch.from_numpy(pts if n else np.zeros((1, 3), np.float32)).cuda()
    keep.append(d_pts)
    if feed == "device":
        assert m.update_device(d_pts.data_ptr(), n, pos, t, quat) == 1
    else:
        src = _birth_cloud(dsp, pts, pos, np.random.default_rng(rng_seed))
        d_src = torch.from_numpy(src.view(np.float32).reshape(-1, 7).copy() if n else np.zeros((1, 7), np.float32)).cuda()
        keep.append(d_src)
        assert m.update_device(d_pts.data_ptr(), n, pos, t, quat, birth_dev_ptr=d_src.data_ptr(), n_birth=n) == 1


def _compare(maps, names, f):
    """full state export, results grid, future status and counters of every map against the first one's: zero differences"""
    ref = maps[0]
    a, ra, fa, ca = ref.export_state(), ref.results(), ref.getFutureStatus(), ref.counters()
    ca.pop("update_ms")
    for name, other in zip(names[1:], maps[1:]):
        cb = other.counters(); cb.pop("update_ms")
        assert ca == cb, (f, name, ca, cb)
        for x, y in zip(a, other.export_state()):
            assert np.array_equal(x, y), (f, name)
        assert np.array_equal(ra, other.results()), (f, name)
        assert np.array_equal(fa, other.getFutureStatus()), (f, name)
    return a, fa


def _run(dsp, torch, maps, names, feed, frames, per_frame=None, between=None):
    keep = []
    for f, frame in enumerate(frames):
        if between:
            between(f, maps)
        for k, m in enumerate(maps):
            if per_frame:
                per_frame(f, k, m)
            _feed(dsp, torch, m, feed, frame, keep, 100 + f)
        if f in CHECK_AT or f == len(frames) - 1:
            state, fut = _compare(maps, names, f)
            keep = keep[-4:]
        for m in maps:
            m.clearOccupancyMapPrediction()
    return state, fut


CASES = [(c, est, feed) for c, est, feed in
         [("20x20x8", 0, "device"), ("20x20x8", 2, "device"), ("20x20x8", 0, "host"), ("20x20x8", 2, "host"), ("20x20x8", 0, "birth"),
          ("24x20x12", 0, "device"), ("24x20x12", 2, "device"), ("24x20x12", 2, "host"),
          ("slots66", 0, "device"), ("slots66", 2, "device"), ("slots66", 2, "host")]]


@pytest.mark.parametrize("cfg_name,est,feed", CASES)
def test_how_the_frame_is_queued_changes_nothing(dsp, cfg_name, est, feed, monkeypatch):
    """Five maps on one stream of 40 frames (one without points, one with as many as the buffers hold): plain launches with a copied
    parameter block (DSPMAP_P_USE_GRAPH = 0, the reference of the comparison), the default (1: these small maps' device-resident frames go
    out as plain launches through the ring), those asked for (2), the graph forced (3), and a map that goes through 1, 2, 3, 0 switching
    every 5 frames -- a frame of every kind behind a frame of every other.  With the device estimator (on its own queue) and without,
    fed through dspmap_update_device, through the host-pointer dspmap_update (which keeps its one graph launch under the default) and
    with a caller-supplied birth cloud.  Counters, every slot and float, results and future status equal at four
    checkpoints; which path ran is read back from the handles."""
    import torch
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")      # (a handle that cannot give the estimator its own queue fails instead of forking)
    cfg = CFGS[cfg_name]
    tables = common.tables(5)
    names = ["plain0", "auto", "ring", "graph", "switch"]
    maps = [_make(dsp, cfg, est, mode, tables) for mode in (PLAIN, None, RING, GRAPH, None)]
    assert maps[1].get_param(dsp.capi.P_USE_GRAPH) == 1     # the reported default
    cycle = (AUTO, RING, GRAPH, PLAIN)

    def per_frame(f, k, m):
        if k == 4 and f % 5 == 0:
            m.set_param(dsp.capi.P_USE_GRAPH, cycle[(f // 5) % 4])

    state, fut = _run(dsp, torch, maps, names, feed, _stream(dsp, cfg, identity=feed == "birth"), per_frame)
    assert len(state[0]) > 500 and fut.max() > 0
    got = [m.plain_frames() for m in maps]
    device_frame = feed != "host" or est == 2               # (host cloud without the device estimator: the frame with host stages, never replayed)
    want_ring = N_FRAMES if device_frame else 0
    want_auto = want_ring if feed != "host" else 0          # host-cloud frames of the default stay on the graph (include/dspmap.h)
    assert got[0] == 0 and got[3] == 0, got
    assert got[2] == want_ring and got[1] == want_auto, got
    assert got[4] == (want_auto + want_ring) // 4, got      # its frames 0-4 and 20-24 on the default, 5-9 and 25-29 on 2
    if est == 2:
        # (the copied-parameter frames -- the first map's, the last map's last five -- keep the estimator as a forked branch)
        assert all(m.estimator_path() == "own_stream" for m in maps[1:4]), [m.estimator_path() for m in maps]
    for m in maps:
        m.close()


@pytest.mark.parametrize("est", [0, 2])
def test_both_sweep_directions_and_every_invalidation(dsp, est, tmp_path, monkeypatch):
    """DSPMAP_P_SWEEP_ALTERNATE = 1: the sweep direction is a kernel argument and flips with every frame, so two executable graphs are alive
    in the maps that replay.  Between frames: dspmap_clear_state and an import of flag-15 records at frame 8 (the velocity-noise variant of k_predict for two frames: another
    key), dspmap_clear_state at frame 16, a checkpoint saved at frame 22 and restored at frame 30 -- each invalidates the graph.  Default,
    ring, graph and copied-parameter maps stay equal to the last bit."""
    import torch
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    cfg = CFGS["24x20x12"]
    tables = common.tables(7)
    names = ["plain0", "auto", "ring", "graph"]
    maps = [_make(dsp, cfg, est, mode, tables, sweep_alt=1) for mode in (PLAIN, None, RING, GRAPH)]
    c = dsp.make_config(**cfg)
    px, py, pz, vx, vy, w = common.random_particles(9, 3000, common.half_extent(c))
    o_rec = np.stack([np.full(len(px), 15.0, np.float32), vx, vy, np.zeros_like(px), px, py, pz, w], 1).astype(np.float32)
    voxel = np.array([maps[0].getPointVoxelsIndexPublic(float(a), float(b), float(cc))[1] for a, b, cc in zip(px, py, pz)], np.int32)
    order = np.argsort(voxel, kind="stable")
    voxel, o_rec = voxel[order], o_rec[order]
    # explicit slots (the rank inside the voxel) into a cleared map: "first free slot" is decided by whichever thread comes first
    slot = (np.arange(len(voxel)) - np.searchsorted(voxel, voxel, side="left")).astype(np.int32)
    assert slot.max() < 2 * cfg["ppv"]

    def between(f, ms):
        for k, m in enumerate(ms):
            if f == 8:
                m.clear_state()
                m.import_state(voxel, o_rec, slot)
            elif f == 16:
                m.clear_state()
            elif f == 22:
                m.save_checkpoint(tmp_path / ("ck_%d.bin" % k))
            elif f == 30:
                m.load_checkpoint(tmp_path / ("ck_%d.bin" % k))

    state, fut = _run(dsp, torch, maps, names, "device", _stream(dsp, cfg, seed=4), between=between)
    assert len(state[0]) > 500
    got = [m.plain_frames() for m in maps]
    assert got == [0, N_FRAMES, N_FRAMES, 0], got
    for m in maps:
        m.close()


def test_five_handles_interleaved_as_plain_launches(dsp, monkeypatch):
    """Five handles with the device estimator alive in one process, their frames interleaved: four queue plain launches (two by default, two
    asked to), one replays its graph -- ten or more streams on the device's hardware queues, every cross-queue wait for work
    queued earlier.  Same bits on all five."""
    import torch
    monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    cfg = CFGS["20x20x8"]
    tables = common.tables(6)
    names = ["graph", "auto_a", "ring_a", "auto_b", "ring_b"]
    maps = [_make(dsp, cfg, 2, mode, tables) for mode in (GRAPH, None, RING, None, RING)]
    _run(dsp, torch, maps, names, "device", _stream(dsp, cfg, seed=8))
    assert [m.plain_frames() for m in maps] == [0] + [N_FRAMES] * 4
    q = [m.estimator_queue() for m in maps]
    assert all(x[0] == N_FRAMES and x[1] == N_FRAMES and x[2] == N_FRAMES and x[3] == 0 for x in q), q
    for m in maps:
        m.close()


def test_deferred_shares_branch_runs_behind_plain_launches(dsp, monkeypatch):
    """Test hook DSPMAP_XQ_TEST_DELAY_US on a handle that queues plain launches: every third frame's estimator is held back 2 ms and the frame's first
    birth kernel takes that frame's cloud for unfinished at its first look -- workgroup 0 waits, the others leave their shares to it.  Same bits as a graph-replaying map without the hook."""
    import torch
    monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    monkeypatch.setenv("DSPMAP_XQ_TEST_DELAY_US", "2000")
    cfg = CFGS["20x20x8"]
    tables = common.tables(6)
    held = _make(dsp, cfg, 2, RING, tables)                 # (the hooks are read when a handle is created)
    monkeypatch.delenv("DSPMAP_XQ_TEST_DELAY_US")
    ref = _make(dsp, cfg, 2, GRAPH, tables)
    _run(dsp, torch, [ref, held], ["graph", "held_ring"], "device", _stream(dsp, cfg, seed=8))
    q = held.estimator_queue()
    assert held.plain_frames() == N_FRAMES and q[0] == N_FRAMES and q[3] == 0, q
    # frames 1, 4, 7, ..., 37 are held back: 13 of them; frame 7 has no point (its birth kernel may have nothing to look at) and the hook's
    # count starts with the handle's first estimator launch: 11 at the least
    assert q[4] >= 11 and q[5] > 0, q
    held.close(); ref.close()
