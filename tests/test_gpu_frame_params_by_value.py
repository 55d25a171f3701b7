"""The first kernel of a plain-launch frame takes the frame's parameter block as a kernel argument (k_obs_points<true, true>) while the
block is still pushed into the pinned ring and k_predict still advances the ring's read position; a replayed graph, and the estimator on
its own queue, read the ring slot as before (run with `-m gpu` on an MI355X).  Every case compares maps that queue plain launches with a
map forced onto the graph (DSPMAP_P_USE_GRAPH = 3), bit for bit: results grid, counters, particle export, future status and, with the
device estimator, the birth cloud.  A stale block, a block of another handle or a ring left behind by the plain frames cannot pass."""
import numpy as np
import pytest

from tests import common
from tests import config_edges as E

pytestmark = pytest.mark.gpu

CFG = dict(nx=16, ny=16, nz=6, res=0.15, ppv=24)
AUTO, RING, GRAPH = 1, 2, 3
COUNTS = (0, 1, 255, 256, 257, 600)        # below, at and above one workgroup of k_obs_points; no point at all
RING_SLOTS = 1024                          # DSPMAP_RING


def _make(dsp, est, mode, tables):
    m = dsp.DSPMap(dsp.make_config(**CFG))
    m.set_tables(*tables)
    m.L.dspmap_init_device(m.h)
    if est:
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, est)
    if mode is not None:
        m.set_param(dsp.capi.P_USE_GRAPH, mode)
    return m


def _frames(dsp, n_frames, seed):
    """every frame has its own position, attitude, time step and point count: the counts go through COUNTS in an order that changes with
    every round of six, the points are drawn from the map's wall + fan with per-frame noise"""
    base = E.observation_cloud(dsp.make_config(**CFG))
    rng = np.random.default_rng(seed)
    assert len(base) >= 600
    frames, t = [], 0.0
    for f in range(n_frames):
        if f % len(COUNTS) == 0:
            order = rng.permutation(len(COUNTS))
        n = COUNTS[order[f % len(COUNTS)]]
        t += 0.02 + 0.001 * (f % 23)
        a = 0.15 * np.sin(0.37 * f) + 0.002 * f
        quat = (float(np.cos(a / 2)), 0.0, 0.0, float(np.sin(a / 2)))
        if f % 7 == 3:
            quat = common.EX_QUATS[(f // 7) % 3]
        pos = (0.02 * np.sin(0.11 * f) + 0.0007 * f, -0.015 * np.cos(0.07 * f) - 0.0005 * f, 0.01 * np.sin(0.5 * f))
        idx = (np.arange(n) * 7 + 13 * f) % len(base)
        pts = (base[idx] + rng.normal(0, 0.004, (n, 3))).astype(np.float32)
        frames.append((pts, pos, quat, t))
    assert len({fr[1] for fr in frames}) == n_frames and len({fr[2] for fr in frames}) > n_frames // 2
    return frames


def _birth_cloud(dsp, pts, pos, rng):
    src = np.zeros(len(pts), dsp.VPOINT_DTYPE)
    src["x"] = pts[:, 0] + np.float32(pos[0]); src["y"] = pts[:, 1] + np.float32(pos[1]); src["z"] = pts[:, 2] + np.float32(pos[2])
    k = min(60, len(src))
    if k:
        dyn = rng.choice(len(src), k, replace=False)
        src["intensity"][dyn] = rng.uniform(0.1, 1.0, k)
        src["nx"][dyn] = rng.uniform(-1, 1, k); src["ny"][dyn] = rng.uniform(-1, 1, k)
        src["nx"][dyn[:k // 3]] = -10000; src["ny"][dyn[:k // 3]] = -10000; src["nz"][dyn[:k // 3]] = -10000
    return src


class _Feeder:
    """the frames' clouds on the device, uploaded once and shared by every map of a case"""

    def __init__(self, dsp, torch, frames, birth):
        self.frames = frames
        self.pts, self.src = [], []
        for f, (pts, pos, _, _) in enumerate(frames):
            self.pts.append(torch.from_numpy(pts if len(pts) else np.zeros((1, 3), np.float32)).cuda())
            if birth:
                src = _birth_cloud(dsp, pts, pos, np.random.default_rng(100 + f))
                self.src.append(torch.from_numpy(src.view(np.float32).reshape(-1, 7).copy() if len(pts) else np.zeros((1, 7), np.float32)).cuda())

    def feed(self, m, f):
        pts, pos, quat, t = self.frames[f]
        if self.src:
            assert m.update_device(self.pts[f].data_ptr(), len(pts), pos, t, quat, birth_dev_ptr=self.src[f].data_ptr(), n_birth=len(pts)) == 1
        else:
            assert m.update_device(self.pts[f].data_ptr(), len(pts), pos, t, quat) == 1


def _compare(maps, names, f, birth_cloud):
    ref = maps[0]
    a, ra, fa, ca = ref.export_state(), ref.results(), ref.getFutureStatus(), ref.counters()
    ca.pop("update_ms")
    ba = ref.get_birth_cloud() if birth_cloud else None
    for name, other in zip(names[1:], maps[1:]):
        cb = other.counters(); cb.pop("update_ms")
        assert ca == cb, (f, name, ca, cb)
        for x, y in zip(a, other.export_state()):
            assert np.array_equal(x, y), (f, name)
        assert np.array_equal(ra, other.results()), (f, name)
        assert np.array_equal(fa, other.getFutureStatus()), (f, name)
        if birth_cloud:
            bb = other.get_birth_cloud()
            assert ba.tobytes() == bb.tobytes(), (f, name, len(ba), len(bb))
    return a


def _clears(f):
    return f % 3 == 1 or f % 10 == 0           # clearOccupancyMapPrediction before some frames, not before others


def _run(feeder, maps, names, check_at, birth_cloud, per_frame=None):
    state = None
    for f in range(len(feeder.frames)):
        for k, m in enumerate(maps):
            if per_frame:
                per_frame(f, k, m)
            if _clears(f):
                m.clearOccupancyMapPrediction()
            feeder.feed(m, f)
        if f in check_at or f == len(feeder.frames) - 1:
            state = _compare(maps, names, f, birth_cloud)
    return state


@pytest.mark.parametrize("est,birth,mode", [(0, False, AUTO), (2, False, AUTO), (2, False, RING), (0, True, RING)])
def test_changing_values_every_frame(dsp, est, birth, mode, monkeypatch):
    """36 frames, each with its own position, attitude, time step and point count (0, 1, 255, 256, 257, 600 in changing order), a pending
    clear of the future accumulators before some of them: without the estimator, with the device estimator on its own queue, and with a
    caller-supplied birth cloud on a map that is asked for plain launches (value 2).  Equal to the graph-forced map at every sixth frame."""
    import torch
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    tables = common.tables(5)
    frames = _frames(dsp, 36, seed=11)
    feeder = _Feeder(dsp, torch, frames, birth)
    maps = [_make(dsp, est, GRAPH, tables), _make(dsp, est, mode if mode != AUTO else None, tables)]
    state = _run(feeder, maps, ["graph", "plain"], set(range(5, 36, 6)), birth_cloud=est == 2)
    assert len(state[0]) > 200
    assert maps[0].plain_frames() == 0 and maps[1].plain_frames() == len(frames)
    if est == 2:
        assert maps[1].estimator_path() == "own_stream"
        assert maps[1].estimator_queue()[3] == 0
    for m in maps:
        m.close()


@pytest.mark.parametrize("est", [0, 2])
def test_ring_wrap_and_switches(dsp, est, monkeypatch):
    """More frames than the ring has slots on one handle of plain launches -- across the wrap and four of the ring's events -- then, in the
    middle of the run, the same handle goes 1 -> 3 -> 2 -> 3: the graph frames find the ring's read position where the plain frames
    left it, and the plain frames theirs behind the graph's.  Equal to a map that replayed its graph all the way."""
    import torch
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    tables = common.tables(6)
    n_plain = RING_SLOTS + 60
    frames = _frames(dsp, n_plain + 36, seed=12)
    feeder = _Feeder(dsp, torch, frames, False)
    maps = [_make(dsp, est, GRAPH, tables), _make(dsp, est, None, tables)]
    switches = {n_plain: GRAPH, n_plain + 12: RING, n_plain + 24: GRAPH}

    def per_frame(f, k, m):
        if k == 1 and f in switches:
            m.set_param(dsp.capi.P_USE_GRAPH, switches[f])

    check_at = {255, 256, RING_SLOTS - 1, RING_SLOTS, RING_SLOTS + 1, n_plain - 1, n_plain, n_plain + 11, n_plain + 12, n_plain + 23, n_plain + 24}
    state = _run(feeder, maps, ["graph", "switching"], check_at, birth_cloud=est == 2, per_frame=per_frame)
    assert len(state[0]) > 200
    assert maps[0].plain_frames() == 0 and maps[1].plain_frames() == n_plain + 12
    if est == 2:
        assert maps[1].estimator_queue()[3] == 0
    for m in maps:
        m.close()


def test_three_handles_interleaved(dsp, monkeypatch):
    """Three handles of plain launches with the device estimator, each on a stream of frames of its own, interleaved frame by frame: the block
    a handle's kernels get is never the one pushed last in the process.  Each equal to its graph-forced twin."""
    import torch
    monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    tables = common.tables(7)
    feeders = [_Feeder(dsp, torch, _frames(dsp, 30, seed=20 + k), False) for k in range(3)]
    plain = [_make(dsp, 2, mode, tables) for mode in (None, RING, None)]
    graph = [_make(dsp, 2, GRAPH, tables) for _ in range(3)]
    for f in range(30):
        for k in range(3):
            if _clears(f + k):
                plain[k].clearOccupancyMapPrediction()
            feeders[k].feed(plain[k], f)
        for k in range(3):
            if _clears(f + k):
                graph[k].clearOccupancyMapPrediction()
            feeders[k].feed(graph[k], f)
        if f % 10 == 9:
            for k in range(3):
                _compare([graph[k], plain[k]], ["graph", "plain%d" % k], f, True)
    assert [m.plain_frames() for m in plain] == [30] * 3 and [m.plain_frames() for m in graph] == [0] * 3
    first = [m.export_state()[2] for m in plain]
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])     # (three different runs)
    for m in plain + graph:
        m.close()


def test_deferred_shares_behind_by_value_frames(dsp, monkeypatch):
    """Test hook DSPMAP_XQ_TEST_DELAY_US on plain-launch and graph-forced handles alike: every third frame's estimator is held back and the
    frame's first birth kernel -- which takes the frame's number from the copy of the block that k_obs_points stored -- takes that frame's cloud
    for unfinished at its first look: workgroup 0 waits, the others leave their shares to it.  Same bits and the same diagnostics: frames on the estimator's
    queue, both hand-over words, no give-up, and the forced frames counted as frames in which somebody had to wait in both maps.  (A frame
    that is NOT forced may find the word late on its own, so the count of waiting frames has a floor, not a value; the shares done for others
    are counted per workgroup, and a replayed frame's grid is sized for the capacity, a plain frame's for its cloud.)"""
    import torch
    monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    monkeypatch.setenv("DSPMAP_XQ_TEST_DELAY_US", "2000")
    tables = common.tables(6)
    ref = _make(dsp, 2, GRAPH, tables)                     # (the hooks are read when a handle is created)
    held = _make(dsp, 2, RING, tables)
    monkeypatch.delenv("DSPMAP_XQ_TEST_DELAY_US")
    # every frame with points: a frame without any has no birth kernel to look at the word
    frames = [fr for fr in _frames(dsp, 48, seed=13) if len(fr[0]) > 0][:36]
    feeder = _Feeder(dsp, torch, frames, False)
    _run(feeder, [ref, held], ["graph", "held_plain"], {11, 23}, birth_cloud=True)
    q, qr = held.estimator_queue(), ref.estimator_queue()
    assert held.plain_frames() == len(frames) and ref.plain_frames() == 0
    print("estimator queue, plain:", q, "graph:", qr)
    assert q[0] == len(frames) and q[3] == 0 and q[:4] == qr[:4], (q, qr)
    # frames 1, 4, ..., 34 are forced: 12 of them in either map
    assert q[4] >= 12 and qr[4] >= 12 and q[5] > 0 and qr[5] > 0, (q, qr)
    held.close(); ref.close()
