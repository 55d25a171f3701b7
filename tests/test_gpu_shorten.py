"""GPU tests of the shortened paths (dspmap_shorten_paths*): bit parity -- zero mismatches in every int of the infos and ends and every
uint32 of the segment records -- with the numpy restatement (tests/shorten_ref.py), and the restatement's checker on the DEVICE's own
output.  Paths of the timeline through hand-made grids fed by set_cast_grid (a door that opens, time-invariant clutter, clutter that
changes with every layer) at the windows 1, 7 and 64; caller-made random walks with waits and jumps on the shapes where the word logic
and the wave logic can break, with paths of exactly 65 and 66 cells; max_seg's edges; static calls; the device chain timeline paths ->
shorten -> casts -> boxes without a host copy, on a hand-made grid and right behind a frame and the grid's build; the state errors; and
read-only behaviour."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cast_ref as CR
from tests import reach_ref as R
from tests import reach_time_ref as TR
from tests import shorten_ref as S
from tests.test_gpu_cast import SMALL, _median_threshold, _twins
from tests.test_gpu_query import _run, _scene_frames
from tests.test_gpu_reach import _blank_map, _grid_cells, _shift, _sources

pytestmark = pytest.mark.gpu
F = np.float32
OK, E_STATE = 1, -3


def _assert_same(got, want, tag):
    """(info, seg, end) against the restatement's: zero differing bits"""
    gi, gs, ge = got
    wi, ws, we = want
    gi = S.info_of(gi.cpu().numpy()) if torch.is_tensor(gi) else gi
    gs, ge = (a.cpu().numpy() if torch.is_tensor(a) else a for a in (gs, ge))
    assert gi.dtype == S.INFO_DTYPE and gi.shape == wi.shape, tag
    for k in S.INFO_DTYPE.names:
        bad = np.flatnonzero(gi[k] != wi[k])
        assert bad.size == 0, (tag, k, bad.size, bad[:5], gi[k][bad[:5]], wi[k][bad[:5]])
    assert ge.dtype == np.int32 and ge.shape == we.shape, tag
    bad = np.argwhere(ge != we)
    assert bad.shape[0] == 0, (tag, "end", bad.shape[0], bad[:5])
    assert gs.dtype == np.float32 and gs.shape == ws.shape, tag
    bad = np.argwhere(np.ascontiguousarray(gs).view(np.uint32) != np.ascontiguousarray(ws).view(np.uint32))
    assert bad.shape[0] == 0, (tag, "seg", bad.shape[0], bad[:5])


def _case(m, lay, steps, cells, tag, **kw):
    """one host call held against the restatement and the checker; returns the device's (info, seg, end) and the checker's counts"""
    got = m.shorten_paths(steps, cells, **kw)
    _assert_same(got, S.shorten(m.cfg, lay, steps, cells, **kw), tag)
    ck = {k: v for k, v in kw.items() if k != "max_seg"}
    return got, S.check(m.cfg, lay, steps, cells, *got, **ck)


@pytest.mark.parametrize("scene", ["door", "invariant", "clutter"])
def test_shorten_timeline_paths_bit_for_bit(dsp, scene):
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
    for sched in scheds:
        m.build_reach_timeline(src, nf, **sched)
        steps, cells = m.reach_timeline_paths(starts, sched["max_steps"] + 1)
        assert (steps >= 0).sum() >= 4
        ts = dict(t_start=sched["t_start"], step_seconds=sched["step_seconds"])
        longest = {}
        for window in (1, 7, 64):
            (info, seg, end), (n_seg, n_blocked, n_trunc, longest[window]) = _case(m, lay, steps, cells, (scene, sched["t_start"], window),
                                                                                    window=window, **ts)
            assert n_trunc == 0 and n_seg >= 4 and np.array_equal(info["n_cells"], np.where(steps >= 0, steps + 1, 0))
            if window == 1:
                assert np.array_equal(info["n_segments"], np.maximum(info["n_cells"] - 1, 0))
            if scene == "door" and window == 64:          # the answers worked by hand in tests/test_shorten_cpu.py
                assert end[0, :4].tolist() == [5, 6, 16, -1] and info["n_blocked"][:4].tolist() == [1, 1, 0, 0]
            if scene == "invariant":                     # a path of the wavefront never crosses an occupied cell of its one layer
                assert n_blocked == 0
                if sched is TR.FROZEN and window == 64:   # ... and the result does not depend on step_seconds
                    other = m.shorten_paths(steps, cells, t_start=0.3, step_seconds=0.4, window=64)
                    assert np.array_equal(other[0], info) and np.array_equal(other[2], end)
                    assert np.array_equal(other[1][..., :3], seg[..., :3]) and np.array_equal(other[1][..., 4:7], seg[..., 4:7])
        assert longest[1] == 1 and 1 < longest[7] <= 7 < longest[64]
        if sched["t_start"] >= 0:                         # the static call on the same cells: layer 0, every time -1
            (info0, seg0, end0), _ = _case(m, lay, steps, cells, (scene, "static"), window=64)
            used = np.arange(seg0.shape[1])[None, :] < info0["n_segments"][:, None]
            assert (seg0[used][:, [3, 7]] == -1).all()
    m.close()


SHAPES = {"64x6x3": dict(nx=64, ny=6, nz=3, res=0.15, ppv=12),
          "65x6x3": dict(nx=65, ny=6, nz=3, res=0.15, ppv=12),
          "132x40x12": dict(nx=132, ny=40, nz=12, res=0.15, ppv=9),
          "50x37x23": dict(nx=50, ny=37, nz=23, res=0.15, ppv=12),
          "t0": dict(nx=40, ny=40, nz=24, res=0.15, ppv=12, pred_times=())}
MAX_LEN = 160


def _random_walks(cfg, lay, n, seed):
    """(steps [n], cells [n, MAX_LEN]): caller-made paths -- face steps, waits (15 %), jumps to any cell (3 %); the even ones keep to cells
    free in every layer where they can.  Path 0 has exactly 65 cells and path 1 exactly 66 (a window of 64 from the first cell ends one
    short of and one past the last one), paths 2, 9 and 10 fill the row, the others have 1 .. MAX_LEN cells; steps are cells - 1 (a wavefront's),
    except for a few that are smaller (clamped at 0), larger, or negative (no path); two rows are ended by an index outside [0, V)"""
    rng = np.random.default_rng(seed)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    occ = lay.any(0)
    cells = np.full((n, MAX_LEN), -1, np.int32)
    steps = np.zeros(n, np.int32)
    moves = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])
    for i in range(n):
        length = {0: 65, 1: 66, 2: MAX_LEN, 9: MAX_LEN, 10: MAX_LEN}.get(i, int(rng.integers(1, MAX_LEN + 1)))
        c = rng.integers(0, nn)
        for j in range(length):
            cells[i, j] = (c[2] * cfg.ny + c[1]) * cfg.nx + c[0]
            u = rng.random()
            if u < 0.15:
                continue
            if u < 0.18:
                c = rng.integers(0, nn)
                continue
            cand = c[None, :] + moves
            cand = cand[((cand >= 0) & (cand < nn)).all(1)]
            if i % 2 == 0:
                free = cand[~occ[cand[:, 2], cand[:, 1], cand[:, 0]]]
                cand = free if len(free) else cand
            c = cand[rng.integers(0, len(cand))]
        steps[i] = length - 1
    steps[5], steps[6], steps[7], steps[8] = 3, 4000, -1, -3
    V = int(nn.prod())
    cells[9, 40], cells[10, 64] = V, -2
    return steps, cells


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shorten_caller_made_paths_on_awkward_shapes(dsp, shape):
    m = _blank_map(dsp, SHAPES[shape], seed=77)
    cfg = m.cfg
    assert m.T == (0 if shape == "t0" else 6)
    rng = np.random.default_rng(4)
    lay = rng.random((m.T + 1, cfg.nz, cfg.ny, cfg.nx)) < 0.10
    m.set_cast_grid(R.pack(lay))
    steps, cells = _random_walks(cfg, lay, 64, 21)
    timed = dict(t_start=0.0, step_seconds=0.03)                              # 0 .. 4.8 s over 2.0 s of predictions: every layer
    blocked = 0
    for kw in (dict(window=64, **timed), dict(window=5, **timed), dict(window=64), dict(window=63, t_start=0.3, step_seconds=0.0)):
        (info, seg, end), (n_seg, n_blocked, n_trunc, longest) = _case(m, lay, steps, cells, (shape, kw), **kw)
        assert info["n_cells"][:3].tolist() == [65, 66, MAX_LEN] and info["n_cells"][7:11].tolist() == [0, 0, 40, 64]
        assert n_trunc == 0 and n_seg > 64 and longest <= kw["window"]
        blocked += n_blocked
    assert blocked > 0                                                        # walks through 10 % clutter are cut somewhere
    if shape == "t0":                                                         # no horizons: every time is -1, whatever t_start says
        a, b = m.shorten_paths(steps, cells, window=64, **timed), m.shorten_paths(steps, cells, window=64)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # in an empty grid a window of 64 takes the 65-cell path in one piece and the 66-cell path in two
    m.set_cast_grid(R.pack(np.zeros_like(lay)))
    (info, seg, end), _ = _case(m, np.zeros_like(lay), steps, cells, (shape, "empty"), window=64, **timed)
    assert end[0, :2].tolist() == [64, -1] and end[1, :3].tolist() == [64, 65, -1] and end[2, :4].tolist() == [64, 128, 159, -1]
    m.close()


def test_shorten_max_seg_edges(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay, src, nf, starts, sched = TR.changing_clutter_scene(cfg)
    m.set_cast_grid(R.pack(lay))
    m.build_reach_timeline(src, nf, **sched)
    steps, cells = m.reach_timeline_paths(starts, 121)
    ts = dict(t_start=sched["t_start"], step_seconds=sched["step_seconds"], window=9)
    full = S.shorten(cfg, lay, steps, cells, **ts)
    most = int(full[0]["n_segments"].max())
    assert most >= 4 and full[1].shape[1] == 120
    for max_seg in (0, 1, 2, most - 1, most, most + 3, 120, 131):
        got = m.shorten_paths(steps, cells, max_seg=max_seg, **ts)
        assert got[1].shape == (len(steps), max_seg, 8) and got[2].shape == (len(steps), max_seg)
        keep = min(max_seg, 120)
        cut = full[0]["n_segments"] > max_seg
        assert np.array_equal(got[0]["truncated"] != 0, cut) and cut.any() == (max_seg < most)
        assert np.array_equal(got[0]["n_segments"], np.minimum(full[0]["n_segments"], max_seg))
        assert np.array_equal(got[2][:, :keep], full[2][:, :keep]) and (got[2][:, keep:] == -1).all()
        assert np.array_equal(got[1][:, :keep].view(np.uint32), full[1][:, :keep].view(np.uint32)) and not got[1][:, keep:].any()
        _assert_same(got, S.shorten(cfg, lay, steps, cells, max_seg=max_seg, **ts), ("max_seg", max_seg))
        S.check(cfg, lay, steps, cells, *got, t_start=ts["t_start"], step_seconds=ts["step_seconds"], window=9)
    # through the C ABI: no segment arrays with max_seg == 0, no arrays at all with n == 0; max_len == 1: no path has a segment
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    info = np.zeros(len(steps), S.INFO_DTYPE)
    assert m.L.dspmap_shorten_paths(m.h, len(steps), 121, p(steps), p(cells), 0.0, 0.02, 9, 0, 0, p(info), None, None) == OK
    assert np.array_equal(info["n_cells"], full[0]["n_cells"]) and np.array_equal(info["truncated"], (full[0]["n_cells"] > 1).astype(np.int32))
    assert m.L.dspmap_shorten_paths(m.h, 0, 121, None, None, 0.0, 0.02, 9, 4, 0, None, None, None) == OK
    one = m.shorten_paths(steps, cells[:, :1].copy(), max_seg=3, **ts)
    assert one[0]["n_cells"].tolist() == (steps >= 0).astype(int).tolist() and not one[0]["n_segments"].any() and (one[2] == -1).all()
    m.close()


def _device_chain(m, td, sched, world, max_seg, grow):
    """timeline paths -> shorten -> casts -> boxes on tensors, nothing copied to the host in between"""
    steps, cells = m.reach_timeline_paths(td, sched["max_steps"] + 1, world=world)
    info, seg, end = m.shorten_paths(steps, cells, t_start=sched["t_start"], step_seconds=sched["step_seconds"], window=64, max_seg=max_seg)
    assert all(torch.is_tensor(x) and x.is_cuda for x in (info, seg, end)) and seg.shape == (td.shape[0], max_seg, 8)
    hits = m.cast_segments(seg.view(-1, 8))
    boxes = m.grow_boxes(seg.view(-1, 8), grow)
    return steps, cells, info, seg, end, hits, boxes


def _host_route(m, starts, sched, world, max_seg, grow):
    steps, cells = m.reach_timeline_paths(starts, sched["max_steps"] + 1, world=world)
    info, seg, end = m.shorten_paths(steps, cells, t_start=sched["t_start"], step_seconds=sched["step_seconds"], window=64, max_seg=max_seg)
    return steps, cells, info, seg, end, m.cast_segments(seg.reshape(-1, 8)), m.grow_boxes(seg.reshape(-1, 8), grow)


def _assert_same_routes(dev, host, tag):
    ds, dc, di, dseg, dend, dh, db = dev
    hs, hc, hi, hseg, hend, hh, hb = host
    assert np.array_equal(ds.cpu().numpy(), hs) and np.array_equal(dc.cpu().numpy(), hc), tag
    _assert_same((di, dseg, dend), (hi, hseg, hend), tag)
    for k in ("s", "voxel", "layer", "status"):
        assert dh[k].cpu().numpy().tobytes() == np.ascontiguousarray(hh[k]).tobytes(), (tag, k)
    for k in ("lo", "hi", "status", "stop"):
        assert np.ascontiguousarray(db[k].cpu().numpy()).tobytes() == np.ascontiguousarray(hb[k]).tobytes(), (tag, k)
    # what the consumers make of the records: every used segment that is not counted as blocked casts FREE
    used = (np.arange(hend.shape[1])[None, :] < hi["n_segments"][:, None]).reshape(-1)
    free = hh["status"] == CR.FREE
    assert (used & ~free).sum() == hi["n_blocked"].sum(), tag
    return int(used.sum())


def test_shorten_device_chain_equals_the_host_route(dsp):
    m = _blank_map(dsp, dict(SMALL))
    cfg = m.cfg
    lay, src, nf, starts, sched = TR.changing_clutter_scene(cfg)
    m.set_cast_grid(R.pack(lay))
    m.build_reach_timeline(src, nf, **sched)
    wide = torch.from_numpy(np.concatenate([starts.view(np.int32).reshape(-1, 4)] * 2, 1)).cuda()
    td = wide[:, :4]                                                          # a non-contiguous view: the binding's temporary
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    with torch.cuda.stream(st):
        dev = _device_chain(m, td, sched, False, 24, (4, 4, 2))
        # strided inputs: the binding makes them contiguous
        both = torch.stack([dev[1], dev[1]], 2)
        again = m.shorten_paths(dev[0], both[:, :, 0], t_start=sched["t_start"], step_seconds=sched["step_seconds"], window=64, max_seg=24)
        st.synchronize()
        host = _host_route(m, starts, sched, False, 24, (4, 4, 2))
    assert all(torch.equal(a, b) for a, b in zip(again, dev[2:5]))
    assert _assert_same_routes(dev, host, "chain") >= 100
    want = S.shorten(cfg, lay, host[0], host[1], t_start=sched["t_start"], step_seconds=sched["step_seconds"], window=64, max_seg=24)
    _assert_same(host[2:5], want, "chain against the restatement")
    S.check(cfg, lay, host[0], host[1], *host[2:5], t_start=sched["t_start"], step_seconds=sched["step_seconds"])
    m.close()


# the seeded twins hold mass everywhere: at 0.3 their grid after six frames is 1 - 2 % occupied per layer raw and 7 - 56 % inflated by 2,
# the layers differing -- room for paths, and layers that change under them.  (At 0.05 the inflated grid is full.)
THR = 0.3


@pytest.mark.parametrize("inflate", [0, 2])
def test_shorten_device_chain_behind_a_frame(dsp, inflate):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 6, seed=31)
    (m,) = _twins(dsp, kw, 1)
    cfg = m.cfg
    cur = np.array(frames[-1][1], F)
    src = _shift(_sources(cfg, 400, 4, 13), cur)
    starts = _shift(_sources(cfg, 200, 4, 14), cur)
    sd = torch.from_numpy(src.view(np.int32).reshape(-1, 4).copy()).cuda()
    td = torch.from_numpy(starts.view(np.int32).reshape(-1, 4).copy()).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    sched = dict(t_start=0.0, step_seconds=0.02, max_steps=120)
    with torch.cuda.stream(st):
        outs = []
        for pts, pos, quat, t in frames:
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            m.build_cast_grid(THR, inflate)                                   # no synchronisation between the frame, the builds and the chain
            m.build_reach_timeline(sd, 4, world=True, **sched)
            outs.append(_device_chain(m, td, sched, True, 32, (6, 6, 3)))
        st.synchronize()
        lay = _grid_cells(m)
        m.build_reach_timeline(src, 4, world=True, **sched)                   # the host variants on the same grid
        host = _host_route(m, starts, sched, True, 32, (6, 6, 3))
    n_used = _assert_same_routes(outs[-1], host, ("frame", inflate))
    print("inflate %d: %d paths with cells, %d segments, %d blocked, %d truncated" % (
        inflate, (host[2]["n_cells"] > 0).sum(), n_used, host[2]["n_blocked"].sum(), host[2]["truncated"].sum()))
    assert not all(torch.equal(a, b) for a, b in zip(outs[0][2:5], outs[-1][2:5]))
    want = S.shorten(cfg, lay, host[0], host[1], t_start=0.0, step_seconds=0.02, window=64, max_seg=32)
    _assert_same(host[2:5], want, ("frame against the restatement", inflate))
    S.check(cfg, lay, host[0], host[1], *host[2:5], t_start=0.0, step_seconds=0.02)
    assert host[2]["n_cells"].max() >= 2 and n_used >= 1
    m.close()


def test_shorten_state_errors(dsp):
    kw = dict(SMALL)
    (m,) = _twins(dsp, kw, 1)
    frames = _scene_frames(dsp, kw, 3, seed=31)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    steps, cells = np.full(4, 5, np.int32), np.tile(np.arange(6, dtype=np.int32), (4, 1))
    info, seg, end = np.zeros(4, S.INFO_DTYPE), np.zeros((4, 5, 8), F), np.zeros((4, 5), np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (steps, cells, info.view(np.int32).reshape(4, 4), seg, end)]

    def refused(h):
        for fn, arr in ((m.L.dspmap_shorten_paths, [p(a) for a in (steps, cells, info, seg, end)]),
                        (m.L.dspmap_shorten_paths_device, [a.data_ptr() for a in dev])):
            assert fn(h.h, 4, 6, arr[0], arr[1], -1.0, 0.0, 64, 5, 0, arr[2], arr[3], arr[4]) == E_STATE
        return h.L.dspmap_last_error(h.h)

    assert b"dspmap_build_cast_grid" in refused(m)                            # never built
    _run(m, frames[:2])
    assert b"dspmap_build_cast_grid" in refused(m)
    m.build_cast_grid(0.05, 0)
    assert m.shorten_paths(steps, cells)[0]["n_cells"].tolist() == [6] * 4
    m.build_reach_timeline(_sources(m.cfg, 20, 1, 3), 1, **TR.SPAN)            # a reach snapshot comes and goes: the call does not care
    assert m.shorten_paths(steps, cells)[0]["n_cells"].tolist() == [6] * 4
    pts, pos, quat, t = frames[2]
    assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1   # the next frame: the grid is stale
    assert b"dspmap_build_cast_grid" in refused(m)
    with pytest.raises(dsp.capi.DSPMapError):
        m.shorten_paths(steps, cells)
    torch.cuda.synchronize()
    assert not info.view(np.int32).any() and not seg.any() and not end.any() and not any(a.any() for a in dev[2:])
    slab = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    assert b"slab" in refused(slab)
    slab.close()
    m.close()


def test_shorten_is_read_only(dsp):
    kw = dict(SMALL)
    frames = _scene_frames(dsp, kw, 8, seed=77)
    a, b = _twins(dsp, kw)
    for x in (a, b):
        _run(x, frames[:6])
    thr = _median_threshold(a)
    for x in (a, b):
        x.build_cast_grid(thr, 1)
    cfg = a.cfg
    grid, ptr = a.cast_grid(), a.cast_grid_ptr()
    lay = R.unpack(grid, cfg.nx)
    steps, cells = _random_walks(cfg, lay, 64, 5)
    got, counts = _case(a, lay, steps, cells, "read-only", window=64, t_start=0.0, step_seconds=0.03)
    dev = a.shorten_paths(torch.from_numpy(steps).cuda(), torch.from_numpy(cells).cuda(), t_start=0.0, step_seconds=0.03)
    _assert_same(dev, got, "device twin of the host call")
    assert counts[0] > 64
    # the grid is the same words at the same address and still valid; the twin that never shortened has the same map
    assert a.cast_grid_ptr() == ptr and np.array_equal(a.cast_grid(), grid) and np.array_equal(b.cast_grid(), grid)
    assert np.array_equal(a.results(), b.results())
    # the next frames are bit-identical, one twin shortening behind every frame
    for pts, pos, quat, t in frames[6:]:
        for x in (a, b):
            assert x.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        a.build_cast_grid(thr, 1)
        a.shorten_paths(steps, cells, t_start=0.0, step_seconds=0.03)
    for x, y in zip(a.export_state(), b.export_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.results(), b.results())
    fa = a.getFutureStatus()
    assert np.array_equal(fa, b.getFutureStatus()) and (fa != 0).any()
    a.close(); b.close()
