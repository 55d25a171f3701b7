"""numpy float32 restatement of the shortened paths (include/dspmap.h, dspmap_shorten_paths) on top of tests/cast_ref.cast: the greedy
farthest-visible rule, one vectorised cast call per round over all paths x candidates.  Independent of the kernel's structure: no waves,
no ballots, bool cells instead of words.  Plus a checker that runs on ANY output and knows nothing of the rule's order of evaluation: the
subsequence property, every unblocked segment FREE under a fresh cast, the speed bound and the padding rule."""
import numpy as np

from tests import cast_ref as CR
from tests import query_ref as Q

F = np.float32
INFO_DTYPE = np.dtype([("n_cells", "i4"), ("n_segments", "i4"), ("n_blocked", "i4"), ("truncated", "i4")])
MAX_WINDOW = 64


def path_lengths(cfg, steps, cells):
    """m [n]: 0 where steps < 0, else the number of leading entries of the row that lie in [0, V)"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    cells = np.asarray(cells, np.int64)
    ok = (cells >= 0) & (cells < n[0] * n[1] * n[2])
    m = np.where(ok.all(1), cells.shape[1], (~ok).argmax(1))
    return np.where(np.asarray(steps) < 0, 0, m).astype(np.int64)


def vertices(cfg, steps, cells, pos, t_start, step_seconds):
    """float32 [..., 4]: {voxel centre, time} of the cells at positions pos [k] of the paths rows [k] (steps [k], cells [k, max_len])"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    c = np.asarray(cells, np.int64)[np.arange(len(pos)), pos]
    x, y, z = c % n[0], (c // n[0]) % n[1], c // (n[0] * n[1])
    out = np.zeros((len(pos), 4), F)
    for a, i in enumerate((x, y, z)):
        out[:, a] = ((i.astype(F) * res).astype(F) + corr[a]).astype(F)          # dspmap_voxel_center: fl(fl(i * res) + (-half + res / 2))
    if t_start < 0 or T == 0:
        out[:, 3] = F(-1.0)
    else:
        e = np.maximum(np.asarray(steps, np.int64) - pos, 0)
        out[:, 3] = (F(t_start) + (e.astype(F) * F(step_seconds)).astype(F)).astype(F)
    return out


def shorten(cfg, lay, steps, cells, t_start=-1.0, step_seconds=0.0, window=MAX_WINDOW, max_seg=None):
    """(info INFO_DTYPE [n], seg float32 [n, max_seg, 8], end int32 [n, max_seg]) of the paths (steps [n], cells [n, max_len])"""
    steps = np.asarray(steps, np.int32).reshape(-1)
    cells = np.asarray(cells, np.int32).reshape(len(steps), -1)
    n, max_len = cells.shape
    assert 1 <= window <= MAX_WINDOW
    max_seg = max(max_len - 1, 0) if max_seg is None else int(max_seg)
    m = path_lengths(cfg, steps, cells)
    info = np.zeros(n, INFO_DTYPE)
    info["n_cells"] = m
    seg = np.zeros((n, max_seg, 8), F)
    end = np.full((n, max_seg), -1, np.int32)
    p = np.zeros(n, np.int64)
    s = np.zeros(n, np.int64)
    while True:
        going = p < m - 1
        cut = going & (s == max_seg)
        info["truncated"][cut] = 1
        act = np.flatnonzero(going & ~cut)
        if not act.size:
            break
        k = p[act, None] + 1 + np.arange(window)[None, :]                     # the candidates of every active path
        valid = k <= (m[act, None] - 1)
        row, col = np.nonzero(valid)
        rows = act[row]
        A = vertices(cfg, steps[rows], cells[rows], p[rows], t_start, step_seconds)
        B = vertices(cfg, steps[rows], cells[rows], k[row, col], t_start, step_seconds)
        hit = CR.cast(cfg, lay, np.concatenate([A, B], 1))
        free = np.zeros(valid.shape, bool)
        free[row, col] = hit["status"] == CR.FREE
        any_free = free.any(1)
        far = window - 1 - free[:, ::-1].argmax(1)                            # the largest free candidate
        q = np.where(any_free, p[act] + 1 + far, p[act] + 1)
        info["n_blocked"][act] += ~any_free
        seg[act, s[act], 0:4] = vertices(cfg, steps[act], cells[act], p[act], t_start, step_seconds)
        seg[act, s[act], 4:8] = vertices(cfg, steps[act], cells[act], q, t_start, step_seconds)
        end[act, s[act]] = q
        p[act] = q
        s[act] += 1
    info["n_segments"] = s
    return info, seg, end


def check(cfg, lay, steps, cells, info, seg, end, t_start=-1.0, step_seconds=0.0, window=MAX_WINDOW):
    """holds ANY output against the contract's consequences; returns (segments, blocked segments, truncated paths, longest segment in
    path positions)"""
    T, pred, res, nn, half, corr = Q._dims(cfg)
    steps = np.asarray(steps, np.int32).reshape(-1)
    cells = np.asarray(cells, np.int32).reshape(len(steps), -1)
    n, max_len = cells.shape
    info = np.asarray(info)
    if info.dtype != INFO_DTYPE:
        info = np.ascontiguousarray(info, np.int32).reshape(n, 4).view(INFO_DTYPE).reshape(n)
    seg = np.ascontiguousarray(seg, F)
    end = np.asarray(end, np.int32)
    assert seg.shape[:1] == (n,) and seg.shape[2:] == (8,) and end.shape == seg.shape[:2]
    max_seg = end.shape[1]
    m = path_lengths(cfg, steps, cells)
    assert np.array_equal(info["n_cells"], m)
    ns = info["n_segments"].astype(np.int64)
    assert (ns >= 0).all() and (ns <= max_seg).all() and (ns <= np.maximum(m - 1, 0)).all()
    used = np.arange(max_seg)[None, :] < ns[:, None]
    # padding: all-zero bits and -1 behind n_segments (a path with m <= 1 has no segment at all)
    assert not seg.view(np.uint32)[~used].any() and (end[~used] == -1).all()
    row, col = np.nonzero(used)
    e1 = end[row, col].astype(np.int64)
    e0 = np.where(col > 0, end[row, np.maximum(col - 1, 0)], 0).astype(np.int64)
    # the subsequence property: strictly ascending positions within the window, vertex for vertex the path's cells at those positions
    assert (e1 > e0).all() and (e1 - e0 <= window).all() and (e1 <= m[row] - 1).all()
    A = vertices(cfg, steps[row], cells[row], e0, t_start, step_seconds)
    B = vertices(cfg, steps[row], cells[row], e1, t_start, step_seconds)
    want = np.concatenate([A, B], 1)
    assert np.array_equal(seg[row, col].view(np.uint32), want.view(np.uint32))
    # the last vertex is the path's last cell unless the path is truncated; truncated means max_seg segments did not get there
    last = np.zeros(n, np.int64)
    last[ns > 0] = end[ns > 0, ns[ns > 0] - 1]
    short = (m > 1) & (last < m - 1)
    assert np.array_equal(info["truncated"] != 0, short) and (ns[short] == max_seg).all() and set(np.unique(info["truncated"])) <= {0, 1}
    # re-casting: every segment is FREE except n_blocked of them, and those advance by one cell
    status = CR.cast(cfg, lay, want)["status"]
    blocked = status != CR.FREE
    assert (e1[blocked] - e0[blocked] == 1).all()
    assert np.array_equal(np.bincount(row[blocked], minlength=n), info["n_blocked"])
    # the speed bound, where consecutive cells are equal or face neighbours: a segment is at most as many voxels long, in the sum over the
    # axes, as positions -- and steps, while the steps are not clamped at 0 -- lie between its ends
    c = cells.astype(np.int64)
    xyz = np.stack([c % nn[0], (c // nn[0]) % nn[1], c // (nn[0] * nn[1])], -1)
    hop = np.abs(np.diff(xyz, axis=1)).sum(-1)
    inpath = np.arange(1, max_len)[None, :] < m[:, None]
    walk = ~((hop > 1) & inpath).any(1)
    w = walk[row]
    man = np.abs(xyz[row, e1] - xyz[row, e0]).sum(-1)
    assert (man[w] <= (e1 - e0)[w]).all()
    timed = w & (steps[row] >= e1)
    assert (man[timed] <= np.abs((steps[row] - e0) - (steps[row] - e1))[timed]).all()
    return int(used.sum()), int(blocked.sum()), int(short.sum()), int((e1 - e0).max()) if len(e1) else 0


def info_of(raw):
    """INFO_DTYPE [n] of the int32 [n, 4] a device call returns"""
    return np.ascontiguousarray(raw, np.int32).reshape(-1, 4).view(INFO_DTYPE).reshape(-1)
