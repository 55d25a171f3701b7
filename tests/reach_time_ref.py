"""numpy restatement of the space-time paths traced backwards through the sets a timeline build keeps (include/dspmap.h,
dspmap_build_reach_timeline and dspmap_reach_timeline_paths), on top of tests/reach_ref.py: the sets are the bool arrays that
reach_ref.fields(..., return_sets=True) returns, one per executed step, and a step behind the early exit repeats the last of them.  Plus a
checker of a result that knows nothing of sets: it holds a path against the blocked cells of the step each of its cells is occupied at."""
import numpy as np

from tests import query_ref as Q
from tests import reach_ref as R


def set_at(sets, step):
    """R_step [n_fields, nz, ny, nx]: the list ends at the early exit, behind which every step repeats its last entry"""
    return sets[min(step, len(sets) - 1)]


def timeline_paths(cfg, val, sets, starts, max_len, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(steps int32 [n], cells int32 [n, max_len]): from each start's cell at its first arrival v backwards, the cell at step s - 1 is
    the cell of step s if R_{s-1} holds it (a wait), else its first face neighbour in the order -x, +x, -y, +y, -z, +z that R_{s-1} holds"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    nx, ny, nz = n
    starts = np.asarray(starts, R.POINT_DTYPE).reshape(-1)
    steps = np.full(len(starts), -3, np.int32)
    cells = np.full((len(starts), max_len), -1, np.int32)
    if not len(starts):
        return steps, cells
    finite, inside, ijk = R.point_cells(cfg, starts, world, cur_pos)
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            continue                                              # -3
        if not inside[i]:
            steps[i] = -2
            continue
        x, y, z = (int(v) for v in ijk[i])
        v = int(val[f, z, y, x])
        if v == R.UNREACHED:
            steps[i] = -1
            continue
        steps[i] = v
        for j in range(max_len):
            cells[i, j] = (z * ny + y) * nx + x
            if v == 0:
                break
            P = set_at(sets, v - 1)[f]
            for dx, dy, dz in ((0, 0, 0),) + R.NEIGHBOURS:
                a, b, c = x + dx, y + dy, z + dz
                if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and P[c, b, a]:
                    x, y, z = a, b, c
                    break
            else:
                break                                             # neither the cell nor a neighbour: the path stops, the rest stays -1
            v -= 1
    return steps, cells


def check_timeline_paths(cfg, lay, src, n_fields, starts, steps, cells, t_start=-1.0, step_seconds=0.0, max_steps=R.MAX_STEPS, world=False,
                         with_current=False, cur_pos=(0.0, 0.0, 0.0), val=None):
    """steps is the field's value (reach_ref.fields, computed here unless given), cells[0] the start's cell, consecutive cells equal or
    face neighbours, the cell at step s free in what step s tests, a complete path ends in a free source cell of its field, and the
    entries behind the end are -1.  Returns (complete paths, paths with at least one wait)."""
    T, pred, res, n, half, corr = Q._dims(cfg)
    nx, ny, nz = n
    lay = np.asarray(lay, bool)
    starts = np.asarray(starts, R.POINT_DTYPE).reshape(-1)
    steps, cells = np.asarray(steps), np.asarray(cells)
    assert steps.shape == (len(starts),) and cells.ndim == 2 and cells.shape[0] == len(starts)
    max_len = cells.shape[1]
    layers = R.schedule(cfg, t_start, step_seconds, max_steps)
    if val is None:
        val = R.fields(cfg, lay, src, n_fields, t_start, step_seconds, max_steps, world, with_current, cur_pos)
    assert val.shape[0] == n_fields
    S0 = R.source_sets(cfg, src, n_fields, world, cur_pos) & ~R.blocked_at(lay, layers, 0, with_current)[None]
    finite, inside, ijk = R.point_cells(cfg, starts, world, cur_pos)
    done = waits = 0
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            assert steps[i] == -3 and (cells[i] == -1).all(), i
            continue
        if not inside[i]:
            assert steps[i] == -2 and (cells[i] == -1).all(), i
            continue
        g0 = (int(ijk[i, 2]) * ny + int(ijk[i, 1])) * nx + int(ijk[i, 0])
        v0 = int(val[f].reshape(-1)[g0])
        if v0 == R.UNREACHED:
            assert steps[i] == -1 and (cells[i] == -1).all(), i
            continue
        assert steps[i] == v0, (i, steps[i], v0)
        length = min(v0 + 1, max_len)
        row = cells[i]
        assert (row[:length] >= 0).all() and (row[:length] < nx * ny * nz).all() and (row[length:] == -1).all(), (i, v0, row[:8])
        if length == 0:
            continue
        assert row[0] == g0, i
        x, y, z = row[:length] % nx, (row[:length] // nx) % ny, row[:length] // (nx * ny)
        hop = np.abs(np.diff(x)) + np.abs(np.diff(y)) + np.abs(np.diff(z))
        assert (hop <= 1).all(), ("a jump", i, hop.max())
        for j in range(length):                                   # the cell at step v0 - j is free in what that step tests
            assert not R.blocked_at(lay, layers, v0 - j, with_current)[z[j], y[j], x[j]], ("a blocked cell", i, j, v0 - j)
        if length == v0 + 1:
            assert S0[f, z[-1], y[-1], x[-1]], ("the path does not end in a free source cell of its field", i)
            done += 1
        waits += int((hop == 0).any())
    return done, waits


# ---- the scenes the CPU and the GPU tests share (40 x 40 x 24 at 0.15 m, six horizons 0.05 .. 2.0 s: L = 7 layers).  Each returns
# (lay bool [L, nz, ny, nx], src, n_fields, starts, schedule)
SCENE_CFG = dict(nx=40, ny=40, nz=24, res=0.15)
STATIC = dict(t_start=-1.0, step_seconds=0.0, max_steps=200)      # (the schedules of tests/test_gpu_reach.py)
FROZEN = dict(t_start=0.3, step_seconds=0.0, max_steps=200)
DOOR = dict(t_start=0.0, step_seconds=0.019, max_steps=150)       # layer 3 (horizon 2) from step 11 on: t_10 = 0.19, t_11 = 0.209 > 0.2
SPAN = dict(t_start=0.0, step_seconds=0.02, max_steps=120)        # every horizon in turn
CLUTTER_SEED = 11


def centre(cfg, x, y, z):
    res = cfg.voxel_resolution
    return (-0.5 * res * cfg.nx + res * (x + 0.5), -0.5 * res * cfg.ny + res * (y + 0.5), -0.5 * res * cfg.nz + res * (z + 0.5))


def at(cfg, *cells):
    """points at the centres of cells (x, y, z[, field])"""
    return R.points([centre(cfg, *c[:3]) + ((c[3] if len(c) > 3 else 0),) for c in cells])


def random_starts(cfg, n, n_fields, rng, reach=1.02):
    """n starts with coordinates up to reach x half (some outside) and `field` in -1 .. n_fields (both ends invalid)"""
    half = 0.5 * cfg.voxel_resolution * np.array([cfg.nx, cfg.ny, cfg.nz])
    p = rng.uniform(-reach, reach, (n, 3)) * half
    out = np.zeros(n, R.POINT_DTYPE)
    out["x"], out["y"], out["z"] = p[:, 0], p[:, 1], p[:, 2]
    out["field"] = rng.integers(-1, n_fields + 1, n)
    return out


def opening_door_scene(cfg):
    """a wall at x = 20 in every layer whose cell (20, 10, 5) is free from layer 3 on; the front from (15, 10, 5) waits before it"""
    L = cfg.prediction_times + 1
    lay = np.zeros((L, cfg.nz, cfg.ny, cfg.nx), bool)
    lay[:, :, :, 20] = True
    lay[3:, 5, 10, 20] = False
    starts = at(cfg, (25, 10, 5), (20, 10, 5), (15, 10, 5), (19, 10, 5), (39, 39, 23))
    return lay, at(cfg, (15, 10, 5)), 1, starts, dict(DOOR)


def invariant_scene(cfg, seed=2):
    """30 % random clutter, the same in all layers; two fields; 300 random starts (for the schedules STATIC and FROZEN)"""
    rng = np.random.default_rng(seed)
    L = cfg.prediction_times + 1
    one = rng.random((cfg.nz, cfg.ny, cfg.nx)) < 0.3
    lay = np.repeat(one[None], L, 0)
    free = np.argwhere(~one)
    pick = free[rng.integers(0, len(free), 4)]
    src = at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k % 2) for k, c in enumerate(pick)])
    starts = random_starts(cfg, 300, 2, rng)
    starts["field"] = rng.integers(0, 2, len(starts))
    return lay, src, 2, starts, None


def changing_clutter_scene(cfg, seed=CLUTTER_SEED):
    """60 random boxes of 2 .. 8 cells an edge per layer, drawn anew for every layer; four fields, each from a cell free in all layers;
    400 starts with `field` in -1 .. 4 and coordinates up to 1.02 x half"""
    rng = np.random.default_rng(seed)
    L = cfg.prediction_times + 1
    lay = np.zeros((L, cfg.nz, cfg.ny, cfg.nx), bool)
    for l in range(L):
        for _ in range(60):
            s = rng.integers(2, 9, 3)
            o = [int(rng.integers(0, m - e + 1)) for m, e in zip((cfg.nx, cfg.ny, cfg.nz), s)]
            lay[l, o[2]:o[2] + s[2], o[1]:o[1] + s[1], o[0]:o[0] + s[0]] = True
    free = np.argwhere(~lay.any(0))
    assert len(free) >= 4
    pick = free[rng.choice(len(free), 4, replace=False)]
    src = at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k) for k, c in enumerate(pick)])
    return lay, src, 4, random_starts(cfg, 400, 4, rng), dict(SPAN)
