"""Every planning layer puts the same point in the same cell.

The cell of a sample -- finite test, optional subtraction of the sensor position, |p| >= half, trunc((p + half) / res), < n -- is one device
function (dspmap_grid.h) behind the arrival fields and their paths, the timeline's paths, the cost fields and their paths, the segment casts
and the free boxes.  One batch of points on and around every edge of that rule goes through all of them, in the map frame and in the world
frame, and each must agree exactly with tests/reach_ref.point_cells."""
import numpy as np
import pytest

from tests import reach_ref as R
from tests.query_ref import _dims
from tests.test_gpu_reach import _blank_map

pytestmark = pytest.mark.gpu
F = np.float32
N_FIELDS = 2
MAPS = {"65x6x3": dict(nx=65, ny=6, nz=3, res=0.15, ppv=4), "8x8x1": dict(nx=8, ny=8, nz=1, res=0.15, ppv=4)}


def _batch(cfg):
    """about forty points {x, y, z, field} in the map frame"""
    _, _, res, n, half, corr = _dims(cfg)
    centre = lambda a, k: F(F(F(k) * res) + corr[a])   # noqa: E731  dspmap_voxel_center
    mid = [centre(a, n[a] // 2) for a in range(3)]
    rows = []

    def add(a, v, field=None):
        """the middle cell's centre with coordinate a replaced by v"""
        p = list(mid)
        p[a] = F(v)
        rows.append((p[0], p[1], p[2], len(rows) % N_FIELDS if field is None else field))

    for k in ((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1), (1, n[1] // 2, 0)):                 # centres of cells
        rows.append((centre(0, k[0]), centre(1, k[1]), centre(2, k[2]), len(rows) % N_FIELDS))
    for a in range(3):
        for s in (F(1), F(-1)):
            add(a, s * half[a])                                                              # +-half exactly: outside
            add(a, np.nextafter(s * half[a], F(0)))                                          # the last float inside it
        for k in (1, n[a] - 1):                                                              # a quotient that lands on a cell face ...
            face = F(F(F(k) * res) - half[a])
            add(a, face)
            add(a, np.nextafter(face, F(-np.inf), dtype=F))                                  # ... and the float below it
    for k in (min(63, n[0] - 1), min(64, n[0] - 1)):                                         # the last bit of a word, the first of the next
        add(0, centre(0, k))
    for a, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (1, np.nan)):                       # not finite
        add(a, v)
    add(0, mid[0], field=-1)                                                                 # fields outside [0, N_FIELDS)
    add(0, mid[0], field=N_FIELDS)
    return R.points(rows)


def _shifted(pts, cur):
    out = pts.copy()
    for a, name in enumerate("xyz"):
        out[name] = (pts[name] + cur[a]).astype(F)
    return out


@pytest.mark.parametrize("shape", sorted(MAPS))
def test_every_layer_puts_a_point_in_the_same_cell(dsp, shape):
    m = _blank_map(dsp, dict(MAPS[shape]))
    cfg = m.cfg
    n = (cfg.nx, cfg.ny, cfg.nz)
    m.set_cast_grid(np.zeros((m.T + 1, cfg.nz, cfg.ny, (cfg.nx + 63) // 64), np.uint64))
    base = _batch(cfg)
    assert 35 <= len(base) <= 50
    max_steps = sum(n)                                                                       # every cell of a blank map is reached
    # the world-frame pass hands fl(p + cur) in and the kernels form fl(that - cur).  The sensor position is made of small powers of two, so
    # that these two roundings lose at most the last bit and the points stay ON the edges they were made for ("+-half exactly", "on a
    # face"); another position would push them off.  The reference does the same arithmetic, so the expectation holds either way
    for world, cur in ((False, np.zeros(3, F)), (True, np.array([0.5, -0.25, 0.125], F))):
        if world:
            m.set_current_position(*[float(v) for v in cur])
        pts = _shifted(base, cur) if world else base
        tag = (shape, world)
        finite, inside, ijk = R.point_cells(cfg, pts, world, cur)
        ijk = np.where(inside[:, None], ijk, 0)
        field_ok = (pts["field"] >= 0) & (pts["field"] < N_FIELDS)
        # not vacuous: cells, points outside (by |p| >= half and by the quotient), non-finite ones and wrong fields all occur
        assert inside.sum() >= 10 and (finite & ~inside).sum() >= 6 and (~finite).sum() == 4 and (~field_ok).sum() == 2, tag
        g = (ijk[:, 2] * cfg.ny + ijk[:, 1]) * cfg.nx + ijk[:, 0]
        zero = np.zeros((N_FIELDS, cfg.nz, cfg.ny, cfg.nx), bool)                            # the cells of the sources, per field
        ok = inside & field_ok
        zero[pts["field"][ok], ijk[ok, 2], ijk[ok, 1], ijk[ok, 0]] = True
        status = np.where(~finite | ~field_ok, -3, np.where(inside, 0, -2))                  # 0: the field's value at the cell

        def check_paths(got, field, what):
            steps, cells = got
            want = np.where(status == 0, field[np.clip(pts["field"], 0, N_FIELDS - 1), ijk[:, 2], ijk[:, 1], ijk[:, 0]].astype(np.int64), status)
            assert np.array_equal(steps, want), (tag, what, steps.tolist(), want.tolist())
            assert (want[status == 0] >= 0).all() and (want[status == 0] != 65535).all(), (tag, what)
            assert np.array_equal(cells[:, 0], np.where(status == 0, g, -1)), (tag, what, cells[:, 0].tolist())

        m.build_reach_fields(pts, N_FIELDS, max_steps=max_steps, world=world)
        reach = m.reach_field(None, N_FIELDS)
        assert np.array_equal(reach == 0, zero), (tag, "reach fields")
        check_paths(m.reach_paths(pts, 1, world=world), reach, "reach paths")

        m.build_reach_timeline(pts, N_FIELDS, max_steps=max_steps, world=world)
        timeline = m.reach_field(None, N_FIELDS)
        assert np.array_equal(timeline, reach), (tag, "timeline fields")
        check_paths(m.reach_timeline_paths(pts, 1, world=world), timeline, "timeline paths")

        m.build_cost_fields(pts, N_FIELDS, t=-1.0, bands=(), world=world)
        cost = m.cost_field(None, N_FIELDS)
        assert np.array_equal(cost == 0, zero), (tag, "cost fields")
        check_paths(m.cost_paths(pts, 1, world=world), cost, "cost paths")

        seg = np.zeros((len(pts), 8), F)                                                     # a == b, the current layer
        for a, name in enumerate("xyz"):
            seg[:, a] = seg[:, 4 + a] = pts[name]
        seg[:, 3] = seg[:, 7] = -1.0
        hit = m.cast_segments(seg, world=world)
        want = np.where(~finite, dsp.capi.CAST_INVALID, np.where(inside, dsp.capi.CAST_FREE, dsp.capi.CAST_START_OUTSIDE))
        assert np.array_equal(hit["status"], want), (tag, "cast", hit["status"].tolist(), want.tolist())

        box = m.grow_boxes(seg, (0, 0, 0), world=world)
        want = np.where(~finite, dsp.capi.BOX_INVALID, np.where(inside, dsp.capi.BOX_OK, dsp.capi.BOX_SEED_OUTSIDE))
        assert np.array_equal(box["status"], want), (tag, "boxes", box["status"].tolist(), want.tolist())
        assert np.array_equal(box["lo"][inside], ijk[inside]) and np.array_equal(box["hi"][inside], ijk[inside]), (tag, "boxes")
