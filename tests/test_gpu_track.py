"""GPU tests of the tracking extension (dspmap_track_update, its accessors and device buffers): exact parity -- zero differing integers in
the tracks (per field) and the counts -- with the numpy restatement (tests/track_ref.py), which is fed with what the device hands out: the
label grid and the records of every build (DSPMap.object_labels, DSPMap.objects) and the positions.  The shapes are those of
tests/test_gpu_frontier.py: 3 x 3 x 3 (one partial wave), 16 x 16 x 6 (one word), 66 x 12 x 8 (two words, a ragged last word) and
130 x 40 x 24 (the compaction's capacity spans many tiles).

Per step of track_ref.scene(shape): set_current_position -> build_cast_grid -> set_cast_grid(the step's occupancy) -> build_objects ->
update_tracks.  Mass and velocity come from the two handles of tests/test_gpu_objects.py: four accepted frames of the wall cloud, and a
handle seeded with moving particles.  The events of the scene are asserted on the restatement's output before anything is compared.  No
test provokes a fault: the full pair table is an ordinary, reported outcome of a capacity argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import objects_ref as OR
from tests import track_ref as R
from tests.test_gpu_frontier import BIG, CUBE, IDS, QUATS, RES, SHAPES, TINY, WALL_DIST, WIDE, _cloud, _device_copy, _frames, _map, _p

pytestmark = pytest.mark.gpu
F = np.float32
E_DEVICE, E_STATE = -2, -3
MAX_SHIFT = 2
DTS = {"frames": (0.0, 0.05), "moving": (0.4, 1.0, 2.5)}


def _moving(dsp, shape):
    """a handle whose voxels hold moving particles (tests/test_gpu_objects.py)"""
    m = _map(dsp, shape, seed=99)
    m.set_tables(*common.tables(5))
    m.seed_uniform(2, 0.01, 17, vmax=0.8)
    m.occupancy_resample()
    return m


def _handle(dsp, shape, kind):
    return _moving(dsp, shape) if kind == "moving" else _frames(dsp, shape)


def _objects(m, occ, pos, max_objects=4096):
    """the step's grid as layer 0 of the cast grid, labelled at the step's position; -> (records, label grid)"""
    m.set_current_position(*[float(v) for v in pos])
    m.build_cast_grid(0.5, 0)
    lay = np.zeros((m.T + 1,) + occ.shape, bool)
    lay[0] = occ
    m.set_cast_grid(OR.pack(lay))
    m.build_objects(t=-1.0, connectivity=26, min_cells=1, max_objects=max_objects)
    return m.objects(), m.object_labels()


def _same(got, want, tag):
    tr, counts = got
    wtr, wcounts, fault = want
    print(tag, "counts", counts)
    assert fault == 0 and counts == wcounts, (tag, counts, wcounts)
    assert tr.dtype == R.TRACK_DTYPE and tr.shape == wtr.shape, (tag, tr.shape, wtr.shape)
    for f in R.TRACK_DTYPE.names:
        bad = np.flatnonzero(tr[f] != wtr[f])
        assert bad.size == 0, (tag, f, bad.size, bad[:5], tr[bad[:5]], wtr[bad[:5]])


def _block_dt(T, e_max):
    """the dt at which the stored block's fastest axis is predicted to move e_max voxels (its velocity as the records give it)"""
    rec = T.prev[1][0]
    assert len(T.prev[1]) == 1 and rec["mass_q"] > 0
    v = np.abs(rec["mom_q"].astype(np.float64) / float(rec["mass_q"])).max()
    assert v > 0
    return float(e_max * float(F(RES)) / v)


def _sequence(m, shape, kind, per_cell=False, max_objects=4096, steps=None, check=True):
    """the scene through the handle and through the restatement; -> per step (tracks, counts, info, records, dt) of the DEVICE"""
    T = R.Tracker(shape, RES)
    sc = R.scene(shape)
    out = []
    for s, (occ, pos) in enumerate(sc[:steps]):
        rec, grid = _objects(m, occ, pos, max_objects)
        dt = DTS[kind][s % len(DTS[kind])]
        if kind == "moving" and s >= len(sc) - R.BLOCK_STEPS:          # the block is stored: a shift of one voxel, then one past the clamp
            dt = _block_dt(T, 1.0 if s == len(sc) - R.BLOCK_STEPS else 10.0)
        m.update_tracks(dt, 1, MAX_SHIFT, 0, per_cell)
        got = (m.tracks(), m.track_counts())
        want = T.update(grid, rec, pos, dt, 1, MAX_SHIFT)
        if check:
            _same(got, want, (shape, kind, s, dt))
        out.append((got[0], got[1], T.info, rec, dt))
    return out


@pytest.mark.parametrize("kind", ["frames", "moving"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tracks_match_the_restatement(dsp, shape, kind):
    """tracks and counts of every step; the device views equal the host copies; a small cap copies a prefix; track_states"""
    m = _handle(dsp, shape, kind)
    runs = _sequence(m, shape, kind)
    # the scene is not degenerate, on the restatement (its output equals the device's, compared above)
    if kind == "frames":
        ev = R.scene_events(shape, [r[:4] for r in runs])
        assert all(ev.values()), ev
    else:
        one, far = runs[-2], runs[-1]
        for (tr, counts, info, rec, dt), clamped in ((one, False), (far, True)):
            assert counts[:2] == (1, 1) and tr["prev_ordinal"][0] == 0, (dt, counts)             # the block is matched
            p, raw = info["p"][0], info["raw"][0]
            print(shape, "block dt", dt, "predicted", p, "before the clamp", raw, "overlap", tr["overlap"][0])
            if clamped:
                assert (np.abs(raw) > MAX_SHIFT).any() and np.abs(p).max() == MAX_SHIFT
            else:
                assert p.any() and (np.abs(raw) <= MAX_SHIFT).all() and (raw == p).all()
        assert any(r[2]["p"].any() for r in runs[:-2]) or shape == TINY                          # ... and the objects before it moved too
    # the device side of the last update
    tr, counts = m.tracks(), m.track_counts()
    k = len(tr)
    assert k == counts[0] > 0
    td = m.tracks(device="cuda")
    assert td.dtype == torch.int32 and tuple(td.shape) == (k, 18)
    assert np.array_equal(td.cpu().numpy(), tr.view(np.int32).reshape(k, 18))
    assert np.array_equal(td[:, :10].contiguous().view(torch.int64).cpu().numpy()[:, 0], tr["id"])
    L = m.L
    assert tuple(_device_copy(dsp, L.dspmap_track_counts_device(m.h), (7,), "<i8")) == counts + (0,)     # (the fault word is 0)
    assert np.array_equal(_device_copy(dsp, L.dspmap_tracks_device(m.h), (k, 18)), tr.view(np.int32).reshape(k, 18))
    # cap < k: a prefix, and still k  (a step with several tracks)
    rec, grid = _objects(m, *R.scene(shape)[8])
    m.update_tracks(0.0)
    tr = m.tracks()
    k = len(tr)
    assert k >= 2 and k == len(rec)
    cap, cnt = k // 2, C.c_int(-1)
    part = np.full(k + 1, -7, R.TRACK_DTYPE)
    assert L.dspmap_get_tracks(m.h, cap, _p(part), C.byref(cnt)) == 1 and cnt.value == k
    assert np.array_equal(part[:cap], tr[:cap]) and (part["age"][cap:] == -7).all()
    for a, b in zip(m.track_states(tr, rec, 0.25), R.states(tr, rec, RES, 0.25)):
        np.testing.assert_array_equal(a, b)
    m.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_per_cell_inserts_and_a_repeated_sequence_give_identical_bytes(dsp, shape):
    seen = []
    for per_cell in (False, True, False):
        m = _moving(dsp, shape)
        runs = _sequence(m, shape, "moving", per_cell=per_cell, check=not seen)
        seen.append([(r[0].tobytes(), r[1]) for r in runs])
        m.close()
    assert seen[0] == seen[1] == seen[2]
    assert sum(c[4] for _, c in seen[0]) > 0                                                       # pairs were counted


def test_tracks_live_through_a_frame(dsp):
    """one accepted frame between two updates: the objects go stale, the tracks stay readable, and the next update carries the ids over"""
    shape = CUBE
    m = _frames(dsp, shape)
    T = R.Tracker(shape, RES)
    occ, pos = R.scene(shape)[2]
    rec, grid = _objects(m, occ, pos)
    m.update_tracks(0.1)
    first = (m.tracks(), m.track_counts())
    _same(first, T.update(grid, rec, pos, 0.1), "before the frame")
    assert m.update(_cloud(WALL_DIST[shape]), tuple(float(v) for v in pos), 4 / 30.0, QUATS["identity"]) == 1
    assert not m.L.dspmap_objects_device(m.h) and m.L.dspmap_tracks_device(m.h)                    # stale / still there
    again = (m.tracks(), m.track_counts())
    assert first[0].tobytes() == again[0].tobytes() and first[1] == again[1]
    assert m.L.dspmap_track_update(m.h, 0.1, 1, 8, 0, 0) == E_STATE and b"dspmap_build_objects" in m.L.dspmap_last_error(m.h)
    rec, grid = _objects(m, occ, pos)
    m.update_tracks(0.1)
    got = (m.tracks(), m.track_counts())
    _same(got, T.update(grid, rec, pos, 0.1), "behind the frame")
    k = len(first[0])
    assert got[1][:4] == (k, k, 0, 0) and np.array_equal(got[0]["id"], first[0]["id"]) and (got[0]["age"] == first[0]["age"] + 1).all()
    # the staleness of the other layers does not know the tracker: builds around an update keep their snapshots
    m.build_distance_field(0.5, 8)
    m.update_tracks(0.1)
    assert m.L.dspmap_distance_field_device(m.h) and m.L.dspmap_cast_grid_device(m.h) and m.L.dspmap_objects_device(m.h)
    m.close()


def test_resets_restart_the_ids(dsp):
    shape = WIDE
    m = _frames(dsp, shape)
    sc = R.scene(shape)
    n, cnt = C.c_int(0), (C.c_longlong * 6)()

    def refused():
        assert m.L.dspmap_get_tracks(m.h, 0, None, C.byref(n)) == E_STATE and b"dspmap_track_update" in m.L.dspmap_last_error(m.h)
        assert m.L.dspmap_track_counts(m.h, cnt) == E_STATE and b"dspmap_track_update" in m.L.dspmap_last_error(m.h)
        assert not m.L.dspmap_tracks_device(m.h) and not m.L.dspmap_track_counts_device(m.h)
        return True
    assert refused()                                                                               # never updated
    for reset in (m.reset_tracks, m.clear_state, m.reset_tracks):
        T = R.Tracker(shape, RES)
        for s in (0, 1, 2):
            rec, grid = _objects(m, *sc[s])
            m.update_tracks(0.0)
            got = (m.tracks(), m.track_counts())
            _same(got, T.update(grid, rec, sc[s][1], 0.0), ("reset", s))
        assert got[1][5] >= got[1][0] > 0 and got[0]["age"].max() == 2 and got[0]["born_seq"].max() == 2 and got[0]["id"].min() == 0
        reset()
        assert refused()
    # a position the window refuses: a state error, nothing is enqueued, the tracker keeps what it has
    rec, grid = _objects(m, *sc[0])
    m.update_tracks(0.0)
    m.set_current_position(float("nan"), 0.0, 0.0)
    assert m.L.dspmap_track_update(m.h, 0.0, 1, 8, 0, 0) == E_STATE and b"current position" in m.L.dspmap_last_error(m.h)
    m.set_current_position(*[float(v) for v in sc[0][1]])
    m.update_tracks(0.0)
    k = len(rec)
    assert m.track_counts() == (k, k, 0, 0, k, k)
    m.close()


def test_ordinals_past_max_objects_take_no_part(dsp):
    shape, cap = WIDE, 3
    m = _moving(dsp, shape)
    T = R.Tracker(shape, RES)
    sc = R.scene(shape)
    for s in range(7):
        rec, grid = _objects(m, *sc[s], max_objects=cap)
        assert len(rec) == cap and grid.max() >= cap and m.object_counts()[0] > cap                # the grid holds ordinals without a record
        m.update_tracks(0.0, 1, 8, 0, s % 2 == 1)
        got = (m.tracks(), m.track_counts())
        _same(got, T.update(grid, rec, sc[s][1], 0.0), ("cap", s))
        assert got[1][0] == cap
        assert all(j < cap and o < cap for j, o in T.info["pairs"])
    # a larger max_objects behind a smaller one: the tracker's arrays grow with their contents
    rec, grid = _objects(m, *sc[7 - 1], max_objects=1 << 20)
    m.update_tracks(0.0)
    got = (m.tracks(), m.track_counts())
    _same(got, T.update(grid, rec, sc[6][1], 0.0), "grown")
    assert got[1][0] == len(rec) > cap and got[1][1] == cap                                        # the three stored tracks are found again
    m.close()


def test_a_full_pair_table_voids_the_update_and_is_reported(dsp):
    shape, max_pairs = CUBE, 2
    m = _frames(dsp, shape)
    T = R.Tracker(shape, RES)
    sc = R.scene(shape)
    rec, grid = _objects(m, *sc[0])
    m.update_tracks(0.0)
    _same((m.tracks(), m.track_counts()), T.update(grid, rec, sc[0][1], 0.0), "first")
    next_id = m.track_counts()[5]
    for per_cell in (False, True):
        rec, grid = _objects(m, *sc[1])
        m.update_tracks(0.0, 1, 8, max_pairs, per_cell)
        tr, counts, fault = T.update(grid, rec, sc[1][1], 0.0, slots=R.table_slots(max_pairs, 4096))
        assert len(T.info["pairs"]) > max_pairs == R.table_slots(max_pairs, 4096) and fault == 1   # the restatement counts more pairs than slots
        assert tuple(_device_copy(dsp, m.L.dspmap_track_counts_device(m.h), (7,), "<i8")) == counts + (1,) == (0, 0, 0, 0, 0, next_id, 1)
        n, cnt = C.c_int(-1), (C.c_longlong * 6)()
        assert m.L.dspmap_get_tracks(m.h, 0, None, C.byref(n)) == E_DEVICE and b"max_pairs" in m.L.dspmap_last_error(m.h)
        assert m.L.dspmap_track_counts(m.h, cnt) == E_DEVICE and b"max_pairs" in m.L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError, match="max_pairs"):
            m.tracks()
        # the next update starts fresh: everything born, nothing ended, the ids go on where they were
        rec, grid = _objects(m, *sc[1])
        m.update_tracks(0.0)
        got = (m.tracks(), m.track_counts())
        _same(got, T.update(grid, rec, sc[1][1], 0.0), ("after the void update", per_cell))
        k = len(rec)
        assert got[1] == (k, 0, k, 0, 0, next_id + k) and got[0]["id"].min() == next_id
        next_id += k
        # ... and one behind it associates again
        rec, grid = _objects(m, *sc[0])
        m.update_tracks(0.0, 1, 8, 1 << 30)                                                        # (capped at 2^24 slots)
        got = (m.tracks(), m.track_counts())
        _same(got, T.update(grid, rec, sc[0][1], 0.0), ("table of 2^24", per_cell))
        assert got[1][1] > 0 and got[1][5] == next_id
    m.close()
