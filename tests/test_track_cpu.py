"""CPU tests of the tracking extension (dspmap_track_update and its accessors): hand-worked answers of the numpy restatement
(tests/track_ref.py) on 3 x 3 x 3 and 8 x 4 x 2 grids -- match, split with parent, merge, both tie-breaks, the min_overlap threshold, shift
rounding at +-0.5 and the clamp, prev_sum under a window move, the fresh start, the full pair table --, the conditions of the scene the GPU
tests run, asserted on the restatement alone, and the real library without a device: symbols declared, exported and bound, the record's
layout."""
import os
import subprocess

import numpy as np
import pytest

from tests import objects_ref as OR
from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dspmap_track_update", "dspmap_track_reset", "dspmap_track_counts", "dspmap_get_tracks", "dspmap_tracks_device",
         "dspmap_track_counts_device"]
SHAPES = [(66, 12, 8), (16, 16, 6), (3, 3, 3), (130, 40, 24)]
IDS = ["66x12x8", "16x16x6", "3x3x3", "130x40x24"]
S8 = (8, 4, 2)
RES = 0.5                                          # (exact in binary: the hand-worked shifts are exact)


def _grid(shape, *objs):
    """label grid [nz, ny, nx]: object o holds the cells objs[o] = [(x, y, z)]"""
    nx, ny, nz = shape
    lab = np.full((nz, ny, nx), -1, np.int32)
    for o, cells in enumerate(objs):
        for x, y, z in cells:
            lab[z, y, x] = o
    return lab


def _row(x0, x1, y=0, z=0):
    return [(x, y, z) for x in range(x0, x1 + 1)]


def _pos(shape, k0=(0, 0, 0)):
    return R.position(k0, shape, RES, 0.25)


def _fields(tr, *names):
    return [tuple(int(t[n]) for n in names) for t in tr]


def test_a_cell_that_stays_is_matched_and_ages():
    shape = (3, 3, 3)
    lab = _grid(shape, [(1, 1, 1)])
    T = R.Tracker(shape, RES)
    tr, counts, fault = T.update(lab, R.records(lab), _pos(shape), 0.1)
    assert fault == 0 and counts == (1, 0, 1, 0, 0, 1)
    assert _fields(tr, "id", "parent", "age", "born_seq", "prev_ordinal", "overlap", "prev_count") == [(0, -1, 0, 0, -1, 0, 0)]
    for age in (1, 2):
        tr, counts, fault = T.update(lab, R.records(lab), _pos(shape), 0.1)
        assert counts == (1, 1, 0, 0, 1, 1)
        assert _fields(tr, "id", "parent", "age", "born_seq", "prev_ordinal", "overlap", "prev_count") == [(0, -1, age, 0, 0, 1, 1)]
        assert _fields(tr, "prev_sum_x", "prev_sum_y", "prev_sum_z", "shift_x", "shift_y", "shift_z") == [(1, 1, 1, 0, 0, 0)]


def test_split_names_its_parent_and_merge_ends_the_smaller():
    whole, left, right = _row(0, 5), _row(0, 1), _row(3, 5)
    T = R.Tracker(S8, RES)
    one, two = _grid(S8, whole), _grid(S8, left, right)
    T.update(one, R.records(one), _pos(S8), 0.0)
    # the split: n(0, left) = 2, n(0, right) = 3 -- the right part keeps the id, the left one is born of it
    tr, counts, _ = T.update(two, R.records(two), _pos(S8), 0.0)
    assert counts == (2, 1, 1, 0, 2, 2)
    assert _fields(tr, "id", "parent", "age", "born_seq", "prev_ordinal", "overlap") == [(1, 0, 0, 1, -1, 2), (0, -1, 1, 0, 0, 3)]
    assert _fields(tr, "prev_count", "prev_sum_x")[1] == (6, 15)
    # the merge: n(0, 0) = 2, n(1, 0) = 3 -- the merged object takes the id of the larger part (ordinal 1, id 0), track 1 ends
    tr, counts, _ = T.update(one, R.records(one), _pos(S8), 0.0)
    assert counts == (1, 1, 0, 1, 2, 2)
    assert _fields(tr, "id", "parent", "age", "born_seq", "prev_ordinal", "overlap", "prev_count", "prev_sum_x") == [(0, -1, 2, 0, 1, 3, 3, 12)]


def test_both_tie_breaks_go_to_the_smaller_index():
    whole, a, b = _row(0, 4), _row(0, 1), _row(3, 4)
    one, two = _grid(S8, whole), _grid(S8, a, b)
    T = R.Tracker(S8, RES)
    T.update(one, R.records(one), _pos(S8), 0.0)
    tr, counts, _ = T.update(two, R.records(two), _pos(S8), 0.0)          # bo(0): n = 2 twice, the smaller o is matched
    assert counts == (2, 1, 1, 0, 2, 2)
    assert _fields(tr, "id", "parent", "prev_ordinal", "overlap") == [(0, -1, 0, 2), (1, 0, -1, 2)]
    tr, counts, _ = T.update(one, R.records(one), _pos(S8), 0.0)          # bj(0): n = 2 twice, the smaller j gives its id
    assert counts == (1, 1, 0, 1, 2, 2)
    assert _fields(tr, "id", "parent", "prev_ordinal", "overlap", "age") == [(0, -1, 0, 2, 2)]
    # not mutual: o = 0 is best for both j, bj(0) = 0; j = 1 finds nobody else -- it ends, nothing is born
    assert T.info["pairs"] == {(0, 0): 2, (1, 0): 2}


def test_min_overlap_is_a_threshold_on_the_mutual_best():
    before, after = _grid(S8, _row(0, 2)), _grid(S8, _row(1, 4))
    for min_overlap, want in ((2, [(0, -1, 0, 2, 1)]), (3, [(1, 0, -1, 2, 0)])):
        T = R.Tracker(S8, RES)
        T.update(before, R.records(before), _pos(S8), 0.0)
        tr, counts, _ = T.update(after, R.records(after), _pos(S8), 0.0, min_overlap=min_overlap)
        assert _fields(tr, "id", "parent", "prev_ordinal", "overlap", "age") == want, min_overlap
        assert counts == ((1, 1, 0, 0, 1, 1) if min_overlap == 2 else (1, 0, 1, 1, 1, 2))


def test_shift_rounds_half_up_and_is_clamped_as_a_double():
    rec = np.zeros(4, OR.OBJECT_DTYPE)
    rec["mass_q"] = [100, 100, 0, -5]
    # v = mom / mass, e = v * dt / res with dt = 1, res = 0.5: 0.5 -> 1, -0.5 -> 0, 0.48 -> 0 | -0.52 -> -1, 1.5 -> 2, -1.5 -> -1
    rec["mom_q"] = [[25, -25, 24], [-26, 75, -75], [1000, 1000, 1000], [1000, 1000, 1000]]
    p, raw = R.predicted(rec, 1.0, RES, 8)
    assert p.tolist() == [[1, 0, 0], [-1, 2, -1], [0, 0, 0], [0, 0, 0]]          # (no mass, or a negative one: no shift)
    rec["mom_q"][0] = [100000, -100000, 425]                                     # e = 2000, -2000, 8.5
    p, raw = R.predicted(rec, 1.0, RES, 8)
    assert p[0].tolist() == [8, -8, 8] and raw[0].tolist() == [2000.0, -2000.0, 9.0]
    assert R.predicted(rec, 1.0, RES, 0)[0].tolist() == [[0, 0, 0]] * 4          # max_shift = 0: pure overlap
    assert R.predicted(rec, 0.0, RES, 8)[0].tolist() == [[0, 0, 0]] * 4          # dt = 0 as well
    # in an update: a cell that moved by two voxels in x is found with dt = 1 and lost with dt = 0
    before, after = _grid(S8, [(1, 1, 0)]), _grid(S8, [(3, 1, 0)])
    moving = R.records(before, mass_q=[100], mom_q=[[100, 12, -12]])            # e = (2, 0.24, -0.24)
    for dt, want in ((1.0, [(0, 0, 1, 2, 0, 0)]), (0.0, [(1, -1, 0, 0, 0, 0)])):
        T = R.Tracker(S8, RES)
        T.update(before, moving, _pos(S8), dt)
        tr, counts, _ = T.update(after, R.records(after), _pos(S8), dt)
        assert _fields(tr, "id", "prev_ordinal", "overlap", "shift_x", "shift_y", "shift_z") == want, dt


def test_prev_sums_follow_the_window():
    """the window moves by (+1, -1, 0): a box that stands in the world is found at (x - 1, y + 1, z), matched through the shift -dk0, and
    its previous sums arrive in the current window's indices"""
    before, after = _grid(S8, [(2, 1, 0), (3, 1, 0), (3, 1, 1)]), _grid(S8, [(1, 2, 0), (2, 2, 0), (2, 2, 1)])
    T = R.Tracker(S8, RES)
    T.update(before, R.records(before), _pos(S8, (4, -3, 7)), 0.3)
    tr, counts, _ = T.update(after, R.records(after), _pos(S8, (5, -4, 7)), 0.3)
    assert counts == (1, 1, 0, 0, 1, 1) and T.info["dk0"].tolist() == [1, -1, 0]
    assert _fields(tr, "shift_x", "shift_y", "shift_z", "overlap", "prev_count", "prev_sum_x", "prev_sum_y", "prev_sum_z") == [(-1, 1, 0, 3, 3, 5, 6, 1)]
    rec = R.records(after)
    assert (rec["sum_x"][0], rec["sum_y"][0], rec["sum_z"][0]) == (5, 6, 1)
    disp, vel = R.states(tr, rec, RES, 0.3)
    assert not disp.any() and not vel.any()                                       # it stood still


def test_a_move_of_a_whole_map_starts_fresh():
    lab = _grid(S8, _row(0, 2), _row(5, 6, 2, 1))
    T = R.Tracker(S8, RES)
    T.update(lab, R.records(lab), _pos(S8), 0.0)
    tr, counts, _ = T.update(lab, R.records(lab), _pos(S8, (7, 3, 1)), 0.0)       # |dk0| < n on every axis: associated (nothing overlaps)
    assert not T.info["fresh"] and counts[0] == 2
    for k0 in ((15, 3, 1), (7, -1, 1), (7, 3, 3)):                                # 8 along x, 4 along y, 2 along z: a whole map
        T = R.Tracker(S8, RES)
        T.update(lab, R.records(lab), _pos(S8, (7, 3, 1)), 0.0)
        tr, counts, _ = T.update(lab, R.records(lab), _pos(S8, k0), 0.0)
        assert T.info["fresh"] and counts == (2, 0, 2, 2, 0, 4), k0
        assert _fields(tr, "id", "parent", "age", "born_seq", "prev_ordinal", "overlap") == [(2, -1, 0, 1, -1, 0), (3, -1, 0, 1, -1, 0)]
    T.reset()
    tr, counts, _ = T.update(lab, R.records(lab), _pos(S8), 0.0)
    assert counts == (2, 0, 2, 0, 0, 2) and tr["id"].tolist() == [0, 1] and tr["born_seq"].tolist() == [0, 0]


def test_a_full_pair_table_voids_the_update():
    one, two = _grid(S8, _row(0, 5)), _grid(S8, _row(0, 1), _row(3, 5))
    T = R.Tracker(S8, RES)
    T.update(one, R.records(one), _pos(S8), 0.0)
    tr, counts, fault = T.update(two, R.records(two), _pos(S8), 0.0, slots=1)     # two pairs, one slot
    assert fault == 1 and len(tr) == 0 and counts == (0, 0, 0, 0, 0, 1)
    tr, counts, fault = T.update(two, R.records(two), _pos(S8), 0.0, slots=2)     # the stored state is gone: a fresh start, ids go on
    assert fault == 0 and counts == (2, 0, 2, 0, 0, 3) and tr["id"].tolist() == [1, 2] and tr["born_seq"].tolist() == [2, 2]
    assert [R.table_slots(v, 4096) for v in (0, 1, 2, 3, 1000, 1 << 30)] == [32768, 1, 2, 4, 1024, 1 << 24] and R.table_slots(0, 16) == 1024


def _run(shape):
    """the restatement over the scene, the objects from the restatement of dspmap_build_objects (no mass: no predicted shift)"""
    nx, ny, nz = shape
    T = R.Tracker(shape, 0.15)
    runs = []
    for occ, pos in R.scene(shape):
        rec, grid, _ = OR.objects(occ, np.zeros((nx * ny * nz, 4), np.float32), 26)
        tr, counts, fault = T.update(grid, rec, pos, 0.1)
        assert fault == 0
        runs.append((tr, counts, T.info, rec))
    return runs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_scene_contains_every_event(shape):
    runs = _run(shape)
    ev = R.scene_events(shape, runs)
    print(shape, [r[1] for r in runs])
    assert all(ev.values()), ev
    assert runs[0][1][2] == runs[0][1][0] > 0 and runs[-1][1][1] == runs[-1][1][0] > 0      # all born at first, all matched in place at last
    if shape[0] > 64:
        assert any((occ[:, :, 63] & occ[:, :, 64]).any() for occ, _ in R.scene(shape))
    ids = np.concatenate([r[0]["id"] for r in runs])
    assert ids.max() + 1 == runs[-1][1][5] and len(np.unique(ids)) == runs[-1][1][5]        # every id handed out once, none skipped


# ---- the library without a device
def test_track_symbols_declared_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert "%s(dspmap_t* m" % n in hdr, n
        assert "object" not in n
    assert sorted(n for n in dsp.capi.SIGNATURES if "track" in n) == sorted(NAMES)
    for meth in ("update_tracks", "tracks", "track_counts", "reset_tracks", "track_states"):
        assert callable(getattr(dsp.DSPMap, meth))
    assert "#define DSPMAP_TRACK_PER_CELL 1" in hdr and dsp.capi.TRACK_PER_CELL == 1
    assert '"dspmap_track.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()
    blob = open(dsp.capi.LIB_PATH, "rb").read()
    for k in (b"k_track_shift", b"k_track_pairs", b"k_track_best", b"k_track_sums", b"k_track_scan", b"k_track_emit", b"k_track_keep"):
        assert k in blob, k
    # the window's arithmetic is ONE function, shared with the known-space layer
    src = open(os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_layers.hip")).read()
    assert src.count("static int known_window(") == 1 and src.count("known_window(m, k0, o)") >= 2


def test_record_layout(dsp, tmp_path):
    """dspmap_track is 72 bytes, field for field what TRACK_DTYPE says, and the drop-in class forwards to the C ABI"""
    assert dsp.capi.TRACK_DTYPE == R.TRACK_DTYPE and dsp.capi.TRACK_DTYPE.itemsize == 72
    offs = " && ".join('offsetof(dspmap_track, %s) == %d' % (n, R.TRACK_DTYPE.fields[n][1]) for n in R.TRACK_DTYPE.names)
    src = tmp_path / "track.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <cstddef>\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    std::vector<dspmap_track> tracks(100);\n    int n = 0;\n"
                   "    int a = my_map.trackObjects(0.1f) + my_map.trackObjects(0.1f, 2, 4, 4096) + my_map.getTracks((int)tracks.size(), tracks.data(), n) + my_map.resetTracks();\n"
                   "    static_assert(sizeof(dspmap_track) == 72 && DSPMAP_TRACK_PER_CELL == 1, \"layout\");\n"
                   "    static_assert(%s, \"fields\");\n" % offs +
                   "    return a + n + (int)tracks[0].id + (int)tracks[0].parent + tracks[0].age + tracks[0].born_seq + tracks[0].overlap;\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_track_update(h_", "dspmap_get_tracks(h_", "dspmap_track_reset(h_"):
        assert call in hdr, call
    # ... and as a C program that prints it
    csrc = tmp_path / "size.c"
    csrc.write_text('#include <stdio.h>\n#include "dspmap.h"\nint main(void) { printf("%zu\\n", sizeof(dspmap_track)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(csrc), "-o", exe])
    assert subprocess.check_output([exe]).decode().strip() == "72"
