"""CPU tests of the objects extension (dspmap_build_objects): the numpy restatement (tests/objects_ref.py) against scipy.ndimage.label and
against a plain flood fill, the conditions that make its scenes worth comparing, and the labelling core itself -- the find / unite of
dsp-map_amd/csrc/dspmap_unionfind.h that the kernels call -- run on the host by a stand-alone program (tests/objects_uf_check.cpp),
sequentially in shuffled orders and from 8 threads, under AddressSanitizer + UndefinedBehaviorSanitizer and, where the toolchain has its
runtime, under ThreadSanitizer.  No device, and no sanitizer near Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import objects_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE, CUBE, TINY, BIG = (66, 12, 8), (16, 16, 6), (3, 3, 3), (130, 40, 24)
SHAPES = [WIDE, CUBE, TINY, BIG]
IDS = ["66x12x8", "16x16x6", "3x3x3", "130x40x24"]
# (components, largest, singles, components with >= 4 cells) of scene(shape) per connectivity, recorded from scipy.ndimage.label when the
# scene was defined: a change of the scene or of the restatement shows here
TABLE = {(BIG, 6): (10163, 2620, 6570, 1282), (BIG, 26): (328, 19997, 227, 21), (WIDE, 6): (441, 402, 275, 55), (WIDE, 26): (33, 402, 18, 12),
         (CUBE, 6): (94, 136, 56, 12), (CUBE, 26): (11, 174, 4, 3), (TINY, 6): (2, 7, 0, 2), (TINY, 26): (2, 7, 0, 2)}
CROSSING = {BIG: 46, WIDE: 8}   # columns (y, z) set at both x = 63 and x = 64

_LAB = {}


def lab_of(shape, conn, seed=11):
    """components of scene(shape, seed), computed once"""
    key = (shape, conn, seed)
    if key not in _LAB:
        _LAB[key] = R.components(R.scene(shape, seed), conn)
        _LAB[key].setflags(write=False)
    return _LAB[key]


def _same_partition(lab, other):
    """`other` (any labels > 0 on set cells, scipy's) splits the set cells exactly as lab does, whose label is the component's minimum index"""
    on = lab >= 0
    assert np.array_equal(on, other > 0)
    pairs = np.unique(np.stack([lab[on], other[on]], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))   # a bijection between the two label sets
    idx = np.arange(lab.size).reshape(lab.shape)
    for o in np.unique(other[on])[:2000]:
        assert lab[other == o][0] == idx[other == o].min()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("conn", [6, 26])
def test_restatement_against_scipy(shape, conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = R.scene(shape)
    other, n = ndimage.label(occ, ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    lab = lab_of(shape, conn)
    assert n == R.summary(lab)[0]
    _same_partition(lab, other)


@pytest.mark.parametrize("shape", [TINY, CUBE], ids=["3x3x3", "16x16x6"])
@pytest.mark.parametrize("conn", [6, 26])
def test_restatement_against_flood_fill(shape, conn):
    for seed in (11, 13, 17):
        assert np.array_equal(lab_of(shape, conn, seed), R.flood(R.scene(shape, seed), conn)), seed


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scenes_are_not_degenerate(shape):
    """the figures recorded for scene(shape), and what the GPU parity test relies on: several components, singles that
    min_cells = 4 filters, partitions that differ between the connectivities, a component across the word edge x = 63 | 64"""
    nx = shape[0]
    occ = R.scene(shape)
    l6, l26 = lab_of(shape, 6), lab_of(shape, 26)
    assert R.summary(l6) == TABLE[shape, 6] and R.summary(l26) == TABLE[shape, 26]
    assert not occ[1].any() and occ[0, 0].all() and l6[0, shape[1] - 1 - (shape[1] - 1) % 2, 0] == 0   # the serpentine is ONE component: label 0 reaches its last row
    for seed in (11, 13, 17):                      # the layers t = -1, 0.1 and 5.0 select in the GPU test
        assert R.summary(lab_of(shape, 6, seed))[0] >= 2 and R.summary(lab_of(shape, 26, seed))[0] >= 2
    if shape != TINY:
        for seed in (11, 13, 17):
            s6, s26 = R.summary(lab_of(shape, 6, seed)), R.summary(lab_of(shape, 26, seed))
            assert s6[2] > 0 and s26[2] > 0 and 0 < s6[3] < s6[0] and 0 < s26[3] < s26[0]   # singles present, and filtered at min_cells = 4
            assert s6[0] > s26[0]                   # the partitions differ
    if nx > 64:
        both = occ[:, :, 63] & occ[:, :, 64]
        assert int(both.sum()) == CROSSING[shape]
        assert (l6[:, :, 63][both] == l6[:, :, 64][both]).all()   # a component crosses the word edge


def test_records_label_grid_and_counts_of_a_hand_made_layer():
    """two bars and a single cell in 5 x 3 x 2: every field of the records by hand"""
    occ = np.zeros((2, 3, 5), bool)
    occ[0, 0, 1:4] = True          # a bar along x: voxels 1, 2, 3
    occ[1, 2, 0] = True            # a single: voxel 25
    occ[0, 1, 4] = True            # touches the bar's end (3) by an edge only: voxel 9
    res = np.zeros((30, 4), np.float32)
    res[:, 0] = 0.5
    res[:, 1] = -2.0
    res[2] = (4096.0, 1.0, np.nan, np.inf)      # mass out of range: the cell adds nothing at all
    res[3] = (3.0, 2000.0, 0.25, np.inf)        # |w * u_x| >= 4096 and u_z not finite: only mass and y momentum
    rec, grid, counts = R.objects(occ, res, 6)
    assert counts == (3, 3, 5) and list(rec["label"]) == [1, 9, 25] and list(rec["count"]) == [3, 1, 1]
    assert list(grid.ravel()[[1, 2, 3, 9, 25]]) == [0, 0, 0, 1, 2] and (grid.ravel() >= 0).sum() == 5
    bar = rec[0]
    assert (bar["min_x"], bar["max_x"], bar["min_y"], bar["max_y"], bar["min_z"], bar["max_z"]) == (1, 3, 0, 0, 0, 0)
    assert (bar["sum_x"], bar["sum_y"], bar["sum_z"]) == (6, 0, 0)
    assert bar["mass_q"] == (1 << 19) + 3 * (1 << 20) and list(bar["mom_q"]) == [-(1 << 20), 3 << 18, 0]
    rec, grid, counts = R.objects(occ, res, 26, min_cells=2, max_objects=1)
    assert counts == (1, 2, 5) and list(rec["label"]) == [1] and rec[0]["count"] == 4 and rec[0]["max_x"] == 4 and rec[0]["max_y"] == 1
    assert list(grid.ravel()[[1, 2, 3, 9, 25]]) == [0, 0, 0, 0, -1]
    rec, grid, counts = R.objects(occ, res, 6, min_cells=1, max_objects=2)
    assert counts == (3, 3, 5) and len(rec) == 2 and grid.ravel()[25] == 2   # the list is cut, the counts and the grid are not
    c, lo, hi, v = R.states(R.objects(occ, res, 6)[0], (5, 3, 2), 0.5)
    assert np.allclose(c[0], (2.5 * 0.5 - 1.25, 0.5 * 0.5 - 0.75, 0.5 * 0.5 - 0.5)) and np.allclose(lo[0], (-0.75, -0.75, -0.5)) and np.allclose(hi[0], (0.75, -0.25, 0.0))
    assert np.allclose(v[0], (-1.0 / 3.5, 0.75 / 3.5, 0.0))


def _write_scene(path, shape, conn, seed):
    occ = R.scene(shape, seed)
    with open(path, "wb") as f:
        f.write(np.array([shape[0], shape[1], shape[2], conn], np.int32).tobytes())
        f.write(occ.astype(np.uint8).tobytes())
        f.write(lab_of(shape, conn, seed).astype(np.int32).tobytes())


def _has_runtime(tmp_path, flag):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp_path / "probe")
    return subprocess.run(["g++", flag, str(src), "-o", exe], capture_output=True).returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_labelling_core_on_the_host_under_sanitizers(tmp_path):
    """tests/objects_uf_check.cpp labels the scenes through dspmap_unionfind.h -- 4 orders sequentially, 4 times from 8 threads -- and
    compares cell for cell with the restatement's labels.  A sanitizer report or a differing cell fails the run."""
    files = []
    for shape, name in zip(SHAPES, IDS):
        for conn in (6, 26):
            files.append(str(tmp_path / ("%s_c%d.bin" % (name, conn))))
            _write_scene(files[-1], shape, conn, 11)
    src = os.path.join(ROOT, "tests", "objects_uf_check.cpp")
    assert _has_runtime(tmp_path, "-fsanitize=address,undefined")
    ran = []
    for tag, flag in (("asan_ubsan", "-fsanitize=address,undefined"), ("tsan", "-fsanitize=thread")):
        if tag == "tsan" and not _has_runtime(tmp_path, flag):
            continue   # (the toolchain has no ThreadSanitizer runtime: the first build has run)
        exe = str(tmp_path / ("uf_check_" + tag))
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-pthread", flag, "-fno-sanitize-recover=all", src, "-o", exe])
        r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.count("OK ") == len(files), (tag, r.stdout[-2000:], r.stderr[-4000:])
        ran.append(tag)
    assert "asan_ubsan" in ran


def test_labelling_core_reports_a_broken_invariant_instead_of_looping(tmp_path):
    """uf_find / uf_unite on label arrays that break L[x] <= x (a cycle, a label above its cell): a fault code, at once"""
    src = tmp_path / "broken.cpp"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_unionfind.h") +
                   "struct Mem { int* L; int load(int i) const { return L[i]; }\n"
                   "    int atomic_min(int i, int v) const { const int o = L[i]; if (v < o) L[i] = v; return o; } };\n"
                   "int main() {\n"
                   "    int cyc[4] = {0, 2, 1, 3}; Mem a{cyc}; int f = 0;\n"
                   "    if (uf_find(a, 1, 4, &f) != -1 || f != UF_FAULT_CHAIN) return 1;\n"
                   "    if (uf_unite(a, 3, 1, 4) != UF_FAULT_CHAIN) return 2;\n"
                   "    int neg[3] = {0, -1, 1}; Mem b{neg}; f = 0;\n"
                   "    if (uf_find(b, 2, 3, &f) != -1 || f != UF_FAULT_CHAIN) return 3;\n"
                   "    int ok[4] = {0, 0, 2, 2}; Mem c{ok}; f = 0;\n"
                   "    if (uf_find(c, 1, 4, &f) != 0 || f || uf_unite(c, 3, 1, 4) != UF_OK || ok[2] != 0 || uf_find(c, 3, 4, &f) != 0) return 4;\n"
                   "    int chain[4] = {0, 0, 1, 2}; Mem d{chain}; f = 0;\n"
                   "    if (uf_find(d, 3, 1, &f) != -1 || f != UF_FAULT_BOUND) return 5;\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "broken")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined", str(src), "-o", exe])
    assert subprocess.run([exe], timeout=60).returncode == 0


def test_dropin_class_offers_object_members(tmp_path):
    """include/dsp_dynamic.h: buildObjects, getObjects and queryObjects type-check under -Wall and forward to the C ABI"""
    src = tmp_path / "objects.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    std::vector<dspmap_object> objs(100);\n    std::vector<dspmap_query> q(4);\n    std::vector<int> ord(4);\n    int n = 0;\n"
                   "    int a = my_map.buildObjects() + my_map.buildObjects(6, 4, 64, 0.5f);\n"
                   "    int b = my_map.getObjects((int)objs.size(), objs.data(), n) + my_map.queryObjects(4, q.data(), ord.data()) + my_map.queryObjects(4, q.data(), ord.data(), true);\n"
                   "    static_assert(sizeof(dspmap_object) == 88, \"layout\");\n"
                   "    return a + b + n + objs[0].label + objs[0].count + objs[0].min_x + objs[0].max_z + (int)(objs[0].sum_x + objs[0].mass_q + objs[0].mom_q[2]);\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_build_objects(h_", "dspmap_get_objects(h_", "dspmap_query_objects(h_"):
        assert call in hdr, call


def test_binding_matches_the_header(dsp):
    """OBJECT_DTYPE is dspmap_object, field for field, and the Python surface exists"""
    assert dsp.capi.OBJECT_DTYPE == R.OBJECT_DTYPE and dsp.capi.OBJECT_DTYPE.itemsize == 88
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    body = hdr[hdr.index("typedef struct dspmap_object {"):hdr.index("} dspmap_object;")]
    order = [body.index(n) for n in ("label;", "count;", "min_x,", "max_x,", "min_y,", "max_y,", "min_z,", "max_z;", "sum_x,", "sum_y,", "sum_z;", "mass_q;", "mom_q[3];")]
    assert order == sorted(order)
    for name in ("build_objects", "object_counts", "objects", "object_labels", "query_objects", "object_states"):
        assert callable(getattr(dsp.DSPMap, name)), name
