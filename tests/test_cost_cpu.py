"""CPU tests of the clearance-weighted cost-to-go fields (dspmap_build_cost_fields*, dspmap_cost_paths*, the accessors and the
dspmap_debug_set_distance_field hook): the entry points are exported and bound, the drop-in class offers the new members, and the numpy
restatement the GPU tests hold the kernels to (tests/cost_ref.py) agrees with itself -- relaxation against a heap Dijkstra on random small
grids, the header's known answer, and the n_bands == 0 identity with tests/reach_ref.fields."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cost_ref as K
from tests import reach_ref as R

NAMES = ("dspmap_build_cost_fields", "dspmap_build_cost_fields_device", "dspmap_cost_fields_device", "dspmap_get_cost_field",
         "dspmap_cost_weights_device", "dspmap_get_cost_weights", "dspmap_cost_paths", "dspmap_cost_paths_device",
         "dspmap_debug_set_distance_field")
F = np.float32
U = K.UNREACHED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _centre(cfg, x, y, z):
    res = cfg.voxel_resolution
    return (-0.5 * res * cfg.nx + res * (x + 0.5), -0.5 * res * cfg.ny + res * (y + 0.5), -0.5 * res * cfg.nz + res * (z + 0.5))


def _at(cfg, *cells):
    return R.points([_centre(cfg, *c[:3]) + ((c[3] if len(c) > 3 else 0),) for c in cells])


def test_cost_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert n + "(dspmap_t* m" in hdr, n
    cap = dsp.capi
    assert (cap.COST_MAX_BANDS, cap.COST_MAX_WEIGHT, cap.COST_MAX_FIELDS, cap.COST_MAX_COST, cap.COST_UNREACHED) == (4, 8, 64, 16384, 65535)
    assert (K.MAX_BANDS, K.MAX_WEIGHT, K.MAX_FIELDS, K.MAX_COST, K.UNREACHED) == (4, 8, 64, 16384, 65535)
    assert C.sizeof(cap.CostBands) == 36
    for line in ("#define DSPMAP_COST_MAX_BANDS 4", "#define DSPMAP_COST_MAX_WEIGHT 8", "#define DSPMAP_COST_MAX_FIELDS 64",
                 "#define DSPMAP_COST_MAX_COST 16384", "#define DSPMAP_COST_UNREACHED 65535"):
        assert line in hdr, line
    for meth in ("build_cost_fields", "cost_field", "cost_fields_ptr", "cost_weights", "cost_paths", "set_distance_field"):
        assert callable(getattr(dsp.DSPMap, meth))
    assert '"dspmap_cost.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()


def test_binding_shapes_and_bands(dsp):
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    b = m._cost_bands([(0.3, 2), (0.6, 1)])
    assert b.n_bands == 2 and list(b.penalty)[:2] == [2, 1] and abs(b.clearance[1] - 0.6) < 1e-6
    assert m._cost_bands([(0.1, 1)] * 5).n_bands == 5                         # the count survives: the library refuses it
    with pytest.raises(ValueError):
        m.build_cost_fields(np.zeros((3, 5), F))
    with pytest.raises(ValueError):
        m.cost_field()
    with pytest.raises(ValueError):
        m.set_distance_field(np.zeros((1, 10, 20, 20), F))
    with pytest.raises(dsp.capi.DSPMapError, match="n_bands 5"):
        m.build_cost_fields(np.zeros((1, 4), F), bands=[(0.1, 1)] * 5)
    assert m.cost_fields_ptr() is None
    m.close()


def test_dropin_class_offers_cost_members(dsp, tmp_path):
    """include/dsp_dynamic.h: buildCostFields, getCostField, getCostWeights and costPaths type-check and forward to the C ABI"""
    src = tmp_path / "cost.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    dspmap_reach_point s[1] = {{0.f, 0.f, 0.f, 0}};\n"
                   '    static_assert(sizeof(dspmap_cost_bands) == 36, "layout");\n'
                   "    dspmap_cost_bands b = {1, {0.3f, 0.f, 0.f, 0.f}, {2, 0, 0, 0}};\n"
                   "    std::vector<unsigned short> v(1); std::vector<unsigned char> w(1); int cost[1], cells[4];\n"
                   "    int rc = my_map.buildCostFields(1, 1, s, -1.f, b, DSPMAP_COST_MAX_COST);\n"
                   "    rc += my_map.getCostField(0, v.data()) + my_map.getCostWeights(w.data()) + my_map.costPaths(1, s, 4, cost, cells, true);\n"
                   "    return rc == 0;\n}\n")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_known_answer_from_the_restatement_alone(dsp):
    """the header's example: 10 x 3 x 1, row y = 0 at F = 0.05, the others at 1.0, band {0.1, 4}, source (0, 0, 0), max_cost 100"""
    cfg = dsp.make_config(nx=10, ny=3, nz=1, res=0.15)
    blocked = np.zeros((1, 3, 10), bool)
    dist = np.full((1, 3, 10), 1.0, F)
    dist[0, 0] = 0.05
    w = K.weights(blocked, dist, [(0.1, 4)])
    assert w[0, 0].tolist() == [5] * 10 and w[0, 1].tolist() == [1] * 10 and w[0, 2].tolist() == [1] * 10
    src = _at(cfg, (0, 0, 0))
    for fn in (K.fields, K.dijkstra):
        val = fn(cfg, w, src, 1, max_cost=100)
        assert val[0, 0, 0].tolist() == [0, 5, 8, 9, 10, 11, 12, 13, 14, 15]
        assert val[0, 0, 1].tolist() == list(range(1, 11)) and val[0, 0, 2].tolist() == list(range(2, 12))
    K.check_fields(cfg, w, val, src, max_cost=100)
    start = _at(cfg, (9, 0, 0))
    cost, cells = K.paths(cfg, val, w, start, 16)
    want = [9, 19] + [10 + x for x in range(8, -1, -1)] + [0]                 # (9,0), (9,1), (8,1) .. (0,1), (0,0)
    assert cost.tolist() == [15] and cells[0, :12].tolist() == want and (cells[0, 12:] == -1).all()
    assert K.check_paths(cfg, val, w, start, cost, cells) == 1
    # the unweighted field reads 9 there, and its path stays in row 0
    w1 = K.weights(blocked, None, [])
    val1 = K.fields(cfg, w1, src, 1, max_cost=100)
    cost1, cells1 = K.paths(cfg, val1, w1, start, 16)
    assert cost1.tolist() == [9] and cells1[0, :10].tolist() == list(range(9, -1, -1))
    # a cut: values above max_cost read UNREACHED
    cut = K.fields(cfg, w, src, 1, max_cost=9)
    assert np.array_equal(cut, np.where(val <= 9, val, U))


@pytest.mark.parametrize("seed", range(6))
def test_relaxation_equals_dijkstra_on_random_small_grids(dsp, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = (int(v) for v in rng.integers(1, 12, 3))
    cfg = dsp.make_config(nx=nx, ny=ny, nz=nz, res=0.15)
    blocked = rng.random((nz, ny, nx)) < 0.25
    dist = rng.random((nz, ny, nx)).astype(F)
    bands = [[(0.5, 7)], [(0.3, 1), (0.6, 2), (0.9, 3)], [(0.2, 1), (0.4, 1), (0.6, 2), (0.8, 3)], []][seed % 4]
    w = K.weights(blocked, dist, bands)
    assert w.max() <= 8 and ((w == 0) == blocked).all()
    nf = 3
    cells = [(int(rng.integers(nx)), int(rng.integers(ny)), int(rng.integers(nz)), int(rng.integers(-1, nf + 1))) for _ in range(8)]
    src = np.concatenate([_at(cfg, *cells), R.points([(np.nan, 0.0, 0.0, 0), (100.0, 0.0, 0.0, 1)])])
    for max_cost in (K.MAX_COST, 9, 1):
        a, b = K.fields(cfg, w, src, nf, max_cost=max_cost), K.dijkstra(cfg, w, src, nf, max_cost=max_cost)
        assert np.array_equal(a, b), (seed, max_cost, np.argwhere(a != b)[:4])
        K.check_fields(cfg, w, a, src, max_cost=max_cost)
        cost, pc = K.paths(cfg, a, w, src, 40)
        K.check_paths(cfg, a, w, src, cost, pc)


@pytest.mark.parametrize("shape", [(40, 40, 24), (65, 6, 3), (8, 8, 1)])
def test_no_bands_is_the_static_reach_field(dsp, shape):
    """n_bands == 0: uint16 for uint16 the static dspmap_build_reach_fields build with max_steps = max_cost, and the same paths"""
    nx, ny, nz = shape
    cfg = dsp.make_config(nx=nx, ny=ny, nz=nz, res=0.15)
    rng = np.random.default_rng(3)
    lay = np.zeros((cfg.prediction_times + 1, nz, ny, nx), bool)
    lay[0] = rng.random((nz, ny, nx)) < 0.3
    free = np.argwhere(~lay[0])
    pick = free[rng.integers(0, len(free), 6)]
    src = _at(cfg, *[(int(c[2]), int(c[1]), int(c[0]), k % 2) for k, c in enumerate(pick)])
    w = K.weights(lay[0], None, [])
    for max_cost in (200, 7):
        mine = K.fields(cfg, w, src, 2, max_cost=max_cost)
        theirs = R.fields(cfg, lay, src, 2, max_steps=max_cost)
        assert np.array_equal(mine, theirs) and (mine != U).sum() > 2
        a, b = K.paths(cfg, mine, w, src, 30), R.paths(cfg, theirs, src, 30)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
