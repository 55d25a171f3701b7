"""CPU tests of the frontier extension (dspmap_build_frontiers and its accessors, dspmap_debug_set_known): hand-worked answers of the numpy
restatement (tests/frontier_ref.py) on grids small enough to count by hand, its invariants on the synthetic scene the GPU tests use, and
the real library without a device: the symbols are exported and bound, every argument error is DSPMAP_E_ARG with a text before any device
is touched, and a valid call reports the missing grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import frontier_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ["dspmap_build_frontiers", "dspmap_frontier_counts", "dspmap_get_frontier_grid", "dspmap_get_frontier_cells",
         "dspmap_get_frontier_blocks", "dspmap_frontier_grid_device", "dspmap_frontier_cells_device", "dspmap_frontier_blocks_device",
         "dspmap_frontier_counts_device", "dspmap_debug_set_known"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rec(*rows):
    return np.array(list(rows), R.BLOCK_DTYPE)


# ---- the restatement, by hand
def test_single_known_free_cell_in_an_unknown_map():
    """3 x 3 x 3, only the centre (1, 1, 1) known and free: all six neighbours lie inside the map and are unknown"""
    age = np.full((3, 3, 3), -1, np.int32)
    age[1, 1, 1] = 0
    occ = np.zeros((3, 3, 3), bool)
    for mu in range(1, 7):
        fr, u, free = R.frontier(occ, age, 0, mu)
        assert R.cells(fr).tolist() == [13] and free.sum() == 1 and u[1, 1, 1] == 6
    # every other cell: unknown, and its u counts unknown neighbours only -- a face centre touches the known centre
    assert u[0, 1, 1] == 4 and u[0, 0, 1] == 4 and u[0, 0, 0] == 3
    assert R.blocks(fr, u, 1).tolist() == _rec((13, 1, 1, 1, 1, 6)).tolist()          # block 1: the block index is the voxel index
    assert R.blocks(fr, u, 32).tolist() == _rec((0, 1, 1, 1, 1, 6)).tolist()          # block 32: one block holds the map
    assert R.blocks(fr, u, 2).tolist() == _rec((0, 1, 1, 1, 1, 6)).tolist()           # (1, 1, 1) / 2 = (0, 0, 0) of 2 x 2 x 2 blocks
    assert R.pack(fr)[1, 1, 0] == 2 and R.pack(fr).sum() == 2


def test_corner_cell_the_map_edge_contributes_nothing():
    age = np.full((3, 3, 3), -1, np.int32)
    age[0, 0, 0] = 1
    occ = np.zeros((3, 3, 3), bool)
    fr, u, free = R.frontier(occ, age, 1, 3)
    assert u[0, 0, 0] == 3 and R.cells(fr).tolist() == [0]                            # three neighbours inside, all unknown
    assert not R.frontier(occ, age, 1, 4)[0].any()                                    # the three outside do not exist
    assert not R.frontier(occ, age, 0, 1)[0].any()                                    # age 1 > max_age 0: the cell itself is unknown
    fr2, u2, _ = R.frontier(occ, age, 1, 1)
    assert R.blocks(fr2, u2, 32).tolist() == _rec((0, 1, 0, 0, 0, 3)).tolist()


def test_occupied_known_cell_is_never_a_frontier_and_min_unknown_1_against_6():
    """the centre known and free, its -x neighbour known and OCCUPIED, the rest unknown: the centre has u = 5"""
    age = np.full((3, 3, 3), -1, np.int32)
    age[1, 1, 1] = 0
    age[1, 1, 0] = 0
    occ = np.zeros((3, 3, 3), bool)
    occ[1, 1, 0] = True
    fr1, u, free = R.frontier(occ, age, 0, 1)
    assert u[1, 1, 1] == 5 and u[1, 1, 0] == 4
    assert R.cells(fr1).tolist() == [13] and free.sum() == 1                          # the occupied cell: known, u = 4, not free
    assert R.cells(R.frontier(occ, age, 0, 5)[0]).tolist() == [13]
    assert not R.frontier(occ, age, 0, 6)[0].any()
    occ[1, 1, 0] = False                                                              # freed: a frontier cell of its own, u = 4 (-x is outside)
    fr, u, free = R.frontier(occ, age, 0, 4)
    assert R.cells(fr).tolist() == [12, 13] and free.sum() == 2
    assert R.blocks(fr, u, 32).tolist() == _rec((0, 2, 1, 2, 2, 9)).tolist()
    assert R.blocks(fr, u, 1).tolist() == _rec((12, 1, 0, 1, 1, 4), (13, 1, 1, 1, 1, 5)).tolist()


def test_row_of_four():
    """4 x 1 x 1, ages {0, 0, -1, 5}: with max_age = 2 the last cell is too old to be known"""
    age = np.array([0, 0, -1, 5], np.int32).reshape(1, 1, 4)
    occ = np.zeros((1, 1, 4), bool)
    fr, u, free = R.frontier(occ, age, 2, 1)
    assert u.ravel().tolist() == [0, 1, 1, 1] and free.ravel().tolist() == [True, True, False, False]
    assert fr.ravel().tolist() == [False, True, False, False]
    fr, u, free = R.frontier(occ, age, 5, 1)
    assert u.ravel().tolist() == [0, 1, 0, 1] and fr.ravel().tolist() == [False, True, False, True]
    assert R.cells(fr).tolist() == [1, 3]
    assert R.blocks(fr, u, 2).tolist() == _rec((0, 1, 1, 0, 0, 1), (1, 1, 3, 0, 0, 1)).tolist()
    assert R.blocks(fr, u, 1).tolist() == _rec((1, 1, 1, 0, 0, 1), (3, 1, 3, 0, 0, 1)).tolist()
    assert R.blocks(fr, u, 32).tolist() == _rec((0, 2, 4, 0, 0, 2)).tolist()
    assert not R.frontier(occ, age, 5, 2)[0].any()
    occ[0, 0, 1] = True
    assert R.cells(R.frontier(occ, age, 5, 1)[0]).tolist() == [3]
    assert R.centers(R.blocks(fr, u, 32), (4, 1, 1), 0.5).tolist() == [[0.25, 0.0, 0.0]]   # mean index 2 -> (2.5) * 0.5 - 1


@pytest.mark.parametrize("shape", [(66, 12, 8), (16, 16, 6), (3, 3, 3), (130, 40, 24)])
def test_invariants_on_the_scene(shape):
    occ, age = R.scene(shape)
    nx, ny, nz = shape
    for mu in (1, 2, 4, 6):
        fr, u, free = R.frontier(occ, age, 2, mu)
        assert not (fr & ~free).any() and 0 <= u.min() and u.max() <= 6
        c = R.cells(fr)
        assert (np.diff(c) > 0).all() and c.size == fr.sum()
        x, y, z = c % nx, (c // nx) % ny, c // (nx * ny)
        for block in (1, 4, 5, 32):
            b = R.blocks(fr, u, block)
            assert (np.diff(b["block"]) > 0).all() and (b["count"] > 0).all()
            assert b["count"].sum() == c.size
            assert (b["sum_x"].sum(), b["sum_y"].sum(), b["sum_z"].sum()) == (x.sum(), y.sum(), z.sum())
            assert b["unknown_faces"].sum() == u[fr].sum()
            if block == 1:
                assert (b["block"] == c).all() and (b["count"] == 1).all()
    counts = {(66, 12, 8): None, (130, 40, 24): None, (16, 16, 6): (439, 268, 35), (3, 3, 3): (7, 4, 1)}[shape]
    if counts:
        assert tuple(int(R.frontier(occ, age, 2, mu)[0].sum()) for mu in (1, 2, 4)) == counts


# ---- the library without a device
def test_frontier_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert "%s(dspmap_t* m" % n in hdr, n
    for meth in ("build_frontiers", "frontier_counts", "frontier_grid", "frontier_cells", "frontier_blocks", "frontier_block_centers",
                 "set_known"):
        assert callable(getattr(dsp.DSPMap, meth))
    assert "#define DSPMAP_FRONTIER_MAX_BLOCK 32" in hdr and dsp.capi.FRONTIER_MAX_BLOCK == 32
    assert dsp.capi.FRONTIER_BLOCK_DTYPE == R.BLOCK_DTYPE and R.BLOCK_DTYPE.itemsize == 24
    assert '"dspmap_frontier.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()
    blob = open(dsp.capi.LIB_PATH, "rb").read()
    for k in (b"k_frontier_mark", b"k_frontier_sums", b"k_frontier_scan", b"k_frontier_emit"):
        assert k in blob, k
    # the slot arithmetic of the known-space store is ONE copy in a shared header
    csrc = os.path.join(ROOT, "dsp-map_amd", "csrc")
    for f in ("dspmap_known.hip", "dspmap_view.hip", "dspmap_frontier.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "dspmap_known_slots.h"' in text and "int kn_slot(" not in text and "int vw_slot(" not in text, f
    assert "int kn_slot(" in open(os.path.join(csrc, "dspmap_known_slots.h")).read()


def test_frontier_argument_errors_without_a_device(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h)   # noqa: E731
    build = L.dspmap_build_frontiers
    assert build(None, -1.0, 2, 1, 4, 0) == E_ARG
    assert build(h, float("nan"), 2, 1, 4, 0) == E_ARG and b"NaN" in err()
    for age in (-1, -1000):
        assert build(h, -1.0, age, 1, 4, 0) == E_ARG and b"max_age" in err()
    for mu in (0, 7, -1):
        assert build(h, -1.0, 2, mu, 4, 0) == E_ARG and b"min_unknown" in err()
    for blk in (0, 33, -4):
        assert build(h, -1.0, 2, 1, blk, 0) == E_ARG and b"block" in err()
    for fl in (1, 2, -1):
        assert build(h, -1.0, 2, 1, 4, fl) == E_ARG and b"flags" in err()
    for t, mu, blk in ((-1.0, 1, 1), (0.3, 6, 32), (float("inf"), 3, 5)):          # valid arguments: the missing grid decides
        assert build(h, t, 0, mu, blk, 0) == E_STATE and b"dspmap_build_cast_grid" in err()
    cnt = (C.c_longlong * 3)(7, 7, 7)
    n = C.c_int(-5)
    words, cells, blocks = np.zeros((10, 20, 1), np.uint64), np.zeros(8, np.int32), np.zeros(8, R.BLOCK_DTYPE)
    assert L.dspmap_frontier_counts(None, cnt) == E_ARG
    assert L.dspmap_frontier_counts(h, None) == E_ARG and b"NULL" in err()
    assert L.dspmap_get_frontier_grid(None, _p(words)) == E_ARG
    assert L.dspmap_get_frontier_grid(h, None) == E_ARG and b"NULL" in err()
    for fn, buf in ((L.dspmap_get_frontier_cells, cells), (L.dspmap_get_frontier_blocks, blocks)):
        assert fn(None, 8, _p(buf), C.byref(n)) == E_ARG
        assert fn(h, -1, _p(buf), C.byref(n)) == E_ARG and b"negative" in err()
        assert fn(h, 8, None, C.byref(n)) == E_ARG and b"NULL" in err()
        assert fn(h, 8, _p(buf), None) == E_ARG and b"NULL" in err()
        assert fn(h, 0, None, None) == E_ARG and b"NULL" in err()
        # the accessors of a snapshot that was never built
        assert fn(h, 8, _p(buf), C.byref(n)) == E_STATE and b"dspmap_build_frontiers" in err()
        assert fn(h, 0, None, C.byref(n)) == E_STATE and b"dspmap_build_frontiers" in err()
    assert L.dspmap_frontier_counts(h, cnt) == E_STATE and b"dspmap_build_frontiers" in err()
    assert L.dspmap_get_frontier_grid(h, _p(words)) == E_STATE and b"dspmap_build_frontiers" in err()
    for fn in (L.dspmap_frontier_grid_device, L.dspmap_frontier_cells_device, L.dspmap_frontier_blocks_device, L.dspmap_frontier_counts_device):
        assert not fn(h) and not fn(None)
    assert list(cnt) == [7, 7, 7] and n.value == -5 and not words.any() and not cells.any()   # nothing was written
    # the test hook
    ages = np.zeros((10, 20, 20), np.int32)
    assert L.dspmap_debug_set_known(None, _p(ages)) == E_ARG
    assert L.dspmap_debug_set_known(h, None) == E_ARG and b"NULL" in err()
    assert L.dspmap_debug_set_known(h, _p(ages)) == E_STATE and b"no frame" in err()   # no accepted frame yet
    with pytest.raises(ValueError):
        m.set_known(np.zeros((10, 20, 19), np.int32))
    for call in (lambda: m.build_frontiers(max_age=2), lambda: m.build_frontiers(max_age=2, min_unknown=0), m.frontier_counts,
                 m.frontier_grid, m.frontier_cells, m.frontier_blocks, m.frontier_block_centers, lambda: m.set_known(ages)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_frontier_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    assert L.dspmap_build_frontiers(m.h, -1.0, 2, 1, 4, 0) == E_STATE and b"slab" in err()
    assert L.dspmap_build_frontiers(m.h, -1.0, 2, 9, 4, 0) == E_ARG                  # the argument checks come first
    assert L.dspmap_debug_set_known(m.h, _p(np.zeros((6, 16, 16), np.int32))) == E_STATE and b"slab" in err()
    m.close()


def test_dropin_class_offers_frontier_members(tmp_path):
    """include/dsp_dynamic.h: buildFrontiers, getFrontierCells and getFrontierBlocks type-check and forward to the C ABI"""
    src = tmp_path / "frontier.cpp"
    src.write_text('#include "dsp_dynamic.h"\n#include <vector>\nDSPMap my_map;\nint main() {\n'
                   "    std::vector<int> cells(1000);\n    std::vector<dspmap_frontier_block> blocks(100);\n    int n = 0, k = 0;\n"
                   "    int a = my_map.buildFrontiers(30) + my_map.buildFrontiers(30, 2, 8, 0.5f);\n"
                   "    int b = my_map.getFrontierCells((int)cells.size(), cells.data(), n) + my_map.getFrontierBlocks((int)blocks.size(), blocks.data(), k);\n"
                   "    static_assert(sizeof(dspmap_frontier_block) == 24 && DSPMAP_FRONTIER_MAX_BLOCK == 32, \"layout\");\n"
                   "    return a + b + n + k + blocks[0].block + blocks[0].count + blocks[0].sum_x + blocks[0].sum_y + blocks[0].sum_z + blocks[0].unknown_faces;\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_build_frontiers(h_", "dspmap_get_frontier_cells(h_", "dspmap_get_frontier_blocks(h_"):
        assert call in hdr, call
