"""CPU tests of the nearest-obstacle fields' restatement (tests/nearest_ref.py) and of the argument checks of their entry points
(include/dspmap.h, dspmap_build_nearest_field): the brute force under the key d2 * V + index equals the separable per-axis lexicographic
argmin on random grids, signed and unsigned, truncated and not; the unsigned distances are the distance field's; the distances agree with
scipy's EDT where scipy exists; the hand-made tie scenes of the GPU tests really contain ties; and every argument error fires before the
device is touched, text for text, in the order of the header's list."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import distance_ref as D
from tests import nearest_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAN = float("nan")


def _random_grids(n, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        shape = tuple(int(v) for v in rng.integers(1, 10, 3))
        dens = (0.02, 0.1, 0.4, 0.98)[i % 4]
        yield rng.random(shape) < dens, int(rng.integers(1, 7))


def test_brute_force_equals_separable_route():
    """shapes 1 .. 9 per axis, densities 0.02 / 0.1 / 0.4 / 0.98, R 1 .. 6 and untruncated, both modes: D2 and the index are equal"""
    seen_tie = seen_none = seen_edge = 0
    for occ, R in _random_grids(240, 5):
        for signed in (False, True):
            for r in (R, None):
                bd, bn = N.nearest_brute(occ, r, signed)
                sd, sn = N.nearest_separable(occ, r, signed)
                assert np.array_equal(bd, sd) and np.array_equal(bn, sn), (occ.shape, R, signed, r)
                assert ((bn == -1) == (bd == N.INF)).all()
            td, tn = N.truncate(*N.nearest_separable(occ, None, signed), R)      # truncation only takes targets away
            d_r, n_r = N.nearest_brute(occ, R, signed)
            assert np.array_equal(td, d_r) and np.array_equal(tn, n_r), (occ.shape, R, signed)
        d2, near = N.nearest_brute(occ, R, False)
        assert (near[occ] == np.flatnonzero(occ.ravel())).all() and (d2[occ] == 0).all()      # an occupied cell targets itself
        d2s, nears = N.nearest_brute(occ, R, True)
        hit = nears >= 0
        assert (occ.ravel()[nears[hit]] != occ[hit]).all() and (d2s[hit] >= 1).all()          # signed: always the other class
        seen_tie += int((N.count_minimisers(occ)[~occ] > 1).sum())
        seen_none += int((near == -1).sum())
        seen_edge += int((d2 == R * R).sum())
    assert seen_tie > 1000 and seen_none > 1000 and seen_edge > 100


def test_unsigned_distance_is_the_distance_field():
    for occ, R in _random_grids(60, 9):
        d2, _ = N.nearest_separable(occ, R, False)
        assert np.array_equal(np.minimum(d2, R * R), np.minimum(D.d2_separable(occ), R * R))
        got = N.value(d2, occ, R, F(0.15)).view(np.uint32)
        assert np.array_equal(got, D.value(D.d2_brute(occ), R, F(0.15)).view(np.uint32))
        sd2, _ = N.nearest_separable(occ, R, True)
        sv = N.value(sd2, occ, R, F(0.15), signed=True)
        assert (sv[occ] < 0).all() and (sv[~occ] > 0).all() and not np.signbit(sv[~occ]).any()


def test_distances_agree_with_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    for occ, R in _random_grids(60, 13):
        if occ.all() or not occ.any():
            continue
        edt2 = np.rint(ndi.distance_transform_edt(~occ) ** 2).astype(np.int64)
        _, near = N.nearest_separable(occ, R, False)
        cells = np.stack(np.meshgrid(*[np.arange(n) for n in occ.shape], indexing="ij"), -1).reshape(-1, 3)
        tgt = np.stack(np.unravel_index(np.maximum(near.ravel(), 0), occ.shape), -1)
        mine = ((cells - tgt) ** 2).sum(1).reshape(occ.shape)
        within = edt2 <= R * R
        assert ((near >= 0) == within).all()
        assert np.array_equal(mine[within], edt2[within])      # distances only: scipy's tie rule is another


def test_tie_scenes_contain_the_ties_they_are_made_for():
    shape = (23, 37, 50)
    scenes = {name: (g, cell) for name, g, cell in N.tie_scenes(shape, 6)}
    for prefix, n_min in (("pair_x", 3), ("pair_y", 3), ("pair_z", 3), ("xy_5", 4), ("xz_5", 4), ("yz_5", 4), ("345_", 10)):
        names = [k for k in scenes if k.startswith(prefix)]
        assert len(names) >= n_min, prefix
        for k in names:
            g, cell = scenes[k]
            assert N.count_minimisers(g)[cell] >= 2, k
            d2, near = N.nearest_brute(g, 6, False)
            sd, sn = N.nearest_separable(g, 6, False)
            assert np.array_equal(near, sn) and np.array_equal(d2, sd), k
            tie = np.flatnonzero(g.ravel())
            assert near[cell] == tie[((np.stack(np.unravel_index(tie, shape), -1) - np.array(cell)) ** 2).sum(1) == d2[cell]].min(), k
    g, cell = scenes["345_xyz_+1"]
    assert N.count_minimisers(g)[cell] == 3 and N.nearest_brute(g, 6)[0][cell] == 25
    g, cell = scenes["345_xyz_-1"]      # mirrored: the far negative z side wins
    assert np.unravel_index(N.nearest_brute(g, 6)[1][cell], shape) == (cell[0] - 5, cell[1], cell[2])
    # the truncation scenes: a cell exactly R away is a target, one R + 1 away is none
    g, _ = scenes["edge_x0"]
    d2, near = N.nearest_separable(g, 6)
    assert near[0, 0, 6] == 0 and d2[0, 0, 6] == 36 and near[0, 0, 7] == -1
    # signed, the last columns: the free target lies to the left
    g, _ = scenes["last_columns"]
    d2, near = N.nearest_separable(g, 6, True)
    assert d2[0, 0, 49] == 16 and near[0, 0, 49] == 45
    # the small shapes keep what fits
    assert len(N.tie_scenes((1, 8, 8), 6)) >= 12 and all(g.shape == (1, 8, 8) for _, g, _ in N.tie_scenes((1, 8, 8), 6))


def test_bits_of_packs_the_cast_grid_layout():
    occ = np.random.default_rng(3).random((2, 3, 4, 70)) < 0.5
    w = N.bits_of(occ)
    assert w.shape == (2, 3, 4, 2) and w.dtype == np.uint64
    for x in (0, 1, 63, 64, 69):
        assert np.array_equal((w[..., x >> 6] >> np.uint64(x & 63)) & np.uint64(1), occ[..., x].astype(np.uint64))
    assert not (w[..., 1] >> np.uint64(6)).any()


class _Buf:
    def __repr__(self):
        return "B"


B = _Buf()
_ZERO = np.zeros(1 << 16, np.uint8)
HANDLES = {"W": dict(nx=20, ny=20, nz=10, res=0.15),
           "S": dict(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3)}
NO_GRID = "%s: no cast grid, or the map has changed since it was built (dspmap_build_cast_grid)"
NO_FIELD = "%s: no nearest field, or the map or the cast grid it was built from has changed since (dspmap_build_nearest_field)"
BLD = "dspmap_build_nearest_field"
# (n, q, flags, outside, out): both query entry points
QUERY = [
    ('W', (-1, B, 0, 0.0, B), -1, 'nearest query: negative sample count -1'),
    ('W', (4, None, 0, 0.0, B), -1, 'nearest query: NULL sample or output array'),
    ('W', (4, B, 0, 0.0, None), -1, 'nearest query: NULL sample or output array'),
    ('W', (4, B, 2, 0.0, B), -1, 'nearest query: unknown flags 0x2'),
    ('W', (4, B, 1, NAN, B), -1, 'nearest query: outside_value is NaN'),
    ('W', (4, B, 1, 0.0, B), -3, NO_FIELD % 'dspmap_query_nearest'),
    ('W', (0, None, 0, 0.0, None), -3, NO_FIELD % 'dspmap_query_nearest'),
    ('S', (4, B, 0, 0.0, B), -3, NO_FIELD % 'dspmap_query_nearest'),
    ('W', (-1, None, 2, NAN, None), -1, 'nearest query: negative sample count -1'),
    ('W', (4, None, 2, NAN, None), -1, 'nearest query: NULL sample or output array'),
    ('W', (4, B, 2, NAN, B), -1, 'nearest query: unknown flags 0x2'),
]
CASES = [
    # dspmap_build_nearest_field (threshold, max_voxels, flags): the arguments, then the slab, then the cast grid
    ('W', BLD, (NAN, 20, 0), -1, BLD + ': threshold is NaN'),
    ('W', BLD, (NAN, 20, 1), -1, BLD + ': threshold is NaN'),
    ('W', BLD, (0.2, 0, 0), -1, BLD + ': max_voxels 0 outside [1, 64]'),
    ('W', BLD, (0.2, 65, 3), -1, BLD + ': max_voxels 65 outside [1, 64]'),
    ('W', BLD, (0.2, 20, 4), -1, BLD + ': unknown flags 0x4'),
    ('W', BLD, (0.2, 20, 11), -1, BLD + ': unknown flags 0xb'),
    ('S', BLD, (0.2, 20, 0), -3, BLD + ': a slab handle holds part of the map; distances cross slabs'),
    ('S', BLD, (0.2, 20, 3), -3, BLD + ': a slab handle holds part of the map; distances cross slabs'),
    ('W', BLD, (0.2, 20, 2), -3, NO_GRID % BLD),
    ('W', BLD, (NAN, 64, 3), -3, NO_GRID % BLD),                 # (from the cast grid the threshold is not read)
    ('W', BLD, (NAN, 0, 8), -1, BLD + ': threshold is NaN'),      # two checks broken at once: the earlier one answers
    ('W', BLD, (NAN, 0, 10), -1, BLD + ': max_voxels 0 outside [1, 64]'),
    ('S', BLD, (0.2, 65, 8), -1, BLD + ': max_voxels 65 outside [1, 64]'),
    ('S', BLD, (0.2, 64, 8), -1, BLD + ': unknown flags 0x8'),
    # dspmap_get_nearest_field (layer, near_out, dist_out)
    ('W', 'dspmap_get_nearest_field', (0, None, None), -1, 'nearest field: both output arrays are NULL'),
    ('W', 'dspmap_get_nearest_field', (-1, B, B), -1, 'nearest field: layer -1 outside [0, 7)'),
    ('W', 'dspmap_get_nearest_field', (7, B, None), -1, 'nearest field: layer 7 outside [0, 7)'),
    ('W', 'dspmap_get_nearest_field', (7, None, None), -1, 'nearest field: both output arrays are NULL'),
    ('W', 'dspmap_get_nearest_field', (0, B, B), -3, NO_FIELD % 'dspmap_get_nearest_field'),
    ('W', 'dspmap_get_nearest_field', (6, None, B), -3, NO_FIELD % 'dspmap_get_nearest_field'),
    ('S', 'dspmap_get_nearest_field', (0, B, None), -3, NO_FIELD % 'dspmap_get_nearest_field'),
] + [(k, fn, a, rc, t) for fn in ("dspmap_query_nearest", "dspmap_query_nearest_device") for k, a, rc, t in QUERY]


def test_nearest_errors_text_for_text(dsp):
    L = dsp.load_library()
    maps = {k: dsp.DSPMap(dsp.make_config(**kw)) for k, kw in HANDLES.items()}
    assert all(m.T == 6 for m in maps.values())
    seen = set()
    for kind, fn, args, rc, text in CASES:
        h = maps[kind].h
        call = [_ZERO.ctypes.data_as(C.c_void_p) if a is B else a for a in args]
        got = getattr(L, fn)(h, *call)
        assert (got, L.dspmap_last_error(h).decode()) == (rc, text), (kind, fn, args)
        if fn not in seen:                      # a NULL handle: DSPMAP_E_ARG from every entry point, before anything else
            assert getattr(L, fn)(None, *call) == E_ARG, fn
            seen.add(fn)
    assert not _ZERO.any()                      # no call wrote into its output array
    for m in maps.values():
        assert L.dspmap_nearest_field_device(m.h) is None and L.dspmap_nearest_distance_device(m.h) is None
        assert m.nearest_field_ptr() is None and m.nearest_distance_ptr() is None
        m.close()
    assert L.dspmap_nearest_field_device(None) is None and L.dspmap_nearest_distance_device(None) is None
    names = {c[1] for c in CASES}
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for fn in names:
        assert fn in dsp.capi.SIGNATURES and "%s(dspmap_t* m" % fn in hdr, fn
    assert names == {BLD, "dspmap_get_nearest_field", "dspmap_query_nearest", "dspmap_query_nearest_device"}


def test_nearest_valid_build_needs_device(dsp):
    """without a device a valid build from the masses is DSPMAP_E_DEVICE ("no HIP device"): there is no CPU fallback; the binding raises
    and names what is missing"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    have = torch.cuda.is_available()
    assert L.dspmap_build_nearest_field(m.h, 0.5, 4, dsp.capi.NEAREST_SIGNED) == (OK if have else E_DEVICE)
    if have:
        near, dist = m.nearest_field(), m.nearest_distance()
        assert near.shape == dist.shape == (7, 10, 20, 20) and near.dtype == np.int32 and dist.dtype == F
        assert (near == -1).all() and (dist == F(4) * F(0.15)).all()      # an empty map: no target anywhere
    else:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError, match="no HIP device"):
            m.build_nearest_field(0.5, 4)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_cast_grid"):
            m.build_nearest_field(0.5, 4, from_cast_grid=True)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_nearest_field"):
            m.nearest_field(0)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_nearest_field"):
            m.nearest_distance()
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_nearest_field"):
            m.query_nearest(np.zeros((3, 4), F))
    m.close()
    assert dsp.capi.NEAREST_DTYPE.itemsize == 32 and N.NEAREST_DTYPE == dsp.capi.NEAREST_DTYPE
