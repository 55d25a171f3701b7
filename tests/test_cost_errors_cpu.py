"""The cost-to-go fields' errors that fire before the device is touched, text for text (include/dspmap.h, dspmap_build_cost_fields).

One table in the manner of tests/test_layer_errors_cpu.py: (handle, entry point, arguments behind the handle, return code, rendered
dspmap_last_error).  Every argument check of the header's list is there in its order, every entry point has a call that breaks two checks
at once, which pins the order -- arguments, then slab, then the snapshots --, and the two variants of a pair reject the same calls with the
same words.  A machine without a device never has a valid cast grid, so the one state error that needs one (bands without a distance
field) is checked with the life cycle in tests/test_gpu_cost.py; here a valid call is a grid and a build: the grid's build reports "no HIP
device" and the cost build finds no grid."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cost_ref as K
from tests import reach_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAN, INF = float("nan"), float("inf")
HANDLES = {"W": dict(nx=20, ny=20, nz=10, res=0.15),                     # a whole map, nothing built
           "S": dict(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3),   # a slab handle
           "G": dict(nx=400, ny=400, nz=210, res=0.15)}                  # large enough for the 2^31-cell caps


class _Buf:
    def __repr__(self):
        return "B"


B = _Buf()                                   # a valid array, large enough for whatever a check reads
_ZERO = np.zeros(1 << 16, np.uint8)
_KEEP = []


class Bands:
    """dspmap_cost_bands by value: n_bands, then up to four (clearance, penalty)"""

    def __init__(self, n, *pairs):
        self.n, self.pairs = n, pairs

    def __repr__(self):
        return "Bands(%d, %s)" % (self.n, self.pairs)

    def ptr(self, capi):
        b = capi.CostBands()
        b.n_bands = self.n
        for i, (c, p) in enumerate(self.pairs):
            b.clearance[i], b.penalty[i] = c, p
        _KEEP.append(b)
        return C.cast(C.pointer(b), C.c_void_p)


def _arg(a, capi):
    if a is B:
        return _ZERO.ctypes.data_as(C.c_void_p)
    if isinstance(a, Bands):
        return a.ptr(capi)
    return a


NONE = Bands(0)
ONE = Bands(1, (0.3, 2))
NO_GRID = "%s: no cast grid, or the map has changed since it was built (dspmap_build_cast_grid)"
NO_COST = ("%s: no cost fields, or the map, its cast grid or its distance field has changed since they were built "
           "(dspmap_build_cost_fields)")

# (n_fields, n_src, src, t, bands, max_cost, flags) -> code, text: both build entry points
BUILD = [
    ('W', (0, 1, B, -1.0, NONE, 100, 0), -1, 'cost fields: n_fields 0 outside [1, 64]'),
    ('W', (65, 1, B, -1.0, NONE, 100, 0), -1, 'cost fields: n_fields 65 outside [1, 64]'),
    ('W', (1, -1, B, -1.0, NONE, 100, 0), -1, 'cost fields: negative source count -1'),
    ('W', (1, 1, None, -1.0, NONE, 100, 0), -1, 'cost fields: NULL source array'),
    ('W', (1, 1, B, NAN, NONE, 100, 0), -1, 'cost fields: t is NaN'),
    ('W', (1, 1, B, -1.0, None, 100, 0), -1, 'cost fields: NULL bands'),
    ('W', (1, 1, B, -1.0, Bands(-1), 100, 0), -1, 'cost fields: n_bands -1 outside [0, 4]'),
    ('W', (1, 1, B, -1.0, Bands(5, (0.1, 1), (0.1, 1), (0.1, 1), (0.1, 1)), 100, 0), -1, 'cost fields: n_bands 5 outside [0, 4]'),
    ('W', (1, 1, B, -1.0, Bands(1, (NAN, 1)), 100, 0), -1, 'cost fields: clearance[0] = nan is NaN, infinite or not positive'),
    ('W', (1, 1, B, -1.0, Bands(2, (0.5, 1), (INF, 1)), 100, 0), -1, 'cost fields: clearance[1] = inf is NaN, infinite or not positive'),
    ('W', (1, 1, B, -1.0, Bands(1, (0.0, 1)), 100, 0), -1, 'cost fields: clearance[0] = 0 is NaN, infinite or not positive'),
    ('W', (1, 1, B, -1.0, Bands(1, (-0.5, 1)), 100, 0), -1, 'cost fields: clearance[0] = -0.5 is NaN, infinite or not positive'),
    ('W', (1, 1, B, -1.0, Bands(1, (0.5, -1)), 100, 0), -1, 'cost fields: penalty[0] = -1 outside [0, 7]'),
    ('W', (1, 1, B, -1.0, Bands(2, (0.5, 0), (0.5, 8)), 100, 0), -1, 'cost fields: penalty[1] = 8 outside [0, 7]'),
    ('W', (1, 1, B, -1.0, Bands(2, (0.5, 4), (0.7, 4)), 100, 0), -1,
     'cost fields: the largest weight 1 + sum of penalty = 9 exceeds DSPMAP_COST_MAX_WEIGHT = 8'),
    ('W', (1, 1, B, -1.0, NONE, 0, 0), -1, 'cost fields: max_cost 0 outside [1, 16384]'),
    ('W', (1, 1, B, -1.0, NONE, 16385, 0), -1, 'cost fields: max_cost 16385 outside [1, 16384]'),
    ('W', (1, 1, B, -1.0, NONE, 100, 2), -1, 'cost fields: unknown flags 0x2'),
    ('W', (1, 1, B, -1.0, NONE, 100, 8), -1, 'cost fields: unknown flags 0x8'),
    ('G', (64, 1, B, -1.0, NONE, 1, 0), -1, 'cost fields: 64 fields of 33600000 cells exceed 2^31 cells'),
    # what passes the arguments meets the state: a slab, then the grid (bands beyond n_bands are not looked at)
    ('S', (1, 1, B, -1.0, NONE, 100, 0), -3, 'cost fields: a slab handle holds part of the map; a wavefront crosses slabs'),
    ('W', (1, 0, None, -1.0, NONE, 100, 0), -3, NO_GRID % 'dspmap_build_cost_fields'),
    ('W', (64, 1, B, 0.3, Bands(4, (0.1, 1), (0.2, 1), (0.3, 2), (9.0, 3)), 16384, 1), -3, NO_GRID % 'dspmap_build_cost_fields'),
    ('W', (1, 1, B, INF, Bands(0, (NAN, 99)), 1, 0), -3, NO_GRID % 'dspmap_build_cost_fields'),
    ('W', (1, 1, B, -1.0, ONE, 100, 0), -3, NO_GRID % 'dspmap_build_cost_fields'),             # (the grid comes before the distance field)
    ('G', (63, 1, B, -1.0, NONE, 1, 0), -3, NO_GRID % 'dspmap_build_cost_fields'),
    # two checks broken at once: the earlier one of the header's list answers
    ('W', (0, -1, None, NAN, None, 0, 8), -1, 'cost fields: n_fields 0 outside [1, 64]'),
    ('W', (1, -1, None, NAN, None, 0, 8), -1, 'cost fields: negative source count -1'),
    ('W', (1, 1, None, NAN, None, 0, 8), -1, 'cost fields: NULL source array'),
    ('W', (1, 1, B, NAN, None, 0, 8), -1, 'cost fields: t is NaN'),
    ('W', (1, 1, B, 0.0, None, 0, 8), -1, 'cost fields: NULL bands'),
    ('W', (1, 1, B, 0.0, Bands(5, (NAN, 9)), 0, 8), -1, 'cost fields: n_bands 5 outside [0, 4]'),
    ('W', (1, 1, B, 0.0, Bands(2, (0.5, 9), (NAN, 1)), 0, 8), -1, 'cost fields: clearance[1] = nan is NaN, infinite or not positive'),
    ('W', (1, 1, B, 0.0, Bands(2, (0.5, 7), (0.5, 9)), 0, 8), -1, 'cost fields: penalty[1] = 9 outside [0, 7]'),
    ('W', (1, 1, B, 0.0, Bands(2, (0.5, 7), (0.5, 7)), 0, 8), -1,
     'cost fields: the largest weight 1 + sum of penalty = 15 exceeds DSPMAP_COST_MAX_WEIGHT = 8'),
    ('W', (1, 1, B, 0.0, Bands(2, (0.5, 7), (0.5, 0)), 0, 8), -1, 'cost fields: max_cost 0 outside [1, 16384]'),
    ('S', (1, 1, B, 0.0, ONE, 5, 8), -1, 'cost fields: unknown flags 0x8'),
    ('G', (64, 1, B, 0.0, ONE, 5, 8), -1, 'cost fields: unknown flags 0x8'),
    ('S', (64, 1, B, 0.0, ONE, 16384, 1), -3, 'cost fields: a slab handle holds part of the map; a wavefront crosses slabs'),
]
# (n, start, max_len, flags, cost_out, cells_out): both path entry points
PATHS = [
    ('W', (-1, B, 8, 0, B, B), -1, 'cost paths: negative start count -1'),
    ('W', (4, B, -1, 0, B, B), -1, 'cost paths: max_len -1 outside [0, 4097]'),
    ('W', (4, B, 4098, 0, B, B), -1, 'cost paths: max_len 4098 outside [0, 4097]'),
    ('W', (4, None, 8, 0, B, B), -1, 'cost paths: NULL start or cost_out array'),
    ('W', (4, B, 8, 0, None, B), -1, 'cost paths: NULL start or cost_out array'),
    ('W', (4, B, 8, 0, B, None), -1, 'cost paths: NULL cells_out array with max_len 8'),
    ('W', (4, B, 8, 2, B, B), -1, 'cost paths: unknown flags 0x2'),
    ('W', (2000000, B, 4097, 0, B, B), -1, 'cost paths: 2000000 paths of 4097 cells exceed 2^31 cells'),
    ('S', (4, B, 8, 0, B, B), -3, 'dspmap_cost_paths: a slab handle holds part of the map; a wavefront crosses slabs'),
    ('W', (4, B, 8, 1, B, B), -3, NO_COST % 'dspmap_cost_paths'),
    ('W', (4, B, 0, 0, B, None), -3, NO_COST % 'dspmap_cost_paths'),
    ('W', (0, None, 4097, 0, None, None), -3, NO_COST % 'dspmap_cost_paths'),
    ('W', (-1, None, -1, 8, None, None), -1, 'cost paths: negative start count -1'),
    ('W', (4, None, -1, 8, None, None), -1, 'cost paths: max_len -1 outside [0, 4097]'),
    ('W', (4, None, 8, 8, None, None), -1, 'cost paths: NULL start or cost_out array'),
    ('W', (4, B, 8, 8, B, None), -1, 'cost paths: NULL cells_out array with max_len 8'),
    ('S', (4, B, 8, 8, B, B), -1, 'cost paths: unknown flags 0x8'),
    ('S', (2000000, B, 4097, 0, B, B), -1, 'cost paths: 2000000 paths of 4097 cells exceed 2^31 cells'),
]
CASES = ([(k, fn, a, rc, t) for fn in ("dspmap_build_cost_fields", "dspmap_build_cost_fields_device") for k, a, rc, t in BUILD]
         + [(k, fn, a, rc, t) for fn in ("dspmap_cost_paths", "dspmap_cost_paths_device") for k, a, rc, t in PATHS] + [
    # dspmap_get_cost_field
    ('W', 'dspmap_get_cost_field', (0, None), -1, 'cost field: NULL output array'),
    ('W', 'dspmap_get_cost_field', (-1, B), -1, 'cost field: field -1 outside [0, 64)'),
    ('W', 'dspmap_get_cost_field', (64, B), -1, 'cost field: field 64 outside [0, 64)'),
    ('W', 'dspmap_get_cost_field', (0, B), -3, NO_COST % 'dspmap_get_cost_field'),
    ('W', 'dspmap_get_cost_field', (63, B), -3, NO_COST % 'dspmap_get_cost_field'),
    ('S', 'dspmap_get_cost_field', (0, B), -3, 'dspmap_get_cost_field: a slab handle holds part of the map; a wavefront crosses slabs'),
    ('S', 'dspmap_get_cost_field', (64, None), -1, 'cost field: NULL output array'),
    ('S', 'dspmap_get_cost_field', (64, B), -1, 'cost field: field 64 outside [0, 64)'),
    # dspmap_get_cost_weights
    ('W', 'dspmap_get_cost_weights', (None,), -1, 'cost weights: NULL output array'),
    ('W', 'dspmap_get_cost_weights', (B,), -3, NO_COST % 'dspmap_get_cost_weights'),
    ('S', 'dspmap_get_cost_weights', (B,), -3, 'dspmap_get_cost_weights: a slab handle holds part of the map; a wavefront crosses slabs'),
    ('S', 'dspmap_get_cost_weights', (None,), -1, 'cost weights: NULL output array'),
])


def test_cost_errors_text_for_text(dsp):
    L = dsp.load_library()
    maps = {k: dsp.DSPMap(dsp.make_config(**kw)) for k, kw in HANDLES.items()}
    seen = set()
    for kind, fn, args, rc, text in CASES:
        h = maps[kind].h
        call = [_arg(a, dsp.capi) for a in args]
        got = getattr(L, fn)(h, *call)
        assert (got, L.dspmap_last_error(h).decode()) == (rc, text), (kind, fn, args)
        if fn not in seen:                      # a NULL handle: DSPMAP_E_ARG from every entry point, before anything else
            assert getattr(L, fn)(None, *call) == E_ARG, fn
            seen.add(fn)
    assert not _ZERO.any()                      # no call wrote into its output array
    for m in maps.values():
        assert L.dspmap_cost_fields_device(m.h) is None and L.dspmap_cost_weights_device(m.h) is None and m.cost_fields_ptr() is None
        m.close()
    assert L.dspmap_cost_fields_device(None) is None and L.dspmap_cost_weights_device(None) is None


def test_cost_error_table_covers_the_entry_points(dsp):
    names = {c[1] for c in CASES}
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for fn in names:
        assert fn in dsp.capi.SIGNATURES and "%s(dspmap_t* m" % fn in hdr, fn
    assert names == {"dspmap_build_cost_fields", "dspmap_build_cost_fields_device", "dspmap_cost_paths", "dspmap_cost_paths_device",
                     "dspmap_get_cost_field", "dspmap_get_cost_weights"}
    assert {c[3] for c in CASES} == {E_ARG, E_STATE}


def test_set_distance_field_errors(dsp):
    """the hook: NULL and a value that is NaN, negative or infinite are argument errors -- the values before the state --, a slab and a
    missing field state errors"""
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h).decode()   # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    good = np.full((m.T + 1, 10, 20, 20), 0.5, np.float32)
    assert L.dspmap_debug_set_distance_field(None, p(good)) == E_ARG
    assert L.dspmap_debug_set_distance_field(h, None) == E_ARG and err() == "set distance field: NULL layer array"
    for bad, shown in ((NAN, "nan"), (-0.25, "-0.25"), (INF, "inf"), (-INF, "-inf")):
        a = good.copy()
        a[m.T, 9, 19, 19] = bad
        assert L.dspmap_debug_set_distance_field(h, p(a)) == E_ARG
        assert err() == "set distance field: value %d = %s is NaN, negative or infinite" % (a.size - 1, shown)
    assert L.dspmap_debug_set_distance_field(h, p(good)) == E_STATE
    assert err() == "dspmap_debug_set_distance_field: no distance field, or the map has changed since it was built (dspmap_build_distance_field)"
    with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_distance_field"):
        m.set_distance_field(good)
    m.close()
    s = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    z = np.zeros((s.T + 1, 6, 16, 16), np.float32)
    assert L.dspmap_debug_set_distance_field(s.h, p(z)) == E_STATE and b"slab" in L.dspmap_last_error(s.h)
    z[0, 0, 0, 0] = NAN
    assert L.dspmap_debug_set_distance_field(s.h, p(z)) == E_ARG                 # the argument checks come first
    s.close()


def test_cost_valid_build_needs_device(dsp):
    """a valid call is a grid and a build: without a device the grid's build is DSPMAP_E_DEVICE ("no HIP device") and the cost build finds
    no grid (no CPU fallback)"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    have = torch.cuda.is_available()
    assert L.dspmap_build_cast_grid(m.h, 0.5, 0, 0) == (OK if have else E_DEVICE)
    if not have:
        assert b"no HIP device" in L.dspmap_last_error(m.h)
    src = R.points([(0.0, 0.0, 0.0, 0)])
    bands = dsp.capi.CostBands()
    rc = L.dspmap_build_cost_fields(m.h, 1, 1, src.ctypes.data_as(C.c_void_p), -1.0, C.cast(C.pointer(bands), C.c_void_p), 5, 0)
    assert rc == (OK if have else E_STATE)
    if have:
        val = m.cost_field(0)
        want = K.fields(m.cfg, K.weights(np.zeros((10, 20, 20), bool), None, []), src, 1, max_cost=5)[0]
        assert val[5, 10, 10] == 0 and np.array_equal(val, want) and (val == 5).any()
    else:
        assert b"dspmap_build_cast_grid" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_cast_grid"):
            m.build_cost_fields(src)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_cost_fields"):
            m.cost_field(0)
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_cost_fields"):
            m.cost_weights()
        with pytest.raises(dsp.capi.DSPMapError, match="dspmap_build_cost_fields"):
            m.cost_paths(src, 4)
        assert m.cost_fields_ptr() is None
    m.close()
