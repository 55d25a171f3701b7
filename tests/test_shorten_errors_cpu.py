"""The errors of dspmap_shorten_paths and dspmap_shorten_paths_device that fire before the device is touched, text for text, in the table
form of tests/test_track_errors_cpu.py: (handle, arguments behind the handle, return code, rendered dspmap_last_error), the same table for
both entry points.  The order is pinned -- the arguments in the order include/dspmap.h lists them, then the slab, then the missing cast
grid -- by calls that break two checks at once.  Nothing here reaches a device."""
import os

from tests.test_layer_errors_cpu import B, E_ARG, E_STATE, HANDLES, INF, NAN, _ZERO, _arg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("dspmap_shorten_paths", "dspmap_shorten_paths_device")
P = "shorten paths: "
NO_GRID = "dspmap_shorten_paths: no cast grid, or the map has changed since it was built (dspmap_build_cast_grid)"
SLAB = P + "a slab handle holds part of the map; casts cross slabs"
DT = P + "step_seconds %s is NaN, negative or infinite"
NULL_IN = P + "NULL steps, cells or info array"
NULL_OUT = P + "NULL seg_out or end_out array with max_seg %d"

CASES = [
    # (n, max_len, steps, cells, t_start, step_seconds, window, max_seg, flags, info_out, seg_out, end_out)
    ('W', (-1, 8, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, P + 'negative path count -1'),
    ('W', (4, 0, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, P + 'max_len 0 outside [1, 4097]'),
    ('W', (4, -3, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, P + 'max_len -3 outside [1, 4097]'),
    ('W', (4, 4098, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, P + 'max_len 4098 outside [1, 4097]'),
    ('W', (4, 8, B, B, -1.0, 0.0, 0, 7, 0, B, B, B), -1, P + 'window 0 outside [1, 64]'),
    ('W', (4, 8, B, B, -1.0, 0.0, -1, 7, 0, B, B, B), -1, P + 'window -1 outside [1, 64]'),
    ('W', (4, 8, B, B, -1.0, 0.0, 65, 7, 0, B, B, B), -1, P + 'window 65 outside [1, 64]'),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, -1, 0, B, B, B), -1, P + 'negative max_seg -1'),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 1, B, B, B), -1, P + 'unknown flags 0x1'),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 2, B, B, B), -1, P + 'unknown flags 0x2'),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, -1, B, B, B), -1, P + 'unknown flags 0xffffffff'),
    ('W', (4, 8, B, B, NAN, 0.0, 64, 7, 0, B, B, B), -1, P + 't_start is NaN'),
    ('W', (4, 8, B, B, 0.0, NAN, 64, 7, 0, B, B, B), -1, DT % 'nan'),
    ('W', (4, 8, B, B, 0.0, -0.5, 64, 7, 0, B, B, B), -1, DT % '-0.5'),
    ('W', (4, 8, B, B, 0.0, INF, 64, 7, 0, B, B, B), -1, DT % 'inf'),
    ('W', (4, 8, B, B, 0.0, -INF, 64, 7, 0, B, B, B), -1, DT % '-inf'),
    ('W', (4, 8, None, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, NULL_IN),
    ('W', (4, 8, B, None, -1.0, 0.0, 64, 7, 0, B, B, B), -1, NULL_IN),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 0, None, B, B), -1, NULL_IN),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 0, B, None, B), -1, NULL_OUT % 7),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 0, B, B, None), -1, NULL_OUT % 7),
    ('W', (1048576, 4097, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -1, P + '1048576 paths of 4097 cells exceed 2^31 cells'),
    ('W', (1048576, 1, B, B, -1.0, 0.0, 64, 4097, 0, B, B, B), -1, P + '1048576 paths of 4097 segments exceed 2^31 segments'),
    # ... valid arguments reach the state checks: the slab first, then the grid no handle here has
    ('S', (4, 8, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -3, SLAB),
    ('W', (4, 8, B, B, -1.0, 0.0, 64, 7, 0, B, B, B), -3, NO_GRID),
    ('W', (4, 8, B, B, INF, 0.0, 1, 7, 0, B, B, B), -3, NO_GRID),
    ('W', (4, 8, B, B, -INF, 1.0e30, 1, 0, 0, B, None, None), -3, NO_GRID),          # max_seg == 0: no segment arrays needed
    ('W', (0, 1, None, None, 0.0, 0.0, 64, 0, 0, None, None, None), -3, NO_GRID),   # n == 0: no arrays needed
    ('W', (0, 4097, None, None, 0.0, 0.0, 64, 1 << 30, 0, None, None, None), -3, NO_GRID),
    ('W', (524288, 4096, B, B, 0.0, 0.0, 64, 4096, 0, B, B, B), -3, NO_GRID),       # exactly 2^31 cells and segments
    ('S', (0, 1, None, None, 0.0, 0.0, 64, 0, 0, None, None, None), -3, SLAB),
    # ... two checks broken at once: the earlier one speaks
    ('W', (-1, 0, None, None, NAN, NAN, 0, -1, 1, None, None, None), -1, P + 'negative path count -1'),
    ('W', (4, 0, None, None, NAN, NAN, 0, -1, 1, None, None, None), -1, P + 'max_len 0 outside [1, 4097]'),
    ('W', (4, 8, None, None, NAN, NAN, 0, -1, 1, None, None, None), -1, P + 'window 0 outside [1, 64]'),
    ('W', (4, 8, None, None, NAN, NAN, 64, -1, 1, None, None, None), -1, P + 'negative max_seg -1'),
    ('W', (4, 8, None, None, NAN, NAN, 64, 7, 1, None, None, None), -1, P + 'unknown flags 0x1'),
    ('W', (4, 8, None, None, NAN, NAN, 64, 7, 0, None, None, None), -1, P + 't_start is NaN'),
    ('W', (4, 8, None, None, 0.0, NAN, 64, 7, 0, None, None, None), -1, DT % 'nan'),
    ('W', (4, 8, None, None, 0.0, 0.0, 64, 7, 0, None, None, None), -1, NULL_IN),
    ('W', (1048576, 4097, B, B, 0.0, 0.0, 64, 4097, 0, B, None, None), -1, NULL_OUT % 4097),
    ('W', (1048576, 4097, B, B, 0.0, 0.0, 64, 4097, 0, B, B, B), -1, P + '1048576 paths of 4097 cells exceed 2^31 cells'),
    ('S', (4, 8, B, B, -1.0, 0.0, 64, 7, 4, B, B, B), -1, P + 'unknown flags 0x4'),
    ('S', (4, 8, B, B, -1.0, -1.0, 64, 7, 0, B, B, B), -1, DT % '-1'),
    ('S', (1048576, 1, B, B, -1.0, 0.0, 64, 4097, 0, B, B, B), -1, P + '1048576 paths of 4097 segments exceed 2^31 segments'),
]


def test_shorten_errors_text_for_text(dsp):
    L = dsp.load_library()
    maps = {k: dsp.DSPMap(dsp.make_config(**HANDLES[k])) for k in ("W", "S")}
    for fn in FNS:
        for kind, args, rc, text in CASES:
            h = maps[kind].h
            call = [_arg(a) for a in args]
            got = getattr(L, fn)(h, *call)
            assert (got, L.dspmap_last_error(h).decode()) == (rc, text), (fn, kind, args)
        assert getattr(L, fn)(None, *[_arg(a) for a in CASES[0][1]]) == E_ARG      # a NULL handle: before anything else
        assert getattr(L, fn)(None, *[_arg(a) for a in CASES[24][1]]) == E_ARG
    assert not _ZERO.any()                          # no call wrote into its output arrays
    for m in maps.values():
        m.close()


def test_shorten_error_table_covers_the_contract(dsp):
    """both entry points are declared and bound, every check of the header's list has a case that fires it alone and one in which it
    speaks before a later one, and both handles see argument and state errors"""
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for fn in FNS:
        assert fn in dsp.capi.SIGNATURES and "%s(dspmap_t* m" % fn in hdr, fn
    assert {n for n in dsp.capi.SIGNATURES if "shorten" in n} == set(FNS)
    assert {c[2] for c in CASES} == {E_ARG, E_STATE}
    texts = [c[3] for c in CASES]
    for key in ("negative path count", "max_len", "window", "negative max_seg", "unknown flags", "t_start is NaN", "step_seconds",
                "NULL steps, cells or info", "NULL seg_out or end_out", "cells exceed 2^31", "segments exceed 2^31", "slab", "dspmap_build_cast_grid"):
        assert sum(key in t for t in texts) >= 2, key
    assert CASES[24][2] == E_STATE and {k for k, *_ in CASES} == {"W", "S"}


def test_python_surface_raises_without_a_grid(dsp):
    import numpy as np
    import pytest
    m = dsp.DSPMap(dsp.make_config(**HANDLES["W"]))
    steps, cells = np.zeros(3, np.int32), np.zeros((3, 5), np.int32)
    for call in (lambda: m.shorten_paths(steps, cells), lambda: m.shorten_paths(steps, cells, window=0),
                 lambda: m.shorten_paths(steps, cells, window=65), lambda: m.shorten_paths(steps, cells, max_seg=-1),
                 lambda: m.shorten_paths(steps, cells, step_seconds=-1.0), lambda: m.shorten_paths(steps[:0], cells[:0])):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    with pytest.raises(ValueError):
        m.shorten_paths(steps, cells[:2])
    m.close()
