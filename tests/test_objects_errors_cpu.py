"""The errors of the objects extension (dspmap_build_objects, its accessors and queries) that fire before the device is touched, text for
text, in the table form of tests/test_layer_errors_cpu.py: (handle, entry point, arguments behind the handle, return code, rendered
dspmap_last_error).  The order is pinned -- arguments, then the slab, then the missing cast grid; accessors and queries: arguments, then the
missing build -- by calls that break two checks at once, at least one per entry point.  Nothing here reaches a device."""
import ctypes as C
import os

from tests.test_layer_errors_cpu import B, E_ARG, E_STATE, HANDLES, INF, NAN, _ZERO, _arg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GRID = "dspmap_build_objects: no cast grid, or the map has changed since it was built (dspmap_build_cast_grid)"
SLAB = "dspmap_build_objects: a slab handle holds part of the map; components cross slabs"
NO_BUILD = "%s: no objects, or the map or its cast grid has changed since they were built (dspmap_build_objects)"

CASES = [
    # dspmap_build_objects(t, connectivity, min_cells, max_objects, flags)
    ('W', 'dspmap_build_objects', (NAN, 26, 1, 64, 0), -1, 'dspmap_build_objects: t is NaN'),
    ('W', 'dspmap_build_objects', (-1.0, 18, 1, 64, 0), -1, 'dspmap_build_objects: connectivity 18 is neither 6 nor 26'),
    ('W', 'dspmap_build_objects', (-1.0, 0, 1, 64, 0), -1, 'dspmap_build_objects: connectivity 0 is neither 6 nor 26'),
    ('W', 'dspmap_build_objects', (-1.0, 6, 0, 64, 0), -1, 'dspmap_build_objects: min_cells 0 below 1'),
    ('W', 'dspmap_build_objects', (-1.0, 6, -3, 64, 0), -1, 'dspmap_build_objects: min_cells -3 below 1'),
    ('W', 'dspmap_build_objects', (-1.0, 6, 1, 0, 0), -1, 'dspmap_build_objects: max_objects 0 outside [1, 1048576]'),
    ('W', 'dspmap_build_objects', (-1.0, 6, 1, 1048577, 0), -1, 'dspmap_build_objects: max_objects 1048577 outside [1, 1048576]'),
    ('W', 'dspmap_build_objects', (-1.0, 26, 1, 64, 1), -1, 'dspmap_build_objects: unknown flags 0x1'),
    ('W', 'dspmap_build_objects', (-1.0, 26, 1, 64, -1), -1, 'dspmap_build_objects: unknown flags 0xffffffff'),
    ('S', 'dspmap_build_objects', (-1.0, 26, 1, 64, 0), -3, SLAB),
    ('W', 'dspmap_build_objects', (-1.0, 26, 1, 64, 0), -3, NO_GRID),
    ('W', 'dspmap_build_objects', (INF, 6, 1 << 30, 1 << 20, 0), -3, NO_GRID),
    ('W', 'dspmap_build_objects', (0.3, 6, 1, 1, 0), -3, NO_GRID),
    # ... two checks broken at once: the earlier one speaks
    ('W', 'dspmap_build_objects', (NAN, 7, 0, 0, 1), -1, 'dspmap_build_objects: t is NaN'),
    ('W', 'dspmap_build_objects', (0.5, 7, 0, 0, 1), -1, 'dspmap_build_objects: connectivity 7 is neither 6 nor 26'),
    ('W', 'dspmap_build_objects', (0.5, 26, 0, 0, 1), -1, 'dspmap_build_objects: min_cells 0 below 1'),
    ('W', 'dspmap_build_objects', (0.5, 26, 1, 0, 1), -1, 'dspmap_build_objects: max_objects 0 outside [1, 1048576]'),
    ('S', 'dspmap_build_objects', (0.5, 26, 1, 64, 1), -1, 'dspmap_build_objects: unknown flags 0x1'),
    ('S', 'dspmap_build_objects', (NAN, 26, 1, 64, 0), -1, 'dspmap_build_objects: t is NaN'),
    ('S', 'dspmap_build_objects', (INF, 6, 4, 1, 0), -3, SLAB),                      # a slab has no grid either: the slab speaks
    # dspmap_object_counts(out)
    ('W', 'dspmap_object_counts', (None,), -1, 'dspmap_object_counts: NULL output array'),
    ('W', 'dspmap_object_counts', (B,), -3, NO_BUILD % 'dspmap_object_counts'),
    ('S', 'dspmap_object_counts', (None,), -1, 'dspmap_object_counts: NULL output array'),   # NULL and no build: the argument speaks
    ('S', 'dspmap_object_counts', (B,), -3, NO_BUILD % 'dspmap_object_counts'),
    # dspmap_get_objects(cap, out, n_out)
    ('W', 'dspmap_get_objects', (-1, B, B), -1, 'dspmap_get_objects: negative capacity -1'),
    ('W', 'dspmap_get_objects', (8, None, B), -1, 'dspmap_get_objects: NULL output'),
    ('W', 'dspmap_get_objects', (8, B, None), -1, 'dspmap_get_objects: NULL output'),
    ('W', 'dspmap_get_objects', (0, None, None), -1, 'dspmap_get_objects: NULL output'),
    ('W', 'dspmap_get_objects', (8, B, B), -3, NO_BUILD % 'dspmap_get_objects'),
    ('W', 'dspmap_get_objects', (0, None, B), -3, NO_BUILD % 'dspmap_get_objects'),
    ('W', 'dspmap_get_objects', (-1, None, None), -1, 'dspmap_get_objects: negative capacity -1'),
    ('S', 'dspmap_get_objects', (8, B, B), -3, NO_BUILD % 'dspmap_get_objects'),
    # dspmap_get_object_labels(out)
    ('W', 'dspmap_get_object_labels', (None,), -1, 'dspmap_get_object_labels: NULL output array'),
    ('W', 'dspmap_get_object_labels', (B,), -3, NO_BUILD % 'dspmap_get_object_labels'),
    ('S', 'dspmap_get_object_labels', (None,), -1, 'dspmap_get_object_labels: NULL output array'),
    ('S', 'dspmap_get_object_labels', (B,), -3, NO_BUILD % 'dspmap_get_object_labels'),
]
# dspmap_query_objects / _device (n, q, flags, ordinal_out): the two variants reject the same calls with the same words
for _fn in ('dspmap_query_objects', 'dspmap_query_objects_device'):
    CASES += [
        ('W', _fn, (-1, B, 0, B), -1, 'objects query: negative sample count -1'),
        ('W', _fn, (4, None, 0, B), -1, 'objects query: NULL sample or output array'),
        ('W', _fn, (4, B, 0, None), -1, 'objects query: NULL sample or output array'),
        ('W', _fn, (4, B, 2, B), -1, 'objects query: unknown flags 0x2'),
        ('W', _fn, (4, B, 0, B), -3, NO_BUILD % 'dspmap_query_objects'),
        ('W', _fn, (4, B, 1, B), -3, NO_BUILD % 'dspmap_query_objects'),
        ('W', _fn, (0, None, 0, None), -3, NO_BUILD % 'dspmap_query_objects'),
        ('W', _fn, (-7, None, 8, None), -1, 'objects query: negative sample count -7'),
        ('W', _fn, (4, None, 8, B), -1, 'objects query: NULL sample or output array'),
        ('W', _fn, (4, B, 8, B), -1, 'objects query: unknown flags 0x8'),
        ('S', _fn, (4, B, 0, B), -3, NO_BUILD % 'dspmap_query_objects'),
    ]
DEVICE_ACCESSORS = ["dspmap_objects_device", "dspmap_object_labels_device", "dspmap_object_counts_device"]


def test_object_errors_text_for_text(dsp):
    L = dsp.load_library()
    maps = {k: dsp.DSPMap(dsp.make_config(**HANDLES[k])) for k in ("W", "S")}
    seen = set()
    for kind, fn, args, rc, text in CASES:
        h = maps[kind].h
        call = [_arg(a) for a in args]
        got = getattr(L, fn)(h, *call)
        assert (got, L.dspmap_last_error(h).decode()) == (rc, text), (kind, fn, args)
        if fn not in seen:                      # a NULL handle: DSPMAP_E_ARG from every entry point, before anything else
            assert getattr(L, fn)(None, *call) == E_ARG, fn
            seen.add(fn)
    assert not _ZERO.any()                      # no call wrote into its output array
    for fn in DEVICE_ACCESSORS:                 # no build: NULL, also for a NULL handle
        for m in maps.values():
            assert not getattr(L, fn)(m.h)
        assert not getattr(L, fn)(None)
    for m in maps.values():
        m.close()


def test_object_error_table_covers_the_entry_points(dsp):
    """every entry point of the section is declared, bound and in the table with a call that breaks two checks; host and _device query
    reject identically"""
    names = {c[1] for c in CASES}
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    assert names | set(DEVICE_ACCESSORS) == {n for n in dsp.capi.SIGNATURES if "object" in n}
    for fn in names | set(DEVICE_ACCESSORS):
        assert "%s(dspmap_t* m" % fn in hdr, fn
    host = [(c[0], c[2], c[3], c[4]) for c in CASES if c[1] == "dspmap_query_objects"]
    dev = [(c[0], c[2], c[3], c[4]) for c in CASES if c[1] == "dspmap_query_objects_device"]
    assert host == dev and len(host) >= 10
    assert {c[3] for c in CASES} == {E_ARG, E_STATE}


def test_python_surface_raises_without_a_build(dsp):
    import numpy as np
    import pytest
    m = dsp.DSPMap(dsp.make_config(**HANDLES["W"]))
    for call in (m.build_objects, lambda: m.build_objects(connectivity=18), m.object_counts, m.objects, m.object_labels,
                 lambda: m.query_objects(np.zeros((2, 4), np.float32))):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    with pytest.raises(ValueError):
        m.query_objects(np.zeros((2, 3), np.float32))
    m.close()
