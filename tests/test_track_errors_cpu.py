"""The errors of the tracking extension (dspmap_track_update and its accessors) that fire before the device is touched, text for text, in
the table form of tests/test_objects_errors_cpu.py: (handle, entry point, arguments behind the handle, return code, rendered
dspmap_last_error).  The order is pinned -- arguments, then the slab, then the missing build of objects; accessors: arguments, then the
missing update -- by calls that break two checks at once, at least one per entry point.  Nothing here reaches a device."""
import os

from tests.test_layer_errors_cpu import B, E_ARG, E_STATE, HANDLES, INF, NAN, _ZERO, _arg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = "dspmap_track_update"
NO_BUILD = U + ": no objects, or the map or its cast grid has changed since they were built (dspmap_build_objects)"
SLAB = U + ": a slab handle holds part of the map; components cross slabs"
NO_UPDATE = "%s: no tracks: no update since the handle was created, reset or given a new state (dspmap_track_update)"
DT = U + ": dt %s is NaN, negative or infinite"

CASES = [
    # dspmap_track_update(dt, min_overlap, max_shift, max_pairs, flags)
    ('W', U, (NAN, 1, 8, 0, 0), -1, DT % 'nan'),
    ('W', U, (-1.0, 1, 8, 0, 0), -1, DT % '-1'),
    ('W', U, (INF, 1, 8, 0, 0), -1, DT % 'inf'),
    ('W', U, (-INF, 1, 8, 0, 0), -1, DT % '-inf'),
    ('W', U, (0.1, 0, 8, 0, 0), -1, U + ': min_overlap 0 below 1'),
    ('W', U, (0.1, -4, 8, 0, 0), -1, U + ': min_overlap -4 below 1'),
    ('W', U, (0.1, 1, -1, 0, 0), -1, U + ': max_shift -1 outside [0, 64]'),
    ('W', U, (0.1, 1, 65, 0, 0), -1, U + ': max_shift 65 outside [0, 64]'),
    ('W', U, (0.1, 1, 8, -1, 0), -1, U + ': negative max_pairs -1'),
    ('W', U, (0.1, 1, 8, 0, 2), -1, U + ': unknown flags 0x2'),
    ('W', U, (0.1, 1, 8, 0, 3), -1, U + ': unknown flags 0x3'),
    ('W', U, (0.1, 1, 8, 0, -1), -1, U + ': unknown flags 0xffffffff'),
    ('S', U, (0.1, 1, 8, 0, 0), -3, SLAB),
    ('W', U, (0.1, 1, 8, 0, 0), -3, NO_BUILD),
    ('W', U, (0.0, 1 << 30, 0, 1 << 30, 1), -3, NO_BUILD),
    ('W', U, (1.0e30, 1, 64, 1, 0), -3, NO_BUILD),
    # ... two checks broken at once: the earlier one speaks
    ('W', U, (NAN, 0, 65, -1, 2), -1, DT % 'nan'),
    ('W', U, (0.1, 0, 65, -1, 2), -1, U + ': min_overlap 0 below 1'),
    ('W', U, (0.1, 1, 65, -1, 2), -1, U + ': max_shift 65 outside [0, 64]'),
    ('W', U, (0.1, 1, 64, -1, 2), -1, U + ': negative max_pairs -1'),
    ('S', U, (0.1, 1, 8, 0, 2), -1, U + ': unknown flags 0x2'),
    ('S', U, (NAN, 1, 8, 0, 0), -1, DT % 'nan'),
    ('S', U, (0.0, 1, 0, 0, 1), -3, SLAB),                                 # a slab has no objects either: the slab speaks
    # dspmap_track_counts(out)
    ('W', 'dspmap_track_counts', (None,), -1, 'dspmap_track_counts: NULL output array'),
    ('W', 'dspmap_track_counts', (B,), -3, NO_UPDATE % 'dspmap_track_counts'),
    ('S', 'dspmap_track_counts', (None,), -1, 'dspmap_track_counts: NULL output array'),   # NULL and no update: the argument speaks
    ('S', 'dspmap_track_counts', (B,), -3, NO_UPDATE % 'dspmap_track_counts'),
    # dspmap_get_tracks(cap, out, n_out)
    ('W', 'dspmap_get_tracks', (-1, B, B), -1, 'dspmap_get_tracks: negative capacity -1'),
    ('W', 'dspmap_get_tracks', (8, None, B), -1, 'dspmap_get_tracks: NULL output'),
    ('W', 'dspmap_get_tracks', (8, B, None), -1, 'dspmap_get_tracks: NULL output'),
    ('W', 'dspmap_get_tracks', (0, None, None), -1, 'dspmap_get_tracks: NULL output'),
    ('W', 'dspmap_get_tracks', (8, B, B), -3, NO_UPDATE % 'dspmap_get_tracks'),
    ('W', 'dspmap_get_tracks', (0, None, B), -3, NO_UPDATE % 'dspmap_get_tracks'),
    ('W', 'dspmap_get_tracks', (-1, None, None), -1, 'dspmap_get_tracks: negative capacity -1'),
    ('S', 'dspmap_get_tracks', (8, B, B), -3, NO_UPDATE % 'dspmap_get_tracks'),
    ('S', 'dspmap_get_tracks', (-2, None, B), -1, 'dspmap_get_tracks: negative capacity -2'),
]
DEVICE_ACCESSORS = ["dspmap_tracks_device", "dspmap_track_counts_device"]
RESET = "dspmap_track_reset"


def test_track_errors_text_for_text(dsp):
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
    for fn in DEVICE_ACCESSORS:                 # no update: NULL, also for a NULL handle
        for m in maps.values():
            assert not getattr(L, fn)(m.h)
        assert not getattr(L, fn)(None)
    # a reset of a handle that never tracked has nothing to forget and touches no device: fine on both handles, and still no tracks
    assert getattr(L, RESET)(None) == E_ARG
    for m in maps.values():
        assert getattr(L, RESET)(m.h) == 1
        assert L.dspmap_track_counts(m.h, _arg(B)) == E_STATE and not L.dspmap_tracks_device(m.h)
    for m in maps.values():
        m.close()


def test_track_error_table_covers_the_entry_points(dsp):
    """every entry point of the section is declared, bound and in the table with a call that breaks two checks"""
    names = {c[1] for c in CASES}
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    assert names | set(DEVICE_ACCESSORS) | {RESET} == {n for n in dsp.capi.SIGNATURES if "track" in n}
    for fn in names | set(DEVICE_ACCESSORS) | {RESET}:
        assert "%s(dspmap_t* m" % fn in hdr, fn
        assert "object" not in fn
    assert {c[3] for c in CASES} == {E_ARG, E_STATE}
    for fn in names:
        assert {k for k, f, *_ in CASES if f == fn} == {"W", "S"}, fn


def test_python_surface_raises_without_an_update(dsp):
    import pytest
    m = dsp.DSPMap(dsp.make_config(**HANDLES["W"]))
    for call in (lambda: m.update_tracks(0.1), lambda: m.update_tracks(-1.0), lambda: m.update_tracks(0.1, max_shift=65), m.track_counts, m.tracks,
                 lambda: m.tracks(device="cuda")):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.reset_tracks()
    m.close()
