"""GPU tests of the depth-image ingest: dspmap_preprocess_depth bit for bit against the numpy restatement (tests/depth_ref.py) over
formats, strides, pixel steps, caps and leaf sizes; the same bits on every run, handle and stream; the old cloud path as the
cross-check; and whole frames from images (dspmap_update_depth, dspmap_update_depth_device) against frames fed the restatement's cloud."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests import depth_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
B = dict(nx=66, ny=66, nz=40, res=0.15, ppv=24)


def _dev(img):
    """the image's bytes on the GPU (uint16 travels as its int16 bits)"""
    a = np.ascontiguousarray(img)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).cuda()


def _ingest_raw(m, cam, d_img, max_points, leaf):
    """through the C ABI on raw pointers (padded rows are a byte buffer): -> (points, n_leaves, n_valid)"""
    out = torch.full((max(max_points, 1), 3), -77.0, dtype=torch.float32, device="cuda")
    n, nl, nv = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    rc = m.L.dspmap_preprocess_depth(m.h, C.byref(cam), d_img.data_ptr(), leaf, max_points, out.data_ptr(), C.byref(n), C.byref(nl), C.byref(nv))
    assert rc == 1, m.L.dspmap_last_error(m.h)
    got = out.cpu().numpy()
    assert np.all(got[n.value:] == F(-77.0))   # nothing written past n_out
    return got[:n.value].copy(), nl.value, nv.value


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


CASES = [
    ("u16_mm_packed", dict(), "u16", 5000, 0.1),
    ("u16_cap_100000", dict(), "u16", 100000, 0.1),
    ("u16_cap_7", dict(), "u16", 7, 0.1),
    ("u16_leaf_025", dict(), "u16", 100000, 0.25),
    ("u16_leaf_025_cap_7", dict(), "u16", 7, 0.25),
    ("f32_metres_nonreturns", dict(fmt=R.F32, depth_scale=1.0), "f32", 100000, 0.1),
    ("f32_cap_5000", dict(fmt=R.F32, depth_scale=1.0), "f32", 5000, 0.1),
    ("u16_padded_stride", dict(row_stride_bytes=640 * 2 + 64), "u16_pad", 100000, 0.1),
    ("f32_padded_stride", dict(fmt=R.F32, depth_scale=1.0, row_stride_bytes=640 * 4 + 36), "f32_pad", 5000, 0.1),
    ("u16_641x479_step2", dict(width=641, height=479, pixel_step=2), "u16_odd", 100000, 0.1),
    ("u16_641x479_step3", dict(width=641, height=479, pixel_step=3), "u16_odd", 5000, 0.1),
    ("u16_641x479_step3_leaf_025", dict(width=641, height=479, pixel_step=3), "u16_odd", 100000, 0.25),
    ("u16_range_1_to_2p9", dict(min_depth=1.0, max_depth=2.9), "u16", 100000, 0.1),
    ("no_valid_pixel", dict(), "zeros", 5000, 0.1),
    ("all_beyond_max_depth", dict(max_depth=0.5), "u16", 5000, 0.1),
    ("one_pixel", dict(width=1, height=1, cx=0.0, cy=0.0), "one", 5000, 0.1),
]


def _image(kind, kw):
    if kind == "u16":
        return R.make_image()
    if kind == "f32":
        return R.make_image_f32()
    if kind == "u16_pad":
        return R.pad_rows(R.make_image(), kw["row_stride_bytes"])
    if kind == "f32_pad":
        return R.pad_rows(R.make_image_f32(), kw["row_stride_bytes"])
    if kind == "u16_odd":
        return R.make_image(641, 479, seed=11)
    if kind == "zeros":
        return np.zeros((480, 640), np.uint16)
    if kind == "one":
        return np.full((1, 1), 2500, np.uint16)
    raise KeyError(kind)


def test_preprocess_depth_bit_equal_to_the_restatement(dsp):
    """every case: equal n_out, n_leaves, n_valid and zero mismatching float bits"""
    m = dsp.DSPMap(dsp.make_config(**B))
    half = common.half_extent(m.cfg)
    for name, over, kind, cap, leaf in CASES:
        kw = R.camera_kw(**over)
        img = _image(kind, kw)
        cam = dsp.capi.make_camera(**kw)
        ref, n_valid = R.preprocess_depth(img, kw, leaf, half, cap)
        got, nl, nv = _ingest_raw(m, cam, _dev(img), cap, leaf)
        bad = int((got.view(np.uint32) != ref["out"].view(np.uint32)).sum()) if got.shape == ref["out"].shape else -1
        print("%-28s n_out %6d / %6d  leaves %6d / %6d  valid %6d / %6d  mismatching values %d" %
              (name, len(got), len(ref["out"]), nl, ref["n_leaves"], nv, n_valid, bad))
        assert (len(got), nl, nv) == (len(ref["out"]), ref["n_leaves"], n_valid), name
        assert _bits_equal(got, ref["out"]), (name, bad)
        if name in ("no_valid_pixel", "all_beyond_max_depth"):
            assert len(got) == 0 and nl == 0
        if name == "one_pixel":
            assert len(got) == 1 and nv == 1
        if name == "u16_cap_7":
            assert len(got) == 7 and nl > 7
        if name == "u16_cap_100000":
            assert 5000 < len(got) < 100000
    # the binding's method on a tensor: the same cloud
    kw = R.camera_kw()
    ref, n_valid = R.preprocess_depth(R.make_image(), kw, 0.1, half, 5000)
    pts, nl, nv = m.preprocess_depth(dsp.capi.make_camera(**kw), _dev(R.make_image()), max_points=5000, leaf=0.1)
    assert _bits_equal(pts.cpu().numpy(), ref["out"]) and (nl, nv) == (ref["n_leaves"], n_valid)
    m.close()


def test_same_bits_on_every_run_handle_and_stream_and_old_path_as_cross_check(dsp):
    """the same image five times on one handle and once on a second handle that runs on a caller-owned stream: identical bits.  The
    old path (dspmap_preprocess_cloud on the host-back-projected cloud, float atomics): same count and order, centroids within the
    worst-case fp32 summation error computed from the input -- the old path is the inexact one."""
    img = R.make_image()
    kw = R.camera_kw()
    cam = dsp.capi.make_camera(**kw)
    m = dsp.DSPMap(dsp.make_config(**B))
    half = common.half_extent(m.cfg)
    ref, n_valid = R.preprocess_depth(img, kw, 0.1, half, 100000)
    assert R.face_distance(ref["out"], half) >= 1e-3   # (condition for comparing counts with a path that rounds differently)
    d_img = _dev(img)
    runs = [_ingest_raw(m, cam, d_img, 100000, 0.1) for _ in range(5)]
    m2 = dsp.DSPMap(dsp.make_config(**B))
    st = torch.cuda.Stream()
    m2._chk(m2.L.dspmap_set_stream(m2.h, st.cuda_stream))
    runs.append(_ingest_raw(m2, cam, d_img, 100000, 0.1))
    for got, nl, nv in runs:
        assert _bits_equal(got, ref["out"]) and (nl, nv) == (ref["n_leaves"], n_valid)
    d_cloud = torch.from_numpy(ref["cloud"]).cuda()
    d_out = torch.zeros((100000, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n_old, leaves_old = m.preprocess_cloud(d_cloud.data_ptr(), len(ref["cloud"]), d_out.data_ptr(), 100000, leaf=0.1, swap_axes=True)
    old = d_out[:n_old].cpu().numpy()
    assert n_old == len(ref["out"]) and leaves_old == ref["n_leaves"]
    bound = R.oracle_bound(ref)
    diff = float(np.abs(old.astype(np.float64) - ref["out"].astype(np.float64)).max())
    print("old path against the restatement: max |difference| %.3g m (bound %.3g), bit-equal values %d of %d" %
          (diff, bound, int((old.view(np.uint32) == ref["out"].view(np.uint32)).sum()), old.size))
    assert diff <= bound
    m.close(); m2.close()


def _snapshot(m):
    m.sync()
    ints = {k: v for k, v in m.counters().items() if isinstance(v, int)}   # every integer field of dspmap_counters
    v, s, rec = m.export_state()
    return m.results(), m.getFutureStatus(), v, s, rec, ints


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


def _sequence(n):
    """moving camera: (image, position, stamp, quaternion) per frame"""
    out = []
    for f in range(n):
        out.append((R.make_image(seed=100 + f, shift=0.05 * f), (0.03 * f, 0.01 * f, 0.0), f / 30.0, (1.0, 0.0, 0.0, 0.0)))
    return out


def _new_map(dsp, stream=None):
    m = dsp.DSPMap(dsp.make_config(**B))
    m.set_tables(*common.tables(5))
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    if stream is not None:
        m._chk(m.L.dspmap_set_stream(m.h, stream.cuda_stream))
    return m


def test_frames_from_images_equal_frames_from_the_restatements_cloud(dsp):
    """update_depth (host image) and update_depth_device over 12 frames, device velocity estimator on, injected tables, against a third
    handle fed update_device with the restatement's cloud of each frame: results, future status, exported state and every integer
    counter equal bit for bit after every frame; a gated frame (|dp| > 10 m) in the middle returns 0 everywhere and changes nothing."""
    kw = R.camera_kw()
    cam = dsp.capi.make_camera(**kw)
    mh, md, mr = _new_map(dsp), _new_map(dsp), _new_map(dsp)
    half = common.half_extent(mh.cfg)
    live = 0
    for f, (img, pos, t, quat) in enumerate(_sequence(12)):
        if f == 6:   # gated: 11 m in one step
            far = (pos[0] + 11.0, pos[1], pos[2])
            before = [_snapshot(x) for x in (mh, md, mr)]
            d_img = _dev(img)
            torch.cuda.synchronize()
            assert mh.update_depth(cam, img, far, t, quat) == 0
            assert md.update_depth(cam, d_img, far, t, quat) == 0
            assert mr.update_device(d_img.data_ptr(), 0, far, t, quat) == 0
            after = [_snapshot(x) for x in (mh, md, mr)]
            for b, a in zip(before, after):
                assert _same(b, a)
        ref, _ = R.preprocess_depth(img, kw, 0.1, half, 5000)
        d_img = _dev(img)
        d_cloud = torch.from_numpy(ref["out"]).cuda()
        torch.cuda.synchronize()
        assert mh.update_depth(cam, img, pos, t, quat, max_points=5000, leaf=0.1) == 1
        assert md.update_depth(cam, d_img, pos, t, quat, max_points=5000, leaf=0.1) == 1
        assert mr.update_device(d_cloud.data_ptr(), len(ref["out"]), pos, t, quat) == 1
        sh, sd, sr = _snapshot(mh), _snapshot(md), _snapshot(mr)
        assert sr[5]["n_points_in"] == len(ref["out"]) > 1000 and len(sr[5]) == 16
        assert _same(sh, sr), f
        assert _same(sd, sr), f
        live = sr[5]["n_live_out"]
    assert live > 10000   # (n_live_out: the frames did something)
    for x in (mh, md, mr):
        x.close()


def test_depth_frames_on_a_caller_owned_stream(dsp):
    """dspmap_set_stream: depth frames on a caller-owned stream give the same bits as on the library's stream"""
    kw = R.camera_kw()
    cam = dsp.capi.make_camera(**kw)
    st = torch.cuda.Stream()
    ma, mb = _new_map(dsp), _new_map(dsp, stream=st)
    for f, (img, pos, t, quat) in enumerate(_sequence(4)):
        d_img = _dev(img)
        torch.cuda.synchronize()
        assert ma.update_depth(cam, d_img, pos, t, quat) == 1
        with torch.cuda.stream(st):
            assert mb.update_depth(cam, d_img, pos, t, quat) == 1
        assert _same(_snapshot(ma), _snapshot(mb)), f
    assert ma.counters()["n_live_out"] > 5000
    ma.close(); mb.close()
