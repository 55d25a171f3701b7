"""CPU tests of the depth-image ingest (dspmap_preprocess_depth / dspmap_update_depth*): the numpy restatement (tests/depth_ref.py)
against the oracle's voxel-grid filter, the argument checks of the three entry points (made before the device is touched), and
the layout of dspmap_camera against the binding's ctypes structure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tests import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_restatement_against_the_oracle_filter(dsp, orc):
    """the integer-sum restatement on the synthetic 640 x 480 image against oracle_py.preprocess_cloud on the back-projected cloud:
    same number of points, same leaf order, every coordinate within the oracle's own worst-case summation error (computed from the
    input: 2^-24 * max|coordinate| * largest leaf population + 2^-21), and within 1e-6 m of the float64 centroids (2^-21 quantisation
    + half an ulp of a coordinate < 8 m).  Condition, checked on the reference's output: no centroid within 1e-3 m of a crop face."""
    half = common.half_extent(dsp.make_config())
    img = R.make_image()
    kw = R.camera_kw()
    for cap in (5000, 100000):
        ref, n_valid = R.preprocess_depth(img, kw, 0.1, half, cap)
        assert 250000 < n_valid < 640 * 480 and ref["n_leaves"] > 3000
        assert R.face_distance(ref["out"], half) >= 1e-3
        orc_out, orc_leaves = orc.preprocess_cloud(ref["cloud"], 0.1, half, max_points=cap, swap_axes=True)
        assert len(orc_out) == len(ref["out"]) == min(cap, len(ref["out"])) and orc_leaves >= ref["n_leaves"]
        bound = R.oracle_bound(ref)
        d_orc = np.abs(ref["out"].astype(np.float64) - orc_out.astype(np.float64)).max()
        d_exact = np.abs(ref["out"].astype(np.float64) - ref["exact"]).max()
        print("cap %d: %d points, %d leaves, |restatement - oracle| %.3g (bound %.3g), |restatement - float64| %.3g" %
              (cap, len(orc_out), ref["n_leaves"], d_orc, bound, d_exact))
        assert d_orc <= bound     # (same order: a swapped pair of leaves would be off by a leaf size)
        assert d_exact <= 1e-6
    assert len(R.preprocess_depth(img, kw, 0.1, half, 100000)[0]["out"]) > 5000   # (the cap of 5000 bites, the other does not)


def _cam(dsp, **over):
    return dsp.capi.make_camera(**R.camera_kw(**over))


def test_argument_checks_before_the_device(dsp):
    """every DSPMAP_E_ARG case returns DSPMAP_E_ARG with a text, whether or not a device exists; a valid call without a device is
    DSPMAP_E_DEVICE"""
    import torch
    L = dsp.load_library()
    m = dsp.DSPMap()
    img = R.make_image()
    out = np.zeros((16, 3), F)
    n = C.c_int()
    pos = (C.c_float * 3)(0, 0, 0)
    quat = (C.c_float * 4)(1, 0, 0, 0)
    ip, op = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    E_ARG, E_DEVICE = -1, -2

    def calls(cam, image=ip, leaf=0.1, max_points=16, handle=m.h):
        camp = C.byref(cam) if cam is not None else None
        return (L.dspmap_preprocess_depth(handle, camp, image, leaf, max_points, op, C.byref(n), None, None),
                L.dspmap_update_depth_device(handle, camp, image, leaf, max_points, C.cast(pos, C.c_void_p), 0.0, C.cast(quat, C.c_void_p)),
                L.dspmap_update_depth(handle, camp, image, leaf, max_points, C.cast(pos, C.c_void_p), 0.0, C.cast(quat, C.c_void_p)))

    inf, nan = float("inf"), float("nan")
    bad_cams = [dict(width=0), dict(height=0), dict(width=-3), dict(pixel_step=0), dict(pixel_step=-1),
                dict(row_stride_bytes=640 * 2 - 2), dict(row_stride_bytes=640 * 2 + 1), dict(row_stride_bytes=-1280),
                dict(fmt=1, row_stride_bytes=640 * 4 + 2), dict(fmt=2), dict(fmt=-1),
                dict(fx=0.0), dict(fx=-320.0), dict(fx=inf), dict(fx=nan), dict(fy=0.0), dict(fy=nan), dict(fy=inf),
                dict(depth_scale=0.0), dict(depth_scale=-0.001), dict(depth_scale=inf), dict(depth_scale=nan),
                dict(cx=inf), dict(cx=nan), dict(cy=-inf), dict(cy=nan),
                dict(min_depth=2.0, max_depth=1.0), dict(min_depth=nan), dict(max_depth=nan)]
    for over in bad_cams:
        for rc in calls(_cam(dsp, **over)):
            assert rc == E_ARG, over
            assert L.dspmap_last_error(m.h), over
    good = _cam(dsp)
    for kwargs in (dict(cam=None), dict(cam=good, image=None), dict(cam=good, leaf=0.0), dict(cam=good, leaf=-0.1), dict(cam=good, leaf=nan),
                   dict(cam=good, max_points=-1)):
        for rc in calls(**kwargs):
            assert rc == E_ARG, kwargs
            assert L.dspmap_last_error(m.h)
    assert calls(good, handle=None) == (E_ARG, E_ARG, E_ARG)
    # NULL outputs / pose
    assert L.dspmap_preprocess_depth(m.h, C.byref(good), ip, 0.1, 16, None, C.byref(n), None, None) == E_ARG
    assert L.dspmap_preprocess_depth(m.h, C.byref(good), ip, 0.1, 16, op, None, None, None) == E_ARG
    assert L.dspmap_update_depth(m.h, C.byref(good), ip, 0.1, 16, None, 0.0, C.cast(quat, C.c_void_p)) == E_ARG
    assert L.dspmap_update_depth_device(m.h, C.byref(good), ip, 0.1, 16, C.cast(pos, C.c_void_p), 0.0, None) == E_ARG
    if not torch.cuda.is_available():   # (no CPU fallback: a valid call fails loudly)
        assert L.dspmap_update_depth(m.h, C.byref(good), ip, 0.1, 16, C.cast(pos, C.c_void_p), 0.0, C.cast(quat, C.c_void_p)) == E_DEVICE
        assert b"no HIP device" in L.dspmap_last_error(m.h)
        with pytest.raises(dsp.capi.DSPMapError, match="no HIP device"):
            m.update_depth(good, img, (0, 0, 0), 0.0, (1, 0, 0, 0))
    m.close()


def test_camera_layout_matches_the_header(dsp, tmp_path):
    """sizeof(dspmap_camera) and its field offsets equal capi.Camera's"""
    fields = [f for f, _ in dsp.capi.Camera._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dspmap.h"\nint main(void) {\n    printf("%zu", sizeof(dspmap_camera));\n' +
                   "".join('    printf(" %%zu", offsetof(dspmap_camera, %s));\n' % f for f in fields) +
                   '    printf(" %d %d\\n", DSPMAP_DEPTH_U16, DSPMAP_DEPTH_F32);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(dsp.capi.Camera)] + [getattr(dsp.capi.Camera, f).offset for f in fields] + [dsp.capi.DEPTH_U16, dsp.capi.DEPTH_F32]
    assert got == want
    assert fields == ["width", "height", "row_stride_bytes", "format", "fx", "fy", "cx", "cy", "depth_scale", "min_depth", "max_depth",
                      "pixel_step"]


def test_dropin_class_offers_update_depth(dsp, tmp_path):
    """include/dsp_dynamic.h: updateDepth type-checks in the plain and in the sharded build of the class"""
    src = tmp_path / "ud.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n    dspmap_camera cam = {};\n    unsigned short px[4] = {0, 0, 0, 0};\n'
                   "    int a = my_map.updateDepth(cam, px, 0.f, 0.f, 0.f, 0.0, 1.f, 0.f, 0.f, 0.f);\n"
                   "    int b = my_map.updateDepth(cam, px, 0.f, 0.f, 0.f, 0.0, 1.f, 0.f, 0.f, 0.f, 0.25f, 100);\n    return a + b;\n}\n")
    for macros in ([], ["-DDSPMAP_WORLD=1"]):
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + macros + [str(src)])
