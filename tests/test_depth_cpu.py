"""CPU tests of the depth-image ingest (dspmap_preprocess_depth / dspmap_update_depth*): the numpy restatement (tests/depth_ref.py)
against the oracle's voxel-grid filter, the argument checks of the three entry points (made before the device is touched), and
the layout of dspmap_camera against the binding's ctypes structure.  The scenes of tests/test_gpu_depth_edges.py are checked here for
what they must reach in k_dp_accumulate -- tiles with more leaves than the LDS table holds, tiles whose probes run out while it has
room, tiles in between, the tiling's edge shapes, the value edges -- from the image and the specification alone, and the table's
constants in depth_ref.py are compared with the kernel's source."""
import ctypes as C
import os
import re
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
    DSPMAP_E_DEVICE.  (pixel_step above 2^24: width + step - 1 and the pixel column of a tile's unused lanes would leave the int.)"""
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
                dict(pixel_step=(1 << 24) + 1), dict(pixel_step=(1 << 30)), dict(pixel_step=2 ** 31 - 1),
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


# ---- what the scenes of tests/test_gpu_depth_edges.py reach, from the image and the specification alone
def _half_b(dsp):
    return common.half_extent(dsp.make_config(nx=66, ny=66, nz=40, res=0.15, ppv=24))


def _census(name, half):
    img, kw, leaf = R.scenes(half)[name]()
    cen = R.tile_census(img, kw, leaf, half)
    n = [len(c) for c in cen]
    fb = [R.forced_fallback(c) for c in cen]
    print("%-18s leaf %-5g tiles %3d  leaves per tile %s  forced_fallback %s" %
          (name, leaf, len(cen), n if len(n) < 12 else "%d .. %d" % (min(n), max(n)), fb if len(fb) < 12 else "%d .. %d" % (min(fb), max(fb))))
    return n, fb


def test_table_constants_match_the_kernel():
    """TILE_W, TILE_H, TAB, PROBES and the hash of depth_ref.py are those of dspmap_depth.hip: a retune of the table cannot silently leave
    the scenes short of the edge"""
    src = open(os.path.join(ROOT, "dsp-map_amd", "csrc", "dspmap_depth.hip")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (DP_TW|DP_TH|DP_TAB|DP_PROBES)\s+(\d+)\b", src, re.M)}
    assert defs == dict(DP_TW=R.TILE_W, DP_TH=R.TILE_H, DP_TAB=R.TAB, DP_PROBES=R.PROBES)
    mul, shift = re.search(r"\(\(unsigned\)cell \* (\d+)u\) >> (\d+);", src).groups()
    assert (int(mul), int(shift)) == (R.HASH_MUL, R.HASH_SHIFT)
    assert (2 ** 32 >> R.HASH_SHIFT) == R.TAB                      # the home slot spans the table
    assert re.search(r"\(hs \+ \(unsigned\)p\) & \(DP_TAB - 1\)", src)   # linear probing from the home slot, which forced_fallback assumes


def test_forced_fallback_on_known_sets():
    """the bound on hand-made sets: empty, one leaf, PROBES and PROBES + 1 leaves with the same home, a full table + 1"""
    homes = {}
    for c in range(200000):
        homes.setdefault(int(R.home_slot([c])[0]), []).append(c)
    same = homes[5]
    assert len(same) > R.PROBES + 3
    assert R.forced_fallback([]) == 0 and R.forced_fallback([7]) == 0
    assert R.forced_fallback(same[:R.PROBES]) == 0
    assert R.forced_fallback(same[:R.PROBES + 1]) == 1
    assert R.forced_fallback(same[:R.PROBES + 3] + same[:2]) == 3   # (distinct leaves count, not runs)
    one_each = [homes[h][0] for h in range(R.TAB)]
    assert R.forced_fallback(one_each) == 0
    assert R.forced_fallback(one_each + [homes[0][1], homes[300][1]]) == 2
    wrap = homes[R.TAB - 1][:R.PROBES] + homes[0][:1]               # homes 511 and 0 share slots 511, 0 .. 7: 9 slots, across the wrap
    assert R.forced_fallback(wrap) == 0
    assert R.forced_fallback(wrap + homes[0][1:2]) == 1
    assert R.forced_fallback(wrap + homes[0][1:2] + homes[1][:8]) == 8   # homes 511, 0, 1 share slots 511 .. 8: 10 slots for 18 leaves


def test_scenes_reach_the_table_paths(dsp):
    """overflow: more than TAB leaves in at least half of the tiles (here: all); probe_exhaustion: some tile with at most TAB leaves and a
    forced fallback; crowded: every tile between TAB / 2 and TAB; smooth: at most TAB / 4 and no forced fallback; few_leaves: 2 x 2 x 2
    leaves, at most 4 occupied, one key per tile, a leaf of more than 50 000 pixels; cropped: occupied leaves that the crop drops"""
    half = _half_b(dsp)
    n, fb = _census("overflow", half)
    assert sum(x > R.TAB for x in n) * 2 >= len(n) and len(n) == 9
    assert all(f >= x - R.TAB for x, f in zip(n, fb))
    n, fb = _census("probe_exhaustion", half)
    assert any(x <= R.TAB and f >= 1 for x, f in zip(n, fb))
    n, fb = _census("crowded", half)
    assert all(R.TAB // 2 <= x <= R.TAB for x in n)
    n, fb = _census("smooth", half)
    assert max(n) <= R.TAB // 4 and max(fb) == 0 and len(n) == 300
    n, fb = _census("few_leaves", half)
    img, kw, leaf = R.scene_few_leaves()
    ref, n_valid = R.preprocess_depth(img, kw, leaf, half, 10 ** 6)
    assert R.lattice(leaf, half)[1] == [2.0, 2.0, 2.0] and n_valid == 640 * 480 == int(ref["all_counts"].sum())
    assert ref["n_leaves"] <= 4 and ref["all_counts"].max() > 50000 and set(n) == {1}
    img, kw, leaf = R.scene_cropped()
    for lf in (leaf, 0.25):
        ref, _ = R.preprocess_depth(img, kw, lf, half, 10 ** 6)
        print("cropped            leaf %-5g leaves %d, kept by the crop %d" % (lf, ref["n_leaves"], len(ref["out"])))
        assert ref["n_leaves"] - len(ref["out"]) >= (10 if lf == leaf else 1)


def test_scenes_reach_the_tiling_edges(dsp):
    """65 x 17, 63 x 1, 1 x 33, 640 x 480 at pixel_step 7, 1000 and 2^24: used columns, used rows, tiles, and a kept pixel in the last used
    column and in the last used row"""
    half = _half_b(dsp)
    for (w, h, step), want in R.SHAPES.items():
        img, kw, leaf = R.SHAPE_SCENES["shape_%dx%d_step%d" % (w, h, step)]()
        assert R.used_shape(kw) == want
        _, keep = R.backproject_grid(img, kw)
        assert keep.shape == (want[1], want[0]) and keep[:, -1].any() and keep[-1, :].any()
        assert len(R.tile_census(img, kw, leaf, half)) == want[2]
        assert len(R.preprocess_depth(img, kw, leaf, half, 10 ** 6)[0]["out"]) >= 1


def test_scenes_reach_the_value_edges(dsp):
    """crop face: one leaf, no point; range limits: exactly the two pixels inside; non-finite: every pixel valid, none makes a leaf"""
    half = _half_b(dsp)
    img, kw, leaf = R.scene_crop_face(half)
    ref, n_valid = R.preprocess_depth(img, kw, leaf, half, 100)
    assert img[0, 0] == F(half[0]) and (n_valid, ref["n_leaves"], len(ref["out"])) == (1, 1, 0)
    img, kw, leaf = R.scene_range_limits()
    _, keep = R.backproject_grid(img, kw)
    assert keep.tolist() == [[False, True, True, False]]
    assert img[0, 0] < F(kw["min_depth"]) == img[0, 1] and img[0, 2] == F(kw["max_depth"]) < img[0, 3]
    ref, n_valid = R.preprocess_depth(img, kw, leaf, half, 100)
    assert (n_valid, ref["n_leaves"], len(ref["out"])) == (2, 2, 2)
    img, kw, leaf = R.scene_nonfinite_x()
    pts, keep = R.backproject_grid(img, kw)
    assert keep.all() and np.isfinite(pts[:, 2]).all()
    assert np.isinf(pts[[0, 4, 5], 0]).all() and np.isfinite(pts[1:4]).all() and np.abs(pts[1:4, 2]).min() >= 1e30
    ref, n_valid = R.preprocess_depth(img, kw, leaf, half, 100)
    assert (n_valid, ref["n_leaves"], len(ref["out"])) == (6, 0, 0)
    img, kw, leaf = R.scene_nonfinite_d()
    pts, keep = R.backproject_grid(img, kw)
    assert keep.all() and np.isinf(pts[:, 2]).all()
    ref, n_valid = R.preprocess_depth(img, kw, leaf, half, 100)
    assert (n_valid, ref["n_leaves"], len(ref["out"])) == (4, 0, 0)


def test_restatement_against_the_oracle_filter_on_noise(dsp, orc):
    """overflow and crowded, the scenes whose GPU test compares counts with the cloud path: no centroid within 1e-3 m of a crop face,
    and the oracle's filter on the restatement's cloud gives the same count and order within oracle_bound"""
    half = _half_b(dsp)
    for name in ("overflow", "crowded"):
        img, kw, leaf = R.TABLE_SCENES[name]()
        full, _ = R.preprocess_depth(img, kw, leaf, half, 10 ** 6)
        assert R.face_distance(full["out"], half) >= 1e-3
        for cap in (10 ** 5, len(full["out"]) // 2):
            ref, _ = R.preprocess_depth(img, kw, leaf, half, cap)
            orc_out, orc_leaves = orc.preprocess_cloud(ref["cloud"], leaf, half, max_points=cap, swap_axes=True)
            assert len(orc_out) == len(ref["out"]) == min(cap, len(full["out"])) and orc_leaves >= ref["n_leaves"]
            bound = R.oracle_bound(ref)
            d_orc = np.abs(ref["out"].astype(np.float64) - orc_out.astype(np.float64)).max()
            print("%s cap %d: %d points, %d leaves, |restatement - oracle| %.3g (bound %.3g)" % (name, cap, len(orc_out), ref["n_leaves"], d_orc, bound))
            assert d_orc <= bound and bound < 0.5 * leaf   # (a swapped pair of leaves would be off by a leaf size)


def test_lattice_sizes_of_the_limit_cases(dsp):
    """the leaf sizes tests/test_gpu_depth_edges.py expects to be refused put more than 2^27 leaves into config B's box"""
    half = _half_b(dsp)
    assert R.lattice(0.01, half)[1] == [992.0, 601.0, 992.0]        # (half_x is 4.95 rounded UP to fp32: 992, not 991)
    for leaf in (0.01, 1e-9, 1e-39):
        assert R.lattice_cells(leaf, half) > 2 ** 27
    assert R.lattice_cells(0.05, half) < 2 ** 27
