"""GPU tests of the depth-image ingest past the inputs of tests/test_gpu_depth.py: tiles that touch more leaves than k_dp_accumulate's LDS
table holds (its runs add to memory themselves), tiles whose probes run out while the table has room, tiles in between, a lattice of 8
leaves, the edge shapes of the tiling, centroids on a crop face, depths on the range limits, non-finite coordinates -- bit for bit against
the numpy restatement (tests/depth_ref.py), on every run, handle and stream, with the cloud path as the cross-check; one handle through
a sequence of lattices, caps and images that a leaf left behind by k_dp_emit would spoil; the lattice limit of both entry points; and
frames from images whose format, size and cap change from frame to frame.  What each scene reaches in the kernel is asserted from the
image alone in tests/test_depth_cpu.py; the lines printed here repeat it next to the device's counts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import common
from tests import depth_ref as R
from tests.test_gpu_depth import _bits_equal, _dev, _ingest_raw, _new_map, _same, _snapshot

pytestmark = pytest.mark.gpu
F = np.float32
B = dict(nx=66, ny=66, nz=40, res=0.15, ppv=24)
HALF = (float(F(0.15) * F(66) * F(0.5)), float(F(0.15) * F(66) * F(0.5)), float(F(0.15) * F(40) * F(0.5)))   # common.half_extent of B
UNCAPPED = 400000          # more than 640 x 480 pixels
E_ARG = -1
SCENE_NAMES = sorted(R.scenes(HALF))


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(image, camera_kw, leaf, uncapped restatement, n_valid, largest per-tile leaf count, largest forced_fallback): computed once, shared
    by every test, never written to"""
    img, kw, leaf = R.scenes(HALF)[name]()
    ref, n_valid = R.preprocess_depth(img, kw, leaf, HALF, UNCAPPED)
    cen = R.tile_census(img, kw, leaf, HALF)
    for a in (img, ref["out"], ref["cloud"]):
        a.setflags(write=False)
    return img, kw, leaf, ref, n_valid, max(len(c) for c in cen), max(R.forced_fallback(c) for c in cen)


def _check(m, dsp, name, cap, leaf=None, d_img=None):
    """one call of dspmap_preprocess_depth on scene `name` against the restatement (whose cap is a cut of its uncapped output)"""
    img, kw, leaf0, ref, n_valid, _, _ = _scene(name)
    leaf = leaf0 if leaf is None else leaf
    if leaf != leaf0:
        ref, n_valid = R.preprocess_depth(img, kw, leaf, HALF, UNCAPPED)
    want = ref["out"][:cap]
    got, nl, nv = _ingest_raw(m, dsp.capi.make_camera(**kw), _dev(img) if d_img is None else d_img, cap, leaf)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum()) if got.shape == want.shape else -1
    assert (len(got), nl, nv) == (len(want), ref["n_leaves"], n_valid), (name, cap, leaf, len(got), nl, nv, len(want), ref["n_leaves"], n_valid)
    assert _bits_equal(got, want), (name, cap, leaf, bad)
    return len(got), nl, nv


@pytest.fixture(scope="module")
def shared_map(dsp):
    """one handle for every scene of test a: each call also meets whatever the scene before it left in the grid"""
    m = dsp.DSPMap(dsp.make_config(**B))
    assert common.half_extent(m.cfg) == HALF
    yield m
    m.close()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_bit_equal_to_the_restatement(dsp, shared_map, name):
    """a. every scene at an uncapped max_points and at a cap that bites (half of the uncapped count, where there are two points to cut):
    equal n_out, n_leaves, n_valid, zero mismatching float bits, nothing written past n_out"""
    img, kw, leaf, ref, n_valid, tile_max, fb_max = _scene(name)
    d_img = _dev(img)
    n_unc = len(ref["out"])
    caps = [UNCAPPED] + ([n_unc // 2] if n_unc >= 2 else [])
    for cap in caps:
        n, nl, nv = _check(shared_map, dsp, name, cap, d_img=d_img)
        print("%-24s leaf %-5g cap %6d  n_out %6d  leaves %6d  valid %6d  mismatching values 0  most leaves in a tile %4d  forced_fallback %3d" %
              (name, leaf, cap, n, nl, nv, tile_max, fb_max))
        assert n == min(cap, n_unc)
    assert caps[-1] < n_unc or n_unc < 2
    if name == "overflow":
        assert tile_max > R.TAB
    if name == "few_leaves":
        assert n_valid == 640 * 480 and ref["n_leaves"] == 4 == n_unc
    if name == "crop_face":
        assert (n_valid, ref["n_leaves"], n_unc) == (1, 1, 0)
    if name == "range_limits":
        assert (n_valid, n_unc) == (2, 2)
    if name in ("nonfinite_x", "nonfinite_d"):
        assert n_valid == img.size and ref["n_leaves"] == 0


@pytest.mark.parametrize("name", ["overflow", "probe_exhaustion", "crowded"])
def test_same_bits_whichever_path_a_run_took(dsp, name):
    """b. five times on one handle and once on a second handle with a caller-owned stream: which runs of a tile find a place in the
    table depends on the order of the waves, the result does not"""
    m = dsp.DSPMap(dsp.make_config(**B))
    m2 = dsp.DSPMap(dsp.make_config(**B))
    st = torch.cuda.Stream()
    m2._chk(m2.L.dspmap_set_stream(m2.h, st.cuda_stream))
    d_img = _dev(_scene(name)[0])
    for _ in range(5):
        _check(m, dsp, name, UNCAPPED, d_img=d_img)
    _check(m2, dsp, name, UNCAPPED, d_img=d_img)
    m.close(); m2.close()


@pytest.mark.parametrize("name", ["overflow", "crowded"])
def test_cloud_path_as_cross_check(dsp, name):
    """c. dspmap_preprocess_cloud(swap_axes = 1) on the restatement's cloud: same count and order, coordinates within the worst-case fp32
    summation error computed from the input (oracle_bound; far below a leaf, so a swapped pair would show)"""
    img, kw, leaf, ref, n_valid, _, _ = _scene(name)
    assert R.face_distance(ref["out"], HALF) >= 1e-3   # (condition for comparing counts with a path that rounds differently)
    m = dsp.DSPMap(dsp.make_config(**B))
    d_cloud = torch.from_numpy(ref["cloud"].copy()).cuda()
    d_out = torch.zeros((len(ref["out"]) + 8, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n_old, leaves_old = m.preprocess_cloud(d_cloud.data_ptr(), len(ref["cloud"]), d_out.data_ptr(), len(d_out), leaf=leaf, swap_axes=True)
    old = d_out[:n_old].cpu().numpy()
    assert n_old == len(ref["out"]) and leaves_old == ref["n_leaves"]
    bound = R.oracle_bound(ref)
    diff = float(np.abs(old.astype(np.float64) - ref["out"].astype(np.float64)).max())
    print("%s: cloud path against the restatement: max |difference| %.3g m (bound %.3g)" % (name, diff, bound))
    assert diff <= bound < 0.5 * leaf
    m.close()


def _refused(m, dsp, leaf):
    """both entry points refuse `leaf` with DSPMAP_E_ARG and a text, and leave n_out untouched or 0"""
    img, kw, _, ref, _, _, _ = _scene("crowded")
    cam = dsp.capi.make_camera(**kw)
    d_img = _dev(img)
    d_cloud = torch.from_numpy(ref["cloud"].copy()).cuda()
    out = torch.full((16, 3), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n, nl, nv = C.c_int(-5), C.c_int(-5), C.c_int(-5)
    rc = m.L.dspmap_preprocess_depth(m.h, C.byref(cam), d_img.data_ptr(), leaf, 16, out.data_ptr(), C.byref(n), C.byref(nl), C.byref(nv))
    text = m.L.dspmap_last_error(m.h)
    assert rc == E_ARG and text and b"leaf" in text, (leaf, rc, text)
    assert n.value in (-5, 0)
    n, nl = C.c_int(-5), C.c_int(-5)
    rc = m.L.dspmap_preprocess_cloud(m.h, len(ref["cloud"]), d_cloud.data_ptr(), 3, leaf, 1, 16, out.data_ptr(), C.byref(n), C.byref(nl))
    text = m.L.dspmap_last_error(m.h)
    assert rc == E_ARG and text and b"leaf" in text, (leaf, rc, text)
    assert n.value in (-5, 0)
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())


def test_one_handle_through_lattices_caps_and_images(dsp):
    """d. leaf 0.1 uncapped on an image with cropped leaves -> leaf 0.05 on `overflow` (the grid grows) -> leaf 0.1 with cap 7 (a coarser
    lattice inside the larger grid, most leaves beyond the cap) -> leaf 0.1 on a different image -> max_points = 0 with a NULL out_dev ->
    leaf 0.25 -> a refused leaf -> leaf 0.1 on the first image again: every accepted call equals the restatement of that call alone,
    which is what a fresh handle gives.  A leaf that k_dp_emit left behind (cropped, beyond the cap, of the finer lattice) would be a
    ghost leaf in n_leaves or a shifted centroid in the next call."""
    m = dsp.DSPMap(dsp.make_config(**B))
    ref = _scene("cropped")[3]
    assert ref["n_leaves"] - len(ref["out"]) >= 10 and len(ref["out"]) > 7   # (cropped leaves and leaves beyond the cap exist)
    _check(m, dsp, "cropped", UNCAPPED)
    _check(m, dsp, "overflow", UNCAPPED)
    assert _check(m, dsp, "cropped", 7)[0] == 7
    _check(m, dsp, "crowded", UNCAPPED)
    # max_points = 0, NULL out_dev
    img, kw, leaf, ref, n_valid, _, _ = _scene("cropped")
    cam = dsp.capi.make_camera(**kw)
    d_img = _dev(img)
    n, nl, nv = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    rc = m.L.dspmap_preprocess_depth(m.h, C.byref(cam), d_img.data_ptr(), leaf, 0, None, C.byref(n), C.byref(nl), C.byref(nv))
    assert rc == 1, m.L.dspmap_last_error(m.h)
    assert (n.value, nl.value, nv.value) == (0, ref["n_leaves"], n_valid)
    _check(m, dsp, "crowded", UNCAPPED)      # (the leaves of the call that wrote nothing are gone too)
    _check(m, dsp, "cropped", UNCAPPED, leaf=0.25)
    _refused(m, dsp, 0.01)
    _check(m, dsp, "cropped", UNCAPPED)
    m.close()


def _smallest_accepted_leaf():
    """the smallest multiple of 0.0005 m whose lattice over B's box stays under 2^26 leaves (accumulators under 2 GB)"""
    for k in range(20, 200):
        leaf = k * 0.0005
        if R.lattice_cells(leaf, HALF) < 2 ** 26:
            return leaf
    raise AssertionError


def test_lattice_limit_of_both_entry_points(dsp):
    """e. leaf 0.01 (992 x 601 x 992 leaves in B's box), 1e-9 and a denormal leaf (whose inverse is +inf) are DSPMAP_E_ARG with a text
    from dspmap_preprocess_depth and from dspmap_preprocess_cloud; the handle ingests correctly after every refusal; a leaf just coarse
    enough (under 2^26 leaves) is accepted by both and equals the restatement (the cloud path within its summation bound)"""
    m = dsp.DSPMap(dsp.make_config(**B))
    assert R.lattice_cells(0.01, HALF) == 992 * 601 * 992 > 2 ** 27
    for leaf in (0.01, 1e-9, 1e-39):
        assert float(F(leaf)) > 0.0
        _refused(m, dsp, leaf)
        _check(m, dsp, "crowded", UNCAPPED)
    leaf = _smallest_accepted_leaf()
    cells = R.lattice_cells(leaf, HALF)
    assert 2 ** 25 < cells < 2 ** 26 and R.lattice_cells(leaf - 0.0005, HALF) >= 2 ** 26
    img, kw, _, _, _, _, _ = _scene("crowded")
    ref, n_valid = R.preprocess_depth(img, kw, leaf, HALF, UNCAPPED)
    n, nl, nv = _check(m, dsp, "crowded", UNCAPPED, leaf=leaf)
    print("leaf %.4f: %d leaves in the lattice, n_out %d, leaves %d" % (leaf, int(cells), n, nl))
    assert R.face_distance(ref["out"], HALF) >= 1e-3
    d_cloud = torch.from_numpy(ref["cloud"].copy()).cuda()
    d_out = torch.zeros((len(ref["out"]) + 8, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n_old, leaves_old = m.preprocess_cloud(d_cloud.data_ptr(), len(ref["cloud"]), d_out.data_ptr(), len(d_out), leaf=leaf, swap_axes=True)
    assert n_old == len(ref["out"]) and leaves_old == ref["n_leaves"]
    diff = float(np.abs(d_out[:n_old].cpu().numpy().astype(np.float64) - ref["out"].astype(np.float64)).max())
    assert diff <= R.oracle_bound(ref) < 0.5 * leaf
    _check(m, dsp, "crowded", UNCAPPED)      # (the coarse lattice inside the large grid)
    m.close()


def _frames():
    """(image as the camera lays it out, camera_kw, max_points) per frame: the format, the row stride, the pixel step, the image size and
    the cap change between frames; one frame has max_points = 0, one is the `crowded` noise image"""
    small = dict(width=320, height=240, fx=160.0, fy=163.2, cx=159.5, cy=119.5)
    f32_small = dict(small, fmt=R.F32, depth_scale=1.0, row_stride_bytes=320 * 4 + 36, pixel_step=2)
    f32_large = dict(fmt=R.F32, depth_scale=1.0, row_stride_bytes=640 * 4 + 64, pixel_step=2)
    crowded_img, crowded_kw, _, _, _, _, _ = _scene("crowded")

    def f32(w, h, seed, stride):
        return R.pad_rows(R.make_image_f32(w, h, seed=seed), stride).view(np.float32)

    return [(R.make_image(320, 240, seed=200), R.camera_kw(**small), 500),
            (f32(320, 240, 201, f32_small["row_stride_bytes"]), R.camera_kw(**f32_small), 500),
            (R.make_image(seed=202, shift=0.1), R.camera_kw(), 500),                                   # the image grows
            (f32(640, 480, 203, f32_large["row_stride_bytes"]), R.camera_kw(**f32_large), 5000),       # max_points grows
            (R.make_image(seed=204, shift=0.2), R.camera_kw(), 0),
            (crowded_img, crowded_kw, 5000),
            (R.make_image(seed=206, shift=0.3), R.camera_kw(), 5000),
            (f32(320, 240, 207, f32_small["row_stride_bytes"]), R.camera_kw(**f32_small), 500)]


def test_frames_from_images_of_changing_format_size_and_cap(dsp):
    """f. update_depth (host images), update_depth_device and update_device with the restatement's cloud over 8 frames: float32 with padded
    rows and pixel_step 2 and packed uint16, 320 x 240 then 640 x 480 (dp_img / dp_img_pin grow), max_points 500 then 5000 (dp_out
    grows), one frame with max_points = 0, one of noise: results, future status, exported state and every integer counter equal bit for
    bit after every frame, n_points_in equal to the restatement's count"""
    mh, md, mr = _new_map(dsp), _new_map(dsp), _new_map(dsp)
    counts = []
    for f, (img, kw, cap) in enumerate(_frames()):
        cam = dsp.capi.make_camera(**kw)
        pos, t, quat = (0.03 * f, 0.01 * f, 0.0), f / 30.0, (1.0, 0.0, 0.0, 0.0)
        ref, _ = R.preprocess_depth(img, kw, 0.1, HALF, cap)
        d_img = torch.from_numpy(img.copy()).cuda() if img.dtype == np.float32 else _dev(img)
        d_cloud = torch.from_numpy(np.ascontiguousarray(ref["out"]) if len(ref["out"]) else np.zeros((1, 3), F)).cuda()
        torch.cuda.synchronize()
        assert mh.update_depth(cam, img, pos, t, quat, max_points=cap, leaf=0.1) == 1
        assert md.update_depth(cam, d_img, pos, t, quat, max_points=cap, leaf=0.1) == 1
        assert mr.update_device(d_cloud.data_ptr(), len(ref["out"]), pos, t, quat) == 1
        sh, sd, sr = _snapshot(mh), _snapshot(md), _snapshot(mr)
        assert sr[5]["n_points_in"] == len(ref["out"]) == sh[5]["n_points_in"] == sd[5]["n_points_in"], f
        assert _same(sh, sr), f
        assert _same(sd, sr), f
        counts.append(len(ref["out"]))
    print("points per frame:", counts)
    assert counts[0] == counts[1] == counts[2] == 500 and counts[3] > 500 and counts[4] == 0 and counts[5] > 2000 and counts[6] == 5000
    assert mr.counters()["n_live_out"] > 10000   # (the frames did something)
    for x in (mh, md, mr):
        x.close()
