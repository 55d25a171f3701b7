"""Timing of the depth-image ingest (dspmap_preprocess_depth, dspmap_update_depth) against what a caller had to do before it: numpy
back-projection on the host, H2D of the cloud, dspmap_preprocess_cloud, dspmap_update_device.  Two 640 x 480 uint16 millimetre images:
the synthetic wall + box image of the tests (tests/depth_ref.py) and a frame of scene.CorridorScene quantised to millimetres.
Config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel).

Device times: HIP events on the handle's stream (a torch stream) around every single call, the arms interleaved call by call in one
process, median over `--reps` after `--warmup` untimed rounds.  Both functions are synchronous and end with the same small read of
their counters, so both figures contain it; the baseline arm is the parent commit's dspmap_preprocess_cloud on the back-projected
cloud already resident in HBM (unchanged in this build).  Wall times per frame: time.perf_counter around whole frames, each arm on
its own handle, interleaved frame by frame, every frame waited for.  Prints one JSON line.  bench.py is not involved.

    python tools/depth_bench.py [--reps 200] [--warmup 20] [--frames 60]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dsp-map_amd"))


def host_backproject(img, fx, fy, cx, cy, scale, max_depth):
    """the caller's host loop, vectorised: uint16 image -> camera-frame cloud [n, 3] float32"""
    h, w = img.shape
    d = img.astype(np.float32) * np.float32(scale)
    keep = (img != 0) & (d <= np.float32(max_depth))
    v, u = np.nonzero(keep)
    d = d[keep]
    x = (u.astype(np.float32) - np.float32(cx)) * d / np.float32(fx)
    y = (v.astype(np.float32) - np.float32(cy)) * d / np.float32(fy)
    return np.stack([x, y, d], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    import build_ext
    build_ext.build()
    import dsp_map_amd as D
    from tests import depth_ref as R
    scene = importlib.import_module("dsp-map_amd.scene")

    w = dict(nx=66, ny=66, nz=40, res=0.15, ppv=24)
    sc = scene.CorridorScene(w["nx"] * w["res"], w["ny"] * w["res"], w["nz"] * w["res"], seed=1234, device="cuda")
    depth, _, _ = sc._depth(1.0)
    depth = depth.reshape(480, 640).cpu().numpy()
    corridor = np.where(np.isfinite(depth), np.clip(np.rint(depth * 1000.0), 1, 65534), 0).astype(np.uint16)
    images = {
        "wall_box": (R.make_image(), dict(fx=320.0, fy=326.4, cx=319.5, cy=239.5)),
        "corridor": (corridor, dict(fx=320.0, fy=240.0 / np.tan(np.radians(30.0)), cx=319.5, cy=239.5)),
    }
    st = torch.cuda.Stream()
    out = {}
    for name, (img, intr) in images.items():
        cam = D.capi.make_camera(640, 480, depth_scale=0.001, min_depth=0.0, max_depth=20.0, **intr)
        cloud = host_backproject(img, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 0.001, 20.0)
        m = D.DSPMap(D.make_config(seed=1234, **w))
        m._chk(m.L.dspmap_init_device(m.h))
        m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
        d_img = torch.from_numpy(img.view(np.int16).copy()).cuda()
        d_cloud = torch.from_numpy(cloud).cuda()
        d_out = torch.zeros((5000, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        res = {}

        def arm_depth():
            pts, nl, nv = m.preprocess_depth(cam, d_img, max_points=5000, leaf=0.1)
            res["depth"] = (int(pts.shape[0]), nl, nv)

        def arm_cloud():
            res["cloud"] = m.preprocess_cloud(d_cloud.data_ptr(), cloud.shape[0], d_out.data_ptr(), 5000, leaf=0.1, swap_axes=True)

        times = {"depth": [], "cloud": []}
        with torch.cuda.stream(st):
            for r in range(args.warmup + args.reps):
                for key, fn in (("depth", arm_depth), ("cloud", arm_cloud)) if r % 2 == 0 else (("cloud", arm_cloud), ("depth", arm_depth)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[key].append(e0.elapsed_time(e1) * 1000.0)
        o = {"valid_pixels": res["depth"][2], "cloud_points": int(cloud.shape[0]), "leaves": res["depth"][1], "points_out": res["depth"][0],
             "points_out_cloud_path": res["cloud"][0],
             "preprocess_depth_us": round(float(np.median(times["depth"])), 2),
             "preprocess_cloud_us": round(float(np.median(times["cloud"])), 2)}
        o["depth_over_cloud"] = round(o["preprocess_depth_us"] / o["preprocess_cloud_us"], 3)
        m.close()

        # whole frames, wall clock: update_depth(host image) against the caller sequence it replaces
        def new_map():
            x = D.DSPMap(D.make_config(seed=1234, **w))
            x.set_param(D.capi.P_VELOCITY_ESTIMATOR, 2)
            return x
        ma, mb = new_map(), new_map()
        wall = {"update_depth": [], "caller_sequence": []}
        for f in range(args.frames + 5):
            pos, t, quat = (0.01 * f, 0.0, 0.0), f / 30.0, (1.0, 0.0, 0.0, 0.0)
            t0 = time.perf_counter()
            assert ma.update_depth(cam, img, pos, t, quat, max_points=5000, leaf=0.1) == 1
            ma.sync()
            t1 = time.perf_counter()
            c = host_backproject(img, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 0.001, 20.0)
            dc = torch.from_numpy(c).cuda()
            torch.cuda.synchronize()
            n, _ = mb.preprocess_cloud(dc.data_ptr(), c.shape[0], d_out.data_ptr(), 5000, leaf=0.1, swap_axes=True)
            assert mb.update_device(d_out.data_ptr(), n, pos, t, quat) == 1
            mb.sync()
            t2 = time.perf_counter()
            if f >= 5:
                wall["update_depth"].append((t1 - t0) * 1e3)
                wall["caller_sequence"].append((t2 - t1) * 1e3)
        o["frame_update_depth_host_image_ms"] = round(float(np.median(wall["update_depth"])), 3)
        o["frame_numpy_backprojection_h2d_preprocess_cloud_update_device_ms"] = round(float(np.median(wall["caller_sequence"])), 3)
        o["image_bytes"] = int(img.nbytes)
        o["cloud_bytes"] = int(cloud.nbytes)
        ma.close(); mb.close()
        out[name] = o
    out["config"] = "B: 66x66x40 @ 0.15 m, 24 particles/voxel; leaf 0.1 m, cap 5000; medians of %d interleaved calls after %d, %d frames" % (
        args.reps, args.warmup, args.frames)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
