"""What the layer benches (tools/*_bench.py) share; imported by them, not run.  The workloads, the command line, the map behind its
side stream after the frames of the synthetic depth stream (scene.py), the event timing of interleaved arms, and the main loop over the
workloads.  Each tool keeps its docstring, its own defaults and extra flags, its arms, its host route, its asserts and its JSON line."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dsp-map_amd"))

WORKLOADS = {"B": dict(nx=66, ny=66, nz=40, res=0.15, ppv=24), "L": dict(nx=132, ny=132, nz=60, res=0.15, ppv=9)}


def parser(reps=200, warmup=20, frames=20, host_reps=None, only=True):
    """the flags the tools share, with the tool's own defaults; host_reps=None / only=False: the tool has no such flag"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--frames", type=int, default=frames)
    if host_reps is not None:
        ap.add_argument("--host-reps", type=int, default=host_reps)
    if only:
        ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    return ap


def open_map(D, scene, name, frames, after_frame=None, spare=0):
    """(handle, its side stream) of workload `name` after `frames` frames of scene.py, queued on that stream and waited for;
    after_frame(m) runs behind every frame (the tools that integrate the known-space layer).  The scene's frames (points, position,
    attitude, stamp; 30 Hz, reproducible) stay on the handle as m.scene_frames, `spare` more of them than were fed, for the tools
    that go on with the stream or need the last position."""
    w = WORKLOADS[name]
    m = D.DSPMap(D.make_config(seed=1234, **w))
    m._chk(m.L.dspmap_init_device(m.h))
    sc = scene.CorridorScene(w["nx"] * w["res"], w["ny"] * w["res"], w["nz"] * w["res"], seed=1234, device="cuda")
    torch.use_deterministic_algorithms(True)
    m.scene_frames = [sc.frame(f / 30.0) + (f / 30.0,) for f in range(frames + spare)]
    torch.use_deterministic_algorithms(False)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    with torch.cuda.stream(st):
        for f, (pts, pos, quat, t) in enumerate(m.scene_frames[:frames]):
            if f:
                m.clearOccupancyMapPrediction()
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            if after_frame is not None:
                after_frame(m)
        st.synchronize()
    return m, st


def timed(st, fns, reps, warmup):
    """device time (us) of each of reps calls of every arm, the arms interleaved call by call -> [(median, min)] per arm"""
    with torch.cuda.stream(st):
        for _ in range(warmup):
            for fn in fns:
                fn()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
        for row in ev:
            for fn, (e0, e1) in zip(fns, row):
                e0.record(st)
                fn()
                e1.record(st)
        st.synchronize()
    t = np.array([[e0.elapsed_time(e1) * 1000.0 for e0, e1 in row] for row in ev])
    return [(round(float(np.median(t[:, j])), 2), round(float(t[:, j].min()), 2)) for j in range(len(fns))]


def main(run, ap, names=("B", "L")):
    """parse the command line, build the library, run(D, scene, name, args) per workload (--only: that one)"""
    args = ap.parse_args()
    import build_ext
    build_ext.build()
    import dsp_map_amd as D
    scene = importlib.import_module("dsp-map_amd.scene")
    for name in ([args.only] if getattr(args, "only", None) else names):
        run(D, scene, name, args)
