"""Timing of the arrival-time fields grown through the cast grid (dspmap_build_reach_fields_device, dspmap_reach_paths_device) against the
route a user has without them: (c) a cast_grid() copy of all layers to the host and the same wavefront there.  The host wavefront is
scipy.ndimage's binary dilation per step if scipy imports, else the numpy restatement of the tests (tests/reach_ref.fields); both are
whole-array operations per step, not per-cell Python loops.  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel; the wave
sets live in LDS) and 132 x 132 x 60 (9 particles / voxel; device sets), each after 20 frames of the synthetic depth stream (scene.py);
L = 7 layers, threshold 0.2, grids inflated by 0 and by 2 voxels, max_steps 256 and 4096.

(a) the build for 1 / 16 / 64 fields (one source each, in cells free in every layer), static (t_start < 0) and scheduled (t_start = 0,
step_seconds = voxel / 1.5 m/s), LDS against DSPMAP_REACH_DEVICE_SETS where both apply; (b) paths for 4 096 starts down the static
16-field build.  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup`
untimed ones, the arms interleaved call by call; the median is reported (and the minimum).  The host route is wall time, the median of
`--host-reps` runs, and the tool asserts that both routes give the same fields.  Prints one JSON line per workload.  bench.py is not
involved.

Space-time paths (dspmap_build_reach_timeline_device, dspmap_reach_timeline_paths_device), at max_steps 256: (d) the timeline build
against the plain build -- the same call in the same run, arms interleaved, for 1 / 16 / 64 fields, both schedules and both homes of the
wave sets; the difference is what the history stores cost (a batch whose kept sets exceed DSPMAP_REACH_TIMELINE_MAX_BYTES is reported as
such and not timed); (e) timeline paths for 4 096 starts through the scheduled 16-field build; (f) the route without the feature: the
cast_grid() copy, the restatement's wavefront with its sets (tests/reach_ref.fields) and its backward walk (tests/reach_time_ref) on the
host, one field, with the assertion that both routes give the same paths.  `--section fields|timeline` runs one half of the tool.

    python tools/reach_bench.py [--reps 200] [--warmup 20] [--host-reps 3] [--only B|L] [--section all|fields|timeline]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
SPEED = 1.5          # m/s: a scheduled front crosses one voxel per step_seconds = res / SPEED
FIELDS = (1, 16, 64)
MAX_STEPS = (256, 4096)
N_START = 4096
TIMELINE_STEPS = 256
LDS_BYTES = 160 * 1024 - 256


def host_fields(reach_ref, cfg, lay, src, n_fields, **kw):
    """the wavefront on the host: scipy.ndimage if it imports (one binary dilation with the 6-neighbourhood per step), else the restatement"""
    try:
        from scipy import ndimage
    except ImportError:
        return reach_ref.fields(cfg, lay, src, n_fields, **kw), "numpy restatement (tests/reach_ref.fields)"
    layers = reach_ref.schedule(cfg, kw["t_start"], kw["step_seconds"], kw["max_steps"])
    st = ndimage.generate_binary_structure(3, 1)[None]
    R = reach_ref.source_sets(cfg, src, n_fields) & ~lay[layers[0]][None]
    val = np.full(R.shape, reach_ref.UNREACHED, np.uint16)
    val[R] = 0
    for k in range(1, kw["max_steps"] + 1):
        new = ndimage.binary_dilation(R, st) & ~lay[layers[k]][None]
        val[new & (val == reach_ref.UNREACHED)] = k
        same = np.array_equal(new, R)
        R = new
        if not R.any() or (same and (layers[k:] == layers[k]).all()):
            break
    return val, "scipy.ndimage.binary_dilation per step"


def run(D, scene, name, args):
    from tests import reach_ref, reach_time_ref
    w = WORKLOADS[name]
    do_fields, do_timeline = args.section in ("all", "fields"), args.section in ("all", "timeline")
    m, st = harness.open_map(D, scene, name, args.frames)

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    cfg = m.cfg
    fits = 2 * 8 * w["nz"] * w["ny"] * ((w["nx"] + 63) // 64) <= LDS_BYTES
    step = w["res"] / SPEED
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": m.T + 1, "threshold": THRESHOLD, "sets_fit_in_lds": fits, "scheduled_step_seconds": round(step, 4)}
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    for r in (0, 2):
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, r)
            lay = reach_ref.unpack(m.cast_grid(), w["nx"])
        cand = np.argwhere(~lay.any(0))
        assert len(cand) >= 64, "no room for 64 sources"
        pick = cand[rng.choice(len(cand), 64, replace=False)]
        src = reach_ref.points([tuple((-half + w["res"] * (c[::-1] + 0.5)).tolist()) + (k,) for k, c in enumerate(pick)])
        dsrc = torch.from_numpy(src.view(np.int32).reshape(-1, 4).copy()).cuda()
        starts = np.zeros(N_START, reach_ref.POINT_DTYPE)
        p = rng.uniform(-0.98, 0.98, (N_START, 3)) * half
        starts["x"], starts["y"], starts["z"], starts["field"] = p[:, 0], p[:, 1], p[:, 2], rng.integers(0, 16, N_START)
        dstarts = torch.from_numpy(starts.view(np.int32).reshape(-1, 4).copy()).cuda()
        torch.cuda.synchronize()
        for ms in MAX_STEPS:
            if do_fields:
                arms, keys = [], []
                for nf in FIELDS:
                    for tag, kw in (("static", dict(t_start=-1.0, step_seconds=0.0)), ("scheduled", dict(t_start=0.0, step_seconds=step))):
                        for dev in ((False, True) if fits else (True,)):
                            arms.append(lambda nf=nf, kw=kw, dev=dev: m.build_reach_fields(dsrc[:nf], nf, max_steps=ms, device_sets=dev, **kw))
                            keys.append("inflate%d_steps%d_fields%d_%s_%s" % (r, ms, nf, tag, "device_sets" if dev or not fits else "lds"))
                for k, v in zip(keys, timed(arms, args.reps)):
                    out["build_us_median_min_" + k] = v
                # (b) paths down the static 16-field build
                with torch.cuda.stream(st):
                    m.build_reach_fields(dsrc[:16], 16, max_steps=ms)
                (pm,) = timed([lambda: m.reach_paths(dstarts, 256)], args.reps)
                out["paths_us_median_min_inflate%d_steps%d_%d_starts_max_len_256" % (r, ms, N_START)] = pm
                with torch.cuda.stream(st):
                    steps = m.reach_paths(dstarts, 256)[0]
                    st.synchronize()
                out["paths_reached_fraction_mean_steps_inflate%d_steps%d" % (r, ms)] = [round(float((steps >= 0).float().mean()), 4),
                                                                                       round(float(steps[steps >= 0].float().mean()), 1)]
                # (c) the host route: the grid copy, then the wavefront on the CPU from the same sources -- and the same answer
                for nf in (1, 16):
                    for tag, kw in (("static", dict(t_start=-1.0, step_seconds=0.0)), ("scheduled", dict(t_start=0.0, step_seconds=step))):
                        tc, tg = [], []
                        for _ in range(args.host_reps):
                            t0 = time.perf_counter()
                            grid = m.cast_grid()
                            t1 = time.perf_counter()
                            want, how = host_fields(reach_ref, cfg, reach_ref.unpack(grid, w["nx"]), src[:nf], nf, max_steps=ms, **kw)
                            t2 = time.perf_counter()
                            tc.append((t1 - t0) * 1e3)
                            tg.append((t2 - t1) * 1e3)
                        out["host_ms_copy_wavefront_inflate%d_steps%d_fields%d_%s" % (r, ms, nf, tag)] = [round(float(np.median(tc)), 3), round(float(np.median(tg)), 1)]
                        out["host_wavefront"] = how
                        with torch.cuda.stream(st):
                            m.build_reach_fields(src[:nf], nf, max_steps=ms, **kw)
                            got = m.reach_field(None, nf)
                        assert np.array_equal(got, want), "the device and the host route disagree"
                        out["reached_fraction_inflate%d_steps%d_fields%d_%s" % (r, ms, nf, tag)] = round(float((got != reach_ref.UNREACHED).mean()), 4)
            if not (do_timeline and ms == TIMELINE_STEPS):
                continue
            # (d) the timeline build against the plain build: what the history stores cost
            lw = w["nz"] * w["ny"] * ((w["nx"] + 63) // 64)
            scheds = (("static", dict(t_start=-1.0, step_seconds=0.0)), ("scheduled", dict(t_start=0.0, step_seconds=step)))
            arms, keys = [], []
            for nf in FIELDS:
                kept = nf * (ms + 1) * lw * 8
                if kept > D.capi.REACH_TIMELINE_MAX_BYTES:
                    out["timeline_not_timed_steps%d_fields%d" % (ms, nf)] = "%d bytes of sets exceed DSPMAP_REACH_TIMELINE_MAX_BYTES" % kept
                    continue
                for tag, kw in scheds:
                    for dev in ((False, True) if fits else (True,)):
                        for tl in (False, True):
                            build = m.build_reach_timeline if tl else m.build_reach_fields
                            arms.append(lambda build=build, nf=nf, kw=kw, dev=dev: build(dsrc[:nf], nf, max_steps=ms, device_sets=dev, **kw))
                            keys.append("inflate%d_steps%d_fields%d_%s_%s_%s" % (r, ms, nf, tag, "device_sets" if dev or not fits else "lds",
                                                                               "timeline" if tl else "plain"))
            for k, v in zip(keys, timed(arms, args.reps)):
                out["build_us_median_min_" + k] = v
            # (e) timeline paths through the scheduled 16-field build
            with torch.cuda.stream(st):
                m.build_reach_timeline(dsrc[:16], 16, max_steps=ms, **scheds[1][1])
            (pm,) = timed([lambda: m.reach_timeline_paths(dstarts, ms + 1)], args.reps)
            out["timeline_paths_us_median_min_inflate%d_steps%d_%d_starts_max_len_%d" % (r, ms, N_START, ms + 1)] = pm
            with torch.cuda.stream(st):
                tsteps, tcells = m.reach_timeline_paths(dstarts, ms + 1)
                st.synchronize()
            ok = tsteps >= 0
            waits = ((tcells[:, 1:] == tcells[:, :-1]) & (tcells[:, 1:] >= 0)).any(1)
            out["timeline_paths_reached_fraction_mean_steps_with_a_wait_inflate%d_steps%d" % (r, ms)] = [
                round(float(ok.float().mean()), 4), round(float(tsteps[ok].float().mean()), 1) if bool(ok.any()) else None, int(waits.sum())]
            # (f) the route without the feature, one field: the grid copy, the wavefront with its sets and the backward walk on the host
            one = starts.copy()
            one["field"] = 0
            tc, tg, tw = [], [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                grid = m.cast_grid()
                t1 = time.perf_counter()
                val, sets = reach_ref.fields(cfg, reach_ref.unpack(grid, w["nx"]), src[:1], 1, max_steps=ms, return_sets=True, **scheds[1][1])
                t2 = time.perf_counter()
                want = reach_time_ref.timeline_paths(cfg, val, sets, one, ms + 1)
                t3 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                tg.append((t2 - t1) * 1e3)
                tw.append((t3 - t2) * 1e3)
            out["host_ms_copy_wavefront_walk_inflate%d_steps%d_fields1_scheduled" % (r, ms)] = [round(float(np.median(tc)), 3), round(float(np.median(tg)), 1),
                                                                                               round(float(np.median(tw)), 1)]
            with torch.cuda.stream(st):
                m.build_reach_timeline(src[:1], 1, max_steps=ms, **scheds[1][1])
                got = m.reach_timeline_paths(one, ms + 1)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the device and the host route disagree on the paths"
            out["host_route_paths_reached_inflate%d_steps%d" % (r, ms)] = int((want[0] >= 0).sum())
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20, host_reps=3)
    ap.add_argument("--section", choices=("all", "fields", "timeline"), default="all")
    harness.main(run, ap)


if __name__ == "__main__":
    main()
