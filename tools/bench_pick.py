#!/usr/bin/env python3
"""What picking costs (crh_pick.cpp), on a BASELINE config at its full resolution.  The application calls MoveTo on every mouse move
(AppViewer.cxx:347) and Select on a click (:359-455); the library answers both from the first-hit id buffer.

  id_pass_ms              the buffer computed from scratch: crh_reset (invalidates it) + crh_pick, host clock, median / min of --trials
                          (ray generation + traversal + resolve + the 16-byte copy; kernel times alone: rocprofv3 --kernel-trace --stats around this tool)
  trace_nearest_same_rays_ms   crh_bench_trace of the very same rays in pixel order (device events, traversal kernel alone)
  pick_from_valid_buffer_us    crh_pick served from the valid buffer, mean of 1000 calls
  read_ldr_ms / read_ldr_overlay_ms   the synchronous LDR read-out without / with a selection and a hover (tone map + overlay + copy)
  drag_frames_per_s / drag_with_moveto_frames_per_s   tools/bench_redraw.py's drag loop, plain and with a MoveTo per frame (the application's mouse-move regime)

  python tools/bench_pick.py [--config C3] [--frames 128] [--trials 15]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np


def drag(v, cam0, frames, moveto):
    from bench_redraw import drag_camera
    W, H = v.width, v.height
    shown = np.empty((H, W, 3), np.uint8)
    for loop in ("warm", "timed"):
        n = 8 if loop == "warm" else frames
        v.sync()
        t = time.perf_counter()
        for i in range(n):
            v.set_camera(drag_camera(cam0, i)); v.reset()
            if moveto: v.MoveTo((W // 2 + 3 * i) % W, H // 2)
            v.Redraw()
            if i >= 2: v.read_ldr_end(shown)
            v.read_ldr_begin()
        v.read_ldr_end(shown); v.read_ldr_end(shown); v.sync()
        dt = time.perf_counter() - t
    return round(frames / dt, 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--trials", type=int, default=15)
    a = ap.parse_args()
    import torch  # noqa: F401
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from cadrays_amd import scenes
    from cadrays_amd.view import View
    sc = scenes.baseline_config(a.config)
    v = View(0).load_scene(sc)
    W, H = v.width, v.height
    out = {"config": a.config, "width": W, "height": H, "triangles": int(len(sc.tri))}
    for _ in range(4): v.Redraw()
    v.sync(); v.pick(0, 0)
    ts = []
    for _ in range(a.trials):
        v.reset(); v.sync()
        t = time.perf_counter(); v.pick(W // 2, H // 2); ts.append(1e3 * (time.perf_counter() - t))
    out["id_pass_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3)}
    ys, xs = np.mgrid[0:H, 0:W]
    rays = v.camera_rays(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32))
    out["trace_nearest_same_rays_ms"] = round(v.bench_trace(rays, False, 10), 3)
    ob = v.read_ids()[0]
    out["hit_share"] = round(float((ob >= 0).mean()), 4)
    t = time.perf_counter()
    for i in range(1000): v.pick((17 * i) % W, (29 * i) % H)
    out["pick_from_valid_buffer_us"] = round(1e3 * (time.perf_counter() - t), 2)
    def ldr_ms():
        v.read_ldr(); ts = []
        for _ in range(a.trials):
            t = time.perf_counter(); v.read_ldr(); ts.append(1e3 * (time.perf_counter() - t))
        return round(statistics.median(ts), 3)
    out["read_ldr_ms"] = ldr_ms()
    v.set_selection(np.ones(v._n_objects, np.uint8), (255, 160, 0), 64); v.set_hover(0, (0, 255, 255), 32)
    out["read_ldr_overlay_ms"] = ldr_ms()
    v.set_selection(None); v.set_hover(-1)
    out["drag_frames_per_s"] = [drag(v, sc.camera, a.frames, False) for _ in range(3)]
    out["drag_with_moveto_frames_per_s"] = [drag(v, sc.camera, a.frames, True) for _ in range(3)]
    v.set_hover(-1)
    print(json.dumps(out))
