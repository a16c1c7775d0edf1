#!/usr/bin/env python3
"""What the reprojected display history costs and what it buys (crh_set_reproject: the image the ending view displayed, fetched through the first-hit points and blended
with the new accumulator in front of the denoise filter; reproject_kernels.hip), on a BASELINE config at its full resolution.  One JSON line:

  resolve_ms / capture_ms             device time per launch of k_reproject_resolve as a read-out runs it, and of what crh_set_camera's capture enqueues (the resolve
                                      into a history image + the copy of the guide planes), against a history one drag step old (HIP events around `--repeats`
                                      launches: crh_bench_reproject)
  resolve_gb_per_s / capture_gb_per_s W * H * 96 B -- accumulator 16, guide 24, every history record once 16 + 24, the write 16: a LOWER bound -- and + 48 B for the
                                      guide copy, over those times
  read_ldr_ms.off / on / off_again    a lone synchronous LDR read-out of a view with a valid history (host clock around a call that ends in a synchronise)
  drag_frames_per_s.*                 the drag loop of tools/bench_redraw.py (crh_set_camera + crh_reset + crh_render(1) + asynchronous LDR read-back two frames
                                      behind), feature off / on / off again, in `--rounds` interleaved rounds: median and range
  displayed_frames_per_s.*            its displayed loop (a still camera: the history is passed through only until until_samples), likewise
  mse                                 after 1, 4 and 16 drag steps of 1 spp each: mean squared error over the hit pixels of the last view against `--truth` spp of
                                      it -- raw, reprojected, filtered alone (crh_set_denoise defaults) and both together

  python tools/bench_reproject.py [--config C3|CAD1M] [--trials 15] [--frames 128] [--rounds 5] [--repeats 20] [--truth 512]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
from tools.bench_redraw import drag_camera  # noqa: E402


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def loop(v, frames, cam_of, shown):
    """frames per second of: [camera change + restart] + one frame + asynchronous LDR read-back, collected two frames later"""
    for n in (8, frames):
        v.sync()
        t = time.perf_counter()
        for i in range(n):
            if cam_of is not None:
                v.set_camera(cam_of(i)); v.reset()
            v.Redraw()
            if i >= 2: v.read_ldr_end(shown)
            v.read_ldr_begin()
        v.read_ldr_end(shown); v.read_ldr_end(shown); v.sync()
        dt = time.perf_counter() - t
    return frames / dt


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--truth", type=int, default=512)
    ap.add_argument("--mse-only", action="store_true", help="skip the drag and displayed loops")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View
    sc = scenes.baseline_config(a.config)
    cam0 = sc.camera
    v = View(0).load_scene(sc)
    W, H = v.width, v.height
    out = {"config": a.config, "n_triangles": int(len(sc.tri)), "width": W, "height": H}
    shown = np.empty((H, W, 3), np.uint8)
    for _ in range(40):                                          # let the library's own measurements after a build settle (tools/bench_redraw.py)
        v.reset(); v.Redraw(); v.sync()

    def step(i):
        v.set_camera(drag_camera(cam0, i)); v.reset(); v.Redraw()

    # ---- per launch
    v.SetReproject()
    step(0); v.read_ldr(); step(1); v.read_ldr()
    assert v.get_reproject()["history_valid"]
    v.bench_reproject(2)
    b = v.bench_reproject(a.repeats)
    out["resolve_ms"], out["capture_ms"] = round(b["resolve_ms"], 4), round(b["capture_ms"], 4)
    out["resolve_gb_per_s"] = round(W * H * 96 / (b["resolve_ms"] * 1e-3) / 1e9, 1)
    out["capture_gb_per_s"] = round(W * H * 144 / (b["capture_ms"] * 1e-3) / 1e9, 1)
    # ---- a lone read-out
    out["read_ldr_ms"] = {"on": timed(v.read_ldr, a.trials)}
    v.ClearReproject()
    out["read_ldr_ms"]["off"] = timed(v.read_ldr, a.trials)
    v.SetReproject(); step(2); step(3)
    out["read_ldr_ms"]["on_again"] = timed(v.read_ldr, a.trials)
    v.ClearReproject()
    # ---- the loops, interleaved
    drag = {"off": [], "on": [], "off_again": []}
    disp = {"off": [], "on": [], "off_again": []}
    for _ in range(0 if a.mse_only else a.rounds):
        for key in ("off", "on", "off_again"):
            if key == "on": v.SetReproject()
            else: v.ClearReproject()
            drag[key].append(loop(v, a.frames, lambda i: drag_camera(cam0, i), shown))
            v.set_camera(cam0); v.reset()
            disp[key].append(loop(v, a.frames, None, shown))
    if not a.mse_only:
        out["drag_frames_per_s"] = {k: spread(x) for k, x in drag.items()}
        out["displayed_frames_per_s"] = {k: spread(x) for k, x in disp.items()}
    # ---- what it buys
    out["mse"] = {"truth_spp": a.truth}
    for steps in (1, 4, 16):
        v.ClearDenoise(); v.ClearReproject()                     # the drag starts WITHOUT a history: the converged image of the previous round must not seed it
        v.set_camera(drag_camera(cam0, 0)); v.reset()
        v.SetReproject()
        v.Redraw(); v.read_ldr()
        for i in range(1, steps + 1):
            step(i); v.read_ldr()
        hit = v.read_ids()[1] >= 0
        raw = v.read_hdr().astype(np.float64)
        rep = v.read_reprojected()[..., :3].astype(np.float64)
        v.SetDenoise()
        both = v.read_denoised()[..., :3].astype(np.float64)
        v.ClearReproject()
        filt = v.read_denoised()[..., :3].astype(np.float64)
        v.ClearDenoise()
        v.render(a.truth - 1)
        truth = v.read_hdr().astype(np.float64)
        e = lambda img: float(((img - truth)[hit] ** 2).mean())
        e_raw = e(raw)
        out["mse"][str(steps)] = {"hit_pixels": int(hit.sum()), "raw": round(e_raw, 6), "reprojected": round(e(rep) / e_raw, 4), "filtered": round(e(filt) / e_raw, 4),
                                  "reprojected_and_filtered": round(e(both) / e_raw, 4)}
    print(json.dumps(out), flush=True)
    v.close()
