#!/usr/bin/env python3
"""What a region query costs (crh_query_region: one pass over the first-hit id buffer on the device, region_kernels.hip), on a BASELINE config.
C3 is measured twice: as ONE object (every wavefront of the chip meets the same record) and as the 27 objects of tools/bench_visibility.py.  Per form:

  first_call_ms      the first crh_query_region after a restart: the id pass (rays, traversal, resolve), then the kernel
  whole_frame_ms     a query on the valid buffer (edge upload + memset + kernel + 32 B per object back + wait), median / min of --trials; likewise
  quarter_rect_ms    the rectangle over the middle quarter of the frame
  lasso_256_ms       a 256-vertex lasso around the frame
  read_ids_plus_host_twin_ms   what a host had to do before: crh_read_ids + crh_region_stats_host on one thread, the three regions in turn

  python tools/bench_region.py [--config C3|CAD1M] [--trials 15] [--host-trials 3]
Kernel time: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_region.py --trials 5 --host-trials 0` in a run of its own and read k_region_stats."""
import argparse, dataclasses, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def lasso(W, H, n=256):
    """n vertices on an ellipse that nearly fills the frame, radius wobbling so that no two edges are parallel"""
    import numpy as np
    a = 2 * np.pi * np.arange(n) / n
    r = 0.9 + 0.08 * np.cos(7 * a)
    return np.stack([np.rint(W / 2 + r * (W / 2) * np.cos(a)), np.rint(H / 2 + r * (H / 2) * np.sin(a))], 1).astype(np.int32)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--host-trials", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View, region_stats_host
    base = scenes.baseline_config(a.config)
    forms = [("as_handed_over", base)]
    if a.config == "C3":                                       # the 27 objects of tools/bench_visibility.py
        cen = base.pos.reshape(-1, 3, 3).mean(1)
        cell = np.clip(((cen + 1.0) * 0.5 * 3).astype(np.int32), 0, 2)
        obj = ((cell[:, 0] * 3 + cell[:, 1]) * 3 + cell[:, 2]).astype(np.int32)
        forms.append(("27_objects", dataclasses.replace(base, tri_object=obj, obj_xform=np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (27, 1)))))
    for name, sc in forms:
        v = View(0).load_scene(sc)
        v.Redraw(); v.sync()
        W, H = v.width, v.height
        nO = 1 if sc.tri_object is None else len(sc.obj_xform)
        regions = {"whole_frame": (None, None), "quarter_rect": ((W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2), None), "lasso_256": (None, lasso(W, H))}
        firsts = []
        for _ in range(max(a.trials // 3, 1)):                 # a restart invalidates the id buffer
            v.reset(); v.sync()
            t = time.perf_counter(); v.query_region(nO); firsts.append((time.perf_counter() - t) * 1e3)
        out = {"config": a.config, "form": name, "width": W, "height": H, "n_objects": nO,
               "first_call_ms": {"median": round(statistics.median(firsts), 4), "min": round(min(firsts), 4)}}
        got = {}
        for rn, (rect, poly) in regions.items():
            got[rn] = v.query_region(nO, rect, poly)
            out[rn + "_ms"] = timed(lambda: v.query_region(nO, rect, poly), a.trials)
        whole = got["whole_frame"]
        out["visible_objects"] = int((whole["pixels_frame"][:nO] > 0).sum()); out["background_pixels"] = int(whole["pixels_frame"][nO])
        out["pixels_in_quarter_rect"] = int(got["quarter_rect"]["pixels"].sum()); out["pixels_in_lasso"] = int(got["lasso_256"]["pixels"].sum())
        if a.host_trials > 0:
            twin = {}
            def run_host():
                ob, _, t = v.read_ids()
                for rn, (rect, poly) in regions.items():
                    twin[rn] = region_stats_host(ob, t, nO, rect, poly)
            out["read_ids_plus_host_twin_ms"] = timed(run_host, a.host_trials)
            ob, _, t = v.read_ids()
            out["read_ids_ms"] = timed(lambda: v.read_ids(), a.host_trials)
            out["host_twin_whole_frame_ms"] = timed(lambda: region_stats_host(ob, t, nO), a.host_trials)
            out["host_twin_lasso_256_ms"] = timed(lambda: region_stats_host(ob, t, nO, None, regions["lasso_256"][1]), a.host_trials)
            out["device_equals_host_twin"] = bool(all(got[rn].tobytes() == twin[rn].tobytes() for rn in regions))
        print(json.dumps(out), flush=True)
        v.close()
