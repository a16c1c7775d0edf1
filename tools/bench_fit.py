#!/usr/bin/env python3
"""What fitting the view costs (crh_fit_view: one pass over the vertices on the device, fit_kernels.hip), on a BASELINE config:

  first_call_ms     the first crh_fit_view after crh_build: the {x, y, z, object} array is built on the host and uploaded, then the kernel
  resident_call_ms  a repeated call with the array resident (object table upload + memset + kernel + 32 B per object back + wait), median / min of --trials
  host_twin_ms      crh_fit_extents_host over the same vertices on one host thread, median / min of --host-trials

  python tools/bench_fit.py [--config C3|CAD1M] [--trials 15] [--host-trials 3]
Kernel time: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_fit.py --trials 5` in a run of its own and read k_fit_extents."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--host-trials", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.01)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View, fit_extents_host
    sc = scenes.baseline_config(a.config)
    v = View(0).load_scene(sc)
    v.sync()
    n_objects = 1 if sc.tri_object is None else len(sc.obj_xform)
    t = time.perf_counter()
    cam, res = v.fit_view(n_objects, None, a.margin, want_extents=True)
    first = (time.perf_counter() - t) * 1e3
    out = {"config": a.config, "n_vertices": int(len(sc.pos)), "n_triangles": int(len(sc.tri)), "n_objects": n_objects, "contributing_vertices": res["n_vertices"],
           "first_call_ms": round(first, 4), "resident_call_ms": timed(lambda: v.fit_view(n_objects, None, a.margin), a.trials)}
    # the host twin over the array the library builds (built here the same way), one thread
    owner = np.full(len(sc.pos), -1, np.int32)
    for k in range(3):
        owner[sc.tri[:, k]] = 0 if sc.tri_object is None else sc.tri_object
    v4 = np.concatenate([np.asarray(sc.pos, np.float32), owner.view(np.float32)[:, None]], 1)
    host = [None]
    def run_host():
        host[0] = fit_extents_host(v4, n_objects, sc.camera, v.width, v.height, a.margin, sc.obj_xform)
    out["host_twin_ms"] = timed(run_host, a.host_trials)
    out["device_equals_host_twin"] = bool(np.array_equal(host[0][0].view(np.uint32), res["object_extents"].view(np.uint32)))
    out["fitted_eye"] = [float(x) for x in cam["eye"]]; out["z_near"] = float(res["z_near"]); out["z_far"] = float(res["z_far"]); out["binding"] = res["binding"]
    print(json.dumps(out), flush=True)
    v.close()
