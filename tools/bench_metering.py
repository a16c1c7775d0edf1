#!/usr/bin/env python3
"""What an LDR read-out costs with auto exposure off and on (crh_set_auto_exposure: memset + k_luma_histogram + k_meter in front of k_tonemap), on a
BASELINE config at its full resolution after a few rendered frames:

  read_ldr_ms                 crh_read_ldr (tone map + copy of the frame to the host + wait), median / min of --trials, auto exposure off / on
  read_ldr_constant_image_ms  the same on a constant image: every lane of every wavefront of k_luma_histogram hits ONE LDS word (the contention case)
  measure_exposure_ms         crh_measure_exposure alone (histogram + rule + a 1 KB copy + wait)
  displayed_frames_per_s      crh_render(1) + asynchronous LDR read-back two frames behind (tools/bench_redraw.py's displayed loop), off / on

  python tools/bench_metering.py [--config C3] [--trials 15] [--frames 128] [--off-only]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_metering.py --trials 5 --frames 16` in a run of its own.
--off-only touches none of the new entry points: the same figures from a library built before they existed (CRH_LIB_PATH)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def displayed(v, frames, shown):
    for loop in ("warm", "timed"):
        n = 8 if loop == "warm" else frames
        v.sync()
        t = time.perf_counter()
        for i in range(n):
            v.Redraw()
            if i >= 2: v.read_ldr_end(shown)
            v.read_ldr_begin()
        v.read_ldr_end(shown); v.read_ldr_end(shown); v.sync()
        dt = time.perf_counter() - t
    return round(frames / dt, 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View
    sc = scenes.baseline_config(a.config)
    v = View(0).load_scene(sc)
    modes = ("off",) if a.off_only else ("off", "on")
    out = {"config": a.config, "width": v.width, "height": v.height, "trials": a.trials, "read_ldr_ms": {}, "read_ldr_constant_image_ms": {}, "displayed_frames_per_s": {}}
    for _ in range(8): v.Redraw()
    v.sync()
    if not a.off_only:
        m = v.measure_exposure()
        out["metered"] = {"exposure": float(m["exposure"]), "white_point": float(m["white_point"]), "white_bin": m["white_bin"], "n_lit": m["n_lit"], "n_unsampled": m["n_unsampled"],
                          "bins_in_use": int(np.count_nonzero(m["hist"]))}
        v.read_ldr()
        out["measure_exposure_ms"] = timed(v.measure_exposure, a.trials)
    for mode in modes:
        if not a.off_only: v.set_auto_exposure(mode == "on")
        v.read_ldr(); v.read_ldr()
        out["read_ldr_ms"][mode] = timed(v.read_ldr, a.trials)
    # the displayed loop (the frame tuning of the first frames after a build settles first, as in tools/bench_redraw.py)
    for _ in range(96):
        ft = v.frame_tuning(); v.tile_order()
        if (not ft["enabled"] or ft["feeders"]) and v.tile_order_calls["verdict"] != 0: break
        v.reset(); v.Redraw(); v.sync()
    shown = np.empty((v.height, v.width, 3), np.uint8)
    for mode in modes:
        if not a.off_only: v.set_auto_exposure(mode == "on")
        out["displayed_frames_per_s"][mode] = displayed(v, a.frames, shown)
    # the contention case
    const = np.zeros((v.height, v.width, 4), np.float32); const[..., :3] = 0.5; const[..., 3] = 8
    v.load_accum(const, 8)
    for mode in modes:
        if not a.off_only: v.set_auto_exposure(mode == "on")
        v.read_ldr(); v.read_ldr()
        out["read_ldr_constant_image_ms"][mode] = timed(v.read_ldr, a.trials)
    print(json.dumps(out), flush=True)
