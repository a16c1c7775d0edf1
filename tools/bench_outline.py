#!/usr/bin/env python3
"""What the feature lines cost (crh_set_outline: object, depth and crease edges over the LDR read-out, outline_kernels.hip), on a BASELINE
config at its full resolution.  One JSON line:

  first_read_out_after_a_restart_ms   crh_reset + crh_render(1), then the first crh_read_ldr with lines: the id pass, (once) the table, the mask, the drawing
  table_first_use_ms                  the first crh_read_outline after crh_build less a later one that only recomputes the mask: building and uploading the table
  read_ldr_off_ms / read_ldr_cached_mask_ms / read_ldr_fresh_mask_ms
                                      crh_read_ldr with the feature off; on with the mask of the frame kept; on after a change of crease_cos (the mask alone is
                                      recomputed: the id buffer stays valid)
  read_outline_ms                     crh_read_outline on the valid mask: W * H bytes back
  displayed_frames_per_s_off / _on    the displayed loop of tools/bench_redraw.py (crh_render(1) + asynchronous LDR read-back two frames behind), lines off / on
  device_equals_host_twin             crh_read_outline == crh_outline_mask_host over the planes of crh_read_ids and the table of the scene's geometry

  python tools/bench_outline.py [--config C3|CAD1M] [--trials 15] [--frames 128]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_outline.py --trials 5 --frames 16` in a run of its own and read k_outline_mask
and k_outline_draw (the fresh-mask read-outs launch both, the cached ones only the drawing)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def timed(fn, trials, before=None):
    ts = []
    for _ in range(trials):
        if before: before()
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def displayed(v, frames):
    import numpy as np
    shown = np.empty((v.height, v.width, 3), np.uint8)
    for n in (8, frames):
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
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View, outline_mask_host, outline_table_host
    sc = scenes.baseline_config(a.config)
    v = View(0).load_scene(sc)
    v.Redraw(); v.sync()
    W, H = v.width, v.height
    out = {"config": a.config, "width": W, "height": H, "n_triangles": int(len(sc.tri))}
    t = time.perf_counter(); v.read_outline(); first = (time.perf_counter() - t) * 1e3           # id pass + table + mask
    def restart():
        v.reset(); v.Redraw(); v.sync()
    ids_and_mask = timed(v.read_outline, max(a.trials // 3, 1), restart)                            # id pass + mask
    out["first_read_outline_after_build_ms"] = round(first, 4)
    out["read_outline_after_a_restart_ms"] = ids_and_mask
    out["table_first_use_ms"] = round(first - ids_and_mask["median"], 4)
    out["read_outline_ms"] = timed(v.read_outline, a.trials)
    out["read_ldr_off_ms"] = timed(v.read_ldr, a.trials)
    v.SetOutline()
    out["first_read_out_after_a_restart_ms"] = timed(v.read_ldr, max(a.trials // 3, 1), restart)
    out["read_ldr_cached_mask_ms"] = timed(v.read_ldr, a.trials)
    flip = [0]
    def other_threshold():
        flip[0] ^= 1
        v.SetOutline(crease_deg=30.0 + flip[0])
    out["read_ldr_fresh_mask_ms"] = timed(v.read_ldr, a.trials, other_threshold)
    v.SetOutline()
    mask = v.read_outline()
    out["line_pixels"] = {k: int(((mask & b) != 0).sum()) for k, b in (("object", 1), ("depth", 2), ("crease", 4), ("any", 7))}
    ob, tr, tt = v.read_ids()
    out["pairs_whose_triangles_differ"] = int((tr[:, 1:] != tr[:, :-1]).sum() + (tr[1:] != tr[:-1]).sum())
    t = time.perf_counter(); tab = outline_table_host(sc.pos, sc.tri); out["table_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    t = time.perf_counter(); twin = outline_mask_host(ob, tr, tt, tab); out["mask_host_twin_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["device_equals_host_twin"] = bool(np.array_equal(mask, twin))
    v.ClearOutline(); v.reset()
    out["displayed_frames_per_s_off"] = displayed(v, a.frames)
    v.SetOutline(); v.reset()
    out["displayed_frames_per_s_on"] = displayed(v, a.frames)
    v.ClearOutline(); v.reset()
    out["displayed_frames_per_s_off_again"] = displayed(v, a.frames)
    print(json.dumps(out), flush=True)
    v.close()
    sys.exit(0 if out["device_equals_host_twin"] else 1)
