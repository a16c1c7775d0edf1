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

  python tools/bench_reproject.py [--config C3|CAD1M] [--trials 15] [--frames 128] [--rounds 5] [--repeats 20] [--truth 512]

--drag object: the MANIPULATOR loop instead (crh_set_reproject_motion: per-object history deltas).  The config's triangles are grouped into 4 x 4 x 4 objects by
their centroid's cell; the part with the most pixels under the camera is translated along x by 0.002 of the scene's extent per frame (crh_set_transforms + one
frame of 1 spp + read-out).  One JSON line:

  resolve_ms.*                        k_reproject_resolve (crh_bench_reproject) against k_reproject_resolve_motion (crh_bench_reproject_motion) per launch, in the same
                                      process: with no record flagged (where read-outs launch the plain kernel: n_flagged == 0 is asserted; the motion figure is the
                                      all-objects-flagged stand-in, the worst case for fetches) and with the one part flagged
                                      (CRH_REPROJECT_STAGED=1 in the environment: the LDS-staged form of the motion kernel; --launch-only stops here)
  object_drag_frames_per_s.*          the loop with both features off / on / off again, `--rounds` interleaved rounds: median and range
  mse                                 per static cap 2 / 4 / 8 / 16 and after 1 / 4 / 8 / 16 steps: error of the displayed image against `--truth` spp of the final
                                      placement as a fraction of the raw 1-spp image's, separately over the moved part's pixels and over the static pixels"""
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


def grouped(sc, G=4):
    """the config with its triangles grouped into G^3 objects by the cell of their centroid, every object at the identity; the scene's extent"""
    import dataclasses
    import numpy as np
    cen = sc.pos[sc.tri[:, :3]].mean(1)
    lo, hi = sc.pos.min(0), sc.pos.max(0)
    cell = np.clip(((cen - lo) / np.maximum(hi - lo, 1e-30) * G).astype(np.int32), 0, G - 1)
    ids, inv = np.unique((cell[:, 0] * G + cell[:, 1]) * G + cell[:, 2], return_inverse=True)
    xf = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (len(ids), 1))
    return dataclasses.replace(sc, tri_object=inv.astype(np.int32), obj_xform=xf), float((hi - lo).max())


def object_drag(a):
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd import scenes
    from cadrays_amd.view import View
    sc, extent = grouped(scenes.baseline_config(a.config))
    n_obj = len(sc.obj_xform)
    v = View(0).load_scene(sc)
    W, H = v.width, v.height
    out = {"config": a.config, "drag": "object", "n_triangles": int(len(sc.tri)), "n_objects": n_obj, "width": W, "height": H}
    shown = np.empty((H, W, 3), np.uint8)
    for _ in range(40):
        v.reset(); v.Redraw(); v.sync()
    ob, tr, _ = v.read_ids()
    part = int(np.bincount(ob[tr >= 0], minlength=n_obj).argmax())
    out["part"], out["part_pixels"] = part, int(((ob == part) & (tr >= 0)).sum())

    def place(k):
        xf = sc.obj_xform.copy(); xf[part, 3] = np.float32(0.002 * extent * k)
        return xf

    def both(on, **caps):
        if on: v.SetReproject(); v.SetReprojectMotion(**caps)
        else: v.ClearReprojectMotion(); v.ClearReproject()

    # ---- per launch
    both(True)
    v.Redraw(); v.read_ldr()
    v.set_camera(drag_camera(sc.camera, 1)); v.reset(); v.Redraw(); v.read_ldr()
    g = v.get_reproject_motion()
    assert v.get_reproject()["history_valid"] and g["on"] and g["n_flagged"] == 0      # no flagged record: read-outs and captures launch k_reproject_resolve
    n0 = v.get_reproject_launches()
    v.read_ldr(); v.read_reprojected()
    n1 = v.get_reproject_launches()
    assert n1["motion"] == n0["motion"] == 0 and n1["plain"] == n0["plain"] + 2      # ... and they did: the new kernel has never been launched
    v.bench_reproject(2); v.bench_reproject_motion(2)
    out["resolve_ms"] = {"none_flagged": {"plain": round(v.bench_reproject(a.repeats)["resolve_ms"], 4), "motion_all_flagged_stand_in": round(v.bench_reproject_motion(a.repeats)["resolve_ms"], 4)}}
    v.set_transforms(place(1)); v.Redraw(); v.read_ldr()
    assert v.get_reproject_motion()["n_flagged"] == 1
    out["resolve_ms"]["one_flagged"] = {"plain": round(v.bench_reproject(a.repeats)["resolve_ms"], 4), "motion": round(v.bench_reproject_motion(a.repeats)["resolve_ms"], 4)}
    out["staged"] = os.environ.get("CRH_REPROJECT_STAGED", "0")      # the motion kernel's form: read by the library when the context is created
    if a.launch_only:
        print(json.dumps(out), flush=True)
        v.close()
        return
    both(False); v.set_camera(sc.camera); v.set_transforms(place(0))

    # ---- the manipulator loop, interleaved
    def loop(frames):
        for n in (8, frames):
            v.sync()
            t = time.perf_counter()
            for i in range(n):
                v.set_transforms(place(i % 32)); v.Redraw()
                if i >= 2: v.read_ldr_end(shown)
                v.read_ldr_begin()
            v.read_ldr_end(shown); v.read_ldr_end(shown); v.sync()
            dt = time.perf_counter() - t
        return frames / dt
    rates = {"off": [], "on": [], "off_again": []}
    for _ in range(0 if a.mse_only else a.rounds):
        for key in rates:
            both(key == "on")
            rates[key].append(loop(a.frames))
    if not a.mse_only:
        out["object_drag_frames_per_s"] = {k: spread(x) for k, x in rates.items()}
    # ---- what it buys, per static cap
    out["mse"] = {"truth_spp": a.truth}
    for steps in (1, 4, 8, 16):
        truth, rec = None, {}
        for cap in (2.0, 4.0, 8.0, 16.0):
            both(False)                                          # the drag starts WITHOUT a history
            v.set_transforms(place(0))
            both(True, max_history_static=cap)
            v.Redraw(); v.read_ldr()
            for k in range(1, steps + 1):
                v.set_transforms(place(k)); v.Redraw(); v.read_ldr()
            raw = v.read_hdr().astype(np.float64)
            rep = v.read_reprojected()[..., :3].astype(np.float64)
            if truth is None:
                ob, tr, _ = v.read_ids()
                moved, static = (tr >= 0) & (ob == part), (tr >= 0) & (ob != part)
                v.render(a.truth - 1)
                truth = v.read_hdr().astype(np.float64)
                e = lambda img, m: float(((img - truth)[m] ** 2).mean())
                rec.update(moved_pixels=int(moved.sum()), static_pixels=int(static.sum()), raw_moved=round(e(raw, moved), 6), raw_static=round(e(raw, static), 6))
            rec[f"static_cap_{int(cap)}"] = {"moved": round(e(rep, moved) / e(raw, moved), 4), "static": round(e(rep, static) / e(raw, static), 4)}
        out["mse"][str(steps)] = rec
    print(json.dumps(out), flush=True)
    v.close()


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
    ap.add_argument("--launch-only", action="store_true", help="--drag object: the per-launch figures only (run once per CRH_REPROJECT_STAGED=0 / 1 to compare the two forms)")
    ap.add_argument("--drag", default="camera", choices=["camera", "object"], help="object: the manipulator loop with the per-object history deltas")
    a = ap.parse_args()
    if a.drag == "object":
        object_drag(a)
        sys.exit(0)
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
