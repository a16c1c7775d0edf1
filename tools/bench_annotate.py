#!/usr/bin/env python3
"""What the annotations cost (crh_set_annotations: world-space segments projected, binned and drawn by the LDR read-outs as the last stage of the display chain;
annotate_kernels.hip), on a BASELINE config at 1920 x 1080 and 3840 x 2160.  One JSON line.

  loads                               "viewer": a 41-line grid, the axes, the light markers and the selection's box; "boxes": the edges of 4096 boxes; "random":
                                      65536 random segments through the scene's bounds
  kernel_ms.<size>.<load>             device time per launch of the three kernels (crh_bench_annotations, HIP events around `--repeats` launches): project, bin, draw
  read_ms.<size>.<load>               wall time of a lone synchronous crh_read_ldr with the list in force, and with the feature off before and after
  displayed_frames_per_s.<size>       a 1-spp loop (crh_render(1) + asynchronous read-back collected two frames later): off, on (the viewer's load), off again
  off_vs_parent                       --parent-lib PATH: the "off" loop in fresh processes, this library and the parent's in turn, `--runs` each (at least 3): the
                                      spread of the parent's own runs is what the difference must lie within -- with the feature off nothing is launched

  The tile edge and the binning form are read from the environment when a context is created (CRH_ANNOT_TILE=8|16|32, CRH_ANNOT_BIN=gather|scatter, unset: by the list's length): one run each.

  python tools/bench_annotate.py [--config C3|CAD1M] [--sizes 1080p,2160p] [--loads viewer,boxes,random] [--repeats 20] [--trials 9] [--frames 96]
                                 [--parent-lib PATH --runs 3] [--loop-only]"""
import argparse, json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def loop(v, frames, shown):
    """frames per second of: one frame + asynchronous LDR read-back, collected two frames later"""
    for n in (6, frames):
        v.sync()
        t = time.perf_counter()
        for i in range(n):
            v.Redraw()
            if i >= 2: v.read_ldr_end(shown)
            v.read_ldr_begin()
        v.read_ldr_end(shown); v.read_ldr_end(shown); v.sync()
        dt = time.perf_counter() - t
    return round(frames / dt, 1)


def loads(sc, np, an):
    lo, hi = sc.pos.min(0).astype(np.float64), sc.pos.max(0).astype(np.float64)
    c, size = (lo + hi) / 2, float((hi - lo).max())
    r = np.random.default_rng(1)
    viewer = an.join(an.grid((c[0], c[1], lo[2]), (1, 0, 0), (0, 1, 0), size / 40, 20), an.axes(c, size / 4), an.light_markers(sc.lights, size / 50, anchor=c),
                     an.box(c - size / 8, c + size / 8))
    centres = r.uniform(lo, hi, (4096, 3)); half = r.uniform(size / 400, size / 80, (4096, 1))
    boxes = an.join(*[an.box(p - h, p + h, mode=m) for p, h, m in zip(centres, half, r.integers(0, 3, 4096))])
    a = r.uniform(lo, hi, (65536, 3))
    rnd = an.segments(a, a + r.normal(0, size / 20, (65536, 3)))
    rnd["rgb"] = r.integers(0, 256, (65536, 3)); rnd["alpha"] = r.integers(0, 256, 65536); rnd["style"] = r.integers(1, 4, 65536) | (r.integers(0, 3, 65536) << 8)
    return {"viewer": viewer, "boxes": boxes, "random": rnd}


def settled_view(sc):
    from cadrays_amd.view import View
    v = View(0).load_scene(sc)
    for _ in range(40):                                          # let the library's own measurements after a build settle (tools/bench_redraw.py)
        v.reset(); v.Redraw(); v.sync()
    return v


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--sizes", default="1080p,2160p")
    ap.add_argument("--loads", default="viewer,boxes,random")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trials", type=int, default=9)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--n-tris", type=int, default=None, help="triangles of the config's scene (default: the config's own)")
    ap.add_argument("--parent-lib", default=None, help="libcadrays_hip.so of the parent commit: the off loop of both libraries in fresh processes, in turn")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--loop-only", action="store_true", help="the displayed-frames loop with the feature off, at the first size; nothing else (what --parent-lib starts)")
    a = ap.parse_args()
    import dataclasses
    import numpy as np
    from cadrays_amd import annotations as an, scenes
    sizes = [s for s in a.sizes.split(",") if s]
    sc0 = scenes.baseline_config(a.config, n_tris=a.n_tris)
    out = {"config": a.config, "n_triangles": int(len(sc0.tri)), "tile": os.environ.get("CRH_ANNOT_TILE", "16"), "bin": os.environ.get("CRH_ANNOT_BIN", "by length")}
    if a.loop_only:
        W, H = SIZES[sizes[0]]
        v = settled_view(dataclasses.replace(sc0, params=dataclasses.replace(sc0.params, width=W, height=H)))
        print(json.dumps({"frames_per_s_off": loop(v, a.frames, np.empty((H, W, 3), np.uint8))}), flush=True)
        v.close()
        sys.exit(0)
    lists = {k: l for k, l in loads(sc0, np, an).items() if k in a.loads.split(",")}
    out["segments"] = {k: int(len(l)) for k, l in lists.items()}
    out["kernel_ms"], out["read_ms"], out["displayed_frames_per_s"] = {}, {}, {}
    for size in sizes:
        W, H = SIZES[size]
        v = settled_view(dataclasses.replace(sc0, params=dataclasses.replace(sc0.params, width=W, height=H)))
        shown = np.empty((H, W, 3), np.uint8)
        out["kernel_ms"][size], out["read_ms"][size] = {}, {"off": timed(v.read_ldr, a.trials)}
        for name, segs in lists.items():
            v.SetAnnotations(segs)
            v.BenchAnnotations(2)
            out["kernel_ms"][size][name] = {k: round(x, 4) for k, x in v.BenchAnnotations(a.repeats).items()}
            out["read_ms"][size][name] = timed(v.read_ldr, a.trials)
            out["kernel_ms"][size][name]["pixels_drawn"] = int((v.ReadAnnotationIds() >= 0).sum())
        v.ClearAnnotations()
        out["read_ms"][size]["off_again"] = timed(v.read_ldr, a.trials)
        fps = {"off": loop(v, a.frames, shown)}
        if "viewer" in lists:
            v.SetAnnotations(lists["viewer"]); fps["on"] = loop(v, a.frames, shown); v.ClearAnnotations()
        fps["off_again"] = loop(v, a.frames, shown)
        out["displayed_frames_per_s"][size] = fps
        v.close()
    if a.parent_lib:
        here = os.path.abspath(__file__)
        runs = {"this": [], "parent": []}
        for _ in range(max(a.runs, 3)):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                env = dict(os.environ)
                env.pop("CRH_LIB_PATH", None)
                if lib: env["CRH_LIB_PATH"] = os.path.abspath(lib)
                cmd = [sys.executable, here, "--config", a.config, "--sizes", sizes[0], "--frames", str(a.frames), "--loop-only"] + (["--n-tris", str(a.n_tris)] if a.n_tris else [])
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    raise SystemExit(f"{who}: the loop failed ({p.returncode}): {p.stderr[-800:]}")
                runs[who].append(json.loads(p.stdout.strip().splitlines()[-1])["frames_per_s_off"])
        out["off_vs_parent"] = {"size": sizes[0], **runs, "parent_spread": [min(runs["parent"]), max(runs["parent"])], "this_median": statistics.median(runs["this"]),
                                "parent_median": statistics.median(runs["parent"])}
    print(json.dumps(out), flush=True)
