#!/usr/bin/env python3
"""What the shade guide of the denoised display costs (crh_set_shade_guide: albedo demodulation and lights in view for the a-trous filter,
shade_guide_kernels.hip), on a BASELINE config at its full resolution.  One JSON line:

  guide_ms                            device time per launch of the plane's kernels (the light test where the scene has a positional light, and the plane)
  guided_pass_ms[5] / unguided_pass_ms[5]
                                      every guided pass (the plain gather form) next to the unguided pass of the same run, plain and staged form (five levels,
                                      until_samples 1024 so that all five work at 1 spp; HIP events around `--repeats` launches: crh_bench_shade_guide, crh_bench_denoise)
  read_ldr_ms.guide_off / .guide_on   a lone synchronous LDR read-out with the filter on (defaults), guide off / on (host clock around a call that ends in a synchronise)
  displayed_frames_per_s              the displayed loop of tools/bench_redraw.py (crh_render(1) + asynchronous LDR read-back two frames behind), filter on: guide
                                      off, on, off again
  flagged_pixels, weights_not_one     what the plane holds for this view

  python tools/bench_shade_guide.py [--config C3|CAD1M] [--trials 15] [--frames 128] [--repeats 20]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

from bench_denoise import displayed, scene_of, timed      # noqa: E402  (the same loops, so that the figures compare)


def unguided(sc, staged, repeats):
    from cadrays_amd.view import View
    os.environ["CRH_DENOISE_STAGED"] = "1" if staged else "0"      # read when the context is created
    v = View(0).load_scene(sc)
    v.Redraw(); v.sync()
    v.set_denoise(True, levels=5, until_samples=1024)
    v.bench_denoise(2)
    b = v.bench_denoise(repeats)
    v.close()
    return [round(x, 4) for x in b["pass_ms"]]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    from cadrays_amd.view import View
    sc = scene_of(a.config)
    out = {"config": a.config, "n_triangles": int(len(sc.tri)), "n_lights": len(sc.lights), "n_textures": len(sc.textures or [])}
    out["unguided_pass_ms"] = {"plain": unguided(sc, False, a.repeats), "staged": unguided(sc, True, a.repeats)}
    v = View(0).load_scene(sc)
    out["width"], out["height"] = v.width, v.height
    v.Redraw(); v.sync()
    v.set_denoise(True, levels=5, until_samples=1024)
    v.set_shade_guide(True)
    v.bench_shade_guide(2)
    b = v.bench_shade_guide(a.repeats)
    out["guide_ms"] = round(b["guide_ms"], 4)
    out["guided_pass_ms"] = [round(x, 4) for x in b["pass_ms"]]
    plane = v.read_shade_guide()
    out["flagged_pixels"] = int((plane[..., 3] != 0).sum())
    out["weights_not_one"] = int((plane[..., :3] != 1).any(-1).sum())
    v.SetDenoise()
    v.set_shade_guide(False)
    off = timed(v.read_ldr, a.trials)
    v.set_shade_guide(True)
    on = timed(v.read_ldr, a.trials)
    out["read_ldr_ms"] = {"guide_off": off, "guide_on": on}
    fps = {}
    for name, guide in (("guide_off", False), ("guide_on", True), ("guide_off_again", False)):
        v.set_shade_guide(guide); v.reset()
        fps[name] = displayed(v, a.frames)
    out["displayed_frames_per_s"] = fps
    print(json.dumps(out), flush=True)
    v.close()
