#!/usr/bin/env python3
"""What the denoised display costs and what it buys (crh_set_denoise: an id-guided a-trous filter in front of the tone map, denoise_kernels.hip; DESIGN.md 4.12 /
6.11), on a BASELINE config at its full resolution.  One JSON line:

  forms.plain / forms.staged          per form of the pass kernel (CRH_DENOISE_STAGED=0 / 1, a context each):
    guide_ms, pass_ms[5]              device time per launch of k_denoise_guide and of every pass, five levels, until_samples 1024 so that all five work at
                                      1 spp (HIP events around `--repeats` launches: crh_bench_denoise)
    pass_gb_per_s[5]                  W * H * 48 B -- the 32 B a pass must read and the 16 B it must write per pixel, a LOWER bound of its traffic -- over that time
    read_ldr_off_ms / read_ldr_on_ms  a lone synchronous LDR read-out, feature off / on with the defaults (host clock around a call that ends in a synchronise)
    displayed_frames_per_s_off / _on  the displayed loop of tools/bench_redraw.py (crh_render(1) + asynchronous LDR read-back two frames behind)
    forms_agree                       crh_read_denoised of the two forms is bit-identical
  mse                                 at 1, 4 and 16 spp: mean squared error over the hit pixels against `--truth` spp, unfiltered and filtered (defaults)

  python tools/bench_denoise.py [--config C3|CAD1M] [--trials 15] [--frames 128] [--repeats 20] [--truth 512]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def timed(fn, trials):
    ts = []
    for _ in range(trials):
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


def scene_of(config):
    from cadrays_amd import scenes
    return scenes.baseline_config(config)


def measure_form(sc, staged, a):
    from cadrays_amd.view import View
    os.environ["CRH_DENOISE_STAGED"] = "1" if staged else "0"      # read when the context is created
    v = View(0).load_scene(sc)
    v.Redraw(); v.sync()
    W, H = v.width, v.height
    out = {}
    v.set_denoise(True, levels=5, until_samples=1024)
    v.bench_denoise(2)
    b = v.bench_denoise(a.repeats)
    out["guide_ms"] = round(b["guide_ms"], 4)
    out["pass_ms"] = [round(x, 4) for x in b["pass_ms"]]
    out["pass_gb_per_s"] = [round(W * H * 48 / (x * 1e-3) / 1e9, 1) if x > 0 else None for x in b["pass_ms"]]
    v.ClearDenoise()
    out["read_ldr_off_ms"] = timed(v.read_ldr, a.trials)
    v.SetDenoise()
    image = v.read_denoised()
    out["read_ldr_on_ms"] = timed(v.read_ldr, a.trials)
    v.ClearDenoise(); v.reset()
    out["displayed_frames_per_s_off"] = displayed(v, a.frames)
    v.SetDenoise(); v.reset()
    out["displayed_frames_per_s_on"] = displayed(v, a.frames)
    v.ClearDenoise(); v.reset()
    out["displayed_frames_per_s_off_again"] = displayed(v, a.frames)
    return v, out, image


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "CAD1M"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--truth", type=int, default=512)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    sc = scene_of(a.config)
    out = {"config": a.config, "n_triangles": int(len(sc.tri)), "forms": {}}
    v, out["forms"]["plain"], plain = measure_form(sc, False, a)
    v.close()
    v, out["forms"]["staged"], staged = measure_form(sc, True, a)
    out["width"], out["height"] = v.width, v.height
    out["forms_agree"] = bool(np.array_equal(plain.view(np.uint32), staged.view(np.uint32)))
    # what it buys: the error against a long accumulation
    v.reset()
    hit = v.read_ids()[1] >= 0
    shots, done = {}, 0
    for spp in (1, 4, 16):
        v.render(spp - done); done = spp
        shots[spp] = (v.read_hdr().astype(np.float64), v.read_denoised()[..., :3].astype(np.float64))
    v.render(a.truth - done)
    truth = v.read_hdr().astype(np.float64)
    out["mse"] = {"truth_spp": a.truth, "hit_pixels": int(hit.sum())}
    for spp, (raw, filtered) in shots.items():
        e_raw, e_f = float(((raw - truth)[hit] ** 2).mean()), float(((filtered - truth)[hit] ** 2).mean())
        out["mse"][str(spp)] = {"raw": round(e_raw, 6), "filtered": round(e_f, 6), "ratio": round(e_f / e_raw, 4) if e_raw > 0 else None}
    print(json.dumps(out), flush=True)
    v.close()
    sys.exit(0 if out["forms_agree"] else 1)
