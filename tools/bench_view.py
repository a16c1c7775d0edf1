#!/usr/bin/env python3
"""What the viewport read-out costs and what it saves (crh_read_view: the finished RGB8 frame resampled to the window's size on the device, the last stage of the
display chain; view_kernels.hip), on a BASELINE config at its full resolution (C3: 1080p, C5: 4K).  One JSON line.  The views: the frame's own
size ("same"), half of it per side ("half", AUTO = AREA) and 1.5 times per side ("x1.5", AUTO = BILINEAR).

  link_gb_per_s                       device-to-pinned-host copies of 8 / 32 / 128 MB on a stream (HIP events): the rate every read-out's copy is bound by
  kernel_ms.<view>.<filter>           device time per launch of the resample kernel (crh_bench_view, HIP events around `--repeats` launches) and the GB/s of
                                      3 W H bytes read + 3 vw vh written over it.  The kernel has one form, the plain gather; the LDS-staged form it was measured
                                      against with this tool, and lost to, is recorded in profiles/view_ab.md
  read_ms.ldr / .view.<view>          wall time of a lone synchronous crh_read_ldr and of crh_read_view in the same run (host clock around calls that end in a
                                      synchronise), and the bytes each brings over the link
  displayed_frames_per_s.<view>       a 1-spp loop (crh_render(1) + asynchronous read-back collected two frames later) with crh_read_view_begin / _end ("device"),
                                      against the same loop with crh_read_ldr_begin / _end followed by crh_view_host on the host ("host": what a host does today),
                                      and the plain LDR loop without any scaling ("ldr_only")

  python tools/bench_view.py [--config C3|C5] [--trials 15] [--frames 96] [--host-frames 12] [--repeats 20] [--n-tris N]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

FILTERS = {"auto": 0, "nearest": 1, "bilinear": 2, "area": 3}


def timed(fn, trials):
    ts = []
    for _ in range(trials):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4)}


def link_rate(torch):
    out = {}
    for mb in (8, 32, 128):
        d = torch.empty(mb << 20, dtype=torch.uint8, device="cuda")
        h = torch.empty(mb << 20, dtype=torch.uint8).pin_memory()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h.copy_(d, non_blocking=True); torch.cuda.synchronize()
        e0.record()
        for _ in range(8): h.copy_(d, non_blocking=True)
        e1.record(); torch.cuda.synchronize()
        out[f"{mb}MB"] = round((mb << 20) * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 2)
    return out


def loop(v, frames, begin, end):
    """frames per second of: one frame + asynchronous read-back, collected two frames later"""
    for n in (6, frames):
        v.sync()
        t = time.perf_counter()
        for i in range(n):
            v.Redraw()
            if i >= 2: end()
            begin()
        end(); end(); v.sync()
        dt = time.perf_counter() - t
    return round(frames / dt, 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C3", "C5"])
    ap.add_argument("--trials", type=int, default=15)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--host-frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n-tris", type=int, default=None, help="triangles of the config's scene (default: the config's own)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from cadrays_amd import scenes
    from cadrays_amd.view import View, view_host
    out = {"config": a.config, "link_gb_per_s": link_rate(torch)}
    sc = scenes.baseline_config(a.config, n_tris=a.n_tris)
    W, H = sc.params.width, sc.params.height
    views = {"same": (W, H), "half": (W // 2, H // 2), "x1.5": (W * 3 // 2, H * 3 // 2)}
    out.update(n_triangles=int(len(sc.tri)), width=W, height=H, views={k: list(s) for k, s in views.items()})

    # ---- a lone read-out, and the loops
    v = View(0).load_scene(sc)
    for _ in range(40):                                          # let the library's own measurements after a build settle (tools/bench_redraw.py)
        v.reset(); v.Redraw(); v.sync()
    out["kernel_ms"] = {}
    for name, (vw, vh) in views.items():
        out["kernel_ms"][name] = {}
        for fname, f in FILTERS.items():
            v.bench_view(vw, vh, filter=f, repeats=2)
            ms = v.bench_view(vw, vh, filter=f, repeats=a.repeats)
            out["kernel_ms"][name][fname] = {"ms": round(ms, 4), "gb_per_s": round(3 * (W * H + vw * vh) / (ms * 1e-3) / 1e9, 1)}
    out["read_ms"] = {"ldr": dict(timed(v.read_ldr, a.trials), bytes=3 * W * H), "view": {}}
    for name, (vw, vh) in views.items():
        out["read_ms"]["view"][name] = dict(timed(lambda: v.read_view(vw, vh), a.trials), bytes=3 * vw * vh)
    out["read_ms"]["ldr_again"] = timed(v.read_ldr, a.trials)
    shown = np.empty((H, W, 3), np.uint8)
    out["displayed_frames_per_s"] = {"ldr_only": loop(v, a.frames, v.read_ldr_begin, lambda: v.read_ldr_end(shown))}
    for name, (vw, vh) in views.items():
        window = np.empty((vh, vw, 3), np.uint8)
        dev = loop(v, a.frames, lambda: v.read_view_begin(vw, vh), lambda: v.read_view_end(window))
        host = loop(v, a.host_frames, v.read_ldr_begin, lambda: view_host(v.read_ldr_end(shown), vw, vh))
        out["displayed_frames_per_s"][name] = {"device": dev, "host": host}
    out["displayed_frames_per_s"]["ldr_only_again"] = loop(v, a.frames, v.read_ldr_begin, lambda: v.read_ldr_end(shown))
    print(json.dumps(out), flush=True)
    v.close()
