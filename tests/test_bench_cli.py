"""bench.py's launcher and roofline bookkeeping (CPU), and the N > 1 flow on one GPU (gpu).

`python bench.py --gpus N` outside a launcher must start N rank processes itself (the parent never touches the GPU) and
rank 0 must report n_gpus == N; counter traffic that belongs to another build of the kernel must not be reported."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra, timeout=600):
    env = dict(os.environ, **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        if k not in env_extra:
            env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


def test_gpus_flag_spawns_that_many_ranks():
    p, out = _run(["--gpus", "3"], {"CRH_BENCH_RANK_PROBE": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert out == {"probe": True, "n_gpus": 3, "rccl_ranks": 3, "sum": 3, "spawned": True}


def test_more_ranks_than_gpus_is_refused_at_once():
    """round-5 verdict, item 6: `bench.py --gpus 8` on a box with fewer GPUs (this container: none) says so in one line within seconds -- it does not start
    eight ranks that wait for each other in a rendezvous; under a launcher every rank checks for itself before the rendezvous"""
    import time
    t0 = time.time()
    p, out = _run(["--gpus", "8"], {})
    assert p.returncode != 0 and time.time() - t0 < 10.0
    assert "--gpus 8 needs 8 GPUs on this node" in p.stderr and "visible" in p.stderr and out is None
    import bench
    assert bench.visible_gpu_count() in (0, None) or bench.visible_gpu_count() >= 1


def test_gpus_flag_must_match_the_launcher():
    p, out = _run(["--gpus", "3"], {"CRH_BENCH_RANK_PROBE": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert p.returncode != 0 and out is None and "WORLD_SIZE=2" in p.stderr


def test_parent_of_spawned_ranks_never_imports_torch():
    code = ("import sys, bench\n"
            "sys.argv = ['bench.py', '--gpus', '2']\n"
            "import os; os.environ['CRH_BENCH_RANK_PROBE'] = '1'\n"
            "try:\n    bench.main()\nexcept SystemExit as e:\n    assert not e.code, e.code\n"
            "assert 'torch' not in sys.modules and 'cadrays_amd' not in sys.modules, 'parent touched the GPU stack'\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]


def test_strong_and_weak_defaults():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--config", "C4"])
    assert a.scaling == "strong" and a.steps == 1 and a.other_list == []
    a = bench.parse_args([])
    assert a.scaling == "weak" and a.config == "C3" and a.gpus == 1 and not a.full
    assert a.other_list == [] and a.live_traffic == "off"            # a plain run measures the headline only
    a = bench.parse_args(["--full"])
    assert a.other_list == ["C5", "C2", "C1", "CAD1M"]             # the default single-GPU --full run also times the other configs (config.other_configs_timed)
    assert bench.parse_args(["--full", "--gpus", "8"]).other_list == [] and bench.parse_args(["--full", "--config", "C2"]).other_list == []
    assert bench.parse_args(["--full", "--other-configs", "none"]).other_list == [] and bench.parse_args(["--full", "--steps", "20", "--warmup", "5"]).other_list == ["C5", "C2", "C1", "CAD1M"]


def test_a_broken_checker_is_not_a_failed_gate(monkeypatch):
    """an exception inside the oracle leg is reported as a checker error (rc 0), pixels == 0 is a FAILED gate, not a vacuous pass"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench

    class FakeOracle:
        def __init__(self, accum):
            self.accum = accum
        def n_tiles(self): return 4
        def reset(self): pass
        def render_tiles(self, *a): pass
        def stats(self): return {"rays_nearest": 100, "rays_any": 0, "seconds": 1e-3}
        def read_accum(self): return self.accum
        def close(self): pass
    g = bench.ParityOracle.__new__(bench.ParityOracle)
    acc = np.zeros((8, 8, 4), np.float32)                            # no pixel holds the asked sample count
    g.o, g.load_s, g.rate = FakeOracle(acc), 0.0, None
    r = g.check(np.zeros((8, 8, 3), np.float32), 0, 2, 1.0, 4)
    assert r["pixels"] == 0 and r["bit_exact"] is False
    acc[..., 3] = 2; acc[..., :3] = 0.5
    g.o = FakeOracle(acc); g.rate = None
    r = g.check(np.full((8, 8, 3), 0.5, np.float32), 0, 2, 1.0, 4)
    assert r["pixels"] == 64 and r["bit_exact"] and r["rel_l2"] == 0.0


def test_stale_counter_traffic_is_refused(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    f = tmp_path / "pmc.json"
    ent = {"source_hash": "0" * 16, "spp_per_step": 128, "hbm_bytes_per_launch": 1.0e11, "tcc_hit_per_launch": 6.0, "tcc_miss_per_launch": 4.0}
    f.write_text(json.dumps({"configs": {"C3": ent}}))
    monkeypatch.setattr(bench, "PMC_FILE", str(f))
    got, why = bench.pmc_entry("C3", 128, False)
    assert got is None and why.startswith("stale")
    r = bench.roofline_report("C3", 128, False, 1.2e11, 16.0, 81 << 20, {})
    assert r["traffic"] is None and r["frac"] is None and r["bound"] == "hbm" and r["limited_by"].startswith("l2-miss")          # cache-resident, no counters: no HBM fraction
    r = bench.roofline_report("C5", 32, False, 1.5e11, 28.0, 1 << 30, {})
    assert r["bound"] == "hbm" and r["traffic"] is None and 0 < r["frac"] < 1
    # a matching entry is used, and a cache-resident scene can then never report more than what crossed the memory side
    ent["source_hash"] = bench.kernel_source_hash()
    f.write_text(json.dumps({"configs": {"C3": ent}}))
    r = bench.roofline_report("C3", 128, False, 1.4e11, 16.0, 81 << 20, {})
    assert r["traffic"] == 1.0e11 and r["l2_hit_rate"] == 0.6 and r["traffic_over_alg"] < 1
    assert abs(r["achieved"] - 1.0e11 / 16e-3 / 1e9) < 1 and r["frac"] <= 1 and r["alg_frac_of_hbm_peak"] > 1
    assert bench.pmc_entry("C3", 64, False)[0] is None and bench.pmc_entry("C3", 128, True)[0] is None


def test_counter_passes_of_this_run_replace_the_committed_bytes(tmp_path, monkeypatch):
    """roofline.traffic from counter passes started by the run itself (bench.live_traffic): used when they worked, reported beside the committed bytes of the same
    build, usable even when the committed file is stale; a failed pass falls back to the committed figures and says why"""
    sys.path.insert(0, ROOT)
    import bench
    f = tmp_path / "pmc.json"
    ent = {"source_hash": bench.kernel_source_hash(), "spp_per_step": 128, "hbm_bytes_per_launch": 1.0e11, "tcc_hit_per_launch": 6.0, "tcc_miss_per_launch": 4.0}
    f.write_text(json.dumps({"configs": {"C3": ent}}))
    monkeypatch.setattr(bench, "PMC_FILE", str(f))
    live = {"fetch_size_kb_per_launch": 4.0e7, "write_size_kb_per_launch": 1.0e7, "hbm_bytes_per_launch": 4.0e7 * 2048 + 1.0e7 * 1024, "launches_per_pass": 30, "seconds": 41.0, "how": "two passes"}
    r = bench.roofline_report("C3", 128, False, 1.4e11, 16.0, 81 << 20, {}, live=live)
    assert r["traffic"] == live["hbm_bytes_per_launch"] and r["traffic_measured"].startswith("IN THIS RUN") and r["traffic_source"] == "two passes"
    assert r["traffic_committed"] == 1.0e11 and abs(r["traffic_this_run_over_committed"] - live["hbm_bytes_per_launch"] / 1.0e11) < 1e-3
    assert abs(r["achieved"] - live["hbm_bytes_per_launch"] / 16e-3 / 1e9) < 1 and r["l2_hit_rate"] == 0.6
    r = bench.roofline_report("C3", 128, False, 1.4e11, 16.0, 81 << 20, {}, live={"error": "rocprofv3 not found"})
    assert r["traffic"] == 1.0e11 and r["traffic_measured"].startswith("NOT in this run") and r["traffic_live_error"] == "rocprofv3 not found"
    ent["source_hash"] = "0" * 16                                   # stale committed passes: the live bytes alone
    f.write_text(json.dumps({"configs": {"C3": ent}}))
    r = bench.roofline_report("C3", 128, False, 1.4e11, 16.0, 81 << 20, {}, live=live)
    assert r["traffic"] == live["hbm_bytes_per_launch"] and r["frac"] is not None and r["committed_passes"].startswith("stale") and "ceilings" not in r
    # the default: on for the plain headline run only; never inside a profiled process
    assert bench.parse_args(["--full"]).live_traffic == "on" and bench.parse_args(["--full", "--other-configs", "none"]).live_traffic == "off"
    assert bench.parse_args(["--full", "--config", "C5"]).live_traffic == "off" and bench.parse_args(["--full", "--gpus", "2"]).live_traffic == "off"
    assert bench.parse_args([]).live_traffic == "off"
    monkeypatch.setenv("ROCPROFILER_SOMETHING", "1")
    assert bench.being_profiled() and "profiler" in bench.live_traffic("C3")["error"]


def test_every_leg_is_in_flat_keys_and_in_the_tail_of_the_line():
    """verdict r4 item 3: the driver's record keeps top-level scalars, the scalars inside config / roofline, and the tail of stdout -- so every leg's rate,
    fractions and gate result, the interactive figures and the measured ceilings are flat keys in all three places and once more in `legs_summary`, the
    LAST key.  Checked on a committed line of round 4 (nested objects only) and on this round's."""
    sys.path.insert(0, ROOT)
    import bench
    old = json.loads(open(os.path.join(ROOT, "profiles", "r4", "bench_default_steps20.json")).read().strip().splitlines()[-1])
    assert "legs_summary" not in old and "c5_mrays" not in old
    bench.flatten_line(old)
    assert list(old)[-1] == "legs_summary" and len(json.dumps(old["legs_summary"])) < 1200
    legs = old["config"]["other_configs_timed"]
    for name in ("C5", "C2", "C1"):
        k = name.lower()
        for place in (old, old["config"], old["legs_summary"]):
            assert place[f"{k}_mrays"] == legs[name]["value"] and place[f"{k}_ms_per_step"] == legs[name]["ms_per_step"]
            assert place[f"{k}_parity_bit_exact"] is True and place[f"{k}_frac_counter"] == legs[name]["roofline"]["traffic_frac"]
    assert old["c3_mrays"] == old["value"] and old["c3_parity_bit_exact"] is True
    assert old["roofline"]["valu_issue"] == old["roofline"]["ceilings"]["valu_issue"] and old["roofline"]["lane_util"] == old["roofline"]["ceilings"]["lane_util"]
    assert old["interactive_redraw_per_s"] == old["config"]["interactive"]["redraw_per_s_lookahead_1"]
    # a gate that errored or failed is not reported as passed
    broken = {"value": 1.0, "ms_per_step": 1.0, "config": {"workload": "C3: x"}, "roofline": {}, "parity": {"error": "boom"}, "parity_step0": {"bit_exact": True}}
    bench.flatten_line(broken)
    assert broken["c3_parity_bit_exact"] is None
    failed = {"value": 1.0, "ms_per_step": 1.0, "config": {"workload": "C3: x"}, "roofline": {}, "parity": {"bit_exact": False}, "parity_step0": {"bit_exact": True}}
    bench.flatten_line(failed)
    assert failed["c3_parity_bit_exact"] is False
    new = os.path.join(ROOT, "profiles", "r5", "bench_default_steps20.json")
    if os.path.exists(new):
        line = json.loads(open(new).read().strip().splitlines()[-1])
        assert list(line)[-1] == "legs_summary" and line["legs_summary"]["c5_mrays"] == line["config"]["other_configs_timed"]["C5"]["value"]
        assert line["interactive_drag_frames_per_s"] > 0 and line["interactive_first_frame_ms"] > 0


def test_committed_counter_traffic_belongs_to_this_build():
    """profiles/pmc_traffic.json must be re-collected (profiles/pmc_collect.sh) whenever the traversal kernel or the node format
    changes: a stale file would silently report another kernel's traffic."""
    sys.path.insert(0, ROOT)
    import bench
    data = json.load(open(bench.PMC_FILE))
    want = bench.kernel_source_hash()
    for cfg in ("C3", "C5", "C2"):
        assert cfg in data["configs"], f"no counter passes for {cfg}"
    stale = {cfg: data["configs"][cfg]["source_hash"] for cfg in ("C3", "C5", "C2") if data["configs"][cfg]["source_hash"] != want}
    if stale:
        # not an error of the code under test: bench.py refuses these figures (test above) and reports traffic = null until
        # profiles/pmc_collect.sh has run on a GPU box for THIS build -- but make it visible
        assert all(bench.pmc_entry(cfg, data["configs"][cfg]["spp_per_step"], False)[0] is None for cfg in stale)
        pytest.skip(f"profiles/pmc_traffic.json is from build(s) {sorted(set(stale.values()))}, sources are {want}: re-run profiles/pmc_collect.sh")


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_report_two(hip_lib):
    """the whole N = 2 flow (spawn, tile shards, framebuffer reduce, rank-0 report) on the single GPU of the test box"""
    p, out = _run(["--full", "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu", "--config", "C1", "--spp", "4"],
                  {"CRH_BENCH_SHARE_DEVICE": "1", "CRH_BENCH_BACKEND": "gloo"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert out["n_gpus"] == 2 and out["config"]["rccl_ranks"] == 2 and out["value"] > 0
    assert out["config"]["tiles_per_rank"] * 2 >= 256 - 1            # 512 x 512 in 32 x 32 tiles, interleaved
    assert out["parity"]["bit_exact"] and out["parity"]["pixels"] > 0   # the ASSEMBLED frame of the timed step goes through the oracle gate
    # the N > 1 line explains itself (verdict r3 item 3): per-rank render / exchange times, shard balance, which exchange step ran and why,
    # and ONE tree build for the job (rank 0 builds, rank 1 takes its tree through crh_build_prebuilt)
    cfg = out["config"]
    assert [p["rank"] for p in cfg["per_rank"]] == [0, 1]
    assert all(p["ms_render"] > 0 and p["ms_reduce"] > 0 and p["rays"] > 0 and p["tiles"] == 128 for p in cfg["per_rank"])
    assert sum(p["rays"] for p in cfg["per_rank"]) == cfg["rays_nearest"] + cfg["rays_any"]
    assert cfg["reduce_ms_per_step"] == max(p["ms_reduce"] for p in cfg["per_rank"]) and 1.0 <= cfg["shard_rays_max_over_mean"] < 1.2
    a = cfg["assemble"]
    assert a["mode"] in ("reduce", "gather") and a["reduce_ms"] > 0 and a["gather_ms"] > 0 and a["gather_bytes_per_rank"] * 2 <= a["reduce_bytes_per_rank"] * 1.01
    assert cfg["scene_hand_over"]["built_here"] is True and cfg["scene_hand_over"]["tree_bytes"] > 0
    assert "rccl_version" in cfg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["reduce", "gather"])
def test_both_exchange_steps_pass_the_gate(hip_lib, mode):
    p, out = _run(["--full", "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu", "--config", "C1", "--spp", "4", "--assemble", mode],
                  {"CRH_BENCH_SHARE_DEVICE": "1", "CRH_BENCH_BACKEND": "gloo"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert out["config"]["assemble"]["mode"] == mode and out["parity"]["bit_exact"] and out["parity"]["pixels"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["reduce", "gather"])
def test_c3_at_the_weak_scaling_step_size_of_two_ranks(hip_lib, mode):
    """verdict r4 item 7: the SHAPE the driver's scaling run has at N = 2 -- the full C3 scene (1 M triangles, 1080p), weak scaling: every rank renders
    spp x N = 1024 samples of its Morton-interleaved half of the tiles in ONE crh_render_tiles call (wide batches of 1020 tiles) -- on the one GPU of the test
    box, both exchange steps; the assembled frame goes through the oracle gates.  No curve is measured here (two ranks share a device): the point is that the
    first real SCALE run cannot fail on something a rehearsal would have caught."""
    p, out = _run(["--full", "--gpus", "2", "--config", "C3", "--steps", "2", "--warmup", "1", "--no-cpu", "--assemble", mode], {"CRH_BENCH_SHARE_DEVICE": "1", "CRH_BENCH_BACKEND": "gloo"}, timeout=1500)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    cfg = out["config"]
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and cfg["workload"].startswith("C3: 1000000")
    assert cfg["spp_per_step_per_rank"] == 1024 and cfg["spp_per_step_whole_frame"] == 512 and cfg["tiles_per_rank"] == 1020
    assert cfg["assemble"]["mode"] == mode and cfg["assemble"]["reduce_ms"] > 0 and (cfg["assemble"]["gather_ms"] or 0) > 0
    assert [q["rank"] for q in cfg["per_rank"]] == [0, 1] and all(q["tiles"] == 1020 and q["ms_render"] > 0 and q["rays"] > 0 for q in cfg["per_rank"])
    assert 1.0 <= cfg["shard_rays_max_over_mean"] < 1.02                  # Morton interleave: DESIGN.md section 5 predicts 0.998 at N = 2
    assert cfg["scene_hand_over"]["built_here"] is True and cfg["scene_hand_over"]["tree_bytes"] > 30e6
    assert out["parity"]["bit_exact"] and out["parity"]["pixels"] > 0 and out["parity"]["spp"] == 2048      # the assembled frame of the timed steps: 2 x 1024 samples per pixel
    assert out["c3_parity_bit_exact"] is True and out["legs_summary"]["c3_mrays"] == out["value"]           # the flat keys of the line (verdict r4 item 3)
    assert list(out)[-1] == "legs_summary"


@pytest.mark.gpu
def test_other_configs_are_timed_in_the_same_run(hip_lib):
    """verdict r3 item 1: the default run times further single-GPU configs after the headline, each with its own gates and roofline; here with the
    small ones so that the test stays short (C5's own leg: tests/test_bench_c4.py)"""
    p, out = _run(["--full", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-interactive", "--config", "C2", "--other-configs", "C1", "--other-steps", "2"], {}, timeout=900)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert out["config"]["workload"].startswith("C2") and out["parity_step0"]["tiles"] >= 32 and out["parity_step0"]["bit_exact"]
    o = out["config"]["other_configs_timed"]["C1"]
    assert o["steps"] == 2 and o["value"] > 0 and o["ms_per_step"] > 0 and o["workload"].startswith("C1")
    assert o["parity"]["bit_exact"] and o["parity_step0"]["bit_exact"] and o["parity_step0"]["tiles"] >= 32
    assert o["roofline"]["alg_frac"] > 0 and o["roofline"]["avg_launch_ms"] > 0
    assert "checker_errors" not in out


@pytest.mark.gpu
def test_strong_scaling_step_is_the_fixed_job(hip_lib):
    p1, o1 = _run(["--gpus", "1", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-interactive", "--config", "C1", "--spp", "8", "--scaling", "strong"], {})
    p2, o2 = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu", "--config", "C1", "--spp", "8", "--scaling", "strong"],
                  {"CRH_BENCH_SHARE_DEVICE": "1", "CRH_BENCH_BACKEND": "gloo"})
    assert p1.returncode == 0 and p2.returncode == 0, (p1.stderr + p2.stderr)[-3000:]
    assert o1["scaling"] == o2["scaling"] == "strong"
    assert o1["config"]["rays_nearest"] == o2["config"]["rays_nearest"]         # same job, sharded: same rays in total


def test_a_plain_run_measures_the_headline_only():
    """a plain run is set-up, warm-up, the timed steps and the line: what measures or checks beyond the headline figure is asked for with --full"""
    sys.path.insert(0, ROOT)
    import bench
    for extra in (["--other-configs", "C1"], ["--live-traffic", "on"]):
        with pytest.raises(SystemExit):
            bench.parse_args(extra)
        a = bench.parse_args(["--full"] + extra)
        assert a.full and (a.other_list == ["C1"] or a.live_traffic == "on")
    a = bench.parse_args(["--steps", "7", "--warmup", "2", "--dump-outputs", "d"])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == "d" and not a.full


def test_dumped_outputs_stay_within_their_budget(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, at most 64 MB together; an image too large for that (C5's 4K frame) becomes the same seeded pixel
    sample in every run"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    small = np.arange(64 * 48 * 3, dtype=np.float32).reshape(48, 64, 3)
    bench.write_outputs(str(tmp_path / "s"), {"hdr": small, "ray_counts": np.array([1.0, 2.0, 3.0])})
    assert np.array_equal(np.load(tmp_path / "s" / "hdr.npy"), small)
    assert np.load(tmp_path / "s" / "ray_counts.npy").dtype == np.float64
    big = np.random.default_rng(5).random((2160, 3840, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"hdr": big, "ray_counts": np.zeros(3)})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["hdr_sample.npy", "hdr_sample_pixels.npy", "ray_counts.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.OUTPUT_BYTES_MAX
    pix = np.load(tmp_path / "a" / "hdr_sample_pixels.npy")
    got = np.load(tmp_path / "a" / "hdr_sample.npy")
    assert pix.dtype == np.float64 and got.dtype == np.float32 and len(pix) == len(got) > 10 ** 6
    assert np.array_equal(got, big.reshape(-1, 3)[pix.astype(np.int64)])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_steps_computed(hip_lib, oracle_lib, tmp_path):
    """a plain run: exactly --steps timed steps, no legs beyond the headline, and --dump-outputs writes the image the timed steps accumulated -- the
    same bits in a second run, and the oracle's for the same samples"""
    import numpy as np
    args = ["--config", "C1", "--spp", "8", "--steps", "3", "--warmup", "1"]
    p, out = _run(args + ["--dump-outputs", str(tmp_path / "a")], {})
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0 and out["metric"] == "Mrays/s"
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["parity"] is None and out["config"]["interactive"] is None
    assert "other_configs_timed" not in out["config"] and out["config"]["full"] is False
    hdr = np.load(tmp_path / "a" / "hdr.npy")
    counts = np.load(tmp_path / "a" / "ray_counts.npy")
    assert hdr.shape == (512, 512, 3) and hdr.dtype == np.float32 and np.isfinite(hdr).all() and hdr.mean() > 0
    assert counts.tolist() == [out["config"]["rays_nearest"], out["config"]["rays_any"], 512 * 512 * 8 * 3]
    p, _ = _run(args + ["--dump-outputs", str(tmp_path / "b")], {})
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert np.array_equal(np.load(tmp_path / "b" / "hdr.npy").view(np.uint32), hdr.view(np.uint32))
    from cadrays_amd import scenes
    o = oracle_lib.Oracle().load_scene(scenes.baseline_config("C1"))
    tiles = np.arange(0, o.n_tiles(), 7, dtype=np.uint32)
    o.render_tiles(tiles, 8, 24)                                   # samples [8, 32): the three timed steps after one warm-up step of 8
    ref = o.read_accum()
    o.close()
    mask = ref[..., 3] == 24
    assert mask.sum() > 0 and np.array_equal(hdr[mask].view(np.uint32), np.ascontiguousarray(ref[..., :3][mask], np.float32).view(np.uint32))
