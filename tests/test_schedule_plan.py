"""The rules of the frame schedule (cadrays_amd/csrc/crh_plan.h) on the CPU: tests/schedule_plan_model.cpp -- an ordering model of the
frame pipeline, pinned values of the pure formulas, order_tiles on small cases -- compiled with ASan + UBSan and run.  No GPU, no HIP."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_plan_model(tmp_path):
    exe = str(tmp_path / "schedule_plan_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "cadrays_amd", "csrc"), os.path.join(ROOT, "tests", "schedule_plan_model.cpp"), "-o", exe])
    # the frame seeds tests/test_golden.py trusts (tests/golden/math.npz, written by the CPU checker): frame_seeds(1, 0, 16) must be these
    seeds = [str(int(x)) for x in np.load(os.path.join(ROOT, "tests", "golden", "math.npz"))["frame_seeds"]]
    assert len(seeds) == 16
    p = subprocess.run([exe] + seeds, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().startswith("ok:"), p.stdout[-2000:] + p.stderr[-6000:]
