"""camera_ray (cadrays_amd/csrc/k_raygen.h, shared with k_frame.h; oracle/crh_oracle.c) against the float64 replay of tests/camera_reference.py:
sub-pixel jitter from the path's RNG stream, the three perspective forms of crh_spec.h #13, orthographic rays and the thin lens, on two sides
with the SAME cases and bounds:
  cpu  the oracle
  gpu  the gfx950 kernels through View(0); there every image must also be bit-equal to the oracle's

HOW THE RAYS ARE OBSERVED: a 16 x 16 grid of cells on the plane z = 0, each showing one texel of a random 16 x 16 texture (the cell's uv is its own
texel centre), Lambert Kd 0.9 under a unit background, max_depth 2: a sample is Kd x the texel of the cell its camera ray lands in, or the
background beside the grid.  The replay draws every sample's jitter and lens point from a numpy restatement of the RNG, builds the ray in float64,
meets the plane and finds the cell; a pixel must lie within the interval the replay gives (undecided samples -- within 1e-4 cell of a border --
count with the smaller and the larger neighbour), widened by Kd K 2^-24 (camera_reference.LAMBERT_K), by the rounding
of the texel's own bilinear lookup (Kd R, lookup_reference) and by that of the running float32 mean of the 8 samples (camera_reference.mean_rounding).

Measured on the cpu side (the gpu's bits are the same): undecided share at most 0.0007 (cap 0.005); worst distance outside the unwidened interval
6.1e-7 of a widening of 1.14e-6.
"""
import dataclasses

import numpy as np
import pytest

from cadrays_amd import scenes

import camera_reference as C
from camera_reference import LAMBERT_K
from lookup_reference import LERP_R

F32 = np.float32
N = 16
KD = 0.9
UNDECIDED_MAX = 0.005
# every case takes 8 samples; no value exceeds the background's 1; the texel itself comes from a bilinear lookup at a texel centre (R of lookup_reference)
WIDEN = KD * (LAMBERT_K + LERP_R) * 2.0 ** -24 + C.mean_rounding(8)
FOVY = float(np.rad2deg(2 * np.arctan(1 / 3)))            # from 3 units away the grid fills the frame's height

PIN = scenes.Camera(eye=(0, 0, 3), dir=(0, 0, -1), up=(0, 1, 0), fovy_deg=FOVY)
ORTHO = dataclasses.replace(PIN, is_ortho=True, ortho_scale=1.0)
OBLIQUE = scenes.Camera(eye=(1.2, -0.8, 2.5), dir=(-0.4, 0.3, -1.0), up=(0.1, 1.0, 0.2), fovy_deg=40.0)
# name -> (camera, width, height, samples, spec / params switches)
CASES = {
    "pinhole_form0": (PIN, 32, 32, 8, {}),
    "pinhole_form1": (PIN, 32, 32, 8, {"form": 1}),
    "pinhole_form2": (PIN, 32, 32, 8, {"form": 2}),
    "pinhole_48x24": (PIN, 48, 24, 8, {}),
    "ortho": (ORTHO, 32, 32, 8, {}),
    "lens_in_focus": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=3.0), 32, 32, 8, {}),
    "lens_near": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=2.0), 32, 32, 8, {}),
    "lens_far": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=5.0), 32, 32, 8, {}),
    "lens_oblique": (dataclasses.replace(OBLIQUE, aperture_radius=0.2, focal_dist=2.2), 32, 32, 8, {}),
    "lens_ortho": (dataclasses.replace(ORTHO, aperture_radius=0.1, focal_dist=2.0), 32, 32, 8, {}),
    "lens_form2": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=2.0), 32, 32, 8, {"form": 2}),
    "coherent_rng": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=2.0), 32, 32, 8, {"coherent_rng": True}),
    "uniform_32bit": (dataclasses.replace(PIN, aperture_radius=0.15, focal_dist=2.0), 32, 32, 8, {"uniform_32bit": True}),
}


def texture():
    return (0.1 + 0.9 * np.random.default_rng(21).random((N, N, 3))).astype(F32)


def cell_values():
    """cell (i, j) shows texel (row N - 1 - j, column i): row 0 of an image is v = 1"""
    return KD * texture()[::-1].astype(np.float64)


def grid_scene(cam, width, height, switches):
    j, i = np.mgrid[0:N, 0:N]
    uv = np.stack([(i + 0.5) / N, (j + 0.5) / N], -1)
    par = scenes.Params(width=width, height=height, tile_size=8, max_depth=2, background=(1.0, 1.0, 1.0), coherent_rng=bool(switches.get("coherent_rng", False)))
    sc = C.cell_grid_scene(N, uv, [C.lambert(KD, 0)], np.zeros((N, N), int), [texture()], cam, par)
    spec = {}
    if switches.get("form"):
        spec["raygen_bilinear"] = switches["form"]
    if switches.get("uniform_32bit"):
        spec["uniform_32bit"] = 1
    return dataclasses.replace(sc, spec=spec or None)


@pytest.fixture(scope="module")
def replays():
    return {}


def replay(replays, name, wrong=None):
    if (name, wrong) not in replays:
        cam, w, h, spp, sw = CASES[name]
        replays[(name, wrong)] = C.replay_image(cam, w, h, spp, cell_values(), (1.0, 1.0, 1.0), N, wrong=wrong, **sw)
    return replays[(name, wrong)]


@pytest.fixture(scope="module", params=[pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def render(request, oracle_lib):
    """render(name) -> the case's HDR image; cached per module; on the gpu side bit-equal to the oracle's"""
    done, gpu = {}, request.param == "gpu"
    if gpu:
        request.getfixturevalue("hip_lib")
        from cadrays_amd.view import View

    def run(name):
        if name not in done:
            cam, w, h, spp, sw = CASES[name]
            sc = grid_scene(cam, w, h, sw)
            o = oracle_lib.Oracle().load_scene(sc); o.render(spp)
            img = o.read_hdr(); o.close()
            if gpu:
                v = View(0).load_scene(sc); v.render(spp)
                g = v.read_hdr(); v.close()
                assert np.array_equal(g.view(np.uint32), img.view(np.uint32)), (name, "gpu != oracle")
                img = g
            done[name] = img.astype(np.float64)
        return done[name]
    run.side = request.param
    return run


def outside(img, lo, hi):
    """how far each value lies outside [lo, hi]"""
    return np.maximum(np.maximum(lo - img, img - hi), 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_image_is_the_replayed_one(render, replays, name):
    img = render(name)
    lo, hi, undecided = replay(replays, name)
    out = outside(img, lo, hi)
    print(f"lens_replay[{render.side}] {name}: undecided share {undecided:.5f}, worst outside the interval {out.max():.2e} (widening {WIDEN:.2e}), "
          f"pixels with an open interval {(hi > lo).any(2).mean():.4f}")
    assert undecided <= UNDECIDED_MAX
    assert (out <= WIDEN).all(), (name, np.argwhere(out > WIDEN)[:4], out.max())
    assert lo.std() > 0.05                                                     # the image has something to say


def test_lens_in_focus_is_the_pinhole_image(render, replays):
    a, b = render("lens_in_focus"), render("pinhole_form0")
    la, ha, _ = replay(replays, "lens_in_focus"); lb, hb, _ = replay(replays, "pinhole_form0")
    assert (np.abs(a - b) <= (ha - la) + (hb - lb) + 2 * WIDEN).all()


@pytest.mark.parametrize("name", ["lens_near", "lens_far"])
def test_lens_out_of_focus_differs(render, name):
    """the lens cases are not vacuous: out of focus most pixels mix other cells than the pinhole's"""
    a, b = render(name), render("pinhole_form0")
    assert (np.abs(a - b).max(2) > 1e-3).mean() > 0.5


def test_rng_restatement(oracle_lib):
    """the numpy RNG is the stream the integrator draws from (orc_rng_stream: the first draws of a path)"""
    seeds = C.frame_seeds()
    assert [oracle_lib.frame_seed(1, i) for i in range(16)] == seeds.tolist()
    for pix, fs in ((0, 0), (12345, 678), (1023, int(seeds[3])), (0xffffffff, 0xfffffff0), (2 ** 31, 2 ** 31 + 5)):
        st = C.rng_seed(np.array([pix], np.uint64), fs)
        mine = []
        for _ in range(64):
            st, u = C.rng_next(st)
            mine.append(F32(u[0]))
        assert oracle_lib.rng_stream(pix, fs, 64).tolist() == mine
    assert C.pixel_index(np.array([17]), np.array([33]), 40, True).tolist() == [2 * 3 + 1] and C.pixel_index(np.array([17]), np.array([33]), 40).tolist() == [33 * 40 + 17]
    # uniform_32bit: the top 128 states round to exactly 1
    st = np.array([0xffffff80, 0xffffff7f, 1 << 31], np.uint64)
    assert (st.astype(F32) * F32(2.0 ** -32)).tolist() == [1.0, float(F32(0xffffff7f) * F32(2.0 ** -32)), 0.5]


def test_wrong_rules_are_caught(replays):
    """a lens that focuses along the ray instead of along the view axis, and a lens radius of r k1 instead of r sqrt(k1): the right replay's interval
    (standing in for a correct implementation's image) must leave the wrong replay's, by more than the widening, on at least 5 % of the pixels"""
    for wrong in ("focal_along_ray", "lens_radius_linear"):
        for name in ("lens_near", "lens_far", "lens_oblique"):
            lo, hi, _ = replay(replays, name)
            wlo, whi, _ = replay(replays, name, wrong)
            miss = (np.maximum(lo - whi, wlo - hi) > WIDEN).any(2).mean()
            print(f"wrong rule {wrong} on {name}: caught on {miss:.3f} of the pixels")
            assert miss >= 0.05, (wrong, name, miss)
