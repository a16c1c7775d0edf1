"""Denoised display: an id-guided a-trous filter in front of the tone map (crh_denoise.cpp, cadrays_amd/csrc/denoise_kernels.hip).

The reference has no counterpart: OCCT's path tracer shows the raw accumulation.  Every comparison of two images is bit for bit, as uint32 views; the only
inequality in this file is the last test's "the filtered 1-spp image is closer to the converged one than the unfiltered one".

  CPU   the struct's layout and the exports; crh_denoise_host == the numpy restatement (tests/denoise_reference.py, written from the header's text) on synthetic
        planes of every frame size and level count; the main case is not vacuous (asserted from the numpy side); each deliberately wrong rule changes the image;
        the exactness case; every refusal
  GPU   crh_read_denoised == the host twin (== numpy) fed with crh_save_accum, crh_read_ids and crh_outline_table_host of the same state, through the states of a
        live scene, tile subsets, adaptive sampling and every level's threshold; the LDR read-outs == those of a second context that was handed the filtered image;
        the asynchronous read-outs; nothing else moves; and it denoises

ONE NEGATIVE CONTROL OF THE ISSUE IS NOT AS IT STATES IT: "weights normalised to /256 before summing" cannot break bit-equality.  1 / 256 is a power of two: every
product, every partial sum and the weight sum are scaled exactly, and the final division cancels the scale exactly (no value of the main case comes near the
denormals).  test_power_of_two_scaling_cannot_change_a_bit pins that.  The control that keeps the issue's intent -- normalise the weights BEFORE summing instead of
dividing the sum afterwards -- divides each weight by the pixel's own weight sum first ("normalised"); that one rounds differently and must break equality.
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as ref
from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("crh_denoise_defaults", "crh_set_denoise", "crh_get_denoise", "crh_read_denoised", "crh_denoise_host", "crh_bench_denoise")
bits = ref.bits


def _host():
    """the host-only entry point through the Python mirror: a missing one FAILS here (AttributeError / ImportError), it does not skip"""
    from cadrays_amd.view import denoise_host
    return denoise_host


def where_differs(a, b):
    d = (bits(a) != bits(b)).any(-1)
    return int(d.sum()), [(int(y), int(x), a[y, x].tolist(), b[y, x].tolist()) for y, x in np.argwhere(d)[:3]]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_denoise_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in abi.crh_denoise_params._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(crh_denoise_params));' + "".join(
        f'printf("%zu ", offsetof(crh_denoise_params, {n}));' for n in fields) + 'return 0;}'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [C.sizeof(abi.crh_denoise_params)] + [getattr(abi.crh_denoise_params, n).offset for n in fields] == [16, 0, 4, 8, 12], got
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS and (f"CRH_API int {name}(" in header or f"CRH_API void {name}(" in header), name
    section = header[header.index("--- denoised display"):header.index("--- kernel-level entry points")]
    assert section.count("no counterpart in the reference: OCCT's path tracer shows the raw accumulation") >= len(NAMES)


def test_entry_points_are_exported_and_defaults_agree(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    hip_lib.crh_env_table.restype = C.c_char_p
    assert b"CRH_DENOISE_STAGED\t" in hip_lib.crh_env_table()                                      # the switch between the two forms of the pass kernel
    p = abi.crh_denoise_params()
    hip_lib.crh_denoise_defaults.restype = None
    hip_lib.crh_denoise_defaults(C.byref(p)); hip_lib.crh_denoise_defaults(None)
    d = abi.DENOISE_DEFAULTS
    assert (p.levels, p.until_samples) == (d["levels"], d["until_samples"]) == (ref.DEFAULTS["levels"], ref.DEFAULTS["until_samples"]) == (4, 256)
    assert f32(p.normal_cos) == f32(d["normal_cos"]) == ref.DEFAULTS["normal_cos"] and f32(p.depth_ratio) == f32(d["depth_ratio"]) == ref.DEFAULTS["depth_ratio"]


# ------------------------------------------------------------------------------------------------ CPU 2: the host twin against numpy
def twin_of(case, **params):
    return _host()(case["rgba"], case["ob"], case["tr"], case["t"], case["table"], **params)


def numpy_of(case, wrong=None, stats=None, **params):
    p = dict(ref.DEFAULTS); p.update(params)
    return ref.denoise(case["rgba"], case["ob"], case["tr"], case["t"], case["table"], wrong=wrong, stats=stats, **p)


@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_restatement(hip_lib, size):
    """levels 1..5 on every frame: at step 16 the window (65 pixels) is wider than 1x1, 1x7, 5x300 across and 130x3 down"""
    case = ref.case(*size)
    for levels in (1, 2, 3, 4, 5):
        p = dict(ref.MAIN_PARAMS, levels=levels)
        got, want = twin_of(case, **p), numpy_of(case, **p)
        assert got.dtype == f32 and same_bits(got, want), (size, levels, where_differs(got, want))
        assert np.array_equal(bits(got)[..., 3], bits(case["rgba"])[..., 3])                  # the sample count travels untouched
    for p in (dict(ref.DEFAULTS), dict(levels=3, until_samples=8, normal_cos=1.0, depth_ratio=1.0), dict(levels=5, until_samples=1 << 20, normal_cos=1e-6, depth_ratio=1e30)):
        got, want = twin_of(case, **p), numpy_of(case, **p)
        assert same_bits(got, want), (size, p, where_differs(got, want))
    # no table at all: only pixels of one triangle mix
    got, want = twin_of(dict(case, table=None), **ref.MAIN_PARAMS), numpy_of(dict(case, table=None), **ref.MAIN_PARAMS)
    assert same_bits(got, want), (size, where_differs(got, want))


MAIN = {}


def main():
    """the main case, its numpy answer and what the numpy side saw on the way: computed once, shared, never changed"""
    if not MAIN:
        case, stats = ref.main_case(), {}
        want = numpy_of(case, stats=stats, **ref.MAIN_PARAMS)
        for a in list(case.values()) + [want]:
            a.setflags(write=False)
        MAIN.update(case=case, want=want, stats=stats)
    return MAIN["case"], MAIN["want"], MAIN["stats"]


def test_main_case_is_not_vacuous(hip_lib):
    case, want, stats = main()
    assert same_bits(twin_of(case, **ref.MAIN_PARAMS), want)
    levels = stats["levels"]
    assert len(levels) == ref.MAIN_PARAMS["levels"] == 5
    hit = levels[0]["hit"]
    for k, lv in enumerate(levels):
        assert lv["filtered"] > 0, k                                                             # every level is active ...
        assert 4 * lv["two_or_more"] >= hit, (k, lv["two_or_more"], hit)                         # ... and a quarter of the hit pixels accept two or more taps
        assert all(lv["through"][why] > 0 for why in ref.PASS_REASONS), (k, lv["through"])       # every pass-through reason
    for why in ref.DROP_REASONS:                                                                 # every reason to drop a tap
        assert sum(lv["drops"][why] for lv in levels) > 0, why
        assert levels[0]["drops"][why] > 0, (why, levels[0]["drops"])
    assert [lv["filtered"] for lv in levels] == sorted([lv["filtered"] for lv in levels], reverse=True) and levels[0]["filtered"] > levels[4]["filtered"]
    assert not same_bits(want, case["rgba"])


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_each_wrong_rule_breaks_bit_equality(hip_lib, wrong):
    """the main case tells the rule from its near misses: were the library to implement one of them, the tests above would fail"""
    case, want, _ = main()
    broken = numpy_of(case, wrong=wrong, **ref.MAIN_PARAMS)
    share = ref.share_differing(broken, twin_of(case, **ref.MAIN_PARAMS))
    print(f"wrong rule '{wrong}': {100.0 * share:.1f} % of the pixels differ")
    assert share > 0.0, wrong


def test_power_of_two_scaling_cannot_change_a_bit(hip_lib):
    """(the module's docstring)  colours scaled by 1 / 256 -- the same products and sums as weights scaled by 1 / 256 -- give the image scaled by 1 / 256"""
    case, want, _ = main()
    scaled = dict(case, rgba=case["rgba"] * np.array([1 / 256, 1 / 256, 1 / 256, 1], f32))
    got = twin_of(scaled, **ref.MAIN_PARAMS)
    assert same_bits(got, want * np.array([1 / 256, 1 / 256, 1 / 256, 1], f32))


def test_exactness_case(hip_lib):
    case = ref.exact_case()
    for p in (ref.MAIN_PARAMS, ref.DEFAULTS):
        got = twin_of(case, **p)
        assert same_bits(got, case["rgba"]) and same_bits(numpy_of(case, **p), case["rgba"])      # every partial sum is exact, and no colour crosses the boundary
    # ... which a filter that ignored the objects would: the same planes as ONE object
    one = twin_of(dict(case, ob=np.zeros_like(case["ob"])), **ref.MAIN_PARAMS)
    assert not same_bits(one, case["rgba"])


def test_properties_that_need_no_restatement(hip_lib):
    case, want, _ = main()
    rgba, ob, tr = case["rgba"], case["ob"], case["tr"]
    through = (tr < 0) | ~(rgba[..., 3] > 0) | ~np.isfinite(rgba[..., :3]).all(-1)
    assert np.array_equal(bits(want)[through], bits(rgba)[through])                               # bitwise, NaN payloads included
    assert np.isfinite(want[~through][:, :3]).all()                                               # nothing that is not finite spreads
    enough = rgba[..., 3] >= ref.MAIN_PARAMS["until_samples"]
    assert enough.any() and np.array_equal(bits(want)[enough], bits(rgba)[enough])
    # transposing all planes transposes the image only up to the order of summation: the taps' weights are symmetric, their order is not -- so not asserted; but a
    # frame of ONE pixel, and levels whose thresholds no pixel meets, return the input
    assert same_bits(twin_of(case, levels=5, until_samples=1), rgba)
    one = {k: (v[:1, :1] if k != "table" else v) for k, v in case.items()}
    assert same_bits(twin_of(one, **ref.MAIN_PARAMS), one["rgba"])
    # a filtered pixel is a convex combination of pixels of its own object
    lo, hi = {}, {}
    fin = np.isfinite(rgba[..., :3]).all(-1) & (rgba[..., 3] > 0)
    for o in np.unique(ob[ob >= 0]):
        m = (ob == o) & fin
        lo[o], hi[o] = rgba[m][:, :3].min(0), rgba[m][:, :3].max(0)
    for o in lo:
        m = (ob == o) & ~through
        assert (want[m][:, :3] >= lo[o] * f32(1 - 1e-5)).all() and (want[m][:, :3] <= hi[o] * f32(1 + 1e-5)).all(), o


# ------------------------------------------------------------------------------------------------ CPU 3: refusals
BAD = ((dict(levels=0), "levels lies outside 1..5"), (dict(levels=6), "levels lies outside 1..5"), (dict(levels=0xFFFFFFFF), "levels lies outside 1..5"),
       (dict(normal_cos=0.0), "normal_cos lies outside"), (dict(normal_cos=-0.5), "normal_cos lies outside"), (dict(normal_cos=1.0000001), "normal_cos lies outside"),
       (dict(depth_ratio=0.999), "depth_ratio is below 1"), (dict(depth_ratio=-2.0), "depth_ratio is below 1"),
       (dict(until_samples=0), "until_samples lies outside"), (dict(until_samples=(1 << 20) + 1), "until_samples lies outside"),
       (dict(normal_cos=float("nan")), "hold a NaN / Inf"), (dict(normal_cos=float("inf")), "hold a NaN / Inf"), (dict(normal_cos=float("-inf")), "hold a NaN / Inf"),
       (dict(depth_ratio=float("nan")), "hold a NaN / Inf"), (dict(depth_ratio=float("inf")), "hold a NaN / Inf"), (dict(depth_ratio=float("-inf")), "hold a NaN / Inf"))


def test_refusals_of_the_host_entry_point(hip_lib):
    host = _host()
    case = ref.case(5, 4)
    args = (case["rgba"], case["ob"], case["tr"], case["t"], case["table"])
    host(*args, levels=1, normal_cos=1.0, depth_ratio=1.0, until_samples=1); host(*args, levels=5, normal_cos=1e-6, depth_ratio=1e30, until_samples=1 << 20)      # the limits themselves
    for bad, _ in BAD:
        with pytest.raises(BackendError):
            host(*args, **bad)
    # NULL pointers and empty frames, straight at the library
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rgba, ob, t, tab = case["rgba"], case["ob"], case["t"], case["table"]
    out = np.zeros_like(rgba)
    pr, po, pt, pout, ptab = rgba.ctypes.data_as(fp), ob.ctypes.data_as(i32p), t.ctypes.data_as(fp), out.ctypes.data_as(fp), tab.ctypes.data_as(C.c_void_p)
    W, H, nT, zero = C.c_uint32(5), C.c_uint32(4), C.c_uint32(len(tab)), C.c_uint32(0)
    p = abi.crh_denoise_params(); hip_lib.crh_denoise_defaults.restype = None; hip_lib.crh_denoise_defaults(C.byref(p))
    fn = hip_lib.crh_denoise_host
    assert fn(pr, po, po, pt, W, H, ptab, nT, C.byref(p), pout) == abi.OK and fn(pr, po, po, pt, W, H, None, zero, C.byref(p), pout) == abi.OK
    assert fn(None, po, po, pt, W, H, ptab, nT, C.byref(p), pout) == abi.E_INVALID and fn(pr, None, po, pt, W, H, ptab, nT, C.byref(p), pout) == abi.E_INVALID
    assert fn(pr, po, None, pt, W, H, ptab, nT, C.byref(p), pout) == abi.E_INVALID and fn(pr, po, po, None, W, H, ptab, nT, C.byref(p), pout) == abi.E_INVALID
    assert fn(pr, po, po, pt, W, H, ptab, nT, None, pout) == abi.E_INVALID and fn(pr, po, po, pt, W, H, ptab, nT, C.byref(p), None) == abi.E_INVALID
    assert fn(pr, po, po, pt, zero, H, ptab, nT, C.byref(p), pout) == abi.E_INVALID and fn(pr, po, po, pt, W, zero, ptab, nT, C.byref(p), pout) == abi.E_INVALID
    assert fn(pr, po, po, pt, W, H, None, nT, C.byref(p), pout) == abi.E_INVALID                  # a count without a table
    assert hip_lib.crh_set_denoise(None, C.byref(p)) == abi.E_INVALID and hip_lib.crh_get_denoise(None, None, None) == abi.E_INVALID
    assert hip_lib.crh_read_denoised(None, pout) == abi.E_INVALID


# ================================================================================================ GPU
def scene_table(pos, tri):
    from cadrays_amd.view import outline_table_host
    return outline_table_host(pos, tri)


def twin_of_view(v, tab, **params):
    """crh_denoise_host over what the context itself hands out: the accumulator, the id planes, the table of its geometry"""
    acc, _ = v.save_accum()
    ob, tr, t = v.read_ids()
    return _host()(acc, ob, tr, t, tab, **params), acc, (ob, tr, t)


def assert_device_equals_twin(v, tab, also_numpy=False, **params):
    got = v.read_denoised()
    want, acc, (ob, tr, t) = twin_of_view(v, tab, **params)
    assert got.shape == want.shape and same_bits(got, want), where_differs(got, want)
    if also_numpy:
        p = dict(ref.DEFAULTS); p.update(params)
        again = ref.denoise(acc, ob, tr, t, tab, **p)
        assert same_bits(got, again), where_differs(got, again)
    return got, acc, (ob, tr, t)


def live_scene(W, H):
    """the Cornell room with its two boxes and the tessellated spheres, every material an object; then objects moved, one erased, one added whose two quads are
    COINCIDENT (and a welded roof): returns (view, table of the grown geometry)"""
    from cadrays_amd.view import View
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    v.set_transforms(moved_xforms(7))
    v.set_visibility(visible_flags(7, [4]))
    p = np.array([(0.35, 0.25, 0.35), (0.5, 0.1, 0.35), (0.5, 0.1, 0.65), (0.35, 0.25, 0.65), (0.65, 0.25, 0.35), (0.65, 0.25, 0.65),
                  (0.1, 0.3, 0.1), (0.3, 0.3, 0.1), (0.3, 0.3, 0.3), (0.1, 0.3, 0.3), (0.1, 0.3, 0.1), (0.3, 0.3, 0.1), (0.3, 0.3, 0.3), (0.1, 0.3, 0.3)], f32)
    n = np.tile(np.array([0, -1, 0], f32), (len(p), 1))
    t = np.array([(0, 1, 2, 0), (0, 2, 3, 0), (1, 4, 5, 0), (1, 5, 2, 0), (6, 7, 8, 0), (6, 8, 9, 0), (10, 12, 11, 0), (10, 13, 12, 0)], np.int32)
    assert v.add_object(p, n, t, rigid()) == 7
    pos2 = np.concatenate([sc.pos, p]); tri2 = np.concatenate([sc.tri, t + np.array([len(sc.pos)] * 3 + [0], np.int32)])
    return v, sc, scene_table(pos2, tri2)


FORMS = pytest.mark.parametrize("staged", ["0", "1"], ids=["plain_gather", "lds_staged"])      # CRH_DENOISE_STAGED, read when a context is created (crh_env_table)


@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("size", [(67, 45), (1, 1), (5, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_twin_through_a_live_scene_and_every_threshold(hip_lib, monkeypatch, size, staged):
    monkeypatch.setenv("CRH_DENOISE_STAGED", staged)
    W, H = size
    v, sc, tab = live_scene(W, H)
    assert v.get_denoise()["on"] is False
    v.Redraw()                                                                   # 1 spp, the defaults while the feature is off
    got, acc, (ob, tr, t) = assert_device_equals_twin(v, tab, also_numpy=True, **ref.DEFAULTS)
    if W * H > 1000:
        assert (ob == 7).any() and (tr[ob == 7] >= len(sc.tri)).all() and not (ob == 4).any() and not same_bits(got, acc)
    v.Redraw(); v.Redraw()                                                       # 3 spp
    assert_device_equals_twin(v, tab, **ref.DEFAULTS)
    # until_samples = 8, levels = 3: level 2 works below 0.5 samples (never), level 1 below 2, level 0 below 8
    p = dict(levels=3, normal_cos=ref.DEFAULTS["normal_cos"], depth_ratio=ref.DEFAULTS["depth_ratio"], until_samples=8)
    v.reset()
    v.set_denoise(True, **p)
    seen = []
    for spp in (1, 2, 3, 8):
        while v.save_accum()[1] < spp:
            v.Redraw()
        got, acc, _ = assert_device_equals_twin(v, tab, also_numpy=(spp == 2), **p)
        seen.append(got)
        if spp == 8:
            assert same_bits(got, acc)                                           # from until_samples on the displayed image IS the accumulator
        elif W * H > 1000:
            assert not same_bits(got, acc)
    if W * H > 1000:
        assert not same_bits(seen[0], seen[1]) and not same_bits(seen[1], seen[2])
    # the parameters in force are the ones crh_read_denoised uses; NULL goes back to the defaults
    v.set_denoise(False)
    assert_device_equals_twin(v, tab, **ref.DEFAULTS)
    v.close()


@pytest.mark.gpu
@FORMS
def test_device_equals_twin_with_unsampled_tiles_and_adaptive_sample_counts(hip_lib, monkeypatch, staged):
    monkeypatch.setenv("CRH_DENOISE_STAGED", staged)
    W, H = 67, 45                                                                # 3 x 2 tiles of 32
    v, sc, tab = live_scene(W, H)
    v.set_denoise(True)
    v.render_tiles(np.array([0, 2, 4], np.uint32), 0, 1)                         # a subset: the other tiles have no sample
    got, acc, (ob, tr, t) = assert_device_equals_twin(v, tab, also_numpy=True, **ref.DEFAULTS)
    w = acc[..., 3]
    assert ((w == 0) & (tr >= 0)).any() and ((w == 1) & (tr >= 0)).any()
    assert np.array_equal(bits(got)[w == 0], bits(acc)[w == 0])                  # an unsampled pixel is passed through ...
    v.close()
    v, sc, tab = live_scene(W, H)
    v.set_adaptive(True, 1)                                                      # one tile per iteration: five iterations cannot leave six tiles with one count
    v.set_denoise(True, levels=5, until_samples=64)
    v.render(5)
    got, acc, _ = assert_device_equals_twin(v, tab, also_numpy=True, **dict(ref.DEFAULTS, levels=5, until_samples=64))
    assert len(np.unique(acc[..., 3])) >= 2                                      # the sample count varies from tile to tile
    v.close()


def ldr_of_a_context_handed(image, frames, sc, display, **state):
    """read_ldr of a fresh context of the same scene that got `image` through crh_load_accum, has the filter off and uses the display values given"""
    from cadrays_amd.view import View
    b = View(0).load_scene(sc)
    b.load_accum(image, frames)
    b.set_display(*display)
    if "outline" in state: b.SetOutline(**state["outline"])
    if "selection" in state: b.set_selection(*state["selection"])
    if "hover" in state: b.set_hover(*state["hover"])
    assert b.get_denoise()["on"] is False
    out = b.read_ldr()
    b.close()
    return out


@pytest.mark.gpu
def test_ldr_read_out_tone_maps_the_filtered_image_and_meters_the_unfiltered_one(hip_lib):
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = object_scene(None, W, H)
    a = View(0).load_scene(sc)
    for _ in range(2): a.Redraw()
    plain = a.read_ldr()
    d = a.get_display()
    display = (d["tonemap_mode"], d["exposure"], d["white_point"])
    a.SetDenoise()
    filtered, frames = a.read_denoised(), a.save_accum()[1]
    assert not same_bits(filtered, a.save_accum()[0])
    got = a.read_ldr()
    assert not np.array_equal(got, plain)
    assert np.array_equal(got, ldr_of_a_context_handed(filtered, frames, sc, display))
    # auto exposure: the second context takes its display values from the FIRST one's crh_measure_exposure, which reads the unfiltered accumulator -- were the
    # metering to read the filtered image, the histogram (and the bytes) would differ
    a.set_auto_exposure(True)
    m = a.measure_exposure()
    metered = a.read_ldr()
    assert np.array_equal(metered, ldr_of_a_context_handed(filtered, frames, sc, (display[0], m["exposure"], m["white_point"])))
    a.ClearDenoise()
    m_off = a.measure_exposure()
    assert np.array_equal(m_off["hist"], m["hist"]) and m_off["exposure"] == m["exposure"] and m_off["white_point"] == m["white_point"]
    a.SetDenoise()
    a.set_auto_exposure(False)
    # outline, selection and hover sit on top, unchanged
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    state = dict(outline=dict(width=2, rgb=(0, 0, 255)), selection=(flags, (255, 0, 0), 128), hover=(4, (0, 255, 0), 64))
    a.SetOutline(**state["outline"]); a.set_selection(*state["selection"]); a.set_hover(*state["hover"])
    over = a.read_ldr()
    assert np.array_equal(over, ldr_of_a_context_handed(filtered, frames, sc, display, **state)) and not np.array_equal(over, got)
    # off again, or never set: the bytes of the parent
    a.ClearOutline(); a.set_selection(None); a.set_hover(-1); a.ClearDenoise()
    assert np.array_equal(a.read_ldr(), plain)
    a.close()


@pytest.mark.gpu
@FORMS
def test_two_read_backs_in_flight_each_equal_the_synchronous_bytes_of_their_moment(hip_lib, monkeypatch, staged):
    from cadrays_amd.view import View
    monkeypatch.setenv("CRH_DENOISE_STAGED", staged)
    W, H = 96, 64
    sc = object_scene(None, W, H)
    twin = View(0).load_scene(sc); twin.SetDenoise()
    for _ in range(2): twin.Redraw()
    s1 = twin.read_ldr()
    twin.render(1)
    s2 = twin.read_ldr()
    twin.close()
    v = View(0).load_scene(sc); v.SetDenoise()
    for _ in range(2): v.Redraw()
    v.read_ldr_begin()
    v.render(1)
    v.read_ldr_begin()
    e1, e2 = v.read_ldr_end(), v.read_ldr_end()
    assert np.array_equal(e1, s1) and np.array_equal(e2, s2) and not np.array_equal(s1, s2)
    v.ClearDenoise()
    v.read_ldr_begin()
    off = v.read_ldr_end()
    assert not np.array_equal(off, s2)
    v.close()


@pytest.mark.gpu
def test_the_filter_leaves_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 128, 96
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    ref_v = View(0).load_scene(sc)
    ref_v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(8): ref_v.Redraw()
    want, (want_acc, want_frames), want_stats, want_ldr = ref_v.read_hdr(), ref_v.save_accum(), ref_v.stats(), ref_v.read_ldr()
    want_ids, want_mask, want_bounds = ref_v.read_ids(), ref_v.read_outline(), ref_v.selection_bounds()
    # the feature set before the scene exists; every new call between blocks of frames; an asynchronous read-out in flight across a change of the parameters
    v = View(0)
    v.SetDenoise(levels=5)
    assert v.get_denoise()["on"] and v.get_denoise()["levels"] == 5
    v.load_scene(sc)
    assert v.get_denoise()["on"]                                                 # display state outlives a new scene
    v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(3): v.Redraw()
    v.read_ldr_begin()
    v.read_denoised()
    v.SetDenoise(levels=2, until_samples=16)
    v.read_ldr_end()
    for _ in range(5): v.Redraw()
    v.read_ldr(); v.read_denoised(); v.get_denoise()
    acc, frames = v.save_accum()
    assert same_bits(v.read_hdr(), want) and frames == want_frames == 8 and same_bits(acc, want_acc)
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    ids = v.read_ids()
    assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(ids, want_ids))
    assert np.array_equal(v.read_outline(), want_mask)
    assert all(np.array_equal(a, b) for a, b in zip(v.selection_bounds(), want_bounds))
    v.ClearDenoise()
    assert np.array_equal(v.read_ldr(), want_ldr)                                # the selection still drawn, and the bytes of a context that never called crh_set_denoise
    v.close()
    # in a free-running loop, three frames in flight, filtered read-backs in flight
    v = View(0).load_scene(sc); v.set_pipeline_depth(3)
    v.set_selection(flags, (255, 0, 0), 128)
    v.SetDenoise()
    for k in range(8):
        v.Redraw()
        if k in (2, 5):
            v.read_ldr_begin(); v.read_denoised(); v.read_ldr_end()
        elif k == 3:
            v.SetDenoise(levels=1, normal_deg=60.0)
    assert same_bits(v.read_hdr(), want) and v.save_accum()[1] == 8
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    v.ClearDenoise()
    assert np.array_equal(v.read_ldr(), want_ldr)
    v.close(); ref_v.close()


@pytest.mark.gpu
def test_set_denoise_refusals_and_state(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    d = v.get_denoise()
    assert d["on"] is False and (d["levels"], d["until_samples"]) == (4, 256) and d["normal_cos"] == ref.DEFAULTS["normal_cos"] and d["depth_ratio"] == ref.DEFAULTS["depth_ratio"]
    for bad, why in BAD:
        with pytest.raises(BackendError, match=f"-> -1: crh_set_denoise: .*{why}"):
            v.set_denoise(True, **bad)
        assert v.get_denoise()["on"] is False                                    # a refused call changes nothing
    v.set_denoise(True, levels=5, normal_cos=1.0, depth_ratio=1.0, until_samples=1 << 20)      # the limits themselves; allowed before crh_build
    g = v.get_denoise()
    assert g["on"] and (g["levels"], float(g["normal_cos"]), float(g["depth_ratio"]), g["until_samples"]) == (5, 1.0, 1.0, 1 << 20)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4.*crh_build has not been called"):
        v.read_denoised()
    assert v._fn("read_denoised")(v._ctx, None) == abi.E_INVALID
    v.load_scene(sc)
    v.Redraw()
    assert_device_equals_twin(v, scene_table(sc.pos, sc.tri), levels=5, normal_cos=1.0, depth_ratio=1.0, until_samples=1 << 20)
    v.close()


def closed_room(W, H):
    """a small CLOSED diffuse scene with one light: the Cornell room with its two boxes, every BSDF diffuse, a front wall added behind the camera, the camera inside
    looking at the back wall, and the room's positional light moved above and behind the field of view (77 degrees off the axis of a 45-degree camera).  The light
    is kept out of view on purpose: a positional light that a camera ray passes REPLACES the hit in the image but not in the id buffer (include/cadrays_hip.h,
    crh_light), so the guide takes its disc for the wall behind it -- a stated known limit of the rule, measured in profiles/denoise_ab.md, not this test's subject"""
    sc = scenes.cornell_box(False, W, H)
    k = len(sc.pos)
    pos = np.concatenate([sc.pos, np.array([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], f32)])
    nrm = np.concatenate([sc.nrm, np.tile(np.array([0, 1, 0], f32), (4, 1))])
    tri = np.concatenate([sc.tri, np.array([(k, k + 1, k + 2, 2), (k, k + 2, k + 3, 2)], np.int32)])
    cam = dataclasses.replace(sc.camera, eye=(0.5, 0.03, 0.5))
    return dataclasses.replace(sc, pos=pos, nrm=nrm, tri=tri, camera=cam, lights=[scenes.Light.positional((0.5, 0.12, 0.9), smoothness=0.06, intensity=25.0)])


@pytest.mark.gpu
def test_it_denoises(hip_lib):
    """THE test that fails without the feature.  closed_room at 96 x 64: over the hit pixels (all of them: the room is closed), the mean squared error of
    crh_read_denoised at 1 spp against crh_read_hdr at 1024 spp is strictly below the error of the unfiltered 1-spp image.  No other value is fixed: the measured
    ratio is printed (profiles/denoise_ab.md carries it)."""
    from cadrays_amd.view import View
    W, H = 96, 64
    v = View(0).load_scene(closed_room(W, H))
    v.Redraw()
    raw = v.read_hdr().astype(np.float64)
    filtered = v.read_denoised()
    assert same_bits(v.save_accum()[0][..., :3], v.read_hdr()) and (filtered[..., 3] == 1.0).all()
    hit = v.read_ids()[1] >= 0
    v.render(1023)
    assert v.save_accum()[1] == 1024
    truth = v.read_hdr().astype(np.float64)
    v.close()
    mse_raw = float(((raw - truth)[hit] ** 2).mean())
    mse_filtered = float(((filtered[..., :3].astype(np.float64) - truth)[hit] ** 2).mean())
    print(f"1 spp against 1024 spp over {int(hit.sum())} hit pixels: mse raw {mse_raw:.6g}, filtered {mse_filtered:.6g}, ratio {mse_filtered / mse_raw:.4f}")
    assert hit.all() and mse_raw > 0.0 and truth.max() < 25.0                    # closed, noisy, and no pixel shows the light itself
    assert mse_filtered < mse_raw
