"""Reprojected display history: the image an ending view displayed, blended into the next view's in front of the denoise filter and the tone map
(crh_reproject.cpp, cadrays_amd/csrc/reproject_kernels.hip).

The reference has no counterpart: OCCT's path tracer shows the raw accumulation.  Every comparison of two images is bit for bit, as uint32 views; the only
inequality in this file is the last test's "eight reprojected drag steps are closer to the converged image than the raw 1-spp frame", whose bar (half the error: two
effective samples already give it) is the issue's condition, not a measurement.

  CPU   the structs' layout and the exports; crh_reproject_host == the numpy restatement (tests/reproject_reference.py, written from the header's text) on two views
        of an analytic scene, every frame size, camera pair and both camera models; the main case is not vacuous (asserted from the numpy side); each deliberately
        wrong rule changes the image; properties that need no restatement; every refusal (make -C cadrays_amd/csrc sanitize-reproject runs the twin under
        ASan + UBSan in a stand-alone program: not from here, it compiles the whole library)
  GPU   crh_read_reprojected == the host twin fed with crh_save_accum, crh_read_ids and crh_camera_rays of both views, through every pass-through branch; the
        recursion over five camera steps; the history's life cycle; the LDR read-outs; read-backs in flight across a capture; nothing else moves; and it helps
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import reproject_reference as ref
from cadrays_amd import abi
from cadrays_amd.binding import BackendError
from test_denoise import closed_room, ldr_of_a_context_handed, scene_table
from test_two_level import moved_xforms, object_scene
from test_visibility import visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("crh_reproject_defaults", "crh_set_reproject", "crh_get_reproject", "crh_read_reprojected", "crh_bench_reproject", "crh_reproject_frame_host", "crh_reproject_host")
bits = ref.bits


def _host():
    """the host-only entry point through the Python mirror: a missing one FAILS here (AttributeError / ImportError), it does not skip"""
    from cadrays_amd.view import reproject_host
    return reproject_host


def where_differs(a, b):
    d = (bits(a) != bits(b)).any(-1)
    return int(d.sum()), [(int(y), int(x), a[y, x].tolist(), b[y, x].tolist()) for y, x in np.argwhere(d)[:3]]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_reproject_structs_layout_matches_header(tmp_path):
    got = []
    for struct, name in ((abi.crh_reproject_params, "crh_reproject_params"), (abi.crh_reproject_frame, "crh_reproject_frame")):
        fields = [n for n, _ in struct._fields_]
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(' + name + '));' + "".join(
            f'printf("%zu ", offsetof({name}, {n}));' for n in fields) + 'return 0;}'
        (tmp_path / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
        out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
        assert out == [C.sizeof(struct)] + [getattr(struct, n).offset for n in fields], (name, out)
        got.append(out)
    assert got == [[16, 0, 4, 8, 12], [64, 0, 12, 24, 36, 48, 52, 56, 60]], got
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS and (f"CRH_API int {name}(" in header or f"CRH_API void {name}(" in header), name
    section = header[header.index("--- reprojected display history"):header.index("--- kernel-level entry points")]
    assert section.count("no counterpart in the reference: OCCT's path tracer shows the raw accumulation") >= len(NAMES)
    for limit in ("raygen_bilinear != 0 the feature NEVER captures", "view-dependent shading", "repeated bilinear"):
        assert limit in section, limit


def test_entry_points_are_exported_and_defaults_agree(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    p = abi.crh_reproject_params()
    hip_lib.crh_reproject_defaults.restype = None
    hip_lib.crh_reproject_defaults(C.byref(p)); hip_lib.crh_reproject_defaults(None)
    d = abi.REPROJECT_DEFAULTS
    assert (p.max_history, p.until_samples) == (d["max_history"], d["until_samples"]) == (ref.DEFAULTS["max_history"], ref.DEFAULTS["until_samples"]) == (16.0, 64)
    assert f32(p.normal_cos) == f32(d["normal_cos"]) == ref.DEFAULTS["normal_cos"] and f32(p.depth_ratio) == f32(d["depth_ratio"]) == ref.DEFAULTS["depth_ratio"]


# ------------------------------------------------------------------------------------------------ CPU 2: the host twin against numpy
def twin_of(case, **params):
    return _host()(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], **params)


def numpy_of(case, wrong=None, stats=None, **params):
    p = dict(ref.DEFAULTS); p.update(params)
    return ref.reproject(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], wrong=wrong, stats=stats, **p)


OTHER_PARAMS = (dict(max_history=1.0, until_samples=1, normal_cos=1.0, depth_ratio=1.0), dict(max_history=1024.0, until_samples=1 << 20, normal_cos=1e-6, depth_ratio=1e30),
                dict(max_history=4.5, until_samples=3, normal_cos=0.5, depth_ratio=1.2))


@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
@pytest.mark.parametrize("pair", ref.PAIRS)
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_restatement(hip_lib, size, pair, ortho):
    case = ref.case(*size, pair, ortho)
    stats = {}
    got, want = twin_of(case, **ref.DEFAULTS), numpy_of(case, stats=stats, **ref.DEFAULTS)
    assert got.dtype == f32 and same_bits(got, want), (size, pair, ortho, where_differs(got, want))
    if pair == "half_turn":
        assert stats["projected"] == 0 and same_bits(got, case["a"])             # every z <= 0: the output is the accumulator, bitwise
    elif size == (67, 45):
        assert stats["took"] > 0 and not same_bits(got, case["a"]), (pair, ortho, stats["took"])
    for p in OTHER_PARAMS:
        got, want = twin_of(case, **p), numpy_of(case, **p)
        assert same_bits(got, want), (size, pair, ortho, p, where_differs(got, want))
    # no table at all (only taps of the same triangle count), and no history at all
    got, want = twin_of(dict(case, table=None), **ref.DEFAULTS), numpy_of(dict(case, table=None), **ref.DEFAULTS)
    assert same_bits(got, want), (size, pair, where_differs(got, want))
    assert same_bits(twin_of(dict(case, hist=None), **ref.DEFAULTS), case["a"])


MAIN = {}


def main():
    """the main case (the sideways step at 67 x 45), its numpy answer and what the numpy side saw on the way: computed once, shared, never changed"""
    if not MAIN:
        case, stats = ref.case(67, 45, "sideways"), {}
        want = numpy_of(case, stats=stats, **ref.DEFAULTS)
        for a in [case["a"], case["rays"], case["ob"], case["tr"], case["t"], want] + [case["hist"][k] for k in ("rgba", "ob", "tr", "t")]:
            a.setflags(write=False)
        MAIN.update(case=case, want=want, stats=stats)
    return MAIN["case"], MAIN["want"], MAIN["stats"]


def test_main_case_is_not_vacuous(hip_lib):
    case, want, st = main()
    assert same_bits(twin_of(case, **ref.DEFAULTS), want)
    print({k: v for k, v in st.items() if not isinstance(v, np.ndarray)})
    assert 2 * st["took"] >= st["hit"], (st["took"], st["hit"])                  # at least half of the hit pixels take history
    assert 100 * st["refused"] >= st["hit"], (st["refused"], st["hit"])          # at least 1 % are refused a tap by the depth or the object test: the disocclusion band
    assert st["refused_object"] >= 1 and st["refused_depth"] >= 1                # ... by each of the two
    assert st["fewer_than_four"] >= 1 and st["four"] >= 1                       # partial footprints and whole ones
    assert st["capped"] >= 1 and st["unsampled_took"] >= 1                       # the cap binds somewhere, and an unsampled pixel shows history alone
    assert not same_bits(want, case["a"])


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_each_wrong_rule_breaks_bit_equality(hip_lib, wrong):
    """the main case tells the rule from its near misses: were the library to implement one of them, the tests above would fail"""
    case, want, _ = main()
    broken = numpy_of(case, wrong=wrong, **ref.DEFAULTS)
    share = ref.share_differing(broken, twin_of(case, **ref.DEFAULTS))
    print(f"wrong rule '{wrong}': {100.0 * share:.1f} % of the pixels differ")
    assert share > 0.0, wrong


def test_properties_that_need_no_restatement(hip_lib):
    case, want, st = main()
    a, tr = case["a"], case["tr"]
    # background pixels, pixels that are not finite and pixels with enough samples of their own: bitwise the accumulator's
    through = (tr < 0) | ~np.isfinite(a[..., :3]).all(-1) | (a[..., 3] >= ref.DEFAULTS["until_samples"])
    assert (tr < 0).any() and (a[..., 3] >= ref.DEFAULTS["until_samples"]).any()
    assert np.array_equal(bits(want)[through], bits(a)[through])
    assert np.array_equal(bits(twin_of(case, **dict(ref.DEFAULTS, until_samples=1)))[a[..., 3] >= 1], bits(a)[a[..., 3] >= 1])
    assert np.isfinite(want[st["took_mask"]]).all()                              # nothing that is not finite spreads
    # the sample count: a.w + min(history, max_history) where history was taken
    took = st["took_mask"] & (a[..., 3] > 0)
    assert (want[took][:, 3] > a[took][:, 3]).all() and (want[took][:, 3] <= a[took][:, 3] + ref.DEFAULTS["max_history"]).all()
    # an IDENTICAL camera with a full history: every footprint is one tap of weight exactly 1 (integer pixel coordinates are exact here: a dyadic frame), so out.rgb
    # is the weighted mean (a * w + h * n) / (w + n), computed here in the same three steps
    W, H = 64, 32
    now = ref.make_frame((0.0, -8.0, 0.0), (0.0, 0.0, 0.0), W, H, ortho_scale=2.0)
    now["eye"], now["right"], now["up"], now["fwd"] = (np.array(v, f32) for v in ((0, -8, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)))
    rays = ref.rays_of(now, W, H)
    r = np.random.default_rng(5)
    acc = np.concatenate([r.random((H, W, 3)).astype(f32), np.full((H, W, 1), 2.0, f32)], -1)
    hist_img = np.concatenate([r.random((H, W, 3)).astype(f32), np.full((H, W, 1), 3.0, f32)], -1)
    ob, trp, t = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32), np.full((H, W), 8.0, f32)      # a wall at y = 0, one triangle
    one = dict(a=acc, rays=rays, ob=ob, tr=trp, t=t, hist=dict(rgba=hist_img, ob=ob, tr=trp, t=t, frame=now), table=None)
    stats = {}
    got = twin_of(one, **ref.DEFAULTS)
    assert same_bits(got, numpy_of(one, stats=stats, **ref.DEFAULTS))
    assert stats["took"] == W * H and (stats["n_taps"] == 1).all()
    mean = (acc[..., :3] * f32(2.0) + hist_img[..., :3] * f32(3.0)) / f32(5.0)
    assert mean.dtype == f32 and same_bits(got[..., :3], mean) and (got[..., 3] == 5.0).all()
    # scaling every radiance by a power of two scales the output exactly
    s = np.array([1 / 64, 1 / 64, 1 / 64, 1], f32)
    scaled = dict(case, a=case["a"] * s, hist=dict(case["hist"], rgba=case["hist"]["rgba"] * s))
    assert same_bits(twin_of(scaled, **ref.DEFAULTS), want * s)


# ------------------------------------------------------------------------------------------------ CPU 3: refusals
BAD = ((dict(max_history=0.5), "max_history lies outside"), (dict(max_history=1024.5), "max_history lies outside"), (dict(max_history=-1.0), "max_history lies outside"),
       (dict(until_samples=0), "until_samples lies outside"), (dict(until_samples=(1 << 20) + 1), "until_samples lies outside"),
       (dict(normal_cos=0.0), "normal_cos lies outside"), (dict(normal_cos=-0.5), "normal_cos lies outside"), (dict(normal_cos=1.0000001), "normal_cos lies outside"),
       (dict(depth_ratio=0.999), "depth_ratio is below 1"), (dict(depth_ratio=-2.0), "depth_ratio is below 1"),
       (dict(max_history=float("nan")), "hold a NaN / Inf"), (dict(max_history=float("inf")), "hold a NaN / Inf"),
       (dict(normal_cos=float("nan")), "hold a NaN / Inf"), (dict(normal_cos=float("-inf")), "hold a NaN / Inf"),
       (dict(depth_ratio=float("nan")), "hold a NaN / Inf"), (dict(depth_ratio=float("inf")), "hold a NaN / Inf"))


def test_refusals_of_the_host_entry_points(hip_lib):
    host = _host()
    case = ref.case(5, 4, "sideways")
    args = (case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"])
    host(*args, max_history=1.0, until_samples=1, normal_cos=1.0, depth_ratio=1.0); host(*args, max_history=1024.0, until_samples=1 << 20, normal_cos=1e-6, depth_ratio=1e30)
    for bad, _ in BAD:
        with pytest.raises(BackendError):
            host(*args, **bad)
    # NULL pointers and empty frames, straight at the library
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    a, rays, ob, t, tab, h = case["a"], case["rays"], case["ob"], case["t"], case["table"], case["hist"]
    out = np.zeros_like(a)
    F = abi.crh_reproject_frame(); F.aspect = 1.25; F.tan_half = 0.4; F.fwd[1] = 1.0; F.right[0] = 1.0; F.up[2] = 1.0
    pa, pr, po, pt, pout, ptab = a.ctypes.data_as(fp), rays.ctypes.data_as(fp), ob.ctypes.data_as(i32p), t.ctypes.data_as(fp), out.ctypes.data_as(fp), tab.ctypes.data_as(C.c_void_p)
    ph = h["rgba"].ctypes.data_as(fp)
    W, H, nT, zero = C.c_uint32(5), C.c_uint32(4), C.c_uint32(len(tab)), C.c_uint32(0)
    p = abi.crh_reproject_params(); hip_lib.crh_reproject_defaults.restype = None; hip_lib.crh_reproject_defaults(C.byref(p))
    fn = hip_lib.crh_reproject_host
    ok = lambda **kw: fn(*[kw.get(k, v) for k, v in (("a", pa), ("r", pr), ("o", po), ("tr", po), ("t", pt), ("h", ph), ("ho", po), ("htr", po), ("ht", pt), ("F", C.byref(F)),
                                                      ("tab", ptab), ("nT", nT), ("W", W), ("H", H), ("p", C.byref(p)), ("out", pout))])
    assert ok() == abi.OK and ok(tab=None, nT=zero) == abi.OK
    assert ok(h=None, ho=None, htr=None, ht=None, F=None) == abi.OK              # no history: none of its planes is needed
    for k in ("a", "r", "o", "tr", "t", "ho", "htr", "ht", "F", "p", "out"):
        assert ok(**{k: None}) == abi.E_INVALID, k
    assert ok(W=zero) == abi.E_INVALID and ok(H=zero) == abi.E_INVALID and ok(tab=None) == abi.E_INVALID      # a count without a table
    assert hip_lib.crh_set_reproject(None, C.byref(p)) == abi.E_INVALID and hip_lib.crh_get_reproject(None, None, None, None) == abi.E_INVALID
    assert hip_lib.crh_read_reprojected(None, pout) == abi.E_INVALID and hip_lib.crh_bench_reproject(None, C.c_uint32(1), None, None) == abi.E_INVALID
    cam = abi.crh_camera(); cam.dir[1] = 1.0; cam.up[2] = 1.0; cam.fovy_deg = 45.0
    assert hip_lib.crh_reproject_frame_host(C.byref(cam), W, H, C.byref(F)) == abi.OK and f32(F.aspect) == f32(1.25) and tuple(F.fwd) == (0.0, 1.0, 0.0)
    assert hip_lib.crh_reproject_frame_host(None, W, H, C.byref(F)) == abi.E_INVALID and hip_lib.crh_reproject_frame_host(C.byref(cam), W, H, None) == abi.E_INVALID
    assert hip_lib.crh_reproject_frame_host(C.byref(cam), zero, H, C.byref(F)) == abi.E_INVALID      # aspect <= 0 needs a frame size
    cam.eye[0] = float("nan")
    assert hip_lib.crh_reproject_frame_host(C.byref(cam), W, H, C.byref(F)) == abi.E_INVALID


# ================================================================================================ GPU
def turned(cam, yaw_deg=0.0, shift=(0.0, 0.0, 0.0), **more):
    """the camera turned about its up axis z and moved"""
    c, s = np.cos(np.deg2rad(yaw_deg)), np.sin(np.deg2rad(yaw_deg))
    d = cam.dir
    return dataclasses.replace(cam, dir=(float(c * d[0] - s * d[1]), float(s * d[0] + c * d[1]), float(d[2])), eye=tuple(float(e + k) for e, k in zip(cam.eye, shift)), **more)


def planes_of(v):
    """what the context itself hands out of the view in force: the accumulator, the pixel-centre rays, the id planes, the camera frame"""
    from cadrays_amd.view import reproject_frame_host
    W, H = v.width, v.height
    py, px = np.mgrid[0:H, 0:W]
    acc, frames = v.save_accum()
    ob, tr, t = v.read_ids()
    return dict(a=acc, frames=frames, rays=v.camera_rays(np.stack([px.ravel(), py.ravel()], 1)), ob=ob, tr=tr, t=t, frame=reproject_frame_host(v._camera, W, H))


def history_from(state, image):
    return dict(rgba=image, ob=state["ob"], tr=state["tr"], t=state["t"], frame=state["frame"])


def twin_of_view(v, hist, tab, **params):
    s = planes_of(v)
    return _host()(s["a"], s["rays"], s["ob"], s["tr"], s["t"], hist, tab, **params), s


def assert_device_equals_twin(v, hist, tab, **params):
    got = v.read_reprojected()
    want, s = twin_of_view(v, hist, tab, **params)
    assert got.shape == want.shape and same_bits(got, want), where_differs(got, want)
    return got, s


def live_scene(W, H, **cam):
    """the Cornell room, every material an object, two objects moved and one erased: (view, scene, table)"""
    from cadrays_amd.view import View
    sc = object_scene(None, W, H)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, **cam))
    v = View(0).load_scene(sc)
    v.set_transforms(moved_xforms(7))
    v.set_visibility(visible_flags(7, [4]))
    return v, sc, scene_table(sc.pos, sc.tri)


def move(v, cam):
    """INTEGRATION.md's sequence"""
    v.set_camera(cam)
    v.reset()


CAMS = pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])


@pytest.mark.gpu
@CAMS
@pytest.mark.parametrize("size", [(67, 45), (1, 1), (5, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_twin_through_a_live_scene_and_every_pass_through(hip_lib, size, ortho):
    W, H = size
    kind = dict(is_ortho=True, ortho_scale=0.55) if ortho else {}
    v, sc, tab = live_scene(W, H, **kind)
    P = dict(max_history=4.0, until_samples=3, normal_cos=ref.DEFAULTS["normal_cos"], depth_ratio=ref.DEFAULTS["depth_ratio"])
    g = v.get_reproject()
    assert g["on"] is False and g["history_valid"] is False
    v.set_reproject(True, **P)
    v.Redraw(); v.Redraw()
    first, s0 = assert_device_equals_twin(v, None, tab, **P)                      # no history yet: the accumulator, bitwise
    assert same_bits(first, s0["a"]) and v.get_reproject()["history_valid"] is False
    step = (1.5, (0.04, 0.0, 0.01)) if W >= 64 else (0.05, (0.001, 0.0, 0.01))      # (a frame five pixels wide sees a strip a fraction of a degree wide)
    move(v, turned(sc.camera, *step, **kind))
    assert v.get_reproject()["history_valid"] is True
    hist = history_from(s0, s0["a"])                                             # what view 0 displayed: without a history of its own, its accumulator
    seen = []
    for spp in (1, 2, 3):                                                        # until_samples - 2, until_samples - 1, until_samples
        v.Redraw()
        got, s1 = assert_device_equals_twin(v, hist, tab, **P)
        seen.append(got)
        assert s1["frames"] == spp
        if spp == 3:
            assert same_bits(got, s1["a"])                                       # a.w >= until_samples: the accumulator, bitwise
        elif W * H > 1000:
            hit = s1["tr"] >= 0
            assert not same_bits(got, s1["a"]) and (got[..., 3][hit] > spp).mean() > 0.5 and np.array_equal(bits(got)[~hit], bits(s1["a"])[~hit])
    # the parameters in force are the ones a read-out uses; changing them keeps the history
    P2 = dict(P, until_samples=64, max_history=1.5)
    v.set_reproject(True, **P2)
    assert v.get_reproject()["history_valid"] is True
    assert_device_equals_twin(v, hist, tab, **P2)
    v.close()


@pytest.mark.gpu
def test_device_equals_twin_with_unsampled_tiles_and_adaptive_sample_counts(hip_lib):
    W, H = 67, 45                                                                # 3 x 2 tiles of 32
    v, sc, tab = live_scene(W, H)
    v.set_reproject(True)
    v.Redraw()
    s0 = planes_of(v)
    move(v, turned(sc.camera, -1.0, (-0.03, 0.0, 0.0)))
    v.render_tiles(np.array([0, 2, 4], np.uint32), 0, 1)                         # a subset: the other tiles have no sample
    got, s1 = assert_device_equals_twin(v, history_from(s0, s0["a"]), tab, **ref.DEFAULTS)
    w, hit = s1["a"][..., 3], s1["tr"] >= 0
    assert ((w == 0) & hit).any() and ((w == 1) & hit).any()
    alone = (w == 0) & hit & (got[..., 3] > 0)
    assert alone.sum() > 100 and (got[..., 3][alone] <= 1.0).all()               # an unsampled tile shows the history alone, with the history's count
    v.close()
    v, sc, tab = live_scene(W, H)
    v.set_adaptive(True, 1)                                                      # one tile per iteration: the sample count varies from tile to tile
    v.set_reproject(True, until_samples=4)
    v.render(5)
    s0 = planes_of(v)
    move(v, turned(sc.camera, 0.8))
    assert v.get_reproject()["history_valid"] is True
    v.render(5)
    got, s1 = assert_device_equals_twin(v, history_from(s0, s0["a"]), tab, **dict(ref.DEFAULTS, until_samples=4))
    assert len(np.unique(s1["a"][..., 3])) >= 2 and not same_bits(got, s1["a"])
    v.close()


@pytest.mark.gpu
def test_recursion_over_five_camera_steps(hip_lib):
    """what is captured is the RESOLVED image: after every step the device image equals the twin applied to the twin's own previous output"""
    W, H = 67, 45
    v, sc, tab = live_scene(W, H)
    P = dict(ref.DEFAULTS, max_history=3.0)                                      # the cap binds from the fourth step on
    v.set_reproject(True, **P)
    v.Redraw()
    shown, s = assert_device_equals_twin(v, None, tab, **P)
    counts = []
    for k in range(1, 6):
        hist = history_from(s, shown)
        move(v, turned(sc.camera, 0.6 * k, (0.01 * k, 0.0, 0.0)))
        v.Redraw()
        shown, s = assert_device_equals_twin(v, hist, tab, **P)
        counts.append(float(shown[..., 3].max()))
    assert counts[:3] == [2.0, 3.0, 4.0] and counts[3] == counts[4] == 4.0, counts      # 1 + min(history, 3)
    v.close()


@pytest.mark.gpu
def test_life_cycle_of_the_history(hip_lib):
    W, H = 67, 45
    v, sc, tab = live_scene(W, H)
    valid = lambda: v.get_reproject()["history_valid"]
    cams = iter(turned(sc.camera, 0.3 * k) for k in range(1, 40))

    def capture():
        v.Redraw(); move(v, next(cams))
        assert valid() is True

    v.Redraw(); move(v, next(cams))
    assert valid() is False                                                      # the feature is off: set_camera captures nothing
    v.set_reproject(True)
    assert v.get_reproject()["on"] is True and valid() is False
    v.set_camera(next(cams))
    assert valid() is False                                                      # nothing rendered since the restart, no history: nothing to capture
    v.reset(); v.Redraw()
    v.reset(); v.set_camera(next(cams))
    assert valid() is False                                                      # the reverse order: the restart came first, frames_done is 0
    capture()
    v.Redraw(); v.set_camera(v._camera)
    v.reset()
    assert valid() is False                                                      # a crh_reset with no camera change drops it
    capture()
    v.set_camera(next(cams)); v.set_camera(next(cams)); v.reset()
    assert valid() is True                                                       # two camera changes in front of one restart: one capture, kept
    capture(); v.set_transforms(moved_xforms(7))
    assert valid() is False
    capture(); v.set_visibility(visible_flags(7, [4]))
    assert valid() is False
    capture(); v.set_materials(sc.materials)
    assert valid() is False
    capture(); v.set_lights(sc.lights)
    assert valid() is False
    capture(); v.set_params(dataclasses.replace(sc.params, width=40, height=30))
    assert valid() is False
    v.set_camera(next(cams))
    capture()                                                                    # ... and a history of the new size is taken like any other
    v.Redraw()
    assert not same_bits(v.read_reprojected(), v.save_accum()[0])
    v.set_params(sc.params)
    capture(); v.set_reproject(False)
    g = v.get_reproject()
    assert g["on"] is False and g["history_valid"] is False
    v.set_reproject(True)
    assert valid() is False                                                      # switching it on again brings nothing back
    # set_camera between capture and restart of a view that a setter other than crh_reset restarts: dropped
    v.Redraw(); v.set_camera(next(cams))
    assert valid() is True
    v.set_spec()
    assert valid() is False
    # raygen_bilinear != 0: never a capture
    v.set_spec(raygen_bilinear=1)
    v.Redraw(); move(v, next(cams))
    assert valid() is False
    v.Redraw()
    assert same_bits(v.read_reprojected(), v.save_accum()[0])
    v.set_spec()
    capture()
    v.close()


@pytest.mark.gpu
def test_ldr_read_out_shows_the_reprojected_image_and_meters_the_accumulator(hip_lib):
    from cadrays_amd.view import View, denoise_host
    W, H = 67, 45
    v, sc, tab = live_scene(W, H)
    v.SetReproject()
    v.Redraw(); v.Redraw()
    s0 = planes_of(v)
    move(v, turned(sc.camera, 1.0, (0.02, 0.0, 0.0)))
    v.Redraw()
    plain_v = View(0).load_scene(sc); plain_v.set_transforms(moved_xforms(7)); plain_v.set_visibility(visible_flags(7, [4]))
    move(plain_v, v._camera); plain_v.Redraw()
    plain = plain_v.read_ldr()                                                   # the bytes of a context that never heard of the feature
    assert same_bits(plain_v.save_accum()[0], v.save_accum()[0])
    plain_v.close()
    shown, s1 = assert_device_equals_twin(v, history_from(s0, s0["a"]), tab, **ref.DEFAULTS)
    d = v.get_display()
    display = (d["tonemap_mode"], d["exposure"], d["white_point"])
    got = v.read_ldr()
    assert not np.array_equal(got, plain)
    assert np.array_equal(got, ldr_of_a_context_handed(shown, 1, sc, display))   # the tone map of the twin's image
    v.read_ldr_begin()
    assert np.array_equal(v.read_ldr_end(), got)
    # the denoise filter reads the reprojected image, counts included
    v.SetDenoise()
    dn = dict(levels=4, normal_cos=abi.DENOISE_DEFAULTS["normal_cos"], depth_ratio=abi.DENOISE_DEFAULTS["depth_ratio"], until_samples=256)
    want = denoise_host(shown, s1["ob"], s1["tr"], s1["t"], tab, **dn)
    filtered = v.read_denoised()
    assert same_bits(filtered, want), where_differs(filtered, want)
    assert not same_bits(filtered, denoise_host(s1["a"], s1["ob"], s1["tr"], s1["t"], tab, **dn))
    assert np.array_equal(v.read_ldr(), ldr_of_a_context_handed(filtered, 1, sc, display))
    # auto exposure still meters the UNFILTERED accumulator: the second context takes its display values from crh_measure_exposure, which reads the accumulator
    v.set_auto_exposure(True)
    m = v.measure_exposure()
    metered = v.read_ldr()
    assert np.array_equal(metered, ldr_of_a_context_handed(filtered, 1, sc, (display[0], m["exposure"], m["white_point"])))
    v.ClearReproject(); v.ClearDenoise()
    m_off = v.measure_exposure()
    assert np.array_equal(m_off["hist"], m["hist"]) and m_off["exposure"] == m["exposure"] and m_off["white_point"] == m["white_point"]
    v.set_auto_exposure(False)
    assert np.array_equal(v.read_ldr(), plain)                                   # off again: the bytes of the parent
    v.close()


def drag(v, sc, reads):
    """three views of one sample each, INTEGRATION.md's sequence; reads(v, k) is called after every frame"""
    out = []
    for k in range(3):
        if k:
            move(v, turned(sc.camera, 0.7 * k))
        v.Redraw()
        out.append(reads(v, k))
    return out


@pytest.mark.gpu
def test_two_read_backs_in_flight_across_a_capture_each_equal_the_synchronous_bytes_of_their_moment(hip_lib):
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    a = View(0).load_scene(sc); a.SetReproject(); a.SetDenoise()
    sync = drag(a, sc, lambda v, k: v.read_ldr())
    a.close()
    b = View(0).load_scene(sc); b.SetReproject(); b.SetDenoise()
    got = []

    def reads(v, k):
        v.read_ldr_begin()                                                       # frames 1 and 2: in flight across the next camera change and its capture
        if k == 2:
            got.append(v.read_ldr_end()); got.append(v.read_ldr_end())
        elif k == 0:
            got.append(v.read_ldr_end())
    drag(b, sc, reads)
    assert len(got) == 3 and all(np.array_equal(x, y) for x, y in zip(got, sync))
    assert not np.array_equal(sync[1], sync[2])
    b.close()


@pytest.mark.gpu
def test_the_feature_leaves_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)

    def everything(v, k):
        acc, frames = v.save_accum()
        st = v.stats()
        ids = v.read_ids()
        return dict(hdr=v.read_hdr(), acc=acc, frames=frames, stats=[st[c] for c in counters], ids=ids, bounds=v.selection_bounds())

    def assert_same(x, y):
        assert same_bits(x["hdr"], y["hdr"]) and same_bits(x["acc"], y["acc"]) and x["frames"] == y["frames"] == 1 and x["stats"] == y["stats"]
        assert all(np.array_equal(bits(p) if p.dtype == f32 else p, bits(q) if q.dtype == f32 else q) for p, q in zip(x["ids"], y["ids"]))
        assert all(np.array_equal(p, q) for p, q in zip(x["bounds"], y["bounds"]))

    never = View(0).load_scene(sc); never.set_selection(flags, (255, 0, 0), 128)
    want = drag(never, sc, everything)
    want_ldr = never.read_ldr()
    never.close()
    never = View(0).load_scene(sc); never.set_selection(flags, (255, 0, 0), 128)
    drag_ldr = drag(never, sc, lambda v, k: v.read_ldr())                         # the parent's behaviour: the LDR bytes of a drag, feature never set
    never.close()
    v = View(0)
    v.SetReproject(max_history=8)                                                # set before the scene exists: display state outlives a new scene
    v.load_scene(sc); v.set_selection(flags, (255, 0, 0), 128)
    assert v.get_reproject()["on"] and v.get_reproject()["max_history"] == 8.0

    def with_read_outs(v, k):
        v.read_ldr(); v.read_reprojected(); v.read_ldr_begin(); v.read_ldr_end(); v.get_reproject()
        return everything(v, k)
    got = drag(v, sc, with_read_outs)
    assert v.get_reproject()["history_valid"]
    for x, y in zip(got, want):
        assert_same(x, y)
    assert not np.array_equal(v.read_ldr(), want_ldr)
    v.ClearReproject()
    assert np.array_equal(v.read_ldr(), want_ldr)                                # the selection still drawn, and the bytes of a context that never called crh_set_reproject
    move(v, sc.camera)                                                           # back to the first view, restarted: the state the other context started its drag from
    cleared = drag(v, sc, lambda v, k: v.read_ldr())
    assert all(np.array_equal(x, y) for x, y in zip(cleared, drag_ldr))          # ClearReproject == never set, through a whole drag
    v.close()


@pytest.mark.gpu
def test_set_reproject_refusals_state_and_bench(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    d = v.get_reproject()
    assert d["on"] is False and (float(d["max_history"]), d["until_samples"]) == (16.0, 64) and d["normal_cos"] == ref.DEFAULTS["normal_cos"] and d["depth_ratio"] == ref.DEFAULTS["depth_ratio"]
    for bad, why in BAD:
        with pytest.raises(BackendError, match=f"-> -1: crh_set_reproject: .*{why}"):
            v.set_reproject(True, **bad)
        assert v.get_reproject()["on"] is False                                  # a refused call changes nothing
    v.set_reproject(True, max_history=1024.0, until_samples=1 << 20, normal_cos=1.0, depth_ratio=1.0)      # the limits themselves; allowed before crh_build
    g = v.get_reproject()
    assert g["on"] and (float(g["max_history"]), g["until_samples"], float(g["normal_cos"]), float(g["depth_ratio"])) == (1024.0, 1 << 20, 1.0, 1.0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4.*crh_build has not been called"):
        v.read_reprojected()
    assert v._fn("read_reprojected")(v._ctx, None) == abi.E_INVALID
    v.load_scene(sc)
    v.Redraw()
    before = v.read_reprojected()
    b = v.bench_reproject(3)                                                     # without a history: the current view stands in, and nothing a read-out sees moves
    assert b["resolve_ms"] > 0.0 and b["capture_ms"] > 0.0
    assert same_bits(v.read_reprojected(), before) and v.get_reproject()["history_valid"] is False
    move(v, turned(sc.camera, 1.0)); v.Redraw()
    before = v.read_reprojected()
    b = v.bench_reproject(3)
    assert b["resolve_ms"] > 0.0 and same_bits(v.read_reprojected(), before) and v.get_reproject()["history_valid"] is True
    v.close()


@pytest.mark.gpu
def test_it_helps(hip_lib):
    """THE test of what the feature is for.  The closed room of test_it_denoises (the light out of view) at 96 x 64: eight drag steps of 0.25 degrees at 1 spp each;
    over the hit pixels (all of them: the room is closed) the mean squared error of the last DISPLAYED image (crh_read_reprojected) against 512 spp of that last view
    is below HALF the error of the raw 1-spp image -- the issue's condition: two effective samples already give it.  The measured ratio is printed
    (DESIGN.md 6.12 carries it)."""
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = closed_room(W, H)
    v = View(0).load_scene(sc)
    v.SetReproject()
    for k in range(9):                                                           # the first view, then eight steps
        if k:
            move(v, turned(sc.camera, 0.25 * k))
        v.Redraw()
        v.read_ldr()                                                             # a host that displays its frames
    assert v.get_reproject()["history_valid"] and v.save_accum()[1] == 1
    raw = v.read_hdr().astype(np.float64)
    shown = v.read_reprojected()
    hit = v.read_ids()[1] >= 0
    v.render(511)
    assert v.save_accum()[1] == 512
    truth = v.read_hdr().astype(np.float64)
    v.close()
    mse_raw = float(((raw - truth)[hit] ** 2).mean())
    mse_shown = float(((shown[..., :3].astype(np.float64) - truth)[hit] ** 2).mean())
    print(f"8 drag steps of 0.25 deg at 1 spp against 512 spp over {int(hit.sum())} hit pixels: mse raw {mse_raw:.6g}, reprojected {mse_shown:.6g}, "
          f"ratio {mse_shown / mse_raw:.4f}, mean effective samples {float(shown[..., 3][hit].mean()):.2f}")
    assert hit.all() and mse_raw > 0.0 and truth.max() < 25.0                    # closed, noisy, and no pixel shows the light itself
    assert mse_shown < 0.5 * mse_raw
