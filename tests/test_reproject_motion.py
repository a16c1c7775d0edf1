"""Per-object history deltas: the reprojected display history kept through an object drag (crh_reproject.cpp, k_reproject_resolve_motion in
cadrays_amd/csrc/reproject_kernels.hip).

The reference has no counterpart: OCCT's path tracer shows the raw accumulation.  Every comparison of two images is bit for bit, as uint32 views.  The only
inequalities: the geometric check of the delta table, whose bound is derived (below), and the last test's "eight reprojected drag steps are closer to the converged
image than the raw 1-spp frame", whose bar (half the error: two effective samples of equal variance already give it) is a condition, not a measurement.

  CPU   the structs' layout, the exports, the defaults through both mirrors; crh_reproject_delta_host == the numpy float64 restatement
        (tests/reproject_motion_reference.py, written from the header's text) and a geometric check that does not depend on the operation order;
        crh_reproject_motion_host == the restatement on two configurations of an analytic scene, every frame size, both camera models, the camera still and moved;
        the cases are not vacuous (asserted from the numpy side); an unflagged or absent table gives crh_reproject_host's image; each deliberately wrong rule
        changes the image; every refusal (make -C cadrays_amd/csrc sanitize-reproject runs both under ASan + UBSan in a stand-alone program: not from here)
  GPU   crh_read_reprojected == the host twin through a sequence of object steps; the recursion over five drag steps; the life cycle; the LDR read-outs; nothing
        else moves; and it helps
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import reproject_motion_reference as ref
from cadrays_amd import abi
from cadrays_amd.binding import BackendError
from test_denoise import closed_room, ldr_of_a_context_handed, scene_table
from test_reproject import history_from, planes_of, same_bits, turned, where_differs
from test_two_level import object_scene, rigid
from test_visibility import visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("crh_reproject_motion_defaults", "crh_set_reproject_motion", "crh_get_reproject_motion", "crh_get_reproject_launches", "crh_bench_reproject_motion", "crh_reproject_delta_host",
         "crh_reproject_motion_host")
bits = ref.bits
CAPS = dict(max_history_moved=f32(5.0), max_history_static=f32(3.0))      # both below max_history's default and below the history's largest counts: both bind


def _delta():
    """the host-only entry points through the Python mirror: a missing one FAILS here (ImportError), it does not skip"""
    from cadrays_amd.view import reproject_delta_host
    return reproject_delta_host


def _host():
    from cadrays_amd.view import reproject_motion_host
    return reproject_motion_host


def _plain_host():
    from cadrays_amd.view import reproject_host
    return reproject_host


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_motion_structs_layout_matches_header(tmp_path):
    got = []
    for struct, name in ((abi.crh_reproject_motion_params, "crh_reproject_motion_params"),):
        fields = [n for n, _ in struct._fields_]
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(' + name + '));' + "".join(
            f'printf("%zu ", offsetof({name}, {n}));' for n in fields) + 'printf("%zu %zu %zu", sizeof(crh_reproject_delta), offsetof(crh_reproject_delta, flag), ' \
            'offsetof(crh_reproject_delta, pad));return 0;}'
        (tmp_path / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
        out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
        assert out[:3] == [C.sizeof(struct)] + [getattr(struct, n).offset for n in fields], (name, out)
        got.append(out)
    assert got == [[8, 0, 4, 64, 48, 52]], got
    dt = np.dtype(abi.REPROJECT_DELTA_DTYPE)
    assert dt == ref.DELTA_DTYPE and dt.itemsize == 64 and dt.fields["flag"][1] == 48 and dt.fields["pad"][1] == 52
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS and (f"CRH_API int {name}(" in header or f"CRH_API void {name}(" in header), name
    section = header[header.index("per-object history deltas"):header.index("--- viewport read-out")]
    for text in ("DIVISION by det", "rounded ONCE to float32", "max_history_static", "NO fused multiply-add"):
        assert text in section, text


def test_motion_entry_points_are_exported_and_defaults_agree(hip_lib):
    from cadrays_amd.binding import reproject_motion_params
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    p = abi.crh_reproject_motion_params()
    hip_lib.crh_reproject_motion_defaults.restype = None
    hip_lib.crh_reproject_motion_defaults(C.byref(p)); hip_lib.crh_reproject_motion_defaults(None)
    d, q = abi.REPROJECT_MOTION_DEFAULTS, reproject_motion_params()
    assert (p.max_history_moved, p.max_history_static) == (d["max_history_moved"], d["max_history_static"]) == (q.max_history_moved, q.max_history_static)
    assert (p.max_history_moved, p.max_history_static) == (float(ref.MOTION_DEFAULTS["max_history_moved"]), float(ref.MOTION_DEFAULTS["max_history_static"]))
    assert p.max_history_moved == float(abi.REPROJECT_DEFAULTS["max_history"]) == 16.0      # the moved cap's default is max_history's
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    assert f"default {int(p.max_history_static)} " in header[header.index("float max_history_static;"):][:200]


# ------------------------------------------------------------------------------------------------ CPU 2: the delta table
def object_pairs():
    """(X_hist, X_cur) of the issue's objects, and the flag each must get"""
    I = ref.IDENTITY
    c, s = np.cos(np.deg2rad(33.0)), np.sin(np.deg2rad(33.0))
    pairs = [
        ("left alone", I, I, 0),
        ("left alone off the identity", rigid(25.0, (0, 0, 1), (-0.25, 0.05, 0.02)), rigid(25.0, (0, 0, 1), (-0.25, 0.05, 0.02)), 0),
        ("translated", I, rigid(0.0, (0, 0, 1), (0.125, -0.3, 7.5)), 1),
        ("rotated, non-uniform scale", rigid(10.0, (1, 2, 3), (0.1, 0.2, 0.3)), ref.xform([[1.7 * c, -0.6 * s, 0.0, 0.4], [1.7 * s, 0.6 * c, 0.0, -2.0], [0.0, 0.0, 2.5, 0.3]]), 1),
        ("mirrored", rigid(5.0, (0, 1, 0), (1, 2, 3)), ref.xform([[-1, 0, 0, 0.7], [0, 1, 0, 0.1], [0, 0, 1, -0.2]]), 1),
        ("sheared", I, ref.xform([[1, 0.7, -0.3, 0.2], [0, 1, 0.45, 0.0], [0.1, 0, 1, -1.5]]), 1),
        ("x 1000", rigid(40.0, (1, 1, 0), (50.0, -20.0, 30.0), 1000.0), rigid(41.0, (1, 1, 0), (51.0, -20.5, 30.0), 1000.0), 1),
        ("singular X_cur", I, ref.xform([[1, 2, 3, 0], [2, 4, 6, 1], [0, 0, 1, 2]]), 2),
        ("all-zero X_cur", I, np.zeros(12, f32), 2),
        ("D overflows float32", rigid(0.0, (0, 0, 1), (0, 0, 0), 1e30), rigid(0.0, (0, 0, 1), (0, 0, 0), 1e-30), 2),
        ("translation of D overflows", ref.xform([[1e20, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]), ref.xform([[1, 0, 0, 3e30], [0, 1, 0, 0], [0, 0, 1, 0]]), 2),
    ]
    return pairs


def test_delta_table_equals_the_float64_restatement_bit_for_bit(hip_lib):
    pairs = object_pairs()
    xh, xc = np.stack([p[1] for p in pairs]).astype(f32), np.stack([p[2] for p in pairs]).astype(f32)
    got, want = _delta()(xh, xc), ref.delta_table(xh, xc)
    assert got.dtype == ref.DELTA_DTYPE and got.tobytes() == want.tobytes(), [(p[0], g, w) for p, g, w in zip(pairs, got, want) if g.tobytes() != w.tobytes()]
    assert got["flag"].tolist() == [p[3] for p in pairs], list(zip([p[0] for p in pairs], got["flag"]))
    assert not got["D"][got["flag"] != 1].any() and not got["pad"].any()
    assert np.isfinite(got["D"]).all() and (np.abs(got["D"][got["flag"] == 1]).max(1) > 0).all()
    # random transforms, some of them far from well conditioned
    r = np.random.default_rng(11)
    xh = r.normal(0, 1, (200, 12)).astype(f32) * (10.0 ** r.integers(-3, 4, (200, 1))).astype(f32)
    xc = r.normal(0, 1, (200, 12)).astype(f32) * (10.0 ** r.integers(-3, 4, (200, 1))).astype(f32)
    xc[::17] = xh[::17]
    got, want = _delta()(xh, xc), ref.delta_table(xh, xc)
    assert got.tobytes() == want.tobytes() and (got["flag"][::17] == 0).all() and (got["flag"] == 1).sum() > 150
    # each deliberately wrong table differs
    for wrong in ref.WRONG_TABLE:
        assert ref.delta_table(xh, xc, wrong=wrong).tobytes() != got.tobytes(), wrong
    assert len(_delta()(np.zeros((0, 12), f32), np.zeros((0, 12), f32))) == 0


def test_delta_table_carries_points_from_the_current_placement_to_the_history_placement(hip_lib):
    """independent of the operation order.  In exact arithmetic D (X_cur p) = X_hist p.  The table rounds each of the twelve entries once to float32 (relative error
    <= 2^-24 each; the float64 work in front of it is 2^-29 times smaller), so row i of D x + D_i3, evaluated in float64 on x = X_cur p, is off by at most
    2^-24 (sum_j |D_ij| |x_j| + |D_i3|); the factor 64 leaves room for the conditioning of the inverse (the pairs' condition numbers are below 1e4: 1e4 * 2^-53 is
    far inside).  Derived, not tuned."""
    pairs = [p for p in object_pairs() if p[3] == 1]
    xh, xc = np.stack([p[1] for p in pairs]).astype(f32), np.stack([p[2] for p in pairs]).astype(f32)
    tab = _delta()(xh, xc)
    r = np.random.default_rng(3)
    for k, (name, _, _, _) in enumerate(pairs):
        D = tab["D"][k].astype(np.float64).reshape(3, 4)
        A, M = xh[k].astype(np.float64).reshape(3, 4), xc[k].astype(np.float64).reshape(3, 4)
        p = r.uniform(-2.0, 2.0, (500, 3))
        x = p @ M[:, :3].T + M[:, 3]
        want = p @ A[:, :3].T + A[:, 3]
        got = x @ D[:, :3].T + D[:, 3]
        bound = 64.0 * 2.0 ** -24 * (np.abs(x) @ np.abs(D[:, :3]).T + np.abs(D[:, 3]))
        worst = float((np.abs(got - want) / bound).max())
        print(f"{name}: worst |D X_cur p - X_hist p| / bound = {worst:.4f}")
        assert (np.abs(got - want) <= bound).all(), (name, worst)


# ------------------------------------------------------------------------------------------------ CPU 3: the host twin against numpy
def table_of(case, wrong=None):
    return ref.delta_table(case["xf_hist"], case["xf_cur"], wrong=wrong)


def twin_of(case, delta, motion=CAPS, **params):
    return _host()(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], delta, motion=motion, **params)


def numpy_of(case, delta, wrong=None, stats=None, motion=CAPS, **params):
    p = dict(ref.DEFAULTS); p.update(params); p.update(motion)
    return ref.reproject_motion(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], delta, wrong=wrong, stats=stats, **p)


OTHER_PARAMS = (dict(max_history=1.0, until_samples=1, normal_cos=1.0, depth_ratio=1.0), dict(max_history=1024.0, until_samples=1 << 20, normal_cos=1e-6, depth_ratio=1e30),
                dict(max_history=4.5, until_samples=3, normal_cos=0.5, depth_ratio=1.2))
OTHER_CAPS = (dict(max_history_moved=f32(1.0), max_history_static=f32(1024.0)), dict(max_history_moved=f32(1024.0), max_history_static=f32(1.0)),
              dict(max_history_moved=f32(2.5), max_history_static=f32(16.0)))


@pytest.mark.parametrize("camera_moved", [False, True], ids=["camera_still", "camera_moved"])
@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
@pytest.mark.parametrize("config", sorted(ref.CONFIGS))
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_twin_equals_the_numpy_restatement(hip_lib, size, config, ortho, camera_moved):
    case = ref.case(*size, config, ortho, camera_moved)
    delta = _delta()(case["xf_hist"], case["xf_cur"])
    assert delta.tobytes() == table_of(case).tobytes() and delta["flag"].tolist() == [0, 1]
    stats = {}
    got, want = twin_of(case, delta, **ref.DEFAULTS), numpy_of(case, delta, stats=stats, **ref.DEFAULTS)
    assert got.dtype == f32 and same_bits(got, want), (size, config, ortho, camera_moved, where_differs(got, want))
    if size == (61, 37):                                                         # not vacuous, from the numpy side
        print({k: v for k, v in stats.items() if not isinstance(v, np.ndarray)})
        assert 2 * stats["took_moved"] >= stats["flagged_hit"] > 20, stats["took_moved"]      # pixels on the moved object gather history
        assert stats["static_refused_all"] >= 1                                  # disoccluded static pixels: every usable tap shows another object, they pass through
        assert stats["cap_bound_moved"] >= 1 and stats["cap_bound_static"] >= 1  # both caps bind somewhere
        assert not same_bits(got, case["a"])
        plain = _plain_host()(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], **ref.DEFAULTS)
        assert not same_bits(got, plain)
    for p, m in zip(OTHER_PARAMS, OTHER_CAPS):
        got, want = twin_of(case, delta, motion=m, **p), numpy_of(case, delta, motion=m, **p)
        assert same_bits(got, want), (size, config, ortho, p, m, where_differs(got, want))
    # a table that covers object 0 only: object 1 lies outside it and runs the plain arithmetic, but the cap does not apply (nothing is flagged)
    got, want = twin_of(case, delta[:1], **ref.DEFAULTS), numpy_of(case, delta[:1], **ref.DEFAULTS)
    assert same_bits(got, want), where_differs(got, want)
    # a flag-2 record: the object's pixels pass through, the cap applies to the others
    none = delta.copy(); none["flag"][1] = 2; none["D"][1] = 0
    stats = {}
    got, want = twin_of(case, none, **ref.DEFAULTS), numpy_of(case, none, stats=stats, **ref.DEFAULTS)
    assert same_bits(got, want) and np.array_equal(bits(got)[case["ob"] == 1], bits(case["a"])[case["ob"] == 1])
    assert same_bits(twin_of(dict(case, hist=None), delta, **ref.DEFAULTS), case["a"])


MAIN = {}


def main():
    """the main case (the turned and scaled quad under a moved perspective camera at 61 x 37): computed once, shared, never changed"""
    if not MAIN:
        case = ref.case(61, 37, "turn_scale", False, True)
        delta = table_of(case)
        want = numpy_of(case, delta, **ref.DEFAULTS)
        for a in [case["a"], case["rays"], case["ob"], case["tr"], case["t"], want, delta] + [case["hist"][k] for k in ("rgba", "ob", "tr", "t")]:
            a.setflags(write=False)
        MAIN.update(case=case, delta=delta, want=want)
    return MAIN["case"], MAIN["delta"], MAIN["want"]


def test_unflagged_and_absent_tables_give_the_plain_image(hip_lib):
    case, delta, want = main()
    plain = _plain_host()(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], **ref.DEFAULTS)
    assert same_bits(plain, base_numpy(case))
    zero = np.zeros(2, ref.DELTA_DTYPE)
    assert same_bits(twin_of(case, zero, **ref.DEFAULTS), plain)                 # all flags 0: no transform and NO cap, whatever the caps are
    assert same_bits(twin_of(case, zero, motion=dict(max_history_moved=f32(1.0), max_history_static=f32(1.0)), **ref.DEFAULTS), plain)
    assert same_bits(twin_of(case, None, **ref.DEFAULTS), plain)                 # NULL table
    assert same_bits(numpy_of(case, zero, **ref.DEFAULTS), plain) and same_bits(numpy_of(case, None, **ref.DEFAULTS), plain)
    assert not same_bits(want, plain)


def base_numpy(case):
    return ref.base.reproject(case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], **ref.DEFAULTS)


@pytest.mark.parametrize("wrong", ref.WRONG_TABLE + ref.WRONG_RULE)
def test_each_wrong_motion_rule_breaks_bit_equality(hip_lib, wrong):
    """the main case tells the rule from its near misses: were the library to implement one of them, the tests above would fail"""
    case, delta, want = main()
    got = twin_of(case, delta, **ref.DEFAULTS)
    assert same_bits(got, want)
    if wrong in ref.WRONG_TABLE:
        broken = numpy_of(case, table_of(case, wrong=wrong), **ref.DEFAULTS)
    elif wrong == "cap_when_unflagged":                                          # told apart where nothing is flagged: the library must NOT cap there
        zero = np.zeros(2, ref.DELTA_DTYPE)
        got, broken = twin_of(case, zero, **ref.DEFAULTS), numpy_of(case, zero, wrong=wrong, **ref.DEFAULTS)
    else:
        broken = numpy_of(case, delta, wrong=wrong, **ref.DEFAULTS)
    share = ref.share_differing(broken, got)
    print(f"wrong rule '{wrong}': {100.0 * share:.1f} % of the pixels differ")
    assert share > 0.0, wrong


# ------------------------------------------------------------------------------------------------ CPU 4: refusals
BAD_CAPS = ((dict(max_history_moved=0.5), "max_history_moved lies outside"), (dict(max_history_moved=1024.5), "max_history_moved lies outside"),
            (dict(max_history_static=0.999), "max_history_static lies outside"), (dict(max_history_static=-3.0), "max_history_static lies outside"),
            (dict(max_history_static=2000.0), "max_history_static lies outside"),
            (dict(max_history_moved=float("nan")), "hold a NaN / Inf"), (dict(max_history_static=float("inf")), "hold a NaN / Inf"),
            (dict(max_history_moved=float("-inf")), "hold a NaN / Inf"))


def test_refusals_of_the_motion_host_entry_points(hip_lib):
    host = _host()
    case = ref.case(5, 4, "slide")
    delta = table_of(case)
    args = (case["a"], case["rays"], case["ob"], case["tr"], case["t"], case["hist"], case["table"], delta)
    host(*args, motion=dict(max_history_moved=1.0, max_history_static=1024.0)); host(*args, motion=dict(max_history_moved=1024.0, max_history_static=1.0))
    for bad, _ in BAD_CAPS:
        with pytest.raises(BackendError):
            host(*args, motion=bad)
    with pytest.raises(BackendError):
        host(*args, max_history=0.5)                                             # the refusals of crh_reproject_host
    with pytest.raises(BackendError):
        host(*args, until_samples=0)
    three = delta.copy(); three["flag"][1] = 3
    with pytest.raises(BackendError):
        host(*args[:-1], three)                                                  # a flag above 2
    # NULL pointers and empty frames, straight at the library
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    a, rays, ob, t, tab, h = case["a"], case["rays"], case["ob"], case["t"], case["table"], case["hist"]
    out = np.zeros_like(a)
    F = abi.crh_reproject_frame(); F.aspect = 1.25; F.tan_half = 0.4; F.fwd[1] = 1.0; F.right[0] = 1.0; F.up[2] = 1.0
    pa, pr, po, pt, pout, ptab = a.ctypes.data_as(fp), rays.ctypes.data_as(fp), ob.ctypes.data_as(i32p), t.ctypes.data_as(fp), out.ctypes.data_as(fp), tab.ctypes.data_as(C.c_void_p)
    ph, pd = h["rgba"].ctypes.data_as(fp), delta.ctypes.data_as(C.c_void_p)
    W, H, nT, nO, zero = C.c_uint32(5), C.c_uint32(4), C.c_uint32(len(tab)), C.c_uint32(2), C.c_uint32(0)
    p = abi.crh_reproject_params(); hip_lib.crh_reproject_defaults.restype = None; hip_lib.crh_reproject_defaults(C.byref(p))
    mp = abi.crh_reproject_motion_params(); hip_lib.crh_reproject_motion_defaults.restype = None; hip_lib.crh_reproject_motion_defaults(C.byref(mp))
    fn = hip_lib.crh_reproject_motion_host
    ok = lambda **kw: fn(*[kw.get(k, v) for k, v in (("a", pa), ("r", pr), ("o", po), ("tr", po), ("t", pt), ("h", ph), ("ho", po), ("htr", po), ("ht", pt), ("F", C.byref(F)),
                                                      ("tab", ptab), ("nT", nT), ("W", W), ("H", H), ("p", C.byref(p)), ("d", pd), ("nO", nO), ("mp", C.byref(mp)), ("out", pout))])
    assert ok() == abi.OK and ok(tab=None, nT=zero) == abi.OK
    assert ok(h=None, ho=None, htr=None, ht=None, F=None) == abi.OK              # no history: none of its planes is needed
    assert ok(d=None, nO=zero, mp=None) == abi.OK                                # no table: the motion parameters are not read
    for k in ("a", "r", "o", "tr", "t", "ho", "htr", "ht", "F", "p", "out", "mp"):
        assert ok(**{k: None}) == abi.E_INVALID, k
    assert ok(W=zero) == abi.E_INVALID and ok(H=zero) == abi.E_INVALID and ok(tab=None) == abi.E_INVALID
    assert ok(d=None) == abi.E_INVALID                                           # a count without a table
    # the delta table's own entry point
    xh = np.tile(ref.IDENTITY, (2, 1)); xp = xh.ctypes.data_as(fp)
    dh = hip_lib.crh_reproject_delta_host
    assert dh(xp, xp, nO, pd) == abi.OK and dh(None, None, zero, None) == abi.OK
    assert dh(None, xp, nO, pd) == abi.E_INVALID and dh(xp, None, nO, pd) == abi.E_INVALID and dh(xp, xp, nO, None) == abi.E_INVALID
    nan = np.full((1, 12), np.nan, f32)
    assert _delta()(nan, nan)["flag"].tolist() == [0] and _delta()(xh[:1], nan)["flag"].tolist() == [2] and _delta()(nan, xh[:1])["flag"].tolist() == [2]
    assert hip_lib.crh_set_reproject_motion(None, C.byref(mp)) == abi.E_INVALID and hip_lib.crh_get_reproject_motion(None, None, None, None) == abi.E_INVALID
    assert hip_lib.crh_bench_reproject_motion(None, C.c_uint32(1), None) == abi.E_INVALID and hip_lib.crh_get_reproject_launches(None, None, None) == abi.E_INVALID


# ================================================================================================ GPU
N_OBJ = 7
P_SHORT = dict(max_history=4.0, until_samples=3, normal_cos=ref.DEFAULTS["normal_cos"], depth_ratio=ref.DEFAULTS["depth_ratio"])
M_SHORT = dict(max_history_moved=f32(3.0), max_history_static=f32(2.0))


def identity_xforms():
    return np.tile(rigid(), (N_OBJ, 1))


def room(W, H, **cam):
    """the seven-object Cornell room, every object at its build-time placement: (view, scene, table)"""
    from cadrays_amd.view import View
    sc = object_scene(None, W, H)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, **cam))
    return View(0).load_scene(sc), sc, scene_table(sc.pos, sc.tri)


def twin_of_view(v, hist, tab, xf_hist, xf_cur, motion, **params):
    s = planes_of(v)
    delta = None if xf_hist is None else _delta()(xf_hist, xf_cur)
    return _host()(s["a"], s["rays"], s["ob"], s["tr"], s["t"], hist, tab, delta, motion=motion, **params), s, delta


def assert_device_equals_twin(v, hist, tab, xf_hist, xf_cur, motion, **params):
    got = v.read_reprojected()
    want, s, delta = twin_of_view(v, hist, tab, xf_hist, xf_cur, motion, **params)
    assert got.shape == want.shape and same_bits(got, want), where_differs(got, want)
    n_flagged = 0 if delta is None or hist is None else int((delta["flag"] != 0).sum())
    assert v.get_reproject_motion()["n_flagged"] == n_flagged
    return got, s


CAMS = pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])


@pytest.mark.gpu
@CAMS
@pytest.mark.parametrize("size", [(67, 45), (1, 1), (5, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_twin_through_object_steps(hip_lib, size, ortho):
    W, H = size
    kind = dict(is_ortho=True, ortho_scale=0.55) if ortho else {}
    v, sc, tab = room(W, H, **kind)
    g = v.get_reproject_motion()
    assert g["on"] is False and g["n_flagged"] == 0 and (float(g["max_history_moved"]), float(g["max_history_static"])) == (16.0, float(ref.MOTION_DEFAULTS["max_history_static"]))
    v.set_reproject(True, **P_SHORT)
    v.set_reproject_motion(True, **M_SHORT)
    assert v.get_reproject_motion()["on"] is True
    big = W >= 64                                                                # (a frame five pixels wide sees a strip of the back wall)
    xf = identity_xforms()
    v.Redraw(); v.Redraw()
    shown, s = assert_device_equals_twin(v, None, tab, None, None, M_SHORT, **P_SHORT)      # no history yet: the accumulator, bitwise
    assert same_bits(shown, s["a"]) and v.get_reproject()["history_valid"] is False

    def step(new_xf, camera=None, check_spp=(1,)):
        """one manipulator step: the capture inside set_transforms, then frames of one sample each; the twin is fed what the ending view displayed"""
        nonlocal shown, s, xf
        hist, xf_hist = history_from(s, shown), xf.copy()
        if camera is not None:
            v.set_camera(camera)                                                 # captures; set_transforms then finds a capture made and keeps it
        v.set_transforms(new_xf)
        assert v.get_reproject()["history_valid"] is True
        xf = np.array(new_xf, f32)
        for spp in range(1, max(check_spp) + 1):
            v.Redraw()
            if spp in check_spp:
                shown, s = assert_device_equals_twin(v, hist, tab, xf_hist, xf, M_SHORT, **P_SHORT)
                assert s["frames"] == spp
        return hist, xf_hist

    # one object translated; a.w at until_samples - 2, until_samples - 1 and until_samples
    one = xf.copy(); one[3] = rigid(0.0, (0, 0, 1), (0.03, 0.0, 0.01))
    step(one, check_spp=(1, 2, 3))
    assert same_bits(shown, s["a"])                                              # a.w >= until_samples: the accumulator, bitwise
    # one rotated and scaled (the first keeps its placement: X_hist has advanced, its flag is 0 again)
    two = xf.copy(); two[5] = rigid(20.0, (0, 0, 1), (0.05, 0.02, 0.03), 0.9)
    step(two, check_spp=(1, 2))
    assert v.get_reproject_motion()["n_flagged"] == 1
    if big:
        moved_px = (s["ob"] == 5) & (s["tr"] >= 0)
        assert moved_px.sum() > 20 and (shown[..., 3][moved_px] > 2.0).mean() > 0.25     # the moved object's pixels gathered history
        assert not same_bits(shown, s["a"])
    # two objects moved at once
    three = xf.copy(); three[3] = rigid(15.0, (0, 0, 1), (-0.05, 0.03, 0.0)); three[6] = rigid(0.0, (0, 0, 1), (0.02, -0.04, 0.05))
    step(three)
    assert v.get_reproject_motion()["n_flagged"] == 2
    # one put back to its build-time placement: a step like any other (flag 1 until the next capture) ...
    four = xf.copy(); four[5] = rigid()
    step(four)
    # ... and a move taken back before a frame was rendered: no capture (frames_done == 0), X_cur == X_hist again, no record flagged, the plain kernel
    hist, xf_hist = history_from(s, shown), xf.copy()
    away = xf.copy(); away[6] = rigid(0.0, (0, 0, 1), (0.2, 0.0, 0.0))
    v.set_transforms(away)
    assert v.get_reproject_motion()["n_flagged"] == 1
    v.set_transforms(xf)
    assert v.get_reproject_motion()["n_flagged"] == 0 and v.get_reproject()["history_valid"] is True
    v.Redraw()
    before = v.get_reproject_launches()
    assert before["motion"] >= 4 and before["plain"] >= 1                        # the steps above ran the motion kernel; the first capture, without a table, the plain one
    shown, s = assert_device_equals_twin(v, hist, tab, xf_hist, xf, M_SHORT, **P_SHORT)
    v.read_ldr(); v.read_ldr_begin(); v.read_ldr_end()
    after = v.get_reproject_launches()
    assert after["motion"] == before["motion"] and after["plain"] == before["plain"] + 3      # no flagged record: the new kernel is NEVER launched
    plain = _plain_host()(s["a"], s["rays"], s["ob"], s["tr"], s["t"], hist, tab, **P_SHORT)
    assert same_bits(shown, plain)                                               # nothing flagged: no cap, the plain rule's bytes
    # the camera and an object changed before one restart
    cam_step = (1.5, (0.04, 0.0, 0.01)) if W >= 64 else (0.05, (0.001, 0.0, 0.01))
    five = xf.copy(); five[3] = rigid(15.0, (0, 0, 1), (-0.02, 0.05, 0.01))
    hist, xf_hist = step(five, camera=turned(sc.camera, *cam_step, **kind))
    assert v.get_reproject_motion()["n_flagged"] == 1
    flagged_now = v.get_reproject_launches()
    assert flagged_now["motion"] == after["motion"] + 1 and flagged_now["plain"] == after["plain"] + 1      # the read-out just made; the camera's capture found nothing flagged
    if big:
        assert not same_bits(shown, s["a"])
        assert not same_bits(shown, _plain_host()(s["a"], s["rays"], s["ob"], s["tr"], s["t"], hist, tab, **P_SHORT))
    # the caps in force are the ones a read-out uses; changing them keeps the history
    m2 = dict(max_history_moved=f32(1.5), max_history_static=f32(1.0))
    v.set_reproject_motion(True, **m2)
    assert v.get_reproject()["history_valid"] is True
    assert_device_equals_twin(v, hist, tab, xf_hist, xf, m2, **P_SHORT)
    v.close()


@pytest.mark.gpu
def test_recursion_over_five_drag_steps(hip_lib):
    """what is captured is the RESOLVED image: after every step the device image equals the twin applied to the twin's own previous output, X_hist advancing at
    every capture"""
    W, H = 67, 45
    v, sc, tab = room(W, H)
    P = dict(ref.DEFAULTS, max_history=f32(6.0))
    M = dict(max_history_moved=f32(3.0), max_history_static=f32(4.0))
    v.set_reproject(True, **P); v.set_reproject_motion(True, **M)
    xf = identity_xforms()
    v.Redraw()
    shown, s, _ = twin_of_view(v, None, tab, None, None, M, **P)
    moved_counts, static_counts = [], []
    for k in range(1, 6):
        hist, xf_hist = history_from(s, shown), xf.copy()
        xf = xf.copy(); xf[3] = rigid(4.0 * k, (0, 0, 1), (0.01 * k, 0.004 * k, 0.0))
        v.set_transforms(xf)
        v.Redraw()
        got = v.read_reprojected()
        shown, s, delta = twin_of_view(v, hist, tab, xf_hist, xf, M, **P)        # the twin's own previous output is its history
        assert delta["flag"].tolist() == [0, 0, 0, 1, 0, 0, 0]
        assert same_bits(got, shown), (k, where_differs(got, shown))
        moved_counts.append(float(shown[..., 3][s["ob"] == 3].max())); static_counts.append(float(shown[..., 3][(s["ob"] != 3) & (s["tr"] >= 0)].max()))
    assert moved_counts == [2.0, 3.0, 4.0, 4.0, 4.0], moved_counts               # 1 + min(history, max_history_moved)
    assert static_counts == [2.0, 3.0, 4.0, 5.0, 5.0], static_counts             # 1 + min(history, max_history_static)
    v.close()


@pytest.mark.gpu
def test_life_cycle_with_object_steps(hip_lib):
    W, H = 67, 45
    v, sc, tab = room(W, H)
    valid = lambda: v.get_reproject()["history_valid"]
    flagged = lambda: v.get_reproject_motion()["n_flagged"]
    n = iter(range(1, 100))

    def xforms():
        """the next placement of the drag: object 3 a little further along x"""
        xf = identity_xforms(); xf[3] = rigid(0.0, (0, 0, 1), (0.004 * next(n), 0.0, 0.0))
        return xf
    cams = iter(turned(sc.camera, 0.3 * k) for k in range(1, 40))

    def capture():
        v.Redraw(); v.set_transforms(xforms())
        assert valid() is True

    # motion off: a transform change drops the history as the parent drops it
    v.set_reproject(True)
    v.Redraw(); v.set_camera(next(cams)); v.reset()
    assert valid() is True
    v.Redraw(); v.set_transforms(xforms())
    assert valid() is False
    # motion on, reprojection off: nothing is captured
    v.set_reproject(False); v.set_reproject_motion(True)
    v.Redraw(); v.set_transforms(xforms())
    assert valid() is False and flagged() == 0
    v.set_reproject(True)
    v.set_transforms(xforms())
    assert valid() is False                                                      # frames_done == 0 and no history: nothing to capture, nothing to keep
    capture()                                                                    # both on: set_transforms captures and keeps
    assert flagged() == 1
    v.set_transforms(xforms())
    assert valid() is True and flagged() == 1                                    # frames_done == 0: kept without a capture, the table follows the transforms in force
    v.Redraw(); v.set_transforms(xforms()); v.set_transforms(xforms())
    assert valid() is True
    same = xforms()
    v.Redraw(); v.set_transforms(same); v.Redraw(); v.set_transforms(same)
    assert valid() is True and flagged() == 1                                    # unchanged transforms: no capture, kept as it is (X_hist is the placement before `same`)
    # a camera capture takes the transforms in force
    capture(); v.Redraw(); v.set_camera(next(cams)); v.reset()
    assert valid() is True and flagged() == 0
    # everything else that drops the history still drops it
    capture(); v.set_visibility(visible_flags(N_OBJ, [4]))
    assert valid() is False
    v.set_visibility(visible_flags(N_OBJ, []))
    capture(); v.set_materials(sc.materials)
    assert valid() is False
    capture(); v.set_lights(sc.lights)
    assert valid() is False
    capture(); v.set_spec()
    assert valid() is False
    capture(); v.set_params(dataclasses.replace(sc.params, width=40, height=30))
    assert valid() is False
    v.set_params(sc.params)
    capture(); v.Redraw(); v.reset()
    assert valid() is False                                                      # a crh_reset without a capture in front of it
    capture(); acc, frames = v.save_accum(); v.load_accum(acc, frames)
    assert valid() is False
    capture(); v.set_reproject(False)
    assert valid() is False and v.get_reproject_motion()["on"] is True
    v.set_reproject(True)
    # crh_set_reproject_motion(NULL): drops the history only when a record is flagged
    capture()
    assert flagged() == 1
    v.set_reproject_motion(False)
    assert valid() is False and v.get_reproject_motion()["on"] is False
    v.set_reproject_motion(True)
    capture(); v.Redraw(); v.set_camera(next(cams)); v.reset()
    assert valid() is True and flagged() == 0
    v.set_reproject_motion(False)
    assert valid() is True                                                       # nothing flagged: the history fits the plain rule and stays
    # switched on while a history is valid: the transforms in force are X_hist, and the next step is reprojected from them
    v.set_reproject_motion(True)
    assert valid() is True and flagged() == 0
    capture()
    assert flagged() == 1
    # raygen_bilinear != 0: never a capture, and with frames rendered nothing valid to keep
    v.set_spec(raygen_bilinear=1)
    v.Redraw(); v.set_transforms(xforms())
    assert valid() is False
    v.set_spec()
    capture()
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(67, 45), (5, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_lds_staged_form_gives_the_same_bytes(hip_lib, monkeypatch, size):
    """CRH_REPROJECT_STAGED=1 (read when the context is created): the motion kernel's other form, the flag-1 records in LDS -- one, two and seven of them, a flag-2
    record beside them, read-outs on both streams and the captures in between: the twin's bytes"""
    hip_lib.crh_env_table.restype = C.c_char_p
    assert b"CRH_REPROJECT_STAGED\t" in hip_lib.crh_env_table()
    monkeypatch.setenv("CRH_REPROJECT_STAGED", "1")
    W, H = size
    v, sc, tab = room(W, H)
    v.set_reproject(True, **P_SHORT); v.set_reproject_motion(True, **M_SHORT)
    xf = identity_xforms()
    v.Redraw()
    s = planes_of(v); shown = v.read_reprojected()
    steps = []
    one = xf.copy(); one[3] = rigid(0.0, (0, 0, 1), (0.03, 0.0, 0.01)); steps.append(one)
    two = one.copy(); two[3] = rigid(12.0, (0, 0, 1), (0.04, 0.01, 0.01)); two[5] = rigid(0.0, (0, 0, 1), (0.02, 0.0, 0.03), 0.9); steps.append(two)
    flat = two.copy(); flat[6] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0.3], f32); steps.append(flat)      # a singular placement: flag 2, no slot
    every = np.stack([rigid(1.0 + k, (0, 0, 1), (0.01 * k, 0.005, 0.002 * k)) for k in range(N_OBJ)]); steps.append(every)
    for k, new in enumerate(steps):
        hist, xf_hist = history_from(s, shown), xf.copy()
        v.set_transforms(new); v.Redraw()
        xf = new
        shown, s = assert_device_equals_twin(v, hist, tab, xf_hist, xf, M_SHORT, **P_SHORT)
        if k == 1:
            ldr = v.read_ldr(); v.read_ldr_begin()
            assert np.array_equal(v.read_ldr_end(), ldr)
    assert v.get_reproject_motion()["n_flagged"] == N_OBJ and v.get_reproject_launches()["motion"] >= 8
    v.close()


def extra_object():
    """two quads in front of the back wall, as test_denoise.live_scene adds them: (pos, nrm, tri)"""
    p = np.array([(0.35, 0.25, 0.35), (0.5, 0.1, 0.35), (0.5, 0.1, 0.65), (0.35, 0.25, 0.65), (0.65, 0.25, 0.35), (0.65, 0.25, 0.65)], f32)
    n = np.tile(np.array([0, -1, 0], f32), (len(p), 1))
    t = np.array([(0, 1, 2, 0), (0, 2, 3, 0), (1, 4, 5, 0), (1, 5, 2, 0)], np.int32)
    return p, n, t


def five_object_room(W, H):
    """the Cornell room WITHOUT the spheres, every material an object: five of them"""
    from cadrays_amd import scenes
    sc = scenes.cornell_box(False, W, H)
    tri_obj = sc.tri[:, 3].astype(np.int32)
    return dataclasses.replace(sc, tri_object=tri_obj, obj_xform=np.tile(rigid(), (int(tri_obj.max()) + 1, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("setter", ["add_object", "geometry_and_build", "environment", "texture"])
def test_scene_setters_drop_a_flagged_history_and_the_next_step_captures_again(hip_lib, setter):
    """the setters that may change the object count, and the two shading setters the life-cycle test does not reach, each met with a FLAGGED table in force (the
    context's X_hist, its table and the device table are sized by the old count): the history is dropped, nothing stays flagged, and the next frame +
    crh_set_transforms captures again and equals the twin over the new object count"""
    W, H = 67, 45
    v, sc, tab = room(W, H)
    v.set_reproject(True, **P_SHORT); v.set_reproject_motion(True, **M_SHORT)
    xf = identity_xforms()
    v.Redraw()
    s = planes_of(v); shown = v.read_reprojected()
    xf1 = xf.copy(); xf1[3] = rigid(0.0, (0, 0, 1), (0.03, 0.0, 0.01)); xf1[6] = rigid(10.0, (0, 0, 1), (0.0, 0.02, 0.03))
    v.set_transforms(xf1); v.Redraw()
    assert_device_equals_twin(v, history_from(s, shown), tab, xf, xf1, M_SHORT, **P_SHORT)
    assert v.get_reproject()["history_valid"] is True and v.get_reproject_motion()["n_flagged"] == 2
    if setter == "add_object":
        p, n, t = extra_object()
        assert v.add_object(p, n, t, rigid(0.0, (0, 0, 1), (0.0, 0.05, 0.0))) == N_OBJ
        tab = scene_table(np.concatenate([sc.pos, p]), np.concatenate([sc.tri, t + np.array([len(sc.pos)] * 3 + [0], np.int32)]))
        xf = np.concatenate([xf1, rigid(0.0, (0, 0, 1), (0.0, 0.05, 0.0))[None]])
        moved = N_OBJ                                                            # the new object itself is dragged next
    elif setter == "geometry_and_build":
        sc = five_object_room(W, H)
        v.load_scene(sc)                                                         # crh_set_geometry ... crh_build: five objects where seven were
        tab = scene_table(sc.pos, sc.tri)
        xf = np.tile(rigid(), (5, 1))
        moved = 4
    else:
        if setter == "environment":
            v.set_envmap(np.full((4, 8, 3), 0.25, f32))
        else:
            v.set_texture(0, np.full((2, 2, 3), 0.5, f32))
        xf, moved = xf1, 3
    assert v.get_reproject()["history_valid"] is False and v.get_reproject_motion()["n_flagged"] == 0
    v.Redraw()
    shown, s = assert_device_equals_twin(v, None, tab, None, None, M_SHORT, **P_SHORT)      # no history: the accumulator, bitwise
    assert same_bits(shown, s["a"])
    xf2 = xf.copy(); xf2[moved] = rigid(5.0, (0, 0, 1), (0.02, 0.03, 0.01)); xf2[0] = rigid(0.0, (0, 0, 1), (0.0, 0.0, 0.004))
    v.set_transforms(xf2)                                                        # captures again, over the new object count
    assert v.get_reproject()["history_valid"] is True and v.get_reproject_motion()["n_flagged"] == 2
    v.Redraw()
    got, s2 = assert_device_equals_twin(v, history_from(s, shown), tab, xf, xf2, M_SHORT, **P_SHORT)
    assert not same_bits(got, s2["a"]) and len(xf2) == {"add_object": 8, "geometry_and_build": 5}.get(setter, 7)
    # ... and a second step, X_hist advanced over the new count
    xf3 = xf2.copy(); xf3[moved] = rigid(8.0, (0, 0, 1), (0.03, 0.03, 0.01))
    v.set_transforms(xf3); v.Redraw()
    assert_device_equals_twin(v, history_from(s2, got), tab, xf2, xf3, M_SHORT, **P_SHORT)
    assert v.get_reproject_motion()["n_flagged"] == 1
    v.close()


@pytest.mark.gpu
def test_ldr_read_outs_show_the_reprojected_image_across_an_object_step(hip_lib):
    W, H = 67, 45
    v, sc, tab = room(W, H)
    v.SetReproject(); v.SetReprojectMotion(max_history_moved=6.0, max_history_static=3.0)
    M = dict(max_history_moved=f32(6.0), max_history_static=f32(3.0))
    xf0 = identity_xforms()
    v.Redraw(); v.Redraw()
    s0 = planes_of(v); shown0 = v.read_reprojected()
    assert same_bits(shown0, s0["a"])
    xf1 = xf0.copy(); xf1[3] = rigid(10.0, (0, 0, 1), (0.03, 0.01, 0.0))
    v.set_transforms(xf1); v.Redraw()
    shown1, s1 = assert_device_equals_twin(v, history_from(s0, shown0), tab, xf0, xf1, M, **ref.DEFAULTS)
    assert not same_bits(shown1, s1["a"])
    d = v.get_display()
    display = (d["tonemap_mode"], d["exposure"], d["white_point"])
    sc1 = dataclasses.replace(sc, obj_xform=xf1)
    want1 = ldr_of_a_context_handed(shown1, 1, sc1, display)
    got = v.read_ldr()
    assert np.array_equal(got, want1)                                            # the tone map of the twin's image
    plain = ldr_of_a_context_handed(s1["a"], 1, sc1, display)
    assert not np.array_equal(got, plain)
    # two read-backs in flight across an object step: each shows the image of its moment
    v.read_ldr_begin()                                                           # frame of placement 1
    xf2 = xf1.copy(); xf2[3] = rigid(14.0, (0, 0, 1), (0.05, 0.02, 0.0)); xf2[6] = rigid(0.0, (0, 0, 1), (0.0, 0.03, 0.04))
    v.set_transforms(xf2); v.Redraw()
    v.read_ldr_begin()                                                           # frame of placement 2
    first, second = v.read_ldr_end(), v.read_ldr_end()
    assert np.array_equal(first, want1)
    shown2, s2 = assert_device_equals_twin(v, history_from(s1, shown1), tab, xf1, xf2, M, **ref.DEFAULTS)
    assert np.array_equal(second, ldr_of_a_context_handed(shown2, 1, dataclasses.replace(sc, obj_xform=xf2), display)) and np.array_equal(second, v.read_ldr())
    assert not np.array_equal(first, second)
    # the metering reads the unfiltered accumulator: the same histogram with both features off
    v.set_auto_exposure(True)
    m = v.measure_exposure()
    metered = v.read_ldr()
    assert np.array_equal(metered, ldr_of_a_context_handed(shown2, 1, dataclasses.replace(sc, obj_xform=xf2), (display[0], m["exposure"], m["white_point"])))
    v.ClearReprojectMotion(); v.ClearReproject()
    m_off = v.measure_exposure()
    assert np.array_equal(m_off["hist"], m["hist"]) and m_off["exposure"] == m["exposure"] and m_off["white_point"] == m["white_point"]
    v.close()


@pytest.mark.gpu
def test_the_motion_feature_leaves_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")

    def placements(k):
        xf = identity_xforms()
        if k:
            xf[3] = rigid(6.0 * k, (0, 0, 1), (0.02 * k, 0.0, 0.0)); xf[5] = rigid(0.0, (0, 0, 1), (0.0, 0.01 * k, 0.02 * k), 0.9)
        return xf

    def drag(v, reads):
        out = []
        for k in range(3):
            if k:
                v.set_transforms(placements(k))
            v.Redraw()
            out.append(reads(v, k))
        return out

    def everything(v, k):
        acc, frames = v.save_accum()
        st = v.stats()
        return dict(hdr=v.read_hdr(), acc=acc, frames=frames, stats=[st[c] for c in counters], ids=v.read_ids(), tiles=v.tile_stats())

    def assert_same(x, y):
        assert same_bits(x["hdr"], y["hdr"]) and same_bits(x["acc"], y["acc"]) and x["frames"] == y["frames"] == 1 and x["stats"] == y["stats"]
        assert all(np.array_equal(bits(p) if p.dtype == f32 else p, bits(q) if q.dtype == f32 else q) for p, q in zip(x["ids"], y["ids"]))
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(x["tiles"], y["tiles"]))

    never = View(0).load_scene(sc)
    want = drag(never, everything)
    never.close()
    never = View(0).load_scene(sc)
    never_ldr = drag(never, lambda v, k: v.read_ldr())                           # the LDR bytes of the drag in a context that never heard of either feature
    never.close()
    only_rp = View(0).load_scene(sc); only_rp.SetReproject()
    rp_ldr = drag(only_rp, lambda v, k: v.read_ldr())                            # reprojection alone: set_transforms drops the history, the bytes of `never`
    only_rp.close()
    assert all(np.array_equal(x, y) for x, y in zip(rp_ldr, never_ldr))
    v = View(0)
    v.SetReprojectMotion(max_history_moved=8.0)                                  # set before the scene exists: display state outlives a new scene
    v.load_scene(sc)
    assert v.get_reproject_motion()["on"] and v.get_reproject_motion()["max_history_moved"] == 8.0
    alone = drag(v, lambda v, k: v.read_ldr())                                   # motion without reprojection: no effect at all
    assert all(np.array_equal(x, y) for x, y in zip(alone, never_ldr)) and v.get_reproject()["history_valid"] is False
    v.close()
    v = View(0)
    v.SetReprojectMotion(max_history_moved=8.0); v.SetReproject()
    v.load_scene(sc)

    def with_read_outs(v, k):
        v.read_ldr(); v.read_reprojected(); v.read_ldr_begin(); v.read_ldr_end(); v.get_reproject_motion()
        return everything(v, k)
    got = drag(v, with_read_outs)
    assert v.get_reproject()["history_valid"] and v.get_reproject_motion()["n_flagged"] == 2
    for x, y in zip(got, want):
        assert_same(x, y)
    assert not np.array_equal(v.read_ldr(), never_ldr[2])
    v.ClearReprojectMotion(); v.ClearReproject()
    assert np.array_equal(v.read_ldr(), never_ldr[2])                            # off again: the bytes of the context that never switched anything on
    v.close()


@pytest.mark.gpu
def test_set_reproject_motion_refusals_state_and_bench(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    for bad, why in BAD_CAPS:
        with pytest.raises(BackendError, match=f"-> -1: crh_set_reproject_motion: .*{why}"):
            v.set_reproject_motion(True, **bad)
        assert v.get_reproject_motion()["on"] is False                           # a refused call changes nothing
    v.set_reproject_motion(True, max_history_moved=1024.0, max_history_static=1.0)      # the limits themselves; allowed before crh_build
    g = v.get_reproject_motion()
    assert g["on"] and (float(g["max_history_moved"]), float(g["max_history_static"]), g["n_flagged"]) == (1024.0, 1.0, 0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4.*crh_build has not been called"):
        v.bench_reproject_motion(1)
    v.load_scene(sc)
    v.SetReproject(); v.SetReprojectMotion()
    v.Redraw()
    before = v.read_reprojected()
    b = v.bench_reproject_motion(3)                                              # no history, nothing flagged: the stand-ins, and nothing a read-out sees moves
    assert b["resolve_ms"] > 0.0 and same_bits(v.read_reprojected(), before) and v.get_reproject()["history_valid"] is False
    xf = identity_xforms(); xf[3] = rigid(5.0, (0, 0, 1), (0.03, 0.0, 0.0))
    v.set_transforms(xf); v.Redraw()
    before = v.read_reprojected()
    b = v.bench_reproject_motion(3)                                              # the table in force
    assert b["resolve_ms"] > 0.0 and same_bits(v.read_reprojected(), before) and v.get_reproject_motion()["n_flagged"] == 1
    assert v.bench_reproject(3)["resolve_ms"] > 0.0 and same_bits(v.read_reprojected(), before)
    v.close()


@pytest.mark.gpu
def test_it_helps_through_an_object_drag(hip_lib):
    """THE test of what the feature is for.  The closed room of test_it_denoises (the light out of view) at 96 x 64, every material an object: the tall box is
    translated in eight steps of 0.002 of the room's extent at 1 spp each, every frame read out.  Over the moved part's hit pixels the mean squared error of the last
    DISPLAYED image against 512 spp of the final placement is below HALF that of the raw 1-spp image -- the issue's condition: two effective samples of equal variance
    already give it.  PRECONDITION, asserted first: the 512-spp images of the first and of the last placement differ over those pixels by less than 1 % of the raw
    image's error, so a lagging history cannot be what decides the test.  The measured ratios for moved and static pixels are printed (DESIGN.md 6.12 carries them)."""
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = closed_room(W, H)
    tri_obj = sc.tri[:, 3].astype(np.int32)
    n = int(tri_obj.max()) + 1
    sc = dataclasses.replace(sc, tri_object=tri_obj, obj_xform=np.tile(rigid(), (n, 1)))
    BOX = 4                                                                      # the tall box: the one the camera inside the room sees
    place = lambda k: np.concatenate([np.tile(rigid(), (BOX, 1)), rigid(0.0, (0, 0, 1), (0.002 * k, 0.0, 0.0))[None], np.tile(rigid(), (n - BOX - 1, 1))])
    t0 = View(0).load_scene(sc)
    t0.render(512)
    truth_first = t0.read_hdr().astype(np.float64)
    t0.close()
    v = View(0).load_scene(sc)
    v.SetReproject(); v.SetReprojectMotion()
    for k in range(9):                                                           # the first placement, then eight steps
        if k:
            v.set_transforms(place(k))
        v.Redraw()
        v.read_ldr()                                                             # a host that displays its frames
    assert v.get_reproject()["history_valid"] and v.get_reproject_motion()["n_flagged"] == 1 and v.save_accum()[1] == 1
    raw = v.read_hdr().astype(np.float64)
    shown = v.read_reprojected()
    ob, tr, _ = v.read_ids()
    hit = tr >= 0
    moved, static = hit & (ob == BOX), hit & (ob != BOX)
    v.render(511)
    assert v.save_accum()[1] == 512
    truth = v.read_hdr().astype(np.float64)
    v.close()
    mse = lambda img, mask: float(((img - truth)[mask] ** 2).mean())
    shown3 = shown[..., :3].astype(np.float64)
    raw_moved, raw_static = mse(raw, moved), mse(raw, static)
    lag = float(((truth_first - truth)[moved] ** 2).mean())
    print(f"8 object steps of 0.002 at 1 spp against 512 spp: moved part {int(moved.sum())} px: mse raw {raw_moved:.6g}, shown {mse(shown3, moved):.6g}, "
          f"ratio {mse(shown3, moved) / raw_moved:.4f}; static {int(static.sum())} px: mse raw {raw_static:.6g}, shown {mse(shown3, static):.6g}, "
          f"ratio {mse(shown3, static) / raw_static:.4f}; first-to-last placement over the moved part {lag:.6g} = {lag / raw_moved:.4f} of the raw error; "
          f"mean effective samples moved {float(shown[..., 3][moved].mean()):.2f}, static {float(shown[..., 3][static].mean()):.2f}")
    assert hit.all() and moved.sum() > 100 and raw_moved > 0.0 and truth.max() < 25.0      # closed, noisy, and no pixel shows the light itself
    assert lag < 0.01 * raw_moved                                                # the precondition
    assert mse(shown3, moved) < 0.5 * raw_moved
