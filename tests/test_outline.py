"""Feature lines on the display: object, depth and crease edges from the first-hit id buffer (crh_outline.cpp, cadrays_amd/csrc/outline_kernels.hip).

The reference has no counterpart: OCCT's path tracer draws no edges, src/Launcher/DataNode.cxx:286 only sets a display mode of the rasteriser.  Everything is compared
bit for bit; no tolerance appears in this file.

  CPU   the struct's layout and the exports; crh_outline_table_host, crh_outline_mask_host and crh_outline_draw_host == the numpy restatement
        (tests/outline_reference.py, written from the header's text); properties that need no restatement; each deliberately wrong rule changes a mask; every refusal
  GPU   known answers under an orthographic camera whose pixel boundaries are the geometry's edges; crh_read_outline == the host twin == numpy through scenes, sizes,
        cameras and the states of a live scene; the LDR read-outs == the numpy drawing rule over the bytes without lines; nothing else moves

ONE CASE OF THE ISSUE IS NOT AS IT STATES IT: "a strip folded by 90 degrees ... no crease at crease_cos = cos 100 degrees taken through the absolute value".  The
normals of such a strip have the dot product 0, and |0| < crease_cos holds for every crease_cos the setter accepts, (0, 1]; cos 100 degrees itself is negative and is
refused.  test_known_answer_folded_strips pins what the stated rule gives (a crease at every accepted threshold, cos 80 = |cos 100| included; the refusal of cos 100)
and shows the absolute value on strips where it decides: a 20-degree fold, and the same with one face wound the other way round (normals 160 degrees apart).
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import outline_reference as ref
from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_overlay import restated as overlay_restated
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("crh_outline_defaults", "crh_set_outline", "crh_get_outline", "crh_read_outline", "crh_outline_table_host", "crh_outline_mask_host", "crh_outline_draw_host")


def _api():
    """the three host-only entry points through the Python mirror: a missing one FAILS here (AttributeError / ImportError), it does not skip"""
    from cadrays_amd.view import outline_draw_host, outline_mask_host, outline_table_host
    return outline_table_host, outline_mask_host, outline_draw_host


def where_differs(a, b):
    return [(int(y), int(x), int(a[y, x]), int(b[y, x])) for y, x in np.argwhere(a != b)[:6]]


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_outline_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in abi.crh_outline_params._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(crh_outline_params));' + "".join(
        f'printf("%zu ", offsetof(crh_outline_params, {n}));' for n in fields) + 'printf("%u %u %u", CRH_OUTLINE_OBJECT, CRH_OUTLINE_DEPTH, CRH_OUTLINE_CREASE);return 0;}'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [C.sizeof(abi.crh_outline_params)] + [getattr(abi.crh_outline_params, n).offset for n in fields] + [abi.OUTLINE_OBJECT, abi.OUTLINE_DEPTH, abi.OUTLINE_CREASE], got
    assert C.sizeof(abi.crh_outline_params) == 20 and np.dtype(abi.OUTLINE_TABLE_DTYPE).itemsize == 32 and np.dtype(abi.OUTLINE_TABLE_DTYPE) == ref.TABLE_DTYPE
    assert (abi.OUTLINE_OBJECT, abi.OUTLINE_DEPTH, abi.OUTLINE_CREASE) == (ref.OBJECT, ref.DEPTH, ref.CREASE)
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS and (f"CRH_API int {name}(" in header or f"CRH_API void {name}(" in header), name


def test_entry_points_are_exported_and_defaults_agree(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    p = abi.crh_outline_params()
    hip_lib.crh_outline_defaults.restype = None
    hip_lib.crh_outline_defaults(C.byref(p))
    d = abi.OUTLINE_DEFAULTS
    assert (p.kinds, p.width, tuple(p.rgb), p.alpha) == (d["kinds"], d["width"], d["rgb"], d["alpha"]) == (7, 1, (0, 0, 0), 255)
    assert f32(p.crease_cos) == f32(d["crease_cos"]) == ref.DEFAULT_COS and f32(p.depth_ratio) == f32(d["depth_ratio"]) == ref.DEFAULT_RATIO
    from cadrays_amd.view import outline_crease_cos, outline_depth_ratio
    assert f32(outline_crease_cos(30.0)) == ref.DEFAULT_COS and f32(outline_depth_ratio(0.02)) == ref.DEFAULT_RATIO


# ------------------------------------------------------------------------------------------------ CPU 2: the table
def test_table_equals_the_float64_restatement(hip_lib):
    table_host, _, _ = _api()
    r = np.random.default_rng(11)
    pos = r.uniform(-3.0, 3.0, (600, 3)).astype(f32)
    tri = np.concatenate([r.integers(0, 600, (900, 3)), r.integers(0, 5, (900, 1))], 1).astype(np.int32)
    tri[3, :3] = (7, 7, 7)                                          # a point
    tri[4, :3] = (9, 9, 12)                                         # two equal vertices
    pos[20], pos[21], pos[22] = (0, 0, 0), (1, 2, 3), (2, 4, 6)     # a zero-area triangle of three different vertices
    tri[5, :3] = (20, 21, 22)
    pos[30], pos[31], pos[32] = (1e30, 0, 0), (-1e30, 1e30, 0), (0, -1e30, 1e30)      # huge edges: the cross product ~1e60, far beyond float32
    tri[6, :3] = (30, 31, 32)
    pos[40], pos[41], pos[42] = (1e-30, 0, 0), (0, 1e-30, 0), (0, 0, 1e-30)           # tiny edges: the cross product ~1e-60
    tri[7, :3] = (40, 41, 42)
    pos[50], pos[51], pos[52] = (1e-45, 0, 0), (0, 1e-45, 0), (0, 0, 0)               # denormal positions
    tri[8, :3] = (50, 51, 52)
    pos[60], pos[61], pos[62] = (3e38, 3e38, 3e38), (-3e38, 3e38, -3e38), (1e-40, -3e38, 3e38)      # the largest finite edges
    tri[9, :3] = (60, 61, 62)
    got, want = table_host(pos, tri), ref.table(pos, tri)
    assert got.dtype == ref.TABLE_DTYPE and got.tobytes() == want.tobytes(), np.flatnonzero(np.frombuffer(got.tobytes(), "V32") != np.frombuffer(want.tobytes(), "V32"))[:5]
    assert list(want["degenerate"][3:10]) == [1, 1, 1, 0, 0, 0, 0] and want["degenerate"].sum() >= 3
    ok = want["degenerate"] == 0
    assert np.all(np.abs(np.linalg.norm(want["n"][ok].astype(np.float64), axis=1) - 1.0) < 1e-6) and not want["n"][~ok].any()
    assert np.array_equal(want["v"], tri[:, :3].astype(np.uint32)) and not want["pad"].any()


# ------------------------------------------------------------------------------------------------ CPU 3: the mask
CASES = None


def fixed_cases():
    global CASES
    if CASES is None:
        CASES = ref.cases()
    return CASES


def test_mask_host_equals_the_numpy_restatement(hip_lib):
    _, mask_host, _ = _api()
    seen = 0
    sizes = set()
    for name, ob, tr, t, tab, cc, dr in fixed_cases():
        want = ref.mask(ob, tr, t, tab, cc, dr)
        got = mask_host(ob, tr, t, tab, cc, dr)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, where_differs(got, want))
        seen |= int(np.bitwise_or.reduce(want, axis=None))
        sizes.add(ob.shape[::-1])
        # other thresholds on the same planes
        if name.startswith("random") and ob.size > 100:
            for cc2, dr2 in ((f32(1.0), f32(1.0)), (f32(0.3), f32(3.0))):
                got, want = mask_host(ob, tr, t, tab, cc2, dr2), ref.mask(ob, tr, t, tab, cc2, dr2)
                assert np.array_equal(got, want), (name, cc2, dr2, where_differs(got, want))
    assert seen == 7 and set(ref.SIZES) <= sizes
    # no table at all: only OBJECT
    name, ob, tr, t, tab, cc, dr = fixed_cases()[40]
    got = mask_host(ob, tr, t, None)
    assert np.array_equal(got, ref.mask(ob, tr, t, None)) and not (got & 6).any() and got.any()


def test_fixed_cases_cover_what_the_issue_lists(hip_lib):
    rand = [c for c in fixed_cases() if c[0].startswith("random")]
    big = [c for c in rand if c[1].size > 1000]
    assert all(0.1 < (c[2] < 0).mean() < 0.3 for c in big)                                      # about 20 % misses
    assert all((c[2][:, 1:] == c[2][:, :-1]).mean() > 0.2 for c in big)                         # runs of equal triangles
    assert all(((c[3][:, 1:] == c[3][:, :-1]) & (c[2][:, 1:] >= 0)).any() for c in big)         # equal t across a pair of hits
    assert all((c[2] >= len(c[4])).any() for c in big)                                          # triangle ids beyond the table
    assert all(c[4]["degenerate"].any() for c in rand)                                          # degenerate records
    share = lambda tab: np.mean([(tab["v"][k][:, None] == tab["v"][k - 1][None, :]).any() for k in range(1, len(tab))])
    rates = sorted({round(float(share(c[4])), 1) for c in rand})
    assert rates[0] < 0.15 and rates[-1] > 0.8 and len(rates) >= 3, rates                        # shared vertices at controlled rates


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_each_wrong_rule_changes_a_mask(hip_lib, wrong):
    """the fixed cases tell the rule from its five near misses: were the library to implement one of them, test_mask_host_equals_the_numpy_restatement would fail"""
    _, mask_host, _ = _api()
    changed = [name for name, ob, tr, t, tab, cc, dr in fixed_cases() if not np.array_equal(ref.mask(ob, tr, t, tab, cc, dr, wrong), mask_host(ob, tr, t, tab, cc, dr))]
    assert changed, wrong


def test_properties_that_need_no_restatement(hip_lib):
    table_host, mask_host, _ = _api()
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 5), (1, 0, 5), (0, 0, 6)], f32)
    tab = table_host(pos, np.array([(0, 1, 2, 0), (3, 4, 5, 0)], np.int32))
    H, W = 5, 6
    # a frame of one triangle has an empty mask
    one = mask_host(np.zeros((H, W), np.int32), np.zeros((H, W), np.int32), np.full((H, W), 3.0, f32), tab)
    assert not one.any()
    # two different objects side by side at different t: a one-pixel column on the nearer one
    ob = np.zeros((H, W), np.int32); ob[:, 3:] = 1
    tr = ob.copy()
    for t_left, t_right, col in ((2.0, 5.0, 2), (5.0, 2.0, 3), (4.0, 4.0, 2)):      # ... and at equal t the left pixel
        t = np.where(ob == 0, f32(t_left), f32(t_right)).astype(f32)
        want = np.zeros((H, W), np.uint8); want[:, col] = abi.OUTLINE_OBJECT
        assert np.array_equal(mask_host(ob, tr, t, tab), want), (t_left, t_right)
    # one above the other at equal t: the upper pixel
    want = np.zeros((W, H), np.uint8); want[2, :] = abi.OUTLINE_OBJECT
    assert np.array_equal(mask_host(ob.T, tr.T, np.full((W, H), 4.0, f32), tab), want)
    # an object beside the background: the line lies on the object
    miss = ob.copy(); miss[:, 3:] = -1
    tm = np.where(miss < 0, f32(1e15), f32(7.0)).astype(f32)
    want = np.zeros((H, W), np.uint8); want[:, 2] = abi.OUTLINE_OBJECT
    assert np.array_equal(mask_host(miss, miss, tm, tab), want)
    # transposing all planes transposes the mask; raising depth_ratio or lowering crease_cos never adds a bit
    for name, ob, tr, t, tb, cc, dr in fixed_cases()[::7]:
        m = mask_host(ob, tr, t, tb, cc, dr)
        assert np.array_equal(mask_host(ob.T, tr.T, t.T, tb, cc, dr), m.T), name
        for cc2, dr2 in ((cc, f32(dr * 1.5)), (f32(cc * 0.5), dr), (f32(cc * 0.01), f32(50.0))):
            m2 = mask_host(ob, tr, t, tb, cc2, dr2)
            assert not (m2 & ~m).any(), (name, cc2, dr2)
            assert np.array_equal(m2 & 1, m & 1), name                       # the thresholds do not move object lines


# ------------------------------------------------------------------------------------------------ CPU 4: the drawing
@pytest.mark.parametrize("width", [1, 2, 3])
def test_draw_host_equals_the_numpy_rule(hip_lib, width):
    _, _, draw_host = _api()
    r = np.random.default_rng(5 + width)
    for W, H in ((1, 1), (2, 1), (1, 3), (7, 5), (65, 9), (130, 67)):
        mask = (r.integers(0, 8, (H, W)) * (r.random((H, W)) < 0.15)).astype(np.uint8)
        mask[0, 0] = 7 if W * H > 1 else 1; mask[-1, -1] |= 4
        ldr = r.integers(0, 256, (H, W, 3)).astype(np.uint8)
        for alpha in (0, 1, 128, 254, 255):
            for kinds in (7, 1, 2, 4, 5, 0):
                rgb = tuple(int(x) for x in r.integers(0, 256, 3))
                got = draw_host(mask, ldr, kinds=kinds, width=width, rgb=rgb, alpha=alpha)
                want = ref.draw(mask, ldr, kinds, width, rgb, alpha)
                assert np.array_equal(got, want), (W, H, alpha, kinds, np.argwhere(got != want)[:4])
                if kinds == 0 or alpha == 0:
                    assert np.array_equal(got, ldr)
    # the window: one marked pixel in the middle of a 5 x 5 frame
    mask = np.zeros((5, 5), np.uint8); mask[2, 2] = 1
    drawn = draw_host(mask, np.zeros((5, 5, 3), np.uint8), width=width, rgb=(255, 255, 255))[..., 0] == 255
    want = np.zeros((5, 5), bool)
    want[{1: slice(2, 3), 2: slice(1, 3), 3: slice(1, 4)}[width], {1: slice(2, 3), 2: slice(1, 3), 3: slice(1, 4)}[width]] = True      # a pixel looks at dx, dy in [0, 1] for width 2: the line grows up and left
    assert np.array_equal(drawn, want)


# ------------------------------------------------------------------------------------------------ CPU 5: refusals
def test_refusals_of_the_host_entry_points(hip_lib):
    table_host, mask_host, draw_host = _api()
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], f32); tri = np.array([(0, 1, 2, 0)], np.int32)
    tab = table_host(pos, tri)
    with pytest.raises(BackendError):
        table_host(pos, np.array([(0, 1, 3, 0)], np.int32))                  # an index beyond the vertices
    with pytest.raises(BackendError):
        table_host(pos, np.array([(0, -1, 2, 0)], np.int32))
    ob = np.zeros((2, 3), np.int32); t = np.ones((2, 3), f32)
    mask_host(ob, ob, t, tab, 1.0, 1.0); mask_host(ob, ob, t, tab, 1e-6, 1e30)
    for cc, dr in ((0.0, 1.02), (-0.5, 1.02), (1.0000001, 1.02), (np.nan, 1.02), (np.inf, 1.02), (0.5, 0.999), (0.5, np.nan), (0.5, np.inf), (0.5, -np.inf)):
        with pytest.raises(BackendError):
            mask_host(ob, ob, t, tab, cc, dr)
    m = np.zeros((2, 3), np.uint8); img = np.zeros((2, 3, 3), np.uint8)
    draw_host(m, img, kinds=0); draw_host(m, img, width=3, alpha=0)
    for bad in (dict(kinds=8), dict(kinds=0x80000001), dict(width=0), dict(width=4), dict(crease_cos=0.0), dict(crease_cos=1.5), dict(crease_cos=float("nan")),
                dict(depth_ratio=0.5), dict(depth_ratio=float("inf")), dict(depth_ratio=float("nan"))):
        with pytest.raises(BackendError):
            draw_host(m, img, **bad)
    # NULL pointers and empty frames, straight at the library
    i32p, fp, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    po, pt, pm, pi, ptab = ob.ctypes.data_as(i32p), t.ctypes.data_as(fp), m.ctypes.data_as(u8p), img.ctypes.data_as(u8p), tab.ctypes.data_as(C.c_void_p)
    W, H, one, cc, dr = C.c_uint32(3), C.c_uint32(2), C.c_uint32(1), C.c_float(0.5), C.c_float(1.02)
    host = hip_lib.crh_outline_mask_host
    assert host(po, po, pt, W, H, ptab, one, cc, dr, pm) == abi.OK and host(po, po, pt, W, H, None, C.c_uint32(0), cc, dr, pm) == abi.OK
    assert host(None, po, pt, W, H, ptab, one, cc, dr, pm) == abi.E_INVALID and host(po, None, pt, W, H, ptab, one, cc, dr, pm) == abi.E_INVALID
    assert host(po, po, None, W, H, ptab, one, cc, dr, pm) == abi.E_INVALID and host(po, po, pt, W, H, ptab, one, cc, dr, None) == abi.E_INVALID
    assert host(po, po, pt, C.c_uint32(0), H, ptab, one, cc, dr, pm) == abi.E_INVALID and host(po, po, pt, W, C.c_uint32(0), ptab, one, cc, dr, pm) == abi.E_INVALID
    assert host(po, po, pt, W, H, None, one, cc, dr, pm) == abi.E_INVALID                     # a count without a table
    p = abi.crh_outline_params(); hip_lib.crh_outline_defaults.restype = None; hip_lib.crh_outline_defaults(C.byref(p)); hip_lib.crh_outline_defaults(None)
    draw = hip_lib.crh_outline_draw_host
    assert draw(pm, W, H, C.byref(p), pi) == abi.OK
    assert draw(None, W, H, C.byref(p), pi) == abi.E_INVALID and draw(pm, W, H, None, pi) == abi.E_INVALID and draw(pm, W, H, C.byref(p), None) == abi.E_INVALID
    assert draw(pm, C.c_uint32(0), H, C.byref(p), pi) == abi.E_INVALID
    tb = hip_lib.crh_outline_table_host
    pp, ptri = pos.ctypes.data_as(fp), tri.astype(np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    three = C.c_uint32(3)
    assert tb(pp, three, ptri, one, ptab) == abi.OK
    assert tb(None, three, ptri, one, ptab) == abi.E_INVALID and tb(pp, three, None, one, ptab) == abi.E_INVALID and tb(pp, three, ptri, one, None) == abi.E_INVALID
    assert tb(pp, three, ptri, C.c_uint32(0), ptab) == abi.E_INVALID and tb(pp, C.c_uint32(2), ptri, one, ptab) == abi.E_INVALID
    for fn in ("crh_set_outline", "crh_get_outline", "crh_read_outline"):
        assert getattr(hip_lib, fn)(None, None) == abi.E_INVALID if fn != "crh_get_outline" else hip_lib.crh_get_outline(None, None, None) == abi.E_INVALID


# ================================================================================================ GPU
def scene_table(pos, tri):
    """the table of a scene's own geometry: the library's bytes, which are the restatement's"""
    table_host, _, _ = _api()
    tab = table_host(pos, tri)
    assert tab.tobytes() == ref.table(pos, tri).tobytes()
    return tab


def assert_device_equals_twin_and_numpy(v, tab, cc=ref.DEFAULT_COS, dr=ref.DEFAULT_RATIO):
    """crh_read_outline on the context's current state against both restatements over the planes crh_read_ids returns; returns (mask, planes)"""
    _, mask_host, _ = _api()
    ob, tr, t = v.read_ids()
    got = v.read_outline()
    want = ref.mask(ob, tr, t, tab, cc, dr)
    assert got.shape == ob.shape and np.array_equal(got, want), where_differs(got, want)
    twin = mask_host(ob, tr, t, tab, cc, dr)
    assert np.array_equal(got, twin), where_differs(got, twin)
    return got, (ob, tr, t)


def ortho_scene(P, T, obj, W, H):
    """triangles seen by an orthographic camera looking along +y whose pixel (px, py) has its centre at x = px + 0.5, z = H - py - 0.5: geometry whose edges lie
    on integers has them on pixel boundaries.  T: rows (v0, v1, v2); obj: the object of every triangle, or None (one scene-wide object)"""
    base = scenes.cornell_box(False, W, H)
    pos = np.array(P, f32)
    tri = np.array([tuple(t) + (0,) for t in T], np.int32)
    cam = scenes.Camera(eye=(W / 2, -5.0, H / 2), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fovy_deg=40.0, is_ortho=True, ortho_scale=H / 2, aspect=W / H)
    kw = {}
    if obj is not None:
        kw = dict(tri_object=np.array(obj, np.int32), obj_xform=np.tile(rigid(), (max(obj) + 1, 1)))
    return dataclasses.replace(base, pos=pos, nrm=np.tile(np.array([0, -1, 0], f32), (len(pos), 1)), tri=tri, uv=None, textures=[], camera=cam, **kw)


def quad(P, T, x0, x1, z0, z1, y00, y10=None, y11=None, y01=None, welded=True, flip=False):
    """a quad over [x0, x1] x [z0, z1] with the depths of its four corners; two triangles split along the diagonal (x0, z0) - (x1, z1)"""
    y10 = y00 if y10 is None else y10; y11 = y10 if y11 is None else y11; y01 = y00 if y01 is None else y01
    k = len(P)
    a, b, c, d = (x0, y00, z0), (x1, y10, z0), (x1, y11, z1), (x0, y01, z1)
    if welded:
        P += [a, b, c, d]
        T += [(k, k + 1, k + 2), (k, k + 3, k + 2) if flip else (k, k + 2, k + 3)]
    else:
        P += [a, b, c, a, c, d]
        T += [(k, k + 1, k + 2), (k + 3, k + 4, k + 5)]


def pixel_box(W, H, x0, x1, z0, z1):
    """the pixels whose centres lie in [x0, x1] x [z0, z1] (integers)"""
    m = np.zeros((H, W), bool)
    m[max(H - z1, 0):max(H - z0, 0), max(x0, 0):max(x1, 0)] = True
    return m


def inner_edge(region, other):
    """the pixels of `region` with a 4-neighbour inside the frame that lies in `other`"""
    n = np.zeros_like(region)
    n[:, 1:] |= other[:, :-1]; n[:, :-1] |= other[:, 1:]; n[1:] |= other[:-1]; n[:-1] |= other[1:]
    return region & n


KW, KH = 16, 16


@pytest.mark.gpu
def test_known_answer_two_objects_and_two_unconnected_quads(hip_lib):
    from cadrays_amd.view import View
    near, far = pixel_box(KW, KH, 6, 14, 6, 14), pixel_box(KW, KH, 2, 10, 2, 10)
    far_seen, back = far & ~near, ~(far | near)
    for objects in ((0, 0, 1, 1), (0, 0, 0, 0)):
        P, T = [], []
        quad(P, T, 2, 10, 2, 10, 2.0)                    # the far square at y = 2, t = 7
        quad(P, T, 6, 14, 6, 14, 1.0)                    # the near one at y = 1, t = 6: 7 > 6 * 1.02
        sc = ortho_scene(P, T, objects, KW, KH)
        v = View(0).load_scene(sc)
        got, (ob, tr, t) = assert_device_equals_twin_and_numpy(v, scene_table(sc.pos, sc.tri))
        assert np.array_equal(ob >= 0, ~back) and np.abs(t[near] - 6.0).max() < 1e-4 and np.abs(t[far_seen] - 7.0).max() < 1e-4
        want = np.zeros((KH, KW), np.uint8)
        want[inner_edge(near, back) | inner_edge(far_seen, back)] |= abi.OUTLINE_OBJECT
        # where the squares overlap the line lies on the NEARER one: its lowest row and leftmost column inside the far square, nothing on the far square there
        want[inner_edge(near, far_seen)] |= abi.OUTLINE_OBJECT if objects[2] else abi.OUTLINE_DEPTH
        assert np.array_equal(got, want), (objects, where_differs(got, want))
        assert got[9, 6] and not got[10, 6] and not got[9, 5] and not got[8, 7]      # (px 6, py 9) is the near square's corner inside the far one
        v.close()


@pytest.mark.gpu
def test_known_answer_tilted_quad_welded_and_unwelded(hip_lib):
    """one quad filling the frame, y = 1 + 4 x: t = 8 + 4 px steps by a factor 1.5 .. 1.0625 from pixel to pixel.  Welded, its two triangles share two vertex indices:
    no depth line.  Unwelded (the documented limit, pinned): a depth line wherever a pixel and its right neighbour lie in different triangles, on the nearer, left one"""
    from cadrays_amd.view import View
    x = np.arange(KW) + 0.5
    z = KH - np.arange(KH) - 0.5
    upper = z[:, None] > -2.0 + (x[None, :] + 1.0) * 19.0 / 18.0           # above the diagonal (-1, -2) - (17, 17): no pixel centre lies on it
    for welded in (True, False):
        P, T = [], []
        quad(P, T, -1, 17, -2, 17, -3.0, 69.0, welded=welded)
        sc = ortho_scene(P, T, None, KW, KH)
        v = View(0).load_scene(sc)
        got, (ob, tr, t) = assert_device_equals_twin_and_numpy(v, scene_table(sc.pos, sc.tri))
        assert np.array_equal(tr, upper.astype(np.int32)) and (ob == 0).all()
        assert (t[:, 1:] > t[:, :-1] * f32(1.05)).all() and np.abs(t - (8.0 + 4.0 * np.arange(KW))[None, :]).max() < 1e-3
        want = np.zeros((KH, KW), np.uint8)
        if not welded:
            want[:, :-1][upper[:, 1:] != upper[:, :-1]] = abi.OUTLINE_DEPTH
            assert want.sum() > 0
        assert np.array_equal(got, want), (welded, where_differs(got, want))
        v.close()


def folded_strip(slope_left, slope_right, flip_right=False):
    """two welded quads that meet in the ridge x = 8, y = 2: y = 2 + slope_left (8 - x) on the left, y = 2 + slope_right (x - 8) on the right"""
    P = [(-1, 2 + 9 * slope_left, -2), (8, 2, -2), (8, 2, 17), (-1, 2 + 9 * slope_left, 17), (17, 2 + 9 * slope_right, -2), (17, 2 + 9 * slope_right, 17)]
    T = [(0, 1, 2), (0, 2, 3)] + ([(1, 5, 4), (1, 2, 5)] if flip_right else [(1, 4, 5), (1, 5, 2)])
    return ortho_scene(P, T, None, KW, KH)


@pytest.mark.gpu
def test_known_answer_folded_strips(hip_lib):
    """(see the module's docstring for the case of the issue that its own rule contradicts)"""
    from cadrays_amd.view import View, outline_crease_cos
    column = lambda px: np.where(np.arange(KW)[None, :] == px, np.uint8(abi.OUTLINE_CREASE), np.uint8(0)) * np.ones((KH, 1), np.uint8)
    # folded by 90 degrees: slopes 2 and 1/2, normals (2, 1) and (-1, 2) over sqrt 5.  t(px 7) = 8, t(px 8) = 7.25: the line lies on px 8
    sc = folded_strip(2.0, 0.5)
    tab = scene_table(sc.pos, sc.tri)
    n = tab["n"]
    assert np.abs((n[0, 0] * n[2, 0] + n[0, 1] * n[2, 1]) + n[0, 2] * n[2, 2]) < 1e-7
    v = View(0).load_scene(sc)
    got, (ob, tr, t) = assert_device_equals_twin_and_numpy(v, tab)
    assert np.array_equal(got, column(8)) and np.abs(t[:, 7] - 8.0).max() < 1e-4 and np.abs(t[:, 8] - 7.25).max() < 1e-4
    for deg in (80.0, 89.9, 1.0):                           # |0| < crease_cos for every threshold the setter takes: cos 80 = |cos 100| included
        v.SetOutline(crease_deg=deg)
        got, _ = assert_device_equals_twin_and_numpy(v, tab, f32(outline_crease_cos(deg)))
        assert np.array_equal(got, column(8)), deg
    with pytest.raises(BackendError, match="-> -1: crh_set_outline: crease_cos lies outside"):
        v.SetOutline(crease_deg=100.0)                      # cos 100 is negative
    v.close()
    # folded by 20 degrees: no crease at 30, one at 10; t(px 7) = 7 < t(px 8): the line lies on px 7
    for flip in (False, True):                              # ... and the same with the right face wound the other way round: normals 160 degrees apart
        sc = folded_strip(0.0, float(np.tan(np.deg2rad(20.0))), flip)
        tab = scene_table(sc.pos, sc.tri)
        dot = float(tab["n"][0] @ tab["n"][2])
        assert abs(abs(dot) - np.cos(np.deg2rad(20.0))) < 1e-6 and (dot < 0) == flip
        v = View(0).load_scene(sc)
        got, _ = assert_device_equals_twin_and_numpy(v, tab)
        assert not got.any(), flip                          # the absolute value: a signed compare would draw the flipped one
        v.SetOutline(crease_deg=10.0)
        got, _ = assert_device_equals_twin_and_numpy(v, tab, f32(outline_crease_cos(10.0)))
        assert np.array_equal(got, column(7)), flip
        v.close()


GPU_SIZES = [(1, 1), (64, 8), (65, 9), (61, 37), (130, 3), (130, 67)]


def soup_scene():
    sc = scenes.baseline_config("C2", 61, 37, 2000)
    return dataclasses.replace(sc, tri_object=(np.arange(2000) % 5).astype(np.int32), obj_xform=np.tile(rigid(), (5, 1)))


def cad_scene():
    pos, nrm, tri, ob = scenes.gen_cad_like(3000, 1, 2, True)
    sc = scenes.baseline_config("C2", 61, 37, 16)
    from cadrays_amd.materials import BSDF
    return dataclasses.replace(sc, pos=pos, nrm=nrm, tri=tri, materials=[BSDF.CreateDiffuse(0.8)] * 3, tri_object=ob, obj_xform=np.tile(rigid(), (int(ob.max()) + 1, 1)))


SCENES = {"soup_5_objects": soup_scene, "cad_like": cad_scene, "no_objects": lambda: scenes.cornell_box(True, 61, 37), "all_miss": lambda: scenes.cornell_box(True, 61, 37)}


@pytest.mark.gpu
@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
@pytest.mark.parametrize("which", list(SCENES))
def test_device_equals_twin_and_numpy_over_scenes_sizes_and_cameras(hip_lib, which, ortho):
    from cadrays_amd.view import View
    sc = SCENES[which]()
    cam = dataclasses.replace(sc.camera, is_ortho=ortho, ortho_scale=1.1)
    if which == "all_miss":
        cam = dataclasses.replace(cam, eye=(0.0, -30.0, 0.0), dir=(0.0, -1.0, 0.0))
    sc = dataclasses.replace(sc, camera=cam)
    v = View(0).load_scene(sc)
    tab = scene_table(sc.pos, sc.tri)
    bits = 0
    for W, H in GPU_SIZES:
        v.set_params(dataclasses.replace(sc.params, width=W, height=H))
        got, (ob, tr, t) = assert_device_equals_twin_and_numpy(v, tab)
        assert got.shape == (H, W)
        bits |= int(np.bitwise_or.reduce(got, axis=None))
        if which == "all_miss":
            assert (ob < 0).all() and not got.any()
    if which == "soup_5_objects":
        assert bits == 7, bits                       # a soup shares no vertex: object, depth and crease lines
    elif which != "all_miss":
        assert bits & abi.OUTLINE_CREASE, bits
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"], ids=["one_walk", "two_passes"])
def test_mask_follows_the_states_of_a_live_scene(hip_lib, monkeypatch, split):
    from cadrays_amd.view import View, outline_crease_cos, outline_depth_ratio
    W, H = 61, 37
    monkeypatch.setenv("CRH_SPLIT_PASSES", split)
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    tab = scene_table(sc.pos, sc.tri)
    flat, _ = assert_device_equals_twin_and_numpy(v, tab)
    assert np.bitwise_or.reduce(flat, axis=None) & abi.OUTLINE_OBJECT and np.bitwise_or.reduce(flat, axis=None) & abi.OUTLINE_CREASE
    v.set_transforms(moved_xforms(7))
    assert v.get_tlas()["n_instances"] >= 1
    moved, _ = assert_device_equals_twin_and_numpy(v, tab)          # a moved object keeps its object-space normals: the same table
    assert not np.array_equal(moved, flat)
    v.set_visibility(visible_flags(7, [3]))
    erased, (ob, _, _) = assert_device_equals_twin_and_numpy(v, tab)
    assert not (ob == 3).any() and not np.array_equal(erased, moved)
    # a welded roof in front of everything, its ridge towards the camera: the two faces meet at 90 degrees
    p = np.array([(0.35, 0.25, 0.35), (0.5, 0.1, 0.35), (0.5, 0.1, 0.65), (0.35, 0.25, 0.65), (0.65, 0.25, 0.35), (0.65, 0.25, 0.65)], f32)
    n = np.tile(np.array([0, -1, 0], f32), (6, 1)); t = np.array([(0, 1, 2, 0), (0, 2, 3, 0), (1, 4, 5, 0), (1, 5, 2, 0)], np.int32)
    assert v.add_object(p, n, t, rigid()) == 7
    pos2 = np.concatenate([sc.pos, p]); tri2 = np.concatenate([sc.tri, t + np.array([len(sc.pos)] * 3 + [0], np.int32)])
    tab2 = scene_table(pos2, tri2)
    added, (ob, tr, _) = assert_device_equals_twin_and_numpy(v, tab2)      # the new rows appear in the table ...
    new = ob == 7
    assert new.any() and (tr[new] >= len(sc.tri)).all()
    _, mask_host, _ = _api()
    stale = mask_host(*v.read_ids(), tab)
    assert (added[new] & abi.OUTLINE_CREASE).any() and not (stale[new] & abi.OUTLINE_CREASE).any() and np.array_equal(stale & 1, added & 1)      # ... and carry the crease of the new object
    v.set_camera(dataclasses.replace(sc.camera, eye=(0.2, -3.2, 0.6), dir=(0.1, 1.0, -0.05)))
    turned, _ = assert_device_equals_twin_and_numpy(v, tab2)
    assert not np.array_equal(turned, added)
    v.set_params(dataclasses.replace(sc.params, width=130, height=67))
    resized, _ = assert_device_equals_twin_and_numpy(v, tab2)
    assert resized.shape == (67, 130)
    # thresholds: read_outline uses those in force, and all three bits whatever `kinds` draws
    v.SetOutline(kinds=abi.OUTLINE_OBJECT, crease_deg=70.0, depth_rel=0.5)
    strict, _ = assert_device_equals_twin_and_numpy(v, tab2, f32(outline_crease_cos(70.0)), f32(outline_depth_ratio(0.5)))
    assert not (strict & ~resized).any() and (strict & abi.OUTLINE_CREASE).any()
    v.ClearOutline()
    again, _ = assert_device_equals_twin_and_numpy(v, tab2)                # the defaults while the feature is off
    assert np.array_equal(again, resized)
    v.close()


def lines_over(v, plain, **params):
    """what read_ldr must return with the feature on: the numpy drawing rule over the bytes without lines"""
    p = dict(kinds=7, width=1, rgb=(0, 0, 0), alpha=255); p.update(params)
    return ref.draw(v.read_outline(), plain, p["kinds"], p["width"], p["rgb"], p["alpha"])


@pytest.mark.gpu
def test_read_ldr_draws_the_lines_over_the_tone_mapped_bytes(hip_lib):
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    for _ in range(3): v.Redraw()
    plain = v.read_ldr()
    assert v.get_outline()["on"] is False
    mask = v.read_outline()
    assert all((mask & k).any() for k in (1, 4))
    for width in (1, 2, 3):
        for kinds in (7, 1, 2, 4, 6, 0):
            for rgb, alpha in (((0, 0, 0), 255), ((255, 40, 0), 128), ((10, 200, 30), 1)):
                v.SetOutline(kinds=kinds, width=width, rgb=rgb, alpha=alpha)
                got, want = v.read_ldr(), ref.draw(mask, plain, kinds, width, rgb, alpha)
                assert np.array_equal(got, want), (width, kinds, rgb, alpha, np.argwhere(got != want)[:4])
                if kinds == 0:
                    assert np.array_equal(got, plain)
    assert not np.array_equal(ref.draw(mask, plain, 7, 1), plain) and not np.array_equal(ref.draw(mask, plain, 7, 3), ref.draw(mask, plain, 7, 2))
    g = v.get_outline()
    assert g["on"] and (g["kinds"], g["width"], g["rgb"], g["alpha"]) == (0, 3, (10, 200, 30), 1)
    # selection and hover come after the lines: a pixel that is both line and selection outline takes the selection's colour
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    v.SetOutline(width=2, rgb=(0, 0, 255))
    v.set_selection(flags, (255, 0, 0), 128); v.set_hover(4, (0, 255, 0), 64)
    ob = v.read_ids()[0]
    got = v.read_ldr()
    want = overlay_restated(ref.draw(mask, plain, 7, 2, (0, 0, 255)), ob, flags, (255, 0, 0), 128, 4, (0, 255, 0), 64)
    assert np.array_equal(got, want)
    line = ref.draw(mask, np.zeros_like(plain), 7, 2, (1, 1, 1))[..., 0] == 1
    both = line & (got == np.array([255, 0, 0], np.uint8)).all(-1) & np.isin(ob, [3, 5])
    assert both.sum() > 10
    v.set_selection(None); v.set_hover(-1)
    # auto exposure changes the bytes under the lines, not the lines
    v.set_auto_exposure(True)
    v.ClearOutline(); metered = v.read_ldr()
    v.SetOutline(width=1)
    assert not np.array_equal(metered, plain) and np.array_equal(v.read_ldr(), ref.draw(mask, metered, 7, 1))
    v.close()


@pytest.mark.gpu
def test_two_read_backs_in_flight_each_show_the_lines_of_their_camera(hip_lib):
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = object_scene(None, W, H)
    cam2 = dataclasses.replace(sc.camera, eye=(0.2, -3.2, 0.6), dir=(0.1, 1.0, -0.05))
    out = {}
    for lines in (False, True):
        v = View(0).load_scene(sc)
        if lines: v.SetOutline(width=2, rgb=(255, 255, 0), alpha=200)
        for _ in range(2): v.Redraw()
        if lines: out["mask1"] = v.read_outline()
        v.read_ldr_begin()
        v.set_camera(cam2); v.reset()
        v.Redraw()
        v.read_ldr_begin()
        out[lines] = (v.read_ldr_end(), v.read_ldr_end())
        if lines: out["mask2"] = v.read_outline()
        v.close()
    assert not np.array_equal(out["mask1"], out["mask2"]) and not np.array_equal(out[False][0], out[False][1])
    for k, m in ((0, out["mask1"]), (1, out["mask2"])):
        want = ref.draw(m, out[False][k], 7, 2, (255, 255, 0), 200)
        assert np.array_equal(out[True][k], want), (k, np.argwhere(out[True][k] != want)[:4])


@pytest.mark.gpu
def test_the_lines_leave_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 128, 96
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    ref_v = View(0).load_scene(sc)
    ref_v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(3): ref_v.Redraw()
    ldr3 = ref_v.read_ldr()
    for _ in range(5): ref_v.Redraw()
    want, (want_acc, want_frames), want_stats, want_ldr = ref_v.read_hdr(), ref_v.save_accum(), ref_v.stats(), ref_v.read_ldr()
    # the feature set before the scene exists, read-outs with lines between blocks of frames, an asynchronous one in flight across a change of the parameters
    v = View(0)
    v.SetOutline(width=3)
    v.load_scene(sc)
    v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(3): v.Redraw()
    v.read_ldr_begin()
    mask = v.read_outline()
    v.SetOutline(width=1, crease_deg=50.0)
    lined3 = v.read_ldr_end()
    ob = v.read_ids()[0]
    drawn = ref.draw(mask, np.zeros_like(ldr3), 7, 3, (1, 1, 1))[..., 0] == 1      # the read-back shows the lines as they were set when it began: 3 wide
    assert np.array_equal(lined3[~drawn], ldr3[~drawn]) and not lined3[drawn & ~np.isin(ob, [3, 5])].any() and drawn.sum() > 100
    for _ in range(5): v.Redraw()
    v.read_ldr(); v.read_outline()
    acc, frames = v.save_accum()
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and frames == want_frames == 8
    assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32))
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    assert np.array_equal(v.read_ids()[0], ob)                     # the id buffer is what it was
    v.ClearOutline()
    assert np.array_equal(v.read_ldr(), want_ldr)                  # the selection still drawn, and the bytes of a context that never called crh_set_outline
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32))
    v.close()
    # in a free-running loop, three frames in flight, a read-back with lines in flight
    v = View(0).load_scene(sc); v.set_pipeline_depth(3)
    v.set_selection(flags, (255, 0, 0), 128)
    v.SetOutline()
    for k in range(8):
        v.Redraw()
        if k in (2, 5):
            v.read_ldr_begin(); v.read_outline(); v.read_ldr_end()
        elif k == 3:
            v.SetOutline(kinds=abi.OUTLINE_CREASE, depth_rel=0.1)
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and v.save_accum()[1] == 8
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    v.ClearOutline()
    assert np.array_equal(v.read_ldr(), want_ldr)
    v.close(); ref_v.close()


@pytest.mark.gpu
def test_set_outline_refusals_and_state(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    d = v.get_outline()
    assert d["on"] is False and (d["kinds"], d["width"], d["rgb"], d["alpha"]) == (7, 1, (0, 0, 0), 255) and d["crease_cos"] == ref.DEFAULT_COS and d["depth_ratio"] == ref.DEFAULT_RATIO
    for bad, why in ((dict(kinds=8), "unknown bits in kinds"), (dict(kinds=0xFFFFFFFF), "unknown bits in kinds"), (dict(width=0), "width lies outside 1..3"),
                     (dict(width=4), "width lies outside 1..3"), (dict(crease_cos=0.0), "crease_cos lies outside"), (dict(crease_cos=-0.2), "crease_cos lies outside"),
                     (dict(crease_cos=1.001), "crease_cos lies outside"), (dict(depth_ratio=0.99), "depth_ratio is below 1"), (dict(depth_ratio=-3.0), "depth_ratio is below 1"),
                     (dict(crease_cos=float("nan")), "crease_cos / depth_ratio hold a NaN / Inf"), (dict(crease_cos=float("inf")), "hold a NaN / Inf"), (dict(depth_ratio=float("nan")), "hold a NaN / Inf"),
                     (dict(depth_ratio=float("inf")), "hold a NaN / Inf")):
        with pytest.raises(BackendError, match=f"-> -1: crh_set_outline: .*{why}"):
            v.set_outline(True, **bad)
        assert v.get_outline()["on"] is False                      # a refused call changes nothing
    v.set_outline(True, kinds=5, crease_cos=1.0, depth_ratio=1.0, width=3, rgb=(1, 2, 3), alpha=0)      # the limits themselves; allowed before crh_build
    g = v.get_outline()
    assert g["on"] and (g["kinds"], g["width"], g["rgb"], g["alpha"], float(g["crease_cos"]), float(g["depth_ratio"])) == (5, 3, (1, 2, 3), 0, 1.0, 1.0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4.*crh_build has not been called"):
        v.read_outline()
    assert v._fn("read_outline")(v._ctx, None) == abi.E_INVALID
    v.load_scene(sc)
    assert v.get_outline()["on"]                                   # display state outlives a new scene
    tab = scene_table(sc.pos, sc.tri)
    assert_device_equals_twin_and_numpy(v, tab, f32(1.0), f32(1.0))
    v.close()
