"""The first-hit id buffer: pick, hover, autofocus, selection bounds (crh_pick.cpp, cadrays_amd/csrc/k_ids.h).

Reference: AIS_InteractiveContext::MoveTo on every mouse move (src/Launcher/AppViewer.cxx:347), Select / ShiftSelect on a click (:359-455), autofocus
(src/Launcher/AppGui.cxx:78-94), the manipulator's pivot = the bounding box of the selection (AppViewer.cxx:863-875).  Here all of them read one derived buffer:
the first hit of the pixel-centre primary ray of every pixel.

  * the rays against a float64 restatement of the three camera models;
  * the ids against the CPU checker's trace_nearest on those very rays, bit for bit -- flat, split (two passes), split (one walk), erased, added;
  * the object per pixel against a float64 brute force that shares no code with either tree (oracle/brute_force.c);
  * invalidation; nothing else moves (HDR bits, sample counts); selection bounds; the View vocabulary; argument errors.

Bounds ("pixel-centre rays"): RAY_ANGLE_BOUND / RAY_OFFSET_BOUND are twice the worst error of a float32 restatement of the same operations
against float64 (test_ray_bounds_are_twice_the_float32_restatement below measures it on the CPU and asserts the factor), and no more than a few ulp of a unit vector.
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import one_object, visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = 2.0 ** -23                      # ulp of a float32 in [1, 2): the unit of a unit vector's component error
RAY_ANGLE_BOUND = 3.06e-7              # radians between the library's direction and the float64 one: 2 x 1.53e-7 (1.28 ulp), the float32 restatement's worst case
RAY_OFFSET_BOUND = 1.6e-7              # orthographic origins: |o - o64| relative to |eye|_inf + ortho_scale * max(aspect, 1): 2 x 7.93e-8 (0.67 ulp), likewise
EPS24 = 2.0 ** -24                     # one rounding of a float32 result, relative

OFF_AXIS = scenes.Camera(eye=(0.31, -2.9, 0.73), dir=(0.21, 1.0, -0.16), up=(0.05, 0.0, 1.0), fovy_deg=37.0)


# ------------------------------------------------------------------------------------------------ restatement of the camera models
def _norm(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def restated_rays(cam, W, H, xy, bilinear=0, T=np.float64):
    """pixel-centre rays of crh_render's camera models, every operation carried out in precision T (float64: the reference; float32: the error model)"""
    f = lambda x: np.asarray(x, T)
    eye, fwd = f(cam.eye), _norm(f(cam.dir))
    right = _norm(np.cross(fwd, f(cam.up)).astype(T))
    up = np.cross(right, fwd).astype(T)
    tan_half = f(np.tan(f(cam.fovy_deg) * f(0.5) * f(np.pi / 180.0)))
    aspect = f(cam.aspect) if cam.aspect > 0 else f(W) / f(H)
    px, py = f(xy[:, 0]), f(xy[:, 1])
    half = f(0.5)
    u, v1 = (px + half) / f(W), (py + half) / f(H)
    nx, ny = u * f(2) - f(1), v1 * f(-2) + f(1)
    if cam.is_ortho:
        s = f(cam.ortho_scale)
        o = eye + right * ((nx * s) * aspect)[:, None] + up * (ny * s)[:, None]
        d = np.broadcast_to(fwd, o.shape)
    elif bilinear:
        def corner(sx, sy):
            c = fwd + right * ((f(sx) * tan_half) * aspect) + up * (f(sy) * tan_half)
            return _norm(c) if bilinear == 2 else c
        lb, rb, lt, rt = corner(-1, -1), corner(1, -1), corner(-1, 1), corner(1, 1)
        v = f(1) - v1
        bot, top = lb + (rb - lb) * u[:, None], lt + (rt - lt) * u[:, None]
        d = _norm(bot + (top - bot) * v[:, None])
        o = np.broadcast_to(eye, d.shape)
    else:
        d = _norm(fwd + right * ((nx * tan_half) * aspect)[:, None] + up * (ny * tan_half)[:, None])
        o = np.broadcast_to(eye, d.shape)
    return np.array(o, T), np.array(d, T)


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(np.cross(a, b), axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def all_pixels(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32)


CAMERA_CASES = [("pinhole", OFF_AXIS, 0), ("ortho", dataclasses.replace(OFF_AXIS, is_ortho=True, ortho_scale=1.7), 0),
                ("bilinear", OFF_AXIS, 1), ("bilinear_unit", OFF_AXIS, 2)]
TARGETS = [(61, 37, None), (1920, 1080, np.array([(0, 0), (1919, 0), (0, 1079), (1919, 1079), (960, 540), (959, 539), (1, 1078)], np.uint32))]


def offset_scale(cam, W, H):
    return np.abs(np.asarray(cam.eye, np.float64)).max() + cam.ortho_scale * max(W / H, 1.0)


def test_ray_bounds_are_twice_the_float32_restatement():
    """the bounds of the GPU test come from the precision of float32, not from what the kernel gives: worst error of a float32 restatement x 2 <= bound <= 4 ulp"""
    worst_a = worst_o = 0.0
    for _, cam, bil in CAMERA_CASES:
        for W, H, xy in TARGETS:
            xy = all_pixels(W, H) if xy is None else xy
            o64, d64 = restated_rays(cam, W, H, xy, bil)
            o32, d32 = restated_rays(cam, W, H, xy, bil, np.float32)
            worst_a = max(worst_a, float(angle(d32, d64).max()))
            worst_o = max(worst_o, float(np.abs(o32.astype(np.float64) - o64).max() / offset_scale(cam, W, H)))
    print(f"float32 restatement: worst angle {worst_a:.3e} rad = {worst_a / ULP1:.2f} ulp, worst ortho offset {worst_o:.3e} = {worst_o / ULP1:.2f} ulp (relative)")
    assert 2.0 * worst_a <= RAY_ANGLE_BOUND <= 2.02 * worst_a and 2.0 * worst_o <= RAY_OFFSET_BOUND <= 2.02 * worst_o      # twice the measured worst case, no more
    assert RAY_ANGLE_BOUND <= 4.0 * ULP1 and RAY_OFFSET_BOUND <= 4.0 * ULP1


def test_pick_result_layout_matches_header(tmp_path):
    """sizeof / offsetof of crh_pick_result as gcc sees include/cadrays_hip.h == the ctypes mirror; every new entry point is declared and listed"""
    fields = [n for n, _ in abi.crh_pick_result._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(crh_pick_result));' + "".join(
        f'printf("%zu ", offsetof(crh_pick_result, {n}));' for n in fields) + "return 0;}"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [C.sizeof(abi.crh_pick_result)] + [getattr(abi.crh_pick_result, n).offset for n in fields], got
    assert C.sizeof(abi.crh_pick_result) == 36
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in ("crh_camera_rays", "crh_pick", "crh_read_ids", "crh_set_selection", "crh_set_hover", "crh_get_selection_bounds"):
        assert name in abi.EXPORTS and f"CRH_API int {name}(" in header, name


# ------------------------------------------------------------------------------------------------ GPU: rays
@pytest.mark.gpu
@pytest.mark.parametrize("name,cam,bilinear", CAMERA_CASES, ids=[c[0] for c in CAMERA_CASES])
def test_camera_rays_against_float64(hip_lib, name, cam, bilinear):
    from cadrays_amd.view import View
    for W, H, xy in TARGETS:
        sc = scenes.cornell_box(False, W, H)
        sc = dataclasses.replace(sc, camera=cam, spec=dict(raygen_bilinear=bilinear) if bilinear else None)
        v = View(0).load_scene(sc)
        xy = all_pixels(W, H) if xy is None else xy
        rays = v.camera_rays(xy)
        o64, d64 = restated_rays(cam, W, H, xy, bilinear)
        assert np.all(rays[:, 3] == np.float32(1e15)) and np.all(rays[:, 7] == 0)
        a = float(angle(rays[:, 4:7], d64).max())
        off = float(np.abs(rays[:, :3].astype(np.float64) - o64).max() / offset_scale(cam, W, H))
        print(f"{name} {W}x{H}: worst angle {a:.3e} rad ({a / ULP1:.2f} ulp), worst origin offset {off:.3e} ({off / ULP1:.2f} ulp)")
        if not cam.is_ortho:
            assert np.array_equal(rays[:, :3], np.broadcast_to(np.asarray(cam.eye, np.float32), (len(xy), 3)))      # exact
        else:
            assert off <= RAY_OFFSET_BOUND
        assert a <= RAY_ANGLE_BOUND
        assert np.abs(np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1) - 1.0).max() <= 2.0 * ULP1
        v.close()


# ------------------------------------------------------------------------------------------------ GPU: the ids are the tree's answer
def tetra_scene(w, h):
    """Cornell room (object 27) + 27 small tetrahedra, one object each (the scene of test_two_level's one-walk test)"""
    r = np.random.default_rng(5)
    base = scenes.cornell_box(True, w, h)
    P, N, T = [], [], []
    for k in range(27):
        c = np.array([0.2 + 0.3 * (k % 3), 0.2 + 0.3 * ((k // 3) % 3), 0.2 + 0.3 * (k // 9)], np.float32)
        q = (c + 0.06 * r.normal(size=(4, 3))).astype(np.float32)
        for f in ((0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)):
            i0 = len(P)
            nrm = np.cross(q[f[1]] - q[f[0]], q[f[2]] - q[f[0]]); nrm = (nrm / np.linalg.norm(nrm)).astype(np.float32)
            P += [q[f[0]], q[f[1]], q[f[2]]]; N += [nrm] * 3; T.append((i0, i0 + 1, i0 + 2, k % len(base.materials), k))
    nV = len(base.pos)
    pos = np.concatenate([base.pos, np.array(P, np.float32)]); nrm = np.concatenate([base.nrm, np.array(N, np.float32)])
    tri = np.concatenate([base.tri, np.array([(a + nV, b + nV, c_ + nV, m) for a, b, c_, m, _ in T], np.int32)])
    tri_obj = np.concatenate([np.full(len(base.tri), 27, np.int32), np.array([t[4] for t in T], np.int32)])
    return dataclasses.replace(base, pos=pos, nrm=nrm, tri=tri, tri_object=tri_obj, obj_xform=np.tile(rigid(), (28, 1)), uv=None)


def two_moved(n):
    xf = np.tile(rigid(), (n, 1)); m = moved_xforms(n)
    xf[3], xf[5] = m[3], m[5]
    return xf


def many_moved(n=28, k=14):
    r = np.random.default_rng(6)
    xf = np.tile(rigid(), (n, 1))
    for i in r.permutation(27)[:k]:
        xf[i] = rigid(float(r.uniform(0, 60)), (0, 0, 1), tuple(0.05 * r.normal(size=3)))
    return xf


def _case(name, w, h):
    """(scene, function applied to BOTH backends after load_scene, tri_object as the backends know it afterwards)"""
    if name == "cornell":
        return scenes.cornell_box(True, w, h), (lambda b: None), None
    if name == "many_moved":
        sc = tetra_scene(w, h)
        return sc, (lambda b: b.set_transforms(many_moved())), sc.tri_object
    sc = object_scene(None, w, h)
    if name == "flat":
        return sc, (lambda b: None), sc.tri_object
    if name == "two_moved":
        return sc, (lambda b: b.set_transforms(two_moved(7))), sc.tri_object
    if name == "erased":
        return sc, (lambda b: b.set_visibility(visible_flags(7, [4]))), sc.tri_object
    if name == "added":
        p, n, t = one_object(sc, 3)
        xf = rigid(30.0, (0, 0, 1), (0.1, -0.3, 0.35))
        return sc, (lambda b: b.add_object(p, n, t, xf)), np.concatenate([sc.tri_object, np.full(len(t), 7, np.int32)])
    raise KeyError(name)


ID_CASES = ["cornell", "flat", "two_moved", "many_moved", "erased", "added"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(61, 37), (1920, 1080)], ids=["61x37", "1920x1080"])
@pytest.mark.parametrize("name", ID_CASES)
def test_ids_equal_the_checkers_trace_of_the_same_rays(hip_lib, oracle_lib, name, size):
    from cadrays_amd.view import View
    W, H = size
    sc, change, tri_object = _case(name, W, H)
    v = View(0).load_scene(sc); o = oracle_lib.Oracle().load_scene(sc)
    change(v); change(o)
    if name == "two_moved": assert v.get_tlas()["n_instances"] == 2
    if name == "many_moved": assert v.get_tlas()["n_instances"] == 14
    xy = all_pixels(W, H)
    rays = v.camera_rays(xy)
    ref = o.trace_nearest(rays)                                   # {t, u, v, prim}: prim is the caller's triangle index on both sides (no mapping needed)
    ob, tr, t = v.read_ids()
    ref_tri = ref[:, 3].view(np.int32).reshape(H, W)
    assert np.array_equal(tr, ref_tri)
    assert np.array_equal(t.view(np.uint32), ref[:, 0].view(np.uint32).reshape(H, W))
    want_ob = np.where(ref_tri < 0, -1, 0 if tri_object is None else tri_object[np.maximum(ref_tri, 0)])
    assert np.array_equal(ob, want_ob)
    assert (ob >= 0).mean() > 0.3                                 # the camera looks into the room
    assert np.array_equal(v.trace_nearest(rays).view(np.uint32), ref.view(np.uint32))      # ... and crh_trace_nearest says the same of these rays
    # crh_pick == the buffer, point and depth against float64
    r = np.random.default_rng(11)
    px, py = r.integers(0, W, 300), r.integers(0, H, 300)
    cam = sc.camera
    fwd64 = _norm(np.asarray(cam.dir, np.float64)); eye64 = np.asarray(cam.eye, np.float64)
    for x, y in zip(px, py):
        p = v.pick(int(x), int(y)); i = int(y) * W + int(x)
        assert (p["object"], p["triangle"]) == (int(ob[y, x]), int(tr[y, x]))
        assert np.float32(p["t"]).view(np.uint32) == t[y, x].view(np.uint32)
        if p["object"] < 0:
            continue
        assert np.float32(p["u"]).view(np.uint32) == ref[i, 1].view(np.uint32) and np.float32(p["v"]).view(np.uint32) == ref[i, 2].view(np.uint32)
        o64, d64, t64 = rays[i, :3].astype(np.float64), rays[i, 4:7].astype(np.float64), float(t[y, x])
        p64 = o64 + t64 * d64
        # point: one fused multiply-add per component = one rounding of the result; the bound is twice that
        assert np.all(np.abs(np.asarray(p["point"], np.float64) - p64) <= 2.0 * EPS24 * (np.abs(o64) + np.abs(t64 * d64)) + 1e-30)
        # depth = dot(point - eye, fwd) in float32: the point's rounding (1), the subtraction (1), the dot product (3), the unit view direction (norm of the
        # caller's vector: ~3) -- 8 roundings of size 2^-24 |point - eye| in the worst case; the bound is twice that
        dist = np.linalg.norm(p64 - eye64)
        assert abs(p["depth"] - float(np.dot(p64 - eye64, fwd64))) <= 16.0 * EPS24 * dist
    v.close()


# ------------------------------------------------------------------------------------------------ GPU: geometric truth, independent of the tree
@pytest.mark.gpu
def test_object_per_pixel_against_float64_brute_force(hip_lib):
    from cadrays_amd.view import View
    from test_geometric_truth import brute_f64
    W, H = 160, 120
    sc = tetra_scene(W, H)                                        # 1954 + 108 triangles, 28 objects
    xf = many_moved()
    v = View(0).load_scene(sc); v.set_transforms(xf)
    rays = v.camera_rays(all_pixels(W, H))
    ob = v.read_ids()[0].ravel()
    # world-space triangles in float64 from the float32 inputs, per object; nearest hit per object by exhaustive double-precision tests
    n = W * H
    t_obj = np.full((28, n), np.inf); margin = np.zeros((28, n))
    for k in range(28):
        M = xf[k].reshape(3, 4).astype(np.float64)
        tri = sc.tri[sc.tri_object == k][:, :3]
        wp = (sc.pos[tri].astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(np.float32)
        tuv, idx, mg = brute_f64(np.ascontiguousarray(wp), rays)
        hit = idx >= 0
        t_obj[k, hit] = tuv[hit, 0]; margin[k] = mg
    order = np.argsort(t_obj, axis=0)
    first, second = order[0], order[1]
    t1, t2 = t_obj[first, np.arange(n)], t_obj[second, np.arange(n)]
    truth = np.where(np.isfinite(t1), first, -1)
    with np.errstate(invalid="ignore"):                          # inf - inf where no second object lies on the ray
        near_tie = np.isfinite(t2) & ((t2 - t1) <= 1e-5 * np.maximum(t1, 1e-30))
    near_edge = np.isfinite(t1) & (np.abs(margin[first, np.arange(n)]) <= 1e-5)
    excluded = near_tie | near_edge
    share = float(excluded.mean())
    wrong = (ob != truth) & ~excluded
    print(f"brute force: {n} pixels, excluded {excluded.sum()} ({100 * share:.2f} %), differing among the excluded {int(((ob != truth) & excluded).sum())}, wrong {int(wrong.sum())}")
    assert share <= 0.02
    assert not wrong.any(), np.flatnonzero(wrong)[:10]
    assert len(np.unique(ob)) > 15                                # most objects are on screen
    v.close()


# ------------------------------------------------------------------------------------------------ GPU: invalidation
@pytest.mark.gpu
def test_the_buffer_follows_transforms_visibility_camera_size_and_added_objects(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 96, 96)
    v = View(0).load_scene(sc)
    ob0, tr0, t0 = v.read_ids()
    ys, xs = np.nonzero(ob0 == 3)
    assert len(ys) > 50
    y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    assert v.pick(x, y)["object"] == 3
    # move object 3 up and sideways: the old pixel shows what was behind it, the object is picked where it is drawn
    xf = np.tile(rigid(), (7, 1)); xf[3] = rigid(0.0, (0, 0, 1), (0.3, 0.0, 0.35))
    v.set_transforms(xf)
    p = v.pick(x, y)
    ob1 = v.read_ids()[0]
    assert p["object"] != 3 and p["object"] >= 0 and p["t"] > t0[y, x]
    ys1, xs1 = np.nonzero(ob1 == 3)
    assert len(ys1) > 50 and xs1.mean() > xs.mean() + 5 and ys1.mean() < ys.mean() - 5      # +x is right, +z is up (row 0 = top)
    y1, x1 = int(ys1[0]), int(xs1[0])
    assert v.pick(x1, y1)["object"] == 3
    v.set_transforms(np.tile(rigid(), (7, 1)))
    back = v.read_ids()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(back, (ob0, tr0, t0)))      # the static tree's records restored
    # erase / display
    v.set_visibility(visible_flags(7, [3]))
    ob2, _, t2 = v.read_ids()
    assert not (ob2 == 3).any() and v.pick(x, y)["object"] != 3 and t2[y, x] > t0[y, x]
    v.set_visibility(np.ones(7, np.uint8))
    assert np.array_equal(v.read_ids()[0], ob0)
    # camera (crh_set_camera alone, without a restart) and target size: the buffer of a fresh context in that state
    cam = dataclasses.replace(sc.camera, eye=(0.2, -3.2, 0.6), dir=(0.1, 1.0, -0.05))
    v.set_camera(cam)
    f = View(0).load_scene(dataclasses.replace(sc, camera=cam))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(v.read_ids(), f.read_ids()))
    assert not np.array_equal(v.read_ids()[0], ob0)
    v.ChangeRenderingParams(width=83, height=57); f.ChangeRenderingParams(width=83, height=57)
    a, b = v.read_ids(), f.read_ids()
    assert a[0].shape == (57, 83) and all(np.array_equal(p_.view(np.uint32), q_.view(np.uint32)) for p_, q_ in zip(a, b))
    with pytest.raises(BackendError):
        v.pick(83, 0)
    # add-object: the new object is pickable at once
    pp, nn, tt = one_object(sc, 3)
    new = v.add_object(pp, nn, tt, rigid(0.0, (0, 0, 1), (-0.2, -0.3, 0.4)))
    ob3, tr3, _ = v.read_ids()
    assert new == 7 and (ob3 == 7).sum() > 30
    assert tr3[ob3 == 7].min() >= len(sc.tri) and tr3[ob3 == 7].max() < len(sc.tri) + len(tt)      # rows of crh_add_object follow those of crh_set_geometry
    yy, xx = np.nonzero(ob3 == 7)
    assert v.pick(int(xx[0]), int(yy[0]))["object"] == 7
    v.close(); f.close()


# ------------------------------------------------------------------------------------------------ GPU: nothing else moves
def _interrupt(v, W, H):
    p = v.pick(W // 2, H // 2)
    ids = v.read_ids()
    flags = np.zeros(v._n_objects, np.uint8); flags[max(p["object"], 0)] = 1
    v.set_selection(flags, (255, 0, 0), 128)
    v.set_hover(max(p["object"], 0), (0, 255, 0), 0)
    return ids


@pytest.mark.gpu
def test_picking_and_selecting_leave_the_accumulation_alone(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 128, 96)
    ref = View(0).load_scene(sc)
    for _ in range(8): ref.Redraw()
    want, want_s = ref.read_hdr(), ref.stats()["samples"]
    plain_ldr = ref.read_ldr()
    # between two blocks of frames
    v = View(0).load_scene(sc)
    for _ in range(4): v.Redraw()
    _interrupt(v, 128, 96)
    for _ in range(4): v.Redraw()
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and v.stats()["samples"] == want_s
    assert not np.array_equal(v.read_ldr(), plain_ldr)            # the overlay is in the LDR read-out ...
    v.set_selection(None); v.set_hover(-1)
    assert np.array_equal(v.read_ldr(), plain_ldr)                # ... and gone without a trace: the bytes of a context that never had a selection
    v.close()
    # in a free-running loop, three frames in flight, an asynchronous read-back in flight around every pick
    v = View(0).load_scene(sc); v.set_pipeline_depth(3)
    for k in range(8):
        v.Redraw()
        if k in (2, 5):
            v.read_ldr_begin()
            _interrupt(v, 128, 96)
            v.read_ldr_end()
        elif k == 3:
            v.pick(5, 7); v.set_hover(-1)
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and v.stats()["samples"] == want_s
    v.close(); ref.close()


# ------------------------------------------------------------------------------------------------ GPU: selection bounds
@pytest.mark.gpu
def test_selection_bounds_against_float64(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 64)
    v = View(0).load_scene(sc)
    with pytest.raises(BackendError):
        v.selection_bounds()                                      # nothing selected
    xf = moved_xforms(7)
    v.set_transforms(xf)
    for chosen in ([3], [5, 6], [0, 3, 4]):
        flags = np.zeros(7, np.uint8); flags[chosen] = 1
        v.set_selection(flags)
        lo, hi = v.selection_bounds()
        lo64, hi64, wid = np.full(3, np.inf), np.full(3, -np.inf), np.zeros(3)
        for k in chosen:
            M = xf[k].reshape(3, 4).astype(np.float64)
            p = sc.pos[np.unique(sc.tri[sc.tri_object == k][:, :3])].astype(np.float64)
            q = p @ M[:, :3].T + M[:, 3]
            w = 4.0 * EPS24 * (np.abs(p) @ np.abs(M[:, :3]).T + np.abs(M[:, 3]))      # three fused multiply-adds and a rounding per coordinate
            assert np.all(q >= lo - w) and np.all(q <= hi + w)                      # every transformed vertex inside the widened box
            lo64, hi64, wid = np.minimum(lo64, q.min(0)), np.maximum(hi64, q.max(0)), np.maximum(wid, w.max(0))
        assert np.all(lo >= lo64 - wid) and np.all(hi <= hi64 + wid)                # ... and the box no larger than the float64 one, widened alike
    v.set_selection(None)
    with pytest.raises(BackendError):
        v.selection_bounds()
    # a scene handed over without objects is one object
    w = View(0).load_scene(scenes.cornell_box(True, 64, 64))
    w.set_selection([1])
    lo, hi = w.selection_bounds()
    pos = scenes.cornell_box(True, 64, 64).pos
    assert np.array_equal(lo, pos.min(0)) and np.array_equal(hi, pos.max(0))
    v.close(); w.close()


# ------------------------------------------------------------------------------------------------ GPU: the View vocabulary, argument errors
@pytest.mark.gpu
def test_view_moveto_select_hide_autofocus(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 96, 96)
    v = View(0).load_scene(sc)
    ob = v.read_ids()[0]
    where = {k: (int(np.nonzero(ob == k)[1][0]), int(np.nonzero(ob == k)[0][0])) for k in (3, 4, 5)}
    plain = v.read_ldr()
    assert v.MoveTo(*where[3]) == 3
    assert not np.array_equal(v.read_ldr(), plain)
    assert v.Select(*where[4]) == {4}
    assert v.Select(*where[5], shift=True) == {4, 5}
    assert v.Select(*where[4], shift=True) == {5}
    lo, hi = v.selection_bounds()
    p5 = sc.pos[np.unique(sc.tri[sc.tri_object == 5][:, :3])]
    assert np.array_equal(lo, p5.min(0)) and np.array_equal(hi, p5.max(0))          # identity transform: exact
    v.HideSelected()
    assert not (v.read_ids()[0] == 5).any() and v.Select(*where[4]) == {4}
    for _ in range(2): v.Redraw()
    r = v.pick(*where[3])
    assert v.autofocus(*where[3]) == pytest.approx(r["depth"]) and v._camera.focal_dist == pytest.approx(r["depth"])
    assert v.stats()["samples"] == 0                              # a camera change restarts the accumulation
    miss_cam = dataclasses.replace(sc.camera, dir=(0.0, -1.0, 0.0))
    v.set_camera(miss_cam); v.reset(); v.Redraw()
    assert v.pick(3, 3)["object"] == -1 and v.pick(3, 3)["triangle"] == -1
    assert v.autofocus(3, 3) is None and v.stats()["samples"] == 96 * 96          # a miss changes nothing
    assert v.MoveTo(3, 3) == -1 and v.Select(3, 3) == set()
    v.close()


@pytest.mark.gpu
def test_pick_argument_errors(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params)
    for call in (lambda: v.pick(1, 1), lambda: v.read_ids(), lambda: v.set_selection(np.ones(7)), lambda: v.set_hover(1), lambda: v.selection_bounds()):
        with pytest.raises(BackendError):
            call()                                                # not built
    v.load_scene(sc)
    for call in (lambda: v.pick(64, 0), lambda: v.pick(0, 48), lambda: v.camera_rays([(64, 1)]), lambda: v.set_selection(np.ones(6)), lambda: v.set_selection(np.ones(8)),
                 lambda: v.set_selection(np.ones(7), alpha=256), lambda: v.set_hover(7), lambda: v.set_hover(2, alpha=300)):
        with pytest.raises(BackendError):
            call()
    v.set_selection(np.ones(7)); v.set_hover(6); v.set_hover(-1); v.set_selection(None)
    # after crh_add_object the flags take one more entry; a new crh_set_geometry clears selection and hover
    p, n, t = one_object(sc, 3)
    v.add_object(p, n, t, rigid(0.0, (0, 0, 1), (0.0, -0.3, 0.4)))
    with pytest.raises(BackendError):
        v.set_selection(np.ones(7))
    v.set_selection(np.ones(8)); v.set_hover(7)
    plain_sc = scenes.cornell_box(True, 64, 48)
    v.load_scene(plain_sc)
    f = View(0).load_scene(plain_sc)
    assert np.array_equal(v.read_ldr(), f.read_ldr())
    with pytest.raises(BackendError):
        v.set_selection(np.ones(7))                               # one object now
    v.close(); f.close()
