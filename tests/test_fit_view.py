"""Fitting the view to the displayed or chosen objects (crh_fit.cpp, cadrays_amd/csrc/fit_kernels.hip).

Reference: V3d_View::FitAll / ZFitAll as the application drives them (src/Launcher/AppViewer.cxx:704, 764-767, 788, 886).

  CPU   crh_fit_extents_host == the float32 restatement (tests/fit_reference.py) bit for bit; crh_fit_from_extents == the float64 restatement bit for bit, every
        binding value reached; every refusal; the fitted camera against float64 geometry with a DERIVED bound (test_fitted_camera_against_float64); the ABI
  GPU   crh_fit_view == the host twin bit for bit at the sizes and object layouts where the kernel takes another path; on a live scene (moved, erased, added);
        end to end through the id buffer; nothing restarts; argument errors
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import fit_reference as ref
from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from cadrays_amd.view import fit_extents_host, fit_from_extents
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import one_object, visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24
OFF_AXIS = scenes.Camera(eye=(0.31, -2.9, 0.73), dir=(0.21, 1.0, -0.16), up=(0.05, 0.0, 1.0), fovy_deg=37.0)
ORTHO = dataclasses.replace(OFF_AXIS, is_ortho=True, ortho_scale=1.7)
AXIAL = scenes.Camera(eye=(0.0, 0.0, 0.0), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fovy_deg=40.0)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def random_xforms(n, seed):
    r = np.random.default_rng(seed)
    return np.stack([rigid(float(r.uniform(0, 360)), tuple(r.normal(size=3)), tuple(0.3 * r.normal(size=3)), float(r.uniform(0.5, 1.5))) for _ in range(n)])


def random_verts4(n, n_objects, seed, unreferenced=0.1):
    r = np.random.default_rng(seed)
    owner = r.integers(0, n_objects, n).astype(np.int32)
    owner[r.random(n) < unreferenced] = -1
    return np.concatenate([r.uniform(-1, 1, (n, 3)).astype(f32), owner.view(f32)[:, None]], 1)


def signed_zero_verts4():
    """object 0: every combination of +-0, +-1 (equal values many times over); object 1: of +-0 and -1, so that a zero decides its maxima"""
    out = []
    for o, vals in enumerate((np.array([0.0, -0.0, 1.0, -1.0, 1.0], f32), np.array([-0.0, 0.0, -1.0, -0.0], f32))):
        g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
        out.append(np.concatenate([g, np.full((len(g), 1), o, np.int32).view(f32)], 1))
    return np.concatenate(out), 2


def _object_scene_case(moved):
    sc = object_scene(moved_xforms(7) if moved else None, 96, 64)
    return ref.scene_verts4(sc.pos, sc.tri, sc.tri_object), 7, sc.obj_xform


EXTENT_CASES = {
    "random": lambda: (random_verts4(1000, 3, 1), 3, random_xforms(3, 2)),
    "random_no_xform": lambda: (random_verts4(333, 2, 3), 2, None),
    "object_scene": lambda: _object_scene_case(False),
    "object_scene_moved": lambda: _object_scene_case(True),
    "signed_zeros": lambda: (signed_zero_verts4()[0], 2, None),
    "signed_zeros_identity_rows": lambda: (signed_zero_verts4()[0], 2, np.tile(rigid(), (2, 1))),
}
CAMERAS = {"perspective": (OFF_AXIS, 96, 64), "ortho": (ORTHO, 96, 64), "axial": (AXIAL, 64, 64), "axial_ortho": (dataclasses.replace(AXIAL, is_ortho=True), 64, 64),
           "own_aspect": (dataclasses.replace(OFF_AXIS, aspect=1.7), 96, 64), "aspect_from_params": (dataclasses.replace(OFF_AXIS, aspect=-1.0), 61, 37),
           "tall": (dataclasses.replace(OFF_AXIS, aspect=0.4), 40, 100), "tall_ortho": (dataclasses.replace(ORTHO, aspect=0.4), 40, 100)}


# ------------------------------------------------------------------------------------------------ CPU: the extents
@pytest.mark.parametrize("cam_name", list(CAMERAS))
@pytest.mark.parametrize("case", list(EXTENT_CASES))
def test_extents_host_equals_the_float32_restatement(hip_lib, case, cam_name):
    v4, nO, xf = EXTENT_CASES[case]()
    cam, W, H = CAMERAS[cam_name]
    for margin in (0.01, 0.125):
        F = ref.frame32(cam, W, H, margin)
        ext, cnt, fr = fit_extents_host(v4, nO, cam, W, H, margin, xf)
        for n in ("right", "up", "fwd", "kx", "ky"):
            assert same_bits(fr[n], F[n]), (n, fr[n], F[n])
        want, want_n, _ = ref.extents32(v4, nO, xf, F)
        assert np.array_equal(cnt, want_n)
        assert same_bits(ext, want), np.argwhere(bits(ext) != bits(want))[:5]
    if cam.is_ortho:
        assert F["kx"] == 0 and F["ky"] == 0
    if case.startswith("signed_zeros") and cam_name == "axial_ortho":
        assert bits(ext)[1, 0] == 0 and bits(ext)[1, 5] == 0                  # object 1: max(x) and max(z) over {-1, -0.0, +0.0} are +0.0, not -0.0


def test_key_orders_negative_zero_below_positive_zero():
    k = ref.key(np.array([-0.0, 0.0, -1.0, 1.0, -np.inf], f32))
    assert k[0] < k[1] and k[2] < k[0] and k[1] < k[3] and k[4] > 0
    assert same_bits(ref.unkey(k), np.array([-0.0, 0.0, -1.0, 1.0, -np.inf], f32))
    # the same bits whatever the order of arrival.  A sum of products is -0.0 only when every term is, so x of a vertex on the axis is +0.0 (the identity's
    # 0 * v terms are +0.0) and -x - z * 0 is -0.0: the second maximum is -0.0, not the +0.0 a float comparison might equally leave
    for order in ([0.0, -0.0], [-0.0, 0.0]):
        v4 = np.zeros((2, 4), f32); v4[:, 1] = 1.0; v4[:, 0] = order      # x = +-0 at depth 1, orthographic: the first value is x itself
        ext, _, _ = fit_extents_host(v4, 1, dataclasses.replace(AXIAL, is_ortho=True), 64, 64, 0.0)
        assert bits(ext)[0, 0] == 0 and bits(ext)[0, 1] == 0x80000000


# ------------------------------------------------------------------------------------------------ CPU: the rule
def _check_rule(e, cam, W, H, margin):
    F = ref.frame32(cam, W, H, margin)
    want = ref.rule64(e, F, cam.is_ortho, margin)
    if want is None:
        with pytest.raises(BackendError):
            fit_from_extents(e, cam, W, H, margin)
        return None
    got, r = fit_from_extents(e, cam, W, H, margin)
    assert same_bits(got["eye"], want["eye"]), (got["eye"], want["eye"])
    assert same_bits(r["z_near"], want["z_near"]) and same_bits(r["z_far"], want["z_far"]) and r["binding"] == want["binding"]
    assert same_bits(r["extents"], e) and r["n_vertices"] == 0
    if cam.is_ortho:
        assert same_bits(got["ortho_scale"], want["ortho_scale"])
    else:
        assert got["ortho_scale"] == float(f32(cam.ortho_scale))
    for n in ("dir", "up", "fovy_deg", "aspect", "aperture_radius", "focal_dist"):      # everything else stays
        assert np.array_equal(np.asarray(got[n], f32), np.asarray(getattr(cam, n), f32)), n
    assert got["is_ortho"] == bool(cam.is_ortho)
    return r


@pytest.mark.parametrize("cam_name", list(CAMERAS))
def test_rule_equals_the_float64_restatement_on_random_extents(hip_lib, cam_name):
    cam, W, H = CAMERAS[cam_name]
    r = np.random.default_rng(7)
    accepted = 0
    for k in range(200):
        margin = float(f32(r.uniform(0.0, 0.9)))
        if k % 2:      # extents of a random point cloud in front of the camera: always accepted
            F = ref.frame32(cam, W, H, margin)
            v4 = random_verts4(50, 1, 100 + k, 0.0); v4[:, :3] = v4[:, :3] * f32(r.uniform(0.01, 3.0)) + np.asarray(cam.eye, f32) + f32(5.0) * F["fwd"]
            e = ref.extents32(v4, 1, None, F)[0][0]
        else:          # six arbitrary numbers: accepted or refused, by both
            e = (r.normal(size=6) * 10.0 ** r.uniform(-3, 3)).astype(f32)
        accepted += _check_rule(e, cam, W, H, margin) is not None
    assert accepted >= 100


def directed_points(which):
    r = np.random.default_rng(3)
    if which == "wide":
        p = np.stack([r.uniform(-2, 2, 200), r.uniform(5, 5.2, 200), r.uniform(-0.1, 0.1, 200)], 1)
    elif which == "tall":
        p = np.stack([r.uniform(-0.1, 0.1, 200), r.uniform(5, 5.2, 200), r.uniform(-2, 2, 200)], 1)
    else:              # a narrow cone of points whose apex faces the camera
        a = r.uniform(0, 2 * np.pi, 200); t = r.uniform(0, 1, 200)
        p = np.stack([0.05 * t * np.cos(a), 5.0 + 5.0 * t, 0.05 * t * np.sin(a)], 1); p[0] = (0.0, 5.0, 0.0)
    return np.concatenate([p.astype(f32), np.zeros((len(p), 1), f32)], 1)


@pytest.mark.parametrize("which,binding", [("wide", 0), ("tall", 1), ("cone", 2)])
def test_each_binding_is_reached(hip_lib, which, binding):
    v4 = directed_points(which)
    ext, cnt, _ = fit_extents_host(v4, 1, AXIAL, 64, 64, 0.01)
    r = _check_rule(ext[0], AXIAL, 64, 64, 0.01)
    assert r["binding"] == binding and cnt[0] == 200
    if which != "cone":      # the orthographic rule names the axis that fixed the scale
        cam = dataclasses.replace(AXIAL, is_ortho=True)
        ext, _, _ = fit_extents_host(v4, 1, cam, 64, 64, 0.01)
        assert _check_rule(ext[0], cam, 64, 64, 0.01)["binding"] == binding


# ------------------------------------------------------------------------------------------------ CPU: refusals
def test_refusals(hip_lib):
    good = directed_points("wide")
    ext = fit_extents_host(good, 1, AXIAL, 64, 64, 0.01)[0][0]
    fit_from_extents(ext, AXIAL, 64, 64, 0.0); fit_from_extents(ext, AXIAL, 64, 64, 0.9)      # the ends of the margin's range are accepted
    for margin in (-0.01, 0.91, float("nan"), float("inf")):
        with pytest.raises(BackendError):
            fit_from_extents(ext, AXIAL, 64, 64, margin)
        with pytest.raises(BackendError):
            fit_extents_host(good, 1, AXIAL, 64, 64, margin)
    # no chosen object has a vertex: every vertex unreferenced -> six times -inf, which the rule refuses
    none = good.copy(); none[:, 3] = np.array([-1], np.int32).view(f32)[0]
    e0, c0, _ = fit_extents_host(none, 1, AXIAL, 64, 64, 0.01)
    assert c0[0] == 0 and np.all(np.isneginf(e0))
    with pytest.raises(BackendError):
        fit_from_extents(e0[0], AXIAL, 64, 64, 0.01)
    # all chosen vertices coincide: z_near would be 0
    same = np.tile(np.array([[0.3, 4.0, -0.2, 0.0]], f32), (5, 1))
    for cam in (AXIAL, dataclasses.replace(AXIAL, is_ortho=True)):
        e1 = fit_extents_host(same, 1, cam, 64, 64, 0.01)[0][0]
        assert ref.rule64(e1, ref.frame32(cam, 64, 64, 0.01), cam.is_ortho, 0.01) is None
        with pytest.raises(BackendError):
            fit_from_extents(e1, cam, 64, 64, 0.01)
    # NaN / Inf in the extents, the camera, the transforms
    for bad in (np.nan, np.inf, -np.inf):
        e = ext.copy(); e[2] = bad
        with pytest.raises(BackendError):
            fit_from_extents(e, AXIAL, 64, 64, 0.01)
        for field in ("eye", "dir", "up"):
            cam = dataclasses.replace(AXIAL, **{field: (0.0, bad, 1.0)})
            with pytest.raises(BackendError):
                fit_from_extents(ext, cam, 64, 64, 0.01)
            with pytest.raises(BackendError):
                fit_extents_host(good, 1, cam, 64, 64, 0.01)
        with pytest.raises(BackendError):
            fit_from_extents(ext, dataclasses.replace(AXIAL, fovy_deg=bad), 64, 64, 0.01)
        xf = np.tile(rigid(), (1, 1)); xf[0, 5] = bad
        with pytest.raises(BackendError):
            fit_extents_host(good, 1, AXIAL, 64, 64, 0.01, xf)


# ------------------------------------------------------------------------------------------------ CPU: geometric truth
def _truth_cases():
    sc = object_scene(moved_xforms(7), 96, 64)
    v4 = ref.scene_verts4(sc.pos, sc.tri, sc.tri_object)
    yield "moved_all", v4, 7, sc.obj_xform, np.ones(7, np.uint8)
    yield "moved_box", v4, 7, sc.obj_xform, visible_flags(7, [0, 1, 2, 4, 5, 6])
    yield "moved_three", v4, 7, sc.obj_xform, np.array([0, 0, 0, 1, 0, 1, 1], np.uint8)
    yield "identity_all", v4, 7, None, np.ones(7, np.uint8)
    yield "random", random_verts4(2000, 3, 11), 3, random_xforms(3, 12), np.array([1, 0, 1], np.uint8)
    far = random_verts4(500, 1, 13, 0.0); far[:, :3] = far[:, :3] * f32(40.0) + f32(1000.0)
    yield "far_from_origin", far, 1, None, np.ones(1, np.uint8)


@pytest.mark.parametrize("cam_name", ["perspective", "ortho", "own_aspect", "tall", "tall_ortho"])
def test_fitted_camera_against_float64(hip_lib, cam_name):
    """Geometric truth.  Every chosen vertex, transformed and taken relative to the FITTED float32 eye in float64 (the reported float32 frame read as exact values),
    satisfies  +-x - z kx <= B,  +-y - z ky <= B,  z >= z_near - Bz,  and on the binding axis the largest  x - z kx  and the largest  -x - z kx  are >= -B: the fit is
    tight, not merely safe.  (Orthographic: kx = 0 and the limit is ortho_scale * aspect * (1 - margin) resp. ortho_scale * (1 - margin) instead of 0.)

    Derivation of B, u = 2^-24, first order, per vertex on float64 quantities.  The library guarantees  E(v) <= R  for the float32 EVALUATION E of x - z kx relative
    to the old eye, and the rule gives, in exact arithmetic with an orthonormal frame,  (x - z kx) relative to the new eye = (x - z kx) - R + [(R + L) / 2 + ez kx] with
    the bracket <= 0 (= 0 on the binding axis).  What separates the float64 value from that:
      a) the evaluation chain.  q_a = p_a - pivot_a: one rounding, u|q_a|.  The three-term dot product: three roundings on the first product, fewer on the others:
         3u sum|q_a||r_a|.  So x carries 4u sum|q_a||r_a|, z likewise with f.  z * kx: one more rounding, 5u kx sum|q_a||f_a|.  The last subtraction:
         u |x - z kx| <= u (sum|q_a||r_a| + kx sum|q_a||f_a|).  Together <= 5u sum|q_a||r_a| + 6u kx sum|q_a||f_a| <= 6u (sum|q_a||r_a| + kx sum|q_a||f_a|).
      b) the transform  p_a = ((m0 v0 + m1 v1) + m2 v2) + m3: the first product passes four roundings, the others fewer: 4u T_a, T_a = sum_j |m_aj||v_j| + |m_a3|;
         it reaches x through |r_a| and z kx through kx |f_a|: 4u sum_a T_a (|r_a| + kx |f_a|).  An object at the identity (or without a table) multiplies by 1 and
         adds 0: exact, no term.
      c) the fitted eye is rounded once per component: u sum|eye_a| (|r_a| + kx |f_a|).
      d) the float32 frame is not exactly orthonormal: moving the eye by ex r + ey u + ez f changes x by ex (r.r) + ey (u.r) + ez (f.r) instead of ex.  With
         G = [r u f][r u f]^T - 1 computed in float64 from the reported frame:  |ex||G_rr| + |ey||G_ur| + |ez||G_fr| + kx (|ex||G_rf| + |ey||G_uf| + |ez||G_ff|)
         (the exact deviation, no constant to choose; the y axis alike).
      e) the rule's own float64 roundings: a dozen operations of relative size 2^-53 on quantities no larger than |R| + .. + |F|:  16 * 2^-53 * sum|extents| (1 + 1/kx).
    Bz (for z >= z_near - Bz): 4u sum|q_a||f_a| (a, without the slope terms) + 4u sum T_a |f_a| + u sum|eye_a||f_a| + the f row of d) + e) + u |z_near| (the reported
    z_near is rounded once)."""
    cam, W, H = CAMERAS[cam_name]
    margin = 0.05
    for name, v4, nO, xf, chosen in _truth_cases():
        ext, cnt, fr = fit_extents_host(v4, nO, cam, W, H, margin, xf)
        e, n = ref.chosen_extents(ref.key(ext), cnt, chosen)
        got, res = fit_from_extents(e, cam, W, H, margin)
        r_, u_, f_ = [np.asarray(fr[k], np.float64) for k in ("right", "up", "fwd")]
        kx, ky = float(fr["kx"]), float(fr["ky"])
        eye, old = np.asarray(got["eye"], np.float64), np.asarray(cam.eye, f32).astype(np.float64)
        ob = v4[:, 3].copy().view(np.int32)
        G = np.array([[a @ b for b in (r_, u_, f_)] for a in (r_, u_, f_)]) - np.eye(3)
        off = np.abs(np.linalg.solve(np.array([r_, u_, f_]).T, eye - old))       # |ex|, |ey|, |ez| as applied
        e64 = np.abs(np.asarray(res["extents"], np.float64)).sum() * 16 * 2.0 ** -53 * (1 + (1 / kx if kx else 0))
        worst = dict(x=-np.inf, nx=-np.inf, y=-np.inf, ny=-np.inf)
        aspect = float(ref.frame32(cam, W, H, margin)["aspect"])
        lim_x = float(got["ortho_scale"]) * aspect * (1 - float(f32(margin))) if cam.is_ortho else 0.0
        lim_y = float(got["ortho_scale"]) * (1 - float(f32(margin))) if cam.is_ortho else 0.0
        lim_u = U * (lim_x + lim_y)                                                # orthographic: ortho_scale is rounded once
        for o in np.flatnonzero(chosen):
            v = v4[ob == o, :3].astype(np.float64)
            if not len(v):
                continue
            ident = xf is None
            M = np.eye(3, 4) if ident else np.asarray(xf, f32).reshape(-1, 12)[o].reshape(3, 4).astype(np.float64)
            p = v @ M[:, :3].T + M[:, 3]
            T = np.zeros_like(p) if (ident or np.array_equal(M, np.eye(3, 4))) else np.abs(v) @ np.abs(M[:, :3]).T + np.abs(M[:, 3])
            q_old, q = p - old, p - eye
            x, y, z = q @ r_, q @ u_, q @ f_
            def bound(axis, k):
                a = 6 * U * (np.abs(q_old) @ np.abs(axis) + k * (np.abs(q_old) @ np.abs(f_)))
                b = 4 * U * (T @ (np.abs(axis) + k * np.abs(f_)))
                c = U * (np.abs(eye) @ (np.abs(axis) + k * np.abs(f_)))
                i = 0 if axis is r_ else 1
                d = off @ np.abs(G[:, i]) + k * (off @ np.abs(G[:, 2]))
                return a + b + c + d + e64 + lim_u
            Bx, By = bound(r_, kx), bound(u_, ky)
            Bz = 4 * U * (np.abs(q_old) @ np.abs(f_)) + 4 * U * (T @ np.abs(f_)) + U * (np.abs(eye) @ np.abs(f_)) + off @ np.abs(G[:, 2]) + e64 + U * abs(float(res["z_near"]))
            assert np.all(x - z * kx - lim_x <= Bx) and np.all(-x - z * kx - lim_x <= Bx), (name, float((np.abs(x) - z * kx - lim_x - Bx).max()))
            assert np.all(y - z * ky - lim_y <= By) and np.all(-y - z * ky - lim_y <= By), (name, float((np.abs(y) - z * ky - lim_y - By).max()))
            assert np.all(z >= float(res["z_near"]) - Bz) and np.all(z <= float(res["z_far"]) + Bz + U * abs(float(res["z_far"]))), name
            worst["x"] = max(worst["x"], float((x - z * kx - lim_x + Bx).max())); worst["nx"] = max(worst["nx"], float((-x - z * kx - lim_x + Bx).max()))
            worst["y"] = max(worst["y"], float((y - z * ky - lim_y + By).max())); worst["ny"] = max(worst["ny"], float((-y - z * ky - lim_y + By).max()))
        print(f"{cam_name} {name}: binding {res['binding']}, slack on the four sides {worst}")
        if res["binding"] == 0:
            assert worst["x"] >= 0 and worst["nx"] >= 0, (name, worst)           # tight on both sides of the binding axis
        elif res["binding"] == 1:
            assert worst["y"] >= 0 and worst["ny"] >= 0, (name, worst)
        assert res["binding"] == (0 if cam_name.startswith("tall") else 1), name     # wide targets bind vertically here, the tall ones horizontally


# ------------------------------------------------------------------------------------------------ CPU: ABI
def test_fit_result_layout_matches_header(tmp_path):
    fields = [n for n, _ in abi.crh_fit_result._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(crh_fit_result));' + "".join(
        f'printf("%zu ", offsetof(crh_fit_result, {n}));' for n in fields) + "return 0;}"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [C.sizeof(abi.crh_fit_result)] + [getattr(abi.crh_fit_result, n).offset for n in fields], got
    assert C.sizeof(abi.crh_fit_result) == 84
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in ("crh_fit_view", "crh_fit_extents_host", "crh_fit_from_extents"):
        assert name in abi.EXPORTS and f"CRH_API int {name}(" in header, name


# ================================================================================================ GPU
def soup(owner, n_objects, seed, w=32, h=32):
    """a synthetic soup of len(owner) vertices: vertex i belongs to object owner[i] (-1: no triangle references it); every object's vertices are strung into
    triangles (k, k+1, k+2 of its own list, cyclically), so every owned vertex is referenced and no vertex is shared between objects"""
    owner = np.asarray(owner, np.int32)
    r = np.random.default_rng(seed)
    base = scenes.cornell_box(False, w, h)
    pos = r.uniform(-1, 1, (len(owner), 3)).astype(f32)
    nrm = np.tile(np.array([0, 0, 1], f32), (len(owner), 1))
    tri, tob = [], []
    for o in range(n_objects):
        idx = np.flatnonzero(owner == o)
        if len(idx):
            tri.append(np.stack([idx, np.roll(idx, -1), np.roll(idx, -2), np.zeros_like(idx)], 1)); tob.append(np.full(len(idx), o))
    tri = np.concatenate(tri).astype(np.int32); tob = np.concatenate(tob).astype(np.int32)
    return dataclasses.replace(base, pos=pos, nrm=nrm, tri=tri, uv=None, textures=[], tri_object=tob, obj_xform=random_xforms(n_objects, seed + 1000),
                               camera=dataclasses.replace(OFF_AXIS, eye=(0.3, -6.0, 0.7)))


def host_fit(v4, nO, xf, cam, W, H, margin, chosen):
    """the host twin, end to end: per-object extents and counts, the chosen objects' key maximum (restated here), the rule"""
    ext, cnt, _ = fit_extents_host(v4, nO, cam, W, H, margin, xf)
    e, n = ref.chosen_extents(ref.key(ext), cnt, chosen)
    fields, res = fit_from_extents(e, cam, W, H, margin)
    return ext, cnt, n, fields, res


def assert_device_equals_host(v, v4, nO, xf, cam, W, H, margin, chosen, passed=True):
    """passed: hand the flags over (else NULL = every displayed object, which `chosen` must describe)"""
    ext, cnt, n, fields, res = host_fit(v4, nO, xf, cam, W, H, margin, chosen)
    got, r = v.fit_view(nO, chosen if passed else None, margin, cam, want_extents=True)
    assert same_bits(r["object_extents"], ext), np.argwhere(bits(r["object_extents"]) != bits(ext))[:5]
    assert r["n_vertices"] == n and r["binding"] == res["binding"]
    for k in ("extents", "right", "up", "fwd", "kx", "ky", "z_near", "z_far"):
        assert same_bits(r[k], res[k]), k
    for k in ("eye", "dir", "up", "fovy_deg", "aspect", "ortho_scale", "aperture_radius", "focal_dist"):
        assert same_bits(np.asarray(got[k], f32), np.asarray(fields[k], f32)), k
    assert got["is_ortho"] == fields["is_ortho"]
    return cnt, r


GRID_LANES = 1024 * 256                 # the fit kernel's largest grid x its workgroup size: above it the grid-stride loop takes a second round


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, GRID_LANES + 37841])
def test_device_equals_host_twin_at_the_sizes_where_the_path_changes(hip_lib, n):
    from cadrays_amd.view import View
    sc = soup(np.zeros(n, np.int32), 1, n % 1000)
    if n == 1:                            # a single vertex cannot be fitted (z_near = 0): a second object gives the rule something to stand on
        sc2 = soup(np.array([0, 1, 1, 1]), 2, 5)
        v = View(0).load_scene(sc2); v4 = ref.scene_verts4(sc2.pos, sc2.tri, sc2.tri_object)
        cnt, _ = assert_device_equals_host(v, v4, 2, sc2.obj_xform, sc2.camera, 32, 32, 0.01, np.ones(2, np.uint8))
        assert list(cnt) == [1, 3]
        with pytest.raises(BackendError, match="-> -1"):
            v.fit_view(2, [1, 0], 0.01)   # the single vertex alone: refused
        v.close()
        return
    v = View(0).load_scene(sc)
    v4 = ref.scene_verts4(sc.pos, sc.tri, sc.tri_object)
    for cam in (sc.camera, dataclasses.replace(sc.camera, is_ortho=True)):
        cnt, _ = assert_device_equals_host(v, v4, 1, sc.obj_xform, cam, 32, 32, 0.01, np.ones(1, np.uint8))
        assert cnt[0] == n
    v.close()


def _layouts():
    r = np.random.default_rng(21)
    yield "boundary_in_a_wavefront", np.r_[np.zeros(37), np.ones(163)], 2, None
    yield "boundaries_at_64_and_256", np.r_[np.zeros(64), np.ones(192), np.full(144, 2)], 3, None
    yield "object_without_vertices", np.r_[np.zeros(100), np.ones(90), np.full(110, 3)], 4, None
    yield "erased_between_displayed", np.r_[np.zeros(130), np.ones(130), np.full(130, 2)], 3, [1, 0, 1]
    yield "interleaved", np.arange(700) % 3, 3, None
    o = np.repeat(np.arange(4), 150); o[r.random(600) < 0.2] = -1
    yield "unreferenced_vertices", o, 4, None
    yield "interleaved_tail_and_unreferenced", np.where(np.arange(GRID_LANES // 256 + 77) % 5 == 4, -1, np.arange(GRID_LANES // 256 + 77) % 2), 2, None


@pytest.mark.gpu
@pytest.mark.parametrize("name", [l[0] for l in _layouts()])
def test_object_layouts(hip_lib, name):
    from cadrays_amd.view import View
    _, owner, nO, visible = next(l for l in _layouts() if l[0] == name)
    sc = soup(owner, nO, 31)
    v = View(0).load_scene(sc)
    v4 = ref.scene_verts4(sc.pos, sc.tri, sc.tri_object)
    assert np.array_equal(v4[:, 3].copy().view(np.int32), np.asarray(owner, np.int32))
    if visible is not None:
        v.set_visibility(visible)
        assert_device_equals_host(v, v4, nO, sc.obj_xform, sc.camera, 32, 32, 0.02, np.asarray(visible, np.uint8), passed=False)
    assert_device_equals_host(v, v4, nO, sc.obj_xform, sc.camera, 32, 32, 0.02, np.ones(nO, np.uint8))
    for o in range(nO):                   # every object alone: its own count, and a refusal where it has no vertex
        one = np.zeros(nO, np.uint8); one[o] = 1
        n_o = int((np.asarray(owner) == o).sum())
        if n_o < 2:
            with pytest.raises(BackendError, match="-> -1"):
                v.fit_view(nO, one, 0.02)
        else:
            cnt, r = assert_device_equals_host(v, v4, nO, sc.obj_xform, sc.camera, 32, 32, 0.02, one)
            assert r["n_vertices"] == n_o == cnt[o]
    v.close()


@pytest.mark.gpu
def test_live_scene_moved_erased_added(hip_lib):
    from cadrays_amd.view import View
    W, H = 96, 64
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    v4 = ref.scene_verts4(sc.pos, sc.tri, sc.tri_object)
    cam = sc.camera
    ones = np.ones(7, np.uint8)
    assert_device_equals_host(v, v4, 7, sc.obj_xform, cam, W, H, 0.01, ones, passed=False)
    xf = moved_xforms(7)
    v.set_transforms(xf)
    _, r = assert_device_equals_host(v, v4, 7, xf, cam, W, H, 0.01, ones, passed=False)
    assert_device_equals_host(v, v4, 7, xf, OFF_AXIS, W, H, 0.2, np.array([0, 0, 0, 1, 0, 1, 0], np.uint8))      # flags and a camera of the caller's
    for o in range(7):                    # extents_out rows are the single-object fits
        one = np.zeros(7, np.uint8); one[o] = 1
        _, ro = assert_device_equals_host(v, v4, 7, xf, cam, W, H, 0.01, one)
        assert same_bits(ro["extents"], r["object_extents"][o])
    vis = visible_flags(7, [0, 4])
    v.set_visibility(vis)
    assert_device_equals_host(v, v4, 7, xf, cam, W, H, 0.01, vis, passed=False)
    assert_device_equals_host(v, v4, 7, xf, cam, W, H, 0.01, ones)                       # flags override the visibility
    p, n, t = one_object(sc, 3)
    new_xf = rigid(30.0, (0, 0, 1), (0.1, -0.3, 0.35))
    assert v.add_object(p, n, t, new_xf) == 7
    v4b = np.concatenate([v4, np.concatenate([np.asarray(p, f32), np.full((len(p), 1), 7, np.int32).view(f32)], 1)])
    xfb = np.concatenate([xf, new_xf[None]])
    with pytest.raises(BackendError, match="-> -1"):
        v.fit_view(7, ones, 0.01)         # the flags take one more entry now
    assert_device_equals_host(v, v4b, 8, xfb, cam, W, H, 0.01, np.r_[vis, 1].astype(np.uint8), passed=False)
    assert_device_equals_host(v, v4b, 8, xfb, cam, W, H, 0.01, np.array([0, 0, 0, 0, 0, 0, 0, 1], np.uint8))
    # the View vocabulary: FitSelected sets the camera and restarts
    v.Redraw()
    v._selected = {7}
    res = v.FitSelected(0.01)
    assert v.stats()["samples"] == 0 and res["z_near"] > 0 and res["z_far"] > res["z_near"]
    assert same_bits(np.asarray(v._camera.eye, f32), np.asarray(host_fit(v4b, 8, xfb, cam, W, H, 0.01, np.array([0] * 7 + [1], np.uint8))[3]["eye"], f32))
    v.close()
    # a scene handed over without objects counts as one object
    plain = scenes.cornell_box(True, 64, 48)
    w = View(0).load_scene(plain)
    assert_device_equals_host(w, ref.scene_verts4(plain.pos, plain.tri), 1, None, plain.camera, 64, 48, 0.01, np.ones(1, np.uint8), passed=False)
    res = w.FitAll()
    assert res["n_vertices"] == len(np.unique(plain.tri[:, :3]))
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "ortho"])
def test_end_to_end_through_the_id_buffer(hip_lib, ortho):
    from cadrays_amd.view import View
    W, H, margin = 96, 64, 0.125
    sc = object_scene(None, W, H)
    cam = dataclasses.replace(sc.camera, is_ortho=True, ortho_scale=1.0) if ortho else sc.camera
    v = View(0).load_scene(dataclasses.replace(sc, camera=cam))
    v.set_visibility(visible_flags(7, [0, 1, 2, 4, 5, 6]))      # only the yellow box, object 3
    fields, r = v.fit_view(7, None, margin)
    v.set_camera(dataclasses.replace(cam, **fields))
    ob = v.read_ids()[0]
    ys, xs = np.nonzero(ob == 3)
    assert len(ys) > 100 and set(np.unique(ob)) <= {-1, 3}
    bx, by = margin * W / 2, margin * H / 2
    print(f"binding {r['binding']}: columns {xs.min()}..{xs.max()} of {W} (band {bx}), rows {ys.min()}..{ys.max()} of {H} (band {by})")
    assert xs.min() >= int(np.floor(bx)) - 1 and xs.max() <= W - 1 - (int(np.floor(bx)) - 1)
    assert ys.min() >= int(np.floor(by)) - 1 and ys.max() <= H - 1 - (int(np.floor(by)) - 1)
    if r["binding"] == 0:
        assert xs.min() <= bx + 2 and xs.max() >= W - 1 - bx - 2
    elif r["binding"] == 1:
        assert ys.min() <= by + 2 and ys.max() >= H - 1 - by - 2
    assert r["binding"] in (0, 1)
    v.close()


@pytest.mark.gpu
def test_fitting_leaves_the_accumulation_alone(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 128, 96)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    plain = View(0).load_scene(sc)
    for _ in range(3): plain.Redraw()
    ldr3 = plain.read_ldr()
    for _ in range(3): plain.Redraw()
    want, (want_acc, want_frames), want_stats = plain.read_hdr(), plain.save_accum(), plain.stats()
    v = View(0).load_scene(sc)
    for _ in range(3): v.Redraw()
    v.read_ldr_begin()                     # one read-back outstanding across the fits
    ids_before = v.read_ids()[0]
    a, _ = v.fit_view(7, None, 0.01)
    b, _ = v.fit_view(7, [0, 0, 0, 1, 0, 1, 0], 0.01)
    assert a["eye"] != b["eye"]
    assert np.array_equal(v.read_ldr_end(), ldr3)
    assert v._fn("pick") and np.array_equal(v.read_ids()[0], ids_before)
    for _ in range(3): v.Redraw()
    acc, frames = v.save_accum()
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and frames == want_frames == 6
    assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32))
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    v.close(); plain.close()


@pytest.mark.gpu
def test_fit_argument_errors(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4"):
        v.fit_view(7, None, 0.01)          # before crh_build
    v.load_scene(sc)
    for n, chosen in ((6, None), (8, None), (6, np.ones(6)), (8, np.ones(8))):
        with pytest.raises(BackendError, match="-> -1"):
            v.fit_view(n, chosen, 0.01)    # flag count wrong
    for margin in (-0.1, 0.95, float("nan")):
        with pytest.raises(BackendError, match="-> -1"):
            v.fit_view(7, None, margin)
    with pytest.raises(BackendError, match="-> -1"):
        v.fit_view(7, np.zeros(7), 0.01)   # nothing chosen
    with pytest.raises(BackendError, match="-> -1"):
        v.fit_view(7, None, 0.01, dataclasses.replace(sc.camera, eye=(0.0, float("inf"), 0.0)))
    v.set_visibility(np.zeros(7, np.uint8))
    with pytest.raises(BackendError, match="-> -1"):
        v.fit_view(7, None, 0.01)          # nothing displayed
    v.fit_view(7, np.ones(7), 0.01)
    v.close()
