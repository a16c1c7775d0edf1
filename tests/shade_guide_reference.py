"""The shade guide of the denoised display, restated in numpy from the text of include/cadrays_hip.h ("shade guide of the denoised display"), not from the C++.

RULE 2 (the guided pass) is integer work and float32 arithmetic of single operations -- one product, one product, one sum, two divisions, each rounded as C
rounds it -- so the library's bytes are expected to be EQUAL to guided_denoise(), and no tolerance appears.

RULE 1 (the plane) holds a bilinear texture lookup and a cone test: these are judged against FLOAT64 evaluations with bounds that come from the references
themselves -- albedo_ref() composes lookup_reference.texture_ref (value and bound D) with the material's lobe weights; light_ref() evaluates the disc test in double
and reports every pixel's margin |cos - cos_max|, so that a test can excuse the pixels a float32 evaluation may decide either way.  The dilation is integer work.

  guided_pass(img, k, G, plane, ...) / guided_denoise(rgba, ob, tr, t, table, plane, ..., wrong=None)
  WRONG                              deliberately broken forms of rule 2: each must change the image
  albedo_ref(mat_rows, images, what, mat, uv, gamma2)   float64 albedo per case and its bound
  pixel_centre_rays(cam, W, H)       float32 rays in crh_camera_rays' layout, computed in double and rounded once (the twin takes whatever rays it is handed)
  light_ref(rays, tr, t, lights)     (seen, margin) in float64
  dilate(seen, r)                    Chebyshev dilation inside the frame
"""
import numpy as np

import denoise_reference as D
import lookup_reference as L

f32 = np.float32
WRONG = ("w_after_sum", "fma", "flag_ignored_for_taps")
PLANE_ONES = (1.0, 1.0, 1.0, 0.0)


# ================================================================================================ rule 2
def guided_pass(img, k, G, plane, normal_cos, depth_ratio, until_samples, wrong=None):
    H, W = G["ob"].shape
    s = 1 << k
    w = img[..., 3]
    flag = plane[..., 3] != 0
    with np.errstate(all="ignore"):
        scaled_w = w * f32(1 << (2 * k))
        enough = ~(scaled_w < f32(until_samples))
    through = (G["tr"] < 0) | ~(w > 0) | ~D._finite3(img) | enough | flag
    yy, xx = np.mgrid[0:H, 0:W]
    sr = np.zeros((H, W, 3), f32)
    wsum = np.zeros((H, W), np.uint32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = yy + dy * s, xx + dx * s
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            q = img[cy, cx]
            same_object = G["ob"] == G["ob"][cy, cx]
            both_hit = (G["tr"] >= 0) & (G["tr"][cy, cx] >= 0)
            same_tri = G["tr"] == G["tr"][cy, cx]
            n, m = G["n"], G["n"][cy, cx]
            with np.errstate(all="ignore"):
                dot = (n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]
                normal_ok = G["has_n"] & G["has_n"][cy, cx] & (np.abs(dot) >= f32(normal_cos))
                ta, tb = G["t"], G["t"][cy, cx]
                lo, hi = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
                step = hi > lo * f32(depth_ratio)
            sim = same_object & both_hit & (same_tri | (normal_ok & ~step))
            take = inside & (q[..., 3] > 0) & D._finite3(q) & sim & ~through
            if wrong != "flag_ignored_for_taps":
                take &= ~flag[cy, cx]
            c = D.H5[dy + 2] * D.H5[dx + 2]
            gq = plane[cy, cx][..., :3]
            with np.errstate(all="ignore"):
                if wrong == "w_after_sum":
                    new = sr + f32(c) * q[..., :3]
                elif wrong == "fma":
                    d = q[..., :3] * gq
                    new = D._fmaf(np.broadcast_to(f32(c), d.shape), d, sr)
                else:
                    d = q[..., :3] * gq                                        # the tap times its own w, rounded ...
                    prod = f32(c) * d                                          # ... the spline weight, rounded ...
                    new = sr + prod                                            # ... then the sum, rounded
                assert new.dtype == f32
            sr = np.where(take[..., None], new, sr)
            wsum += np.where(take, np.uint32(c), np.uint32(0)).astype(np.uint32)
    with np.errstate(all="ignore"):
        mean = sr / wsum.astype(f32)[..., None]
        if wrong == "w_after_sum":
            mean = mean * plane[..., :3]
        rgb = mean / plane[..., :3]                                            # two plain divisions
    assert rgb.dtype == f32
    out = img.copy()
    filt = ~through
    assert (wsum[filt] >= 36).all()
    out.view(np.uint32)[..., :3][filt] = rgb.view(np.uint32)[filt]
    return out


def guided_denoise(rgba, ob, tr, t, table, plane, levels=4, normal_cos=D.DEFAULTS["normal_cos"], depth_ratio=D.DEFAULTS["depth_ratio"], until_samples=256, wrong=None):
    img = np.ascontiguousarray(rgba, f32).copy()
    G = D.guide(np.asarray(ob, np.int32), np.asarray(tr, np.int32), np.asarray(t, f32), table)
    pl = np.ascontiguousarray(plane, f32)
    for k in range(int(levels)):
        img = guided_pass(img, k, G, pl, normal_cos, depth_ratio, until_samples, wrong)
    return img


def random_plane(r, W, H):
    """w of every magnitude the rule meets (1 / 64 ... 64, and exact ones), ~6 % of the pixels flagged, in runs"""
    p = np.zeros((H, W, 4), f32)
    p[..., :3] = np.exp2(r.uniform(-6, 6, (H, W, 3))).astype(f32)
    p[r.random((H, W)) < 0.2, :3] = 1.0
    flag = r.random((H, W)) < 0.03
    flag |= np.roll(flag, 1, 1)
    p[..., 3] = flag
    return p


# ================================================================================================ rule 1: the albedo
OPS = 5       # the stated float32 operations between the texel and 1 / w: Kd * tx, three sums, the division -- one ulp of the result's magnitude each


def albedo_ref(mat_rows, images, what, mat, uv, gamma2):
    """float64 albedo m = Kd tx + Ks + Kc + Kt of every case (n, 3) and the bound (n, 3) a float32 evaluation of the header's rule may differ from it by.
    mat_rows (n_mats, 32) float32: the packed crh_bsdf; what[k] = (slot, scale) of material k; mat (n,), uv (n, 2) float32: the cases; textures with alpha 1"""
    rows = np.asarray(mat_rows, f32).astype(np.float64)
    val, bound = np.zeros((len(mat), 3)), np.zeros((len(mat), 3))
    for k, (slot, scale) in enumerate(what):
        sel = mat == k
        if not sel.any():
            continue
        tx, Dk = L.texture_ref(images[slot], uv[sel, 0], uv[sel, 1], scale, gamma2)
        kc, kd, ks, kt = rows[k, 0:3], rows[k, 4:7], rows[k, 8:11], rows[k, 12:15]
        m = kd * tx[:, :3] + ks + kc + kt
        val[sel] = m
        bound[sel] = kd * Dk[:, :3] + OPS * L.ulp32(np.abs(m) + kd * Dk[:, :3])
    return val, bound


# ================================================================================================ rule 1: the lights
def camera_basis(cam, W, H):
    fwd = np.asarray(cam.dir, np.float64); fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(cam.up, np.float64)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    aspect = cam.aspect if cam.aspect > 0 else W / H
    return fwd, right, up, aspect


def pixel_centre_rays(cam, W, H):
    """(H * W, 8) float32 {o.xyz, 1e15, d.xyz, 0}: the pixel-centre rays of a scenes.Camera, in double, rounded once"""
    fwd, right, up, aspect = camera_basis(cam, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    nx, ny = (xx + 0.5) / W * 2 - 1, 1 - (yy + 0.5) / H * 2
    eye = np.asarray(cam.eye, np.float64)
    if cam.is_ortho:
        o = eye + (nx * cam.ortho_scale * aspect)[..., None] * right + (ny * cam.ortho_scale)[..., None] * up
        d = np.broadcast_to(fwd, o.shape)
    else:
        th = np.tan(np.deg2rad(cam.fovy_deg) / 2)
        d = fwd + (nx * th * aspect)[..., None] * right + (ny * th)[..., None] * up
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        o = np.broadcast_to(eye, d.shape)
    rays = np.zeros((H * W, 8), f32)
    rays[:, 0:3] = o.reshape(-1, 3); rays[:, 3] = 1e15; rays[:, 4:7] = d.reshape(-1, 3)
    return rays


def light_ref(rays, tr, t, lights):
    """(seen (H, W) bool, margin (H, W)) in float64 for the float32 rays handed over: a positional light of radius r > 0 at distance dist < hd from the ray's origin
    shows when cos(angle between d and the centre) >= cos_max = 1 / sqrt(1 + (r / dist)^2); margin = the smallest |cos - cos_max| over the lights in front of
    the hit: what a float32 evaluation must not be asked to decide when it is tiny"""
    H, W = tr.shape
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    hd = np.where(tr.reshape(-1) >= 0, np.asarray(t, f32).astype(np.float64).reshape(-1), 1e15)
    seen, margin = np.zeros(H * W, bool), np.full(H * W, np.inf)
    for l in lights:
        if not l.is_point:
            continue
        tl = np.asarray(l.vec, f32).astype(np.float64) - o
        dist = np.linalg.norm(tl, axis=1)
        r = float(f32(l.smoothness))
        cm = 1.0 / np.sqrt(1.0 + (r / dist) ** 2)
        cos = (d * tl).sum(1) / dist
        near = dist < hd
        seen |= near & (cm < 1.0) & (cos >= cm)
        if r > 0:
            margin = np.minimum(margin, np.where(near, np.abs(cos - cm), np.inf))
    return seen.reshape(H, W), margin.reshape(H, W)


def dilate(seen, r):
    H, W = seen.shape
    out = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] |= seen[ys, xs]
    return out
