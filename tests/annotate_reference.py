"""The annotations' rules restated from the text of include/cadrays_hip.h (section "annotations"): THE PROJECTION in float64 (Python floats: IEEE double, every
operation rounded on its own, no fused multiply-add), THE PIXEL RULE and the composite in numpy float32 / uint32.  Nothing here looks at the library's sources.

    frame    the camera frame as crh_reproject_frame_host hands it out (cadrays_amd.view.reproject_frame_host): eye, right, up, fwd, tan_half, aspect, ortho_scale, is_ortho
    project  the records of a list, numpy records {x0, y0, x1, y1, q0, q1, flags, pad}
    draw     the list over an image: (image, id plane, parameter plane); `wrong` names one deliberately wrong rule (WRONG)
"""
import numpy as np

f32, u32 = np.float32, np.uint32
ON_TOP, HIDE, XRAY = 0, 1, 2
SEGMENT_DTYPE = np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3,)), ("rgb", "u1", (3,)), ("alpha", "u1"), ("style", "<u4")])
RECORD_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("q0", "<f4"), ("q1", "<f4"), ("flags", "<u4"), ("pad", "<u4")])
DEFAULT_BIAS, DEFAULT_HIDDEN = f32(2.0 ** -9), 64
MISS = f32(1.0e15)
WRONG = ("strict_coverage", "descending_order", "no_bias", "xray_as_hide")


def style(width, mode=ON_TOP):
    return int(width) | (int(mode) << 8)


def _dot(v, b):
    return (v[0] * float(b[0]) + v[1] * float(b[1])) + v[2] * float(b[2])


def _edge(p, q, t):
    """one edge of Liang-Barsky over t = [t0, t1]: False when nothing is left"""
    if p == 0.0:
        return q >= 0.0
    r = q / p
    if p < 0.0:
        if r > t[1]:
            return False
        if r > t[0]:
            t[0] = r
    else:
        if r < t[0]:
            return False
        if r < t[1]:
            t[1] = r
    return True


def project_one(F, W, H, a, b):
    """(x0, y0, x1, y1, q0, q1) rounded to float32, or None: the record is invalid"""
    eye = [float(x) for x in F["eye"]]
    va, vb = [float(a[k]) - eye[k] for k in range(3)], [float(b[k]) - eye[k] for k in range(3)]
    xa, ya, za = _dot(va, F["right"]), _dot(va, F["up"]), _dot(va, F["fwd"])
    xb, yb, zb = _dot(vb, F["right"]), _dot(vb, F["up"]), _dot(vb, F["fwd"])
    zmax = za if za > zb else zb
    if not zmax > 0.0:
        return None
    ortho = bool(F["is_ortho"])
    zmin = 0.0 if ortho else zmax * 2.0 ** -16
    if za < zmin:
        u = (zmin - za) / (zb - za)
        xa, ya, za = xa + u * (xb - xa), ya + u * (yb - ya), zmin
    elif zb < zmin:
        u = (zmin - zb) / (za - zb)
        xb, yb, zb = xb + u * (xa - xb), yb + u * (ya - yb), zmin
    kx, ky = float(F["tan_half"]) * float(F["aspect"]), float(F["tan_half"])
    hw, hh = float(W) * 0.5, float(H) * 0.5
    with np.errstate(all="ignore"):
        one, za_, zb_ = np.float64(1.0), np.float64(za), np.float64(zb)      # numpy doubles: a division by zero gives inf / nan instead of raising
        xa, ya, xb, yb = np.float64(xa), np.float64(ya), np.float64(xb), np.float64(yb)
        if ortho:
            dx, dy = np.float64(float(F["ortho_scale"]) * float(F["aspect"])), np.float64(float(F["ortho_scale"]))
            X0, Y0, X1, Y1 = (xa / dx + one) * hw, (one - ya / dy) * hh, (xb / dx + one) * hw, (one - yb / dy) * hh
            Q0, Q1 = za_, zb_
        else:
            X0, Y0, X1, Y1 = (xa / (za_ * kx) + one) * hw, (one - ya / (za_ * ky)) * hh, (xb / (zb_ * kx) + one) * hw, (one - yb / (zb_ * ky)) * hh
            Q0, Q1 = one / za_, one / zb_
        Wd, Hd = np.float64(W), np.float64(H)
        DX, DY, DQ = X1 - X0, Y1 - Y0, Q1 - Q0
        t = [np.float64(0.0), np.float64(1.0)]
        if not (_edge(-DX, X0 + Wd, t) and _edge(DX, (Wd + Wd) - X0, t) and _edge(-DY, Y0 + Hd, t) and _edge(DY, (Hd + Hd) - Y0, t)):
            return None
        x1, y1, q1 = (X0 + t[1] * DX, Y0 + t[1] * DY, Q0 + t[1] * DQ) if t[1] < 1.0 else (X1, Y1, Q1)
        x0, y0, q0 = (X0 + t[0] * DX, Y0 + t[0] * DY, Q0 + t[0] * DQ) if t[0] > 0.0 else (X0, Y0, Q0)
        if not all(np.isfinite(v) for v in (x0, y0, x1, y1, q0, q1)):
            return None
        band = lambda v, lo, hi: (lambda m: m if m < hi else hi)(v if v > lo else lo)
        out = tuple(f32(v) for v in (band(x0, -Wd, Wd + Wd), band(y0, -Hd, Hd + Hd), band(x1, -Wd, Wd + Wd), band(y1, -Hd, Hd + Hd), q0, q1))
    return out if all(np.isfinite(v) for v in out) else None


def project(F, W, H, segs):
    rec = np.zeros(len(segs), RECORD_DTYPE)
    with np.errstate(over="ignore"):
        for i, s in enumerate(segs):
            r = project_one(F, W, H, s["a"], s["b"])
            if r is not None:
                rec[i] = r + (1, 0)
    return rec


def hit_depth(F, rays, t_px):
    """zh per pixel: t (d . fwd) in float32, the dot product as (d.x f.x + d.y f.y) + d.z f.z; t itself under an orthographic camera"""
    t = np.asarray(t_px, f32)
    if F["is_ortho"]:
        return t
    d = np.asarray(rays, f32).reshape(t.shape + (8,))[..., 4:7]
    f = np.asarray(F["fwd"], f32)
    return t * ((d[..., 0] * f[0] + d[..., 1] * f[1]) + d[..., 2] * f[2])


def draw(rec, segs, F, W, H, ldr=None, rays=None, t_px=None, depth_bias=DEFAULT_BIAS, hidden_alpha=DEFAULT_HIDDEN, wrong=None):
    """(image uint8 (H, W, 3), ids int32 (H, W), s float32 (H, W)): the segments composited in ascending index over a copy of `ldr` (zeros when None)"""
    img = (np.zeros((H, W, 3), np.uint8) if ldr is None else np.asarray(ldr, np.uint8)).astype(u32)
    ids, s_px = np.full((H, W), -1, np.int32), np.zeros((H, W), f32)
    py, px = np.meshgrid(np.arange(H).astype(f32) + f32(0.5), np.arange(W).astype(f32) + f32(0.5), indexing="ij")
    ortho = bool(F["is_ortho"])
    zh = t = None
    order = range(len(segs) - 1, -1, -1) if wrong == "descending_order" else range(len(segs))
    with np.errstate(all="ignore"):
        for i in order:
            R, S = rec[i], segs[i]
            if not int(R["flags"]) & 1:
                continue
            width, mode = int(S["style"]) & 15, (int(S["style"]) >> 8) & 3
            x0, y0, ex, ey = R["x0"], R["y0"], R["x1"] - R["x0"], R["y1"] - R["y0"]
            l2 = ex * ex + ey * ey
            if l2 > 0:
                s = ((px - x0) * ex + (py - y0) * ey) / l2
                s = np.where(s > 0, s, f32(0))
                s = np.where(s < 1, s, f32(1))
            else:
                s = np.zeros((H, W), f32)
            dx, dy = px - (x0 + s * ex), py - (y0 + s * ey)
            h = f32(width) * f32(0.5)
            d2 = dx * dx + dy * dy
            covered = d2 < h * h if wrong == "strict_coverage" else d2 <= h * h
            A = np.full((H, W), int(S["alpha"]), u32)
            skip = np.zeros((H, W), bool)
            if mode != ON_TOP:
                if zh is None:
                    t = np.asarray(t_px, f32); zh = hit_depth(F, rays, t)
                qs = R["q0"] + s * (R["q1"] - R["q0"])
                zb = zh if wrong == "no_bias" else zh * (f32(1.0) + f32(depth_bias))
                occluded = ((qs > zb) if ortho else (qs * zb < f32(1.0))) & (t < MISS)
                if mode == XRAY and wrong != "xray_as_hide":
                    A = np.where(occluded, u32((int(S["alpha"]) * int(hidden_alpha) + 128) >> 8), A).astype(u32)
                else:
                    skip = occluded
            m = covered & ~skip
            for ch in range(3):
                img[..., ch] = np.where(m, (img[..., ch] * (u32(256) - A) + u32(int(S["rgb"][ch])) * A + u32(128)) >> u32(8), img[..., ch])
            ids[m] = i
            s_px[m] = s[m]
    return img.astype(np.uint8), ids, s_px
