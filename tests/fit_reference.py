"""numpy restatement of view fitting (include/cadrays_hip.h, crh_fit_view): nothing of the library enters it.

  frame32      right / up / fwd, tan(fovy / 2), aspect, kx, ky in float32 exactly as the library's host code derives them (include/crh_math.h: fused
               multiply-adds where that header writes them -- emulated exactly with rationals -- and its sin / cos polynomials)
  extents32    the six maxima and the vertex count per object: plain float32 products, sums and differences in the stated order, maxima on the integer key
  rule64       the closed-form rule in float64 (Python floats), every output rounded to float32 once
"""
from fractions import Fraction

import numpy as np

f32 = np.float32
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ float32 scalar helpers
def fma32(a, b, c):
    """round_to_nearest_even_float32(a * b + c), exactly: the sum as a rational, then the nearest of the float32 neighbours of its double value"""
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = f32(float(r))
    cands = {float(g), float(np.nextafter(g, f32(np.inf))), float(np.nextafter(g, f32(-np.inf)))}
    best = None
    for x in cands:
        if not np.isfinite(x):
            continue
        d = abs(Fraction(x) - r)
        even = (int(f32(x).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, x)
    return f32(best[1])


def _dot3(a, b):
    return fma32(a[2], b[2], fma32(a[1], b[1], f32(a[0] * b[0])))


def _cross3(a, b):
    return np.array([fma32(a[1], b[2], -f32(a[2] * b[1])), fma32(a[2], b[0], -f32(a[0] * b[2])), fma32(a[0], b[1], -f32(a[1] * b[0]))], f32)


def _norm3(a):
    l2 = _dot3(a, a)
    inv = f32(1.0) / np.sqrt(l2) if l2 > 0 else f32(0.0)
    return np.array([a[0] * inv, a[1] * inv, a[2] * inv], f32)


def _sin_poly(a):
    z = f32(a * a)
    p = fma32(z, f32(-1.9515295891e-4), f32(8.3321608736e-3))
    p = fma32(z, p, f32(-1.6666654611e-1))
    return fma32(f32(a * z), p, a)


def _cos_poly(a):
    z = f32(a * a)
    p = fma32(z, f32(2.443315711809948e-5), f32(-1.388731625493765e-3))
    p = fma32(z, p, f32(4.166664568298827e-2))
    return fma32(f32(z * z), p, fma32(z, f32(-0.5), f32(1.0)))


def _sincos(a):
    t = f32(a * f32(0.15915494309189533577))
    fl = f32(int(t))
    if fl > t:
        fl = f32(fl - f32(1.0))
    x = f32(t - fl)
    q = int(fma32(x, f32(4.0), f32(0.5)))
    r = fma32(f32(q), f32(-0.25), x)
    ang = f32(r * f32(6.28318530717958647692))
    sp, cp = _sin_poly(ang), _cos_poly(ang)
    return [(sp, cp), (cp, -sp), (-sp, -cp), (-cp, sp)][q & 3]


def frame32(cam, W, H, margin):
    """dict(pivot, right, up, fwd (float32[3]), tan_half, aspect, kx, ky (float32)) of a scenes.Camera on a W x H target"""
    fwd = _norm3(np.asarray(cam.dir, f32))
    right = _norm3(_cross3(fwd, np.asarray(cam.up, f32)))
    up = _cross3(right, fwd)
    s, c = _sincos(f32(f32(f32(cam.fovy_deg) * f32(0.5)) * f32(f32(3.14159265358979323846) / f32(180.0))))
    tan_half = f32(s / c)
    aspect = f32(cam.aspect) if f32(cam.aspect) > 0 else f32(f32(W) / f32(H))
    m = float(f32(margin))
    if cam.is_ortho:
        kx = ky = f32(0.0)
    else:
        kx = f32((float(tan_half) * float(aspect)) * (1.0 - m))
        ky = f32(float(tan_half) * (1.0 - m))
    return dict(pivot=np.asarray(cam.eye, f32), right=right, up=up, fwd=fwd, tan_half=tan_half, aspect=aspect, kx=kx, ky=ky)


# ------------------------------------------------------------------------------------------------ the extents
def key(x):
    """order-preserving uint32 key of float32 values: all bits flipped for negatives, the sign bit flipped otherwise"""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(f32)


def vertex_values32(v, m, F):
    """(n, 6) float32: the six values of vertices v (n, 3) float32 of an object with rows m (12 float32), one rounding per operation, no fused operation"""
    v = np.asarray(v, f32); m = np.asarray(m, f32)
    p = [((m[4 * a] * v[:, 0] + m[4 * a + 1] * v[:, 1]) + m[4 * a + 2] * v[:, 2]) + m[4 * a + 3] for a in range(3)]
    q = [p[a] - F["pivot"][a] for a in range(3)]
    x, y, z = [(q[0] * F[n][0] + q[1] * F[n][1]) + q[2] * F[n][2] for n in ("right", "up", "fwd")]
    zx, zy = z * F["kx"], z * F["ky"]
    out = np.stack([x - zx, -x - zx, y - zy, -y - zy, -z, z], 1)
    assert out.dtype == f32
    return out


def extents32(verts4, n_objects, xf, F):
    """(extents (n_objects, 6) float32 with -inf rows for objects without a vertex, counts (n_objects,) uint32, keys (n_objects, 6) uint32 with 0 = no vertex)"""
    v4 = np.ascontiguousarray(verts4, f32).reshape(-1, 4)
    ob = v4[:, 3].copy().view(np.int32)
    keys, cnt = np.zeros((n_objects, 6), np.uint32), np.zeros(n_objects, np.uint32)
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
    for o in range(n_objects):
        sel = ob == o
        cnt[o] = sel.sum()
        if cnt[o]:
            keys[o] = key(vertex_values32(v4[sel, :3], ident if xf is None else np.asarray(xf, f32).reshape(-1, 12)[o], F)).max(0)
    ext = np.where(cnt[:, None] > 0, unkey(keys), f32(-np.inf)).astype(f32)
    return ext, cnt, keys


def chosen_extents(keys, cnt, chosen):
    """key maximum over the chosen objects that have a vertex -> (6 float32, number of vertices)"""
    use = (np.asarray(chosen) != 0) & (cnt > 0)
    if not use.any():
        return None, 0
    return unkey(keys[use].max(0)), int(cnt[use].sum())


def scene_verts4(pos, tri, tri_object=None):
    """the array the library builds from a scene: {x, y, z, object as int bits}; object 0 without objects, -1 for a vertex no triangle references"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    owner = np.full(len(pos), -1, np.int32)
    t = np.asarray(tri, np.int32).reshape(-1, 4)
    for k in range(3):
        owner[t[:, k]] = 0 if tri_object is None else np.asarray(tri_object, np.int32)
    return np.concatenate([pos, owner.view(f32)[:, None]], 1)


# ------------------------------------------------------------------------------------------------ the rule
def rule64(e, F, is_ortho, margin):
    """the fitted eye (float32[3]), ortho_scale (float32 or None), z_near, z_far (float32), binding; None where the rule refuses"""
    if not np.all(np.isfinite(e)):
        return None
    R, L, U, D, N, Fz = [float(x) for x in e]
    ex, ey = (R - L) / 2.0, (U - D) / 2.0
    half = None
    if not is_ortho:
        zx, zy, clear = -(R + L) / (2.0 * float(F["kx"])), -(U + D) / (2.0 * float(F["ky"])), -N - (Fz + N) / 16.0
        ez, binding = zx, 0
        if zy < ez: ez, binding = zy, 1
        if clear < ez: ez, binding = clear, 2
    else:
        hv, hh = (U + D) / 2.0, (R + L) / (2.0 * float(F["aspect"]))
        binding = 1 if hv >= hh else 0
        half = max(hv, hh) / (1.0 - float(f32(margin)))
        ez = -N - max(Fz + N, 2.0 * half)
    zn, zf = -N - ez, Fz - ez
    with np.errstate(over="ignore"):
        eye = np.array([f32(((float(F["pivot"][a]) + ex * float(F["right"][a])) + ey * float(F["up"][a])) + ez * float(F["fwd"][a])) for a in range(3)], f32)
        outs = [f32(zn), f32(zf)] + ([f32(half)] if half is not None else [])
    if not (np.all(np.isfinite(eye)) and np.all(np.isfinite(outs)) and np.isfinite(ez)) or not zn > 0.0:
        return None
    return dict(eye=eye, ortho_scale=None if half is None else f32(half), z_near=f32(zn), z_far=f32(zf), binding=binding, offsets=(ex, ey, ez))
