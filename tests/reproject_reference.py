"""Reprojected display history, restated in numpy from the text of include/cadrays_hip.h ("reprojected display history"), not from the C++.

Everything here is integer work or float32 arithmetic of single operations -- one product, one sum, one division, one square root, one floor at a time, each rounded as
C rounds it: no transcendental, no fused multiply-add.  So the library's bytes are expected to be EQUAL to these, and no tolerance appears.

  reproject(a, rays, ob, tr, t, hist, table, max_history, until_samples, normal_cos, depth_ratio, wrong=None, stats=None)
                                                the rule; hist = None or dict(rgba, ob, tr, t, frame); wrong = one of WRONG: a deliberately broken rule; stats: a dict
                                                that receives how many pixels took history, were refused, and how many taps counted
  make_frame / rays_of / view_of                a camera frame, its pixel-centre rays (a float32 restatement of the pinhole and the orthographic ray) and the id planes
                                                of an ANALYTIC scene under them: intersections in float64, rounded once
  case(W, H, pair, ortho=False)                 the fixed inputs the CPU tests run: two views of the scene (PAIRS), a noisy accumulator, a history image
"""
import numpy as np

from denoise_reference import TABLE_DTYPE, bits, guide, share_differing  # noqa: F401  (bits / share_differing: for the tests)

f32 = np.float32
DEFAULTS = dict(max_history=f32(16.0), until_samples=64, normal_cos=f32(np.cos(np.deg2rad(25.0))), depth_ratio=f32(1.05))
WRONG = ("no_half_pixel", "nearest", "no_flip", "z_for_distance", "no_renorm", "no_depth", "no_cap")
PAIRS = ("sideways", "rotation", "dolly", "third_out", "half_turn")
SIZES = [(67, 45), (1, 1), (5, 300)]
T_MISS = np.finfo(f32).max                      # what the id buffer holds for a miss: the ray's tmax


def _finite3(img):
    return np.isfinite(img[..., 0]) & np.isfinite(img[..., 1]) & np.isfinite(img[..., 2])


def reproject(a, rays, ob, tr, t, hist, table, max_history=DEFAULTS["max_history"], until_samples=64, normal_cos=DEFAULTS["normal_cos"],
              depth_ratio=DEFAULTS["depth_ratio"], wrong=None, stats=None):
    a = np.ascontiguousarray(a, f32)
    out = a.copy()
    if hist is None:
        return out
    ob, tr, t = np.asarray(ob, np.int32), np.asarray(tr, np.int32), np.asarray(t, f32)
    H, W = ob.shape
    G1 = guide(ob, tr, t, table)
    G0 = guide(np.asarray(hist["ob"], np.int32), np.asarray(hist["tr"], np.int32), np.asarray(hist["t"], f32), table)
    himg = np.ascontiguousarray(hist["rgba"], f32)
    F = hist["frame"]
    eye, right, up, fwd = (np.asarray(F[k], f32) for k in ("eye", "right", "up", "fwd"))
    tan_half, aspect, ortho_scale = f32(F["tan_half"]), f32(F["aspect"]), f32(F["ortho_scale"])
    rays = np.ascontiguousarray(rays, f32).reshape(H, W, 8)
    o, d = rays[..., 0:3], rays[..., 4:7]
    w1 = a[..., 3]
    through = (tr < 0) | ~_finite3(a) | (w1 >= f32(until_samples))
    with np.errstate(all="ignore"):
        # PROJECT
        q = [(o[..., k] + t * d[..., k]) - eye[k] for k in range(3)]
        dot3 = lambda v: (q[0] * v[0] + q[1] * v[1]) + q[2] * v[2]
        x, y, z = dot3(right), dot3(up), dot3(fwd)
        if not int(F["is_ortho"]):
            ok = z > 0
            den = z * tan_half
            ny, nx = y / den, x / (den * aspect)
            te = z if wrong == "z_for_distance" else np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        else:
            ny, nx = y / ortho_scale, x / (ortho_scale * aspect)
            te = z
            ok = te > 0
        half = f32(0.0) if wrong == "no_half_pixel" else f32(0.5)
        fx = (nx + f32(1.0)) * (f32(0.5) * f32(W)) - half
        fy = ((ny + f32(1.0)) if wrong == "no_flip" else (f32(1.0) - ny)) * (f32(0.5) * f32(H)) - half
        assert fx.dtype == f32 and fy.dtype == f32 and te.dtype == f32
        ok &= np.isfinite(fx) & np.isfinite(fy) & (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        if wrong == "nearest":
            ax, ay = (ax >= f32(0.5)).astype(f32), (ay >= f32(0.5)).astype(f32)
        x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
        live = ok & ~through
        # GATHER
        bx, by = f32(1.0) - ax, f32(1.0) - ay
        wgt = (bx * by, ax * by, bx * ay, ax * ay)
        S, sn = np.zeros((H, W), f32), np.zeros((H, W), f32)
        sc = np.zeros((H, W, 3), f32)
        n_taps = np.zeros((H, W), np.int32)
        refused, refused_depth = np.zeros((H, W), bool), np.zeros((H, W), bool)      # pixels that were refused a usable tap by the object test / by the depth test
        for j in range(4):
            qx, qy = x0 + (j & 1), y0 + (j >> 1)
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            h = himg[cy, cx]
            wj = wgt[j]
            usable = inside & (h[..., 3] > 0) & _finite3(h) & (wj > 0)
            same_object = G0["ob"][cy, cx] == G1["ob"]
            old_hit = G0["tr"][cy, cx] >= 0
            same_tri = G0["tr"][cy, cx] == G1["tr"]
            n, m = G1["n"], G0["n"][cy, cx]
            dot = (n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]
            normal_ok = G1["has_n"] & G0["has_n"][cy, cx] & (np.abs(dot) >= f32(normal_cos))
            t0 = G0["t"][cy, cx]
            lo, hi = np.where(te < t0, te, t0), np.where(te < t0, t0, te)
            scaled = lo * f32(depth_ratio)
            assert scaled.dtype == f32 and dot.dtype == f32
            step = np.zeros((H, W), bool) if wrong == "no_depth" else (hi > scaled)
            match = same_object & old_hit & (same_tri | (normal_ok & ~step))
            take = live & usable & match
            refused |= live & usable & ~same_object
            refused_depth |= live & usable & same_object & old_hit & ~same_tri & normal_ok & (hi > scaled)
            S = np.where(take, S + wj, S)
            sc = np.where(take[..., None], sc + wj[..., None] * h[..., :3], sc)
            sn = np.where(take, sn + wj * h[..., 3], sn)
            n_taps += take
        assert S.dtype == f32 and sc.dtype == f32 and sn.dtype == f32
        took = live & (n_taps > 0)
        if wrong == "no_renorm":
            hc, hq = sc, sn
        else:
            hc, hq = sc / S[..., None], sn / S
        hn = hq if wrong == "no_cap" else np.where(hq < f32(max_history), hq, f32(max_history))
        # BLEND
        W2 = w1 + hn
        blended = np.concatenate([(a[..., :3] * w1[..., None] + hc * hn[..., None]) / W2[..., None], W2[..., None]], -1)
        alone = np.concatenate([hc, hn[..., None]], -1)
        res = np.where((w1 > 0)[..., None], blended, alone)
        assert res.dtype == f32
    out.view(np.uint32)[took] = res.view(np.uint32)[took]          # bits, not values: pass-through pixels keep their NaN payloads
    if stats is not None:
        stats.update(hit=int((tr >= 0).sum()), live=int(live.sum()), took=int(took.sum()), refused=int(((refused | refused_depth) & (tr >= 0)).sum()),
                     refused_object=int(refused.sum()), refused_depth=int(refused_depth.sum()),
                     fewer_than_four=int((took & (n_taps < 4)).sum()), four=int((took & (n_taps == 4)).sum()), projected=int((ok & (tr >= 0)).sum()),
                     capped=int((took & (hq >= f32(max_history))).sum()), unsampled_took=int((took & ~(w1 > 0)).sum()), n_taps=n_taps, took_mask=took)
    return out


# ------------------------------------------------------------------------------------------------ cameras and the analytic scene
def make_frame(eye, target, W, H, fovy_deg=40.0, ortho_scale=None, up=(0.0, 0.0, 1.0)):
    """the camera frame the rule takes, computed in float64 and rounded once (the tests need a frame, not the library's rounding of it)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    return dict(eye=eye.astype(f32), right=right.astype(f32), up=upv.astype(f32), fwd=fwd.astype(f32), tan_half=f32(np.tan(np.deg2rad(fovy_deg) / 2.0)),
                aspect=f32(f32(W) / f32(H)), ortho_scale=f32(0.0 if ortho_scale is None else ortho_scale), is_ortho=0 if ortho_scale is None else 1)


def rays_of(F, W, H):
    """(H * W, 8) float32 {o.xyz, tmax, d.xyz, 0}: the pixel-centre ray of every pixel, row-major -- the pinhole and the orthographic ray in float32"""
    py, px = np.mgrid[0:H, 0:W]
    nx = ((px.astype(f32) + f32(0.5)) / f32(W)) * f32(2.0) - f32(1.0)
    ny = ((py.astype(f32) + f32(0.5)) / f32(H)) * f32(-2.0) + f32(1.0)
    rays = np.zeros((H, W, 8), f32)
    rays[..., 3] = T_MISS
    if F["is_ortho"]:
        sx, sy = (nx * F["ortho_scale"]) * F["aspect"], ny * F["ortho_scale"]
        rays[..., 0:3] = F["eye"] + sx[..., None] * F["right"] + sy[..., None] * F["up"]
        rays[..., 4:7] = F["fwd"]
    else:
        sx, sy = (nx * F["tan_half"]) * F["aspect"], ny * F["tan_half"]
        d = F["fwd"] + sx[..., None] * F["right"] + sy[..., None] * F["up"]
        rays[..., 0:3] = F["eye"]
        rays[..., 4:7] = d / np.sqrt((d * d).sum(-1, dtype=f32))[..., None]
    assert rays.dtype == f32
    return rays.reshape(-1, 8)


# The scene: object 0 is a floor z = 0 over [-4, 4]^2 (triangles 0, 1, split along x == y) with a raised terrace z = 0.9 over x > 2 (triangles 4, 5: the SAME object
# and the same normal, so only the depth test tells it from the floor); object 1 is a quad z = 1 over [-0.8, 0.8]^2 (triangles 2, 3) that hides part of the floor.
SLABS = ((0.0, (-4.0, 4.0), (-4.0, 4.0), 0, 0), (0.9, (2.0, 4.0), (-4.0, 4.0), 0, 4), (1.0, (-0.8, 0.8), (-0.8, 0.8), 1, 2))      # z, x range, y range, object, first triangle
TABLE = np.zeros(6, TABLE_DTYPE)
TABLE["n"][:, 2] = 1.0
TABLE["v"] = np.arange(18).reshape(6, 3)


def view_of(F, W, H):
    """rays and id planes of the scene under frame F: intersections in float64 from the float32 rays, the nearest one per pixel, rounded once"""
    rays = rays_of(F, W, H)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    best_t = np.full(len(rays), np.inf)
    ob, tr = np.full(len(rays), -1, np.int32), np.full(len(rays), -1, np.int32)
    with np.errstate(all="ignore"):
        for z, (xa, xb), (ya, yb), obj, tri0 in SLABS:
            tt = (z - o[:, 2]) / d[:, 2]
            p = o + tt[:, None] * d
            hit = (tt > 1e-6) & (p[:, 0] >= xa) & (p[:, 0] < xb) & (p[:, 1] >= ya) & (p[:, 1] < yb) & (tt < best_t)
            best_t = np.where(hit, tt, best_t)
            ob = np.where(hit, obj, ob).astype(np.int32)
            tr = np.where(hit, tri0 + (p[:, 0] - xa > p[:, 1] - ya), tr).astype(np.int32)
    t = np.where(tr >= 0, best_t, T_MISS).astype(f32)
    return dict(rays=rays, ob=ob.reshape(H, W), tr=tr.reshape(H, W), t=t.reshape(H, W))


def camera_pair(pair, W, H, ortho=False):
    """(frame of the current view, frame of the history's view)"""
    eye, target = np.array([0.3, -6.0, 4.0]), np.array([0.3, 0.0, 0.3])
    kw = dict(ortho_scale=3.0) if ortho else {}
    now = make_frame(eye, target, W, H, **kw)
    side = np.array([1.0, 0.0, 0.0])
    if pair == "sideways":
        old = make_frame(eye - 0.45 * side, target - 0.45 * side, W, H, **kw)
    elif pair == "rotation":
        old = make_frame(eye, target + np.array([0.25, 0.0, 0.12]), W, H, **kw)
    elif pair == "dolly":
        old = make_frame(eye - 0.9 * (target - eye) / np.linalg.norm(target - eye), target, W, H, ortho_scale=3.4) if ortho else \
            make_frame(eye - 0.9 * (target - eye) / np.linalg.norm(target - eye), target, W, H)
    elif pair == "third_out":
        old = make_frame(eye - 1.9 * side, target - 1.9 * side, W, H, **kw)
    elif pair == "half_turn":
        old = make_frame(eye, eye - (target - eye), W, H, **kw)
        if ortho:                                   # an orthographic camera sees what lies in front of its PLANE: step back behind everything as well
            old = make_frame(eye + 40.0 * (eye - target) / np.linalg.norm(eye - target), eye + 80.0 * (eye - target), W, H, **kw)
    else:
        raise ValueError(pair)
    return now, old


def images(r, W, H, until_samples):
    """a noisy accumulator of 1 spp mostly -- some pixels unsampled, some beyond until_samples, a few not finite -- and a history image with counts on both sides of
    max_history, some empty and a few not finite"""
    a = np.zeros((H, W, 4), f32)
    a[..., :3] = r.gamma(0.7, 1.2, (H, W, 3)).astype(f32)
    counts = np.array([1, 1, 1, 1, 1, 1, 2, 3, 7, until_samples - 1, until_samples, until_samples + 5], f32)
    a[..., 3] = counts[r.integers(0, len(counts), (H, W))]
    u = r.random((H, W))
    a[u < 0.06, 3] = 0.0
    a[(u >= 0.06) & (u < 0.065), 3] = f32(-1.0)
    v = r.random((H, W))
    a[v < 0.01, 0] = f32(np.inf)
    a[(v >= 0.01) & (v < 0.02), 1] = f32(np.nan)
    h = np.zeros((H, W, 4), f32)
    h[..., :3] = r.gamma(0.7, 1.2, (H, W, 3)).astype(f32)
    hc = np.array([1, 1, 2, 3, 5, 9, 15.5, 16, 17, 40], f32)
    h[..., 3] = hc[r.integers(0, len(hc), (H, W))]
    u = r.random((H, W))
    h[u < 0.05, 3] = 0.0
    h[(u >= 0.05) & (u < 0.055), 3] = f32(-2.0)
    v = r.random((H, W))
    h[v < 0.01, 2] = f32(np.inf)
    h[(v >= 0.01) & (v < 0.02), 0] = f32(np.nan)
    return a, h


def case(W, H, pair, ortho=False, seed=0):
    now, old = camera_pair(pair, W, H, ortho)
    v1, v0 = view_of(now, W, H), view_of(old, W, H)
    r = np.random.default_rng(1000 * W + H + seed + 7 * PAIRS.index(pair) + (100 if ortho else 0))
    a, h = images(r, W, H, DEFAULTS["until_samples"])
    return dict(a=a, rays=v1["rays"], ob=v1["ob"], tr=v1["tr"], t=v1["t"], hist=dict(rgba=h, ob=v0["ob"], tr=v0["tr"], t=v0["t"], frame=old), table=TABLE, now=now)
