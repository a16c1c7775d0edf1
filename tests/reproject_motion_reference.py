"""Per-object history deltas of the reprojected display history, restated in numpy from the text of include/cadrays_hip.h ("per-object history deltas"), not from
the C++.

The delta table is float64 arithmetic of single operations on Python floats (IEEE doubles: one product, one difference, one sum, one division at a time, no fused
multiply-add), each of the twelve results rounded once to float32; the rule is float32 arithmetic of single operations as in reproject_reference.py.  So the library's
bytes are expected to be EQUAL to these, and no tolerance appears.

  delta_table(xf_hist, xf_cur, wrong=None)      the table (DELTA_DTYPE records); wrong = "inverse_direction" / "transposed": a deliberately broken table
  reproject_motion(a, rays, ob, tr, t, hist, table, delta, max_history_moved, max_history_static, ..., wrong=None, stats=None)
                                                the rule; delta = None or a table; wrong = one of WRONG_RULE: a deliberately broken rule
  view_of / case                                the analytic scene of reproject_reference.py with object 1 (the quad) under a 3x4 transform: intersections in
                                                float64 in the quad's object space, rounded once
"""
import numpy as np

import reproject_reference as base
from denoise_reference import guide
from reproject_reference import DEFAULTS, SLABS, TABLE, T_MISS, _finite3, bits, camera_pair, images, make_frame, rays_of, share_differing  # noqa: F401

f32 = np.float32
DELTA_DTYPE = np.dtype([("D", "<f4", (12,)), ("flag", "<u4"), ("pad", "<u4", (3,))])
MOTION_DEFAULTS = dict(max_history_moved=f32(16.0), max_history_static=f32(8.0))
WRONG_TABLE = ("inverse_direction", "transposed")
WRONG_RULE = ("no_delta", "cap_wrong_class", "cap_when_unflagged")
SIZES = [(61, 37), (1, 1), (5, 300)]
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _record(A, M):
    """(D as twelve Python floats or None, flag) of one object: A = X_hist, M = X_cur, both twelve float32"""
    if A.tobytes() == M.tobytes():
        return None, 0
    M = [float(v) for v in M]
    A = [float(v) for v in A]
    r0, r1, r2, t = (M[0], M[1], M[2]), (M[4], M[5], M[6]), (M[8], M[9], M[10]), (M[3], M[7], M[11])
    c0, c1, c2 = _cross(r1, r2), _cross(r2, r0), _cross(r0, r1)
    det = _dot(r0, c0)
    if det == 0.0 or not np.isfinite(det):
        return None, 2
    with np.errstate(all="ignore"):
        det = np.float64(det)                       # numpy's division: Inf and NaN instead of exceptions
        i = [tuple(float(np.float64(c[k]) / det) for c in (c0, c1, c2)) for k in range(3)]
        u = [-_dot(i[j], t) for j in range(3)]
        D = []
        for j in range(3):
            a = A[4 * j:4 * j + 4]
            for m in range(3):
                D.append((a[0] * i[0][m] + a[1] * i[1][m]) + a[2] * i[2][m])
            D.append(((a[0] * u[0] + a[1] * u[1]) + a[2] * u[2]) + a[3])
        D32 = np.array(D, np.float64).astype(f32)
    if not np.isfinite(D32).all():
        return None, 2
    return D32, 1


def delta_table(xf_hist, xf_cur, wrong=None):
    xh, xc = np.ascontiguousarray(xf_hist, f32).reshape(-1, 12), np.ascontiguousarray(xf_cur, f32).reshape(-1, 12)
    out = np.zeros(len(xh), DELTA_DTYPE)
    for k in range(len(xh)):
        D, flag = _record(xc[k], xh[k]) if wrong == "inverse_direction" else _record(xh[k], xc[k])
        out["flag"][k] = flag
        if flag == 1:
            if wrong == "transposed":
                D = np.concatenate([D.reshape(3, 4)[:, :3].T, D.reshape(3, 4)[:, 3:]], 1).reshape(12)
            out["D"][k] = D
    return out


def reproject_motion(a, rays, ob, tr, t, hist, table, delta, max_history_moved=MOTION_DEFAULTS["max_history_moved"], max_history_static=MOTION_DEFAULTS["max_history_static"],
                     max_history=DEFAULTS["max_history"], until_samples=64, normal_cos=DEFAULTS["normal_cos"], depth_ratio=DEFAULTS["depth_ratio"], wrong=None, stats=None):
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
    # the flag of every pixel's object; 0 outside the table, and everywhere without a table
    n_obj = 0 if delta is None else len(delta)
    inside_table = (ob >= 0) & (ob < n_obj)
    k_of = np.where(inside_table, ob, 0)
    flag = np.where(inside_table, delta["flag"][k_of], 0) if n_obj else np.zeros((H, W), np.uint32)
    capped = bool(n_obj and (delta["flag"] != 0).any())
    through = (tr < 0) | ~_finite3(a) | (w1 >= f32(until_samples)) | (flag == 2)
    with np.errstate(all="ignore"):
        # PROJECT
        P = [o[..., k] + t * d[..., k] for k in range(3)]
        if n_obj and wrong != "no_delta":
            D = delta["D"][k_of]                                                 # (H, W, 12)
            moved = [((D[..., 4 * k] * P[0] + D[..., 4 * k + 1] * P[1]) + D[..., 4 * k + 2] * P[2]) + D[..., 4 * k + 3] for k in range(3)]
            P = [np.where(flag == 1, moved[k], P[k]) for k in range(3)]
        assert all(p.dtype == f32 for p in P)
        q = [P[k] - eye[k] for k in range(3)]
        dot3 = lambda v: (q[0] * v[0] + q[1] * v[1]) + q[2] * v[2]
        x, y, z = dot3(right), dot3(up), dot3(fwd)
        if not int(F["is_ortho"]):
            ok = z > 0
            den = z * tan_half
            ny, nx = y / den, x / (den * aspect)
            te = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        else:
            ny, nx = y / ortho_scale, x / (ortho_scale * aspect)
            te = z
            ok = te > 0
        fx = (nx + f32(1.0)) * (f32(0.5) * f32(W)) - f32(0.5)
        fy = (f32(1.0) - ny) * (f32(0.5) * f32(H)) - f32(0.5)
        assert fx.dtype == f32 and fy.dtype == f32 and te.dtype == f32
        ok &= np.isfinite(fx) & np.isfinite(fy) & (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
        live = ok & ~through
        # GATHER
        bx, by = f32(1.0) - ax, f32(1.0) - ay
        wgt = (bx * by, ax * by, bx * ay, ax * ay)
        S, sn = np.zeros((H, W), f32), np.zeros((H, W), f32)
        sc = np.zeros((H, W, 3), f32)
        n_taps = np.zeros((H, W), np.int32)
        refused_object = np.zeros((H, W), bool)
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
            step = hi > lo * f32(depth_ratio)
            match = same_object & old_hit & (same_tri | (normal_ok & ~step))
            take = live & usable & match
            refused_object |= live & usable & ~same_object
            S = np.where(take, S + wj, S)
            sc = np.where(take[..., None], sc + wj[..., None] * h[..., :3], sc)
            sn = np.where(take, sn + wj * h[..., 3], sn)
            n_taps += take
        assert S.dtype == f32 and sc.dtype == f32 and sn.dtype == f32
        took = live & (n_taps > 0)
        hc, hq = sc / S[..., None], sn / S
        hn = np.where(hq < f32(max_history), hq, f32(max_history))
        # CAP
        is_moved = (flag == 0) if wrong == "cap_wrong_class" else (flag == 1)
        cap = np.where(is_moved, f32(max_history_moved), f32(max_history_static)).astype(f32)
        hn_uncapped = hn
        if capped or wrong == "cap_when_unflagged":
            hn = np.where(hn < cap, hn, cap)
        # BLEND
        W2 = w1 + hn
        blended = np.concatenate([(a[..., :3] * w1[..., None] + hc * hn[..., None]) / W2[..., None], W2[..., None]], -1)
        alone = np.concatenate([hc, hn[..., None]], -1)
        res = np.where((w1 > 0)[..., None], blended, alone)
        assert res.dtype == f32
    out.view(np.uint32)[took] = res.view(np.uint32)[took]          # bits, not values: pass-through pixels keep their NaN payloads
    if stats is not None:
        bound = took & (hn < hn_uncapped)
        stats.update(took=int(took.sum()), took_moved=int((took & (flag == 1)).sum()), took_static=int((took & (flag == 0)).sum()), flagged_hit=int(((flag == 1) & (tr >= 0)).sum()),
                     static_refused_all=int((live & (flag == 0) & refused_object & (n_taps == 0)).sum()), cap_bound_moved=int((bound & (flag == 1)).sum()),
                     cap_bound_static=int((bound & (flag == 0)).sum()), no_history_object=int(((flag == 2) & (tr >= 0)).sum()), took_mask=took, flag=flag)
    return out


# ------------------------------------------------------------------------------------------------ the analytic scene with a moved quad
def xform(rows):
    return np.asarray(rows, np.float64).reshape(12).astype(f32)


def _inverse64(X):
    M = np.asarray(X, np.float64).reshape(3, 4)
    Ai = np.linalg.inv(M[:, :3])
    return Ai, -Ai @ M[:, 3]


def view_of(F, W, H, X1):
    """rays and id planes under frame F with object 1 (the quad) under the 3x4 transform X1: the static slabs as reproject_reference.view_of intersects them, the quad in
    its own object space (an affine map keeps the ray parameter), everything in float64 from the float32 rays, the nearest hit per pixel, rounded once"""
    rays = rays_of(F, W, H)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    Ai, ti = _inverse64(X1)
    best_t = np.full(len(rays), np.inf)
    ob, tr = np.full(len(rays), -1, np.int32), np.full(len(rays), -1, np.int32)
    with np.errstate(all="ignore"):
        for z, (xa, xb), (ya, yb), obj, tri0 in SLABS:
            oo, dd = (o @ Ai.T + ti, d @ Ai.T) if obj == 1 else (o, d)
            tt = (z - oo[:, 2]) / dd[:, 2]
            p = oo + tt[:, None] * dd
            hit = (tt > 1e-6) & (p[:, 0] >= xa) & (p[:, 0] < xb) & (p[:, 1] >= ya) & (p[:, 1] < yb) & (tt < best_t)
            best_t = np.where(hit, tt, best_t)
            ob = np.where(hit, obj, ob).astype(np.int32)
            tr = np.where(hit, tri0 + (p[:, 0] - xa > p[:, 1] - ya), tr).astype(np.int32)
    t = np.where(tr >= 0, best_t, T_MISS).astype(f32)
    return dict(rays=rays, ob=ob.reshape(H, W), tr=tr.reshape(H, W), t=t.reshape(H, W))


_c, _s = np.cos(np.deg2rad(20.0)), np.sin(np.deg2rad(20.0))
# (X_hist, X_cur) of the quad: a slide across the floor; a turn about z with a non-uniform scale and a lift, from a placement that was itself off the identity
CONFIGS = {
    "slide": (IDENTITY, xform([[1, 0, 0, 0.55], [0, 1, 0, 0.3], [0, 0, 1, 0]])),
    "turn_scale": (xform([[1, 0, 0, -0.2], [0, 1, 0, 0.1], [0, 0, 1, 0.05]]), xform([[1.3 * _c, -0.8 * _s, 0, 0.35], [1.3 * _s, 0.8 * _c, 0, -0.25], [0, 0, 1.1, 0.1]])),
}


def case(W, H, config, ortho=False, camera_moved=False, seed=0):
    """the fixed inputs the CPU tests run: the history's view with the quad at X_hist, the current view with the quad at X_cur, a noisy accumulator, a history image"""
    now, old = camera_pair("sideways", W, H, ortho)
    if not camera_moved:
        old = now
    xh, xc = CONFIGS[config]
    v1, v0 = view_of(now, W, H, xc), view_of(old, W, H, xh)
    r = np.random.default_rng(1000 * W + H + seed + 13 * sorted(CONFIGS).index(config) + (100 if ortho else 0) + (50 if camera_moved else 0))
    a, h = images(r, W, H, DEFAULTS["until_samples"])
    xf_hist, xf_cur = np.stack([IDENTITY, xh]), np.stack([IDENTITY, xc])
    return dict(a=a, rays=v1["rays"], ob=v1["ob"], tr=v1["tr"], t=v1["t"], hist=dict(rgba=h, ob=v0["ob"], tr=v0["tr"], t=v0["t"], frame=old), table=TABLE, now=now,
                xf_hist=xf_hist, xf_cur=xf_cur)
