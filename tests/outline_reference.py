"""Feature lines on the display, restated in numpy from the text of include/cadrays_hip.h ("feature lines on the display"), not from the C++.

Everything here is integer work, float64 arithmetic whose every operation numpy rounds as C does, or float32 arithmetic of single operations: no transcendental, no
fused multiply-add.  So the library's bytes are expected to be EQUAL to these, and no tolerance appears.

  table(pos, tri)                               the per-triangle records (abi.OUTLINE_TABLE_DTYPE)
  mask(ob, tr, t, table, crease_cos, depth_ratio, wrong=None)   the mask over PAIRS, scattered (the library gathers); wrong = one of WRONG: a deliberately broken rule
  draw(mask, ldr, kinds, width, rgb, alpha)     the drawing rule
  cases()                                       the fixed planes / tables the CPU tests run
"""
import numpy as np

f32 = np.float32
OBJECT, DEPTH, CREASE = 1, 2, 4
TABLE_DTYPE = np.dtype([("n", "<f4", (3,)), ("degenerate", "<u4"), ("v", "<u4", (3,)), ("pad", "<u4")])
DEFAULT_COS, DEFAULT_RATIO = f32(np.cos(np.deg2rad(30.0))), f32(1.02)
WRONG = ("farther", "ignore_shared", "signed_dot", "ge", "fma")


def table(pos, tri):
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3).astype(np.float64)
    v = np.asarray(tri).reshape(-1, 4)[:, :3].astype(np.int64)
    p0, p1, p2 = pos[v[:, 0]], pos[v[:, 1]], pos[v[:, 2]]
    a, b = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        ok = (l > 0) & np.isfinite(l)
        n = c / np.where(ok, l, 1.0)[:, None]
    out = np.zeros(len(v), TABLE_DTYPE)
    out["n"] = np.where(ok[:, None], n, 0.0).astype(f32)
    out["degenerate"] = (~ok).astype(np.uint32)
    out["v"] = v.astype(np.uint32)
    return out


def _fmaf(a, b, c):
    """a * b + c with one rounding (the product of two float32 is exact in float64; the sum's double rounding cannot be told from one here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _pair(oa, ob, ta, tb, da, db, tab, crease_cos, depth_ratio, wrong):
    """kinds of every pair (a, b) of the arrays"""
    k = np.zeros(oa.shape, np.uint8)
    k[oa != ob] = OBJECT
    n_tri = len(tab)
    if n_tri == 0:
        return k
    same = (oa == ob) & (ta >= 0) & (tb >= 0) & (ta != tb) & (ta < n_tri) & (tb < n_tri)
    A, B = tab[np.where(same, ta, 0)], tab[np.where(same, tb, 0)]
    shared = (A["v"][..., :, None] == B["v"][..., None, :]).any(axis=(-1, -2))
    if wrong == "ignore_shared":
        shared = np.zeros_like(shared)
    lo, hi = np.minimum(da, db), np.maximum(da, db)
    scaled = lo * f32(depth_ratio)                            # one float32 product
    assert scaled.dtype == f32
    step = (hi >= scaled) if wrong == "ge" else (hi > scaled)
    k[same & ~shared & step] |= DEPTH
    n, m = A["n"], B["n"]
    if wrong == "fma":
        dot = _fmaf(n[..., 2], m[..., 2], _fmaf(n[..., 1], m[..., 1], n[..., 0] * m[..., 0]))
    else:
        dot = (n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]
    assert dot.dtype == f32
    sharp = (dot < f32(crease_cos)) if wrong == "signed_dot" else (np.abs(dot) < f32(crease_cos))
    k[same & (A["degenerate"] == 0) & (B["degenerate"] == 0) & sharp] |= CREASE
    return k


def mask(ob, tr, t, tab, crease_cos=DEFAULT_COS, depth_ratio=DEFAULT_RATIO, wrong=None):
    ob, tr, t = np.asarray(ob, np.int32), np.asarray(tr, np.int32), np.asarray(t, f32)
    tab = np.zeros(0, TABLE_DTYPE) if tab is None else tab
    m = np.zeros(ob.shape, np.uint8)
    for sa, sb in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        k = _pair(ob[sa], ob[sb], tr[sa], tr[sb], t[sa], t[sb], tab, crease_cos, depth_ratio, wrong)
        to_b = t[sb] < t[sa]                                  # the nearer pixel; a tie goes to a
        if wrong == "farther":
            to_b = ~to_b
        m[sb] |= np.where(to_b, k, 0).astype(np.uint8)
        m[sa] |= np.where(to_b, 0, k).astype(np.uint8)
    return m


def draw(msk, ldr, kinds=7, width=1, rgb=(0, 0, 0), alpha=255):
    msk, ldr = np.asarray(msk, np.uint8), np.asarray(ldr, np.uint8)
    H, W = msk.shape
    on = (msk & np.uint8(kinds)) != 0
    lo, hi = -((width - 1) // 2), width // 2                 # [-floor((w - 1) / 2), ceil((w - 1) / 2)]
    drawn = np.zeros((H, W), bool)
    for dy in range(lo, hi + 1):
        for dx in range(lo, hi + 1):
            # drawn[y, x] |= on[y + dy, x + dx] where that pixel exists
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                drawn[y0:y1, x0:x1] |= on[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    col = np.array(rgb, np.uint32)
    v = ldr.astype(np.uint32)
    new = np.broadcast_to(col, v.shape) if alpha == 255 else (v * (256 - alpha) + col * alpha + 128) >> 8
    return np.where(drawn[..., None], new, v).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ fixed cases
SIZES = [(1, 1), (1, 7), (7, 1), (64, 2), (65, 9), (61, 37), (130, 67)]


def random_table(r, n_tri, share):
    """n_tri triangles over random vertices; a fraction `share` of the triangles reuses a vertex index of its predecessor; every 11th is degenerate"""
    nv = 3 * n_tri
    pos = r.uniform(-2.0, 2.0, (nv, 3)).astype(f32)
    tri = np.zeros((n_tri, 4), np.int32)
    tri[:, :3] = np.arange(nv).reshape(-1, 3)
    for k in range(1, n_tri):
        if r.random() < share:
            tri[k, int(r.integers(0, 3))] = tri[k - 1, int(r.integers(0, 3))]
        if k % 11 == 5:
            tri[k, 1] = tri[k, 0]                                # two equal vertices
    tri[:, 3] = r.integers(0, 4, n_tri)
    return pos, tri


def planes(r, W, H, n_objects, n_tri, runs=True):
    """random planes: ~20 % misses; runs of equal triangles; equal t across some pairs; triangle ids beyond the table; objects consistent with nothing in particular"""
    tr = r.integers(0, n_tri + max(n_tri // 8, 2), (H, W)).astype(np.int32)        # some ids beyond the table
    if runs:
        keep = r.random((H, W)) < 0.5
        for x in range(1, W):
            tr[:, x] = np.where(keep[:, x], tr[:, x - 1], tr[:, x])
        keep = r.random((H, W)) < 0.25
        for y in range(1, H):
            tr[y] = np.where(keep[y], tr[y - 1], tr[y])
    ob = (tr.astype(np.int64) * 2654435761 % n_objects).astype(np.int32)           # a triangle belongs to one object
    ob[r.random((H, W)) < 0.1] = int(r.integers(0, n_objects))                     # ... except where it does not (the rule does not care)
    t = r.uniform(0.5, 40.0, (H, W)).astype(f32)
    t = np.where(r.random((H, W)) < 0.4, np.round(t), t).astype(f32)               # equal t across pairs, and steps that are exact ratios
    miss = r.random((H, W)) < 0.2
    ob[miss] = -1; tr[miss] = -1; t[miss] = f32(1e15)
    return ob, tr, t


def fma_table():
    """two triangles whose normals' dot product differs between the plain float32 sum and the fused one, and the threshold that tells them apart"""
    r = np.random.default_rng(77)
    while True:
        pos = r.uniform(-1.0, 1.0, (6, 3)).astype(f32)
        tri = np.array([(0, 1, 2, 0), (3, 4, 5, 0)], np.int32)
        tab = table(pos, tri)
        n, m = tab["n"][0], tab["n"][1]
        plain = np.abs((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2])
        fused = np.abs(_fmaf(n[2:3], m[2:3], _fmaf(n[1:2], m[1:2], n[0:1] * m[0:1]))[0])
        if plain != fused and 0.05 < plain < 0.95:
            return pos, tri, tab, f32(max(plain, fused))     # the smaller of the two is a crease, the larger is not


def cases():
    """(name, ob, tr, t, table, crease_cos, depth_ratio): random planes of every size and object count, plus the hand-made ones that make each rule bite"""
    out = []
    for W, H in SIZES:
        for n_objects in (1, 7, 5000):
            for share in (0.0, 0.5, 0.95):
                r = np.random.default_rng(W * 1000 + H * 10 + n_objects + int(share * 100))
                n_tri = 40
                pos, tri = random_table(r, n_tri, share)
                ob, tr, t = planes(r, W, H, n_objects, n_tri)
                out.append((f"random_{W}x{H}_{n_objects}_{share}", ob, tr, t, table(pos, tri), DEFAULT_COS, DEFAULT_RATIO))
    # one object, two unconnected triangles, t an EXACT ratio apart: `>` draws nothing, `>=` would
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)], f32)
    tri = np.array([(0, 1, 2, 0), (3, 4, 5, 0)], np.int32)
    flat = table(pos, tri)
    ob = np.zeros((2, 4), np.int32); tr = np.array([[0, 0, 1, 1], [0, 1, 1, 0]], np.int32); t = np.where(tr == 0, f32(1.0), f32(1.5)).astype(f32)
    out.append(("exact_ratio", ob, tr, t, flat, DEFAULT_COS, f32(1.5)))
    out.append(("just_above_ratio", ob, tr, t, flat, DEFAULT_COS, np.nextafter(f32(1.5), f32(0))))
    # the same two triangles wound the other way round (normals opposite): no crease through the absolute value
    tri_flipped = np.array([(0, 1, 2, 0), (3, 5, 4, 0)], np.int32)
    out.append(("opposite_winding", ob, tr, np.ones((2, 4), f32), table(pos, tri_flipped), DEFAULT_COS, DEFAULT_RATIO))
    # two triangles that share ONE vertex index, at a depth step
    tri_shared = np.array([(0, 1, 2, 0), (2, 4, 5, 0)], np.int32)
    out.append(("shared_vertex_step", ob, tr, t, table(pos, tri_shared), DEFAULT_COS, DEFAULT_RATIO))
    # a dot product on the threshold
    pos, tri, tab, cc = fma_table()
    out.append(("fma_threshold", ob, tr, np.ones((2, 4), f32), tab, cc, DEFAULT_RATIO))
    return out
