"""Region queries on the first-hit id buffer, restated in numpy from the text of include/cadrays_hip.h ("region queries"), not from the C++.

  region    = rectangle (half-open, cut to the frame; None = the whole frame) intersected with the polygon (None = none)
  polygon   = even-odd, exact in integers: vertex (2x, 2y), pixel centre (2 px + 1, 2 py + 1); an edge a -> b counts iff (a.y < cy) != (b.y < cy) and
              cross * sign(b.y - a.y) > 0 with cross = (b.x - a.x)(cy - a.y) - (cx - a.x)(b.y - a.y)   [int64 here as there]
  records   = per object, background (misses and ids outside [0, n_objects)) last: pixels, pixels_frame, half-open box, t_min / t_max of the pixels inside
  selection = pixels >= max(min_pixels, 1) [TOUCHED]  and pixels == pixels_frame [ENCLOSED]
"""
import numpy as np

STATS_DTYPE = np.dtype([("pixels", "<u4"), ("pixels_frame", "<u4"), ("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4"), ("t_min", "<f4"), ("t_max", "<f4")])
TOUCHED, ENCLOSED = 0, 1


def polygon_mask(poly, W, H):
    """(H, W) bool: the pixels whose centre the polygon holds"""
    P = 2 * np.asarray(poly, np.int64).reshape(-1, 2)
    cx = (2 * np.arange(W, dtype=np.int64) + 1)[None, :]
    cy = (2 * np.arange(H, dtype=np.int64) + 1)[:, None]
    inside = np.zeros((H, W), bool)
    for k in range(len(P)):
        a, b = P[k], P[(k + 1) % len(P)]
        crosses = (a[1] < cy) != (b[1] < cy)
        cross = (b[0] - a[0]) * (cy - a[1]) - (cx - a[0]) * (b[1] - a[1])
        inside ^= crosses & (cross * np.sign(b[1] - a[1]) > 0)
    return inside


def rect_mask(rect, W, H):
    m = np.zeros((H, W), bool)
    if rect is None:
        m[:] = True
        return m
    x0, y0, x1, y1 = [int(v) for v in rect]
    assert x0 <= x1 and y0 <= y1
    m[min(y0, H):min(y1, H), min(x0, W):min(x1, W)] = True
    return m


def region_mask(W, H, rect=None, poly=None):
    m = rect_mask(rect, W, H)
    return m if poly is None else m & polygon_mask(poly, W, H)


def stats(object_px, t_px, n_objects, rect=None, poly=None):
    ob, t = np.asarray(object_px, np.int64), np.asarray(t_px, np.float32)
    H, W = ob.shape
    m = region_mask(W, H, rect, poly)
    slot = np.where((ob >= 0) & (ob < n_objects), ob, n_objects)
    out = np.zeros(n_objects + 1, STATS_DTYPE)
    out["pixels_frame"] = np.bincount(slot.ravel(), minlength=n_objects + 1)
    out["pixels"] = np.bincount(slot[m], minlength=n_objects + 1)
    ys, xs = np.nonzero(m)
    s = slot[m]
    big = np.iinfo(np.int64).max
    x0, y0 = np.full(n_objects + 1, big), np.full(n_objects + 1, big)
    x1, y1 = np.zeros(n_objects + 1, np.int64), np.zeros(n_objects + 1, np.int64)
    np.minimum.at(x0, s, xs); np.minimum.at(y0, s, ys); np.maximum.at(x1, s, xs + 1); np.maximum.at(y1, s, ys + 1)
    tmin, tmax = np.full(n_objects + 1, np.inf, np.float32), np.zeros(n_objects + 1, np.float32)
    np.minimum.at(tmin, s, t[m]); np.maximum.at(tmax, s, t[m])
    some = out["pixels"] > 0
    for name, v in (("x0", x0), ("y0", y0), ("x1", x1), ("y1", y1)):
        out[name][some] = v[some]
    some[n_objects] = False                                    # the background has no distance
    out["t_min"][some] = tmin[some]; out["t_max"][some] = tmax[some]
    return out


def select(st, mode, min_pixels):
    st = st[:-1]
    sel = st["pixels"] >= max(int(min_pixels), 1)
    if mode == ENCLOSED:
        sel &= st["pixels"] == st["pixels_frame"]
    return sel.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the regions every comparison runs (CPU and GPU)
def pentagram(cx, cy, r):
    a = np.deg2rad(-90 + 144 * np.arange(5))
    return np.stack([np.rint(cx + r * np.cos(a)), np.rint(cy + r * np.sin(a))], 1).astype(np.int32)


def regions(W, H):
    """[(name, rect or None, polygon or None)]"""
    r = np.random.default_rng(W * 1000 + H)
    m = min(W, H)
    out = [("null", None, None), ("full", (0, 0, W, H), None), ("one_pixel", (W // 2, H // 2, W // 2 + 1, H // 2 + 1), None),
           ("beyond", (W // 3, H // 4, W + 50, H + 9), None), ("outside", (W + 5, H + 5, W + 20, H + 30), None), ("empty", (W // 2, H // 2, W // 2, H // 2 + 1), None)]
    P = {
        "triangle": [(1, 0), (W - 1, H // 2), (W // 3, H)],
        "concave_L": [(0, 0), (W // 3 + 1, 0), (W // 3 + 1, H // 2), (W, H // 2), (W, H), (0, H)],
        "pentagram": pentagram(W // 2, H // 2, max(m // 2, 1)),
        "bow_tie": [(0, 0), (W, H), (W, 0), (0, H)],
        "far_vertices": [(-(1 << 20), -(1 << 20)), ((1 << 20), -(1 << 20) + 3), (W // 2, (1 << 20))],
        "diagonal_through_centres": [(0, 0), (m, m), (0, m)],
        "repeated_vertex": [(0, 0), (W, 0), (W, 0), (W // 2, H), (W // 2, H), (0, 0)],
        "horizontal_edges": [(0, 1), (W // 2, 1), (W, 1), (W, H // 2), (W // 2, H // 2), (W // 2, H), (W // 4, H), (0, H)],
        "random_256": np.stack([r.integers(-3, W + 4, 256), r.integers(-3, H + 4, 256)], 1),
    }
    out += [(n, None, np.asarray(p, np.int32)) for n, p in P.items()]
    out.append(("pentagram_in_rect", (W // 4, 0, W, H - H // 3), np.asarray(P["pentagram"], np.int32)))
    out.append(("random_256_outside_rect", (0, 0, 0, 0), np.asarray(P["random_256"], np.int32)))
    return out
