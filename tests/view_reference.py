"""The viewport read-out's rule, restated in numpy from the text of include/cadrays_hip.h (section "viewport read-out"): per-axis tap lists in Python integers,
the per-pixel sums in int64 (a channel's sum stays below 2^37), the exact rounded quotient.  Nothing here was derived from the library's output.

  taps(i, s, v, off, S, filter)     the (frame index, weight) pairs of output index i of one axis, and the divisor D
  view(ldr, vw, vh, src, filter)    the resampled image
  fit(W, H, aw, ah)                 the letterbox, in float32
  to_frame(...)                     the NEAREST tap of both axes
  WRONG                             three deliberately wrong rules: each must change at least one image of the case list
"""
import numpy as np

AUTO, NEAREST, BILINEAR, AREA = 0, 1, 2, 3
FILTERS = (AUTO, NEAREST, BILINEAR, AREA)
MAX_SIDE = 8192

FRAME = (37, 23)                                                                           # W, H of the random frame of the host-twin cases
VIEWS = ((37, 23), (18, 11), (19, 12), (74, 46), (53, 31), (1, 1), (37, 1), (1, 23), (111, 5))
RECTS = ((0, 0, 0, 0), (5, 4, 20, 15), (36, 22, 37, 23), (7, 7, 8, 8))                     # whole, a window, the last pixel, one pixel inside


def resolve(filter, s, v):
    return (AREA if s >= v else BILINEAR) if filter == AUTO else filter


def taps(i, s, v, off, S, filter, wrong=None):
    """[(frame index, weight)], D -- Python integers throughout"""
    i, s, v, off, S = int(i), int(s), int(v), int(off), int(S)
    f = resolve(filter, s, v)
    if f == AREA:
        lo, hi = i * s, (i + 1) * s
        return [(off + k, min((k + 1) * v, hi) - max(k * v, lo)) for k in range(lo // v, (hi - 1) // v + 1)], s
    if f == BILINEAR:
        n = 2 * i * s if wrong == "no_half_pixel" else (2 * i + 1) * s - v
        k0 = n // (2 * v)                                                                   # Python's // is the floor division
        fr = n - k0 * 2 * v
        lo, hi = (off, off + s - 1) if wrong == "clamp_to_rectangle" else (0, S - 1)
        clamp = lambda k: min(max(k, lo), hi)
        return [(clamp(off + k0), 2 * v - fr), (clamp(off + k0 + 1), fr)], 2 * v
    return [(off + ((2 * i + 1) * s) // (2 * v), 1)], 1


def rect_of(src, W, H):
    x0, y0, x1, y1 = (int(x) for x in src)
    return (0, 0, W, H) if not (x0 or y0 or x1 or y1) else (x0, y0, x1, y1)


def axis_matrix(s, v, off, S, filter, wrong=None):
    """(v, S) int64: row i holds the weights of output index i over the frame axis; the divisor"""
    M = np.zeros((v, S), np.int64)
    D = None
    for i in range(v):
        t, D = taps(i, s, v, off, S, filter, wrong)
        assert sum(w for _, w in t) == D and all(w >= 0 for _, w in t)
        for k, w in t:
            assert 0 <= k < S
            M[i, k] += w
    return M, D


def view(ldr, vw, vh, src=(0, 0, 0, 0), filter=AUTO, wrong=None):
    ldr = np.asarray(ldr)
    assert ldr.dtype == np.uint8 and ldr.ndim == 3 and ldr.shape[2] == 3
    H, W = ldr.shape[:2]
    x0, y0, x1, y1 = rect_of(src, W, H)
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and 1 <= vw <= MAX_SIDE and 1 <= vh <= MAX_SIDE
    MX, DX = axis_matrix(x1 - x0, vw, x0, W, filter, wrong)
    MY, DY = axis_matrix(y1 - y0, vh, y0, H, filter, wrong)
    D = DX * DY
    img = ldr.astype(np.int64)
    out = np.empty((vh, vw, 3), np.int64)
    for c in range(3):
        out[:, :, c] = MY @ img[:, :, c] @ MX.T                                             # sum_y w_y sum_x w_x byte, exact in int64
    q = out // D if wrong == "round_down" else (out + D // 2) // D
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)


WRONG = ("round_down", "clamp_to_rectangle", "no_half_pixel")


def fit(W, H, aw, ah):
    """the letterbox of the header's text, in float32; (vw, vh)"""
    f32 = np.float32
    aspect = f32(W) / f32(H)
    if f32(aw) / f32(ah) < aspect:
        vw, vh = int(aw), int(f32(aw) / aspect)                                             # int(): the truncation of the C cast (the values are positive)
    else:
        vw, vh = int(f32(ah) * aspect), int(ah)
    return max(vw, 1), max(vh, 1)


def to_frame(W, H, vx, vy, vw, vh, src=(0, 0, 0, 0)):
    x0, y0, x1, y1 = rect_of(src, W, H)
    return taps(vx, x1 - x0, vw, x0, W, NEAREST)[0][0][0], taps(vy, y1 - y0, vh, y0, H, NEAREST)[0][0][0]


def random_frame(W=FRAME[0], H=FRAME[1], seed=5):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def checkerboard(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def cases(frame_size=FRAME):
    """(vw, vh, src, filter) of the host-twin case list: 9 views x 4 rectangles x 4 filters = 144"""
    return [(vw, vh, r, f) for (vw, vh) in VIEWS for r in RECTS for f in FILTERS]


def scaled_rects(W, H):
    """the rectangles above scaled from the 37 x 23 frame to a W x H one: whole, a window, the last pixel, one pixel inside"""
    sx, sy = lambda x: x * W // FRAME[0], lambda y: y * H // FRAME[1]
    return ((0, 0, 0, 0), (sx(5), sy(4), sx(20), sy(15)), (W - 1, H - 1, W, H), (sx(7), sy(7), sx(7) + 1, sy(7) + 1))
