"""The denoised display, restated in numpy from the text of include/cadrays_hip.h ("denoised display"), not from the C++.

Everything here is integer work or float32 arithmetic of single operations -- one product, one sum, one division at a time, each rounded as C rounds it: no
transcendental, no fused multiply-add.  So the library's bytes are expected to be EQUAL to these, and no tolerance appears.

  guide(ob, tr, t, table)                       has_n and the normal under every pixel
  one_pass(img, k, G, ...)                      pass k, all 25 taps as whole-image shifts, summed in the rule's order
  denoise(rgba, ob, tr, t, table, levels, normal_cos, depth_ratio, until_samples, wrong=None, stats=None)
                                                every pass; wrong = one of WRONG: a deliberately broken rule; stats: a dict that receives, per level, why taps were
                                                dropped, why pixels passed through and how many taps the filtered pixels accepted
  case(W, H) / main_case() / exact_case()       the fixed planes / tables the CPU tests run
"""
import numpy as np

f32 = np.float32
TABLE_DTYPE = np.dtype([("n", "<f4", (3,)), ("degenerate", "<u4"), ("v", "<u4", (3,)), ("pad", "<u4")])
DEFAULTS = dict(levels=4, normal_cos=f32(np.cos(np.deg2rad(25.0))), depth_ratio=f32(1.05), until_samples=256)
H5 = (1, 4, 6, 4, 1)
# "norm256" is NOT in this list: see test_denoise.py -- scaling every weight by the power of two 1 / 256 commutes with every rounding, so it cannot change a bit
WRONG = ("order", "normalised", "fma", "signed_dot", "ge", "no_4k")
DROP_REASONS = ("border", "unsampled", "non_finite", "object", "normal", "depth")
PASS_REASONS = ("miss", "unsampled", "non_finite", "enough_samples")


def guide(ob, tr, t, table):
    tab = np.zeros(0, TABLE_DTYPE) if table is None else np.asarray(table, TABLE_DTYPE)
    n_tri = len(tab)
    in_table = (tr >= 0) & (tr < n_tri)
    rec = tab[np.where(in_table, tr, 0)] if n_tri else np.zeros(tr.shape, TABLE_DTYPE)
    has_n = in_table & (rec["degenerate"] == 0)
    return dict(ob=ob, tr=tr, t=t, has_n=has_n, n=np.ascontiguousarray(rec["n"], f32))


def _finite3(img):
    return np.isfinite(img[..., 0]) & np.isfinite(img[..., 1]) & np.isfinite(img[..., 2])


def _fmaf(a, b, c):
    """a * b + c with one rounding (the product of two float32 is exact in float64; the sum's double rounding cannot be told from one here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def one_pass(img, k, G, normal_cos, depth_ratio, until_samples, wrong=None, stats=None):
    H, W = G["ob"].shape
    s = 1 << k
    w = img[..., 3]
    with np.errstate(all="ignore"):
        scaled_w = w * f32(1 << (2 * k))
        assert scaled_w.dtype == f32
        enough = ~((w if wrong == "no_4k" else scaled_w) < f32(until_samples))
    miss, unsampled, nonfin = G["tr"] < 0, ~(w > 0), ~_finite3(img)
    through = miss | unsampled | nonfin | enough
    yy, xx = np.mgrid[0:H, 0:W]
    sr = np.zeros((H, W, 3), f32)
    wsum = np.zeros((H, W), np.uint32)
    n_taps = np.zeros((H, W), np.int32)
    drops = dict.fromkeys(DROP_REASONS, 0)
    offsets = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
    if wrong == "order":
        offsets = [(dy, dx) for dx in range(-2, 3) for dy in range(-2, 3)]
    taps = []
    for dy, dx in offsets:
        qy, qx = yy + dy * s, xx + dx * s
        inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
        q = img[cy, cx]
        q_unsampled, q_nonfin = ~(q[..., 3] > 0), ~_finite3(q)
        same_object = G["ob"] == G["ob"][cy, cx]
        both_hit = (G["tr"] >= 0) & (G["tr"][cy, cx] >= 0)
        same_tri = G["tr"] == G["tr"][cy, cx]
        n, m = G["n"], G["n"][cy, cx]
        with np.errstate(all="ignore"):
            dot = (n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]
            assert dot.dtype == f32
            normal_ok = G["has_n"] & G["has_n"][cy, cx] & ((dot if wrong == "signed_dot" else np.abs(dot)) >= f32(normal_cos))
            ta, tb = G["t"], G["t"][cy, cx]
            lo, hi = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            scaled = lo * f32(depth_ratio)
            assert scaled.dtype == f32
            step = (hi >= scaled) if wrong == "ge" else (hi > scaled)
        sim = same_object & both_hit & (same_tri | (normal_ok & ~step))
        take = inside & ~q_unsampled & ~q_nonfin & sim & ~through
        c = H5[dy + 2] * H5[dx + 2]
        taps.append((take, c, q))
        wsum += np.where(take, np.uint32(c), np.uint32(0)).astype(np.uint32)
        n_taps += take
        if stats is not None:
            live = ~through
            drops["border"] += int((live & ~inside).sum())
            drops["unsampled"] += int((live & inside & q_unsampled).sum())
            drops["non_finite"] += int((live & inside & ~q_unsampled & q_nonfin).sum())
            drops["object"] += int((live & inside & ~same_object).sum())
            drops["normal"] += int((live & inside & same_object & both_hit & ~same_tri & ~normal_ok).sum())
            drops["depth"] += int((live & inside & same_object & both_hit & ~same_tri & normal_ok & step).sum())
    with np.errstate(all="ignore"):
        for take, c, q in taps:
            if wrong == "normalised":
                wgt = (f32(c) / wsum.astype(f32))[..., None]                  # the weight normalised first ...
                new = sr + wgt * q[..., :3]
            elif wrong == "fma":
                new = _fmaf(np.broadcast_to(f32(c), q[..., :3].shape), q[..., :3], sr)
            else:
                prod = f32(c) * q[..., :3]                                     # the product rounded ...
                new = sr + prod                                                # ... then the sum rounded
            assert new.dtype == f32
            sr = np.where(take[..., None], new, sr)
        rgb = sr if wrong == "normalised" else sr / wsum.astype(f32)[..., None]   # ... and no division at the end
    assert rgb.dtype == f32
    out = img.copy()
    filt = ~through
    assert (wsum[filt] >= 36).all()                                            # the centre always counts
    out.view(np.uint32)[..., :3][filt] = rgb.view(np.uint32)[filt]             # bits, not values: pass-through pixels keep their NaN payloads
    if stats is not None:
        stats.setdefault("levels", []).append(dict(
            drops=drops, filtered=int(filt.sum()), hit=int((~miss).sum()), two_or_more=int((filt & (n_taps >= 2)).sum()),
            through=dict(miss=int(miss.sum()), unsampled=int((~miss & unsampled).sum()), non_finite=int((~miss & ~unsampled & nonfin).sum()),
                         enough_samples=int((~miss & ~unsampled & ~nonfin & enough).sum()))))
    return out


def denoise(rgba, ob, tr, t, table, levels=4, normal_cos=DEFAULTS["normal_cos"], depth_ratio=DEFAULTS["depth_ratio"], until_samples=256, wrong=None, stats=None):
    img = np.ascontiguousarray(rgba, f32).copy()
    G = guide(np.asarray(ob, np.int32), np.asarray(tr, np.int32), np.asarray(t, f32), table)
    for k in range(int(levels)):
        img = one_pass(img, k, G, normal_cos, depth_ratio, until_samples, wrong, stats)
    return img


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def share_differing(a, b):
    """the share of pixels in which the two images differ in any bit"""
    return float((bits(a) != bits(b)).any(-1).mean())


# ------------------------------------------------------------------------------------------------ fixed cases
def random_table(r, n_tri):
    """normals in four loose bundles, so that different triangles often pass the normal test and often fail it; every 5th wound the other way round; every 11th
    record degenerate (and its normal zero, as the library writes it)"""
    base = np.array([(0, 0, 1), (0, 1, 0), (0.6, 0, 0.8), (0.3, 0.3, 0.9)], np.float64)
    n = base[np.arange(n_tri) % 4] + r.normal(0.0, 0.1, (n_tri, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[np.arange(n_tri) % 5 == 2] *= -1.0
    tab = np.zeros(n_tri, TABLE_DTYPE)
    tab["n"] = n.astype(f32)
    tab["degenerate"] = (np.arange(n_tri) % 11 == 5).astype(np.uint32)
    tab["n"][tab["degenerate"] == 1] = 0
    tab["v"] = r.integers(0, 3 * n_tri, (n_tri, 3))
    return tab


def planes(r, W, H, n_objects, n_tri):
    """patches of equal triangles (the taps of a coarse step need neighbours 32 pixels away), ~15 % misses in patches, triangle ids beyond the table, distances that
    are EXACT ratios apart across many triangle borders, objects that mostly follow the triangles"""
    by, bx = np.arange(H)[:, None] // 5, np.arange(W)[None, :] // 9
    patch = (by * 131 + bx * 17 + (by * bx) % 7)
    tr = (patch % (n_tri + 3)).astype(np.int32)                                  # the last three ids lie beyond the table
    noise = r.random((H, W)) < 0.08
    tr[noise] = r.integers(0, n_tri + 3, int(noise.sum()))
    ob = (tr % n_objects).astype(np.int32)                                       # triangles 12 apart share the object (n_objects = 3) and the normal bundle
    ob[r.random((H, W)) < 0.03] = int(r.integers(0, n_objects))
    base = np.array([2.0, 3.0, 2.5, 4.5, 3.0, 3.1, 2.6, 3.0], f32)[tr % 8]       # ... and their distances are 2 and 3, 4.5 and 3 (2 * 1.5 == 3, 3 * 1.5 == 4.5 exactly), or close
    t = np.where(r.random((H, W)) < 0.6, base, base * (1 + 0.04 * r.random((H, W)))).astype(f32)
    miss = ((patch % 7) == 3) | (r.random((H, W)) < 0.02)
    ob[miss] = -1; tr[miss] = -1; t[miss] = f32(1e15)
    return ob, tr, t


def colours(r, W, H):
    """a noisy image of 1 - 3 spp mostly, sample counts on both sides of every level's threshold, a few pixels unsampled, a few not finite"""
    rgba = np.zeros((H, W, 4), f32)
    rgba[..., :3] = r.gamma(0.7, 1.2, (H, W, 3)).astype(f32)
    counts = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 5, 20, 100, 300, 2000], f32)
    rgba[..., 3] = counts[r.integers(0, len(counts), (H, W))]
    u = r.random((H, W))
    rgba[u < 0.04, 3] = 0.0
    rgba[(u >= 0.04) & (u < 0.045), 3] = f32(-1.0)
    rgba[(u >= 0.045) & (u < 0.05), 3] = f32(np.nan)
    v = r.random((H, W))
    rgba[v < 0.01, 0] = f32(np.inf)
    rgba[(v >= 0.01) & (v < 0.02), 1] = f32(np.nan)
    rgba[(v >= 0.02) & (v < 0.025), 2] = f32(-np.inf)
    return rgba


def case(W, H, seed=0, n_objects=3, n_tri=41):
    r = np.random.default_rng(1000 * W + H + seed)
    tab = random_table(r, n_tri)
    ob, tr, t = planes(r, W, H, n_objects, n_tri)
    return dict(rgba=colours(r, W, H), ob=ob, tr=tr, t=t, table=tab)


# the main case: five levels, all of them active (until_samples = 1024: level 4 works below 4 samples), a depth ratio that the planes' distances hit exactly
MAIN_PARAMS = dict(levels=5, normal_cos=f32(np.cos(np.deg2rad(25.0))), depth_ratio=f32(1.5), until_samples=1024)
SIZES = [(1, 1), (1, 7), (5, 300), (67, 45), (130, 3)]


def main_case():
    return case(67, 45)


def exact_case(W=40, H=24):
    """two coplanar neighbouring objects, each of several triangles, with constant colours whose floats have at most 12 significant bits: every product c * colour
    (c <= 36) and every partial sum (<= 256 * colour) is exact, and so is the division of the full sum by its weight"""
    ob = np.zeros((H, W), np.int32); ob[:, W // 2:] = 1
    tr = (np.arange(H)[:, None] // 4 * 8 + np.arange(W)[None, :] // 5).astype(np.int32)
    t = np.full((H, W), 3.0, f32)
    tab = np.zeros(int(tr.max()) + 1, TABLE_DTYPE)
    tab["n"][:, 2] = 1.0
    col = np.array([[0.7998046875, 0.0999755859375, 1.5], [0.2001953125, 3.998046875, 0.0625]], f32)      # 4095 / 5120 ... : 12 significant bits at most
    m, e = np.frexp(col)
    assert np.array_equal(np.round(m * 4096), m * 4096)
    rgba = np.zeros((H, W, 4), f32)
    rgba[..., :3] = col[ob]
    rgba[..., 3] = 1.0
    return dict(rgba=rgba, ob=ob, tr=tr, t=t, table=tab)
