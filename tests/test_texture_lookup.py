"""sample_texture (cadrays_amd/csrc/k_lights_env.h, oracle/crh_oracle.c) against the float64 restatement of tests/lookup_reference.py, on two
sides with the SAME cases and bounds:
  cpu  the oracle
  gpu  the gfx950 kernels through View(0); there every image must also be bit-equal to the oracle's

HOW THE LOOKUP IS OBSERVED: a 16 x 16 grid of quads whose four vertices carry the same uv, so a quad shows the texture at that uv wherever a ray
hits it; an orthographic view onto 64 x 64 pixels (4 x 4 per cell), Lambert Kd 0.9 under a unit background, max_depth 2, 4 samples.  A sample is
Kd x texel(uv); the inner 2 x 2 pixels of each cell must lie within Kd D + Kd K 2^-24 of Kd x the reference (D: lookup_reference.texture_ref,
K: camera_reference.LAMBERT_K; the four samples of a pixel are equal, so their running mean adds nothing).
One scene holds three texture slots of different sizes (one of them RGBA with alpha 1) and fifteen materials (slot x scale); neighbouring cells take
different materials, so a wrong slot offset, a wrong scale or a wrong size shows.

Measured on the cpu side (the gpu's bits are the same), per (slot set, gamma): see WORST_SEEN; a case whose D exceeds 5 % of the texture's value range
proves nothing beyond "a texel of that image" (the coordinates next to 2^22, where one ulp is half a repeat): their share is printed, and no case
with |u scale| < 2^16 may be among them.
"""
import numpy as np
import pytest

from cadrays_amd import scenes

import camera_reference as C
import lookup_reference as L
from camera_reference import LAMBERT_K

F32 = np.float32
N, RES, SPP, KD = 16, 64, 4, 0.9
EXCUSE, WRONG_MIN = 0.05, 0.05
SCALES = ((1.0, 1.0), (0.0, 0.0), (3.0, 2.0), (-2.0, 0.5), (1e30, 3e38))
# worst err / bound and excused share, cpu side: (slot set, gamma) -> (ratio, share)
WORST_SEEN = {("A", 0): (0.361, 0.0331), ("A", 1): (0.141, 0.0331), ("B", 0): (0.375, 0.0425), ("B", 1): (0.303, 0.0425)}
CAM = scenes.Camera(eye=(0, 0, 3), dir=(0, 0, -1), up=(0, 1, 0), is_ortho=True, ortho_scale=1.0)
PAR = scenes.Params(width=RES, height=RES, tile_size=8, max_depth=2, background=(1.0, 1.0, 1.0))


def rng(seed):
    return np.random.default_rng(seed)


def slot_sets():
    """name -> three images (H, W, C) of different sizes; the last one RGBA with alpha 1"""
    r = rng(31)

    def img(w, h, c=3):
        a = r.random((h, w, c)).astype(F32)
        if c == 4:
            a[..., 3] = 1.0
        return a
    return {"A": [img(1, 1), img(5, 7), img(64, 32, 4)], "B": [img(1, 4), img(4, 1), img(16, 16, 4)]}


def materials():
    """(material list, [(slot, scale)]): material k = slot k % 3 with scale k // 3"""
    what = [(k % 3, SCALES[k // 3]) for k in range(15)]
    return [C.lambert(KD, s, sc) for s, sc in what], what


def ulps_around(x):
    """x - 2 ulp, x, x + 2 ulp in float32"""
    b = F32(x)
    return [np.nextafter(np.nextafter(b, F32(-np.inf)), F32(-np.inf)), b, np.nextafter(np.nextafter(b, F32(np.inf)), F32(np.inf))]


DIRECTED = [F32(v) for v in (-3, -2, -1, 0.0, -0.0, 1, 2, 3, -1e-30, 1 - 2.0 ** -24, 4194303.5, -4194303.5, 4194304, -4194304, 3e9, -7.5e12, 0.5)]


def uv_cases(W, H, seed):
    """the (u, v) float32 pairs one material is asked for, and the slice of them that sits on texel centres at scale 1"""
    r = rng(seed)
    rand = lambda n: r.uniform(-3, 3, n).astype(F32)
    out = [(d, v) for d, v in zip(DIRECTED, rand(len(DIRECTED)))] + [(u, d) for d, u in zip(DIRECTED, rand(len(DIRECTED)))]
    out += [(d, d) for d in DIRECTED]
    c0 = len(out)
    n = max(W, H)
    out += [(F32((i % W + 0.5) / W), F32((i % H + 0.5) / H)) for i in range(n)]                   # texel centres: (column i % W, row H - 1 - i % H)
    c1 = len(out)
    for i in sorted({0, 1, W // 2, W - 1, W}):                                                      # texel boundaries +- 2 ulp
        out += [(b, v) for b, v in zip(ulps_around(i / W), rand(3))]
    for i in sorted({0, 1, H // 2, H - 1, H}):
        out += [(u, b) for b, u in zip(ulps_around(i / H), rand(3))]
    out += list(zip(rand(30), rand(30)))
    return out, slice(c0, c1)


def case_table(images):
    """every (material, u, v) of a slot set, flat: arrays mat (n,), uv (n, 2), centre (n,) bool"""
    _, what = materials()
    mat, uv, centre = [], [], []
    for k, (slot, scale) in enumerate(what):
        H, W, _ = images[slot].shape
        cases, cs = uv_cases(W, H, 100 + k)
        mat += [k] * len(cases); uv += cases
        c = np.zeros(len(cases), bool)
        if scale in ((1.0, 1.0), (0.0, 0.0)):
            c[cs] = True
        centre += list(c)
    order = rng(7).permutation(len(mat))                                                            # neighbouring cells: different materials and slots
    return np.array(mat)[order], np.array(uv, F32)[order], np.array(centre)[order]


def reference(images, mat, uv, gamma2, wrong=None):
    """(value (n, 4), D (n, 4), span (n, 4)) of every case"""
    _, what = materials()
    pool = np.concatenate([L.rgba(im).reshape(-1, 4) for im in images])
    val, D, span = np.zeros((len(mat), 4)), np.zeros((len(mat), 4)), np.zeros((len(mat), 4))
    for k, (slot, scale) in enumerate(what):
        sel = mat == k
        val[sel], D[sel] = L.texture_ref(images[slot], uv[sel, 0], uv[sel, 1], scale, gamma2, wrong=wrong, pool=pool)
        a = L.rgba(images[slot])
        a = np.concatenate([a[..., :3] ** 2, a[..., 3:]], 2) if gamma2 else a
        span[sel] = a.max((0, 1)) - a.min((0, 1))
    return val, D, span


def page_scene(images, mat, uv):
    """one grid = 256 cases (the rest of the last page: material 0 at uv 1/2, not checked); cell (i, j) = case j * 16 + i"""
    m = np.zeros(N * N, int); u = np.full((N * N, 2), 0.5, F32)
    m[:len(mat)] = mat; u[:len(mat)] = uv
    return C.cell_grid_scene(N, u.reshape(N, N, 2), materials()[0], m.reshape(N, N), list(images), CAM, PAR)


def inner_pixels(img, n):
    """the inner 2 x 2 pixels of the first n cells: (n, 4, 3); cell (i, j) covers columns 4 i .. 4 i + 3 and rows 63 - 4 j - 3 .. 63 - 4 j"""
    k = np.arange(n); i, j = k % N, k // N
    px = (4 * i[:, None] + np.array([1, 2, 1, 2]))
    py = (RES - 1 - (4 * j[:, None] + np.array([1, 1, 2, 2])))
    return img[py, px]


class Side:
    def __init__(self, name, ctx, twin=None):
        self.name, self.ctx, self.twin = name, ctx, twin

    def image(self, sc, gamma2):
        imgs = []
        for b in (self.ctx, self.twin):
            if b is None:
                continue
            b.load_scene(sc); b.set_spec(texel_gamma2=gamma2); b.render(SPP)
            imgs.append(b.read_hdr())
        if self.twin is not None:
            assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), "gpu != oracle"
        return imgs[0].astype(np.float64)

    def close(self):
        for b in (self.ctx, self.twin):
            if b is not None:
                b.close()


@pytest.fixture(scope="module", params=[pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def side(request, oracle_lib):
    if request.param == "cpu":
        s = Side("cpu", oracle_lib.Oracle())
    else:
        request.getfixturevalue("hip_lib")
        from cadrays_amd.view import View
        s = Side("gpu", View(0), oracle_lib.Oracle())
    yield s
    s.close()


def judge(got, val, D, span):
    """got (n, 4 pixels, 3): (err / bound per case, excused per case)"""
    bound = KD * D[:, None, :3] + KD * LAMBERT_K * 2.0 ** -24
    ratio = (np.abs(got - KD * val[:, None, :3]) / bound).max((1, 2))
    excused = ((D[:, :3] > EXCUSE * span[:, :3]) & (span[:, :3] > 0)).any(1)
    return ratio, excused


@pytest.mark.parametrize("gamma2", [0, 1])
@pytest.mark.parametrize("which", ["A", "B"])
def test_texture_lookup_within_bound(side, which, gamma2):
    images = slot_sets()[which]
    mat, uv, centre = case_table(images)
    val, D, span = reference(images, mat, uv, gamma2)
    got = np.concatenate([inner_pixels(side.image(page_scene(images, mat[a:a + N * N], uv[a:a + N * N]), gamma2), min(N * N, len(mat) - a))
                          for a in range(0, len(mat), N * N)])
    ratio, excused = judge(got, val, D, span)
    print(f"texture_lookup[{side.name} {which} g{gamma2}]: {len(mat)} cases, worst err/bound {ratio.max():.3f}, excused share {excused.mean():.4f}")
    bad = ratio > 1
    assert not bad.any(), [(mat[i], uv[i], got[i, 0], KD * val[i, :3], D[i, :3]) for i in np.flatnonzero(bad)[:4]]
    # only a coordinate whose ulp is a visible part of a repeat may be excused (|u scale| >= 2^16: an ulp is 1/256 repeat and more)
    _, what = materials()
    scale = np.array([[c if c != 0 else 1.0 for c in what[k][1]] for k in mat])
    with np.errstate(over="ignore"):
        scaled = np.abs(uv.astype(np.float64) * scale)
    assert not excused[(scaled < 2.0 ** 16).all(1)].any()
    # a texel centre shows the texel itself
    for i in np.flatnonzero(centre):
        im = L.rgba(images[what[mat[i]][0]]); H, W, _ = im.shape
        col, row = int(np.floor(float(uv[i, 0]) * W)), H - 1 - int(np.floor(float(uv[i, 1]) * H))
        t = im[row, col, :3] ** 2 if gamma2 else im[row, col, :3]
        assert np.abs(val[i, :3] - t).max() <= 1e-6 and not excused[i]
    # coordinates beyond 2^22, or overflowing with the scale, sample at 0: decided cases, like any other (2^22 itself is excused: the blend of three
    # equal values may come out one ulp = half a repeat below it)
    far = (scaled >= 2 * L.GUARD).all(1)
    assert far.any() and not excused[far].any()


def test_lambert_weight_constant(side):
    """the K of the bound: a constant texture c under Kd against the float64 product (LAMBERT_K allows twice the worst seen on the cpu side)"""
    worst = 0.0
    for kd in (0.9, 0.5, 0.73):
        for c in (1.0, 0.3, 0.77, 0.123):
            sc = C.cell_grid_scene(N, np.full((N, N, 2), 0.3), [C.lambert(kd, 0)], np.zeros((N, N), int), [np.full((4, 4, 3), c, F32)], CAM, PAR)
            img = side.image(sc, 0)
            worst = max(worst, np.abs(img - float(F32(kd)) * float(F32(c))).max() / (float(F32(kd)) * 2.0 ** -24))
    print(f"lambert weight[{side.name}]: worst K {worst:.3f} (allowed {LAMBERT_K})")
    assert worst <= LAMBERT_K


def test_wrong_rules_are_caught():
    for which, images in slot_sets().items():
        mat, uv, _ = case_table(images)
        for gamma2 in (0, 1):
            val, D, _ = reference(images, mat, uv, gamma2)
            bound = KD * D[:, :3] + KD * LAMBERT_K * 2.0 ** -24
            for wrong in ("half_texel", "nearest", "v_not_flipped", "slot_offset_0"):
                bad, _, _ = reference(images, mat, uv, gamma2, wrong=wrong)
                share = (KD * np.abs(bad[:, :3] - val[:, :3]) > bound).any(1).mean()
                print(f"wrong rule {wrong} on {which} g{gamma2}: violates the bound on {share:.3f} of {len(mat)}")
                assert share >= WRONG_MIN, (wrong, which, gamma2, share)
