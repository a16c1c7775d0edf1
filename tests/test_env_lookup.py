"""env_lookup (cadrays_amd/csrc/k_lights_env.h, oracle/crh_oracle.c) against the float64 restatement of tests/lookup_reference.py, on two
sides with the SAME cases and bounds:
  cpu  the oracle
  gpu  the gfx950 kernels through View(0); there every image must also be bit-equal to the oracle's
The oracle is a transliteration of the kernels, so bit parity cannot see an error both share; this module can.

HOW THE LOOKUP IS OBSERVED: an orthographic camera with nothing in view (one tiny triangle behind the eye), max_depth 1, the map as
background, no lights.  Every sample of every pixel is then env_lookup(normalise(camera.dir)) whatever the jitter: one 8 x 8 image, one
tile, one sample per direction; the image must be uniform bit for bit and its value within D of the reference (lookup_reference.env_ref:
D is built from the map and the direction alone).

A case whose D exceeds 5 % of the map's value range proves nothing ("excused"): at most 1 % of a sweep, none of the directed cases.
Measured on the cpu side (the gpu's bits are the same), worst err / D and excused share per (orientation, gamma) sweep: see WORST_SEEN.
"""
import dataclasses

import numpy as np
import pytest

from cadrays_amd import scenes
from cadrays_amd.materials import BSDF

import lookup_reference as L

F32 = np.float32
EXCUSE = 0.05                           # D above this share of the map's value range proves nothing
EXCUSED_MAX = 0.01                      # at most this share of a sweep (and no directed case)
WRONG_MIN = 0.05                        # a wrong rule must violate the bound on at least this share of the sweep
# worst err / D over every map of the sweep, cpu side: (orientation, gamma) -> value; excused share 0 in all four
WORST_SEEN = {(0, 0): 0.227, (0, 1): 0.214, (1, 0): 0.217, (1, 1): 0.211}
BG = (0.25, 0.5, 0.125)


def rng(seed):
    return np.random.default_rng(seed)


def empty_scene(env):
    pos = F32([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]])
    nrm = F32([[0, 0, 1]] * 3)
    tri = np.array([[0, 1, 2, 0]], np.int32)
    return scenes.Scene(pos, nrm, tri, [BSDF.CreateDiffuse(0.5)], env=env, camera=camera_along(F32([0, 1, 0])),
                        params=scenes.Params(width=8, height=8, tile_size=8, max_depth=1, background=BG, env_as_background=True), name="empty")


def camera_along(d):
    """orthographic, looking along d from 10 units down the direction: the triangle at the origin lies behind the eye"""
    d64 = np.asarray(d, np.float64)
    n = d64 / np.linalg.norm(d64)
    up = np.eye(3)[int(np.argmin(np.abs(n)))]
    return scenes.Camera(eye=tuple(10.0 * n), dir=tuple(float(c) for c in d), up=tuple(up), is_ortho=True, ortho_scale=1.0)


class Side:
    def __init__(self, name, ctx, twin=None):
        self.name, self.ctx, self.twin = name, ctx, twin

    def each(self):
        return [b for b in (self.ctx, self.twin) if b is not None]

    def setup(self, env, orientation, gamma2):
        for b in self.each():
            b.set_envmap(env)
            b.set_spec(env_orientation=orientation, texel_gamma2=gamma2)

    def look(self, d):
        """the image's one value along d; uniform bit for bit, and on the gpu the oracle's bits"""
        imgs = []
        for b in self.each():
            b.set_camera(camera_along(d)); b.reset(); b.render(1)
            imgs.append(b.read_hdr())
        flat = imgs[0].reshape(-1, 3).view(np.uint32)
        assert (flat == flat[0]).all(), ("not uniform", d)
        if self.twin is not None:
            assert np.array_equal(flat, imgs[1].reshape(-1, 3).view(np.uint32)), ("gpu != oracle", d)
        return imgs[0][0, 0].astype(np.float64)

    def sweep(self, dirs):
        return np.array([self.look(d) for d in dirs])

    def close(self):
        for b in self.each():
            b.close()


@pytest.fixture(scope="module", params=[pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def side(request, oracle_lib):
    sc = empty_scene(np.ones((1, 1, 3), F32))
    if request.param == "cpu":
        s = Side("cpu", oracle_lib.Oracle().load_scene(sc))
    else:
        request.getfixturevalue("hip_lib")
        from cadrays_amd.view import View
        s = Side("gpu", View(0).load_scene(sc), oracle_lib.Oracle().load_scene(sc))
    yield s
    s.close()


# ================================================================================================== maps and directions
def maps():
    r = rng(11)
    return {"random8x16": r.random((8, 16, 3)).astype(F32), "3x5": r.random((3, 5, 3)).astype(F32), "1x1": F32([[[0.3, 0.6, 0.9]]]),
            "1x4": r.random((1, 4, 3)).astype(F32), "2x1": r.random((2, 1, 3)).astype(F32), "sky": scenes.procedural_sky(512, 256, 1),
            "sky_dim": scenes.procedural_sky(512, 256, 1, sun=2.0)}


AXES = [F32(v) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
TILTS = (1e-7, 1e-6, 1e-5, 1e-4, 1e-3)


def pole_dirs():
    out = [F32([0, 0, 1]), F32([0, 0, -1]), F32([-0.0, 0.0, 1]), F32([0.0, -0.0, -1])]
    for s in (1, -1):
        for t in TILTS:
            for a in (0.3, 2.5, -1.9):
                out.append(F32([t * np.cos(a), t * np.sin(a), s]))
    return out


def seam_dirs():
    """the azimuth where atan2 jumps (x < 0, y = +-tiny: the map's seam under orientation 0, its middle under orientation 1) and the opposite one
    (x > 0: the middle under 0, the seam, where the texel coordinate turns negative, under 1)"""
    return [F32([sx, sy * t, z]) for sx in (-1, 1) for sy in (1, -1) for t in (0.0, 1e-40, 1e-30, 1e-7, 1e-3) for z in (0.0, 0.3)]


def centre_dirs(W, H, orientation, cells):
    return [L.env_texel_centre_dir(W, H, c, r, orientation) for r, c in cells]


def crossing_dirs(W, H, orientation):
    """9 steps of 1e-6 texel .. across a texel's edge and across its centre, along a row and along a column"""
    out = []
    steps = np.array([-1e-3, -1e-5, -1e-6, -1e-7, 0, 1e-7, 1e-6, 1e-5, 1e-3])
    for at in (3.0, 3.5):
        for k in steps:
            out.append(L.env_texel_centre_dir(W, H, at + k - 0.5, H // 2 - 0.3, orientation))
        if H > 2:
            for k in steps:
                out.append(L.env_texel_centre_dir(W, H, 2.2, at - 2 + k - 0.5, orientation))
    return out


def sphere_dirs(r, n):
    v = r.standard_normal((n, 3))
    return list((v / np.linalg.norm(v, axis=1)[:, None]).astype(F32))


def case_set(name, env, orientation):
    """(directed directions, random directions) for one map"""
    H, W, _ = env.shape
    r = rng(zlib_seed(name))
    every = [(row, col) for row in range(H) for col in range(W)]
    if name == "random8x16":
        return AXES + pole_dirs() + seam_dirs() + centre_dirs(W, H, orientation, every) + crossing_dirs(W, H, orientation), sphere_dirs(r, 90)
    if name == "3x5":
        return AXES + pole_dirs() + centre_dirs(W, H, orientation, every), sphere_dirs(r, 50)
    if name == "1x1":
        return AXES, sphere_dirs(r, 6)
    if name == "1x4":
        return AXES + seam_dirs()[::2] + centre_dirs(W, H, orientation, every), sphere_dirs(r, 20)
    if name == "2x1":
        return AXES + pole_dirs()[::2] + centre_dirs(W, H, orientation, every), sphere_dirs(r, 20)
    if name in ("sky", "sky_dim"):      # the sun of 5e4 sets the sky's Lx: its D says little away from the sun; the dim one is the same map with a sun of 2
        cells = [(int(a), int(b)) for a, b in zip(r.integers(0, H, 8), r.integers(0, W, 8))]
        return AXES + seam_dirs()[::2] + centre_dirs(W, H, orientation, cells), sphere_dirs(r, 40)
    raise KeyError(name)


def zlib_seed(name):
    import zlib
    return zlib.crc32(name.encode())


def value_range(env, gamma2):
    a = np.asarray(env, np.float64)
    a = a * a if gamma2 else a
    return a.max((0, 1)) - a.min((0, 1))


SWEEP_MAPS = ("random8x16", "3x5", "1x1", "1x4", "2x1", "sky", "sky_dim")


def all_cases(orientation):
    """[(map name, env, directions, n_directed)]"""
    m = maps()
    out = []
    for name in SWEEP_MAPS:
        directed, rand = case_set(name, m[name], orientation)
        out.append((name, m[name], directed + rand, len(directed)))
    return out


def judge(got, ref, D, span):
    """(err / D per case, excused per case): a case is excused where D exceeds EXCUSE of the range in some channel that has a range"""
    ratio = (np.abs(got - ref) / D).max(1)
    excused = ((D > EXCUSE * span) & (span > 0)).any(1)
    return ratio, excused


# ================================================================================================== the sweep
@pytest.mark.parametrize("gamma2", [0, 1])
@pytest.mark.parametrize("orientation", [0, 1])
def test_env_lookup_within_bound(side, orientation, gamma2):
    worst, n_all, n_exc = 0.0, 0, 0
    assert sum(len(c[2]) for c in all_cases(orientation)) <= 700
    for name, env, dirs, n_directed in all_cases(orientation):
        side.setup(env, orientation, gamma2)
        got = side.sweep(dirs)
        ref, D = L.env_ref(env, np.array(dirs), orientation, gamma2)
        ratio, excused = judge(got, ref, D, value_range(env, gamma2))
        assert not excused[:n_directed].any(), (name, "directed cases excused", np.flatnonzero(excused[:n_directed])[:8])
        bad = ratio > 1
        assert not bad.any(), (name, [(dirs[i], got[i], ref[i], D[i]) for i in np.flatnonzero(bad)[:4]])
        worst, n_all, n_exc = max(worst, ratio.max()), n_all + len(dirs), n_exc + int(excused.sum())
        print(f"env_lookup[{side.name} o{orientation} g{gamma2}] {name}: {len(dirs)} directions, worst err/D {ratio.max():.3f}, excused {excused.mean():.4f}")
        if name in ("random8x16", "3x5", "1x4", "2x1"):               # texel centres: the texel itself (the sharp test of the half-texel rule)
            H, W, _ = env.shape
            first = {"random8x16": len(AXES) + len(pole_dirs()) + len(seam_dirs()), "3x5": len(AXES) + len(pole_dirs()),
                     "1x4": len(AXES) + len(seam_dirs()[::2]), "2x1": len(AXES) + len(pole_dirs()[::2])}[name]
            texels = env.reshape(-1, 3).astype(np.float64)
            texels = texels * texels if gamma2 else texels
            sl = slice(first, first + H * W)
            assert (np.abs(got[sl] - texels) <= D[sl] + np.abs(ref[sl] - texels)).all() and np.abs(ref[sl] - texels).max() <= 1e-6, name
        if name == "random8x16":                                       # the crossings: continuous (no step beyond the reference's own)
            k = len(AXES) + len(pole_dirs()) + len(seam_dirs()) + 128
            for a in range(k, k + 36, 9):
                step, rstep = np.abs(np.diff(got[a:a + 9], axis=0)), np.abs(np.diff(ref[a:a + 9], axis=0))
                assert (step <= rstep + D[a:a + 8] + D[a + 1:a + 9]).all(), (name, a)
    print(f"env_lookup[{side.name} o{orientation} g{gamma2}]: worst err/D {worst:.3f}, excused share {n_exc / n_all:.4f}")
    assert n_exc <= EXCUSED_MAX * n_all


# ================================================================================================== directed
# What each axis looks at, as the contract words it (Scene.env: row 0 = zenith; crh_spec.h #14: u = (atan2(y, x) + pi) / 2 pi, so -X is the seam,
# +X the middle, +Y three quarters, -Y one quarter; the alternative: the map turned by half a turn and upside down).  On the 8-wide, 5-high
# compass the horizon is row 2 exactly, and every horizontal axis falls halfway between two columns: each gets weight 1/2.
COMPASS = {  # (orientation, axis) -> ((row, left column, right column) | row)
    (0, (1, 0, 0)): (2, 3, 4), (0, (-1, 0, 0)): (2, 7, 0), (0, (0, 1, 0)): (2, 5, 6), (0, (0, -1, 0)): (2, 1, 2), (0, (0, 0, 1)): 0, (0, (0, 0, -1)): 4,
    (1, (1, 0, 0)): (2, 7, 0), (1, (-1, 0, 0)): (2, 3, 4), (1, (0, 1, 0)): (2, 1, 2), (1, (0, -1, 0)): (2, 5, 6), (1, (0, 0, 1)): 4, (1, (0, 0, -1)): 0,
}


@pytest.mark.parametrize("orientation", [0, 1])
def test_compass(side, orientation):
    for (o, axis), where in COMPASS.items():
        if o != orientation:
            continue
        if isinstance(where, int):                                     # a pole: the whole row is lit (which column atan2(0, 0) picks is not the point)
            env = np.zeros((5, 8, 3), F32); env[where] = 1.0
            side.setup(env, orientation, 0)
            got = side.look(F32(axis))
            assert np.abs(got - 1.0).max() <= 1e-6, (orientation, axis, got)
            env = 1.0 - env
            side.setup(env, orientation, 0)
            assert np.abs(side.look(F32(axis))).max() <= 1e-6, (orientation, axis)
            continue
        row, left, right = where
        for col in (left, right):
            env = np.zeros((5, 8, 3), F32); env[row, col] = 1.0
            side.setup(env, orientation, 0)
            got = side.look(F32(axis))
            ref, D = L.env_ref(env, F32([axis]), orientation, 0)
            assert np.abs(got - 0.5).max() <= D.max() + 1e-6 and D.max() < 1e-5, (orientation, axis, col, got, D)
        env = np.ones((5, 8, 3), F32); env[row, left] = env[row, right] = 0.0
        side.setup(env, orientation, 0)
        assert np.abs(side.look(F32(axis))).max() <= 1e-5, (orientation, axis)


def test_background_when_the_map_is_not_the_background(side):
    """env_as_background = 0: the camera sees crh_params.background exactly, map or no map; with the switch on and no map, too"""
    env = maps()["random8x16"]
    sc = empty_scene(env)
    off = dataclasses.replace(sc.params, env_as_background=False)
    try:
        for b in side.each():
            b.set_params(off)
        side.setup(env, 0, 0)
        for d in AXES + sphere_dirs(rng(5), 6):
            assert side.look(d).astype(F32).tolist() == F32(BG).tolist()
        for b in side.each():
            b.set_params(sc.params)
        side.setup(None, 0, 0)
        assert side.look(AXES[0]).astype(F32).tolist() == F32(BG).tolist()
    finally:
        for b in side.each():
            b.set_params(sc.params)


# ================================================================================================== the tests must be able to fail
def test_wrong_rules_are_caught():
    """deliberately wrong references on the same cases: each must violate the bound on at least WRONG_MIN of the sweep (the right rule's
    value stands in for a correct implementation's output: it is within D by the tests above)"""
    for orientation in (0, 1):
        for gamma2 in (0, 1):
            for wrong in ("half_texel", "nearest", "no_wrap", "other_orientation"):
                n_bad = n_all = 0
                for name, env, dirs, _ in all_cases(orientation):
                    if name == "1x1":
                        continue                                       # a constant map cannot tell any rule from another
                    if wrong == "no_wrap" and name != "random8x16":
                        continue                                       # judged on the map whose case set holds the seam
                    ref, D = L.env_ref(env, np.array(dirs), orientation, gamma2)
                    bad, _ = L.env_ref(env, np.array(dirs), orientation, gamma2, wrong=wrong)
                    sel = slice(None)
                    if wrong == "no_wrap":                             # the seam cases are the sweep that speaks about the wrap
                        k = len(AXES) + len(pole_dirs())
                        sel = slice(k, k + len(seam_dirs()))
                    n_bad += int((np.abs(bad - ref) > D).any(1)[sel].sum()); n_all += len(dirs[sel])
                share = n_bad / n_all
                print(f"wrong rule {wrong} o{orientation} g{gamma2}: violates the bound on {share:.3f} of {n_all}")
                assert share >= WRONG_MIN, (wrong, orientation, gamma2, share)
