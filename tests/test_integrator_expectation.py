"""The path integrator -- shade_path (cadrays_amd/csrc/k_shade.h), intersect_light (k_lights_env.h) and their twins in oracle/crh_oracle.c -- held to
float64 expected radiances (tests/integrator_reference.py, written from DESIGN.md section 3 and the contract headers), on two sides with the SAME cases:
  cpu  the oracle
  gpu  the gfx950 kernels through View(0); there every image must also be bit-equal to the oracle's

Every case is one surface point seen through a 0.5 degree camera: 64 x 64 pixels with independent seeds, 128 samples each unless the case says more.
For every channel with a non-zero expectation

    |mean - want| <= 4.5 SE + q

SE = the standard deviation of the per-pixel means / sqrt(pixels) (for the slab without roulette: no less than the exact standard error of its
known distribution -- the truncation of the series is an event rarer than one in the 5e5 paths, which no sample variance can see); q = |want(n) - want(2 n)|, the quadrature's own error (want is taken at 2 n).  Two
conditions keep a pass meaningful: q <= SE / 10 and SE <= 0.5 % of want.  4.5 standard errors are a false alarm of 7e-6 per comparison; the seeds are
fixed, so a run is deterministic.  test_wrong_rules_are_caught shows the power: each deliberately wrong rule of the reference misses a case by more than
10 SE.

Two behaviours of the spec depart from physics and are pinned AS SPECIFIED: overlapping directional cones, and the
min_contribution cut, which tests the MIS-weighted contribution without the throughput.
"""
import dataclasses
import functools

import numpy as np
import pytest

from cadrays_amd import scenes
from cadrays_amd.materials import BSDF, Fresnel
from cadrays_amd.scenes import Camera, Light, Params, Scene

import bsdf_reference as B
import integrator_reference as R

RES, SPP, FOVY, DIST = 64, 128, 0.5, 5.0
Z_PASS, Z_POWER = 4.5, 10.0
NO_CUTS = dict(min_contribution=0.0, min_throughput=0.0)
DEFAULTS = dict(min_contribution=1e-2, min_throughput=1e-3)          # crh_spec.h #11, #12 as they default


def sph(theta, phi):
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def view_from(wo, target=(0.0, 0.0, 0.0), dist=DIST):
    wo = R.unit(wo)
    up = (0.0, 1.0, 0.0) if abs(wo[1]) < 0.9 else (1.0, 0.0, 0.0)
    return Camera(eye=tuple(np.asarray(target) + dist * wo), dir=tuple(-wo), up=up, fovy_deg=FOVY)


def plane(half=50.0, z=0.0, normal=(0.0, 0.0, 1.0), mat=0):
    p = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float32)
    n = np.tile(np.asarray(normal, np.float32), (4, 1))
    t = np.array([[0, 1, 2, mat], [0, 2, 3, mat]], np.int32)
    return p, n, t


def join(*meshes):
    pos, nrm, tri, base = [], [], [], 0
    for p, n, t in meshes:
        t = t.copy(); t[:, :3] += base; base += len(p)
        pos.append(p); nrm.append(n); tri.append(t)
    return np.concatenate(pos), np.concatenate(nrm), np.concatenate(tri)


def cone(towards, half, L, colour=(1.0, 0.8, 0.6)):
    return Light.directional(tuple(-R.unit(towards)), smoothness=half, intensity=L, color=colour)


@dataclasses.dataclass
class Case:
    scene: Scene
    want: object                     # n -> rgb (float64): the expectation at quadrature resolution n; None for a closed form in `exact`
    n: int = 48
    spp: int = SPP
    exact: object = None             # rgb known without quadrature
    physical: object = None          # n -> rgb: the physical integral, for the cases that pin a departure from it
    wrong: object = None             # (mode, n) -> rgb: the expectation under a deliberately wrong rule
    deterministic: float = 0.0       # > 0: every pixel equals `exact` within this rtol; no statistics
    variance: object = None          # rgb: the exact variance of one path where it is known (the sample's SE is then no less than what it gives)


def make(mesh, mats, lights, wo, spec, *, target=(0.0, 0.0, 0.0), max_depth=2, two_sided=True, rr=False, env=None, background=(0.0, 0.0, 0.0),
         camera=None, res=RES):
    pos, nrm, tri = mesh
    par = Params(width=res, height=res, tile_size=32, max_depth=max_depth, two_sided=two_sided, russian_roulette=rr, background=background)
    return Scene(pos, nrm, tri, list(mats), lights=list(lights), env=env, camera=camera or view_from(wo, target), params=par, spec=dict(spec),
                 name="integrator_expectation")


# ================================================================================================== materials and lights of the cases
def schlick_coated():
    b = BSDF.Glossy(roughness=0.25)
    b.Kc = np.array([1.0, 1.0, 1.0, 0.2], np.float32)
    b.FresnelCoat = Fresnel.CreateSchlick((0.04, 0.08, 0.16))
    return b


MATERIALS = {
    "matte": BSDF.Matte, "glossy": lambda: BSDF.Glossy(roughness=0.25), "metal": lambda: BSDF.Metal(roughness=0.3),
    "paint": lambda: BSDF.Paint(roughness=0.3, coat_roughness=0.2), "coated": schlick_coated,
}
THETAS = (0.3, 1.1)
A_DIR, B_DIR = sph(0.55, 2.4), sph(0.7, -0.8)                        # towards the lights; the mirror direction of a viewer at phi 0 lies at phi pi
CONE_A = cone(A_DIR, 0.25, 8.0)
CONE_WIDE = cone(A_DIR, 0.8, 2.0)                                    # density 0.53: here BSDF sampling carries as much weight as NEE
CONE_B = cone(B_DIR, 0.2, 5.0, (0.5, 0.7, 1.0))
# two cones 0.225 rad apart that overlap, the first around the mirror direction of the viewer at theta 0.3, where BSDF sampling carries weight
OVERLAP = [cone(sph(0.3, np.pi), 0.25, 8.0), cone(sph(0.525, np.pi), 0.2, 5.0, (0.5, 0.7, 1.0))]
SPHERE = Light.positional((-1.2, 0.4, 1.5), smoothness=0.4, intensity=8.0, color=(1.0, 0.8, 0.6))
CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = fn
        return fn
    return reg


def on_plane(b, lights, wo, spec, kind, *, spp=SPP, n=48, normal=(0.0, 0.0, 1.0), env=None, two_sided=True, single_lobe=False, sky=1):
    """one material on the large plane; kind = 'physical' | 'estimator'"""
    mesh = plane(normal=normal)
    sp = dict(spec, mis_single_lobe=int(single_lobe))
    sc = make(mesh, [b], lights, wo, sp, env=env, two_sided=two_sided)
    eps = R.scene_epsilon(mesh[0])
    geo = dict(ns=normal, ng=(0, 0, 1), env=env, two_sided=two_sided)

    def phys(n):
        return R.physical_direct(b, wo, lights, n=n, n_sky=sky * n, **geo)

    def est(n, wrong=None):
        return R.estimator_expectation(b, wo, lights, n=n, n_sky=sky * n, eps=eps, min_contribution=sp["min_contribution"],
                                       min_throughput=sp["min_throughput"], mis_single_lobe=single_lobe, wrong=wrong, **geo)

    def wrong(mode, n):
        return R.physical_direct(b, wo, lights, n=n, wrong=mode, **geo) if (kind == "physical" and mode == "asin_cone") else est(n, mode)

    return Case(sc, phys if kind == "physical" else est, n=n, spp=spp, physical=phys, wrong=wrong)


def lit_plane(material, light, theta=0.3):
    return on_plane(MATERIALS[material](), [light], sph(theta, 0.0), NO_CUTS, "physical")


for _m in MATERIALS:
    for _t in THETAS:
        CASES[f"cone-{_m}-{_t}"] = functools.partial(lit_plane, _m, CONE_A, _t)
        CASES[f"sphere-{_m}-{_t}"] = functools.partial(lit_plane, _m, SPHERE, _t)
for _m in ("glossy", "paint", "coated"):                              # beyond the narrow cones: both strategies at comparable weight
    CASES[f"wide-cone-{_m}"] = functools.partial(lit_plane, _m, CONE_WIDE)


@case("two-cones-ab")
def _():
    return on_plane(MATERIALS["glossy"](), [CONE_A, CONE_B], sph(0.3, 0.0), NO_CUTS, "physical")


@case("two-cones-ba")
def _():
    return on_plane(MATERIALS["glossy"](), [CONE_B, CONE_A], sph(0.3, 0.0), NO_CUTS, "physical")


@case("overlapping-cones")
def _():
    return on_plane(MATERIALS["glossy"](), OVERLAP, sph(0.3, 0.0), NO_CUTS, "estimator", n=96)


@case("cut-L0.3")
def _():
    return on_plane(BSDF.Matte(0.7), [cone(A_DIR, 0.25, 0.3, (1, 1, 1))], sph(0.3, 0.0), DEFAULTS, "estimator", n=96)


@case("cut-L0.02")
def _():
    return on_plane(BSDF.Matte(0.7), [cone(A_DIR, 0.25, 0.02, (1, 1, 1))], sph(0.3, 0.0), DEFAULTS, "estimator", spp=320)


@case("sphere-inside-cone")
def _():
    to_sphere = R.unit(SPHERE.vec)
    return on_plane(MATERIALS["glossy"](), [cone(to_sphere, 0.35, 3.0, (0.5, 0.7, 1.0)), SPHERE], sph(0.3, 0.0), NO_CUTS, "estimator", n=96)


@case("single-lobe-paint")
def _():
    return on_plane(MATERIALS["paint"](), [CONE_A], sph(0.3, 0.0), NO_CUTS, "estimator", single_lobe=True)


@case("two-sided-from-below")
def _():
    below = sph(np.pi - 0.55, 2.4)
    return on_plane(MATERIALS["glossy"](), [cone(below, 0.25, 8.0)], sph(np.pi - 0.3, 0.0), NO_CUTS, "physical")


@case("one-sided-from-below")
def _():
    below = sph(np.pi - 0.55, 2.4)
    c = on_plane(MATERIALS["glossy"](), [cone(below, 0.25, 8.0)], sph(np.pi - 0.3, 0.0), NO_CUTS, "physical", two_sided=False)
    return dataclasses.replace(c, want=None, exact=np.zeros(3), deterministic=1e-30, spp=8)


SKY = scenes.procedural_sky(64, 32, 1)


def under_sky(normal):
    return on_plane(MATERIALS["glossy"](), [], sph(0.6, 0.7), NO_CUTS, "physical", normal=normal, env=SKY, sky=8)


CASES["sky-normal-up"] = functools.partial(under_sky, (0.0, 0.0, 1.0))
CASES["sky-normal-tilted"] = functools.partial(under_sky, (0.2, -0.1, 1.0))


# ---- a coloured delta mirror in front of a glossy floor: camera -> mirror -> floor -> light
MIRROR_KS, MIRROR_F0 = np.array([1.0, 0.8, 0.6]), (0.9, 0.6, 0.3)
FLOOR_LIGHT = sph(0.5, 0.5)                                           # towards +x, +y: away from the mirror at x = -1


def mirror_case(L, spec, kind, n=48, spp=SPP):
    floor = BSDF.Glossy(kd=(0.6, 0.3, 0.1), ks=(0.2, 0.5, 0.7), roughness=0.25)       # coloured weights: the lobe pick depends on the throughput
    mirror = BSDF.CreateMetallic(MIRROR_KS, Fresnel.CreateSchlick(MIRROR_F0), 0.0)
    quad = (np.array([[-1, -0.5, 0.5], [-1, 0.5, 0.5], [-1, 0.5, 1.5], [-1, -0.5, 1.5]], np.float32), np.tile(np.array([[1, 0, 0]], np.float32), (4, 1)),
            np.array([[0, 1, 2, 1], [0, 2, 3, 1]], np.int32))
    mesh = join(plane(), quad)
    d_in = R.unit((-1.0, 0.0, -1.0))                                    # the camera ray; reflected at (-1, 0, 1) about +x it runs to the origin
    lights = [cone(FLOOR_LIGHT, 0.25, L)]
    sc = make(mesh, [floor, mirror], lights, -d_in, spec, target=(-1.0, 0.0, 1.0), max_depth=3)
    weight = MIRROR_KS * B.fresnel(float(-d_in[0]), Fresnel.CreateSchlick(MIRROR_F0).Serialize())      # Ks x F_base(cos) of the delta lobe
    wo = R.unit((-1.0, 0.0, 1.0))                                       # at the floor: back towards the mirror
    eps = R.scene_epsilon(mesh[0])

    def phys(n):
        return weight * R.physical_direct(floor, wo, lights, n=n)

    def est(n, wrong=None):
        return R.estimator_expectation(floor, wo, lights, n=n, eps=eps, weight=weight, min_contribution=spec["min_contribution"],
                                       min_throughput=spec["min_throughput"], wrong=wrong)

    return Case(sc, phys if kind == "physical" else est, n=n, spp=spp, physical=phys, wrong=lambda mode, n: est(n, mode))


CASES["mirror"] = functools.partial(mirror_case, 8.0, NO_CUTS, "physical")
CASES["mirror-dim-default-cut"] = functools.partial(mirror_case, 0.25, DEFAULTS, "estimator", 96)


# ---- the absorbing slab under a constant sky
SLAB = dict(ior=1.5, thickness=0.5, coeff=3.0, colour=(0.8, 0.5, 1.0))


def slab_case(theta, depth, rr):
    glass = BSDF.CreateGlass(1.0, SLAB["colour"], SLAB["coeff"], SLAB["ior"])
    mesh = join(plane(), plane(z=-SLAB["thickness"], normal=(0.0, 0.0, -1.0)))
    sc = make(mesh, [glass], [], sph(theta, 0.0), DEFAULTS, max_depth=depth, rr=rr, background=(1.0, 1.0, 1.0))
    eps = R.scene_epsilon(mesh[0])

    def series(wrong=None):
        return R.slab_series(SLAB["ior"], SLAB["thickness"], SLAB["coeff"], SLAB["colour"], theta, depth, eps=eps, cam_dist=DIST, wrong=wrong)

    m1, m2 = R.slab_series(SLAB["ior"], SLAB["thickness"], SLAB["coeff"], SLAB["colour"], theta, depth, eps=eps, moments=True)
    return Case(sc, None, exact=series(), wrong=lambda mode, n: series(mode), variance=None if rr else m2 - m1 * m1)


for _t, _d, _rr in ((0.0, 4, False), (0.9, 4, False), (0.9, 8, False), (1.3, 12, False), (1.3, 12, True)):
    CASES[f"slab-{_t}-depth{_d}{'-roulette' if _rr else ''}"] = functools.partial(slab_case, _t, _d, _rr)


# ---- the furnace: inside a closed emissive diffuse box every path of k bounces returns E sum rho^j, j <= k
def furnace_case(rho, depth, rr, spec, terms, deterministic=0.0):
    m = scenes._Mesh(); m.box((2, 2, 2), 0, (-1, -1, -1))
    pos, nrm, tri = m.arrays()
    E = 0.75
    b = BSDF.CreateDiffuse(rho); b.Le = np.array([E, E, E], np.float32)
    cam = Camera(eye=(0.1, -0.2, 0.05), dir=(0.3, 1, 0.2), up=(0, 0, 1), fovy_deg=60)
    res = 16 if deterministic else RES
    sc = make((pos, -nrm, tri), [b], [], None, spec, max_depth=depth, rr=rr, camera=cam, res=res)
    rho = np.broadcast_to(np.asarray(rho, np.float64), (3,))
    return Case(sc, None, exact=E * sum(rho ** k for k in range(terms)), deterministic=deterministic, spp=2 if deterministic else SPP)


CASES["furnace-roulette-from-3"] = functools.partial(furnace_case, (0.8, 0.5, 0.3), 8, True, dict(DEFAULTS, rr_start_bounce=3), 8)
CASES["furnace-roulette-from-0"] = functools.partial(furnace_case, (0.8, 0.5, 0.3), 8, True, dict(DEFAULTS, rr_start_bounce=0), 8)
# rho 0.3: the throughput 0.3^6 = 7.3e-4 falls under min_throughput after the sixth hit: emission of hits 0 .. 5, whatever the depth allows
CASES["furnace-min-throughput"] = functools.partial(furnace_case, 0.3, 10, False, DEFAULTS, 6, 2e-6)


# ================================================================================================== the two sides
MEASURED = {}                        # (side, case) -> (mean, SE, image): every case is rendered once per side


class Side:
    def __init__(self, name, ctx, twin=None):
        self.name, self.ctx, self.twin = name, ctx, twin

    def image(self, sc, spp):
        imgs = []
        for b in (self.ctx, self.twin):
            if b is None:
                continue
            b.load_scene(sc); b.render(spp)
            imgs.append(b.read_hdr())
        if self.twin is not None:
            assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), "gpu != oracle"
        return imgs[0]

    def measure(self, name):
        """(mean, SE, image) of a case, rendered once per side"""
        key = (self.name, name)
        if key not in MEASURED:
            c = built(name)
            img = self.image(c.scene, c.spp)
            px = img.reshape(-1, 3).astype(np.float64)
            se = px.std(0, ddof=1) / np.sqrt(len(px))
            if c.variance is not None:
                se = np.maximum(se, np.sqrt(np.maximum(c.variance, 0.0) / (len(px) * c.spp)))
            MEASURED[key] = (px.mean(0), se, img)
        return MEASURED[key]

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


@functools.lru_cache(maxsize=None)
def built(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def wanted(name):
    """(want, q) of a case, computed once for both sides"""
    c = built(name)
    if c.want is None:
        return np.asarray(c.exact, np.float64), np.zeros(3)
    fine = c.want(2 * c.n)
    return fine, np.abs(fine - c.want(c.n))


def verdict(name, mean, se, want, q):
    """the per-channel figures of one comparison, printed before anything is asserted"""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (mean - want) / se
    print(f"{name}: want {want} mean {mean} SE {se} q {q} z {z}")
    return z


# ================================================================================================== the tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_radiance(side, name):
    c = built(name)
    mean, se, img = side.measure(name)
    want, q = wanted(name)
    if c.deterministic:
        print(f"{name}: want {want} min {img.min((0, 1))} max {img.max((0, 1))}")
        np.testing.assert_allclose(img.reshape(-1, 3), np.broadcast_to(want, (img.shape[0] * img.shape[1], 3)), rtol=c.deterministic, atol=0)
        return
    verdict(name, mean, se, want, q)
    lit = want != 0
    assert lit.any()
    assert (q[lit] <= se[lit] / 10).all(), "the quadrature is too coarse for this case"
    assert (se[lit] <= 0.005 * want[lit]).all(), "too few samples: a pass would mean nothing"
    assert (np.abs(mean - want)[lit] <= Z_PASS * se[lit] + q[lit]).all()
    assert (mean[~lit] == 0).all()


@pytest.mark.parametrize("name", ["overlapping-cones", "cut-L0.3", "cut-L0.02", "mirror-dim-default-cut"])
def test_departure_from_physics_is_real(side, name):
    """the cases that pin a rule of the spec which is NOT the physical integral: the image is more than 10 standard errors away from that integral
    (and test_expected_radiance holds it to the estimator's expectation)"""
    c = built(name)
    mean, se, _ = side.measure(name)
    phys = c.physical(2 * c.n)
    z = verdict(name + " against the physical integral", mean, se, phys, np.abs(phys - c.physical(c.n)))
    assert (np.abs(z) > Z_POWER).any()


def random_directions(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


@pytest.mark.parametrize("name", sorted(MATERIALS))
def test_vectorised_bsdf_is_bsdf_reference(name):
    """the array forms in integrator_reference.py are bsdf_reference.py's functions: same value and density, direction by direction"""
    b = MATERIALS[name]()
    wis = random_directions(200, 1)
    for wo, W, two in ((sph(0.3, 0.0), (1, 1, 1), True), (sph(1.1, 2.0), (0.9, 0.5, 0.1), True), (sph(np.pi - 0.4, 1.0), (0.2, 1.0, 0.7), True),
                       (sph(np.pi - 0.4, 1.0), (1, 1, 1), False)):
        f, p = R.lobes(b, wo, wis, W, two)
        want_f = np.array([B.eval_fcos(b, wo, wi, two) for wi in wis])
        want_p = np.array([B.pdf(b, wo, wi, W, two) for wi in wis])
        np.testing.assert_allclose(f.sum(0), want_f, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(p.sum(0), want_p, rtol=1e-12, atol=1e-300)
        if two:
            assert (want_f > 0).any() and (want_p > 0).any()


def test_reference_weights_sum_to_one():
    """with the power heuristic, one light and no cut the two terms of the estimator add up to the physical integral; with the balance heuristic too"""
    b, wo = MATERIALS["paint"](), sph(0.3, 0.0)
    phys = R.physical_direct(b, wo, [CONE_WIDE], n=64)
    for wrong in (None, "balance"):
        np.testing.assert_allclose(R.estimator_expectation(b, wo, [CONE_WIDE], min_contribution=0.0, n=64, wrong=wrong), phys, rtol=1e-12)
    nee, imp = R.estimator_expectation(b, wo, [CONE_WIDE], min_contribution=0.0, n=64, parts=True)
    assert (nee > 0.2 * phys).all() and (imp > 0.2 * phys).all()        # under the wide cone both strategies carry weight


# which case must expose which wrong rule: (mode, case)
POWER = [
    ("balance", "cut-L0.3"), ("no_light_pick", "two-cones-ab"), ("asin_cone", "sphere-matte-0.3"), ("cut_throughput", "mirror-dim-default-cut"),
    ("implicit_per_light", "overlapping-cones"), ("absorb_outside", "slab-0.9-depth8"), ("no_eps", "slab-0.0-depth4"),
]


def test_power_covers_every_wrong_rule():
    assert {m for m, _ in POWER} == set(R.WRONG_ESTIMATOR) | set(R.WRONG_SLAB)


@pytest.fixture(scope="module")
def cpu_side(oracle_lib):
    s = Side("cpu", oracle_lib.Oracle())
    yield s
    s.close()


@pytest.mark.parametrize("mode,name", POWER)
def test_wrong_rules_are_caught(cpu_side, mode, name):
    """CPU only: against the reference with one rule deliberately wrong, the case that pins that rule fails by more than 10 standard errors"""
    c = built(name)
    mean, se, _ = cpu_side.measure(name)
    n = 2 * c.n
    bad = np.asarray(c.wrong(mode, n), np.float64)
    z = verdict(f"{name} against '{mode}'", mean, se, bad, np.zeros(3))
    assert (np.abs(z) > Z_POWER).any()
