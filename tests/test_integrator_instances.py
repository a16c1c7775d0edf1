"""What is SHADED from placed, moved and occluded objects, held to float64 expected radiances: the `in_object` branch of shade_path
(cadrays_amd/csrc/k_shade.h), its baked twin in crh_build (crh_scene.cpp), their twins in oracle/crh_oracle.c, and occlusion inside the integrator
(shadow rays, the split any-hit passes, an implicit light hit behind a blocker).  Same two sides, camera, acceptance rule and helpers as
tests/test_integrator_expectation.py (imported, not copied); the expectations are tests/integrator_reference.py's.

PRINCIPLE.  The WORLD scene of a case is fixed.  Its objects are handed over in object space as X^-1 world (float64, rounded to float32) together
with X, so the expected radiance is the world scene's whatever X is.  Routes:
  flat    no objects at all (the baseline of the occlusion cases)
  baked   tri_object / obj_xform go to set_geometry and crh_build bakes them (n_instances == 0 is asserted)
  moved   the scene is built with another placement X0 (the same matrix, shifted by 0.07 extents), then set_transforms brings the object to X:
          it IS an instance of the two-level tree (get_tlas()["n_instances"] == the number of moved objects is asserted)
Every world scene carries two tiny static triangles at the corners of a cube 4 extents in half-width (`anchored`): crh_spec.h #6 takes eps from the
scene's bounds, and the bounds of a scene with instances are those of loose transformed boxes and of the static tree as built; inside the cube they
are the cube on every route, so eps = scene_epsilon(world positions) everywhere.  (A ray meets an anchor with probability < 1e-8.)

PLACEMENTS (the contract is gp_Trsf: rigid motion, uniform scale, mirror).  R = 1 rad about (0.3, -0.5, 0.8); t = (2.5, -3, 1.5) extents.
  ident    the identity as an instance (the control)          rot      R, t
  x1000    1000 R, t            x0.001   0.001 R, t            mirror   R diag(-1, 1, 1), t            mirror-x1000   1000 R diag(-1, 1, 1), t
  nonuniform (case E only, OUTSIDE the contract)  R (1 + 2 a a^T), a = unit(0.6, 0.3, -0.7): scaled (1, 1, 3) about a skew axis

CASES.  64 x 64 pixels, fovy 0.5 degrees.  SE / want and q / SE: the worst channel, oracle side (the GPU's images are bit-equal).
  case                      routes / placements                                                   spp   n    SE / want  q / SE
  A normals-sky-tilted      baked rot, baked x1000, moved ident, moved rot, moved mirror          128   48   0.00046    0.005
  A normals-glossy-cone     moved x1000, baked mirror                                             128   48   0.00035    9e-6
  A normals-glossy-sphere   moved x0.001, baked rot                                               128   48   0.0005     2e-5
  A normals-paint-cone      moved mirror, baked x0.001                                            128   48   0.00028    2e-5
  A normals-paint-sphere    moved rot, baked x1000                                                128   48   0.00042    1e-5
  B slab (0.9 rad, depth 8) baked x1000, moved x1000, baked x0.001, moved x0.001                  128   -    0.00048    0 (closed form)
  C occl-<material>-<light>-<blocked | clear | edge>, material-light = matte-cone, glossy-sphere, matte-sphere, glossy-cone
      flat                  all four pairs, three positions
      quad-moved            matte-cone: quad rot; glossy-sphere: quad x1000
      receiver-moved        matte-cone: receiver mirror; glossy-sphere: receiver x0.001
    + occl-glossy-widecone-edge flat and quad-moved rot (a cone of 0.8 rad: the BSDF-sampled ray carries half the weight)
      blocked               every pixel EXACTLY 0, the BSDF-sampled ray's term included (deterministic)   8     -
      clear                 the unoccluded expectation, as the parent module takes it             128   48   0.0005 at most, 2e-5 at most
      edge                  matte-cone 0.0016, 0.057; glossy-cone 0.0016, 0.053; matte-sphere     128   144  0.0016 at most, 0.057 at most
                            0.0014, 0.003; glossy-sphere 0.0014, 0.009; glossy-widecone 0.0013, 0.010
    edge: the quad's straight edge crosses the axis of the light's cone as seen from the shading point, and the expectation is integrated over
    the camera's footprint (2 x 2 Gauss-Legendre points; one point is 0.3 SE off, 4 x 4 points change less than 0.1 SE).  The builder asserts,
    from every footprint point, that the camera's ray passes the quad and that the cone (plus a rim of 0.02 in cos) is wholly covered / wholly
    open / between 0.3 and 0.7 covered.  The quad hangs 1.0 above the receiver; eps = 6.9e-4: 1440 eps.  Even so the reference lets both rays
    leave from their offset origins: an expectation taken from p itself is 0.13 - 0.2 % (about 1 - 1.5 SE) darker than the images, over 8 seeds.
  D furnace                 baked mirror-x1000, moved mirror-x1000, two_sided = False             2     -    every pixel within 2e-6
  E nonuniform-sky-tilted   baked nonuniform, moved nonuniform                                    128   48   0.0012     0.0014
    AS SPECIFIED, not physics: both sides carry a shading normal as normalize(M n); the expectation under the inverse transpose is
    more than 10 SE away (test_nonuniform_normals_follow_M_not_the_inverse_transpose).

LEFT OUT of the cross product (5 world scenes of A x 2 routes x 5 placements, and so on): every pair not listed above.  Every placement and both
routes appear in A; B has both scales on both routes; in C the moved roles take two of the four material-light pairs, one placement each, so that
rot, x1000, mirror and x0.001 each move a quad or a receiver once; ident appears once (A); the flat route has no placement.

On the GPU the moved roles of C are rendered again under CRH_SPLIT_PASSES = 0 / 1 and the AUTO / WIDE / STAGED schedules; every such image must be
bit-equal to the oracle's, which test_expected_radiance holds to the expectation.

test_wrong_rules_are_caught (CPU): each rule of integrator_reference.WRONG_INSTANCE misses a named case by more than 10 SE.
"""
import dataclasses
import functools

import numpy as np
import pytest

from cadrays_amd.materials import BSDF

import integrator_reference as R
import test_integrator_expectation as E
from test_integrator_expectation import Case, Z_PASS, Z_POWER, verdict

ANCHOR = 4.0                          # the anchors' cube: half-width in extents
AXIS, ANGLE, SHIFT = (0.3, -0.5, 0.8), 1.0, np.array([2.5, -3.0, 1.5])
NUDGE = np.array([0.06, -0.03, 0.02])                               # X0 = X shifted by this many extents
ROT = R.rotation(AXIS, ANGLE)
FLIP = np.diag([-1.0, 1.0, 1.0])
_a = R.unit((0.6, 0.3, -0.7))
FAMILIES = {
    "ident": np.eye(3), "rot": ROT, "x1000": 1000.0 * ROT, "x0.001": 0.001 * ROT, "mirror": ROT @ FLIP, "mirror-x1000": 1000.0 * ROT @ FLIP,
    "nonuniform": ROT @ (np.eye(3) + 2.0 * np.outer(_a, _a)),
}

def placement(family, extent, nudged=False):
    t = np.zeros(3) if family == "ident" else SHIFT * extent
    return R.xform(FAMILIES[family], t + (NUDGE * extent if nudged else 0.0))


IDENT = R.xform(np.eye(3))


# ================================================================================================== world scenes
@dataclasses.dataclass
class World:
    case: Case                       # scene: the WORLD scene (tri_object set: one id per part, the anchors last); want / exact as in the parent module
    extent: float
    wrong: object = None             # (mode, X of the placed object, n) -> rgb under a wrong rule
    normals: str = "contract"        # how normals go to object space (integrator_reference.to_object_space)
    physical: object = None          # n -> rgb: case E's yardstick


def anchored(parts, extent):
    """the parts (one object each) + the two anchor triangles as the last object: (pos, nrm, tri, tri_object)"""
    A, s = ANCHOR * extent, extent / 64.0
    p = np.array([[-A, -A, -A], [-A + s, -A, -A], [-A, -A + s, -A], [A, A, A], [A - s, A, A], [A, A - s, A]], np.float32)
    anchor = (p, np.tile(np.array([[0, 0, 1]], np.float32), (6, 1)), np.array([[0, 1, 2, 0], [3, 4, 5, 0]], np.int32))
    parts = list(parts) + [anchor]
    pos, nrm, tri = E.join(*parts)
    obj = np.concatenate([np.full(len(t), k, np.int32) for k, (_, _, t) in enumerate(parts)])
    return pos, nrm, tri, obj


def world_scene(parts, extent, mats, lights, wo, spec, **kw):
    pos, nrm, tri, obj = anchored(parts, extent)
    sc = E.make((pos, nrm, tri), mats, lights, wo, spec, **kw)
    return dataclasses.replace(sc, tri_object=obj, name="integrator_instances"), R.scene_epsilon(pos)


WORLDS = {}


def world(name):
    def reg(fn):
        WORLDS[name] = fn
        return fn
    return reg


# ---- A: normals
def normals_world(material, lights, wo, normal, env=None, sky=1, normals="contract"):
    b = E.MATERIALS[material]()
    sc, _ = world_scene([E.plane(normal=normal)], 50.0, [b], lights, wo, E.NO_CUTS, env=env)

    def phys(n, ns=normal):
        return R.physical_direct(b, wo, lights, n=n, n_sky=sky * n, ns=ns, ng=(0, 0, 1), env=env)

    def wrong(mode, X, n):
        n_obj = R.to_object_space(X, np.zeros((1, 3)), np.asarray([normal], np.float64), normals)[1][0]
        return phys(n, R.carried_normal(X, n_obj, mode))

    return World(Case(sc, phys), 50.0, wrong, normals)


TILTED = (0.2, -0.1, 1.0)
WORLDS["normals-sky-tilted"] = functools.partial(normals_world, "glossy", [], E.sph(0.6, 0.7), TILTED, E.SKY, 8)
for _m in ("glossy", "paint"):
    WORLDS[f"normals-{_m}-cone"] = functools.partial(normals_world, _m, [E.CONE_A], E.sph(0.3, 0.0), (0.0, 0.0, 1.0))
    WORLDS[f"normals-{_m}-sphere"] = functools.partial(normals_world, _m, [E.SPHERE], E.sph(0.3, 0.0), (0.0, 0.0, 1.0))


# ---- E: a non-uniform scale carries the normal as normalize(M n)
@world("nonuniform-sky-tilted")
def _():
    w = normals_world("glossy", [], E.sph(0.6, 0.7), TILTED, E.SKY, 8, normals="covector")
    X = placement("nonuniform", w.extent)
    phys = w.case.want
    n_obj = R.to_object_space(X, np.zeros((1, 3)), np.asarray([TILTED], np.float64), "covector")[1][0]
    assert np.allclose(R.carried_normal(X, n_obj, "inverse_transpose"), R.unit(TILTED), atol=1e-6)      # physics would give the world scene's normal back
    ns = R.carried_normal(X, n_obj)
    assert np.arccos(ns @ R.unit(TILTED)) > 0.2 and ns[2] > 0.5
    return dataclasses.replace(w, case=dataclasses.replace(w.case, want=lambda n: phys(n, ns)), physical=lambda n: phys(n))


# ---- B: the absorbing slab as one object
@world("slab")
def _():
    S, theta, depth = E.SLAB, 0.9, 8
    glass = BSDF.CreateGlass(1.0, S["colour"], S["coeff"], S["ior"])
    sc, eps = world_scene([E.join(E.plane(), E.plane(z=-S["thickness"], normal=(0.0, 0.0, -1.0)))], 50.0, [glass], [], E.sph(theta, 0.0), E.DEFAULTS,
                          max_depth=depth, rr=False, background=(1.0, 1.0, 1.0))

    def series(**kw):
        return R.slab_series(S["ior"], S["thickness"], S["coeff"], S["colour"], theta, depth, eps=eps, cam_dist=E.DIST, **kw)

    def wrong(mode, X, n):
        scale = abs(np.linalg.det(np.asarray(X, np.float64).reshape(3, 4)[:, :3])) ** (1.0 / 3.0)
        return series(wrong=mode, scale=scale)

    m1, m2 = series(moments=True)
    return World(Case(sc, None, exact=series(), variance=m2 - m1 * m1), 50.0, wrong)


# ---- D: the closed emissive box, one-sided
@world("furnace")
def _():
    c = E.furnace_case(0.3, 10, False, E.DEFAULTS, 6, 2e-6)
    s = c.scene
    pos, nrm, tri, obj = anchored([(s.pos, s.nrm, s.tri)], 1.0)
    sc = dataclasses.replace(s, pos=pos, nrm=nrm, tri=tri, tri_object=obj, params=dataclasses.replace(s.params, two_sided=False), name="integrator_instances")
    want = np.asarray(c.exact, np.float64)
    return World(dataclasses.replace(c, scene=sc), 1.0, lambda mode, X, n: want * max(R.facing_sign(X, mode), 0.0))


# ---- C: occlusion
HC, HANG, QUAD_LEN = 5.0, 1.0, 4.0
OCCL_WO = E.sph(0.3, 0.0)
OCCL_LIGHTS = {"cone": E.CONE_A, "sphere": E.SPHERE, "widecone": E.CONE_WIDE}
EDGE_N = 144                          # an edge through the cone: q <= SE / 10 needs more cells than the smooth cases' 48


def footprint(wo, k=2):
    """k x k Gauss-Legendre points of the camera's footprint on the plane z = 0 and their weights (sum 1): the mean over the image is the mean over
    the image plane's square, [-tan(fovy / 2), tan(fovy / 2)]^2 (square pixels, 64 x 64).  The node set is symmetric, so which way the camera's axes
    point does not matter."""
    cam = E.view_from(wo)
    eye, d = np.asarray(cam.eye, np.float64), np.asarray(cam.dir, np.float64)
    right = R.unit(np.cross(d, np.asarray(cam.up, np.float64)))
    up = np.cross(right, d)
    x, w = np.polynomial.legendre.leggauss(k)
    th = np.tan(np.radians(E.FOVY) / 2)
    pts, wts = [], []
    for i in range(k):
        for j in range(k):
            r = d + th * (x[i] * right + x[j] * up)
            pts.append(eye - eye[2] / r[2] * r); wts.append(w[i] * w[j] / 4.0)
    return eye, np.array(pts), np.array(wts)


def occlusion_world(material, light, position):
    b, l = E.MATERIALS[material](), OCCL_LIGHTS[light]
    axis = R._Cone(l, np.zeros(3)).axis
    x_edge = {"blocked": HANG * np.tan(0.3) - 0.2, "clear": -2.5, "edge": HANG * axis[0] / axis[2]}[position]
    corners = np.array([[x_edge - QUAD_LEN, -QUAD_LEN, HANG], [x_edge, -QUAD_LEN, HANG], [x_edge, QUAD_LEN, HANG], [x_edge - QUAD_LEN, QUAD_LEN, HANG]], np.float32)
    quad = (corners, np.tile(np.array([[0, 0, -1]], np.float32), (4, 1)), np.array([[0, 1, 2, 1], [0, 2, 3, 1]], np.int32))
    black = BSDF.CreateDiffuse(0.0)
    sc, eps = world_scene([E.plane(half=HC), quad], HC, [b, black], [l], OCCL_WO, E.NO_CUTS)
    blocker = R.Quad(corners.astype(np.float64))
    eye, pts, wts = footprint(OCCL_WO)
    # the set-up is what its name says, from every point of the footprint: the camera sees the receiver, the light's cone is covered / open / cut
    for p in pts:
        assert not blocker.blocks(p, R.unit(eye - p)[None]).any()
        c = R._Cone(l, p)
        rim = R.directions(c.axis, c.cm - 0.02, np.ones(64), (np.arange(64) + 0.5) / 64)         # a rim 0.02 in cos outside the cone: a margin
        covered = blocker.blocks(p, np.concatenate([R.cone_grid(c.axis, c.cm, 16)[0], rim]), c.dist)
        assert {"blocked": covered.all(), "clear": not covered.any(), "edge": 0.3 < covered.mean() < 0.7}[position]

    def est(n, wrong=None, at=None):
        if position == "clear" and wrong is None:                          # the unoccluded case, as the parent module takes it: from the origin
            return R.estimator_expectation(b, OCCL_WO, [l], n=n, eps=eps, min_contribution=0.0)
        return sum(w * R.estimator_expectation(b, R.unit(eye - p), [l], p=p, n=n, eps=eps, min_contribution=0.0, blocker=blocker, wrong=wrong)
                   for p, w in zip(pts, wts))

    if position == "blocked":
        assert not est(16).any()
        return World(Case(sc, None, exact=np.zeros(3), deterministic=1e-30, spp=8), HC, lambda mode, X, n: est(n, mode))
    return World(Case(sc, est, n=EDGE_N if position == "edge" else 48), HC, lambda mode, X, n: est(n, mode))


OCCL_PAIRS = (("matte", "cone"), ("glossy", "sphere"), ("matte", "sphere"), ("glossy", "cone"))
for _m, _l in OCCL_PAIRS + (("glossy", "widecone"),):
    for _p in ("blocked", "clear", "edge"):
        if _l != "widecone" or _p == "edge":
            WORLDS[f"occl-{_m}-{_l}-{_p}"] = functools.partial(occlusion_world, _m, _l, _p)


# ================================================================================================== the placed cases
@dataclasses.dataclass(frozen=True)
class Placed:
    world: str
    route: str                       # flat | baked | moved
    family: tuple = ()               # ((object id, family), ...): the placed objects; every other object sits at the identity


PLACED = {}


def put(world_name, route, family=None, obj=0, tag=None):
    fam = () if family is None else ((obj, family),)
    PLACED[f"{world_name}/{tag or route}" + (f"/{family}" if family else "")] = Placed(world_name, route, fam)


for _r, _f in (("baked", "rot"), ("baked", "x1000"), ("moved", "ident"), ("moved", "rot"), ("moved", "mirror")):
    put("normals-sky-tilted", _r, _f)
for _w, _pairs in (("normals-glossy-cone", (("moved", "x1000"), ("baked", "mirror"))), ("normals-glossy-sphere", (("moved", "x0.001"), ("baked", "rot"))),
                   ("normals-paint-cone", (("moved", "mirror"), ("baked", "x0.001"))), ("normals-paint-sphere", (("moved", "rot"), ("baked", "x1000")))):
    for _r, _f in _pairs:
        put(_w, _r, _f)
for _r in ("baked", "moved"):
    for _f in ("x1000", "x0.001"):
        put("slab", _r, _f)
    put("furnace", _r, "mirror-x1000")
    put("nonuniform-sky-tilted", _r, "nonuniform")
MOVED_OCCLUSION = []
for _p in ("blocked", "clear", "edge"):
    for _m, _l in OCCL_PAIRS:
        put(f"occl-{_m}-{_l}-{_p}", "flat")
    for (_m, _l), _fq, _fr in ((("matte", "cone"), "rot", "mirror"), (("glossy", "sphere"), "x1000", "x0.001")):
        put(f"occl-{_m}-{_l}-{_p}", "moved", _fq, obj=1, tag="quad-moved")
        put(f"occl-{_m}-{_l}-{_p}", "moved", _fr, obj=0, tag="receiver-moved")
        MOVED_OCCLUSION += [f"occl-{_m}-{_l}-{_p}/quad-moved/{_fq}", f"occl-{_m}-{_l}-{_p}/receiver-moved/{_fr}"]
put("occl-glossy-widecone-edge", "flat")
put("occl-glossy-widecone-edge", "moved", "rot", obj=1, tag="quad-moved")
MOVED_OCCLUSION.append("occl-glossy-widecone-edge/quad-moved/rot")


@functools.lru_cache(maxsize=None)
def built(world_name):
    return WORLDS[world_name]()


@functools.lru_cache(maxsize=None)
def wanted(world_name):
    """(want, q) of a world scene, computed once for every route, placement and side"""
    c = built(world_name).case
    if c.want is None:
        return np.asarray(c.exact, np.float64), np.zeros(3)
    fine = c.want(2 * c.n)
    return fine, np.abs(fine - c.want(c.n))


def placed_scene(name):
    """(the scene to load, the transforms to move to or None, the number of objects that are then instances)"""
    pl = PLACED[name]
    w = built(pl.world)
    sc = w.case.scene
    if pl.route == "flat":
        return dataclasses.replace(sc, tri_object=None), None, 0
    n_obj = int(sc.tri_object.max()) + 1
    X = np.tile(IDENT, (n_obj, 1))
    X0 = X.copy()
    pos, nrm = sc.pos.copy(), sc.nrm.copy()
    for ob, fam in pl.family:
        X[ob], X0[ob] = placement(fam, w.extent), placement(fam, w.extent, nudged=True)
        vid = np.unique(sc.tri[sc.tri_object == ob, :3])
        pos[vid], nrm[vid] = R.to_object_space(X[ob], sc.pos[vid], sc.nrm[vid], w.normals)
    if pl.route == "baked":
        return dataclasses.replace(sc, pos=pos, nrm=nrm, obj_xform=X), None, 0
    return dataclasses.replace(sc, pos=pos, nrm=nrm, obj_xform=X0), X, len(pl.family)


def load(b, name):
    """the placed case in the backend b, on its route; the library's own report says whether the route is the one meant"""
    sc, moves, n_inst = placed_scene(name)
    b.load_scene(sc)
    if sc.tri_object is not None:
        assert b.get_tlas()["n_instances"] == 0
    if moves is not None:
        b.set_transforms(moves)
        assert b.get_tlas()["n_instances"] == n_inst > 0, "the moved route must walk an instance"
    return b


# ================================================================================================== the two sides
class Side(E.Side):
    MEASURED = {}

    def image(self, name, spp):
        imgs = []
        for b in (self.ctx, self.twin):
            if b is None:
                continue
            load(b, name).render(spp)
            imgs.append(b.read_hdr())
        if self.twin is not None:
            assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)), "gpu != oracle"
        return imgs[0]

    def measure(self, name):
        key = (self.name, name)
        if key not in self.MEASURED:
            c = built(PLACED[name].world).case
            img = self.image(name, c.spp)
            px = img.reshape(-1, 3).astype(np.float64)
            se = px.std(0, ddof=1) / np.sqrt(len(px))
            if c.variance is not None:
                se = np.maximum(se, np.sqrt(np.maximum(c.variance, 0.0) / (len(px) * c.spp)))
            self.MEASURED[key] = (px.mean(0), se, img)
        return self.MEASURED[key]


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


@pytest.fixture(scope="module")
def gpu_side(oracle_lib, hip_lib):
    from cadrays_amd.view import View
    s = Side("gpu", View(0), oracle_lib.Oracle())
    yield s
    s.close()


@pytest.fixture(scope="module")
def cpu_side(oracle_lib):
    s = Side("cpu", oracle_lib.Oracle())
    yield s
    s.close()


# ================================================================================================== the tests
@pytest.mark.parametrize("name", sorted(PLACED))
def test_expected_radiance(side, name):
    """the acceptance rule of tests/test_integrator_expectation.py, unchanged"""
    c = built(PLACED[name].world).case
    mean, se, img = side.measure(name)
    want, q = wanted(PLACED[name].world)
    if c.deterministic:
        print(f"{name}: want {want} min {img.min((0, 1))} max {img.max((0, 1))}")
        if not want.any():
            assert not img.any(), "the blocked direct term is exactly 0"
        np.testing.assert_allclose(img.reshape(-1, 3), np.broadcast_to(want, (img.shape[0] * img.shape[1], 3)), rtol=c.deterministic, atol=0)
        return
    verdict(name, mean, se, want, q)
    print(f"{name}: SE / want {np.max(se / want):.2g} q / SE {np.max(q / se):.2g}")
    lit = want != 0
    assert lit.all()
    assert (q[lit] <= se[lit] / 10).all(), "the quadrature is too coarse for this case"
    assert (se[lit] <= 0.005 * want[lit]).all(), "too few samples: a pass would mean nothing"
    assert (np.abs(mean - want)[lit] <= Z_PASS * se[lit] + q[lit]).all()


@pytest.mark.parametrize("name", ["nonuniform-sky-tilted/baked/nonuniform", "nonuniform-sky-tilted/moved/nonuniform"])
def test_nonuniform_normals_follow_M_not_the_inverse_transpose(side, name):
    """case E: a non-uniform scale is outside the contract, and the shading normal of such an object follows M; the image is more than 10 standard
    errors away from the expectation under the inverse transpose (and test_expected_radiance holds it to the one under M)"""
    w = built(PLACED[name].world)
    mean, se, _ = side.measure(name)
    phys = w.physical(2 * w.case.n)
    z = verdict(name + " against the inverse transpose", mean, se, phys, np.abs(phys - w.physical(w.case.n)))
    assert (np.abs(z) > Z_POWER).any()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["AUTO", "WIDE", "STAGED"])
@pytest.mark.parametrize("split_passes", ["0", "1"])
@pytest.mark.parametrize("name", MOVED_OCCLUSION)
def test_gpu_moved_occlusion_whichever_walk(gpu_side, monkeypatch, name, split_passes, schedule):
    """the moved roles of case C under both CRH_SPLIT_PASSES settings and every schedule: bit-equal to the oracle's image, which
    test_expected_radiance holds to the expectation"""
    from cadrays_amd import abi
    from cadrays_amd.view import View
    _, _, img = gpu_side.measure(name)
    monkeypatch.setenv("CRH_SPLIT_PASSES", split_passes)
    v = View(0)
    try:
        load(v, name)
        v.set_schedule(getattr(abi, "SCHEDULE_" + schedule))
        v.render(built(PLACED[name].world).case.spp)
        assert np.array_equal(v.read_hdr().view(np.uint32), img.view(np.uint32))
    finally:
        v.close()


# which case must expose which wrong rule: (mode, case)
POWER = [
    ("normals_object_space", "normals-sky-tilted/moved/rot"), ("normals_object_space", "normals-paint-sphere/baked/x1000"),
    ("rotation_transposed", "normals-glossy-cone/baked/mirror"), ("rotation_transposed", "normals-glossy-sphere/moved/x0.001"),
    ("absorb_object_length", "slab/moved/x1000"), ("absorb_object_length", "slab/baked/x0.001"),
    ("shadow_ignores_instances", "occl-matte-cone-edge/quad-moved/rot"), ("shadow_ignores_instances", "occl-glossy-sphere-edge/quad-moved/x1000"),
    ("implicit_ignores_blocker", "occl-glossy-widecone-edge/quad-moved/rot"),
    ("sidedness_from_flipped_ng", "furnace/moved/mirror-x1000"), ("sidedness_from_flipped_ng", "furnace/baked/mirror-x1000"),
]


def test_power_covers_every_wrong_rule():
    assert {m for m, _ in POWER} == set(R.WRONG_INSTANCE)


@pytest.mark.parametrize("mode,name", POWER)
def test_wrong_rules_are_caught(cpu_side, mode, name):
    """CPU only: against the reference with one rule deliberately wrong, the case that pins that rule fails by more than 10 standard errors"""
    pl = PLACED[name]
    w = built(pl.world)
    mean, se, _ = cpu_side.measure(name)
    bad = np.asarray(w.wrong(mode, placement(pl.family[0][1], w.extent), 2 * w.case.n), np.float64)
    z = verdict(f"{name} against '{mode}'", mean, se, bad, np.zeros(3))
    assert (np.abs(z) > Z_POWER).any()
