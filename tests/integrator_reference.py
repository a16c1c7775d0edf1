"""Float64 expectations of the path integrator -- what `shade_path` and `intersect_light` compose out of BSDF, lights and environment -- written
from the prose of DESIGN.md section 3 ("Lights / environment / integrator") and the contract in include/cadrays_hip.h (crh_light) and
include/crh_spec.h (#3, #6, #9 - #12), on top of tests/bsdf_reference.py and tests/lookup_reference.py.  NOT written from k_shade.h, k_lights_env.h or
oracle/crh_oracle.c, which are transliterations of each other: tests/test_integrator_expectation.py holds the mean of rendered images to these numbers,
so that a composition error the twins share (an MIS weight, a pick probability, a cone, a cut, an offset) shows up.

The shading point is `p` (the origin unless said otherwise) on a surface with the unit shading normal `ns` and the geometric normal `ng`; `wo` is
the WORLD direction towards the viewer.  The set-ups of tests/test_integrator_expectation.py are single surfaces, on which neither a shadow ray nor a
BSDF-sampled ray meets anything again.  tests/test_integrator_instances.py hangs one black quad (`Quad`) over the surface: `blocker=` multiplies the
NEE term and the implicit light term of the BSDF-sampled ray by its visibility predicate -- a ray from p along wi crosses the quad's plane on the
covered or on the open side of its edges, nearer than the light or not -- and the quadrature subdivides the cells an edge cuts.  Nothing else
occludes.  Lights are cadrays_amd.scenes.Light objects:
  directional  a cone of half-angle `smoothness` around the direction TOWARDS the light, -vec
  positional   a cone of half-angle atan(r / d) around the direction to the centre, d = the distance from the ray's origin to the centre
Radiance of a light = colour x intensity.  A light of smoothness 0 is a delta light: not supported here.

Quadrature: midpoint, uniform in (cos, phi) about the cone's axis (about ns for the hemisphere), n x n cells; the cells a discontinuity
cuts are subdivided (`quadrature`).

    physical_direct        integral of f cos L over the lights' cones (+ over the rest of the hemisphere of ns for background / environment)
    estimator_expectation  the expectation of the estimator AS SPECIFIED: one light picked uniformly and sampled in its cone (next event estimation),
                           plus the BSDF-sampled ray picking up what it sees, each with its power-heuristic weight, the NEE sample dropped when
                           every channel of its MIS-weighted contribution is <= min_contribution
    slab_series            an absorbing dielectric slab under a constant sky: reflection + the truncated series of internal reflections

The `wrong=` arguments evaluate deliberately wrong rules on the same cases (test_wrong_rules_are_caught): the tests must be able to fail.

Placed objects (tests/test_integrator_instances.py).  The world scene of a case is fixed; an object is handed over in object space as X^-1 world
(`to_object_space`: float64, then rounded to float32) together with its 3x4 placement X, so the expectation is the world scene's whatever X is.
What a placement does to a shading normal is `carried_normal` (n -> normalize(M n), M the 3x3 part -- the physical rule for
the rigid motions, uniform scales and mirrors of the contract, NOT for a non-uniform scale); the wrong rules of WRONG_INSTANCE restate what a
placement could do wrongly to normals, lengths, sidedness and occlusion.
"""
import numpy as np

import bsdf_reference as B
import lookup_reference as LK

WRONG_ESTIMATOR = ("balance", "no_light_pick", "asin_cone", "cut_throughput", "implicit_per_light")
WRONG_SLAB = ("absorb_outside", "no_eps")
# what a placement could do wrongly (tests/test_integrator_instances.py); each is evaluated where it applies:
#   normals_object_space, rotation_transposed   carried_normal
#   absorb_object_length                        slab_series(scale=)
#   shadow_ignores_instances, implicit_ignores_blocker   estimator_expectation(blocker=)
#   sidedness_from_flipped_ng                   facing_sign
WRONG_INSTANCE = ("normals_object_space", "rotation_transposed", "absorb_object_length", "shadow_ignores_instances", "implicit_ignores_blocker",
                  "sidedness_from_flipped_ng")
WRONG_OCCLUSION = ("shadow_ignores_instances", "implicit_ignores_blocker")


# ================================================================================================== the BSDF, vectorised over wi
# bsdf_reference.py evaluates one direction per call; a quadrature needs 10^5.  These are the same formulas over arrays of wi, lobe by lobe;
# test_integrator_expectation.py::test_vectorised_bsdf_is_bsdf_reference holds them to bsdf_reference.eval_fcos / pdf at rtol 1e-12.
def fresnel_v(cos_i, f):
    """bsdf_reference.fresnel over an array of cosines: (N, 3)"""
    cos_i = np.asarray(cos_i, np.float64)
    tag, c = f[0], np.abs(cos_i)
    if tag > -0.5:
        f0 = np.asarray(f[:3], np.float64)
        return f0 + (1.0 - f0) * ((1.0 - c) ** 5)[:, None]
    if tag > -1.5:
        return np.full(cos_i.shape + (3,), float(f[2]))
    if tag > -2.5:
        n, k = float(f[1]), float(f[2])
        n2k2 = n * n + k * k
        r_perp = (n2k2 - 2 * n * c + c * c) / (n2k2 + 2 * n * c + c * c)
        r_parl = (n2k2 * c * c - 2 * n * c + 1) / (n2k2 * c * c + 2 * n * c + 1)
        return np.repeat((0.5 * (r_perp + r_parl))[:, None], 3, 1)
    n = float(f[1])
    eta_i, eta_t = np.where(cos_i > 0, 1.0, n), np.where(cos_i > 0, n, 1.0)
    sin_t2 = (eta_i / eta_t) ** 2 * (1.0 - cos_i * cos_i)
    ct = np.sqrt(np.maximum(1.0 - sin_t2, 0.0))
    r_parl = (eta_t * c - eta_i * ct) / (eta_t * c + eta_i * ct)
    r_perp = (eta_i * c - eta_t * ct) / (eta_i * c + eta_t * ct)
    return np.repeat(np.where(sin_t2 >= 1.0, 1.0, 0.5 * (r_parl ** 2 + r_perp ** 2))[:, None], 3, 1)


def smith_g1_v(w, m, rough):
    w = np.broadcast_to(w, m.shape)
    wz = w[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        tan_t = np.sqrt(np.maximum(1.0 - wz * wz, 0.0)) / wz
        a = 1.0 / (rough * tan_t)
        g = np.minimum((3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a), 1.0)
    g = np.where(tan_t == 0.0, 1.0, g)
    return np.where(np.einsum("ij,ij->i", w, m) * wz <= 0, 0.0, g)


def _blinn_v(wi, wo, fr, rough):
    """(f cos (N, 3), pdf (N,)) of one Blinn lobe for wi, wo already mirrored into +z; both 0 where wi.z <= 0 or wo.z <= 0"""
    ok = (wi[:, 2] > 0) & (wo[2] > 0)
    h = wi + wo
    h = h / np.linalg.norm(h, axis=1)[:, None]
    e = B.blinn_exponent(rough)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (e + 2.0) / (2.0 * np.pi) * np.abs(h[:, 2]) ** e
        G = smith_g1_v(wo, h, rough) * smith_g1_v(wi, h, rough)
        val = fresnel_v(h @ wo, fr) * (D * G / (4.0 * wo[2]))[:, None]
        pdf = (e + 2.0) / (2.0 * np.pi) * np.abs(h[:, 2]) ** (e + 1.0) / (4.0 * np.abs(np.einsum("ij,ij->i", wi, h)))
    return np.where(ok[:, None], val, 0.0), np.where(ok, pdf, 0.0)


def lobes(b, wo, wi, weight=(1.0, 1.0, 1.0), two_sided=True):
    """The layered BSDF for the local direction wo (3,) and local directions wi (N, 3), lobe by lobe in the order coat, diffuse, glossy:
    (f cos per lobe (3, N, 3), density per lobe times its selection probability (3, N)).  Their sums over the lobes are
    bsdf_reference.eval_fcos and bsdf_reference.pdf.  weight = the path's throughput, which the selection probabilities depend on."""
    wo, wi, W = np.array(wo, np.float64), np.array(wi, np.float64).reshape(-1, 3), np.asarray(weight, np.float64)
    Kc, Rc, Kd, Ks, Rs, Kt, fc, fb = B._parts(b)
    Fc = B.fresnel(float(wo[2]), fc); Tc = 1.0 - Fc
    if two_sided and wo[2] < 0:
        wo[2] = -wo[2]; wi[:, 2] = -wi[:, 2]
    N = len(wi)
    up = (wi[:, 2] > 0) & (wo[2] > 0)
    lam = np.where(up, wi[:, 2] / np.pi, 0.0)
    f = np.zeros((3, N, 3)); p = np.zeros((3, N))
    f[1] = (Kd * Tc) * lam[:, None]; p[1] = lam
    if Rc > B.BSDF_EPS:
        v, q = _blinn_v(wi, wo, fc, Rc); f[0] = Kc * v; p[0] = q
    if Rs > B.BSDF_EPS:
        v, q = _blinn_v(wi, wo, fb, Rs); f[2] = (Ks * Tc) * v; p[2] = q
    sel = np.array([np.dot(Kc * Fc, W), np.dot(Kd * Tc, W), np.dot(Ks * Tc, W)])
    total = sel.sum() + np.dot(Kt * Tc, W)
    p = p * (sel / total)[:, None] if total > B.BSDF_EPS else np.zeros_like(p)
    return f, p


# ================================================================================================== geometry
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def frame(n):
    """an orthonormal frame (t, b, n) around the unit vector n: rows.  The BSDF is isotropic, so which tangent is taken does not matter."""
    n = unit(n)
    t = unit(np.cross(np.eye(3)[int(np.argmin(np.abs(n)))], n))
    return np.stack([t, np.cross(n, t), n])


def directions(axis, cos_max, u_cos, u_phi, cos_min=1.0):
    """the directions at the fractions (u_cos, u_phi) of the cap cos_max <= cos <= cos_min about `axis`, uniform in (cos, phi)"""
    ct, ph = cos_min - np.asarray(u_cos) * (cos_min - cos_max), np.asarray(u_phi) * 2 * np.pi
    st = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    return np.stack([st * np.cos(ph), st * np.sin(ph), ct], -1).reshape(-1, 3) @ frame(axis)


def cone_grid(axis, cos_max, n, cos_min=1.0):
    """midpoint directions (n*n, 3) uniform in (cos, phi) over the cap cos_max <= cos <= cos_min about `axis`, and the solid angle of one cell"""
    u = (np.arange(n) + 0.5) / n
    uc, up = np.meshgrid(u, u, indexing="ij")
    return directions(axis, cos_max, uc, up, cos_min), 2 * np.pi * (cos_min - cos_max) / (n * n)


def quadrature(fn, axis, cos_max, n, sub=16):
    """Midpoint rule over the cap about `axis`, n x n cells uniform in (cos, phi), of fn(w) -> (value (N, 3), class (N,) of ints).  The class
    names the side of every discontinuity the integrand has (a cut, the edge of another light's cone): a cell whose class differs from a
    neighbour's is cut by one and is evaluated on sub x sub cells of its own, so that a cut costs n^-1.5 sub^-1.5 instead of n^-1.5."""
    u = (np.arange(n) + 0.5) / n
    uc, up = np.meshgrid(u, u, indexing="ij")
    val, cls = fn(directions(axis, cos_max, uc, up))
    val, cls = val.reshape(n, n, 3), np.asarray(cls).reshape(n, n)
    edge = np.zeros((n, n), bool)
    d = cls[1:] != cls[:-1]; edge[1:] |= d; edge[:-1] |= d
    d = cls != np.roll(cls, 1, axis=1); edge |= d; edge |= np.roll(d, -1, axis=1)            # phi wraps
    dw = 2 * np.pi * (1.0 - cos_max) / (n * n)
    total = val[~edge].sum(0) * dw
    if edge.any():
        i, j = np.nonzero(edge)
        s = (np.arange(sub) + 0.5) / sub
        uc = np.broadcast_to((i[:, None, None] + s[None, :, None]) / n, (len(i), sub, sub))
        up = np.broadcast_to((j[:, None, None] + s[None, None, :]) / n, (len(i), sub, sub))
        total = total + fn(directions(axis, cos_max, uc.ravel(), up.ravel()))[0].sum(0) * dw / (sub * sub)
    return total


def emission(l):
    return np.asarray(l.color, np.float64) * float(l.intensity)


def scene_epsilon(pos, rule=0):
    """crh_spec.h #6 from the scene's vertices: max(1e-6, 1e-5 |diagonal|)  (rule 1: 1e-4 x the radius)"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    diag = np.linalg.norm(pos.max(0) - pos.min(0))
    return max(1e-6, 1e-4 * diag / 2 if rule else 1e-5 * diag)


class Quad:
    """A parallelogram that blocks light: corners (4, 3) in order around it, world space, float64.  `blocks` is the visibility predicate: the ray
    from o along w crosses the quad's plane at 0 < t < tmax and does so on the covered side of all four edge lines (the set-ups of the tests put
    ONE edge near the rays; the other three lie far outside every cone)."""

    def __init__(self, corners):
        c = np.asarray(corners, np.float64).reshape(4, 3)
        self.c, self.e1, self.e2 = c[0], c[1] - c[0], c[3] - c[0]
        assert np.allclose(c[2], c[0] + self.e1 + self.e2)
        self.n = np.cross(self.e1, self.e2)
        self.gram = np.linalg.inv(np.array([[self.e1 @ self.e1, self.e1 @ self.e2], [self.e1 @ self.e2, self.e2 @ self.e2]]))

    def blocks(self, o, w, tmax=np.inf):
        """o: one origin (3,) or one per direction (N, 3); w (N, 3)"""
        w, o = np.asarray(w, np.float64).reshape(-1, 3), np.asarray(o, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - o) @ self.n) / (w @ self.n)
            x = o + t[:, None] * w - self.c
            a, b = self.gram @ np.stack([x @ self.e1, x @ self.e2])
            return (t > 0) & (t < tmax) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)


def rotation(axis, angle):
    """the rotation matrix by `angle` about `axis` (Rodrigues)"""
    x, y, z = unit(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], np.float64)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def xform(A, t=(0, 0, 0)):
    """the 3x4 placement (row-major, 12 floats) as the library takes it: float32"""
    return np.concatenate([np.asarray(A, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(np.float32).reshape(12)


def to_object_space(X, pos, nrm, normals="contract"):
    """World vertices and unit normals -> the object space of the placement X (12 float32): X^-1 applied in float64 to the float32 matrix, rounded
    to float32.  normals='contract': n_obj = normalize(M^-1 n), whose image under carried_normal is n again; for the rigid motions, uniform scales
    and mirrors of the contract that is the physical rule too.  normals='covector': n_obj = normalize(M^T n), the object normal whose PHYSICAL
    image (inverse transpose) is n -- for the case that pins that a non-uniform scale does NOT carry normals that way."""
    M = np.asarray(X, np.float32).reshape(3, 4).astype(np.float64)
    A, t = M[:, :3], M[:, 3]
    Ai = np.linalg.inv(A)
    p = (np.asarray(pos, np.float64) - t) @ Ai.T
    n = np.asarray(nrm, np.float64) @ (Ai.T if normals == "contract" else A)
    n = n / np.linalg.norm(n, axis=1)[:, None]
    return p.astype(np.float32), n.astype(np.float32)


def carried_normal(X, n_obj, wrong=None):
    """the world shading normal of an object-space normal under the placement X.  As specified: normalize(M n_obj).
    wrong: None | 'normals_object_space' (n_obj itself) | 'rotation_transposed' (M^T) | 'inverse_transpose' (the physical rule for a covector:
    not a wrong rule under the contract, where it names the same direction; the yardstick of the non-uniform case)"""
    A = np.asarray(X, np.float32).reshape(3, 4).astype(np.float64)[:, :3]
    n = np.asarray(n_obj, np.float64)
    if wrong == "normals_object_space":
        return unit(n)
    if wrong == "rotation_transposed":
        return unit(A.T @ n)
    if wrong == "inverse_transpose":
        return unit(np.linalg.inv(A).T @ n)
    if wrong is not None:
        raise ValueError(wrong)
    return unit(A @ n)


def facing_sign(X, wrong=None):
    """+1: the side of a surface its carried shading normal names is the side the world scene means.  Under 'sidedness_from_flipped_ng' the side
    follows the geometric normal of the OBJECT-space winding, which a mirror (det < 0) turns over: -1."""
    A = np.asarray(X, np.float32).reshape(3, 4).astype(np.float64)[:, :3]
    if wrong == "sidedness_from_flipped_ng":
        return 1.0 if np.linalg.det(A) > 0 else -1.0
    if wrong is not None:
        raise ValueError(wrong)
    return 1.0


class _Cone:
    """what one light is from the origin o: axis, cos of the half-angle, the cone's density, the distance (inf: directional)"""

    def __init__(self, l, o, wrong=None):
        self.light, self.L = l, emission(l)
        if l.is_point:
            tl = np.asarray(l.vec, np.float64) - o
            self.dist = np.linalg.norm(tl); self.axis = tl / self.dist
            half = np.arcsin(min(l.smoothness / self.dist, 1.0)) if wrong == "asin_cone" else np.arctan(l.smoothness / self.dist)
        else:
            self.dist = np.inf; self.axis = -unit(l.vec)
            half = float(l.smoothness)
        if not half > 0:
            raise NotImplementedError("delta lights have no cone")
        self.cm = np.cos(half)
        self.pdf = 1.0 / (2 * np.pi * (1.0 - self.cm))

    def covers(self, w):
        return w @ self.axis >= self.cm


class _Point:
    """the shading point: local frame of ns, local wo, and the two origins rays leave from"""

    def __init__(self, b, wo, ns, ng, p, weight, two_sided):
        self.b, self.W, self.two = b, np.asarray(weight, np.float64), two_sided
        self.ns, self.ng, self.p = unit(ns), unit(ng), np.asarray(p, np.float64)
        self.fr = frame(self.ns)
        self.wo = self.fr @ unit(wo)

    def lobes(self, w):
        return lobes(self.b, self.wo, w @ self.fr.T, self.W, self.two)

    def offset(self, d, eps):
        """where a ray along d starts: eps along the ray, eps along Ng on the ray's side"""
        return self.p + eps * (d + (1.0 if self.ng @ d >= 0 else -1.0) * self.ng)

    def offsets(self, d, eps):
        """`offset` for directions (N, 3): (N, 3)"""
        return self.p + eps * (d + np.where(d @ self.ng >= 0, 1.0, -1.0)[:, None] * self.ng)

    def side(self):
        return -1.0 if (self.two and self.wo[2] < 0) else 1.0


def _env_radiance(env, background, w, orientation, gamma2):
    if env is None:
        return np.broadcast_to(np.asarray(background, np.float64), w.shape)
    return LK.env_ref(env, w.astype(np.float32), orientation, gamma2)[0]


def _sky_term(pt, seen, env, background, n, orientation=0, gamma2=False):
    """integral of f cos L over the hemisphere of ns on wo's side, outside the cones of `seen`, of the background or the environment map"""
    if env is None and not np.any(np.asarray(background, np.float64) != 0):
        return np.zeros(3)

    def fn(w):
        free = np.ones(len(w), bool)
        for c in seen:
            free &= ~c.covers(w)
        return pt.lobes(w)[0].sum(0) * _env_radiance(env, background, w, orientation, gamma2) * free[:, None], free

    return quadrature(fn, pt.side() * pt.ns, 0.0, n)


# ================================================================================================== the two expectations
def physical_direct(b, wo, lights, ns=(0, 0, 1), ng=None, p=(0, 0, 0), env=None, background=(0, 0, 0), two_sided=True, n=64, n_sky=None,
                    env_orientation=0, texel_gamma2=False, wrong=None):
    """integral of f cos L d omega (rgb): over each light's cone as seen from p, and over the rest of the hemisphere of ns for the background or
    the environment map.  Where cones overlap the radiances add.  wrong: None | 'asin_cone'"""
    pt = _Point(b, wo, ns, ns if ng is None else ng, p, (1, 1, 1), two_sided)
    cones = [_Cone(l, pt.p, wrong) for l in lights]
    out = np.zeros(3)
    for c in cones:
        out += quadrature(lambda w: (pt.lobes(w)[0].sum(0) * c.L, np.zeros(len(w), int)), c.axis, c.cm, n)
    return out + _sky_term(pt, cones, env, background, n_sky or n, env_orientation, texel_gamma2)


def _mis(a, other, balance):
    """weight of the strategy with density a against the one with density `other`, times 1 / a: a / (a^2 + other^2)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / (a + other) if balance else a / (a * a + other * other)
    return np.where(a > 0, r, 0.0)


def estimator_expectation(b, wo, lights, ns=(0, 0, 1), ng=None, p=(0, 0, 0), env=None, background=(0, 0, 0), weight=(1, 1, 1), two_sided=True,
                          min_contribution=1e-2, min_throughput=0.0, mis_single_lobe=False, eps=0.0, n=64, n_sky=None, env_orientation=0, texel_gamma2=False, wrong=None,
                          parts=False, blocker=None):
    """The expectation (rgb, times `weight`) of the estimator DESIGN.md section 3 specifies for a path of throughput `weight` that arrives at p:

    NEE    one of the n_l lights, each with probability 1 / n_l, a direction uniform in its cone as seen from p (density p_c), so p_e = p_c / n_l;
           the sample's value is L f cos p_e / (p_e^2 + p_i^2), p_i = the mixture density of BSDF sampling for that direction, and it is DROPPED
           when every channel of that value -- the throughput is not in it -- is <= min_contribution:
               sum_i  1 / n_l  integral over cone i of  p_c [value > cut] value
    BSDF   the sampled ray leaves from p + eps (d + Ng) (Ng on the ray's side) and picks up L_seen with p_i^2 / (p_exp^2 + p_i^2):
               integral of f cos L_seen p_i^2 / (p_exp^2 + p_i^2)
           L_seen and p_exp by the rule of crh_light: a positional light whose cone (from the RAY'S origin) holds the direction is seen, the nearest
           one, alone, with p_exp = its own p_c / n_l; else the directional cones that hold the direction ADD, radiance and density alike; else the
           background / environment with p_exp = 0.  (The offset origin enters through the cone's axis; its dependence on the direction within one
           cone -- eps x the half-angle -- is neglected: 1e-4 of the solid angle in the tests' set-ups.)
           With mis_single_lobe (crh_spec.h #3) p_i is, lobe by lobe, the sampled lobe's density times its selection probability.
           The ray is traced only while a channel of the new throughput, weight x (f cos / p) of the sampled lobe, exceeds min_throughput (#12;
           applied to the lights' cones; the sky term is taken whole).

    wrong: None | 'balance' (balance heuristic on both sides) | 'no_light_pick' (p_e = p_c on the NEE side) | 'asin_cone' (the sphere's outline)
           | 'cut_throughput' (the cut tests weight x value) | 'implicit_per_light' (overlapping cones weighted one by one on the BSDF side)
    parts: return (nee, bsdf) instead of their sum.

    blocker: a Quad of a black material between the surface and the lights.  A shadow ray is stopped by it below tmax = the distance to a positional
           light's centre (anywhere for a directional light); a BSDF-sampled ray that meets it sees a positional light only when the light's centre
           is nearer than the quad, never a directional one, and ends on the quad, which neither emits nor reflects.  Both terms are multiplied
           by that visibility.  Either ray leaves from its own offset origin p + eps (d + Ng): against a quad 1400 eps away that moves the
           crossing by eps x the ray's slope, 0.1 - 0.2 % of the light an edge through the cone's axis lets pass -- a third of the standard error
           the tests work at, so it is in.  Needs a black background and no map.
           wrong: 'shadow_ignores_instances' (the NEE term takes no notice of the quad) | 'implicit_ignores_blocker' (the BSDF-sampled ray's)"""
    if wrong is not None and wrong not in WRONG_ESTIMATOR + WRONG_OCCLUSION:
        raise ValueError(wrong)
    if blocker is not None and (env is not None or np.any(np.asarray(background, np.float64) != 0)):
        raise NotImplementedError("a blocker under a sky")
    pt = _Point(b, wo, ns, ns if ng is None else ng, p, weight, two_sided)
    nee_sees = (lambda w, c: np.ones(len(w), bool)) if (blocker is None or wrong == "shadow_ignores_instances") else \
        (lambda w, c: ~blocker.blocks(pt.offsets(w, eps), w, c.dist))
    imp_sees = (lambda w, c: np.ones(len(w), bool)) if (blocker is None or wrong == "implicit_ignores_blocker") else \
        (lambda w, c: ~blocker.blocks(pt.offsets(w, eps), w, c.dist))
    nl = len(lights)
    balance = wrong == "balance"
    nee, imp = np.zeros(3), np.zeros(3)
    # ---- next event estimation
    for l in lights:
        c = _Cone(l, pt.p, wrong)
        p_e = c.pdf if wrong == "no_light_pick" else c.pdf / nl

        def sample(w, c=c, p_e=p_e):
            f, pl = pt.lobes(w)
            value = f.sum(0) * c.L * _mis(p_e, pl.sum(0), balance)[:, None]
            keep = ((value * pt.W if wrong == "cut_throughput" else value) > min_contribution).any(1)
            open_ = nee_sees(w, c)
            return value * (keep & open_)[:, None], 2 * keep.astype(np.int64) + open_

        nee += quadrature(sample, c.axis, c.cm, n) * c.pdf / nl
    # ---- the BSDF-sampled ray
    seen = [_Cone(l, pt.offset(_Cone(l, pt.p, wrong).axis, eps), wrong) for l in lights]
    for i, c in enumerate(seen):
        def sampled(w, i=i, c=c):
            f, pl = pt.lobes(w)
            hidden = np.zeros(len(w), bool)
            p_exp = np.full(len(w), c.pdf / nl)
            cls = np.zeros(len(w), np.int64)
            for j, o in enumerate(seen):
                if j == i:
                    continue
                inside = o.covers(w)
                if o.light.is_point:
                    if (not c.light.is_point) or o.dist < c.dist or (o.dist == c.dist and j < i):
                        hidden |= inside                               # a positional light in front: it is seen instead, alone
                elif not c.light.is_point and wrong != "implicit_per_light":
                    p_exp = p_exp + np.where(inside, o.pdf / nl, 0.0)  # directional cones add, density like radiance
                cls = 2 * cls + inside
            with np.errstate(divide="ignore", invalid="ignore"):       # the ray is traced while a channel of weight x f cos / p of its lobe exceeds the cut
                alive = [((pt.W * f[k] / pl[k][:, None]) > min_throughput).any(1) & (pl[k] > 0) for k in range(3)]
            pi = pl.sum(0)
            val = sum(f[k] * (alive[k] * (pl[k] * _mis(pl[k], p_exp, balance) if mis_single_lobe else pi * _mis(pi, p_exp, balance)))[:, None]
                      for k in range(3))
            for k in range(3):
                cls = 2 * cls + alive[k]
            open_ = imp_sees(w, c)
            return val * (~hidden & open_)[:, None] * c.L, 2 * cls + open_

        imp += quadrature(sampled, c.axis, c.cm, n)
    imp += _sky_term(pt, seen, env, background, n_sky or n, env_orientation, texel_gamma2)
    nee, imp = nee * pt.W, imp * pt.W
    return (nee, imp) if parts else nee + imp


# ================================================================================================== slab
def slab_series(ior, thickness, coeff, colour, theta, max_depth, eps=0.0, sky=1.0, cam_dist=0.0, wrong=None, moments=False, scale=1.0):
    """An absorbing dielectric slab (faces z = 0 and z = -thickness, absorption `coeff` x (1 - colour) per unit length) seen at the incidence
    theta under a constant sky: what leaves towards the viewer's ray, per channel.

    Ray 0 is the camera ray.  It is reflected (exact unpolarised Fresnel R, the same from either side at the matching angles) and leaves as ray 1, or
    enters (T = 1 - R) and crosses the slab k times, reflected k - 1 times inside, before it leaves as ray k + 1:  T^2 R^(k-1) A^k.  A path is
    max_depth rays long, so a ray that leaves sees the sky only when its index is <= max_depth - 1: k <= max_depth - 2.
    A ray inside starts eps along itself and eps along the face's normal off the face it left: a crossing is (thickness - eps) / cos(theta_t) - eps
    long, and A = exp(-coeff (1 - colour) x that length).

    Without roulette every event is a delta lobe picked with its Fresnel probability and weight 1, so a path returns sky x A^k with probability
    T^2 R^(k-1) (sky with probability R, nothing with what is left): moments=True returns (mean, second moment) of one path.

    wrong: None | 'no_eps' (crossings thickness / cos(theta_t) long) | 'absorb_outside' (the segment OUTSIDE the slab -- the camera ray, cam_dist
    long -- absorbs, the crossings do not) | 'absorb_object_length' (the slab is an object placed with the uniform scale `scale`, and a crossing
    absorbs over its length in OBJECT units, 1 / scale of the world length)"""
    if wrong is not None and wrong not in WRONG_SLAB + ("absorb_object_length",):
        raise ValueError(wrong)
    f = (-3.0, float(ior), 0.0, 0.0)
    ci = np.cos(theta)
    R = B.fresnel(float(ci), f)[0]
    st = np.sin(theta) / ior
    ct = np.sqrt(1.0 - st * st)
    assert abs(B.fresnel(-float(ct), f)[0] - R) < 1e-12          # from inside at the refracted angle: the same R
    e = 0.0 if wrong == "no_eps" else eps
    seg = (thickness - e) / ct - e
    sigma = coeff * (1.0 - np.asarray(colour, np.float64))
    A = np.exp(-sigma * (seg / scale if wrong == "absorb_object_length" else seg))
    pre = 1.0
    if wrong == "absorb_outside":
        A = np.ones(3); pre = np.exp(-sigma * cam_dist)
    T = 1.0 - R
    out, m2 = np.zeros(3), np.zeros(3)
    if max_depth >= 2:
        out, m2 = out + R, m2 + R
    for k in range(1, max_depth - 1):
        out = out + T * T * R ** (k - 1) * A ** k
        m2 = m2 + T * T * R ** (k - 1) * A ** (2 * k)
    sky = np.asarray(sky, np.float64)
    if moments:
        return out * pre * sky, m2 * (pre * sky) ** 2
    return out * pre * sky
