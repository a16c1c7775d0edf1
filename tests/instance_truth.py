"""Helpers of tests/test_instance_truth.py: scenes whose objects really are instances, their world-space triangles in double precision, and the
double-precision truths of a nearest-hit walk's (t, u, v), of an any-hit query with a finite tmax and of a hit / miss image.

Nothing here includes or restates include/crh_xform.h, crh_math.h or crh_bvh_format.h: a world corner is the float32 vertex under the float32 3x4
matrix, multiplied out in float64 by numpy; rays meet triangles in oracle/brute_force.c (no BVH, no crh_* header)."""
import ctypes as C
import dataclasses

import numpy as np

from cadrays_amd import scenes
from cadrays_amd.materials import BSDF
from test_geometric_truth import bf, brute_f64, check_against_truth, grouped, make_rays

IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
FAMILIES = ("rigid", "translation", "nonuniform", "mirrored", "sheared", "x1000", "squashed")
# moved objects of 27 -> the walk a frame takes (kMaxIBox = 12): no live static triangle: top level only; a split scene; more than kMaxIBox: one walk
CONFIGS = {"all": 27, "split": 9, "onewalk": 18}
SCALES = (0.01, 1.0, 50.0)


def report(**fields):
    """one line per measurement on stdout (pytest -s): docs/instance_truth.md is made of these"""
    print("INSTANCE_TRUTH " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in fields.items()), flush=True)


def objects_of(pos, nrm, tri, n_obj):
    """the soup cut into n_obj objects by centroid cell: the rule of test_geometric_truth.grouped"""
    return grouped(pos, nrm, tri, n_obj, 0)[0].tri_object


def rotation(r):
    a = r.normal(size=3); a /= np.linalg.norm(a)
    ang = r.random() * 2 * np.pi
    cs, sn = np.cos(ang), np.sin(ang); x, y, z = a
    return np.array([[cs + x * x * (1 - cs), x * y * (1 - cs) - z * sn, x * z * (1 - cs) + y * sn],
                     [y * x * (1 - cs) + z * sn, cs + y * y * (1 - cs), y * z * (1 - cs) - x * sn],
                     [z * x * (1 - cs) - y * sn, z * y * (1 - cs) + x * sn, cs + z * z * (1 - cs)]])


def family_xform(family, r, ext):
    """one 3x4 float32 transform of the family; ext: the scene's extent (translations are 0.05 extents, as in grouped())"""
    t = r.normal(size=3) * 0.05 * ext
    if family == "translation":
        A = np.eye(3)
    elif family == "rigid":
        A = rotation(r) * r.uniform(0.6, 1.4)
    elif family == "nonuniform":
        A = rotation(r) @ np.diag(np.exp(r.uniform(np.log(0.3), np.log(3.0), 3)))
    elif family == "mirrored":
        A = rotation(r) @ np.diag([-1.0, 1.0, 1.0]) * r.uniform(0.6, 1.4)
    elif family == "sheared":
        S = np.eye(3); S[0, 1], S[0, 2], S[1, 2] = r.uniform(-0.7, 0.7, 3)
        A = rotation(r) @ S
    elif family == "x1000":
        A = rotation(r) * 1000.0; t = t * 1000.0
    elif family == "squashed":
        D = np.ones(3); D[r.integers(0, 3)] = 1e-4
        A = rotation(r) @ np.diag(D)
    else:
        raise ValueError(family)
    return np.concatenate([A, t[:, None]], 1).astype(np.float32).reshape(12)


def placements(family, n_obj, n_moved, seed, ext):
    """(n_obj, 12) transforms: n_moved objects off the identity; every third of them is only translated (the rule of grouped()), the others take
    `family` ("mixed": the first five families in turn)"""
    r = np.random.default_rng(seed)
    xf = np.tile(IDENT, (n_obj, 1))
    moved = np.sort(r.permutation(n_obj)[:n_moved])
    for k, ob in enumerate(moved):
        fam = FAMILIES[k % 5] if family == "mixed" else family
        xf[ob] = family_xform("translation" if ob % 3 == 0 else fam, r, ext)
    return xf, moved


def world_corners(pos, tri, obj, xf, visible=None):
    """(nT, 3, 3) float64: float32 vertices under the float32 matrices, in double; the triangles of an erased object are all zero (no ray meets them)"""
    world = np.zeros((len(tri), 3, 3), np.float64)
    for ob in range(len(xf)):
        if visible is not None and not visible[ob]:
            continue
        sel = obj == ob
        M = np.asarray(xf[ob], np.float32).reshape(3, 4).astype(np.float64)
        world[sel] = pos[tri[sel, :3]].astype(np.float64) @ M[:, :3].T + M[:, 3]
    return world


def flat9(world):
    return np.ascontiguousarray(world.reshape(-1, 9))


def rays_at(world, n, seed):
    """make_rays on the (live) world triangles; origins spread over the world's extent"""
    live = world[np.abs(world).reshape(len(world), -1).max(1) > 0]
    return make_rays(live.reshape(-1, 3), np.arange(3 * len(live)).reshape(-1, 3), n, seed, float(np.abs(live).max()))


def soup_scene(pos, nrm, tri, obj, xf):
    return scenes.Scene(pos, nrm, tri, [BSDF.CreateDiffuse(0.5)], tri_object=np.ascontiguousarray(obj, np.int32), obj_xform=np.ascontiguousarray(xf, np.float32))


def instanced(make_backend, pos, nrm, tri, obj, xf):
    """the scene built with every object at the identity, then moved: the objects off the identity ARE instances"""
    b = make_backend(soup_scene(pos, nrm, tri, obj, np.tile(IDENT, (len(xf), 1))))
    assert b.get_tlas()["n_instances"] == 0
    b.set_transforms(xf)
    return b


# ------------------------------------------------------------------------------------------------ item 3: t, u, v
def tuv_errors(hits, world, rays, tuv, idx, swap_uv=False):
    """On the rays where walk and truth name the same triangle: |P(u, v) - (o + t64 d)| cos(incidence) and |t - t64| cos(incidence), both over
    (scene size + |t64|), with P = v0 + u (v1 - v0) + v (v2 - v0) from the walk's (u, v) and the float64 corners.  -> (worst uv, worst t, median uv, n)"""
    prim = hits[:, 3].view(np.int32)
    rows = np.where((prim >= 0) & (prim == idx))[0]
    c = world[prim[rows]]
    o, d = rays[rows, :3].astype(np.float64), rays[rows, 4:7].astype(np.float64)
    t64 = tuv[rows, 0]
    u, v = hits[rows, 1].astype(np.float64), hits[rows, 2].astype(np.float64)
    if swap_uv:
        u, v = v, u
    P = c[:, 0] + u[:, None] * (c[:, 1] - c[:, 0]) + v[:, None] * (c[:, 2] - c[:, 0])
    Q = o + t64[:, None] * d
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    dl = np.linalg.norm(d, axis=1)
    cosi = np.abs(np.einsum("ij,ij->i", d, n)) / (np.linalg.norm(n, axis=1) * dl)
    norm = float(np.abs(world).max()) + np.abs(t64) * dl
    e_uv = np.linalg.norm(P - Q, axis=1) * cosi / norm
    e_t = np.abs(hits[rows, 0].astype(np.float64) - t64) * dl * cosi / norm
    return float(e_uv.max()), float(e_t.max()), float(np.median(e_uv)), len(rows)


# ------------------------------------------------------------------------------------------------ item 4: any-hit with a finite tmax
def blockers(world, rays):
    """per ray (nearest t of a robust blocker, nearest t of a possible blocker); inf: none.  The band is the one of _inside_distance."""
    tp = flat9(world)
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.empty((len(rays), 2), np.float64)
    bf().bf_blockers_f64(tp.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(tp)), rays.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(rays)),
                         C.c_double(float(np.abs(tp).max())), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out[:, 0], out[:, 1]


def draw_tmax(t64, hit64, t_rob, t_pos, scene, seed):
    """float32 tmax per ray from {0.5 t64, 2 t64, 1e15, uniform random}, never within 3e-4 (relative) of the truth's hit or of the nearest robust or
    possible blocker: the rules compare at tmax (1 -+ 1e-4), so a tmax drawn 3e-4 away is clear of both thresholds after its rounding to float32, and
    whatever is ambiguous is so for the geometry's sake (a crossing inside the band of an edge), not for tmax's"""
    r = np.random.default_rng(seed)
    n = len(t64)
    kind = np.where(hit64, r.integers(0, 4, n), r.integers(2, 4, n))
    th = np.where(hit64, t64, 1.0)
    uni = r.random(n) * np.where(hit64, 2.0 * th, 3.0 * scene)
    tmax = np.select([kind == 0, kind == 1, kind == 2], [0.5 * th, 2.0 * th, np.full(n, 1e15)], uni)
    tmax = np.maximum(tmax, 1e-30).astype(np.float32)

    def close(tm):
        c = np.zeros(n, bool)
        for t in (np.where(hit64, t64, np.inf), t_rob, t_pos):
            c |= np.isfinite(t) & (np.abs(tm.astype(np.float64) - t) <= 3e-4 * t)
        return c
    for _ in range(4):
        tmax = np.where(close(tmax), tmax * np.float32(1.01), tmax).astype(np.float32)
    assert not close(tmax).any()
    return tmax


def check_any_against_truth(vis, t_rob, t_pos, tmax, aimed, cap=True):
    """vis: trace_any's answer (0 = occluded) for the rays with these tmax.  -> (ambiguous share of the rays not aimed at an edge, of all rays)
    cap=False: the two hard rules only (cases whose share the truth alone puts above the cap; the share is still returned and reported)"""
    tm = tmax.astype(np.float64)
    must_occlude = t_rob < tm * (1 - 1e-4)
    must_see = ~(t_pos < tm * (1 + 1e-4))
    occluded = np.asarray(vis) == 0
    wrong = must_occlude & ~occluded
    assert not wrong.any(), f"{wrong.sum()} rays have a robust blocker below tmax and come out visible (first: ray {np.argmax(wrong)})"
    wrong = must_see & occluded
    assert not wrong.any(), f"{wrong.sum()} rays have no possible blocker below tmax and come out occluded (first: ray {np.argmax(wrong)})"
    ambiguous = ~(must_occlude | must_see)
    share = float(ambiguous[~aimed].mean())
    assert share <= 0.02 or not cap, f"{share:.4f} of the rays not aimed at an edge are ambiguous"
    return share, float(ambiguous.mean())


def with_tmax(rays, tmax):
    out = rays.copy(); out[:, 3] = tmax
    return out


def check_walks(b, world, rays, aimed, seed, tag, walk_tmax_factor=1.0, cap=True):
    """items 2 and 4 for backend b against the world triangles `world`; returns the truth (tuv, idx) of the nearest hit"""
    tp = flat9(world)
    hits = b.trace_nearest(rays)
    n_fp, n_bad = check_against_truth(hits, tp, rays, aimed, False)
    tuv, idx, _ = brute_f64(tp, rays)
    share, share_all, n_occ = check_any_walk(b, world, rays, aimed, seed, tuv, idx, walk_tmax_factor, cap)
    report(what="walks", case=tag, rays=len(rays), hit=int((idx >= 0).sum()), excusable=n_bad, ambiguous_unaimed=share, ambiguous_all=share_all, occluded=n_occ, cap=int(cap))
    return hits, tuv, idx


def check_any_walk(b, world, rays, aimed, seed, tuv, idx, walk_tmax_factor=1.0, cap=True):
    """item 4 for backend b: (tuv, idx) is the nearest-hit truth of `world`, from which tmax is drawn"""
    hit64 = idx >= 0
    t_rob, t_pos = blockers(world, rays)
    tmax = draw_tmax(tuv[:, 0], hit64, t_rob, t_pos, float(np.abs(world).max()), seed)
    vis = b.trace_any(with_tmax(rays, tmax * np.float32(walk_tmax_factor)))
    return check_any_against_truth(vis, t_rob, t_pos, tmax, aimed, cap) + (int((np.asarray(vis) == 0).sum()),)


# ------------------------------------------------------------------------------------------------ item 6: a hit / miss image
def black_scene(sc):
    """every surface absorbs, nothing emits, the background is white: a sample that hits anything contributes 0, one that misses contributes 1"""
    return dataclasses.replace(sc, materials=[BSDF.CreateDiffuse(0.0) for _ in sc.materials], lights=[], env=None,
                               params=dataclasses.replace(sc.params, background=(1.0, 1.0, 1.0)))


def lattice_rays(cam, width, height, sub=4):
    """pinhole rays through the (sub*W + 1) x (sub*H + 1) lattice of sub-pixel positions x + k / sub (pixel corners included), float64 arithmetic from the
    camera's definition: pixel (x, y) covers [x, x + 1] x [y, y + 1] of the image, row 0 at the top.  -> (rays (n, 8) float32, lattice shape)"""
    from camera_reference import basis
    fwd, right, up = basis(cam)
    aspect = float(np.float32(cam.aspect)) if cam.aspect > 0 else width / height
    t = np.tan(np.deg2rad(float(np.float32(cam.fovy_deg))) / 2)
    ly, lx = np.mgrid[0:sub * height + 1, 0:sub * width + 1]
    nx, ny = 2 * (lx / (sub * width)) - 1, 2 * (1.0 - ly / (sub * height)) - 1
    d = fwd + right * (nx * t * aspect)[..., None] + up * (ny * t)[..., None]
    d /= np.linalg.norm(d, axis=-1)[..., None]
    rays = np.zeros((d.shape[0] * d.shape[1], 8), np.float32)
    rays[:, :3] = np.asarray(cam.eye, np.float32); rays[:, 3] = 1e30; rays[:, 4:7] = d.reshape(-1, 3)
    return rays, d.shape[:2]


def pixel_all(lat, sub=4):
    """lat: bool over the lattice -> per pixel: true at all (sub + 1)^2 lattice points of the pixel"""
    h, w = (lat.shape[0] - 1) // sub, (lat.shape[1] - 1) // sub
    out = np.ones((h, w), bool)
    for j in range(sub + 1):
        for i in range(sub + 1):
            out &= lat[j:j + sub * h:sub, i:i + sub * w:sub]
    return out
