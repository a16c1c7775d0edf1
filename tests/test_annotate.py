"""Annotations: world-space line segments over the display, depth-tested (crh_annotate.cpp, cadrays_amd/csrc/annotate_kernels.hip).

The reference has no counterpart: it paints its manipulator and its light markers with ImGui over the finished image (src/ImGui/ImRaytraceControls.cxx:64, :93-111).
Everything is compared bit for bit; no tolerance appears in this file.

  CPU   the structs' layout and the exports; every refusal of the host entry points; crh_annot_project_host == the numpy restatement (tests/annotate_reference.py,
        written from the header's text) over the camera sweep of test_display_chain and the segments the issue lists; crh_annot_draw_host == numpy on synthetic
        t planes; each deliberately wrong rule changes an output; the builders of cadrays_amd/annotations.py
  GPU   on the two-level Cornell room at 67 x 45 and 130 x 70: known answers under an orthographic camera; the device's records == the twin == numpy; the id plane and
        the LDR bytes == the twin == numpy over the bytes read with the feature off, through list sizes, cameras and the states of a live scene; the read-out paths;
        staleness; nothing else moves
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import annotate_reference as ref
from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_display_chain import both_slots, camera_sweep
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("crh_annot_defaults", "crh_set_annotations", "crh_get_annotations", "crh_read_annotation_ids", "crh_pick_annotation", "crh_read_annotation_records",
         "crh_bench_annotations", "crh_annot_project_host", "crh_annot_draw_host")
SIZES = ((67, 45), (130, 70))


def _api():
    """the host-only entry points through the Python mirror: a missing one FAILS here (AttributeError / ImportError), it does not skip"""
    from cadrays_amd.view import annot_draw_host, annot_project_host, reproject_frame_host
    return annot_project_host, annot_draw_host, reproject_frame_host


def seg_list(rows):
    """rows of (a, b, rgb, alpha, width, mode)"""
    out = np.zeros(len(rows), ref.SEGMENT_DTYPE)
    for i, (a, b, rgb, alpha, width, mode) in enumerate(rows):
        out[i] = (a, b, rgb, alpha, ref.style(width, mode))
    return out


def random_segments(n, seed, lo=-0.4, hi=1.4):
    """n segments around and through the unit room: mixed modes, widths 1..8, alphas, a point marker every 16th"""
    r = np.random.default_rng(seed)
    out = np.zeros(n, ref.SEGMENT_DTYPE)
    out["a"] = r.uniform(lo, hi, (n, 3)); out["b"] = out["a"] + r.normal(0.0, 0.35, (n, 3))
    out["b"][::16] = out["a"][::16]
    out["rgb"] = r.integers(0, 256, (n, 3)); out["alpha"] = r.choice([0, 1, 64, 128, 200, 255], n)
    out["style"] = r.integers(1, 9, n) | (r.integers(0, 3, n) << 8)
    return out


def same_records(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_annotation_structs_layout_matches_header(tmp_path):
    probes = []
    for st in (abi.crh_annot_segment, abi.crh_annot_params):
        name = st.__name__
        probes.append(f'printf("%zu ", sizeof({name}));' + "".join(f'printf("%zu ", offsetof({name}, {n}));' for n, _ in st._fields_))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){' + "".join(probes) +
           'printf("%u %u %u %u %u", CRH_ANNOT_ON_TOP, CRH_ANNOT_HIDE, CRH_ANNOT_XRAY, CRH_ANNOT_MAX_SEGMENTS, CRH_ANNOT_STYLE(5, CRH_ANNOT_XRAY));return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    want = []
    for st in (abi.crh_annot_segment, abi.crh_annot_params):
        want += [C.sizeof(st)] + [getattr(st, n).offset for n, _ in st._fields_]
    want += [abi.ANNOT_ON_TOP, abi.ANNOT_HIDE, abi.ANNOT_XRAY, abi.ANNOT_MAX_SEGMENTS, abi.annot_style(5, abi.ANNOT_XRAY)]
    assert got == want, (got, want)
    assert C.sizeof(abi.crh_annot_segment) == 32 and C.sizeof(abi.crh_annot_params) == 8
    assert np.dtype(abi.ANNOT_SEGMENT_DTYPE) == ref.SEGMENT_DTYPE and np.dtype(abi.ANNOT_RECORD_DTYPE) == ref.RECORD_DTYPE and ref.RECORD_DTYPE.itemsize == 32
    assert (abi.ANNOT_ON_TOP, abi.ANNOT_HIDE, abi.ANNOT_XRAY) == (ref.ON_TOP, ref.HIDE, ref.XRAY) and abi.annot_style(5, 2) == ref.style(5, 2) == 0x205
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS and (f"CRH_API int {name}(" in header or f"CRH_API void {name}(" in header), name
    section = header[header.index("/* --- annotations"):header.index("/* --- kernel-level entry points")]
    assert section.count("no counterpart in the reference") >= len(NAMES) and "ImRaytraceControls.cxx:64" in section and ":93-111" in section


def test_entry_points_are_exported_and_defaults_agree(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    p = abi.crh_annot_params(7.0, 7)
    hip_lib.crh_annot_defaults.restype = None
    hip_lib.crh_annot_defaults(C.byref(p))
    assert (f32(p.depth_bias), p.hidden_alpha) == (f32(abi.ANNOT_DEFAULTS["depth_bias"]), abi.ANNOT_DEFAULTS["hidden_alpha"]) == (f32(2.0 ** -9), 64)
    assert (ref.DEFAULT_BIAS, ref.DEFAULT_HIDDEN) == (f32(2.0 ** -9), 64)


# ------------------------------------------------------------------------------------------------ CPU 2: the refusals of the host entry points
def bad_lists():
    ok = (0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (1, 2, 3), 255
    yield "width 0", seg_list([ok + (0, 0)])
    yield "width 9", seg_list([ok + (9, 0)])
    yield "mode 3", seg_list([ok + (1, 3)])
    for bit in (4, 7, 10, 16, 31):
        s = seg_list([ok + (1, 0)]); s["style"] |= np.uint32(1 << bit)
        yield f"style bit {bit}", s
    for k, v in ((0, np.nan), (2, np.inf), (1, -np.inf)):
        for end in "ab":
            s = seg_list([ok + (1, 0), ok + (2, 1)]); s[end][1, k] = v
            yield f"{end}[{k}] = {v}", s


def test_refusals_of_the_host_entry_points(hip_lib):
    project_host, draw_host, _ = _api()
    cam = scenes.Camera()
    good = seg_list([((0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (1, 2, 3), 255, 1, 0)])
    rec = project_host(cam, 8, 8, good)
    img = np.zeros((8, 8, 3), np.uint8)
    draw_host(rec, good, cam, 8, 8, ldr=img)
    for why, bad in bad_lists():
        with pytest.raises(BackendError):
            project_host(cam, 8, 8, bad)
        with pytest.raises(BackendError):
            draw_host(np.zeros(len(bad), ref.RECORD_DTYPE), bad, cam, 8, 8, ldr=img)
    for w, h in ((0, 8), (8, 0)):
        with pytest.raises(BackendError):
            project_host(cam, w, h, good)
    for kw in (dict(depth_bias=-1.0e-3), dict(depth_bias=np.nan), dict(depth_bias=np.inf), dict(hidden_alpha=256)):
        with pytest.raises(BackendError):
            draw_host(rec, good, cam, 8, 8, ldr=img, **kw)
    hidden = seg_list([((0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (1, 2, 3), 255, 1, ref.HIDE)])
    with pytest.raises(BackendError):                          # a segment that asks for depth, and no planes
        draw_host(project_host(cam, 8, 8, hidden), hidden, cam, 8, 8, ldr=img)
    sg, rc = (abi.crh_annot_segment * 1)(), (C.c_uint8 * 32)()
    sg[0].style = 1
    cs = abi.crh_camera(); cs.dir[1] = 1.0; cs.up[2] = 1.0; cs.fovy_deg = 45.0
    assert hip_lib.crh_annot_project_host(None, 8, 8, sg, 1, rc) == abi.E_INVALID
    assert hip_lib.crh_annot_project_host(C.byref(cs), 8, 8, None, 1, rc) == abi.E_INVALID
    assert hip_lib.crh_annot_project_host(C.byref(cs), 8, 8, sg, 1, None) == abi.E_INVALID
    assert hip_lib.crh_annot_project_host(C.byref(cs), 8, 8, sg, 1, rc) == abi.OK
    assert hip_lib.crh_annot_draw_host(rc, sg, 1, None, C.byref(cs), 8, 8, None, None, None, None) == abi.E_INVALID      # neither output


# ------------------------------------------------------------------------------------------------ CPU 3: the projection
def issue_segments(F):
    """the segments the issue lists, placed in the camera's own frame so that every camera of the sweep meets every case"""
    eye, r, u, f = (np.asarray(F[k], np.float64) for k in ("eye", "right", "up", "fwd"))
    at = lambda x, y, z: tuple(f32(eye + x * r + y * u + z * f))
    def ndc(nx, ny, z):                                        # the point at depth z that lands at (nx, ny) of the frame, -1 .. 1 across it
        k = float(F["ortho_scale"]) if F["is_ortho"] else z * float(F["tan_half"])
        return at(nx * k * float(F["aspect"]), ny * k, z)
    den = float(np.float32(1.0e-45)) * 3.0
    rows = [(ndc(-0.4, 0.2, 2.0), ndc(0.6, -0.4, 3.0)),       # 0: both end points in view
            (ndc(0.2, 0.2, 2.0), at(0.4, -0.3, -1.0)),        # 1: one behind the eye
            (at(-0.3, 0.2, -1.0), ndc(0.2, 0.1, 1.5)),        # 2: ... the other one
            (at(0.1, 0.1, -2.0), at(0.4, -0.3, -0.5)),        # 3: both behind the eye
            (tuple(f32(eye)), ndc(0.4, 0.2, 2.0)),            # 4: one exactly on z = 0 (the eye itself: v = 0)
            (at(0.3, 0.0, 0.0), ndc(-0.2, 0.3, 1.0)),         # 5: ... beside the eye (exactly on z = 0 under the axis-aligned cameras)
            (ndc(-2.0e6, 0.0, 1.0), ndc(2.0e6, 0.0, 1.0)),    # 6: 1e6 frame widths outside, both sides
            (ndc(5.0, 5.0, 1.0), ndc(5.0, 8.0, 1.0)),         # 7: entirely outside the guard band
            (ndc(0.2, -0.2, 2.5), ndc(0.2, -0.2, 2.5)),       # 8: zero length
            (ndc(0.0, 2.0e6, 2.0), ndc(0.1, 0.0, 2.0)),       # 9: 1e6 frame heights outside, one side
            ((den, -den, den), (2.0 * den, den, 0.0)),        # 10: denormal coordinates
            ((den, 0.0, 0.0), ndc(0.0, 0.0, 1.0)),
            ((3.0e38, 3.0e38, 3.0e38), ndc(0.0, 0.0, 1.0)),   # 12: 3e38 coordinates
            ((-3.0e38, 3.0e38, -3.0e38), (3.0e38, -3.0e38, 3.0e38)),
            ((3.0e38, 0.0, 0.0), (3.0e38, 1.0, 0.0))]
    return seg_list([(a, b, (255, 255, 255), 255, 1, 0) for a, b in rows])


def test_project_host_equals_the_numpy_restatement(hip_lib):
    project_host, _, frame_host = _api()
    n = n_valid = n_clipped = 0
    for cam in camera_sweep():
        for W, H in SIZES:
            F = frame_host(cam, W, H)
            segs = issue_segments(F)
            got, want = project_host(cam, W, H, segs), ref.project(F, W, H, segs)
            assert same_records(got, want), (cam, W, H, [(i, got[i], want[i]) for i in range(len(segs)) if got[i] != want[i]][:3])
            assert got["flags"][0] == 1 and got["flags"][3] == 0 and got["flags"][7] == 0 and got["flags"][8] == 1, (cam, got)
            assert got["x0"][8] == got["x1"][8] and got["y0"][8] == got["y1"][8]
            ok = got[got["flags"] == 1]
            assert (ok["x0"] >= -W).all() and (ok["x1"] <= 2 * W).all() and (ok["y0"] >= -H).all() and (ok["y1"] <= 2 * H).all()
            n += 1; n_valid += int((got["flags"] == 1).sum()); n_clipped += int(got["flags"][6]) + int(got["flags"][9])
    assert n >= 128 and n_valid > 5 * n and n_clipped > n
    # a list of random segments around the room, under the room's cameras
    segs = random_segments(500, 1)
    for cam in (scenes.Camera(eye=(0.5, -1.45, 0.5)), scenes.Camera(eye=(0.5, -1.45, 0.5), is_ortho=True, ortho_scale=0.5), scenes.Camera(eye=(0.5, 0.5, 0.5), dir=(0.3, 1.0, -0.2))):
        F = frame_host(cam, 67, 45)
        got = project_host(cam, 67, 45, segs)
        assert same_records(got, ref.project(F, 67, 45, segs)) and 100 < (got["flags"] == 1).sum()


# ------------------------------------------------------------------------------------------------ CPU 4: the pixel rule on synthetic planes
def synthetic(cam, W, H, seed):
    """rays as the pixel-centre pinhole gives them (float64, rounded once: the rule only reads them) and a t plane of three depths and misses"""
    _, _, frame_host = _api()
    F = frame_host(cam, W, H)
    r = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    nx, ny = x / W * 2 - 1, 1 - y / H * 2
    rays = np.zeros((H, W, 8), f32)
    if cam.is_ortho:
        rays[..., 4:7] = F["fwd"]
    else:
        d = (F["fwd"].astype(np.float64) + (nx * float(F["tan_half"]) * float(F["aspect"]))[..., None] * F["right"] + (ny * float(F["tan_half"]))[..., None] * F["up"])
        rays[..., 4:7] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    t = r.choice(np.array([1.5, 2.45, 3.25, 1.0e15], f32), (H, W))
    t[:, W // 2:] = np.where(t[:, W // 2:] < 1e15, t[:, W // 2:] + r.uniform(-0.2, 0.2, (H, W - W // 2)).astype(f32), t[:, W // 2:])
    return F, rays.reshape(-1, 8), t.astype(f32)


CAMS = {"perspective": scenes.Camera(eye=(0.5, -1.45, 0.5)), "orthographic": scenes.Camera(eye=(0.5, -1.45, 0.5), is_ortho=True, ortho_scale=0.5),
        "oblique": scenes.Camera(eye=(0.4, -1.0, 0.7), dir=(0.2, 1.0, -0.15), up=(0.1, 0.0, 1.0), fovy_deg=70.0)}


@pytest.mark.parametrize("which", list(CAMS))
def test_draw_host_equals_the_numpy_rule_on_synthetic_planes(hip_lib, which):
    project_host, draw_host, _ = _api()
    cam = CAMS[which]
    for (W, H), n in (((67, 45), 300), ((33, 21), 33)):
        F, rays, t = synthetic(cam, W, H, 5)
        segs = random_segments(n, 7)
        rec = project_host(cam, W, H, segs)
        base = np.random.default_rng(3).integers(0, 256, (H, W, 3)).astype(np.uint8)
        for bias, hidden in ((ref.DEFAULT_BIAS, 64), (f32(0.0), 255), (f32(0.25), 0)):
            img, ids = draw_host(rec, segs, cam, W, H, ldr=base, rays=rays, t_px=t, depth_bias=bias, hidden_alpha=hidden)
            want_img, want_ids, _ = ref.draw(rec, segs, F, W, H, base, rays, t, bias, hidden)
            assert np.array_equal(ids, want_ids), (which, W, bias, np.argwhere(ids != want_ids)[:4])
            assert np.array_equal(img, want_img), (which, W, bias, np.argwhere(img != want_img)[:4])
        assert (want_ids >= 0).sum() > W * H // 4 and len(np.unique(want_ids)) > n // 8
        assert np.array_equal(base, np.random.default_rng(3).integers(0, 256, (H, W, 3)).astype(np.uint8))      # the input was copied, not drawn over


def wrong_case():
    """one small list on which every deliberately wrong rule shows: an exact tie of the coverage, two overlapping segments, a depth inside the bias, an x-ray pixel"""
    cam = scenes.Camera(eye=(0.0, 0.0, 0.0), dir=(0, 1, 0), up=(0, 0, 1), is_ortho=True, ortho_scale=8.0, aspect=1.0)
    W = H = 16                                                 # one world unit per pixel, exactly: X = x + 8, Y = 8 - z
    px = lambda X, Y, depth: (X - 8.0, depth, 8.0 - Y)
    rows = [(px(2.5, 3.0, 1.0), px(9.5, 3.0, 1.0), (255, 0, 0), 255, 1, ref.ON_TOP),        # on a row boundary, width 1: d = 0.5 = h exactly for two rows
            (px(2.5, 8.5, 1.0), px(9.5, 8.5, 1.0), (0, 255, 0), 255, 3, ref.ON_TOP),        # two overlapping segments of different colours
            (px(5.5, 6.5, 1.0), px(5.5, 12.5, 1.0), (0, 0, 255), 200, 3, ref.ON_TOP),
            (px(2.5, 13.5, 2.001), px(9.5, 13.5, 2.001), (9, 9, 9), 255, 1, ref.HIDE),      # behind t = 2 by less than the bias
            (px(11.5, 2.5, 3.0), px(11.5, 13.5, 3.0), (200, 100, 50), 255, 1, ref.XRAY)]    # clearly behind: x-ray
    t = np.full((H, W), 2.0, f32)
    rays = np.zeros((H * W, 8), f32); rays[:, 5] = 1.0
    return cam, W, H, seg_list(rows), rays, t


def test_the_wrong_case_is_what_it_says(hip_lib):
    project_host, draw_host, frame_host = _api()
    cam, W, H, segs, rays, t = wrong_case()
    rec = project_host(cam, W, H, segs)
    assert np.array_equal(rec["x0"][:2], f32([2.5, 2.5])) and np.array_equal(rec["y0"][:2], f32([3.0, 8.5])) and np.array_equal(rec["q0"], f32([1, 1, 1, 2.001, 3]))
    img, ids = draw_host(rec, segs, cam, W, H, ldr=np.zeros((H, W, 3), np.uint8), rays=rays, t_px=t)
    want_img, want_ids, _ = ref.draw(rec, segs, frame_host(cam, W, H), W, H, None, rays, t)
    assert np.array_equal(ids, want_ids) and np.array_equal(img, want_img)
    assert (ids[2, 2:10] == 0).all() and (ids[3, 2:10] == 0).all() and (ids[1] == -1).all() and (ids[4, :11] == -1).all()      # the tie counts: two rows
    assert (ids[13, 2:10] == 3).all() and (ids[2:14, 11] == 4).all()
    assert tuple(img[5, 11]) == tuple((c * 64 + 128) >> 8 for c in (200, 100, 50))                                           # 255 * 64 + 128 >> 8 = 64


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_each_wrong_rule_changes_an_output(hip_lib, wrong):
    project_host, draw_host, frame_host = _api()
    cam, W, H, segs, rays, t = wrong_case()
    rec = project_host(cam, W, H, segs)
    img, ids = draw_host(rec, segs, cam, W, H, ldr=np.zeros((H, W, 3), np.uint8), rays=rays, t_px=t)
    bad_img, bad_ids, _ = ref.draw(rec, segs, frame_host(cam, W, H), W, H, None, rays, t, wrong=wrong)
    assert not np.array_equal(img, bad_img), wrong
    if wrong != "descending_order":
        assert not np.array_equal(ids, bad_ids), wrong


# ------------------------------------------------------------------------------------------------ CPU 5: the builders
def test_builders_counts_and_end_points():
    from cadrays_amd import annotations as an
    assert an.DTYPE == ref.SEGMENT_DTYPE
    b = an.box((0, 1, 2), (3, 5, 7))
    assert len(b) == 12
    edges = {(tuple(s["a"]), tuple(s["b"])) for s in b}
    assert len(edges) == 12
    corners = {(x, y, z) for x in (0.0, 3.0) for y in (1.0, 5.0) for z in (2.0, 7.0)}
    assert {p for e in edges for p in e} == corners
    assert all(sum(p != q for p, q in zip(a, c)) == 1 for a, c in edges)                     # every edge runs along one axis
    assert all(sum(c in e for e in edges) == 3 for c in corners)                             # closed: three edges meet in every corner
    assert sorted(np.abs(b["b"] - b["a"]).sum(1)) == [3.0] * 4 + [4.0] * 4 + [5.0] * 4
    assert (b["style"] == ref.style(1, ref.XRAY)).all()
    g = an.grid((1, 2, 3), (1, 0, 0), (0, 1, 0), 0.5, 20)
    assert len(g) == 82 and (g["a"][:, 2] == 3).all() and (g["b"][:, 2] == 3).all()
    assert np.array_equal(g["a"][0], f32([-9, -8, 3])) and np.array_equal(g["b"][0], f32([11, -8, 3])) and np.array_equal(g["a"][81], f32([11, -8, 3])) and np.array_equal(g["b"][81], f32([11, 12, 3]))
    a = an.axes((1, 1, 1), 2.0)
    assert len(a) == 3 and np.array_equal(a["b"], f32([[3, 1, 1], [1, 3, 1], [1, 1, 3]])) and np.array_equal(a["rgb"], np.eye(3, dtype=np.uint8) * 255)
    c = an.circle((1, 2, 3), (0, 0, 2), 0.5, 24)
    assert len(c) == 24 and np.array_equal(c["b"][:-1], c["a"][1:]) and np.array_equal(c["b"][-1], c["a"][0])      # closed
    assert np.allclose(np.linalg.norm(c["a"].astype(np.float64) - (1, 2, 3), axis=1), 0.5, atol=1e-6) and (c["a"][:, 2] == 3).all()
    lights = [scenes.Light.positional((0.5, 0.5, 0.85)), scenes.Light.directional((0, 0, 1)), scenes.Light.positional((0, 0, 0))]
    m = an.light_markers(lights, 0.05, n=16)
    assert len(m) == 3 * 16 + 5 + 3 * 16
    assert np.array_equal(m["a"][48], f32([0, 0, 0.2])) and np.array_equal(m["b"][48], f32([0, 0, 0]))             # the arrow: from the light's side to the anchor
    mp = an.manipulator((0.5, 0.5, 0.5), 0.2, n=32)
    assert len(mp) == 15 + 96
    assert [an.manipulator_handle(i, 32) for i in (0, 4, 5, 14, 15, 46, 47, 110, 111)] == ["move_x", "move_x", "move_y", "move_z", "turn_x", "turn_x", "turn_y", "turn_z", None]
    assert np.array_equal(mp["b"][0], f32([0.7, 0.5, 0.5])) and tuple(mp["rgb"][5]) == (0, 255, 0)
    j = an.join(b, a)
    assert len(j) == 15 and np.array_equal(j[:12], b) and len(an.join()) == 0
    s = an.segments((0, 0, 0), (1, 1, 1), rgb=(1, 2, 3), alpha=9, width=8, mode=ref.HIDE)
    assert len(s) == 1 and s["style"][0] == 0x108 and s["alpha"][0] == 9
    assert len(an.polyline([(0, 0, 0), (1, 0, 0), (1, 1, 0)])) == 2 and len(an.polyline([(0, 0, 0), (1, 0, 0), (1, 1, 0)], closed=True)) == 3


# ================================================================================================ GPU
def ortho_cam(W, H):
    return scenes.Camera(eye=(0.5, -1.45, 0.5), dir=(0, 1, 0), up=(0, 0, 1), is_ortho=True, ortho_scale=0.5)


def at_pixel(W, H, X, Y, y_world):
    """the world point that ortho_cam projects to the continuous pixel coordinates (X, Y), at depth y_world - eye.y"""
    return (0.5 + (X / (W / 2) - 1.0) * 0.5 * (W / H), y_world, 0.5 + 0.5 * (1.0 - Y / (H / 2)))


def all_rays(v, W, H):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return v.camera_rays(np.stack([x.ravel(), y.ravel()], 1))


def expected(v, cam, W, H, segs, plain, depth_bias=ref.DEFAULT_BIAS, hidden_alpha=ref.DEFAULT_HIDDEN):
    """(records, image, ids, s) by numpy from the device's own id buffer and camera rays"""
    _, _, frame_host = _api()
    F = frame_host(cam, W, H)
    rec = ref.project(F, W, H, segs)
    return (rec,) + ref.draw(rec, segs, F, W, H, plain, all_rays(v, W, H), v.read_ids()[2], depth_bias, hidden_alpha)


def assert_all_agree(v, cam, W, H, segs, plain, depth_bias=ref.DEFAULT_BIAS, hidden_alpha=ref.DEFAULT_HIDDEN):
    """the list is in force: records, id plane and LDR bytes of the device == the twins == numpy; returns (image, ids, s)"""
    project_host, draw_host, _ = _api()
    rec, img, ids, s = expected(v, cam, W, H, segs, plain, depth_bias, hidden_alpha)
    got_rec = v.ReadAnnotationRecords()
    assert same_records(got_rec, project_host(cam, W, H, segs)) and same_records(got_rec, rec)
    t_img, t_ids = draw_host(rec, segs, cam, W, H, ldr=plain, rays=all_rays(v, W, H), t_px=v.read_ids()[2], depth_bias=depth_bias, hidden_alpha=hidden_alpha)
    got_ids = v.ReadAnnotationIds()
    assert np.array_equal(got_ids, t_ids) and np.array_equal(got_ids, ids), np.argwhere(got_ids != ids)[:4]
    got = v.read_ldr()
    assert np.array_equal(got, t_img) and np.array_equal(got, img), np.argwhere(got != img)[:4]
    return img, ids, s


def room(W, H, cam=None, frames=2):
    from cadrays_amd.view import View
    sc = object_scene(None, W, H)
    if cam is not None:
        sc = dataclasses.replace(sc, camera=cam)
    v = View(0).load_scene(sc)
    for _ in range(frames): v.Redraw()
    return sc, v


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_known_answers_under_an_orthographic_camera(hip_lib, W, H):
    cam = ortho_cam(W, H)
    sc, v = room(W, H, cam)
    plain = v.read_ldr()
    r, x0, x1 = 5, W // 2 - 5, W // 2 + 5                      # near the ceiling: nothing stands between the camera and the back wall (y = 1) there
    P = lambda X, Y, y=0.9: at_pixel(W, H, X, Y, y)
    white = lambda a, b, width, mode=ref.ON_TOP, alpha=255: seg_list([(a, b, (255, 255, 255), alpha, width, mode)])
    def ids_of(segs, **kw):
        v.SetAnnotations(segs, **kw)
        return v.ReadAnnotationIds()
    def block(rows, cols):
        m = np.zeros((H, W), bool); m[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = True
        return m
    # width 1 through the pixel centres of row r: exactly that row's span
    assert np.array_equal(ids_of(white(P(x0 + 0.5, r + 0.5), P(x1 + 0.5, r + 0.5), 1)) == 0, block((r, r), (x0, x1)))
    # width 2 along the boundary between rows r - 1 and r, from pixel boundary to pixel boundary: both rows, and the round caps reach one pixel further (0.5 + 0.5 <= 1)
    assert np.array_equal(ids_of(white(P(x0, r), P(x1, r), 2)) == 0, block((r - 1, r), (x0 - 1, x1)))
    # width 3 through the centres: three rows, the caps one pixel further (1 + 1 <= 2.25)
    assert np.array_equal(ids_of(white(P(x0 + 0.5, r + 0.5), P(x1 + 0.5, r + 0.5), 3)) == 0, block((r - 1, r + 1), (x0 - 1, x1 + 1)))
    # a point marker: one pixel at width 1, 3 x 3 at width 3
    for width, reach in ((1, 0), (3, 1)):
        assert np.array_equal(ids_of(white(P(30.5, 20.5), P(30.5, 20.5), width)) == 0, block((20 - reach, 20 + reach), (30 - reach, 30 + reach)))
    # in front of the back wall: fully visible in every mode; behind it: absent (HIDE), hidden_alpha-blended (XRAY), drawn (ON_TOP)
    assert (np.abs(v.read_ids()[2][r, x0:x1 + 1].astype(np.float64) - 2.45) < 1e-4).all()      # (the scene, not the feature: the wall is where the case needs it)
    span = block((r, r), (x0, x1))
    full = lambda alpha: np.where(span[..., None], ((plain.astype(np.uint32) * (256 - alpha) + 255 * alpha + 128) >> 8).astype(np.uint8), plain)
    for mode in (ref.ON_TOP, ref.HIDE, ref.XRAY):
        assert np.array_equal(ids_of(white(P(x0 + 0.5, r + 0.5, 0.9), P(x1 + 0.5, r + 0.5, 0.9), 1, mode, 200)) == 0, span)
        assert np.array_equal(v.read_ldr(), full(200))
    behind = lambda mode: white(P(x0 + 0.5, r + 0.5, 1.1), P(x1 + 0.5, r + 0.5, 1.1), 1, mode, 200)
    assert (ids_of(behind(ref.HIDE)) == -1).all() and np.array_equal(v.read_ldr(), plain)
    assert np.array_equal(ids_of(behind(ref.XRAY), hidden_alpha=100) == 0, span) and np.array_equal(v.read_ldr(), full((200 * 100 + 128) >> 8))
    assert np.array_equal(ids_of(behind(ref.ON_TOP)) == 0, span) and np.array_equal(v.read_ldr(), full(200))
    # piercing the wall: y from 0.5 to 1.5 along the row, the wall at y = 1 is met halfway; visible while depth <= 2.45 (1 + 2^-9)
    ids = ids_of(white(P(x0 + 0.5, r + 0.5, 0.5), P(x1 + 0.5, r + 0.5, 1.5), 1, ref.HIDE))
    depth = 1.95 + (np.arange(x0, x1 + 1) - x0) / (x1 - x0)
    assert np.abs(depth - 2.45 * (1 + 2.0 ** -9)).min() > 1e-3
    want = np.zeros((H, W), bool); want[r, x0:x1 + 1] = depth <= 2.45 * (1 + 2.0 ** -9)
    assert np.array_equal(ids == 0, want) and want.sum() == 6 and want[r, x0] and not want[r, x1]
    s = np.array([v.PickAnnotation(x, r)[1] for x in range(x0, x0 + 6)])
    assert 0.0 <= s[0] < 0.01 and (np.diff(s) > 0.09).all() and 0.49 < s[5] < 0.51 and v.PickAnnotation(x1, r) == (-1, 0.0)
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 100, 2000])
def test_device_equals_twin_and_numpy_over_list_sizes(hip_lib, W, H, n):
    """more than one bitmask word from n = 33 on; 67 x 45 and 130 x 70 leave partial tiles at every tile edge; up to 256 segments the bins are gathered, 2000 are scattered"""
    sc, v = room(W, H)
    plain = v.read_ldr()
    segs = random_segments(n, 100 + n)
    v.SetAnnotations(segs)
    img, ids, _ = assert_all_agree(v, sc.camera, W, H, segs, plain)
    if n >= 100:
        modes = (segs["style"] >> 8) & 3
        assert all((modes[np.unique(ids[ids >= 0])] == m).any() for m in (0, 1, 2)) and not np.array_equal(img, plain)
    v.ClearAnnotations()
    assert np.array_equal(v.read_ldr(), plain) and (v.ReadAnnotationIds() == -1).all()
    v.close()


VIEWS = {"perspective": scenes.Camera(eye=(0.5, -1.45, 0.5)), "orthographic": scenes.Camera(eye=(0.5, -1.45, 0.5), is_ortho=True, ortho_scale=0.5),
         "inside": scenes.Camera(eye=(0.5, 0.5, 0.5), dir=(0.3, 1.0, -0.2), fovy_deg=80.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(VIEWS))
def test_device_equals_twin_and_numpy_over_cameras_and_parameters(hip_lib, which):
    W, H = 67, 45
    cam = VIEWS[which]
    sc, v = room(W, H, cam)
    plain = v.read_ldr()
    segs = random_segments(100, 9, 0.05, 0.95) if which == "inside" else random_segments(100, 9)
    for bias, hidden in ((ref.DEFAULT_BIAS, 64), (f32(0.0), 255), (f32(0.5), 0)):
        v.SetAnnotations(segs, depth_bias=bias, hidden_alpha=hidden)
        g = v.GetAnnotations()
        assert g["on"] and g["depth_bias"] == bias and g["hidden_alpha"] == hidden and np.array_equal(g["segments"], segs)
        _, ids, _ = assert_all_agree(v, cam, W, H, segs, plain, bias, hidden)
    assert (ids >= 0).sum() > 200
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile,form", [("8", "gather"), ("32", "gather"), ("16", "scatter"), ("8", "scatter"), ("32", "by length")])
def test_no_result_depends_on_the_tile_edge_or_the_binning_form(hip_lib, monkeypatch, tile, form):
    hip_lib.crh_env_table.restype = C.c_char_p
    assert b"CRH_ANNOT_TILE\t" in hip_lib.crh_env_table() and b"CRH_ANNOT_BIN\t" in hip_lib.crh_env_table()
    monkeypatch.setenv("CRH_ANNOT_TILE", tile); monkeypatch.setenv("CRH_ANNOT_BIN", form)      # read when the context is created
    W, H = 130, 70
    sc, v = room(W, H)
    plain = v.read_ldr()
    segs = random_segments(300, 11)
    v.SetAnnotations(segs)
    assert_all_agree(v, sc.camera, W, H, segs, plain)
    v.close()


@pytest.mark.gpu
def test_annotations_follow_the_states_of_a_live_scene(hip_lib):
    """a moved object, an erased object, an added object (the states of test_outline's live scene): the occlusion follows the id buffer of the state in force"""
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    v, w = View(0).load_scene(sc), View(0).load_scene(sc)      # w: the same calls, never an annotation -- the bytes underneath
    # behind the yellow box where the scene is built; inside the box where it is moved to; behind the roof that is added -- drawn last, so they show in the id plane
    placed = seg_list([((0.6, 0.7, 0.1), (0.9, 0.7, 0.1), (255, 0, 0), 255, 2, ref.HIDE), ((0.25, 0.69, 0.05), (0.32, 0.69, 0.05), (0, 255, 0), 255, 2, ref.HIDE),
                       ((0.45, 0.5, 0.5), (0.55, 0.5, 0.5), (0, 0, 255), 255, 2, ref.HIDE)])
    segs = np.concatenate([random_segments(100, 21), placed])
    v.SetAnnotations(segs)
    seen = []
    def step(change):
        for x in (v, w):
            change(x)
            for _ in range(2): x.Redraw()
        seen.append(assert_all_agree(v, sc.camera, W, H, segs, w.read_ldr())[1])
    step(lambda x: None)
    step(lambda x: x.set_transforms(moved_xforms(7)))
    assert v.get_tlas()["n_instances"] >= 1
    step(lambda x: x.set_visibility(visible_flags(7, [3])))
    p = np.array([(0.35, 0.25, 0.35), (0.5, 0.1, 0.35), (0.5, 0.1, 0.65), (0.35, 0.25, 0.65), (0.65, 0.25, 0.35), (0.65, 0.25, 0.65)], f32)
    n = np.tile(np.array([0, -1, 0], f32), (6, 1)); t = np.array([(0, 1, 2, 0), (0, 2, 3, 0), (1, 4, 5, 0), (1, 5, 2, 0)], np.int32)
    step(lambda x: x.add_object(p, n, t, rigid()))
    shown = [[int((ids == 100 + k).sum()) for k in range(3)] for ids in seen]
    assert shown[1][0] > shown[0][0] and shown[1][1] == 0 < shown[2][1] and shown[2][2] > 0 == shown[3][2], shown
    v.close(); w.close()


@pytest.mark.gpu
def test_read_out_paths(hip_lib):
    from cadrays_amd.view import view_host
    W, H = 130, 70
    sc, v = room(W, H)
    plain = v.read_ldr()
    segs = random_segments(100, 31)
    v.SetAnnotations(segs)
    img, ids, s = assert_all_agree(v, sc.camera, W, H, segs, plain)
    for got in both_slots(v):                                  # synchronous == asynchronous, both read-back slots
        assert np.array_equal(got, img)
    v.read_ldr_begin(); v.read_ldr_begin()                     # ... and two in flight
    assert np.array_equal(v.read_ldr_end(), img) and np.array_equal(v.read_ldr_end(), img)
    for vw, vh in ((61, 33), (200, 90)):
        assert np.array_equal(v.read_view(vw, vh), view_host(img, vw, vh))
        v.read_view_begin(vw, vh)
        assert np.array_equal(v.read_view_end(), view_host(img, vw, vh))
    for y, x in [(0, 0), (H - 1, W - 1)] + [tuple(p) for p in np.argwhere(ids >= 0)[::97]] + [tuple(p) for p in np.argwhere(ids < 0)[::977]]:
        seg, par = v.PickAnnotation(int(x), int(y))
        assert seg == ids[y, x] and par.view(np.uint32) == (s[y, x] if seg >= 0 else f32(0)).view(np.uint32), (x, y)
    with pytest.raises(BackendError):
        v.PickAnnotation(W, 0)
    # selection and hover lie UNDER the annotations: a handle keeps its own colour over a tinted selection
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    v.ClearAnnotations(); v.set_selection(flags, (255, 0, 0), 128); v.set_hover(4, (0, 255, 0), 64); v.SetOutline(width=2)
    under = v.read_ldr()
    assert not np.array_equal(under, plain)
    v.SetAnnotations(segs)
    assert np.array_equal(v.read_ldr(), expected(v, sc.camera, W, H, segs, under)[1])
    b = v.BenchAnnotations(2)
    assert all(b[k] > 0 for k in ("project_ms", "bin_ms", "draw_ms")) and np.array_equal(v.read_ldr(), expected(v, sc.camera, W, H, segs, under)[1])
    v.close()


@pytest.mark.gpu
def test_derived_state_is_never_stale(hip_lib):
    """after crh_set_camera, crh_set_params (size), crh_set_transforms and a new list the NEXT read-out -- synchronous or asynchronous -- matches numpy for the new state"""
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    v, w = View(0).load_scene(sc), View(0).load_scene(sc)
    segs = random_segments(100, 41)
    v.SetAnnotations(segs)
    state = dict(cam=sc.camera, W=W, H=H, segs=segs)
    def check(change=None, **new):
        state.update(new)
        for x in (v, w):
            if change: change(x)
            x.Redraw()
        want = expected(v, state["cam"], state["W"], state["H"], state["segs"], w.read_ldr())
        v.read_ldr_begin()                                     # the asynchronous read-out first: its own records and bins
        assert np.array_equal(v.read_ldr_end(), want[1])
        assert np.array_equal(v.read_ldr(), want[1]) and np.array_equal(v.ReadAnnotationIds(), want[2]) and same_records(v.ReadAnnotationRecords(), want[0])
        return want[2]
    a = check()
    cam2 = dataclasses.replace(sc.camera, eye=(0.2, -1.3, 0.6), dir=(0.1, 1.0, -0.05))
    b = check(lambda x: x.set_camera(cam2), cam=cam2)
    c = check(lambda x: x.set_params(dataclasses.replace(sc.params, width=130, height=70)), W=130, H=70)
    d = check(lambda x: x.set_transforms(moved_xforms(7)))
    segs2 = random_segments(33, 42)
    v.SetAnnotations(segs2)
    e = check(segs=segs2)
    assert not np.array_equal(a, b) and c.shape == (70, 130) and not np.array_equal(c, d) and 0 <= e.max() <= 32
    v.close(); w.close()


@pytest.mark.gpu
def test_the_annotations_leave_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 67, 45
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    w = View(0).load_scene(sc)
    for _ in range(6): w.Redraw()
    # the list set before the scene exists, read-outs and queries between the frames
    v = View(0)
    segs = random_segments(200, 51)
    v.SetAnnotations(segs)
    v.load_scene(sc)
    for k in range(6):
        v.Redraw()
        if k in (1, 4):
            v.read_ldr(); v.read_ldr_begin(); v.ReadAnnotationIds(); v.PickAnnotation(3, 3); v.read_ldr_end(); v.ReadAnnotationRecords()
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    assert same(v.read_hdr(), w.read_hdr())
    (acc, frames), (want_acc, want_frames) = v.save_accum(), w.save_accum()
    assert same(acc, want_acc) and frames == want_frames == 6
    st, want_st = v.stats(), w.stats()
    assert all(st[k] == want_st[k] for k in counters), (st, want_st)
    assert all(np.array_equal(a, b) for a, b in zip(v.read_ids(), w.read_ids()))
    assert np.array_equal(v.read_outline(), w.read_outline()) and same(v.read_denoised(), w.read_denoised())
    assert not np.array_equal(v.read_ldr(), w.read_ldr())
    v.ClearAnnotations()
    assert np.array_equal(v.read_ldr(), w.read_ldr()) and not v.GetAnnotations()["on"] and len(v.GetAnnotations()["segments"]) == 0
    v.close(); w.close()


@pytest.mark.gpu
def test_set_annotations_refusals_and_state(hip_lib):
    from cadrays_amd.view import View
    from cadrays_amd import annotations as an
    W, H = 67, 45
    v = View(0)
    g = v.GetAnnotations()
    assert not g["on"] and g["depth_bias"] == ref.DEFAULT_BIAS and g["hidden_alpha"] == 64 and len(g["segments"]) == 0
    good = random_segments(5, 61)
    v.SetAnnotations(good)                                     # before crh_build
    for why, bad in bad_lists():
        with pytest.raises(BackendError, match="crh_set_annotations: segment"):
            v.SetAnnotations(bad)
    for kw, msg in ((dict(depth_bias=-1.0e-3), "negative"), (dict(depth_bias=np.nan), "NaN"), (dict(depth_bias=np.inf), "NaN"), (dict(hidden_alpha=256), "hidden_alpha")):
        with pytest.raises(BackendError, match=msg):
            v.SetAnnotations(good, **kw)
    too_many = np.zeros(abi.ANNOT_MAX_SEGMENTS + 1, ref.SEGMENT_DTYPE); too_many["style"] = 1
    with pytest.raises(BackendError, match="65536"):
        v.SetAnnotations(too_many)
    assert np.array_equal(v.GetAnnotations()["segments"], good) and v.GetAnnotations()["on"]      # a refused call leaves the list in force
    with pytest.raises(BackendError):                          # no scene yet
        v.ReadAnnotationIds()
    sc = object_scene(None, W, H)
    v.load_scene(sc); v.Redraw()
    v.SetAnnotations(too_many[:-1])                            # 65536 is allowed
    assert len(v.ReadAnnotationRecords()) == abi.ANNOT_MAX_SEGMENTS
    # the selection's box
    v.ClearAnnotations(); plain = v.read_ldr()
    v._selected = {3}; v._push_selection()
    lo, hi = v.selection_bounds()
    sg = v.ShowSelectionBox(extra=an.axes((0.5, 0.5, 0.0), 0.2))
    assert len(sg) == 15 and np.array_equal(sg[:12], an.box(lo, hi)) and np.array_equal(v.GetAnnotations()["segments"], sg)
    ids = v.ReadAnnotationIds()
    assert set(np.unique(ids)) >= set(range(12)) | {-1}        # every edge of the box shows: hidden edges as x-ray
    v._selected = set(); v._push_selection()
    assert len(v.ShowSelectionBox()) == 0 and not v.GetAnnotations()["on"] and np.array_equal(v.read_ldr(), plain)
    v.close()
