"""The rules the library keeps ONE copy of: the display chain both LDR read-outs enqueue, the geometry generation behind the three derived
tables, the camera frame.

  CPU   the shape of the sources: one call site of launch_tonemap, one displayed-image expression, one camera-frame expression, no per-table dirty flags;
        the camera frames crh_reproject_frame_host and crh_fit_extents_host hand out agree to the bit over a sweep of cameras
  GPU   at 67 x 45 (more than one 64-pixel chunk per row, partial 8 x 8 blocks, partial tiles) on the two-level Cornell room: the synchronous and the asynchronous
        read-out give the same bytes with every display feature on, and after each is switched off; every geometry change reaches the triangle-to-object table of the
        id buffer, the vertex array of the view fit and the per-triangle table of the feature lines
"""
import dataclasses
import glob
import itertools
import os

import numpy as np
import pytest

from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_reproject import move, turned
from test_two_level import object_scene, rigid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 67, 45


# ================================================================================================ CPU
def test_each_shared_rule_is_written_once():
    """Over csrc/crh_*.cpp and crh_context.h: the tone map has one call site (the display chain), the displayed-image expression and the half-angle of the camera
    frame occur once, and the three hand-set flags of the derived tables are gone (the geometry generation took their place)."""
    csrc = os.path.join(ROOT, "cadrays_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "crh_*.cpp"))) + [os.path.join(csrc, "crh_context.h")]
    assert len(files) >= 13, files
    text = {os.path.basename(f): open(f).read() for f in files}
    where = lambda needle: {name: t.count(needle) for name, t in text.items() if needle in t}
    assert where("launch_tonemap(") == {"crh_readback.cpp": 1}
    assert where("assembled_valid ?") == {"crh_context.h": 1}
    assert where("fovy_deg * 0.5f") == {"crh_context.h": 1}
    for flag in ("pk_tri_obj_dirty", "fit_verts_dirty", "ol_table_dirty"):
        assert where(flag) == {}, flag


def camera_sweep():
    dirs = ((0.0, 1.0, 0.0), (0.0, 7.5, 0.0), (0.3, 1.0, -0.2), (-12.0, 3.0, 5.0))                  # unit, unnormalised, oblique
    ups = ((0.0, 0.0, 1.0), (0.2, 0.4, 0.9))                                                        # orthogonal to the first two directions, orthogonal to none
    fovs = (1.0, 20.0, 45.0, 90.0, 135.0, 170.0)
    for ortho, aspect, d, u, fov in itertools.product((False, True), (1.37, 0.0), dirs, ups, fovs):
        yield scenes.Camera(eye=(0.25, -3.0, 0.5), dir=d, up=u, fovy_deg=fov, aspect=aspect, is_ortho=ortho, ortho_scale=1.5)


def test_camera_frames_of_the_fit_and_of_the_reprojection_agree_to_the_bit(hip_lib):
    """crh_reproject_frame_host and crh_fit_extents_host derive right / up / fwd, tan_half and aspect from a crh_camera by the same expressions as the kernels' scene
    record.  This test also passes on the commit BEFORE the camera frame got its one copy (crh_context.h camera_frame): it is the pin that refactor was made under."""
    from cadrays_amd.view import fit_extents_host, reproject_frame_host
    bits = lambda a: np.asarray(a, f32).view(np.uint32)
    n = 0
    for cam in camera_sweep():
        F = reproject_frame_host(cam, W, H)
        _, _, G = fit_extents_host(np.zeros((0, 4), f32), 1, cam, W, H, margin=0.0)
        for k in ("right", "up", "fwd"):
            assert np.array_equal(bits(F[k]), bits(G[k])), (cam, k, F[k], G[k])
        assert np.isfinite(F["tan_half"]) and F["tan_half"] > 0
        assert bits(F["aspect"]) == bits(f32(cam.aspect) if cam.aspect > 0 else f32(W) / f32(H)), cam
        if cam.is_ortho:
            assert G["kx"] == 0 and G["ky"] == 0, cam
        else:
            assert bits(G["ky"]) == bits(F["tan_half"]), (cam, G["ky"], F["tan_half"])
            assert bits(G["kx"]) == bits(f32(np.float64(F["tan_half"]) * np.float64(F["aspect"]))), (cam, G["kx"])
        n += 1
    assert n >= 64


# ================================================================================================ GPU
def both_slots(v):
    """the asynchronous read-out, twice: the two read-back slots in turn"""
    out = []
    for _ in range(2):
        v.read_ldr_begin()
        out.append(v.read_ldr_end())
    return out


@pytest.mark.gpu
def test_synchronous_and_asynchronous_read_outs_agree_with_every_display_feature_on(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    v.set_auto_exposure(True); v.SetReproject(); v.SetDenoise(); v.SetOutline(kinds=abi.OUTLINE_ALL)
    sel = np.zeros(7, np.uint8); sel[[3, 5]] = 1
    v.set_selection(sel); v.set_hover(4)
    v.Redraw(); v.Redraw()
    move(v, turned(sc.camera, 0.7))
    v.Redraw()
    assert v.get_reproject()["history_valid"]                 # the reprojection really runs in the chain
    full = v.read_ldr()
    for got in both_slots(v):
        assert np.array_equal(got, full)
    switches = (("auto exposure", lambda: v.set_auto_exposure(False)), ("reproject", v.ClearReproject), ("denoise", v.ClearDenoise), ("outline", v.ClearOutline),
                ("selection", lambda: v.set_selection(None)), ("hover", lambda: v.set_hover(-1)))
    for name, off in switches:
        off()
        sync = v.read_ldr()
        for got in both_slots(v):
            assert np.array_equal(got, sync), name
    assert not np.array_equal(full, sync)                     # `sync` now: the bytes of the same state with all five display features off
    v.close()


def quad(x0, z0, y, side=0.2):
    """a square facing the camera of the Cornell room, in front of everything: (pos, nrm, tri) with material 0"""
    p = np.array([(x0, y, z0), (x0 + side, y, z0), (x0 + side, y, z0 + side), (x0, y, z0 + side)], f32)
    return p, np.tile(np.array([0, -1, 0], f32), (4, 1)), np.array([(0, 1, 2, 0), (0, 2, 3, 0)], np.int32)


def appended(pos, nrm, tri, tri_object, part, ob):
    p, n, t = part
    return (np.concatenate([pos, p]), np.concatenate([nrm, n]), np.concatenate([tri, t + np.array([len(pos)] * 3 + [0], np.int32)]),
            np.concatenate([tri_object, np.full(len(t), ob, np.int32)]))


def assert_every_derived_table_knows(v, new, n_objects, pos, tri):
    """the three consumers, each the FIRST call that needs its table after the change"""
    from cadrays_amd.view import outline_mask_host, outline_table_host
    picked = {(x, y): v.pick(x, y)["object"] for y in range(0, H, 3) for x in range(0, W, 3)}         # the triangle-to-object table of the id buffer
    assert new in picked.values(), sorted(set(picked.values()))
    one = np.zeros(n_objects, np.uint8); one[new] = 1
    with pytest.raises(BackendError):
        v.fit_view(n_objects - 1, None)                                                                # the flags take one more entry now
    _, r = v.fit_view(n_objects, one, want_extents=True)                                               # the vertex array of the view fit
    assert r["object_extents"].shape == (n_objects, 6) and np.isfinite(r["object_extents"]).all() and r["n_vertices"] == 4
    ob, tr, t = v.read_ids()
    assert all(ob[y, x] == o for (x, y), o in picked.items())
    mask = v.read_outline()                                                                            # the per-triangle table of the feature lines
    assert np.array_equal(mask, outline_mask_host(ob, tr, t, outline_table_host(pos, tri)))
    assert (mask[ob == new] & abi.OUTLINE_OBJECT).any()


@pytest.mark.gpu
def test_every_geometry_change_reaches_every_derived_table(hip_lib):
    """crh_add_object, then crh_set_geometry + crh_build: pick, fit_view and read_outline all see the geometry now in force.  Passes before and after the three dirty
    flags became one generation."""
    from cadrays_amd.view import View, outline_mask_host, outline_table_host
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    assert v.pick(W // 2, H // 2)["object"] >= 0                   # every consumer has built its table of the first geometry
    _, r = v.fit_view(7, None, want_extents=True)
    assert r["object_extents"].shape == (7, 6)
    assert np.array_equal(v.read_outline(), outline_mask_host(*v.read_ids(), outline_table_host(sc.pos, sc.tri)))
    first = quad(0.3, 0.3, 0.2)
    assert v.add_object(*first, rigid()) == 7
    pos, nrm, tri, tob = appended(sc.pos, sc.nrm, sc.tri, sc.tri_object, first, 7)
    assert_every_derived_table_knows(v, 7, 8, pos, tri)
    pos, nrm, tri, tob = appended(pos, nrm, tri, tob, quad(0.55, 0.55, 0.15), 8)                      # a different scene: one more object again
    v.set_geometry(pos, nrm, tri, None, tob, np.tile(rigid(), (9, 1)))
    v.build()
    assert_every_derived_table_knows(v, 8, 9, pos, tri)
    v.close()
