"""Hover / selection overlay of the LDR read-out (k_overlay, cadrays_amd/csrc/k_ids.h) against a numpy restatement of its integer rule.

Reference: the selected and the detected (hovered) objects of AIS_InteractiveContext are drawn highlighted (Select / ShiftSelect src/Launcher/AppViewer.cxx:359-455,
MoveTo :347).  Rule (include/cadrays_hip.h): a pixel is MARKED for a set when its object is in the set; a marked pixel on the image border, or with a 4-neighbour
that is not marked for the same set, takes the set's colour; every other marked pixel becomes (ldr * (256 - a) + colour * a + 128) >> 8 per channel; the selection
first, the hovered object second; after tone map and after the ShowSamplingTiles outline.
"""
import dataclasses

import numpy as np
import pytest

from cadrays_amd import scenes
from test_two_level import object_scene, rigid


def overlay_set(ldr, marked, rgb, alpha):
    """one set of the rule, integer arithmetic only"""
    H, W = marked.shape
    inner = np.zeros_like(marked)
    inner[1:-1, 1:-1] = marked[1:-1, 1:-1] & marked[:-2, 1:-1] & marked[2:, 1:-1] & marked[1:-1, :-2] & marked[1:-1, 2:]
    outline = marked & ~inner                                     # the border rows and columns are never `inner`
    out = ldr.astype(np.uint32)
    col = np.asarray(rgb, np.uint32)
    blend = (out * (256 - alpha) + col * alpha + 128) >> 8
    out[inner] = blend[inner]
    out[outline] = col
    return out.astype(np.uint8)


def restated(ldr, obj, flags, sel_rgb, sel_a, hover, hov_rgb, hov_a):
    out = ldr
    if flags is not None and np.any(flags):
        out = overlay_set(out, (obj >= 0) & (np.asarray(flags, bool)[np.maximum(obj, 0)]), sel_rgb, sel_a)
    if hover >= 0:
        out = overlay_set(out, obj == hover, hov_rgb, hov_a)
    return out


def flags_of(n, chosen):
    f = np.zeros(n, np.uint8); f[list(chosen)] = 1
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(96, 96), (61, 37), (131, 75)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_overlay_equals_the_restated_rule(hip_lib, size):
    from cadrays_amd.view import View
    W, H = size
    sc = object_scene(None, W, H)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, eye=(0.5, -0.7, 0.5)))      # close enough for walls, floor and a box to leave the image
    v = View(0).load_scene(sc)
    for _ in range(3): v.Redraw()
    plain = v.read_ldr()
    obj = v.read_ids()[0]
    on_border = set(np.unique(np.concatenate([obj[0], obj[-1], obj[:, 0], obj[:, -1]]))) - {-1}
    assert {0, 3} <= on_border                                    # a wall and the short box touch the image border
    wall = 0
    cases = [
        (flags_of(7, [3]), (255, 160, 0), 0, -1, (0, 0, 0), 0),               # outline only; the box touches the border
        (flags_of(7, [3, 5]), (255, 160, 0), 128, -1, (0, 0, 0), 0),
        (flags_of(7, [4]), (10, 200, 30), 255, 6, (0, 255, 255), 128),        # a full tint; hover on another object
        (flags_of(7, [wall]), (200, 0, 200), 128, -1, (0, 0, 0), 0),          # an object that touches the image border
        (flags_of(7, [3, 4]), (255, 0, 0), 64, 3, (0, 0, 255), 128),          # hover on a selected object: hover wins where both apply
        (None, (0, 0, 0), 0, 5, (0, 255, 255), 255),                          # hover alone
        (flags_of(7, range(7)), (255, 255, 255), 128, wall, (1, 2, 3), 0),    # everything selected
    ]
    for flags, srgb, sa, hov, hrgb, ha in cases:
        v.set_selection(flags, srgb, sa); v.set_hover(hov, hrgb, ha)
        got = v.read_ldr()
        want = restated(plain, obj, flags, srgb, sa, hov, hrgb, ha)
        assert np.array_equal(got, want), (size, srgb, sa, hov, int((got != want).any(-1).sum()))
        assert not np.array_equal(got, plain)
        v.read_ldr_begin()                                        # the asynchronous read-out draws the same
        assert np.array_equal(v.read_ldr_end(), want)
    # the HDR read-outs and the checkpoint never see it
    hdr = v.read_hdr(); acc = v.save_accum()[0]
    v.set_selection(None); v.set_hover(-1)
    assert np.array_equal(v.read_ldr(), plain)
    assert np.array_equal(v.read_hdr().view(np.uint32), hdr.view(np.uint32)) and np.array_equal(v.save_accum()[0].view(np.uint32), acc.view(np.uint32))
    v.close()


@pytest.mark.gpu
def test_a_selected_object_partly_hidden_by_an_unselected_one(hip_lib):
    """the outline follows what is VISIBLE of the object: where another object covers it, the boundary between the two is outlined"""
    from cadrays_amd.view import View
    sc = object_scene(None, 128, 96)
    v = View(0).load_scene(sc)
    # the tall box (object 4) pushed in front of the short one (object 3), towards the camera
    xf = np.tile(rigid(), (7, 1)); xf[4] = rigid(0.0, (0, 0, 1), (0.0, -0.3, 0.0))
    v.set_transforms(xf)
    for _ in range(2): v.Redraw()
    plain, obj = v.read_ldr(), v.read_ids()[0]
    m3, m4 = obj == 3, obj == 4
    touching = (m3[:, 1:] & m4[:, :-1]) | (m3[:, :-1] & m4[:, 1:])
    assert m3.sum() > 20 and touching.sum() > 3                   # object 4 covers a part of object 3: they share a boundary on screen
    v.set_selection(flags_of(7, [3]), (255, 255, 0), 0)
    got = v.read_ldr()
    assert np.array_equal(got, restated(plain, obj, flags_of(7, [3]), (255, 255, 0), 0, -1, (0, 0, 0), 0))
    changed = (got != plain).any(-1)
    assert changed.any() and not (changed & ~m3).any()            # alpha 0: only outline pixels of object 3 change, nothing of the covering object
    v.close()


@pytest.mark.gpu
def test_overlay_is_drawn_after_the_sampling_tile_outline(hip_lib):
    """ShowSamplingTiles and a selection at once: tone map, red tile outlines, THEN hover / selection"""
    from cadrays_amd.view import View
    sc = object_scene(None, 128, 96)
    v = View(0).load_scene(sc)
    v.set_adaptive(True, 4); v.set_show_tiles(True)
    for _ in range(3): v.Redraw()
    with_tiles = v.read_ldr()
    v.set_show_tiles(False)
    assert not np.array_equal(v.read_ldr(), with_tiles)           # the tile outlines are there
    v.set_show_tiles(True)
    obj = v.read_ids()[0]
    flags = flags_of(7, range(7))
    v.set_selection(flags, (0, 255, 0), 128); v.set_hover(3, (0, 0, 255), 255)
    got = v.read_ldr()
    assert np.array_equal(got, restated(with_tiles, obj, flags, (0, 255, 0), 128, 3, (0, 0, 255), 255))
    red = (with_tiles == (255, 0, 0)).all(-1) & (obj >= 0)
    assert red.any() and not (got[red] == (255, 0, 0)).all(-1).any()      # the selection lies over the red outlines, not under them
    v.close()


@pytest.mark.gpu
def test_a_scene_without_objects_is_one_object(hip_lib):
    from cadrays_amd.view import View
    v = View(0).load_scene(scenes.cornell_box(True, 64, 48))
    v.Redraw()
    plain, obj = v.read_ldr(), v.read_ids()[0]
    assert set(np.unique(obj)) <= {-1, 0}
    v.set_selection([1], (255, 0, 255), 64)
    assert np.array_equal(v.read_ldr(), restated(plain, obj, [1], (255, 0, 255), 64, -1, (0, 0, 0), 0))
    v.close()
