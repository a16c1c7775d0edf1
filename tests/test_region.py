"""Region queries on the first-hit id buffer: rectangle and lasso selection, visible objects (crh_region.cpp, cadrays_amd/csrc/region_kernels.hip).

Reference: the application selects one object per click (src/Launcher/AppViewer.cxx:347-457); rubber-band and lasso selection are OCCT's
AIS_InteractiveContext::Select(xmin, ymin, xmax, ymax, view) and its polyline form.  Here they are one reduction over the id buffer, in integers and extrema.

  CPU   the struct's layout; crh_region_stats_host == the numpy restatement (tests/region_reference.py, written from the header's text), struct bytes equal; the
        polygon rule's properties, checked without the restatement's bookkeeping; crh_region_select's truth table; every refusal
  GPU   crh_query_region == numpy over the planes crh_read_ids returns == the host twin, struct bytes equal: through the states of a live scene, many small objects,
        one object filling a frame large enough for a second round of the kernel's loop, an all-miss frame; nothing else moves; the View vocabulary; errors
The id buffer itself is held to the checker and to a float64 brute force by tests/test_pick.py.
"""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import region_reference as ref
from cadrays_amd import abi, scenes
from cadrays_amd.binding import BackendError
from test_two_level import moved_xforms, object_scene, rigid
from test_visibility import one_object, visible_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [(1, 1), (5, 3), (64, 2), (61, 37), (130, 67)]


def _api():
    """the three entry points through the Python mirror: a missing one FAILS here (AttributeError / ImportError), it does not skip"""
    from cadrays_amd.view import region_select, region_stats_host
    return region_stats_host, region_select


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(a, b):
    return [(int(i), a[i], b[i]) for i in np.flatnonzero(np.frombuffer(a.tobytes(), "V32") != np.frombuffer(b.tobytes(), "V32"))[:4]]


def planes(W, H, n_objects, seed):
    """random ids with -1 entries; t random positive with 0.0 and a denormal among the hits, 1e15 at the misses"""
    r = np.random.default_rng(seed)
    ob = r.integers(0, n_objects, (H, W)).astype(np.int32)
    ob[r.random((H, W)) < 0.2] = -1
    t = r.uniform(0.01, 50.0, (H, W)).astype(f32)
    hits = np.argwhere(ob >= 0)
    if len(hits) > 0: t[tuple(hits[0])] = 0.0
    if len(hits) > 1: t[tuple(hits[-1])] = np.frombuffer(np.uint32(5).tobytes(), f32)[0]      # a denormal
    t[ob < 0] = f32(1e15)
    return ob, t


# ------------------------------------------------------------------------------------------------ CPU 1: the ABI
def test_region_stats_layout_matches_header(tmp_path):
    fields = [n for n, _ in abi.crh_region_stats._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "cadrays_hip.h"\nint main(){printf("%zu ", sizeof(crh_region_stats));' + "".join(
        f'printf("%zu ", offsetof(crh_region_stats, {n}));' for n in fields) + 'printf("%d %d", CRH_REGION_TOUCHED, CRH_REGION_ENCLOSED);return 0;}'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [C.sizeof(abi.crh_region_stats)] + [getattr(abi.crh_region_stats, n).offset for n in fields] + [abi.REGION_TOUCHED, abi.REGION_ENCLOSED], got
    assert C.sizeof(abi.crh_region_stats) == 32 and np.dtype(abi.REGION_STATS_DTYPE).itemsize == 32 and np.dtype(abi.REGION_STATS_DTYPE) == ref.STATS_DTYPE
    assert [np.dtype(abi.REGION_STATS_DTYPE).fields[n][1] for n in fields] == [getattr(abi.crh_region_stats, n).offset for n in fields]
    header = open(os.path.join(ROOT, "include", "cadrays_hip.h")).read()
    for name in ("crh_query_region", "crh_region_stats_host", "crh_region_select"):
        assert name in abi.EXPORTS and f"CRH_API int {name}(" in header, name


def test_entry_points_are_exported(hip_lib):
    for name in ("crh_query_region", "crh_region_stats_host", "crh_region_select"):
        assert hasattr(hip_lib, name), name


# ------------------------------------------------------------------------------------------------ CPU 2: the host twin == numpy
@pytest.mark.parametrize("n_objects", [1, 7, 5000])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_twin_equals_the_numpy_restatement(hip_lib, size, n_objects):
    region_stats_host, _ = _api()
    W, H = size
    ob, t = planes(W, H, n_objects, W * 7 + H + n_objects)
    for name, rect, poly in ref.regions(W, H):
        want = ref.stats(ob, t, n_objects, rect, poly)
        got = region_stats_host(ob, t, n_objects, rect, poly)
        assert same_bytes(got, want), (name, differing(got, want))
        assert want["pixels_frame"].sum() == W * H and np.all(want["pixels"] <= want["pixels_frame"])
        if name in ("outside", "empty", "random_256_outside_rect"):
            assert not want["pixels"].any() and not np.frombuffer(want.tobytes(), np.uint32).reshape(-1, 8)[:, 2:].any()
        if name in ("null", "full"):
            assert np.array_equal(want["pixels"], want["pixels_frame"])
    assert want[n_objects]["t_min"] == 0 and want[n_objects]["t_max"] == 0
    # an id outside [0, n_objects) counts as background
    ob2 = ob.copy(); ob2[0, 0] = n_objects + 3
    got, want = region_stats_host(ob2, t, n_objects), ref.stats(ob2, t, n_objects)
    assert same_bytes(got, want)


def test_zero_and_denormal_distances_order_as_values(hip_lib):
    region_stats_host, _ = _api()
    den = np.frombuffer(np.uint32(5).tobytes(), f32)[0]
    t = np.array([[den, 0.0, 3.0, 1e15]], f32); ob = np.array([[0, 0, 1, -1]], np.int32)
    st = region_stats_host(ob, t, 2)
    assert st["t_min"][0].view(np.uint32) == 0 and st["t_max"][0].view(np.uint32) == 5 and st["t_min"][1] == 3.0 == st["t_max"][1]
    st = region_stats_host(ob, t, 2, (0, 0, 1, 1))
    assert st["t_min"][0].view(np.uint32) == 5 == st["t_max"][0].view(np.uint32) and st["pixels"][1] == 0 and st["t_max"][1] == 0 and st["pixels_frame"][1] == 1


# ------------------------------------------------------------------------------------------------ CPU 3: the polygon rule's properties
PW, PH = 61, 37


def twin_mask(poly, rect=None, W=PW, H=PH):
    """the mask the library's rule gives: every pixel its own object, so pixels[o] is the mask"""
    region_stats_host, _ = _api()
    ob = np.arange(W * H, dtype=np.int32).reshape(H, W)
    st = region_stats_host(ob, np.ones((H, W), f32), W * H, rect, poly)
    assert st["pixels"].max() <= 1 and st["pixels"][-1] == 0
    return st["pixels"][:-1].reshape(H, W).astype(bool)


def random_polygon(r, n, lo=-4, W=PW, H=PH):
    return np.stack([r.integers(lo, W - lo + 1, n), r.integers(lo, H - lo + 1, n)], 1).astype(np.int32)


def test_a_rectangle_polygon_is_the_half_open_rectangle(hip_lib):
    for x0, y0, x1, y1 in ((0, 0, PW, PH), (3, 5, 40, 30), (10, 10, 11, 11), (-5, -5, 20, 50), (7, 9, 7, 20)):
        want = np.zeros((PH, PW), bool); want[max(y0, 0):max(min(y1, PH), 0), max(x0, 0):max(min(x1, PW), 0)] = True
        for poly in ([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]):
            assert np.array_equal(twin_mask(poly), want), (x0, y0, x1, y1)
        if x0 >= 0 and y0 >= 0:
            assert np.array_equal(twin_mask(None, (x0, y0, x1, y1)), want)


def test_reversal_and_rotation_of_the_start_vertex_change_nothing(hip_lib):
    r = np.random.default_rng(2)
    for k in range(60):
        p = random_polygon(r, int(r.integers(3, 12)))
        m = twin_mask(p)
        assert np.array_equal(twin_mask(p[::-1]), m)
        assert np.array_equal(twin_mask(np.roll(p, int(r.integers(1, len(p))), 0)), m)


def test_chord_split_a_xor_b_is_p(hip_lib):
    """two polygons that share an edge never both claim a pixel and never both drop it -- centres exactly ON the chord included"""
    r = np.random.default_rng(3)
    on_chord = 0
    for k in range(220):
        n = int(r.integers(4, 14))
        p = random_polygon(r, n)
        if k % 4 == 0:                                   # a chord along a diagonal through pixel centres
            i, j = 0, n // 2
            p[i] = (2, 1); p[j] = (2 + 30, 1 + 30)
        else:
            i, j = sorted(r.choice(n, 2, replace=False))
            if j - i < 2 or (i == 0 and j == n - 1):
                i, j = 0, 2
        A, B = p[i:j + 1], np.concatenate([p[j:], p[:i + 1]])
        mp, ma, mb = twin_mask(p), twin_mask(A), twin_mask(B)
        assert np.array_equal(ma ^ mb, mp), k
        if k % 4 == 0:
            d = np.arange(2, 32)
            on_chord += int((ma[d - 1, d] | mb[d - 1, d]).sum())      # the centres of pixels (d, d - 1) lie on the chord
    assert on_chord > 0                                  # centres on the chord were claimed by one side or the other


def test_a_shift_by_whole_pixels_shifts_the_mask(hip_lib):
    r = np.random.default_rng(4)
    for k in range(40):
        p = np.stack([r.integers(8, PW - 8, 9), r.integers(8, PH - 8, 9)], 1).astype(np.int32)
        dx, dy = int(r.integers(-8, 9)), int(r.integers(-8, 9))
        m, s = twin_mask(p), twin_mask(p + np.array([dx, dy], np.int32))
        assert m.any() and np.array_equal(np.roll(np.roll(m, dy, 0), dx, 1), s)      # the polygon stays inside the frame: nothing wraps


def test_pentagram_centre_is_outside_and_rule_agrees_with_the_restatement(hip_lib):
    p = ref.pentagram(30, 18, 17)
    m = twin_mask(p)
    assert not m[18, 30] and m[18 - 12, 30] and m.sum() > 50      # the centre pentagon is outside under even-odd, the points are inside
    r = np.random.default_rng(5)
    for k in range(40):
        q = random_polygon(r, int(r.integers(3, 40)))
        assert np.array_equal(twin_mask(q), ref.polygon_mask(q, PW, PH))
    far = np.array([(-(1 << 20), -(1 << 20)), ((1 << 20), -(1 << 20)), ((1 << 20), (1 << 20)), (-(1 << 20), (1 << 20))], np.int32)
    assert twin_mask(far).all()


# ------------------------------------------------------------------------------------------------ CPU 4: the selection rule
def test_region_select_truth_table(hip_lib):
    _, region_select = _api()
    st = np.zeros(7, ref.STATS_DTYPE)
    st["pixels"] = [0, 1, 5, 5, 9, 0, 50]
    st["pixels_frame"] = [0, 1, 5, 8, 20, 4, 50]         # hidden; enclosed x2; partly inside x2; visible elsewhere; the background
    for min_pixels in (0, 1, 5, 6, 10):
        for mode in (abi.REGION_TOUCHED, abi.REGION_ENCLOSED):
            got = region_select(st, mode, min_pixels)
            assert got.dtype == np.uint8 and np.array_equal(got, ref.select(st, mode, min_pixels)), (mode, min_pixels)
    assert list(region_select(st, abi.REGION_TOUCHED, 0)) == [0, 1, 1, 1, 1, 0] == list(region_select(st, abi.REGION_TOUCHED, 1))
    assert list(region_select(st, abi.REGION_ENCLOSED, 0)) == [0, 1, 1, 0, 0, 0]
    assert list(region_select(st, abi.REGION_TOUCHED, 5)) == [0, 0, 1, 1, 1, 0] and list(region_select(st, abi.REGION_ENCLOSED, 5)) == [0, 0, 1, 0, 0, 0]
    assert not region_select(st, abi.REGION_TOUCHED, 10).any()
    # an object with no visible pixel is never selected, whatever its other fields say
    st["pixels"][0] = 0; st["pixels_frame"][0] = 0
    assert region_select(st, abi.REGION_ENCLOSED, 0)[0] == 0 and region_select(st, abi.REGION_TOUCHED, 0)[0] == 0
    for mode in (-1, 2):
        with pytest.raises(BackendError):
            region_select(st, mode, 1)


# ------------------------------------------------------------------------------------------------ CPU 5: refusals
def test_refusals(hip_lib):
    region_stats_host, region_select = _api()
    ob, t = planes(20, 10, 3, 1)
    tri = [(0, 0), (10, 0), (5, 8)]
    region_stats_host(ob, t, 3, (0, 0, 20, 10), tri)
    region_stats_host(ob, t, 3, None, [(k % 16, k // 16) for k in range(256)])           # 256 vertices: accepted
    region_stats_host(ob, t, 3, (5, 5, 5, 5))                                              # empty is not inverted
    for n in (1, 2, 257):
        with pytest.raises(BackendError):
            region_stats_host(ob, t, 3, None, [(k % 16, k // 16) for k in range(n)])
    for bad in ((1 << 20) + 1, -(1 << 20) - 1, 2 ** 31 - 1, -2 ** 31):
        for axis in (0, 1):
            p = np.array(tri, np.int64); p[1, axis] = bad
            with pytest.raises(BackendError):
                region_stats_host(ob, t, 3, None, p)
    region_stats_host(ob, t, 3, None, [(1 << 20, -(1 << 20)), (0, 0), (-(1 << 20), 1 << 20)])   # the limit itself is accepted
    for rect in ((5, 0, 4, 10), (0, 7, 20, 6), (30, 0, 25, 5)):
        with pytest.raises(BackendError):
            region_stats_host(ob, t, 3, rect)
    with pytest.raises(BackendError):
        region_stats_host(ob, t, 0)                                                        # n_objects == 0
    # NULL pointers, straight at the library
    out = np.zeros(4, ref.STATS_DTYPE); flags = np.zeros(3, np.uint8)
    po, pt, ps = ob.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(abi.crh_region_stats))
    W, H, n3 = C.c_uint32(20), C.c_uint32(10), C.c_uint32(3)
    host = hip_lib.crh_region_stats_host
    assert host(po, pt, W, H, None, None, C.c_uint32(0), ps, n3) == abi.OK
    assert host(po, pt, W, H, None, None, C.c_uint32(0), None, n3) == abi.E_INVALID
    assert host(None, pt, W, H, None, None, C.c_uint32(0), ps, n3) == abi.E_INVALID
    assert host(po, None, W, H, None, None, C.c_uint32(0), ps, n3) == abi.E_INVALID
    assert host(po, pt, W, H, None, None, C.c_uint32(3), ps, n3) == abi.E_INVALID           # a vertex count without vertices
    assert host(po, pt, C.c_uint32(0), H, None, None, C.c_uint32(0), ps, n3) == abi.E_INVALID
    assert host(po, pt, W, H, None, None, C.c_uint32(0), ps, C.c_uint32(0)) == abi.E_INVALID
    sel = hip_lib.crh_region_select
    pf = flags.ctypes.data_as(C.POINTER(C.c_uint8))
    assert sel(ps, n3, C.c_int(0), C.c_uint32(1), pf) == abi.OK
    assert sel(None, n3, C.c_int(0), C.c_uint32(1), pf) == abi.E_INVALID and sel(ps, n3, C.c_int(0), C.c_uint32(1), None) == abi.E_INVALID
    assert sel(ps, C.c_uint32(0), C.c_int(0), C.c_uint32(1), pf) == abi.E_INVALID
    assert hip_lib.crh_query_region(None, None, None, C.c_uint32(0), ps, n3) == abi.E_INVALID


# ================================================================================================ GPU
def assert_device_equals_numpy_and_twin(v, n_objects, names=None):
    """every region of ref.regions on the context's current state; returns the whole-frame records"""
    region_stats_host, _ = _api()
    ob, _, t = v.read_ids()
    H, W = ob.shape
    whole = None
    for name, rect, poly in ref.regions(W, H):
        if names is not None and name not in names:
            continue
        got = v.query_region(n_objects, rect, poly)
        want = ref.stats(ob, t, n_objects, rect, poly)
        assert same_bytes(got, want), (name, differing(got, want))
        twin = region_stats_host(ob, t, n_objects, rect, poly)
        assert same_bytes(got, twin), (name, differing(got, twin))
        if name == "null":
            whole = got
    return whole


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(61, 37), (200, 120)], ids=["61x37", "200x120"])
def test_a_scene_without_objects_is_one_object(hip_lib, size):
    from cadrays_amd.view import View
    W, H = size
    v = View(0).load_scene(scenes.cornell_box(True, W, H))
    st = assert_device_equals_numpy_and_twin(v, 1)
    assert st["pixels_frame"].sum() == W * H and st["pixels_frame"][0] > 0.3 * W * H and st["t_min"][0] > 0
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"], ids=["one_walk", "two_passes"])
@pytest.mark.parametrize("size", [(61, 37), (200, 120)], ids=["61x37", "200x120"])
def test_device_equals_numpy_and_twin_through_the_states_of_a_live_scene(hip_lib, monkeypatch, size, split):
    from cadrays_amd.view import View
    W, H = size
    monkeypatch.setenv("CRH_SPLIT_PASSES", split)
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc)
    flat = assert_device_equals_numpy_and_twin(v, 7)
    assert (flat["pixels_frame"][:7] > 0).sum() >= 6
    v.set_transforms(moved_xforms(7))
    assert v.get_tlas()["n_instances"] >= 1
    moved = assert_device_equals_numpy_and_twin(v, 7)
    assert not same_bytes(moved, flat)                                  # the query follows the transforms ...
    v.set_visibility(visible_flags(7, [3]))
    erased = assert_device_equals_numpy_and_twin(v, 7)
    assert erased["pixels_frame"][3] == 0 and moved["pixels_frame"][3] > 0      # ... the visibility ...
    p, n, t = one_object(sc, 3)
    assert v.add_object(p, n, t, rigid(30.0, (0, 0, 1), (0.1, -0.3, 0.35))) == 7
    with pytest.raises(BackendError, match="-> -1"):
        v.query_region(7)                                               # one more record now
    added = assert_device_equals_numpy_and_twin(v, 8)
    assert added["pixels_frame"][7] > 0                                 # ... an added object ...
    v.set_camera(dataclasses.replace(sc.camera, eye=(0.2, -3.2, 0.6), dir=(0.1, 1.0, -0.05)))
    turned = assert_device_equals_numpy_and_twin(v, 8, ("null", "pentagram", "beyond"))
    assert not same_bytes(turned, added)                                # ... and the camera
    v.close()


def quad_grid_scene(nx, ny, W, H, extra=0):
    """nx x ny one-quad objects facing an orthographic camera that sees exactly the grid (gaps between the quads: background), plus `extra` one-triangle objects
    far off screen"""
    base = scenes.cornell_box(False, W, H)
    P, T = [], []
    for j in range(ny):
        for i in range(nx):
            x0, x1, z0, z1 = i + 0.1, i + 0.9, j + 0.02, j + 0.98      # (with the eye 0.03 up no pixel centre of a 120-row target falls into the gap between two rows of quads)
            k = len(P)
            P += [(x0, 0, z0), (x1, 0, z0), (x1, 0, z1), (x0, 0, z1)]
            T += [(k, k + 1, k + 2, 0, j * nx + i), (k, k + 2, k + 3, 0, j * nx + i)]
    n_on = nx * ny
    for e in range(extra):
        k = len(P)
        P += [(1000.0 + e, 5.0, 0.0), (1000.5 + e, 5.0, 0.0), (1000.0 + e, 5.0, 0.5)]
        T.append((k, k + 1, k + 2, 0, n_on + e))
    pos = np.array(P, f32); T = np.array(T, np.int32)
    nO = n_on + extra
    cam = scenes.Camera(eye=(nx / 2, -5.0, ny / 2 + 0.03), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fovy_deg=40.0, is_ortho=True, ortho_scale=ny / 2, aspect=nx / ny)
    return dataclasses.replace(base, pos=pos, nrm=np.tile(np.array([0, -1, 0], f32), (len(pos), 1)), tri=np.ascontiguousarray(T[:, :4]), uv=None, textures=[],
                               tri_object=np.ascontiguousarray(T[:, 4]), obj_xform=np.tile(rigid(), (nO, 1)), camera=cam), nO


@pytest.mark.gpu
def test_many_small_objects_every_wavefront_meets_several(hip_lib):
    from cadrays_amd.view import View
    sc, nO = quad_grid_scene(24, 16, 200, 120)
    v = View(0).load_scene(sc)
    st = assert_device_equals_numpy_and_twin(v, nO)
    assert (st["pixels_frame"][:nO] > 0).all() and st["pixels_frame"][nO] > 0      # every quad and the gaps between them are on screen
    ob = v.read_ids()[0]
    assert min(len(np.unique(row[x:x + 64])) for row in ob for x in (0, 64, 128)) >= 5      # several records in every full 64-pixel chunk of every row
    v.close()


@pytest.mark.gpu
def test_five_thousand_objects_most_of_them_off_screen(hip_lib):
    from cadrays_amd.view import View
    sc, nO = quad_grid_scene(12, 8, 200, 120, extra=5000)
    assert nO == 5096
    v = View(0).load_scene(sc)
    st = assert_device_equals_numpy_and_twin(v, nO, ("null", "beyond", "pentagram", "random_256", "concave_L"))
    assert (st["pixels_frame"][:96] > 0).all() and not st["pixels_frame"][96:nO].any()
    _, region_select = _api()
    assert region_select(st, abi.REGION_TOUCHED, 1).sum() == 96
    v.close()


GRID_CHUNKS = 1024 * 4 * 4            # at least the region kernel's largest grid (at most 4 workgroups per compute unit, 256 of them) x wavefronts per workgroup x chunks of 64 pixels per round


@pytest.mark.gpu
def test_one_object_filling_a_frame_that_takes_a_second_round(hip_lib):
    from cadrays_amd.view import View
    W = 1000                            # 16 chunks per row, the last one 40 pixels wide
    H = GRID_CHUNKS // 16 + 7           # 16496 chunks: every wavefront's first round is full, 112 chunks go to a second one
    assert -(-W // 64) * H > GRID_CHUNKS
    base = scenes.cornell_box(False, W, H)
    pos = np.array([(-50, 2, -50), (50, 2, -50), (50, 2, 50), (-50, 2, 50)], f32)
    sc = dataclasses.replace(base, pos=pos, nrm=np.tile(np.array([0, -1, 0], f32), (4, 1)), tri=np.array([(0, 1, 2, 0), (0, 2, 3, 0)], np.int32), uv=None, textures=[],
                             camera=scenes.Camera(eye=(0.0, -1.0, 0.0), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fovy_deg=40.0))
    v = View(0).load_scene(sc)
    st = assert_device_equals_numpy_and_twin(v, 1, ("null", "beyond", "one_pixel", "pentagram", "outside"))
    assert st["pixels_frame"][0] == W * H and st["pixels"][0] == W * H and st["pixels_frame"][1] == 0
    assert (st["x0"][0], st["y0"][0], st["x1"][0], st["y1"][0]) == (0, 0, W, H) and 3.0 <= st["t_min"][0] < st["t_max"][0]
    # the camera turned away: only the background record is non-zero
    v.set_camera(dataclasses.replace(sc.camera, dir=(0.0, -1.0, 0.0)))
    st = assert_device_equals_numpy_and_twin(v, 1, ("null", "pentagram"))
    assert not np.frombuffer(st[:1].tobytes(), np.uint32).any()
    assert st["pixels"][1] == W * H == st["pixels_frame"][1] and st["t_min"][1] == 0 and st["t_max"][1] == 0 and st["x1"][1] == W and st["y1"][1] == H
    v.close()


def _queries(v, W, H):
    v.query_region(7)
    v.query_region(7, (W // 4, H // 4, W, H))
    v.query_region(7, None, ref.pentagram(W // 2, H // 2, H // 2))


@pytest.mark.gpu
def test_queries_leave_everything_else_alone(hip_lib):
    from cadrays_amd.view import View
    W, H = 128, 96
    sc = object_scene(None, W, H)
    counters = ("rays_nearest", "rays_any", "shaded_hits", "samples")
    flags = np.array([0, 0, 0, 1, 0, 1, 0], np.uint8)
    ref_v = View(0).load_scene(sc)
    ref_v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(3): ref_v.Redraw()
    ldr3 = ref_v.read_ldr()
    for _ in range(5): ref_v.Redraw()
    want, (want_acc, want_frames), want_stats, want_ldr = ref_v.read_hdr(), ref_v.save_accum(), ref_v.stats(), ref_v.read_ldr()
    # between blocks of frames, with an asynchronous LDR read-back that draws an overlay in flight across the queries (the id buffer is stale when they start)
    v = View(0).load_scene(sc)
    v.set_selection(flags, (255, 0, 0), 128)
    for _ in range(3): v.Redraw()
    v.read_ldr_begin()
    _queries(v, W, H)
    assert np.array_equal(v.read_ldr_end(), ldr3)
    ids = v.read_ids()[0]
    for _ in range(5): v.Redraw()
    _queries(v, W, H)
    acc, frames = v.save_accum()
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and frames == want_frames == 8
    assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32))
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    assert np.array_equal(v.read_ldr(), want_ldr) and np.array_equal(v.read_ids()[0], ids)      # the selection and the id buffer are what they were
    v.close()
    # in a free-running loop, three frames in flight, a read-back in flight around the queries
    v = View(0).load_scene(sc); v.set_pipeline_depth(3)
    v.set_selection(flags, (255, 0, 0), 128)
    for k in range(8):
        v.Redraw()
        if k in (2, 5):
            v.read_ldr_begin()
            _queries(v, W, H)
            v.read_ldr_end()
        elif k == 3:
            v.query_region(7, (1, 1, 9, 9))
    assert np.array_equal(v.read_hdr().view(np.uint32), want.view(np.uint32)) and v.save_accum()[1] == 8
    st = v.stats()
    assert all(st[k] == want_stats[k] for k in counters), (st, want_stats)
    assert np.array_equal(v.read_ldr(), want_ldr)
    v.close(); ref_v.close()


@pytest.mark.gpu
def test_view_select_rect_lasso_and_visible_objects(hip_lib):
    from cadrays_amd.view import View
    W, H = 96, 96
    sc = object_scene(None, W, H)
    v = View(0).load_scene(sc); f = View(0).load_scene(sc)
    for _ in range(2): v.Redraw(); f.Redraw()
    ob, _, t = v.read_ids()

    def expect(flags):
        f.set_selection(flags if flags.any() else None, f.selection_rgb, f.selection_alpha)
        return f.read_ldr()

    lasso = ref.pentagram(W // 2, H // 2, 40)
    cases = [(lambda **k: v.SelectRect(20, 30, 80, 90, **k), (20, 30, 80, 90), None), (lambda **k: v.SelectLasso(lasso, **k), None, lasso)]
    for call, rect, poly in cases:
        st = ref.stats(ob, t, 7, rect, poly)
        for mode in (abi.REGION_TOUCHED, abi.REGION_ENCLOSED):
            for min_pixels in (1, 200):
                want = ref.select(st, mode, min_pixels)
                assert call(mode=mode, min_pixels=min_pixels) == set(np.flatnonzero(want).tolist())
                assert np.array_equal(v.read_ldr(), expect(want))
        assert ref.select(st, abi.REGION_TOUCHED, 1).sum() > ref.select(st, abi.REGION_ENCLOSED, 1).sum() > 0 or poly is not None
    # shift toggles
    v.SelectRect(0, 0, W, H)
    everything = set(np.flatnonzero(ref.select(ref.stats(ob, t, 7), abi.REGION_TOUCHED, 1)).tolist())
    assert v._selected == everything and len(everything) >= 6
    inner = set(np.flatnonzero(ref.select(ref.stats(ob, t, 7, (20, 30, 80, 90)), abi.REGION_TOUCHED, 1)).tolist())
    assert v.SelectRect(20, 30, 80, 90, shift=True) == everything - inner
    flags = np.zeros(7, np.uint8); flags[sorted(everything - inner)] = 1
    assert np.array_equal(v.read_ldr(), expect(flags))
    assert v.SelectRect(W + 1, 0, W + 5, 5) == set() and np.array_equal(v.read_ldr(), expect(np.zeros(7, np.uint8)))
    # visible objects
    vis = v.VisibleObjects()
    whole = ref.stats(ob, t, 7)
    assert set(vis) == set(np.flatnonzero(whole["pixels_frame"][:7] > 0).tolist())
    for o, r in vis.items():
        assert all(r[n] == whole[n][o] for n in whole.dtype.names)
    assert set(v.VisibleObjects(500)) == set(np.flatnonzero(whole["pixels_frame"][:7] >= 500).tolist())
    assert v.stats()["samples"] == 2 * W * H                 # none of this restarted anything
    v.close(); f.close()


@pytest.mark.gpu
def test_query_argument_errors(hip_lib):
    from cadrays_amd.view import View
    sc = object_scene(None, 64, 48)
    v = View(0)
    v.set_geometry(sc.pos, sc.nrm, sc.tri, None, sc.tri_object, sc.obj_xform); v.set_params(sc.params); v.set_camera(sc.camera)
    with pytest.raises(BackendError, match="-> -4.*crh_build has not been called"):
        v.query_region(7)
    v.load_scene(sc)
    for n in (0, 6, 8):
        with pytest.raises(BackendError, match=rf"-> -1: crh_query_region: {n} records for a scene of 7 objects"):
            v.query_region(n)
    with pytest.raises(BackendError, match="-> -1: crh_query_region: the rectangle is inverted"):
        v.query_region(7, (10, 0, 9, 5))
    for n in (1, 2, 257):
        with pytest.raises(BackendError, match="-> -1: crh_query_region: a polygon takes 3 to 256 vertices"):
            v.query_region(7, None, [(k % 16, k // 16) for k in range(n)])
    with pytest.raises(BackendError, match=r"-> -1: crh_query_region: a polygon coordinate lies beyond"):
        v.query_region(7, None, [(0, 0), ((1 << 20) + 1, 0), (5, 5)])
    out = np.zeros(8, ref.STATS_DTYPE)
    assert v._fn("query_region")(v._ctx, None, None, C.c_uint32(0), None, C.c_uint32(7)) == abi.E_INVALID      # NULL output
    st = v.query_region(7, (0, 0, 1 << 30, 1 << 30))         # cut to the target
    assert same_bytes(st, v.query_region(7))
    v.close()
    w = View(0).load_scene(scenes.cornell_box(True, 64, 48))
    with pytest.raises(BackendError, match="1 objects"):
        w.query_region(7)
    assert w.query_region(1)["pixels_frame"].sum() == 64 * 48
    w.close()
