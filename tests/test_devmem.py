"""The owning buffer type of the host side (cadrays_amd/csrc/crh_devmem.h) on the CPU: tests/devmem_model.cpp -- the library's allocation sequences against a
memory policy that records the live blocks and refuses its k-th allocation, for every k -- compiled with ASan + UBSan and run.  No GPU, no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_model(tmp_path):
    exe = str(tmp_path / "devmem_model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "cadrays_amd", "csrc"), os.path.join(ROOT, "tests", "devmem_model.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().startswith("ok:"), p.stdout[-2000:] + p.stderr[-6000:]


# ------------------------------------------------------------------------------------------------ GPU: buffers that grow, shrink and grow again
def _parts():
    """the smallest CAD-like scene (8 parts of 60 - 64 triangles): parts 0..2 are the scene's objects, part 3 and parts 4..7 (as ONE object) are added later"""
    import numpy as np
    from cadrays_amd import scenes
    pos, nrm, tri, ob = scenes.gen_cad_like(512, 1, 2, True)

    def take(which):
        t = tri[np.isin(ob, which)]
        vid, inv = np.unique(t[:, :3], return_inverse=True)
        return pos[vid], nrm[vid], np.concatenate([inv.reshape(-1, 3).astype(np.int32), t[:, 3:4]], 1)
    return take, ob


def _scene(W, H):
    import numpy as np
    from cadrays_amd import scenes
    from cadrays_amd.materials import BSDF
    take, ob = _parts()
    pos, nrm, tri = take([0, 1, 2])
    owner = ob[ob <= 2].astype(np.int32)
    ident = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (3, 1))
    return scenes.Scene(pos, nrm, tri, [BSDF.CreateDiffuse(0.8), BSDF.Glossy(0.5, 0.5, 0.1, 0.8), BSDF.CreateGlass(1.0, (0.8, 0.8, 1.0), 6.0, 1.5)],
                        lights=[scenes.Light.directional(**scenes.DEFAULT_LIGHT)], camera=scenes.Camera(),
                        params=scenes.Params(width=W, height=H, max_depth=4, seed=3, background=(0.3, 0.35, 0.4)), tri_object=owner, obj_xform=ident)


def _shift(x, y, z):
    import numpy as np
    return np.array([1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z], np.float32)


def _add_two(v):
    take, ob = _parts()
    n0, n1, n2 = int((ob <= 2).sum()), int((ob == 3).sum()), int((ob >= 4).sum())
    # crh_build leaves 2 * n0 leaf positions, all of them spoken for; crh_add_object grows the arrays to n_pos + reserved + 2 * nT + cap / 4: the second
    # object must need more than the first one's growth left over
    assert n2 > n1 + n0 // 2
    assert v.add_object(*take([3]), _shift(0.1, -0.2, 0.1)) == 3
    assert v.add_object(*take([4, 5, 6, 7]), _shift(-0.1, -0.3, -0.1)) == 4
    import numpy as np
    v.set_transforms(np.stack([_shift(0.0, 0.0, 0.0), _shift(0.05, 0.0, 0.1), _shift(0.0, 0.0, 0.0), _shift(0.1, -0.25, 0.0), _shift(-0.15, -0.3, -0.1)]))


def _observe(v):
    """everything a host reads, in one fixed order; bytes only"""
    import numpy as np
    W, H, n = v.width, v.height, v._n_objects
    out = []
    v.reset(); v.render(2); out.append(v.read_hdr().tobytes())
    flags = np.zeros(n, np.uint8); flags[1] = 1
    v.set_selection(flags); v.set_hover(n - 1)
    out.append(v.read_ldr().tobytes())
    v.read_ldr_begin(); out.append(v.read_ldr_end().tobytes())
    out += [a.tobytes() for a in v.read_ids()]
    poly = np.array([(W // 8, H // 8), (W - 3, H // 5), (W - W // 4, H - 2), (W // 2, H // 2), (W // 6, H - H // 7)], np.int32)
    out.append(v.query_region(n, None, poly).tobytes())
    cam, res = v.fit_view(n, want_extents=True)
    out.append(repr(sorted((k, np.asarray(x, np.float32).tobytes()) for k, x in cam.items())) + repr(sorted((k, np.asarray(x).tobytes()) for k, x in res.items())))
    v.set_adaptive(True, 8); v.set_show_tiles(True)
    v.render(2); out.append(v.read_ldr().tobytes()); out.append(v.read_hdr().tobytes())
    v.set_show_tiles(False); v.set_adaptive(False); v.set_selection(None); v.set_hover(None)
    return out


@pytest.mark.gpu
def test_hip_buffers_regrow_in_both_directions_like_a_fresh_context(hip_lib):
    """ONE context through the growth of its buffers in both directions -- target size 64x64 -> 200x136 (no multiple of the 32-pixel tile or the 8x8 id block)
    -> 64x64, two added objects (the second makes the leaf-ordered arrays grow), the path budget down to 1024 * 64 slots and back -- reads, at every step, the
    bytes of a fresh context brought straight to that state (the state the oracle-parity tests pin): the frame, both LDR read-outs with selection and hover,
    the id buffer, a lasso query, the fitted view, an adaptive iteration with ShowSamplingTiles."""
    import dataclasses
    from cadrays_amd.view import View

    def fresh(W, H, added=False, budget=None):
        f = View(0).load_scene(_scene(W, H))
        if added:
            _add_two(f)
        if budget:
            f.set_path_budget(budget)
        got = _observe(f)
        f.close()
        return got

    def same(a, b, what):
        assert len(a) == len(b) and [i for i in range(len(a)) if a[i] != b[i]] == [], what

    sc = _scene(64, 64)
    v = View(0).load_scene(sc)
    for W, H in ((64, 64), (200, 136), (64, 64)):
        v.set_params(dataclasses.replace(sc.params, width=W, height=H))
        same(_observe(v), fresh(W, H), (W, H))
    _add_two(v)
    grown = fresh(64, 64, added=True)
    same(_observe(v), grown, "two added objects")
    full = v.get_path_budget()
    v.set_path_budget(1024 * 64)
    same(_observe(v), fresh(64, 64, added=True, budget=1024 * 64), "path budget down")
    v.set_path_budget(full)
    same(_observe(v), grown, "path budget back")
    v.close()
