"""Thin ctypes binding over a library that exports the cadrays_hip.h entry points under a prefix.

The product binds prefix 'crh_' on libcadrays_hip.so (cadrays_amd/view.py); the test suite binds
prefix 'orc_' on the CPU oracle with this same class, so the parity tests drive both sides through
the same calls with the same bytes.
"""
import ctypes as C
import os
import numpy as np

from . import abi
from .materials import pack_materials

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)


class BackendError(RuntimeError):
    pass


def _fp(a):
    return a.ctypes.data_as(_f32p) if a is not None else None


_live = None      # weak set of open contexts: closed by an atexit hook, i.e. BEFORE the interpreter tears modules (and with them the HIP
                  # runtime torch loaded) down in arbitrary order -- a context destroyed after that calls into a dead runtime


def _close_all():
    for b in list(_live or ()):
        try:
            b.close()
        except Exception:
            pass


def _params(kind, what, fields):
    """abi.crh_<kind>_params: the defaults (abi.<KIND>_DEFAULTS == crh_<kind>_defaults) with the named fields replaced, each converted to its ctypes field's type;
    an unknown name is an error, worded with `what`"""
    defaults, struct = getattr(abi, f"{kind.upper()}_DEFAULTS"), getattr(abi, f"crh_{kind}_params")
    unknown = sorted(set(fields) - set(defaults))
    if unknown:
        raise ValueError(f"no such {what} parameter {unknown}; crh_{kind}_params has {sorted(defaults)}")
    v, p = dict(defaults, **fields), struct()
    for name, ctype in struct._fields_:
        is_array = hasattr(ctype, "_length_")
        conv = float if (ctype._type_ if is_array else ctype) is C.c_float else int
        if is_array:
            getattr(p, name)[:] = [conv(x) for x in v[name]]
        else:
            setattr(p, name, conv(v[name]))
    return p


def meter_params(**fields):
    """abi.crh_meter_params: the defaults (abi.METER_DEFAULTS == crh_meter_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("meter", "metering", fields)


def camera_struct(cam):
    """abi.crh_camera of a scenes.Camera (or anything with its fields)"""
    c = abi.crh_camera()
    c.eye[:] = [float(x) for x in cam.eye]
    c.dir[:] = [float(x) for x in cam.dir]
    c.up[:] = [float(x) for x in cam.up]
    c.fovy_deg, c.aspect = float(cam.fovy_deg), float(cam.aspect)
    c.is_ortho, c.ortho_scale = int(cam.is_ortho), float(cam.ortho_scale)
    c.aperture_radius, c.focal_dist = float(cam.aperture_radius), float(cam.focal_dist)
    return c


def camera_fields(c):
    """the fields of an abi.crh_camera as keyword arguments of scenes.Camera / dataclasses.replace (float32 values as Python floats: they survive the way back)"""
    return dict(eye=tuple(float(x) for x in c.eye), dir=tuple(float(x) for x in c.dir), up=tuple(float(x) for x in c.up), fovy_deg=float(c.fovy_deg),
                aspect=float(c.aspect), is_ortho=bool(c.is_ortho), ortho_scale=float(c.ortho_scale), aperture_radius=float(c.aperture_radius),
                focal_dist=float(c.focal_dist))


def region_args(rect, poly):
    """(rect pointer or None, polygon pointer or None, vertex count, the arrays kept alive) for crh_query_region / crh_region_stats_host: rect = (x0, y0, x1, y1)
    half-open or None = the whole frame; poly = (n, 2) integer pixel-corner vertices or None"""
    r = None if rect is None else np.ascontiguousarray(rect, np.uint32).reshape(4)
    q = None if poly is None else np.ascontiguousarray(poly, np.int32).reshape(-1, 2)
    return (None if r is None else r.ctypes.data_as(_u32p), None if q is None else q.ctypes.data_as(_i32p), C.c_uint32(0 if q is None else len(q)), (r, q))


def outline_params(**fields):
    """abi.crh_outline_params: the defaults (abi.OUTLINE_DEFAULTS == crh_outline_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("outline", "outline", fields)


def denoise_params(**fields):
    """abi.crh_denoise_params: the defaults (abi.DENOISE_DEFAULTS == crh_denoise_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("denoise", "denoise", fields)


def shade_guide_params(**fields):
    """abi.crh_shade_guide_params: the defaults (abi.SHADE_GUIDE_DEFAULTS == crh_shade_guide_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("shade_guide", "shade guide", fields)


def reproject_params(**fields):
    """abi.crh_reproject_params: the defaults (abi.REPROJECT_DEFAULTS == crh_reproject_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("reproject", "reproject", fields)


def reproject_motion_params(**fields):
    """abi.crh_reproject_motion_params: the defaults (abi.REPROJECT_MOTION_DEFAULTS == crh_reproject_motion_defaults) with the named fields replaced; an unknown name is an error"""
    return _params("reproject_motion", "reproject motion", fields)


def view_params(**fields):
    """abi.crh_view_params: the whole frame under CRH_VIEW_AUTO (abi.VIEW_DEFAULTS) with the named fields replaced -- width and height must be; an unknown name is an error"""
    return _params("view", "view", fields)


def pack_lights(lights):
    """an array of abi.crh_light (at least one entry) of scenes.Light objects, as crh_set_lights takes them"""
    arr = (abi.crh_light * max(len(lights), 1))()
    for i, l in enumerate(lights):
        arr[i].vec[:] = [float(x) for x in l.vec]
        arr[i].is_point = 1.0 if l.is_point else 0.0
        arr[i].emission[:] = [float(np.float32(c) * np.float32(l.intensity)) for c in l.color]
        arr[i].smoothness = float(l.smoothness)
    return arr


class Backend:
    """One rendering context ( == one V3d_View on one GPU )."""

    def __init__(self, lib, prefix, create_args=()):
        global _live
        self._lib, self._p = lib, prefix
        f = self._fn("create")
        f.restype = C.c_void_p
        self._ctx = C.c_void_p(f(*create_args))
        if not self._ctx.value:
            raise BackendError(f"{prefix}create failed")
        if _live is None:
            import atexit, weakref
            _live = weakref.WeakSet()
            if not os.environ.get("CRH_NO_ATEXIT_CLOSE"): atexit.register(_close_all)      # the switch exists to measure what the hook prevents
        _live.add(self)
        self.width = self.height = 0
        self._fn("last_error").restype = C.c_char_p

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _call(self, name, *args):
        rc = self._fn(name)(self._ctx, *args)                  # (restype of a ctypes function defaults to c_int)
        if rc != 0:
            msg = self._fn("last_error")(self._ctx)
            raise BackendError(f"{self._p}{name} -> {rc}: {msg.decode() if msg else ''}")
        return rc

    def close(self):
        if self._ctx and self._ctx.value:
            f = self._fn("destroy")
            f.restype = None
            f(self._ctx)
            self._ctx = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene ---------------------------------------------------------------------------
    def set_geometry(self, pos, nrm, tri, uv=None, tri_object=None, obj_xform=None):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 4)
        uv = None if uv is None else np.ascontiguousarray(uv, np.float32)
        to = None if tri_object is None else np.ascontiguousarray(tri_object, np.int32)
        self._has_objects = to is not None
        xf = None if obj_xform is None else np.ascontiguousarray(obj_xform, np.float32).reshape(-1, 12)
        self._call("set_geometry", _fp(pos), _fp(nrm), _fp(uv), C.c_uint32(len(pos)),
                   tri.ctypes.data_as(_i32p), C.c_uint32(len(tri)),
                   to.ctypes.data_as(_i32p) if to is not None else None,
                   _fp(xf), C.c_uint32(0 if xf is None else len(xf)))

    def set_transforms(self, obj_xform):
        """new per-object 3x4 transforms of a two-level scene: only the top-level tree is rebuilt (ImRaytraceControls.cxx:58-89)"""
        xf = np.ascontiguousarray(obj_xform, np.float32).reshape(-1, 12)
        self._call("set_transforms", _fp(xf), C.c_uint32(len(xf)))

    def set_visibility(self, visible):
        """Display / Erase without a rebuild (DataNode.cxx:304-344): one flag per object"""
        v = np.ascontiguousarray(np.asarray(visible) != 0, np.uint8)
        self._call("set_visibility", v.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(len(v)))

    def add_object(self, pos, nrm, tri, xform, uv=None):
        """a new object into the built scene (an instance until the next full build); returns its object index"""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 4)
        uv = None if uv is None else np.ascontiguousarray(uv, np.float32)
        xf = np.ascontiguousarray(xform, np.float32).reshape(12)
        out = C.c_uint32(0)
        self._call("add_object", _fp(pos), _fp(nrm), _fp(uv), C.c_uint32(len(pos)), tri.ctypes.data_as(_i32p), C.c_uint32(len(tri)), _fp(xf), C.byref(out))
        return int(out.value)

    def get_tlas(self):
        r, n, b = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._call("get_tlas", C.byref(r), C.byref(n), C.byref(b))
        return {"root": r.value, "n_instances": n.value, "n_blas_nodes": b.value}

    def set_materials(self, bsdfs):
        arr = pack_materials(bsdfs)
        self._call("set_materials", arr, C.c_uint32(len(bsdfs)))

    def set_lights(self, lights):
        self._call("set_lights", pack_lights(lights), C.c_uint32(len(lights)))

    def set_envmap(self, env):
        if env is None:
            self._call("set_envmap", None, C.c_uint32(0), C.c_uint32(0))
        else:
            env = np.ascontiguousarray(env, np.float32)
            h, w, _ = env.shape
            self._call("set_envmap", _fp(env), C.c_uint32(w), C.c_uint32(h))

    def set_texture(self, slot, image):
        if image is None:
            self._call("set_texture", C.c_uint32(slot), None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(3))
        else:
            image = np.ascontiguousarray(image, np.float32)
            h, w, ch = image.shape                       # (H, W, 3) RGB or (H, W, 4) RGBA
            self._call("set_texture", C.c_uint32(slot), _fp(image), C.c_uint32(w), C.c_uint32(h), C.c_uint32(ch))

    def set_camera(self, cam):
        self._call("set_camera", C.byref(camera_struct(cam)))

    def set_params(self, p):
        q = abi.crh_params()
        q.width, q.height, q.max_depth = int(p.width), int(p.height), int(p.max_depth)
        q.radiance_clamp, q.two_sided, q.coherent_rng = float(p.radiance_clamp), int(p.two_sided), int(p.coherent_rng)
        q.seed, q.tile_size, q.tonemap_mode = int(p.seed), int(p.tile_size), int(p.tonemap_mode)
        q.exposure, q.white_point = float(p.exposure), float(p.white_point)
        q.background[:] = [float(x) for x in p.background]
        q.env_as_background, q.scene_epsilon = int(p.env_as_background), float(p.scene_epsilon)
        q.russian_roulette = int(p.russian_roulette)
        self._call("set_params", C.byref(q))
        self.width, self.height, self.tile_size = int(p.width), int(p.height), int(p.tile_size)

    def set_spec(self, **switches):
        """crh_set_spec: flip switches of include/crh_spec.h (abi.SPEC_DEFAULTS names them all); the ones not named return to their defaults.
        An unknown name is an error, not a silently ignored switch.  Restarts accumulation."""
        unknown = sorted(set(switches) - set(abi.SPEC_DEFAULTS))
        if unknown:
            raise ValueError(f"set_spec: no such switch {unknown}; include/crh_spec.h has {sorted(abi.SPEC_DEFAULTS)}")
        vals = dict(abi.SPEC_DEFAULTS); vals.update(switches)
        sp = abi.crh_spec(size=C.sizeof(abi.crh_spec))
        for name, ctype in abi.crh_spec._fields_[1:]:
            setattr(sp, name, float(vals[name]) if ctype is C.c_float else int(vals[name]))
        self._call("set_spec", C.byref(sp))

    def get_spec(self):
        sp = abi.crh_spec(size=C.sizeof(abi.crh_spec))      # in / out: the caller's struct size, exactly that many bytes are written
        self._call("get_spec", C.byref(sp))
        return sp.as_dict()

    def spec_order_exact(self):
        """the build-time switch CRH_SPEC_ORDER_EXACT of the loaded library (crh_spec.h #4)"""
        f = self._fn("spec_order_exact"); f.restype = C.c_int
        return int(f())

    def spec_anyhit_slot_order(self):
        """the build-time switch CRH_SPEC_ANYHIT_SLOT_ORDER of the loaded library (crh_spec.h #8)"""
        f = self._fn("spec_anyhit_slot_order"); f.restype = C.c_int
        return int(f())

    def load_scene(self, scene, prebuilt=None):
        """prebuilt = (nodes, prim_order) of another context's tree over the same geometry (crh_build_prebuilt) instead of building one here"""
        self.set_geometry(scene.pos, scene.nrm, scene.tri, scene.uv, getattr(scene, "tri_object", None), getattr(scene, "obj_xform", None))
        self.set_materials(scene.materials)
        self.set_lights(scene.lights)
        self.set_envmap(scene.env)
        self.set_camera(scene.camera)
        self.set_params(scene.params)
        for slot, img in enumerate(getattr(scene, "textures", []) or []):
            self.set_texture(slot, img)
        if getattr(scene, "spec", None):
            self.set_spec(**scene.spec)
        if prebuilt is not None:
            self.build_prebuilt(*prebuilt)
        else:
            self.build()
        return self

    # -- rendering -----------------------------------------------------------------------
    def build(self):
        self._call("build")

    def build_prebuilt(self, nodes, prim_order):
        """crh_build_prebuilt: this context takes the tree another one built for the same geometry (export_tree)"""
        nodes = np.ascontiguousarray(nodes).view(np.float32).reshape(-1, abi.NODE_DWORDS)
        order = np.ascontiguousarray(prim_order, np.uint32)
        self._call("build_prebuilt", _fp(nodes), C.c_uint32(len(nodes)), order.ctypes.data_as(_u32p), C.c_uint32(len(order)))

    def export_tree(self):
        """(nodes, prim_order) for build_prebuilt of another context: the node array and the leaf order (dword 3 of the leaf-ordered triangle records)"""
        nodes, tris = self.get_bvh()
        return nodes, np.ascontiguousarray(tris[:, 3]).view(np.uint32).copy()

    def reset(self):
        self._call("reset")

    def render(self, n_iterations=1):
        self._call("render", C.c_uint32(n_iterations))

    def render_tiles(self, tile_ids, first_sample, n_samples):
        t = np.ascontiguousarray(tile_ids, np.uint32)
        self._call("render_tiles", t.ctypes.data_as(_u32p), C.c_uint32(len(t)),
                   C.c_uint32(first_sample), C.c_uint32(n_samples))

    def set_adaptive(self, on=True, tiles_per_iteration=128):
        """AdaptiveScreenSampling / NbRayTracingTiles (SettingsWidget.cxx:427-477); restarts accumulation."""
        self._call("set_adaptive", C.c_int(int(on)), C.c_uint32(int(tiles_per_iteration)))

    def set_show_tiles(self, on=True):
        """ShowSamplingTiles (SettingsWidget.cxx:443-449): outline the tiles of the last adaptive iteration in read_ldr()."""
        self._call("set_show_tiles", C.c_int(int(on)))

    def tile_stats(self):
        n = C.c_uint32(0)
        self._call("get_tile_stats", None, None, C.byref(n))
        err, cnt = np.empty(n.value, np.float32), np.empty(n.value, np.uint32)
        self._call("get_tile_stats", _fp(err), cnt.ctypes.data_as(_u32p), C.byref(n))
        return err, cnt

    def n_tiles(self):
        ts = self.tile_size or 32
        return ((self.width + ts - 1) // ts) * ((self.height + ts - 1) // ts)

    def read_hdr(self):
        out = np.empty((self.height, self.width, 3), np.float32)
        self._call("read_hdr", _fp(out))
        return out

    def read_ldr(self):
        out = np.empty((self.height, self.width, 3), np.uint8)
        self._call("read_ldr", out.ctypes.data_as(_u8p))
        return out

    def read_ldr_begin(self):
        """queue tone map + read-back of the frame as submitted so far; returns at once (crh_read_ldr_begin)"""
        self._call("read_ldr_begin")
        self._rb_shapes = getattr(self, "_rb_shapes", []) + [(self.height, self.width, 3)]

    def read_ldr_end(self, out=None):
        """the oldest begun read-back (crh_read_ldr_end).  `out`: a C-contiguous uint8 array of the frame's shape to fill instead of a fresh one -- what a GUI
        host does (one staging buffer for the texture upload, INTEGRATION.md `myLdr`): a fresh 6 MB array per 1080p frame is 1500 first-touch page faults"""
        pending = getattr(self, "_rb_shapes", None)
        shape = pending[0] if pending else (self.height, self.width, 3)
        if out is None:
            out = np.empty(shape, np.uint8)
        elif out.dtype != np.uint8 or out.shape != tuple(shape) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError(f"read_ldr_end(out=...): need a writeable C-contiguous uint8 array of shape {tuple(shape)}")
        self._call("read_ldr_end", out.ctypes.data_as(_u8p))
        if pending: pending.pop(0)
        return out

    def read_hdr_begin(self):
        """queue the HDR read-back of the frame as submitted so far; returns at once (crh_read_hdr_begin)"""
        self._call("read_hdr_begin")
        self._rbh_shapes = getattr(self, "_rbh_shapes", []) + [(self.height, self.width, 3)]

    def read_hdr_end(self):
        shape = self._rbh_shapes.pop(0) if getattr(self, "_rbh_shapes", None) else (self.height, self.width, 3)
        out = np.empty(shape, np.float32)
        self._call("read_hdr_end", _fp(out))
        return out

    # -- viewport read-out: the frame at the window's size (crh_view.cpp; AppViewer.cxx:929-1102) ------
    def read_view(self, width, height, src=(0, 0, 0, 0), filter=abi.VIEW_AUTO):
        """crh_read_view: (height, width, 3) uint8, the frame read_ldr would return resampled to the window's size; src = (x0, y0, x1, y1) half-open in frame
        pixels (all zero: the whole frame) zooms and pans without a restart; filter: abi.VIEW_AUTO / _NEAREST / _BILINEAR / _AREA"""
        p = view_params(width=width, height=height, src=src, filter=filter)
        out = np.empty((p.height, p.width, 3), np.uint8)
        self._call("read_view", C.byref(p), out.ctypes.data_as(_u8p))
        return out

    def read_view_begin(self, width, height, src=(0, 0, 0, 0), filter=abi.VIEW_AUTO):
        """queue display chain + resample + read-back of the frame as submitted so far; returns at once (crh_read_view_begin).  Shares the two slots with
        read_ldr_begin / read_hdr_begin: the oldest in flight is ended by the call of its own kind"""
        p = view_params(width=width, height=height, src=src, filter=filter)
        self._call("read_view_begin", C.byref(p))
        self._rbv_shapes = getattr(self, "_rbv_shapes", []) + [(p.height, p.width, 3)]

    def read_view_end(self, out=None):
        """the oldest begun view (crh_read_view_end); `out` as in read_ldr_end, of the shape its read_view_begin asked for"""
        pending = getattr(self, "_rbv_shapes", None)
        if not pending and out is None:
            raise ValueError("read_view_end: no read_view_begin of this object is pending, so the size of the view is not known; pass out=")
        shape = pending[0] if pending else out.shape
        if out is None:
            out = np.empty(shape, np.uint8)
        elif out.dtype != np.uint8 or out.shape != tuple(shape) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError(f"read_view_end(out=...): need a writeable C-contiguous uint8 array of shape {tuple(shape)}")
        self._call("read_view_end", out.ctypes.data_as(_u8p))
        if pending: pending.pop(0)
        return out

    def bench_view(self, width, height, src=(0, 0, 0, 0), filter=abi.VIEW_AUTO, repeats=20):
        """crh_bench_view: device time per launch of the resample kernel over the frame a read-out issued now would show, in ms (HIP events)"""
        p, ms = view_params(width=width, height=height, src=src, filter=filter), C.c_float(0)
        self._call("bench_view", C.byref(p), C.c_uint32(int(repeats)), C.byref(ms))
        return float(ms.value)

    # -- display state and auto exposure (no restart; SettingsWidget.cxx:343-404) -----------
    def set_display(self, tonemap_mode, exposure, white_point):
        """crh_set_display: tone-map mode, exposure [stops] and white point of every LDR read-out from now on; the accumulation goes on"""
        self._call("set_display", C.c_int(int(tonemap_mode)), C.c_float(float(exposure)), C.c_float(float(white_point)))

    def get_display(self):
        """crh_get_display: dict(tonemap_mode, exposure, white_point, auto_on) as in force"""
        m, e, w, a = C.c_int(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._call("get_display", C.byref(m), C.byref(e), C.byref(w), C.byref(a))
        return {"tonemap_mode": int(m.value), "exposure": e.value, "white_point": w.value, "auto_on": bool(a.value)}

    def set_auto_exposure(self, on=True, **params):
        """crh_set_auto_exposure: every LDR read-out meters the image it is about to show (fields of crh_meter_params by name, the others take
        crh_meter_defaults; rect = (x0, y0, x1, y1)); on=False / None switches it off.  The accumulation goes on."""
        if not on:
            self._call("set_auto_exposure", None)
            return
        p = meter_params(**params)
        self._call("set_auto_exposure", C.byref(p))

    def measure_exposure(self, **params):
        """crh_measure_exposure: one synchronous metering of the image read_ldr would show; dict(hist (256,) uint32, n_unsampled, n_lit, exposure,
        white_point, white_bin).  Changes nothing: hand exposure and white_point to set_display to apply them."""
        p, r = meter_params(**params), abi.crh_meter_result()
        self._call("measure_exposure", C.byref(p), C.byref(r))
        return {"hist": np.frombuffer(r, np.uint32, 256).copy(), "n_unsampled": int(r.n_unsampled), "n_lit": int(r.n_lit),
                "exposure": np.float32(r.exposure), "white_point": np.float32(r.white_point), "white_bin": int(r.white_bin)}

    def stats(self):
        s = abi.crh_stats()
        self._call("get_stats", C.byref(s))
        return s.as_dict()

    # -- picking, hover, selection (crh_pick.cpp) ------------------------------------------
    def camera_rays(self, xy):
        """crh_camera_rays: the pixel-centre primary rays of the (x, y) pixels, (n, 8) float32 in trace_nearest's layout"""
        xy = np.ascontiguousarray(xy, np.uint32).reshape(-1, 2)
        out = np.empty((len(xy), 8), np.float32)
        self._call("camera_rays", xy.ctypes.data_as(_u32p), C.c_uint32(len(xy)), _fp(out))
        return out

    def pick(self, x, y):
        """crh_pick == MoveTo + PickedData: dict(object, triangle, t, depth, u, v, point) under pixel (x, y); object -1 = nothing"""
        r = abi.crh_pick_result()
        self._call("pick", C.c_uint32(int(x)), C.c_uint32(int(y)), C.byref(r))
        return r.as_dict()

    def read_ids(self):
        """crh_read_ids: (object int32, triangle int32, t float32), each (H, W)"""
        ob, tr = np.empty((self.height, self.width), np.int32), np.empty((self.height, self.width), np.int32)
        t = np.empty((self.height, self.width), np.float32)
        self._call("read_ids", ob.ctypes.data_as(_i32p), tr.ctypes.data_as(_i32p), _fp(t))
        return ob, tr, t

    def set_selection(self, selected, rgb=(255, 160, 0), alpha=64):
        """crh_set_selection: one flag per object (None = nothing selected), outline colour, interior alpha 0..255; only read_ldr shows it"""
        if selected is None:
            self._call("set_selection", None, C.c_uint32(0), None, C.c_uint32(0))
            return
        f = np.ascontiguousarray(np.asarray(selected) != 0, np.uint8)
        col = (C.c_uint8 * 3)(*[int(v) for v in rgb])
        self._call("set_selection", f.ctypes.data_as(_u8p), C.c_uint32(len(f)), col, C.c_uint32(int(alpha)))

    def set_hover(self, obj, rgb=(0, 255, 255), alpha=32):
        """crh_set_hover: the object under the cursor (-1 / None = none)"""
        col = (C.c_uint8 * 3)(*[int(v) for v in rgb])
        self._call("set_hover", C.c_int32(-1 if obj is None else int(obj)), col, C.c_uint32(int(alpha)))

    def selection_bounds(self):
        """crh_get_selection_bounds: (lo, hi) world-space box of the selected objects under the current transforms"""
        lo, hi = np.empty(3, np.float32), np.empty(3, np.float32)
        self._call("get_selection_bounds", _fp(lo), _fp(hi))
        return lo, hi

    # -- fitting the view (crh_fit.cpp) ----------------------------------------------------
    def fit_view(self, n_objects, chosen=None, margin=0.01, cam=None, want_extents=False):
        """crh_fit_view == FitAll + ZFitAll (AppViewer.cxx:704, 764-767, 788, 886): the camera that frames the chosen objects (flags; None = every displayed
        object) seen with `cam` (None = the camera in force), on the device.  Sets nothing.  Returns (camera fields as a dict for scenes.Camera /
        dataclasses.replace, result dict); with want_extents the result carries "object_extents", (n_objects, 6) float32."""
        f = None if chosen is None else np.ascontiguousarray(np.asarray(chosen) != 0, np.uint8)
        n = int(n_objects) if f is None else len(f)
        out, res = abi.crh_camera(), abi.crh_fit_result()
        ext = np.empty((n, 6), np.float32) if want_extents else None
        self._call("fit_view", None if cam is None else C.byref(camera_struct(cam)), None if f is None else f.ctypes.data_as(_u8p), C.c_uint32(n),
                   C.c_float(float(margin)), C.byref(out), C.byref(res), _fp(ext))
        r = res.as_dict()
        if want_extents:
            r["object_extents"] = ext
        return camera_fields(out), r

    # -- region queries on the id buffer (crh_region.cpp) ----------------------------------
    def query_region(self, n_objects, rect=None, poly=None):
        """crh_query_region: the records of every object and of the background (last) for the region rect (x0, y0, x1, y1 half-open; None = whole frame) cut by
        the polygon poly ((n, 2) pixel-corner vertices, even-odd; None = none): a numpy record array of n_objects + 1 entries (abi.REGION_STATS_DTYPE).  Sets nothing."""
        out = np.zeros(int(n_objects) + 1, abi.REGION_STATS_DTYPE)
        r, q, n, _keep = region_args(rect, poly)
        self._call("query_region", r, q, n, out.ctypes.data_as(C.POINTER(abi.crh_region_stats)), C.c_uint32(int(n_objects)))
        return out

    # -- feature lines on the LDR read-out (crh_outline.cpp) -------------------------------
    def set_outline(self, on=True, **params):
        """crh_set_outline: every LDR read-out draws object / depth / crease lines from the id buffer (fields of crh_outline_params by name, the others take
        crh_outline_defaults); on=False / None switches them off.  Display state: the accumulation goes on."""
        if not on:
            self._call("set_outline", None)
            return
        p = outline_params(**params)
        self._call("set_outline", C.byref(p))

    def get_outline(self):
        """crh_get_outline: dict(kinds, crease_cos, depth_ratio, width, rgb, alpha, on) as in force (the defaults while the feature is off)"""
        p, on = abi.crh_outline_params(), C.c_int(0)
        self._call("get_outline", C.byref(p), C.byref(on))
        return {"kinds": int(p.kinds), "crease_cos": np.float32(p.crease_cos), "depth_ratio": np.float32(p.depth_ratio), "width": int(p.width),
                "rgb": tuple(int(x) for x in p.rgb), "alpha": int(p.alpha), "on": bool(on.value)}

    def read_outline(self):
        """crh_read_outline: (H, W) uint8, per pixel the OR of abi.OUTLINE_OBJECT / _DEPTH / _CREASE, all three whatever `kinds` draws"""
        out = np.empty((self.height, self.width), np.uint8)
        self._call("read_outline", out.ctypes.data_as(_u8p))
        return out

    # -- denoised display in front of the LDR read-outs' tone map (crh_denoise.cpp) -----------
    def set_denoise(self, on=True, **params):
        """crh_set_denoise: every LDR read-out tone-maps the id-guided a-trous filter of the accumulator (fields of crh_denoise_params by name, the others take
        crh_denoise_defaults); on=False / None switches it off.  Display state: the accumulation goes on, and nothing but the LDR bytes changes."""
        if not on:
            self._call("set_denoise", None)
            return
        p = denoise_params(**params)
        self._call("set_denoise", C.byref(p))

    def get_denoise(self):
        """crh_get_denoise: dict(levels, normal_cos, depth_ratio, until_samples, on) as in force (the defaults while the feature is off)"""
        p, on = abi.crh_denoise_params(), C.c_int(0)
        self._call("get_denoise", C.byref(p), C.byref(on))
        return {"levels": int(p.levels), "normal_cos": np.float32(p.normal_cos), "depth_ratio": np.float32(p.depth_ratio), "until_samples": int(p.until_samples),
                "on": bool(on.value)}

    def read_denoised(self):
        """crh_read_denoised: (H, W, 4) float32 (r, g, b, w), the image the tone map of a read_ldr issued now would read (the defaults while the feature is off)"""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._call("read_denoised", _fp(out))
        return out

    def bench_denoise(self, repeats=20):
        """crh_bench_denoise: dict(guide_ms, pass_ms) -- device time per launch of the guide kernel and of every pass of the parameters in force (HIP events)"""
        g, p = C.c_float(0), (C.c_float * 5)()
        self._call("bench_denoise", C.c_uint32(int(repeats)), C.byref(g), p)
        return {"guide_ms": float(g.value), "pass_ms": [float(x) for x in p]}

    # -- shade guide of the denoised display: albedo demodulation, lights in view (crh_shade_guide.cpp) --
    def set_shade_guide(self, on=True, **params):
        """crh_set_shade_guide: the denoise filter works on the image divided by the first hit's albedo and leaves the pixels that show a positional light alone
        (fields of crh_shade_guide_params by name, the others take crh_shade_guide_defaults); on=False / None switches it off.  Display state; it shows only while
        the denoise filter is on, or through read_denoised."""
        if not on:
            self._call("set_shade_guide", None)
            return
        p = shade_guide_params(**params)
        self._call("set_shade_guide", C.byref(p))

    def get_shade_guide(self):
        """crh_get_shade_guide: dict(demodulate, lights, albedo_floor, light_dilate, on) as in force (the defaults while the feature is off)"""
        p, on = abi.crh_shade_guide_params(), C.c_int(0)
        self._call("get_shade_guide", C.byref(p), C.byref(on))
        return {"demodulate": int(p.demodulate), "lights": int(p.lights), "albedo_floor": np.float32(p.albedo_floor), "light_dilate": int(p.light_dilate),
                "on": bool(on.value)}

    def read_shade_guide(self):
        """crh_read_shade_guide: (H, W, 4) float32 {1 / albedo rgb, light flag} with the parameters in force (the defaults while the feature is off)"""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._call("read_shade_guide", _fp(out))
        return out

    def read_hit_uv(self):
        """crh_read_hit_uv: (H, W, 2) float32, the barycentric coordinates of the id buffer's hits (what read_ids leaves out)"""
        out = np.empty((self.height, self.width, 2), np.float32)
        self._call("read_hit_uv", _fp(out))
        return out

    def bench_shade_guide(self, repeats=20):
        """crh_bench_shade_guide: dict(guide_ms, pass_ms) -- device time per launch of the plane's kernels and of every guided pass of the filter parameters in force"""
        g, p = C.c_float(0), (C.c_float * 5)()
        self._call("bench_shade_guide", C.c_uint32(int(repeats)), C.byref(g), p)
        return {"guide_ms": float(g.value), "pass_ms": [float(x) for x in p]}

    # -- reprojected display history in front of the denoise filter (crh_reproject.cpp) ------
    def set_reproject(self, on=True, **params):
        """crh_set_reproject: set_camera keeps what the ending view displayed, and every LDR read-out of the next view blends it in through the first-hit points
        (fields of crh_reproject_params by name, the others take crh_reproject_defaults); on=False / None switches it off and drops the history.  Display state."""
        if not on:
            self._call("set_reproject", None)
            return
        p = reproject_params(**params)
        self._call("set_reproject", C.byref(p))

    def get_reproject(self):
        """crh_get_reproject: dict(max_history, until_samples, normal_cos, depth_ratio, on, history_valid) as in force (the defaults while the feature is off)"""
        p, on, valid = abi.crh_reproject_params(), C.c_int(0), C.c_int(0)
        self._call("get_reproject", C.byref(p), C.byref(on), C.byref(valid))
        return {"max_history": np.float32(p.max_history), "until_samples": int(p.until_samples), "normal_cos": np.float32(p.normal_cos),
                "depth_ratio": np.float32(p.depth_ratio), "on": bool(on.value), "history_valid": bool(valid.value)}

    def read_reprojected(self):
        """crh_read_reprojected: (H, W, 4) float32 (r, g, b, w), the image the denoise filter / the tone map of a read_ldr issued now would receive"""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._call("read_reprojected", _fp(out))
        return out

    def bench_reproject(self, repeats=20):
        """crh_bench_reproject: dict(resolve_ms, capture_ms) -- device time per launch of a read-out's resolve kernel and of what a capture enqueues (HIP events)"""
        r, k = C.c_float(0), C.c_float(0)
        self._call("bench_reproject", C.c_uint32(int(repeats)), C.byref(r), C.byref(k))
        return {"resolve_ms": float(r.value), "capture_ms": float(k.value)}

    def set_reproject_motion(self, on=True, **params):
        """crh_set_reproject_motion: with set_reproject on as well, set_transforms captures and keeps the history, and a moved object's history follows it (fields of
        crh_reproject_motion_params by name, the others take crh_reproject_motion_defaults); on=False / None switches it off.  Display state."""
        if not on:
            self._call("set_reproject_motion", None)
            return
        p = reproject_motion_params(**params)
        self._call("set_reproject_motion", C.byref(p))

    def get_reproject_motion(self):
        """crh_get_reproject_motion: dict(max_history_moved, max_history_static, on, n_flagged) as in force (the defaults while the feature is off)"""
        p, on, n = abi.crh_reproject_motion_params(), C.c_int(0), C.c_uint32(0)
        self._call("get_reproject_motion", C.byref(p), C.byref(on), C.byref(n))
        return {"max_history_moved": np.float32(p.max_history_moved), "max_history_static": np.float32(p.max_history_static), "on": bool(on.value), "n_flagged": int(n.value)}

    def get_reproject_launches(self):
        """crh_get_reproject_launches: dict(plain, motion) -- launches of k_reproject_resolve / k_reproject_resolve_motion by read-outs and captures so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._call("get_reproject_launches", C.byref(a), C.byref(b))
        return {"plain": int(a.value), "motion": int(b.value)}

    def bench_reproject_motion(self, repeats=20):
        """crh_bench_reproject_motion: dict(resolve_ms) -- device time per launch of k_reproject_resolve_motion with the table in force (or the all-flagged stand-in)"""
        r = C.c_float(0)
        self._call("bench_reproject_motion", C.c_uint32(int(repeats)), C.byref(r))
        return {"resolve_ms": float(r.value)}

    # -- kernel-level --------------------------------------------------------------------
    def trace_nearest(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.empty((len(rays), 4), np.float32)
        self._call("trace_nearest", _fp(rays), C.c_uint32(len(rays)), _fp(out))
        return out

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.empty(len(rays), np.uint32)
        self._call("trace_any", _fp(rays), C.c_uint32(len(rays)), out.ctypes.data_as(_u32p))
        return out

    def get_bvh(self):
        nn, nt = C.c_uint32(0), C.c_uint32(0)
        self._call("get_bvh", None, C.byref(nn), None, C.byref(nt))
        nodes = np.empty((nn.value, abi.NODE_DWORDS), np.float32)      # 64-B stride nodes (include/crh_bvh_format.h)
        tris = np.empty((nt.value, 12), np.float32)
        self._call("get_bvh", _fp(nodes), C.byref(nn), _fp(tris), C.byref(nt))
        return nodes, tris
