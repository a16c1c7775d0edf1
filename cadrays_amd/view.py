"""Host-side mirror of the rendering boundary CADRays drives (reference file:line in brackets).

    view = View(device=0)                       # new OpenGl_GraphicDriver + V3d_Viewer + CreateView   [AppViewer.cxx:601-638]
    view.load_scene(scene)                      # AIS Display + SetBSDF + lights + env + camera          [AisMesh.cxx:357-423, MaterialEditor.cxx:331-337]
    view.ChangeRenderingParams(max_depth=5)     # Graphic3d_RenderingParams field writes                 [SettingsWidget.cxx:263-477]
    view.Redraw()                               # +1 sample per pixel                                    [AppViewer.cxx:1047]
    img = view.BufferDump(BT_RGB_RayTraceHdrLeft)   # linear HDR read-back                               [AppGui.cxx:345-349]

Everything below the method names is libcadrays_hip.so (hand-written gfx950 kernels) through ctypes.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import abi
from ._lib import load_library
from .binding import Backend, BackendError

BT_RGB = "Graphic3d_BT_RGB"                             # AppViewer.cxx:1259-1261
BT_RGB_RayTraceHdrLeft = "Graphic3d_BT_RGB_RayTraceHdrLeft"   # AppGui.cxx:349


class View(Backend):
    def __init__(self, device=0):
        super().__init__(load_library(), "crh_", (C.c_int(int(device)),))
        self.device = int(device)
        self._params = None
        self._camera, self._n_objects, self._selected, self._visible = None, 1, set(), None
        self.selection_rgb, self.selection_alpha, self.hover_rgb, self.hover_alpha = (255, 160, 0), 64, (0, 255, 255), 32
        import os
        from . import pipeline_capacity
        frames, _ = pipeline_capacity()
        if frames > 3 and "CRH_PIPE_DEPTH" not in os.environ:      # the process has the hardware queues for a deeper frame pipeline (crh_query_pipeline_capacity)
            self.set_pipeline_depth(frames)

    # ---- V3d_View vocabulary ----------------------------------------------------------------
    def Redraw(self):
        """One progressive iteration: +1 spp over the whole target (AppViewer.cxx:1047)."""
        self.render(1)

    def BufferDump(self, buffer_type=BT_RGB):
        if buffer_type == BT_RGB_RayTraceHdrLeft:
            return self.read_hdr()
        if buffer_type == BT_RGB:
            return self.read_ldr()
        raise ValueError(buffer_type)

    def set_params(self, p):
        self._params = dataclasses.replace(p)
        super().set_params(p)

    def ChangeRenderingParams(self, **fields):
        """Write Graphic3d_RenderingParams fields; like OCCT, any change restarts accumulation."""
        if self._params is None:
            raise RuntimeError("set_params / load_scene first")
        self.set_params(dataclasses.replace(self._params, **fields))

    # ---- AIS_InteractiveContext vocabulary: hover, selection, autofocus (crh_pick.cpp) ---------------
    def set_geometry(self, pos, nrm, tri, uv=None, tri_object=None, obj_xform=None):
        super().set_geometry(pos, nrm, tri, uv, tri_object, obj_xform)
        self._n_objects = 1 if tri_object is None else len(np.asarray(obj_xform, np.float32).reshape(-1, 12))
        self._selected, self._visible = set(), None          # a new scene: nothing selected, everything displayed

    def add_object(self, pos, nrm, tri, xform, uv=None):
        ob = super().add_object(pos, nrm, tri, xform, uv)
        self._n_objects = ob + 1
        if self._visible is not None:
            self._visible = np.append(self._visible, np.uint8(1))
        return ob

    def set_visibility(self, visible):
        super().set_visibility(visible)
        self._visible = np.ascontiguousarray(np.asarray(visible) != 0, np.uint8)

    def set_camera(self, cam):
        self._camera = dataclasses.replace(cam)
        super().set_camera(cam)

    def _push_selection(self):
        flags = np.zeros(self._n_objects, np.uint8)
        flags[sorted(self._selected)] = 1
        self.set_selection(flags if self._selected else None, self.selection_rgb, self.selection_alpha)

    def MoveTo(self, x, y):
        """AIS_InteractiveContext::MoveTo (AppViewer.cxx:347): the object under the cursor becomes the hovered one; returns it (-1: none)"""
        ob = self.pick(x, y)["object"]
        self.set_hover(ob, self.hover_rgb, self.hover_alpha)
        return ob

    def Select(self, x, y, shift=False):
        """Select / ShiftSelect (AppViewer.cxx:359-455): a click replaces the selection by the object under the cursor (nothing there: clears it),
        a shift-click toggles that object; returns the selected set"""
        ob = self.pick(x, y)["object"]
        if shift:
            if ob >= 0:
                self._selected ^= {ob}
        else:
            self._selected = {ob} if ob >= 0 else set()
        self._push_selection()
        return set(self._selected)

    def HideSelected(self):
        """"Hide selected" (AppViewer.cxx:1149-1153): erase the selected objects (set_visibility) and drop the selection"""
        if not self._selected:
            return
        if self._n_objects == 1 and not getattr(self, "_has_objects", False):
            raise RuntimeError("HideSelected needs a scene handed over with objects")
        vis = np.ones(self._n_objects, np.uint8) if self._visible is None else self._visible.copy()
        vis[sorted(self._selected)] = 0
        self._selected = set()
        self._push_selection()
        self.set_hover(-1)
        self.set_visibility(vis)

    def autofocus(self, x, y):
        """autofocus (AppGui.cxx:78-94): CameraFocalPlaneDist = depth of what lies under the pixel; like every camera change it restarts the
        accumulation.  Nothing under the pixel: nothing changes.  Returns the new focal distance or None."""
        r = self.pick(x, y)
        if r["object"] < 0:
            return None
        self.set_camera(dataclasses.replace(self._camera, focal_dist=float(r["depth"])))
        self.reset()
        return float(r["depth"])

    # ---- rubber band, lasso, visible objects (crh_region.cpp; OCCT: AIS_InteractiveContext::Select(xmin, ymin, xmax, ymax, view) and its polyline form) ----
    def _select_region(self, stats, mode, min_pixels, shift):
        hit = set(int(o) for o in np.flatnonzero(region_select(stats, mode, min_pixels)))
        self._selected = (self._selected ^ hit) if shift else hit
        self._push_selection()
        return set(self._selected)

    def SelectRect(self, x0, y0, x1, y1, mode=abi.REGION_TOUCHED, min_pixels=1, shift=False):
        """rubber-band selection over the pixels [x0, x1) x [y0, y1): the objects with at least min_pixels visible pixels inside (abi.REGION_TOUCHED), or those
        whose visible pixels all lie inside (abi.REGION_ENCLOSED), replace the selection; shift toggles them instead (ShiftSelect); returns the selected set.
        Selection is by visible surface: an object wholly hidden behind others is never selected."""
        return self._select_region(self.query_region(self._n_objects, (x0, y0, x1, y1)), mode, min_pixels, shift)

    def SelectLasso(self, points, mode=abi.REGION_TOUCHED, min_pixels=1, shift=False):
        """the same over a polygon of 3 .. 256 pixel-corner vertices (x, y), even-odd"""
        return self._select_region(self.query_region(self._n_objects, None, points), mode, min_pixels, shift)

    def VisibleObjects(self, min_pixels=1):
        """{object: record} of the objects with at least min_pixels (>= 1) visible pixels in the frame: a dict of pixels_frame, the screen box (x0, y0, x1, y1,
        half-open) and the depth range (t_min, t_max) of what is visible of each"""
        st = self.query_region(self._n_objects)
        return {int(o): {n: st[n][o].item() for n in st.dtype.names} for o in np.flatnonzero(st["pixels_frame"][:-1] >= max(int(min_pixels), 1))}

    # ---- feature lines, "shaded with edges" (crh_outline.cpp; no counterpart in the reference's path tracer, DataNode.cxx:286 sets a display mode of the rasteriser) ----
    def SetOutline(self, kinds=abi.OUTLINE_ALL, crease_deg=30.0, depth_rel=0.02, width=1, rgb=(0, 0, 0), alpha=255):
        """lines along object boundaries, depth steps (first-hit distance larger by more than depth_rel, relative) and creases (planes meeting at more than
        crease_deg) over every LDR read-out from now on; nothing restarts.  The angle and the step become crease_cos / depth_ratio in double, rounded once."""
        self.set_outline(True, kinds=int(kinds), crease_cos=outline_crease_cos(crease_deg), depth_ratio=outline_depth_ratio(depth_rel), width=int(width),
                         rgb=tuple(int(x) for x in rgb), alpha=int(alpha))

    def ClearOutline(self):
        """no lines: the LDR bytes of a view that never called SetOutline"""
        self.set_outline(False)

    def ReadOutline(self):
        """(H, W) uint8 mask of the lines' pixels: abi.OUTLINE_OBJECT | _DEPTH | _CREASE per pixel, with the thresholds in force (the defaults while off)"""
        return self.read_outline()

    # ---- denoised display (crh_denoise.cpp; no counterpart in the reference: OCCT's path tracer shows the raw accumulation) ----
    def SetDenoise(self, levels=4, normal_deg=25.0, depth_rel=0.05, until_samples=256):
        """an id-guided a-trous filter in front of the tone map of every LDR read-out from now on: taps mix within an object, across triangles whose planes meet at
        less than normal_deg and whose first-hit distances differ by at most depth_rel (relative); level k works on a pixel while samples * 4^k < until_samples.
        Nothing restarts.  The angle and the step become normal_cos / depth_ratio in double, rounded once."""
        self.set_denoise(True, levels=int(levels), normal_cos=outline_crease_cos(normal_deg), depth_ratio=outline_depth_ratio(depth_rel), until_samples=int(until_samples))

    def ClearDenoise(self):
        """the raw accumulation: the LDR bytes of a view that never called SetDenoise"""
        self.set_denoise(False)

    def ReadDenoised(self):
        """(H, W, 4) float32: the image the tone map of an LDR read-out issued now would read, with the parameters in force (the defaults while off)"""
        return self.read_denoised()

    # ---- shade guide of the denoised display (crh_shade_guide.cpp; no counterpart in the reference: OCCT's path tracer shows the raw accumulation) ----
    def SetShadeGuide(self, demodulate=True, lights=True, albedo_floor=1.0 / 64.0, light_dilate=1):
        """the denoise filter from now on smooths the image divided by the first hit's albedo (textures and material borders survive) and leaves the disc of a
        positional light in view alone, grown by light_dilate pixels.  Nothing restarts; it shows while SetDenoise is on."""
        self.set_shade_guide(True, demodulate=int(bool(demodulate)), lights=int(bool(lights)), albedo_floor=float(albedo_floor), light_dilate=int(light_dilate))

    def ClearShadeGuide(self):
        """the filter as it is without the guide: the LDR bytes of a view that never called SetShadeGuide"""
        self.set_shade_guide(False)

    def ReadShadeGuide(self):
        """(H, W, 4) float32: per pixel 1 / albedo (rgb) and the light flag, with the parameters in force (the defaults while off)"""
        return self.read_shade_guide()

    # ---- reprojected display history (crh_reproject.cpp; no counterpart in the reference: OCCT's path tracer shows the raw accumulation) ----
    def SetReproject(self, max_history=16.0, until_samples=64, normal_deg=25.0, depth_rel=0.05):
        """keep the picture through a camera move: set_camera + reset from now on carry what the ending view displayed over to the next one, blended in with weight up
        to max_history samples until a pixel has until_samples of its own.  Nothing restarts.  The angle and the step become normal_cos / depth_ratio in double,
        rounded once."""
        self.set_reproject(True, max_history=float(max_history), until_samples=int(until_samples), normal_cos=outline_crease_cos(normal_deg),
                           depth_ratio=outline_depth_ratio(depth_rel))

    def ClearReproject(self):
        """no history: the LDR bytes of a view that never called SetReproject"""
        self.set_reproject(False)

    def ReadReprojected(self):
        """(H, W, 4) float32: the image the denoise filter / the tone map of an LDR read-out issued now would receive"""
        return self.read_reprojected()

    def SetReprojectMotion(self, max_history_moved=16.0, max_history_static=8.0):
        """keep the picture through an object drag as well: with SetReproject on, set_transforms from now on captures what the ending placement displayed and a moved
        object's history follows it; the two caps bound the history's weight on the moved object's pixels and -- while any object is off its captured placement --
        on all the others (their geometry is unchanged, their lighting is not).  Nothing restarts."""
        self.set_reproject_motion(True, max_history_moved=float(max_history_moved), max_history_static=float(max_history_static))

    def ClearReprojectMotion(self):
        """set_transforms drops the history again, as in a view that never called SetReprojectMotion"""
        self.set_reproject_motion(False)

    # ---- annotations: world-space segments over the display, depth-tested (crh_annotate.cpp; the reference paints its helpers with ImGui, ImRaytraceControls.cxx:64, :93-111) ----
    def SetAnnotations(self, segments, depth_bias=abi.ANNOT_DEFAULTS["depth_bias"], hidden_alpha=abi.ANNOT_DEFAULTS["hidden_alpha"]):
        """draw this list (a record array of abi.ANNOT_SEGMENT_DTYPE: cadrays_amd.annotations builds them) over every LDR read-out from now on, each segment hidden,
        dimmed or left on top where the scene is nearer; nothing restarts.  An empty list switches the feature off."""
        sg = _annot_list(segments)
        p = abi.crh_annot_params(float(depth_bias), int(hidden_alpha))
        self._call("set_annotations", sg.ctypes.data_as(C.POINTER(abi.crh_annot_segment)) if len(sg) else None, C.c_uint32(len(sg)), C.byref(p))

    def ClearAnnotations(self):
        """no annotations: the LDR bytes of a view that never called SetAnnotations"""
        self._call("set_annotations", None, C.c_uint32(0), None)

    def GetAnnotations(self):
        """dict(segments, depth_bias, hidden_alpha, on): the list and the parameters in force (the defaults while the feature is off)"""
        n, on, p = C.c_uint32(0), C.c_int(0), abi.crh_annot_params()
        self._call("get_annotations", None, C.c_uint32(0), C.byref(n), C.byref(p), C.byref(on))
        sg = np.zeros(n.value, abi.ANNOT_SEGMENT_DTYPE)
        self._call("get_annotations", sg.ctypes.data_as(C.POINTER(abi.crh_annot_segment)) if len(sg) else None, C.c_uint32(len(sg)), None, None, None)
        return {"segments": sg, "depth_bias": np.float32(p.depth_bias), "hidden_alpha": int(p.hidden_alpha), "on": bool(on.value)}

    def ReadAnnotationIds(self):
        """(H, W) int32: per pixel the index of the last segment that drew there (an x-ray pixel counts), or -1"""
        out = np.empty((self.height, self.width), np.int32)
        self._call("read_annotation_ids", out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def PickAnnotation(self, x, y):
        """the hit test for a handle: (segment index or -1, the parameter s along that segment's clipped screen record at the pixel)"""
        seg, s = C.c_int32(-1), C.c_float(0.0)
        self._call("pick_annotation", C.c_uint32(int(x)), C.c_uint32(int(y)), C.byref(seg), C.byref(s))
        return int(seg.value), np.float32(s.value)

    def ReadAnnotationRecords(self):
        """the projected records as the device computed them for the camera in force: a record array of abi.ANNOT_RECORD_DTYPE, one per segment"""
        n = C.c_uint32(0)
        self._call("get_annotations", None, C.c_uint32(0), C.byref(n), None, None)
        out = np.zeros(n.value, abi.ANNOT_RECORD_DTYPE)
        self._call("read_annotation_records", out.ctypes.data_as(C.c_void_p) if len(out) else None)
        return out

    def BenchAnnotations(self, repeats=20):
        """crh_bench_annotations: dict(project_ms, bin_ms, draw_ms), device time per launch of the three kernels for the list in force"""
        a, b, d = C.c_float(0), C.c_float(0), C.c_float(0)
        self._call("bench_annotations", C.c_uint32(int(repeats)), C.byref(a), C.byref(b), C.byref(d))
        return {"project_ms": a.value, "bin_ms": b.value, "draw_ms": d.value}

    def ShowSelectionBox(self, extra=None, **style):
        """the bounding box of the selection (crh_get_selection_bounds: the manipulator's pivot box, AppViewer.cxx:863-875) as the annotation list, in front of the
        segments of `extra`; nothing selected: `extra` alone (an empty list switches the feature off).  Returns the list that was set."""
        from . import annotations
        parts = [] if extra is None else [_annot_list(extra)]
        if self._selected:
            lo, hi = self.selection_bounds()
            parts.insert(0, annotations.box(lo, hi, **style))
        sg = annotations.join(*parts)
        self.SetAnnotations(sg)
        return sg

    # ---- V3d_View::FitAll / ZFitAll (crh_fit.cpp) --------------------------------------------------
    def _fit(self, chosen, margin):
        fields, r = self.fit_view(self._n_objects, chosen, margin)
        self.set_camera(dataclasses.replace(self._camera, **fields))
        self.reset()
        return r

    def FitAll(self, margin=0.01):
        """View->FitAll() + ZFitAll() (AppViewer.cxx:704, 764-767, 788, 886): frame every displayed object tightly (margin: OCCT's default); sets the fitted
        camera and, like every camera change, restarts the accumulation.  Returns the result dict (z_near / z_far: the depth range)."""
        return self._fit(None, margin)

    def FitSelected(self, margin=0.01):
        """the same over the selected objects"""
        if not self._selected:
            raise BackendError("FitSelected: nothing is selected")
        flags = np.zeros(self._n_objects, np.uint8)
        flags[sorted(self._selected)] = 1
        return self._fit(flags, margin)

    # ---- display state (SettingsWidget.cxx:343-404): the sliders re-tone the accumulated image, nothing restarts ----
    def set_display(self, tonemap_mode, exposure, white_point):
        super().set_display(tonemap_mode, exposure, white_point)
        if self._params is not None:      # ChangeRenderingParams builds on these: a later restart keeps what the sliders show
            self._params = dataclasses.replace(self._params, tonemap_mode=int(tonemap_mode), exposure=float(exposure), white_point=float(white_point))

    def AutoExpose(self, **params):
        """meter the image once (measure_exposure) and apply the result (set_display); returns the measurement"""
        m = self.measure_exposure(**params)
        self.set_display(self.get_display()["tonemap_mode"], float(m["exposure"]), float(m["white_point"]))
        return m

    # ---- device-side extras -----------------------------------------------------------------
    def sync(self):
        self._call("sync")

    def set_lookahead(self, frames):
        """trace `frames` Redraw()s ahead in one wide batch; images after every Redraw stay bit-identical"""
        self._call("set_lookahead", C.c_uint32(int(frames)))

    def set_lookahead_auto(self, max_frames):
        """crh_set_lookahead_auto: one sample right after a restart, then batches of 4, 16, ... max_frames; 0 / 1 = off"""
        self._call("set_lookahead_auto", C.c_uint32(int(max_frames)))

    def set_pipeline_depth(self, frames):
        """crh_set_pipeline_depth: frames in flight of free-running Redraw()s, 2 .. cadrays_amd.pipeline_capacity()[0] (3 on the runtime's default four hardware queues)"""
        self._call("set_pipeline_depth", C.c_uint32(int(frames)))

    def set_path_budget(self, max_paths):
        """crh_set_path_budget: at most this many path slots (196 B each) in flight per batch; images do not depend on it"""
        self._call("set_path_budget", C.c_uint64(int(max_paths)))

    def get_path_budget(self):
        n = C.c_uint64(0)
        self._call("get_path_budget", C.byref(n))
        return int(n.value)

    def frame_tuning(self):
        """crh_get_frame_tuning: the frame kernel's feeder count chosen by measurement after every build (no image depends on it)"""
        out = (C.c_uint32 * 5)()
        self._call("get_frame_tuning", out)
        return {"enabled": bool(out[0]), "feeders": int(out[1]), "frames_measured": int(out[2]), "mean_us_3_feeders": int(out[3]), "mean_us_4_feeders": int(out[4])}

    def tile_order(self):
        """crh_get_tile_order: the order crh_render lists the tiles in (no pixel depends on it), and how often it has been replaced"""
        n, r = C.c_uint32(0), (C.c_uint64 * 7)()
        self._call("get_tile_order", None, C.byref(n), r)
        order = np.zeros(n.value, np.uint32)
        self._call("get_tile_order", order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), r)
        self.tile_order_calls = {"sorted": int(r[1]), "row_major": int(r[2]), "frames_collected": int(r[3]), "verdict": int(r[4]), "mean_us_sorted": int(r[5]), "mean_us_row_major": int(r[6])}
        return order, int(r[0])

    def packet_stats(self):
        """camera rays walked as packets since the last restart, and those of them handed to the per-ray fall-back pass (ties at equal distance)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._call("get_packet_stats", C.byref(a), C.byref(b))
        return {"packet_rays": int(a.value), "fallback_rays": int(b.value)}

    def set_schedule(self, mode):
        """crh_set_schedule: abi.SCHEDULE_AUTO / _WIDE (the big-batch schedule bench.py times) / _SMALL; images do not depend on it"""
        self._call("set_schedule", C.c_int(int(mode)))

    def enable_counters(self, on=True):
        self._call("enable_counters", C.c_int(int(on)))

    def enable_kernel_timing(self, on=True):
        self._call("enable_kernel_timing", C.c_int(int(on)))

    def kernel_timing(self):
        ms, n, allms = C.c_double(0), C.c_uint64(0), C.c_double(0)
        self._call("get_kernel_timing", C.byref(ms), C.byref(n), C.byref(allms))
        return {"trace_nearest_ms_total": ms.value, "trace_nearest_launches": n.value, "render_ms_total": allms.value}

    def save_accum(self):
        """checkpoint: (H, W, 4) float32 accumulator (rgb mean + sample count) and the iteration counter"""
        out = np.empty((self.height, self.width, 4), np.float32)
        n = C.c_uint32(0)
        self._call("save_accum", out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n))
        return out, n.value

    def load_accum(self, rgba, frames_done):
        rgba = np.ascontiguousarray(rgba, np.float32)
        assert rgba.shape == (self.height, self.width, 4)
        self._call("load_accum", rgba.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(int(frames_done)))

    def scene_bytes(self):
        """HBM residency of the built scene: 64-B-stride nodes, 64-B-stride triangle records, 64-B shading records -- and, for a scene without placed
        objects, the 128-B packet nodes the camera rays of wide batches read (kernels.hip k_expand_packet_nodes; not part of what the per-ray walk touches)"""
        nn, nt = C.c_uint32(0), C.c_uint32(0)
        self._call("get_bvh", None, C.byref(nn), None, C.byref(nt))
        two_level = getattr(self, "_has_objects", False)
        return {"nodes": 4 * abi.NODE_DWORDS * nn.value, "triangles": 64 * nt.value, "shading": 64 * nt.value,
                "packet_nodes": 0 if two_level else 128 * nn.value, "n_nodes": nn.value, "n_triangles": nt.value}

    def accum_device_ptr(self):
        p, n = C.c_void_p(0), C.c_uint64(0)
        self._call("accum_device_ptr", C.byref(p), C.byref(n))
        return p.value, n.value

    @staticmethod
    def reduce(views, root=0, fake_devices=False):
        """crh_reduce: assemble the tile-sharded frame of `views` (one context per GPU) on views[root]; that view's
        read_hdr / read_ldr / save_accum return the assembled frame until it renders again.  fake_devices: the test hook
        crh_debug_reduce_fake_devices (the RCCL branch on contexts that share a device)"""
        lib = views[root]._lib
        arr = (C.c_void_p * len(views))(*[v._ctx.value for v in views])
        fn = lib.crh_debug_reduce_fake_devices if fake_devices else lib.crh_reduce
        fn.restype = C.c_int
        rc = fn(arr, C.c_uint32(len(views)), C.c_uint32(int(root)))
        if rc != 0:
            msg = views[root]._fn("last_error")(views[root]._ctx)
            raise BackendError(f"crh_reduce -> {rc}: {msg.decode() if msg else ''}")

    def bench_trace(self, rays, any_hit=False, repeat=10):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        ms = C.c_float(0)
        self._call("bench_trace", rays.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(rays)), C.c_int(int(any_hit)),
                   C.c_uint32(repeat), C.byref(ms))
        return ms.value

    def debug_math(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), np.float32)
        out, out2 = np.empty_like(a), np.empty_like(a)
        fp = C.POINTER(C.c_float)
        self._call("debug_math", C.c_int(fn), a.ctypes.data_as(fp), b.ctypes.data_as(fp), out.ctypes.data_as(fp),
                   out2.ctypes.data_as(fp), C.c_uint32(a.size))
        return out, out2


    def debug_bsdf(self, fn, bsdf, a, b=None, two_sided=True):
        """crh_debug_bsdf: fn 0 eval (f cos), 1 pdf, 2 sample, 3 Fresnel of the coat on the device; a, b: (n, 3) float32"""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), np.float32).reshape(-1, 3)
        n = len(a)
        out = np.empty((n, {0: 3, 1: 1, 2: 8, 3: 3}[fn]), np.float32)
        m = bsdf.to_abi()
        fp = C.POINTER(C.c_float)
        self._call("debug_bsdf", C.c_int(fn), C.byref(m), a.ctypes.data_as(fp), b.ctypes.data_as(fp), out.ctypes.data_as(fp),
                   C.c_uint32(n), C.c_int(int(two_sided)))
        return out


def meter_from_histogram(hist, exposure_in=0.0, white_in=1.0, **params):
    """crh_meter_from_histogram on the host only (no GPU): (exposure float32, white_point float32, white_bin) of a (256,) uint32 histogram; exposure_in /
    white_in are the display values in force (the answer when nothing is lit); params as in Backend.set_auto_exposure"""
    from .binding import meter_params
    lib = load_library()
    h = np.ascontiguousarray(hist, np.uint32)
    assert h.shape == (256,)
    p = meter_params(**params)
    e, w, b = C.c_float(0), C.c_float(float(white_in)), C.c_uint32(0)
    rc = lib.crh_meter_from_histogram(h.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p), C.c_float(float(exposure_in)), C.byref(e), C.byref(w), C.byref(b))
    if rc != 0:
        raise BackendError(f"crh_meter_from_histogram -> {rc}")
    return np.float32(e.value), np.float32(w.value), int(b.value)


def fit_extents_host(verts4, n_objects, cam, width, height, margin=0.01, obj_xform=None):
    """crh_fit_extents_host on the host only (no GPU): verts4 (n, 4) float32 {x, y, z, object index as int bits}; returns (extents (n_objects, 6) float32,
    counts (n_objects,) uint32, dict with the frame used: right, up, fwd, kx, ky)"""
    from .binding import camera_struct
    lib = load_library()
    v = np.ascontiguousarray(verts4, np.float32).reshape(-1, 4)
    xf = None if obj_xform is None else np.ascontiguousarray(obj_xform, np.float32).reshape(-1, 12)
    assert xf is None or len(xf) == n_objects
    ext, cnt, res = np.empty((int(n_objects), 6), np.float32), np.empty(int(n_objects), np.uint32), abi.crh_fit_result()
    fp = C.POINTER(C.c_float)
    rc = lib.crh_fit_extents_host(v.ctypes.data_as(fp), C.c_uint32(len(v)), None if xf is None else xf.ctypes.data_as(fp), C.c_uint32(int(n_objects)),
                                  C.byref(camera_struct(cam)), C.c_uint32(int(width)), C.c_uint32(int(height)), C.c_float(float(margin)), ext.ctypes.data_as(fp),
                                  cnt.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(res))
    if rc != 0:
        raise BackendError(f"crh_fit_extents_host -> {rc}")
    r = res.as_dict()
    return ext, cnt, {k: r[k] for k in ("right", "up", "fwd", "kx", "ky")}


def fit_from_extents(extents, cam, width, height, margin=0.01):
    """crh_fit_from_extents on the host only (no GPU): the rule alone; returns (camera fields as a dict, result dict)"""
    from .binding import camera_fields, camera_struct
    lib = load_library()
    e = np.ascontiguousarray(extents, np.float32).reshape(6)
    out, res = abi.crh_camera(), abi.crh_fit_result()
    rc = lib.crh_fit_from_extents(e.ctypes.data_as(C.POINTER(C.c_float)), C.byref(camera_struct(cam)), C.c_uint32(int(width)), C.c_uint32(int(height)),
                                  C.c_float(float(margin)), C.byref(out), C.byref(res))
    if rc != 0:
        raise BackendError(f"crh_fit_from_extents -> {rc}")
    return camera_fields(out), res.as_dict()


def region_stats_host(object_px, t_px, n_objects, rect=None, poly=None):
    """crh_region_stats_host on the host only (no GPU): object_px (H, W) int32 ids (-1: nothing hit), t_px (H, W) float32 first-hit distances; the records as
    Backend.query_region returns them (n_objects + 1, the background last)"""
    from .binding import region_args
    lib = load_library()
    ob, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == t.shape
    out = np.zeros(int(n_objects) + 1, abi.REGION_STATS_DTYPE)
    r, q, n, _keep = region_args(rect, poly)
    rc = lib.crh_region_stats_host(ob.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]), r, q, n,
                                   out.ctypes.data_as(C.POINTER(abi.crh_region_stats)), C.c_uint32(int(n_objects)))
    if rc != 0:
        raise BackendError(f"crh_region_stats_host -> {rc}")
    return out


def region_select(stats, mode=abi.REGION_TOUCHED, min_pixels=1):
    """crh_region_select on the host only: flags (n_objects,) uint8 from the records of query_region / region_stats_host (the background record, last, is not looked at)"""
    lib = load_library()
    st = np.ascontiguousarray(stats, abi.REGION_STATS_DTYPE)
    flags = np.zeros(max(len(st) - 1, 0), np.uint8)
    rc = lib.crh_region_select(st.ctypes.data_as(C.POINTER(abi.crh_region_stats)), C.c_uint32(len(flags)), C.c_int(int(mode)), C.c_uint32(int(min_pixels)),
                               flags.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise BackendError(f"crh_region_select -> {rc}")
    return flags


def outline_crease_cos(crease_deg):
    """the float32 crease_cos of an angle in degrees: the cosine in double, rounded once"""
    import math
    return float(np.float32(math.cos(math.radians(float(crease_deg)))))


def outline_depth_ratio(depth_rel):
    """the float32 depth_ratio of a relative step: 1 + depth_rel in double, rounded once"""
    return float(np.float32(1.0 + float(depth_rel)))


def outline_table_host(pos, tri):
    """crh_outline_table_host on the host only (no GPU): pos (n, 3) float32, tri (m, 4) rows {v0, v1, v2, material} as set_geometry takes them; the per-triangle
    table, a numpy record array of m entries (abi.OUTLINE_TABLE_DTYPE, 32 B each)"""
    lib = load_library()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(np.asarray(tri).astype(np.int64) & 0xFFFFFFFF, np.uint32).reshape(-1, 4)
    out = np.zeros(len(tri), abi.OUTLINE_TABLE_DTYPE)
    rc = lib.crh_outline_table_host(pos.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(pos)), tri.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(len(tri)),
                                    out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise BackendError(f"crh_outline_table_host -> {rc}")
    return out


def outline_mask_host(object_px, triangle_px, t_px, table, crease_cos=abi.OUTLINE_DEFAULTS["crease_cos"], depth_ratio=abi.OUTLINE_DEFAULTS["depth_ratio"]):
    """crh_outline_mask_host on the host only (no GPU): the planes as read_ids returns them, each (H, W); table as outline_table_host returns it (None / empty:
    no triangle is known); the (H, W) uint8 mask as read_outline returns it"""
    lib = load_library()
    ob, tr, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == tr.shape == t.shape
    tb = np.zeros(0, abi.OUTLINE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.OUTLINE_TABLE_DTYPE)
    out = np.zeros(ob.shape, np.uint8)
    rc = lib.crh_outline_mask_host(ob.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float)),
                                   C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]), tb.ctypes.data_as(C.c_void_p) if len(tb) else None, C.c_uint32(len(tb)),
                                   C.c_float(float(crease_cos)), C.c_float(float(depth_ratio)), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise BackendError(f"crh_outline_mask_host -> {rc}")
    return out


def outline_draw_host(mask, ldr, **params):
    """crh_outline_draw_host on the host only (no GPU): the lines of an (H, W) uint8 mask drawn over a copy of the (H, W, 3) uint8 image; params as in
    Backend.set_outline (fields of crh_outline_params)"""
    from .binding import outline_params
    lib = load_library()
    m = np.ascontiguousarray(mask, np.uint8)
    img = np.array(ldr, np.uint8, order="C")
    assert m.ndim == 2 and img.shape == m.shape + (3,)
    p = outline_params(**params)
    rc = lib.crh_outline_draw_host(m.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(m.shape[1]), C.c_uint32(m.shape[0]), C.byref(p), img.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise BackendError(f"crh_outline_draw_host -> {rc}")
    return img


def denoise_host(rgba, object_px, triangle_px, t_px, table, **params):
    """crh_denoise_host on the host only (no GPU): rgba (H, W, 4) float32 as save_accum returns it, the planes as read_ids returns them, table as
    outline_table_host returns it (None / empty: no triangle has a normal); params as in Backend.set_denoise (fields of crh_denoise_params); the (H, W, 4)
    float32 image read_denoised returns"""
    from .binding import denoise_params
    lib = load_library()
    img = np.ascontiguousarray(rgba, np.float32)
    ob, tr, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == tr.shape == t.shape and img.shape == ob.shape + (4,)
    tb = np.zeros(0, abi.OUTLINE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.OUTLINE_TABLE_DTYPE)
    p = denoise_params(**params)
    out = np.zeros(img.shape, np.float32)
    rc = lib.crh_denoise_host(img.ctypes.data_as(C.POINTER(C.c_float)), ob.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_int32)),
                              t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]), tb.ctypes.data_as(C.c_void_p) if len(tb) else None,
                              C.c_uint32(len(tb)), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise BackendError(f"crh_denoise_host -> {rc}")
    return out


def guide_table_host(uv, tri):
    """crh_guide_table_host on the host only (no GPU): uv (n, 2) float32 per vertex or None (no texture coordinates), tri (m, 4) rows {v0, v1, v2, material}; the
    shade guide's per-triangle table, a numpy record array of m entries (abi.GUIDE_TABLE_DTYPE, 32 B each)"""
    lib = load_library()
    uv = None if uv is None else np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    tri = np.ascontiguousarray(np.asarray(tri).astype(np.int64) & 0xFFFFFFFF, np.uint32).reshape(-1, 4)
    out = np.zeros(len(tri), abi.GUIDE_TABLE_DTYPE)
    rc = lib.crh_guide_table_host(None if uv is None else uv.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(0 if uv is None else len(uv)),
                                  tri.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(len(tri)), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise BackendError(f"crh_guide_table_host -> {rc}")
    return out


def pack_texture_pool(textures):
    """(texels (n, 4) float32, desc (slots, 4) uint32) of a list of (H, W, 3 | 4) images or None entries, as crh_shade_guide_scene takes them: every slot's
    RGBA texels back to back (an RGB image gets alpha 1), per slot {first texel, width, height, 0}"""
    pool, desc, at = [], np.zeros((len(textures), 4), np.uint32), 0
    for k, im in enumerate(textures):
        if im is None:
            continue
        a = np.asarray(im, np.float32)
        if a.shape[2] == 3:
            a = np.concatenate([a, np.ones(a.shape[:2] + (1,), np.float32)], 2)
        desc[k] = (at, a.shape[1], a.shape[0], 0)
        pool.append(a.reshape(-1, 4)); at += a.shape[0] * a.shape[1]
    return (np.ascontiguousarray(np.concatenate(pool), np.float32) if pool else np.zeros((0, 4), np.float32)), desc


def shade_guide_host(materials, textures, scene_lights, gamma2, rays, triangle_px, t_px, uv_px, table, **params):
    """crh_shade_guide_host on the host only (no GPU): materials / scene_lights as Backend.set_materials / set_lights take them, textures a list of (H, W, 3 | 4) images
    (None: an empty slot), gamma2 = crh_spec's texel_gamma2; rays (H * W, 8) float32 as camera_rays returns them for the pixels in row-major order; the planes as
    read_ids / read_hit_uv return them; table as guide_table_host returns it; params as in Backend.set_shade_guide; the (H, W, 4) float32 plane read_shade_guide
    returns"""
    from .binding import pack_lights, shade_guide_params
    from .materials import pack_materials
    lib = load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    tr, t = np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    uv = np.ascontiguousarray(uv_px, np.float32)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    assert tr.ndim == 2 and tr.shape == t.shape and uv.shape == tr.shape + (2,) and len(r) == tr.size
    mats = pack_materials(materials)
    ls = pack_lights(scene_lights)
    pool, desc = pack_texture_pool(list(textures or []))
    tb = np.zeros(0, abi.GUIDE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.GUIDE_TABLE_DTYPE)
    S = abi.crh_shade_guide_scene()
    S.mats = C.cast(mats, C.POINTER(abi.crh_bsdf)); S.n_mats = len(materials)
    S.texels = pool.ctypes.data_as(fp) if len(pool) else None; S.n_texels = len(pool)
    S.tex_desc = desc.ctypes.data_as(C.POINTER(C.c_uint32)) if len(desc) else None; S.n_tex = len(desc)
    S.lights = C.cast(ls, C.POINTER(abi.crh_light)) if len(scene_lights) else None; S.n_lights = len(scene_lights)
    S.gamma2 = int(gamma2)
    p = shade_guide_params(**params)
    out = np.zeros(tr.shape + (4,), np.float32)
    rc = lib.crh_shade_guide_host(C.byref(S), r.ctypes.data_as(fp), tr.ctypes.data_as(ip), t.ctypes.data_as(fp), uv.ctypes.data_as(fp), C.c_uint32(tr.shape[1]),
                                  C.c_uint32(tr.shape[0]), tb.ctypes.data_as(C.c_void_p) if len(tb) else None, C.c_uint32(len(tb)), C.byref(p), out.ctypes.data_as(fp))
    if rc != 0:
        raise BackendError(f"crh_shade_guide_host -> {rc}")
    return out


def denoise_guided_host(rgba, object_px, triangle_px, t_px, table, plane, **params):
    """crh_denoise_guided_host on the host only (no GPU): denoise_host's arguments plus the (H, W, 4) plane as read_shade_guide / shade_guide_host return it"""
    from .binding import denoise_params
    lib = load_library()
    img, sg = np.ascontiguousarray(rgba, np.float32), np.ascontiguousarray(plane, np.float32)
    ob, tr, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == tr.shape == t.shape and img.shape == sg.shape == ob.shape + (4,)
    tb = np.zeros(0, abi.OUTLINE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.OUTLINE_TABLE_DTYPE)
    p = denoise_params(**params)
    out = np.zeros(img.shape, np.float32)
    rc = lib.crh_denoise_guided_host(img.ctypes.data_as(C.POINTER(C.c_float)), ob.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_int32)),
                                     t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]),
                                     tb.ctypes.data_as(C.c_void_p) if len(tb) else None, C.c_uint32(len(tb)), sg.ctypes.data_as(C.POINTER(C.c_float)), C.byref(p),
                                     out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise BackendError(f"crh_denoise_guided_host -> {rc}")
    return out


def reproject_frame_host(cam, width, height):
    """crh_reproject_frame_host on the host only (no GPU): the camera frame of a scenes.Camera at a frame size, as a dict of float32 arrays / scalars
    (eye, right, up, fwd, tan_half, aspect, ortho_scale, is_ortho)"""
    from .binding import camera_struct
    lib = load_library()
    F = abi.crh_reproject_frame()
    rc = lib.crh_reproject_frame_host(C.byref(camera_struct(cam)), C.c_uint32(int(width)), C.c_uint32(int(height)), C.byref(F))
    if rc != 0:
        raise BackendError(f"crh_reproject_frame_host -> {rc}")
    return dict(eye=np.array(F.eye[:], np.float32), right=np.array(F.right[:], np.float32), up=np.array(F.up[:], np.float32), fwd=np.array(F.fwd[:], np.float32),
                tan_half=np.float32(F.tan_half), aspect=np.float32(F.aspect), ortho_scale=np.float32(F.ortho_scale), is_ortho=int(F.is_ortho))


def reproject_host(accum, rays, object_px, triangle_px, t_px, history, table, **params):
    """crh_reproject_host on the host only (no GPU): accum (H, W, 4) float32 as save_accum returns it; rays (H * W, 8) float32 as camera_rays returns them for the
    pixels in row-major order; the planes as read_ids returns them; history = None (every pixel passes through) or a dict(rgba, ob, tr, t, frame): the image, the id
    planes of its view and that view's camera frame as reproject_frame_host returns it; table as outline_table_host returns it (None / empty: only taps of the
    same triangle count); params as in Backend.set_reproject (fields of crh_reproject_params); the (H, W, 4) float32 image read_reprojected returns"""
    from .binding import reproject_params
    lib = load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    img = np.ascontiguousarray(accum, np.float32)
    ob, tr, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == tr.shape == t.shape and img.shape == ob.shape + (4,)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    assert len(r) == ob.size
    tb = np.zeros(0, abi.OUTLINE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.OUTLINE_TABLE_DTYPE)
    h = [None] * 5
    if history is not None:
        himg = np.ascontiguousarray(history["rgba"], np.float32)
        hob, htr, ht = np.ascontiguousarray(history["ob"], np.int32), np.ascontiguousarray(history["tr"], np.int32), np.ascontiguousarray(history["t"], np.float32)
        assert himg.shape == img.shape and hob.shape == htr.shape == ht.shape == ob.shape
        f = history["frame"]
        F = abi.crh_reproject_frame()
        F.eye[:] = [float(x) for x in f["eye"]]; F.right[:] = [float(x) for x in f["right"]]; F.up[:] = [float(x) for x in f["up"]]; F.fwd[:] = [float(x) for x in f["fwd"]]
        F.tan_half, F.aspect, F.ortho_scale, F.is_ortho = float(f["tan_half"]), float(f["aspect"]), float(f["ortho_scale"]), int(f["is_ortho"])
        h = [himg.ctypes.data_as(fp), hob.ctypes.data_as(ip), htr.ctypes.data_as(ip), ht.ctypes.data_as(fp), C.byref(F)]
    p = reproject_params(**params)
    out = np.zeros(img.shape, np.float32)
    rc = lib.crh_reproject_host(img.ctypes.data_as(fp), r.ctypes.data_as(fp), ob.ctypes.data_as(ip), tr.ctypes.data_as(ip), t.ctypes.data_as(fp), *h,
                                tb.ctypes.data_as(C.c_void_p) if len(tb) else None, C.c_uint32(len(tb)), C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]), C.byref(p),
                                out.ctypes.data_as(fp))
    if rc != 0:
        raise BackendError(f"crh_reproject_host -> {rc}")
    return out


def reproject_delta_host(xf_hist, xf_cur):
    """crh_reproject_delta_host on the host only (no GPU): the delta table (abi.REPROJECT_DELTA_DTYPE records) of two (n, 12) float32 arrays of 3x4 transforms --
    those in force when the history was captured, and those in force now"""
    lib = load_library()
    a, b = np.ascontiguousarray(xf_hist, np.float32).reshape(-1, 12), np.ascontiguousarray(xf_cur, np.float32).reshape(-1, 12)
    assert a.shape == b.shape
    out = np.zeros(len(a), abi.REPROJECT_DELTA_DTYPE)
    fp = C.POINTER(C.c_float)
    rc = lib.crh_reproject_delta_host(a.ctypes.data_as(fp), b.ctypes.data_as(fp), C.c_uint32(len(a)), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise BackendError(f"crh_reproject_delta_host -> {rc}")
    return out


def reproject_motion_host(accum, rays, object_px, triangle_px, t_px, history, table, delta_table, motion=None, **params):
    """crh_reproject_motion_host on the host only (no GPU): reproject_host's arguments, the delta table as reproject_delta_host returns it (None: the image of
    reproject_host) and motion = dict of crh_reproject_motion_params fields (None: the defaults); the (H, W, 4) float32 image read_reprojected returns"""
    from .binding import reproject_motion_params, reproject_params
    lib = load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    img = np.ascontiguousarray(accum, np.float32)
    ob, tr, t = np.ascontiguousarray(object_px, np.int32), np.ascontiguousarray(triangle_px, np.int32), np.ascontiguousarray(t_px, np.float32)
    assert ob.ndim == 2 and ob.shape == tr.shape == t.shape and img.shape == ob.shape + (4,)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    assert len(r) == ob.size
    tb = np.zeros(0, abi.OUTLINE_TABLE_DTYPE) if table is None else np.ascontiguousarray(table, abi.OUTLINE_TABLE_DTYPE)
    h = [None] * 5
    if history is not None:
        himg = np.ascontiguousarray(history["rgba"], np.float32)
        hob, htr, ht = np.ascontiguousarray(history["ob"], np.int32), np.ascontiguousarray(history["tr"], np.int32), np.ascontiguousarray(history["t"], np.float32)
        assert himg.shape == img.shape and hob.shape == htr.shape == ht.shape == ob.shape
        f = history["frame"]
        F = abi.crh_reproject_frame()
        F.eye[:] = [float(x) for x in f["eye"]]; F.right[:] = [float(x) for x in f["right"]]; F.up[:] = [float(x) for x in f["up"]]; F.fwd[:] = [float(x) for x in f["fwd"]]
        F.tan_half, F.aspect, F.ortho_scale, F.is_ortho = float(f["tan_half"]), float(f["aspect"]), float(f["ortho_scale"]), int(f["is_ortho"])
        h = [himg.ctypes.data_as(fp), hob.ctypes.data_as(ip), htr.ctypes.data_as(ip), ht.ctypes.data_as(fp), C.byref(F)]
    p = reproject_params(**params)
    dt = None if delta_table is None else np.ascontiguousarray(delta_table, abi.REPROJECT_DELTA_DTYPE)
    mp = reproject_motion_params(**(motion or {}))
    out = np.zeros(img.shape, np.float32)
    rc = lib.crh_reproject_motion_host(img.ctypes.data_as(fp), r.ctypes.data_as(fp), ob.ctypes.data_as(ip), tr.ctypes.data_as(ip), t.ctypes.data_as(fp), *h,
                                       tb.ctypes.data_as(C.c_void_p) if len(tb) else None, C.c_uint32(len(tb)), C.c_uint32(ob.shape[1]), C.c_uint32(ob.shape[0]), C.byref(p),
                                       None if dt is None else dt.ctypes.data_as(C.c_void_p), C.c_uint32(0 if dt is None else len(dt)), C.byref(mp), out.ctypes.data_as(fp))
    if rc != 0:
        raise BackendError(f"crh_reproject_motion_host -> {rc}")
    return out


def view_host(ldr, width, height, src=(0, 0, 0, 0), filter=abi.VIEW_AUTO):
    """crh_view_host on the host only (no GPU): the (H, W, 3) uint8 frame read_ldr returns, resampled to (height, width, 3) by the rule of read_view -- what a host
    without the device-side view has to do with every frame it shows"""
    from .binding import view_params
    lib = load_library()
    img = np.ascontiguousarray(ldr, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    p = view_params(width=width, height=height, src=src, filter=filter)
    out = np.zeros((p.height, p.width, 3), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = lib.crh_view_host(img.ctypes.data_as(u8), C.c_uint32(img.shape[1]), C.c_uint32(img.shape[0]), C.byref(p), out.ctypes.data_as(u8))
    if rc != 0:
        raise BackendError(f"crh_view_host -> {rc}")
    return out


def view_fit(frame_w, frame_h, area_w, area_h):
    """crh_view_fit on the host only (no GPU): the letterbox of AppViewer.cxx:930-953 -- dict(width, height, src, filter), the keyword arguments of read_view for a
    frame_w x frame_h frame shown whole in a panel of area_w x area_h"""
    lib = load_library()
    p = abi.crh_view_params()
    rc = lib.crh_view_fit(C.c_uint32(int(frame_w)), C.c_uint32(int(frame_h)), C.c_uint32(int(area_w)), C.c_uint32(int(area_h)), C.byref(p))
    if rc != 0:
        raise BackendError(f"crh_view_fit -> {rc}")
    return dict(width=int(p.width), height=int(p.height), src=tuple(int(x) for x in p.src), filter=int(p.filter))


def view_to_frame(frame_w, frame_h, vx, vy, width, height, src=(0, 0, 0, 0), filter=abi.VIEW_AUTO):
    """crh_view_to_frame on the host only (no GPU): the frame pixel (fx, fy) under pixel (vx, vy) of the view these parameters describe -- what pick, set_hover and
    query_region are to be asked about"""
    from .binding import view_params
    lib = load_library()
    p = view_params(width=width, height=height, src=src, filter=filter)
    fx, fy = C.c_uint32(0), C.c_uint32(0)
    rc = lib.crh_view_to_frame(C.byref(p), C.c_uint32(int(frame_w)), C.c_uint32(int(frame_h)), C.c_uint32(int(vx)), C.c_uint32(int(vy)), C.byref(fx), C.byref(fy))
    if rc != 0:
        raise BackendError(f"crh_view_to_frame -> {rc}")
    return int(fx.value), int(fy.value)


def _annot_list(segments):
    """a contiguous record array of abi.ANNOT_SEGMENT_DTYPE (an empty one for None)"""
    return np.zeros(0, abi.ANNOT_SEGMENT_DTYPE) if segments is None else np.ascontiguousarray(segments, abi.ANNOT_SEGMENT_DTYPE).reshape(-1)


def annot_project_host(cam, width, height, segments):
    """crh_annot_project_host on the host only (no GPU): the screen records of the segments under a scenes.Camera at a frame size, a record array of
    abi.ANNOT_RECORD_DTYPE"""
    from .binding import camera_struct
    lib = load_library()
    sg = _annot_list(segments)
    out = np.zeros(len(sg), abi.ANNOT_RECORD_DTYPE)
    rc = lib.crh_annot_project_host(C.byref(camera_struct(cam)), C.c_uint32(int(width)), C.c_uint32(int(height)),
                                    sg.ctypes.data_as(C.POINTER(abi.crh_annot_segment)) if len(sg) else None, C.c_uint32(len(sg)),
                                    out.ctypes.data_as(C.c_void_p) if len(sg) else None)
    if rc != 0:
        raise BackendError(f"crh_annot_project_host -> {rc}")
    return out


def annot_draw_host(records, segments, cam, width, height, ldr=None, rays=None, t_px=None, depth_bias=abi.ANNOT_DEFAULTS["depth_bias"],
                    hidden_alpha=abi.ANNOT_DEFAULTS["hidden_alpha"]):
    """crh_annot_draw_host on the host only (no GPU): the segments drawn over a copy of the (H, W, 3) uint8 image `ldr` (None: no image) from their records; rays
    (H * W, 8) as camera_rays returns them for the pixels in row-major order and t_px (H, W) as read_ids returns it (both None when no segment asks for depth).
    Returns (image or None, (H, W) int32 id plane)."""
    from .binding import camera_struct
    lib = load_library()
    sg = _annot_list(segments)
    rec = np.ascontiguousarray(records, abi.ANNOT_RECORD_DTYPE).reshape(-1)
    assert len(rec) == len(sg)
    W, H = int(width), int(height)
    img = None if ldr is None else np.array(ldr, np.uint8, order="C")
    assert img is None or img.shape == (H, W, 3)
    r = None if rays is None else np.ascontiguousarray(rays, np.float32).reshape(H * W, 8)
    t = None if t_px is None else np.ascontiguousarray(t_px, np.float32).reshape(H, W)
    ids = np.empty((H, W), np.int32)
    p = abi.crh_annot_params(float(depth_bias), int(hidden_alpha))
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.crh_annot_draw_host(rec.ctypes.data_as(C.c_void_p) if len(sg) else None, sg.ctypes.data_as(C.POINTER(abi.crh_annot_segment)) if len(sg) else None,
                                 C.c_uint32(len(sg)), C.byref(p), C.byref(camera_struct(cam)), C.c_uint32(W), C.c_uint32(H), fp(r), fp(t),
                                 None if img is None else img.ctypes.data_as(C.POINTER(C.c_uint8)), ids.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise BackendError(f"crh_annot_draw_host -> {rc}")
    return img, ids


def build_bvh_host(pos, tri, threads=0):
    """Run the product's BVH builder on the host only (no GPU): returns (nodes[n,16] u32-as-f32, prim_order[nT] u32)."""
    lib = load_library()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 4)
    nn = C.c_uint32(0)
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    args = (pos.ctypes.data_as(fp), C.c_uint32(len(pos)), tri.ctypes.data_as(ip), C.c_uint32(len(tri)), C.c_int(threads))
    nodes = np.empty((max(len(tri), 4), abi.NODE_DWORDS), np.float32)   # nodes <= max(1, ~nT/2), 64 B each
    order = np.empty(len(tri), np.uint32)
    rc = lib.crh_build_bvh_host(*args, nodes.ctypes.data_as(fp), C.byref(nn), order.ctypes.data_as(up))
    if rc != 0:
        raise RuntimeError(f"crh_build_bvh_host -> {rc}")
    return nodes[:nn.value].copy(), order
