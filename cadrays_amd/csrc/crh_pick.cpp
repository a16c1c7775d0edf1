// crh_pick.cpp -- what the application does to a RENDERED scene on every mouse move and click: which object lies under a pixel (AIS_InteractiveContext::MoveTo /
// Select, reference src/Launcher/AppViewer.cxx:347, 359-455), how far away (autofocus, AppGui.cxx:78-94), the selection drawn highlighted, its bounds (the
// manipulator's pivot, AppViewer.cxx:863-875).  All of it reads ONE derived buffer: the first hit of the pixel-centre camera ray of every pixel, traced by the very
// kernels crh_trace_nearest runs (k_ids.h generates the rays and sorts the answers; the traversal is k_trace_rays, unchanged).
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"

using namespace crh;
using namespace crh::api;

namespace {

bool good_rgb_alpha(const uint8_t* rgb, uint32_t alpha) { return rgb && alpha <= 255u; }

}  // namespace

namespace crh {
namespace api {

// The id buffer of the state in force, computed if a change has invalidated it.  Synchronous on its own stream: when this returns, every stream may read it.
int ensure_ids(crh_ctx* c)
{
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  const uint32_t W = c->par.width, H = c->par.height;
  if (c->ids_valid && c->ids_w == W && c->ids_h == H) return CRH_OK;
  CRH_HIP(hipSetDevice(c->device));
  int rc = pick_stream(c); if (rc) return rc;
  if ((rc = wait_overlay_readers(c))) return rc;
  const size_t n_slots = 64 * (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u), n_px = (size_t)W * H;
  CRH_HIP(c->d_pk_rays.reserve(2 * n_slots)); CRH_HIP(c->d_pk_hit_slot.reserve(n_slots));      // (what read the old blocks has been waited for: this stream runs
  CRH_HIP(c->d_pk_hit.reserve(n_px)); CRH_HIP(c->d_pk_obj.reserve(n_px));                       //  synchronously, the overlay's readers just above)
  if (c->pk_tri_obj_gen != c->geom_gen && !c->tri_obj.empty() && (rc = side_upload(c, c->d_pk_tri_obj, c->tri_obj.data(), c->tri_obj.size()))) return rc;
  c->pk_tri_obj_gen = c->geom_gen;                       // (also of a scene without objects: there is nothing to upload)
  if ((rc = fork_from_context(c))) return rc;
  DScene S; fill_scene(c, S);
  Launch Ls{c->pk_stream, c->grid, false};
  Launch Lt{c->pk_stream, c->grid_trace, false, c->clamp_grid ? c->cus : 0};
  launch_first_hit_rays(Ls, S, nullptr, (uint32_t)n_slots, c->d_pk_rays);
  launch_trace_rays(Lt, S, c->d_pk_rays, (uint32_t)n_slots, 0, c->d_pk_hit_slot, nullptr, c->d_pk_cursor, c->d_pk_counters);
  launch_first_hit_resolve(Ls, W, H, (uint32_t)n_slots, c->d_pk_hit_slot, c->tri_obj.empty() ? nullptr : c->d_pk_tri_obj, (uint32_t)c->tri_obj.size(), c->d_pk_hit, c->d_pk_obj);
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->ids_valid = true; c->ids_w = W; c->ids_h = H; ++c->ids_gen;
  return CRH_OK;
}

uint32_t n_pick_objects(const crh_ctx* c) { return c->tri_obj.empty() ? 1u : c->nO; }      // a scene handed over without objects is one object, 0

int pick_stream(crh_ctx* c)
{
  if (c->pk_stream) return CRH_OK;
  CRH_HIP(hipStreamCreateWithFlags(&c->pk_stream, hipStreamNonBlocking));
  CRH_HIP(hipEventCreateWithFlags(&c->pk_fork, hipEventDisableTiming));
  CRH_HIP(c->d_pk_cursor.reserve(16));
  CRH_HIP(c->d_pk_counters.reserve(1));
  CRH_HIP(hipMemsetAsync(c->d_pk_counters, 0, sizeof(DCounters), c->pk_stream));
  return CRH_OK;
}

// the side stream starts behind whatever the setters have put on the context's stream (scene uploads are stream-ordered there); the frames in flight on the
// pipeline streams are NOT joined and the schedule's bookkeeping (cstream()) is not touched: they only read the scene, as this does
int fork_from_context(crh_ctx* c)
{
  CRH_HIP(hipEventRecord(c->pk_fork, c->stream_));
  CRH_HIP(hipStreamWaitEvent(c->pk_stream, c->pk_fork, 0));
  return CRH_OK;
}

// an asynchronous LDR read-back may still be running its overlay over the id buffer and the selection flags: wait for those kernels before either is overwritten
int wait_overlay_readers(crh_ctx* c)
{
  if (c->rb_outstanding) for (int k = 0; k < 2; ++k) if (c->rb_tm[k]) CRH_HIP(hipEventSynchronize(c->rb_tm[k]));
  return CRH_OK;
}

void clear_selection(crh_ctx* c) { c->sel.clear(); c->sel_any = false; c->sel_dirty = false; c->hover = -1; }

// Called by the LDR read-outs right after the tone map (which includes the ShowSamplingTiles outline: the overlay comes LAST), on the stream the tone map ran on.
// No selection and no hover: nothing is launched and nothing is computed -- the bytes are the tone map's.
int overlay_ldr(crh_ctx* c, hipStream_t on, uint8_t* d_ldr)
{
  if (!c->sel_any && c->hover < 0) return CRH_OK;
  if (!c->built) return CRH_OK;                          // a selection cannot outlive its scene (crh_set_geometry clears it); nothing to draw over
  int rc = ensure_ids(c); if (rc) return rc;
  if (c->sel_any && c->sel_dirty) {
    if ((rc = wait_overlay_readers(c))) return rc;
    CRH_HIP(c->d_sel.reserve(c->sel.size(), 64));
    CRH_HIP(hipMemcpyAsync(c->d_sel, c->sel.data(), c->sel.size(), hipMemcpyHostToDevice, c->pk_stream));
    CRH_HIP(hipStreamSynchronize(c->pk_stream));
    c->sel_dirty = false;
  }
  Launch L{on, c->grid, false};
  launch_overlay(L, d_ldr, c->d_pk_obj, c->par.width, c->par.height, c->sel_any ? c->d_sel : nullptr, (uint32_t)c->sel.size(), c->sel_rgb, c->sel_alpha, c->hover, c->hov_rgb, c->hov_alpha);
  CRH_HIP(hipGetLastError());
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

int crh_camera_rays(crh_ctx* c, const uint32_t* xy, uint32_t n, float* rays_out)
{
  if (!c || (n && (!xy || !rays_out))) return fail(c, CRH_E_INVALID, "null pixel list / ray buffer");
  for (uint32_t i = 0; i < n; ++i)
    if (xy[2 * (size_t)i] >= c->par.width || xy[2 * (size_t)i + 1] >= c->par.height) { char b[96]; snprintf(b, sizeof b, "pixel %u lies outside the %u x %u target", i, c->par.width, c->par.height); return fail(c, CRH_E_INVALID, b); }
  if (!n) return CRH_OK;
  CRH_HIP(hipSetDevice(c->device));
  int rc = pick_stream(c); if (rc) return rc;
  DevBuf<uint32_t> d_xy; DevBuf<float4> d_rays;       // this call's own: released when it returns
  CRH_HIP(d_xy.reserve(2 * (size_t)n)); CRH_HIP(d_rays.reserve(2 * (size_t)n));
  hipError_t e = hipMemcpyAsync(d_xy, xy, 8 * (size_t)n, hipMemcpyHostToDevice, c->pk_stream);
  if (e == hipSuccess) {
    DScene S; fill_scene(c, S);
    Launch L{c->pk_stream, c->grid, false};
    launch_first_hit_rays(L, S, d_xy, n, d_rays);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rays_out, d_rays, 32 * (size_t)n, hipMemcpyDeviceToHost, c->pk_stream);
  const hipError_t e2 = hipStreamSynchronize(c->pk_stream);      // whatever went wrong: nothing still uses the two blocks when they go
  CRH_HIP(e); CRH_HIP(e2);
  return CRH_OK;
}

int crh_pick(crh_ctx* c, uint32_t x, uint32_t y, crh_pick_result* out)
{
  if (!c || !out) return fail(c, CRH_E_INVALID, "null pick result");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (x >= c->par.width || y >= c->par.height) return fail(c, CRH_E_INVALID, "pixel outside the render target");
  int rc = ensure_ids(c); if (rc) return rc;
  float h[4];
  CRH_HIP(hipMemcpyAsync(h, c->d_pk_hit + ((size_t)y * c->par.width + x), sizeof h, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  int32_t tri; std::memcpy(&tri, &h[3], 4);
  std::memset(out, 0, sizeof *out);
  out->triangle = tri; out->t = h[0];
  out->object = tri < 0 ? -1 : (c->tri_obj.empty() ? 0 : ((size_t)tri < c->tri_obj.size() ? c->tri_obj[tri] : -1));
  if (tri < 0) return CRH_OK;                           // a miss: t = the ray's tmax, everything else zero
  out->u = h[1]; out->v = h[2];
  DScene S; fill_scene(c, S);
  float o[3], d[3];
  pixel_centre_ray_host(S, x, y, o, d);
  const crh_v3 p = crh_madd3(crh_mk3(o[0], o[1], o[2]), crh_mk3(d[0], d[1], d[2]), h[0]);
  out->point[0] = p.x; out->point[1] = p.y; out->point[2] = p.z;
  out->depth = crh_dot3(crh_sub3(p, S.eye), S.fwd);
  return CRH_OK;
}

int crh_read_ids(crh_ctx* c, int32_t* object_out, int32_t* triangle_out, float* t_out)
{
  if (!c) return CRH_E_INVALID;
  int rc = ensure_ids(c); if (rc) return rc;
  const size_t n = (size_t)c->par.width * c->par.height;
  if (object_out) CRH_HIP(hipMemcpyAsync(object_out, c->d_pk_obj, 4 * n, hipMemcpyDeviceToHost, c->pk_stream));
  std::vector<float> h;
  if (triangle_out || t_out) { h.resize(4 * n); CRH_HIP(hipMemcpyAsync(h.data(), c->d_pk_hit, 16 * n, hipMemcpyDeviceToHost, c->pk_stream)); }
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  if (triangle_out) for (size_t i = 0; i < n; ++i) std::memcpy(&triangle_out[i], &h[4 * i + 3], 4);
  if (t_out) for (size_t i = 0; i < n; ++i) t_out[i] = h[4 * i];
  return CRH_OK;
}

int crh_set_selection(crh_ctx* c, const uint8_t* selected, uint32_t n_objects, const uint8_t rgb[3], uint32_t alpha)
{
  if (!c) return CRH_E_INVALID;
  if (!selected) { c->sel.clear(); c->sel_any = false; c->sel_dirty = false; return CRH_OK; }
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (n_objects != n_pick_objects(c)) { char b[128]; snprintf(b, sizeof b, "crh_set_selection: %u flags for a scene of %u objects", n_objects, n_pick_objects(c)); return fail(c, CRH_E_INVALID, b); }
  if (!good_rgb_alpha(rgb, alpha)) return fail(c, CRH_E_INVALID, "crh_set_selection: null colour or alpha above 255");
  c->sel.assign(selected, selected + n_objects);
  c->sel_any = false; for (uint8_t f : c->sel) if (f) c->sel_any = true;
  c->sel_dirty = true; c->sel_alpha = alpha; std::memcpy(c->sel_rgb, rgb, 3);
  return CRH_OK;
}

int crh_set_hover(crh_ctx* c, int32_t object, const uint8_t rgb[3], uint32_t alpha)
{
  if (!c) return CRH_E_INVALID;
  if (object < 0) { c->hover = -1; return CRH_OK; }
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if ((uint32_t)object >= n_pick_objects(c)) return fail(c, CRH_E_INVALID, "crh_set_hover: object id out of range");
  if (!good_rgb_alpha(rgb, alpha)) return fail(c, CRH_E_INVALID, "crh_set_hover: null colour or alpha above 255");
  c->hover = object; c->hov_alpha = alpha; std::memcpy(c->hov_rgb, rgb, 3);
  return CRH_OK;
}

int crh_get_selection_bounds(crh_ctx* c, float lo[3], float hi[3])
{
  if (!c || !lo || !hi) return fail(c, CRH_E_INVALID, "null bounds");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->sel_any) return fail(c, CRH_E_INVALID, "nothing is selected");
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  // every vertex under its object's CURRENT transform: three fused multiply-adds per coordinate (one rounding each)
  auto add = [&](const float* p, const float* m) {
    for (int a = 0; a < 3; ++a) {
      const float q = m ? CRH_FMA(m[4 * a], p[0], CRH_FMA(m[4 * a + 1], p[1], CRH_FMA(m[4 * a + 2], p[2], m[4 * a + 3]))) : p[a];
      if (q < mn[a]) mn[a] = q;
      if (q > mx[a]) mx[a] = q;
    }
  };
  if (c->tri_obj.empty()) {                              // one object, world-space vertices
    for (size_t v = 0; v < c->pos.size() / 3; ++v) add(&c->pos[3 * v], nullptr);
  } else {
    for (uint32_t ob = 0; ob < c->nO && ob < c->sel.size(); ++ob) {
      if (!c->sel[ob] || ob >= c->objs.size()) continue;
      const TwoLevelState::Obj& o = c->objs[ob];
      for (uint32_t k = 0; k < o.ntri; ++k) {
        const uint32_t t = c->obj_tris[o.first + k];
        for (int j = 0; j < 3; ++j) add(&c->pos[3 * (size_t)c->tri[4 * (size_t)t + j]], &c->xf[12 * (size_t)ob]);
      }
    }
  }
  if (mn[0] > mx[0]) return fail(c, CRH_E_INVALID, "the selected objects have no triangles");
  for (int a = 0; a < 3; ++a) { lo[a] = mn[a]; hi[a] = mx[a]; }
  return CRH_OK;
}

}  // extern "C"
