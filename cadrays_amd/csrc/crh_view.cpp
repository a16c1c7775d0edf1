// crh_view.cpp -- the viewport read-out: the application renders into a target whose size the user sets apart from the window's (reference "Resolution" panel,
// SettingsWidget.cxx:104-149), letterboxes it into the panel (src/Launcher/AppViewer.cxx:929-957) and lets the GL texture unit scale the FBO's RGB8 colour texture to
// the panel's size (:1095-1102).  Here the read-outs do that scaling on the device, as the LAST stage of the display chain: the host receives width x height x 3 bytes
// of the window's size instead of the frame's, and a source rectangle gives zoom and pan on the accumulated frame without a restart.
// One kernel (view_kernels.hip); the rule has ONE copy (view_kernels.h), compiled for the kernels and for the host twin below.
// Nothing of the rendering state is touched, and nothing is kept between calls but scratch memory.  DESIGN.md section 4.15.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "view_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_view_params) == 32, "crh_view_params is 32 bytes");
static_assert(kViewAuto == CRH_VIEW_AUTO && kViewNearest == CRH_VIEW_NEAREST && kViewBilinear == CRH_VIEW_BILINEAR && kViewArea == CRH_VIEW_AREA, "the filters of the header");
static_assert(kViewMaxSide == CRH_VIEW_MAX_SIDE, "the largest side of the header");

namespace {

// why these parameters cannot be applied to a W x H frame (nullptr: they can, and *plan holds both axes)
const char* view_refused(const crh_view_params* p, uint32_t W, uint32_t H, ViewPlan* plan)
{
  if (!W || !H || W > kViewMaxSide || H > kViewMaxSide) return "the frame has a side of 0 or above 8192";
  if (!p->width || !p->height || p->width > kViewMaxSide || p->height > kViewMaxSide) return "the view has a side of 0 or above 8192";
  if (p->filter > kViewArea) return "filter is none of CRH_VIEW_AUTO / _NEAREST / _BILINEAR / _AREA";
  if (p->reserved) return "reserved is not 0";
  uint32_t x0 = p->src[0], y0 = p->src[1], x1 = p->src[2], y1 = p->src[3];
  if (!(x0 | y0 | x1 | y1)) { x1 = W; y1 = H; }      // all zero: the whole frame
  if (x0 >= x1 || y0 >= y1) return "the source rectangle is empty";
  if (x1 > W || y1 > H) return "the source rectangle leaves the frame";
  plan->X = view_axis(x1 - x0, p->width, x0, W, p->filter);
  plan->Y = view_axis(y1 - y0, p->height, y0, H, p->filter);
  plan->identity = p->width == W && p->height == H && x1 - x0 == W && y1 - y0 == H;
  return nullptr;
}

// the checks every call on a context shares; CRH_OK: *plan is the plan over the frame in force
int plan_of(crh_ctx* c, const char* who, const crh_view_params* p, ViewPlan* plan)
{
  const char* why = !p ? "null parameters" : !c->d_accum ? "no accumulator" : view_refused(p, c->par.width, c->par.height, plan);
  if (!why) return CRH_OK;
  const std::string m = std::string(who) + ": " + why;
  return fail(c, CRH_E_INVALID, m.c_str());
}

}  // namespace

namespace crh {
namespace api {

int view_resample(crh_ctx* c, hipStream_t on, const uint8_t* d_full, const ViewPlan& P, uint8_t* d_out)
{
  launch_view(on, d_full, c->par.width, c->par.height, P, d_out);
  CRH_HIP(hipGetLastError());
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

int crh_read_view(crh_ctx* c, const crh_view_params* p, uint8_t* out)
{
  if (!c) return CRH_E_INVALID;
  c->read_since_render = true;
  if (!out) return fail(c, CRH_E_INVALID, "crh_read_view: null output");
  ViewPlan P;
  if (int rc = plan_of(c, "crh_read_view", p, &P)) return rc;
  if (P.identity) return crh_read_ldr(c, out);           // the view is the frame: no resample kernel, crh_read_ldr's bytes
  CRH_HIP(hipSetDevice(c->device));
  const size_t full = 3 * (size_t)c->par.width * c->par.height, bytes = 3 * (size_t)P.X.v * P.Y.v;
  if (int rc = grow_display_scratch(c, 0, &c->d_vw_full[0], 1, full)) return rc;
  CRH_HIP(c->d_scratch.reserve(bytes));
  Launch L{cstream(c), c->grid, false};
  if (int rc = enqueue_display_chain(c, L, 0, 0, c->d_vw_full[0])) return rc;
  if (int rc = view_resample(c, L.stream, c->d_vw_full[0], P, c->d_scratch.as<uint8_t>())) return rc;
  CRH_HIP(hipMemcpyAsync(out, c->d_scratch, bytes, hipMemcpyDeviceToHost, L.stream));
  CRH_HIP(hipStreamSynchronize(L.stream));
  return CRH_OK;
}

int crh_read_view_begin(crh_ctx* c, const crh_view_params* p)
{
  if (!c) return CRH_E_INVALID;
  ViewPlan P;
  if (int rc = plan_of(c, "crh_read_view_begin", p, &P)) return rc;
  return read_begin(c, kReadView, &P);
}

int crh_read_view_end(crh_ctx* c, uint8_t* out) { return read_end(c, out, kReadView); }

int crh_bench_view(crh_ctx* c, const crh_view_params* p, uint32_t repeats, float* resample_ms)
{
  if (!c) return CRH_E_INVALID;
  if (!repeats) return fail(c, CRH_E_INVALID, "crh_bench_view: no repeats");
  ViewPlan P;
  if (int rc = plan_of(c, "crh_bench_view", p, &P)) return rc;
  c->read_since_render = true;
  CRH_HIP(hipSetDevice(c->device));
  const uint32_t W = c->par.width, H = c->par.height;
  // this call's own blocks, released when it returns: the frame as a read-out issued now would show it, and the view
  DevBuf<uint8_t> d_full, d_out;
  CRH_HIP(d_full.reserve(3 * (size_t)W * H)); CRH_HIP(d_out.reserve(3 * (size_t)P.X.v * P.Y.v));
  Launch L{cstream(c), c->grid, false};
  if (int rc = enqueue_display_chain(c, L, 0, 0, d_full)) { hipStreamSynchronize(L.stream); return rc; }
  launch_view(L.stream, d_full, W, H, P, d_out);         // the code is loaded
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = time_launches(L.stream, repeats, [&] { launch_view(L.stream, d_full, W, H, P, d_out); return hipGetLastError(); }, resample_ms);
  else hipStreamSynchronize(L.stream);
  CRH_HIP(e);                                            // (the stream has been waited for: this call's blocks may go)
  return CRH_OK;
}

int crh_view_host(const uint8_t* ldr, uint32_t W, uint32_t H, const crh_view_params* p, uint8_t* out)
{
  if (!ldr || !p || !out) return CRH_E_INVALID;
  ViewPlan P;
  if (view_refused(p, W, H, &P)) return CRH_E_INVALID;
  view_host(ldr, W, H, P, out);
  return CRH_OK;
}

// AppViewer.cxx:930-935 with the truncation of :952-953, in float32 as written there
int crh_view_fit(uint32_t W, uint32_t H, uint32_t area_w, uint32_t area_h, crh_view_params* out)
{
  if (!out || !W || !H || !area_w || !area_h || W > kViewMaxSide || H > kViewMaxSide || area_w > kViewMaxSide || area_h > kViewMaxSide) return CRH_E_INVALID;
  const float aspect = (float)W / (float)H;
  const float window_aspect = (float)area_w / (float)area_h;
  uint32_t vw, vh;
  if (window_aspect < aspect) { vw = area_w; vh = (uint32_t)((float)area_w / aspect); }
  else { vw = (uint32_t)((float)area_h * aspect); vh = area_h; }
  std::memset(out, 0, sizeof *out);                      // the whole frame, CRH_VIEW_AUTO
  out->width = std::min(std::max(vw, 1u), kViewMaxSide); out->height = std::min(std::max(vh, 1u), kViewMaxSide);
  return CRH_OK;
}

int crh_view_to_frame(const crh_view_params* p, uint32_t W, uint32_t H, uint32_t vx, uint32_t vy, uint32_t* fx, uint32_t* fy)
{
  if (!p || !fx || !fy) return CRH_E_INVALID;
  ViewPlan P;
  if (view_refused(p, W, H, &P) || vx >= p->width || vy >= p->height) return CRH_E_INVALID;
  const ViewAxis X = view_axis(P.X.s, P.X.v, P.X.off, P.X.S, kViewNearest), Y = view_axis(P.Y.s, P.Y.v, P.Y.off, P.Y.S, kViewNearest);
  *fx = view_tap_index(X, view_taps(X, vx), 0u); *fy = view_tap_index(Y, view_taps(Y, vy), 0u);
  return CRH_OK;
}

}  // extern "C"
