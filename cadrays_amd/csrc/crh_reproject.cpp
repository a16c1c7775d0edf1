// crh_reproject.cpp -- reprojected display history: the application restarts the accumulation on every camera change (reference src/Launcher/AppViewer.cxx:979-984) and
// shows one Redraw() per GUI frame (:1045-1047), so during a drag every image has one sample and everything rendered one frame earlier, from a camera a fraction of a
// degree away, is thrown away.  Here crh_set_camera keeps what the ending view DISPLAYED -- image, guide, camera frame -- and the LDR read-outs of the next view fetch it
// through the first-hit point of every pixel and blend it with the new accumulator, in front of the denoise filter.  The reference has no counterpart.
// One kernel (reproject_kernels.hip); the rule has ONE copy (reproject_kernels.h), compiled for the kernel and for the host twin below.  Display state: nothing of the
// rendering state is touched, and only the source of the filter / the tone map changes.  DESIGN.md section 4.13.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "reproject_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_reproject_params) == 16, "crh_reproject_params is 16 bytes");
static_assert(sizeof(crh_reproject_frame) == 64, "crh_reproject_frame is 64 bytes");

namespace {

const char* params_refused(const crh_reproject_params* p)
{
  const float f[] = {p->max_history, p->normal_cos, p->depth_ratio};
  if (!all_finite(f, 3)) return "max_history / normal_cos / depth_ratio hold a NaN / Inf";
  if (!(p->max_history >= 1.f && p->max_history <= 1024.f)) return "max_history lies outside 1..1024";
  if (p->until_samples < 1u || p->until_samples > (1u << 20)) return "until_samples lies outside 1..2^20";
  if (!(p->normal_cos > 0.f && p->normal_cos <= 1.f)) return "normal_cos lies outside (0, 1]";
  if (!(p->depth_ratio >= 1.f)) return "depth_ratio is below 1";
  return nullptr;
}

ReprojectRule rule_of(const crh_reproject_params& p) { return ReprojectRule{p.max_history, (float)p.until_samples, p.normal_cos, p.depth_ratio}; }      // (2^20 is exact)

crh_reproject_params params_in_force(const crh_ctx* c)
{
  crh_reproject_params p; crh_reproject_defaults(&p);
  if (c->rp_on) p = c->rp_par;
  return p;
}

// The camera frame of the view S describes: what fill_scene derived (crh_scene.cpp), field by field.
crh_reproject_frame frame_of(const DScene& S)
{
  crh_reproject_frame F;
  F.eye[0] = S.eye.x; F.eye[1] = S.eye.y; F.eye[2] = S.eye.z;
  F.right[0] = S.right.x; F.right[1] = S.right.y; F.right[2] = S.right.z;
  F.up[0] = S.up.x; F.up[1] = S.up.y; F.up[2] = S.up.z;
  F.fwd[0] = S.fwd.x; F.fwd[1] = S.fwd.y; F.fwd[2] = S.fwd.z;
  F.tan_half = S.tan_half; F.aspect = S.aspect; F.ortho_scale = S.ortho_scale; F.is_ortho = S.is_ortho ? 1u : 0u;
  return F;
}

bool history_valid(const crh_ctx* c) { return c->rp_valid && c->rp_w == c->par.width && c->rp_h == c->par.height && c->d_rp_hist[c->rp_cur].cap() >= (size_t)c->rp_w * c->rp_h; }

ReprojectHistory history_of(const crh_ctx* c)
{
  ReprojectHistory h{};
  if (history_valid(c)) { h.img = c->d_rp_hist[c->rp_cur]; h.guide = c->d_rp_hguide; h.ids = c->d_rp_hids; h.frame = c->rp_frame; h.valid = 1; }
  return h;
}

// The rule over the view in force from `src` into `out`, enqueued on `on` (the guide of the view must be valid: ensure_guide)
void resolve(crh_ctx* c, hipStream_t on, const float4* src, const ReprojectHistory& hist, const ReprojectRule& R, float4* out)
{
  DScene S; fill_scene(c, S);
  launch_reproject_resolve(on, S, c->d_dn_guide, c->d_dn_ids, src, hist, R, out);
}

}  // namespace

namespace crh {
namespace api {

// Called by the LDR read-outs between the metering and the denoise filter, on the stream the tone map runs on.  Feature off, no scene or no valid history: nothing is
// allocated, nothing is launched -- the filter / the tone map reads `src`.  The read-back's rb_tm event, recorded behind the tone map and the overlays, covers this
// kernel's reads of the accumulator and of the history (crh_denoise.cpp, THE ACCUMULATE GUARD; reproject_capture waits for it before it overwrites either).
int reproject_src(crh_ctx* c, hipStream_t on, const float4* src, int set, const float4** shown)
{
  *shown = src;
  if (!c->rp_on || !c->built || !history_valid(c)) return CRH_OK;
  if (int rc = ensure_guide(c)) return rc;
  const size_t n = (size_t)c->par.width * c->par.height;
  DevBuf<float4>& out = c->d_rp_out[set];
  if (int rc = grow_display_scratch(c, set, &out, 1, n)) return rc;
  resolve(c, on, src, history_of(c), rule_of(c->rp_par), out);
  CRH_HIP(hipGetLastError());
  *shown = out;
  return CRH_OK;
}

// crh_set_camera, before `next` replaces the camera in force.  Everything is enqueued on the context's stream, which cstream() first makes wait for the frames in
// flight: the accumulator read here is the ending view's last, and crh_reset's clears come behind.  The host waits only where the header says it may.
int reproject_capture(crh_ctx* c, const crh_camera* next)
{
  if (!c->rp_on || !c->built || c->rp_captured || c->spec.raygen_bilinear != 0) return CRH_OK;
  if (std::memcmp(next, &c->cam, sizeof(crh_camera)) == 0) return CRH_OK;
  const bool have = history_valid(c);
  if (!(c->frames_done > 0 || have)) return CRH_OK;
  const uint32_t W = c->par.width, H = c->par.height;
  if (!c->d_accum || c->accumW != W || c->accumH != H) return CRH_OK;      // no accumulator of this size yet: nothing was displayed
  if (!have) c->rp_valid = false;                        // (a history of another frame size)
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = ensure_guide(c)) return rc;               // the ENDING view's: a host that displays its frames has it already
  if (int rc = wait_overlay_readers(c)) return rc;       // an asynchronous read-back two frames old may still read the image and the guide copy overwritten below
  const size_t n = (size_t)W * H;
  const uint32_t other = c->rp_cur ^ 1u;
  const uint64_t uses = c->stream_uses;
  const hipStream_t cs = cstream(c);
  if (c->d_rp_hist[other].cap() < n || c->d_rp_hguide.cap() < n || c->d_rp_hids.cap() < n) {
    CRH_HIP(hipStreamSynchronize(cs));                   // first need, or a larger frame: an earlier capture may still be writing the blocks that go
    CRH_HIP(c->d_rp_hist[other].reserve(n)); CRH_HIP(c->d_rp_hguide.reserve(n)); CRH_HIP(c->d_rp_hids.reserve(n));      // (with a valid history the guide copies have this size already)
  }
  DScene S; fill_scene(c, S);
  launch_reproject_resolve(cs, S, c->d_dn_guide, c->d_dn_ids, display_source(c), history_of(c), rule_of(c->rp_par), c->d_rp_hist[other]);      // reads the OLD guide copy ...
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipMemcpyAsync(c->d_rp_hguide, c->d_dn_guide, sizeof(float4) * n, hipMemcpyDeviceToDevice, cs));                         // ... which this then replaces
  CRH_HIP(hipMemcpyAsync(c->d_rp_hids, c->d_dn_ids, sizeof(int2) * n, hipMemcpyDeviceToDevice, cs));
  // The next frame's ACCUMULATE waits for reset_ev (render_impl), its tracing does not: the capture reads the accumulator, nothing a frame's tracing reads or writes.
  if (!c->reset_ev) CRH_HIP(hipEventCreateWithFlags(&c->reset_ev, hipEventDisableTiming));
  CRH_HIP(hipEventRecord(c->reset_ev, cs)); c->reset_pending = true;
  if (int rc = fork_from_context(c)) return rc;          // the side stream rewrites the guide for the next view: behind the two copies
  c->stream_uses = uses;
  c->rp_frame = frame_of(S); c->rp_w = W; c->rp_h = H; c->rp_cur = other;
  c->rp_valid = c->rp_fresh = c->rp_captured = true;
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

void crh_reproject_defaults(crh_reproject_params* p)
{
  if (!p) return;
  p->max_history = 16.f;
  p->until_samples = 64u;
  p->normal_cos = 0.90630778704f;      // cos 25 deg
  p->depth_ratio = 1.05f;
}

int crh_set_reproject(crh_ctx* c, const crh_reproject_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) { c->rp_on = false; reproject_drop(c); return CRH_OK; }
  if (const char* why = params_refused(p)) { std::string m = std::string("crh_set_reproject: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  c->rp_par = *p; c->rp_on = true;      // read by crh_set_camera, the LDR read-outs and crh_read_reprojected only
  return CRH_OK;
}

int crh_get_reproject(crh_ctx* c, crh_reproject_params* out, int* on, int* valid)
{
  if (!c) return CRH_E_INVALID;
  if (out) *out = params_in_force(c);
  if (on) *on = c->rp_on ? 1 : 0;
  if (valid) *valid = history_valid(c) ? 1 : 0;
  return CRH_OK;
}

int crh_read_reprojected(crh_ctx* c, float* rgba_out)
{
  if (!c || !rgba_out) return fail(c, CRH_E_INVALID, "crh_read_reprojected: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  c->read_since_render = true;
  CRH_HIP(hipSetDevice(c->device));
  const float4* shown = nullptr;
  hipStream_t on = cstream(c);
  if (int rc = reproject_src(c, on, display_source(c), 0, &shown)) return rc;
  CRH_HIP(hipMemcpyAsync(rgba_out, shown, sizeof(float4) * (size_t)c->par.width * c->par.height, hipMemcpyDeviceToHost, on));
  CRH_HIP(hipStreamSynchronize(on));
  return CRH_OK;
}

int crh_bench_reproject(crh_ctx* c, uint32_t repeats, float* resolve_ms, float* capture_ms)
{
  if (!c || !repeats) return fail(c, CRH_E_INVALID, "crh_bench_reproject: no repeats");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  const ReprojectRule R = rule_of(params_in_force(c));
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = ensure_guide(c)) return rc;
  hipStream_t on = cstream(c);
  CRH_HIP(hipStreamSynchronize(on));
  const uint32_t W = c->par.width, H = c->par.height;
  const size_t n = (size_t)W * H;
  // this call's own blocks, released when it returns: the output image, the capture's guide copies, a stand-in history where there is none
  DevBuf<float4> d_out, d_himg, d_hguide_cp; DevBuf<int2> d_hids_cp;
  CRH_HIP(d_out.reserve(n)); CRH_HIP(d_hguide_cp.reserve(n)); CRH_HIP(d_hids_cp.reserve(n));
  const float4* src = display_source(c);
  ReprojectHistory hist = history_of(c);
  if (!hist.valid) {                                     // the current view as its own history: the identity reprojection
    CRH_HIP(d_himg.reserve(n));
    CRH_HIP(hipMemcpyAsync(d_himg, src, sizeof(float4) * n, hipMemcpyDeviceToDevice, on));
    DScene S; fill_scene(c, S);
    hist.img = d_himg; hist.guide = c->d_dn_guide; hist.ids = c->d_dn_ids; hist.frame = frame_of(S); hist.valid = 1;
  }
  resolve(c, on, src, hist, R, d_out);                   // the code is loaded
  hipError_t e = time_launches(on, repeats, [&] { resolve(c, on, src, hist, R, d_out); return hipGetLastError(); }, resolve_ms);
  if (e == hipSuccess) e = time_launches(on, repeats, [&] {
    resolve(c, on, src, hist, R, d_out);
    hipError_t ec = hipGetLastError();
    if (ec == hipSuccess) ec = hipMemcpyAsync(d_hguide_cp, c->d_dn_guide, sizeof(float4) * n, hipMemcpyDeviceToDevice, on);
    if (ec == hipSuccess) ec = hipMemcpyAsync(d_hids_cp, c->d_dn_ids, sizeof(int2) * n, hipMemcpyDeviceToDevice, on);
    return ec;
  }, capture_ms);
  CRH_HIP(e);                                            // (time_launches has waited for the stream: this call's blocks may go)
  return CRH_OK;
}

int crh_reproject_frame_host(const crh_camera* cam, uint32_t width, uint32_t height, crh_reproject_frame* out)
{
  if (!cam || !out) return CRH_E_INVALID;
  const float v[] = {cam->eye[0], cam->eye[1], cam->eye[2], cam->dir[0], cam->dir[1], cam->dir[2], cam->up[0], cam->up[1], cam->up[2], cam->fovy_deg, cam->aspect, cam->ortho_scale};
  if (!all_finite(v, sizeof v / sizeof v[0], 1.0e30f)) return CRH_E_INVALID;
  if (!(cam->aspect > 0.f) && (!width || !height)) return CRH_E_INVALID;
  const CameraFrame f = camera_frame(*cam, width, height);      // what fill_scene puts into the kernels' DScene
  DScene S{};
  S.eye = crh_mk3(cam->eye[0], cam->eye[1], cam->eye[2]); S.fwd = f.fwd; S.right = f.right; S.up = f.up;
  S.tan_half = f.tan_half; S.aspect = f.aspect;
  S.ortho_scale = cam->ortho_scale; S.is_ortho = cam->is_ortho;
  *out = frame_of(S);
  return CRH_OK;
}

int crh_reproject_host(const float* accum_rgba, const float* rays_px, const int32_t* object_px, const int32_t* triangle_px, const float* t_px, const float* hist_rgba,
                       const int32_t* hist_object, const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame* hist_cam, const void* table, uint32_t n_tri,
                       uint32_t width, uint32_t height, const crh_reproject_params* p, float* rgba_out)
{
  if (!accum_rgba || !rays_px || !object_px || !triangle_px || !t_px || !rgba_out || !p || !width || !height || (n_tri && !table)) return CRH_E_INVALID;
  if (hist_rgba && (!hist_object || !hist_triangle || !hist_t || !hist_cam)) return CRH_E_INVALID;
  if (params_refused(p)) return CRH_E_INVALID;
  const size_t n = (size_t)width * height;
  std::vector<OutlineTri> tb; std::vector<float4> in, hist, out;      // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, table, n_tri) || aligned_copy(in, accum_rgba, n) || aligned_copy(out, nullptr, n) || aligned_copy(hist, hist_rgba, hist_rgba ? n : 0)) return CRH_E_NOMEM;
  crh_reproject_frame F{}; if (hist_rgba) F = *hist_cam;
  reproject_host(in.data(), rays_px, object_px, triangle_px, t_px, hist_rgba ? hist.data() : nullptr, hist_object, hist_triangle, hist_t, F, tb.data(), n_tri, width, height,
                 rule_of(*p), out.data());
  std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
  return CRH_OK;
}

}  // extern "C"
