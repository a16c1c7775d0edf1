// crh_reproject.cpp -- reprojected display history: the application restarts the accumulation on every camera change (reference src/Launcher/AppViewer.cxx:979-984) and
// shows one Redraw() per GUI frame (:1045-1047), so during a drag every image has one sample and everything rendered one frame earlier, from a camera a fraction of a
// degree away, is thrown away.  Here crh_set_camera keeps what the ending view DISPLAYED -- image, guide, camera frame -- and the LDR read-outs of the next view fetch it
// through the first-hit point of every pixel and blend it with the new accumulator, in front of the denoise filter.  The reference has no counterpart.
// One kernel (reproject_kernels.hip); the rule has ONE copy (reproject_kernels.h), compiled for the kernel and for the host twin below.  Display state: nothing of the
// rendering state is touched, and only the source of the filter / the tone map changes.  DESIGN.md section 4.13.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include <cfloat>
#include <cmath>
#include <cstddef>

#include "crh_context.h"
#include "reproject_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_reproject_params) == 16, "crh_reproject_params is 16 bytes");
static_assert(sizeof(crh_reproject_frame) == 64, "crh_reproject_frame is 64 bytes");
static_assert(sizeof(crh_reproject_motion_params) == 8, "crh_reproject_motion_params is 8 bytes");
static_assert(offsetof(crh_reproject_delta, flag) == 48 && offsetof(ReprojectDelta, flag) == 48, "a delta record: twelve floats, the flag, three pad words");

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

const char* motion_refused(const crh_reproject_motion_params* p)
{
  const float f[] = {p->max_history_moved, p->max_history_static};
  if (!all_finite(f, 2)) return "max_history_moved / max_history_static hold a NaN / Inf";
  if (!(p->max_history_moved >= 1.f && p->max_history_moved <= 1024.f)) return "max_history_moved lies outside 1..1024";
  if (!(p->max_history_static >= 1.f && p->max_history_static <= 1024.f)) return "max_history_static lies outside 1..1024";
  return nullptr;
}

crh_reproject_motion_params motion_in_force(const crh_ctx* c)
{
  crh_reproject_motion_params p; crh_reproject_motion_defaults(&p);
  if (c->rpm_on) p = c->rpm_par;
  return p;
}

// THE DELTA TABLE, record k (the header's text, line by line): everything in double, one operation at a time (-ffp-contract=off), each result rounded once to float
struct D3 { double x, y, z; };
inline D3 cross_d(const D3& a, const D3& b)
{
  const double p0 = a.y * b.z, m0 = a.z * b.y, p1 = a.z * b.x, m1 = a.x * b.z, p2 = a.x * b.y, m2 = a.y * b.x;
  return D3{p0 - m0, p1 - m1, p2 - m2};
}
inline double dot_d(const D3& a, const D3& b) { const double p0 = a.x * b.x, p1 = a.y * b.y, p2 = a.z * b.z; return (p0 + p1) + p2; }

// e rounded once to float32 (to nearest, ties to even) in *f; false when the result is not finite.  No conversion of a value outside float's range is ever made:
// 0x1.ffffffp+127 = FLT_MAX + half an ulp is where rounding reaches Inf, and what lies between FLT_MAX and that rounds to FLT_MAX.
inline bool round_to_float(double e, float* f)
{
  if (!(std::fabs(e) < 0x1.ffffffp+127)) return false;   // NaN, Inf, or rounds to Inf
  if (std::fabs(e) > (double)FLT_MAX) { *f = e < 0.0 ? -FLT_MAX : FLT_MAX; return true; }
  *f = (float)e;
  return true;
}

void delta_record(const float* A, const float* M, crh_reproject_delta* out)
{
  std::memset(out, 0, sizeof *out);
  if (std::memcmp(A, M, 12 * sizeof(float)) == 0) return;                     // flag 0
  out->flag = 2u;
  const D3 r0{M[0], M[1], M[2]}, r1{M[4], M[5], M[6]}, r2{M[8], M[9], M[10]}, t{M[3], M[7], M[11]};
  const D3 c0 = cross_d(r1, r2), c1 = cross_d(r2, r0), c2 = cross_d(r0, r1);
  const double det = dot_d(r0, c0);
  if (det == 0.0 || !std::isfinite(det)) return;
  const D3 i[3] = {D3{c0.x / det, c1.x / det, c2.x / det}, D3{c0.y / det, c1.y / det, c2.y / det}, D3{c0.z / det, c1.z / det, c2.z / det}};
  const double u[3] = {-dot_d(i[0], t), -dot_d(i[1], t), -dot_d(i[2], t)};
  const double im[3][3] = {{i[0].x, i[0].y, i[0].z}, {i[1].x, i[1].y, i[1].z}, {i[2].x, i[2].y, i[2].z}};
  float D[12];
  for (int j = 0; j < 3; ++j) {
    const double a0 = A[4 * j], a1 = A[4 * j + 1], a2 = A[4 * j + 2], a3 = A[4 * j + 3];
    for (int m = 0; m < 3; ++m) {
      const double p0 = a0 * im[0][m], p1 = a1 * im[1][m], p2 = a2 * im[2][m];
      const double e = (p0 + p1) + p2;
      if (!round_to_float(e, &D[4 * j + m])) return;                           // not finite after the rounding: flag 2
    }
    const double q0 = a0 * u[0], q1 = a1 * u[1], q2 = a2 * u[2];
    const double e = ((q0 + q1) + q2) + a3;
    if (!round_to_float(e, &D[4 * j + 3])) return;
  }
  std::memcpy(out->D, D, sizeof D); out->flag = 1u;
}

// The table of (X_hist, the transforms in force) on the host, its flagged count, and -- only while a record is flagged -- its bytes on the device: stream-ordered on
// the context's stream, so behind a capture's resolve that still reads the old table; a read-back in flight that reads it is waited for first.
int motion_rebuild(crh_ctx* c)
{
  c->rpm_flagged = 0;
  const size_t nO = c->two_level ? c->nO : 0u;
  if (!c->rpm_on || !nO || c->rpm_xf_hist.size() != 12 * nO || c->xf.size() != 12 * nO) { c->rpm_table.clear(); return CRH_OK; }
  c->rpm_table.resize(nO);
  uint32_t moved = 0;
  for (size_t k = 0; k < nO; ++k) {
    delta_record(&c->rpm_xf_hist[12 * k], &c->xf[12 * k], &c->rpm_table[k]);
    if (c->rpm_table[k].flag) ++c->rpm_flagged;
    if (c->rpm_table[k].flag == 1u) c->rpm_table[k].pad[0] = moved++;      // the device copy only: the record's slot among the flag-1 records (the staged form)
  }
  c->rpm_stageable = moved <= kReprojectStagedMax; c->rpm_n_staged = c->rpm_stageable ? moved : 0u;
  if (!c->rpm_flagged) return CRH_OK;
  std::vector<crh_reproject_delta> up(c->rpm_table);      // the table, then -- for the staged form -- the flag-1 records again, in slot order
  if (c->rpm_staged && c->rpm_stageable) for (size_t k = 0; k < nO; ++k) if (c->rpm_table[k].flag == 1u) up.push_back(c->rpm_table[k]);
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = wait_overlay_readers(c)) return rc;
  const size_t bytes = sizeof(crh_reproject_delta) * up.size();
  if (bytes > c->d_rpm_table.bytes()) { CRH_HIP(hipStreamSynchronize(cstream(c))); CRH_HIP(c->d_rpm_table.reserve(bytes, bytes / 4)); }
  if (bytes <= (4u << 20)) return stage_copy(c, c->d_rpm_table, up.data(), bytes);
  CRH_HIP(hipMemcpyAsync(c->d_rpm_table, up.data(), bytes, hipMemcpyHostToDevice, cstream(c))); CRH_HIP(hipStreamSynchronize(cstream(c)));
  return CRH_OK;
}

// the motion kernel in the form in force: the LDS-staged one only where it was asked for and the flag-1 records fit
void launch_motion(hipStream_t on, const DScene& S, const float4* guide, const int2* ids, const float4* src, const ReprojectHistory& hist, const ReprojectRule& R,
                   const ReprojectMotion& M, bool staged, uint32_t n_staged, float4* out)
{
  if (staged) launch_reproject_resolve_motion_staged(on, S, guide, ids, src, hist, R, M, n_staged, out);
  else launch_reproject_resolve_motion(on, S, guide, ids, src, hist, R, M, out);
}

// the table a resolve issued now takes: flagged records, a valid history, both features on (else none: the plain kernel)
bool motion_in_use(const crh_ctx* c) { return c->rpm_on && c->rpm_flagged > 0 && c->rpm_table.size() == c->nO && c->d_rpm_table; }

ReprojectMotion motion_of(const crh_ctx* c)
{
  ReprojectMotion M;
  M.table = c->d_rpm_table.as<ReprojectDelta>(); M.n_objects = (uint32_t)c->rpm_table.size();
  M.max_moved = c->rpm_par.max_history_moved; M.max_static = c->rpm_par.max_history_static; M.capped = 1;
  return M;
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
  const bool motion = hist.valid && motion_in_use(c);
  if (motion) launch_motion(on, S, c->d_dn_guide, c->d_dn_ids, src, hist, R, motion_of(c), c->rpm_staged && c->rpm_stageable, c->rpm_n_staged, out);
  else launch_reproject_resolve(on, S, c->d_dn_guide, c->d_dn_ids, src, hist, R, out);      // no flagged record: the plain kernel, its bytes and its time
  ++c->rp_launches[motion ? 1 : 0];
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
namespace {
// The capture itself, the conditions of the calling setter apart: `have` = a valid history exists
int capture(crh_ctx* c, bool have)
{
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
  resolve(c, cs, display_source(c), history_of(c), rule_of(c->rp_par), c->d_rp_hist[other]);      // reads the OLD guide copy (and the table in force) ...
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
  if (c->rpm_on) { c->rpm_xf_hist = c->two_level ? c->xf : std::vector<float>(); return motion_rebuild(c); }      // X_hist = the transforms in force: no record is flagged
  return CRH_OK;
}
}  // namespace

int reproject_capture(crh_ctx* c, const crh_camera* next)
{
  if (!c->rp_on || !c->built || c->rp_captured || c->spec.raygen_bilinear != 0) return CRH_OK;
  if (std::memcmp(next, &c->cam, sizeof(crh_camera)) == 0) return CRH_OK;
  const bool have = history_valid(c);
  if (!(c->frames_done > 0 || have)) return CRH_OK;
  return capture(c, have);
}

int reproject_transforms_begin(crh_ctx* c, const float* xf)
{
  if (!c->rp_on || !c->rpm_on || !c->built) return CRH_OK;
  const bool differ = c->xf.size() != 12 * (size_t)c->nO || std::memcmp(xf, c->xf.data(), sizeof(float) * c->xf.size()) != 0;
  if (differ && !c->rp_captured && c->spec.raygen_bilinear == 0 && c->frames_done > 0)
    if (int rc = capture(c, history_valid(c))) return rc;
  c->rp_keep_restart = history_valid(c);                 // the restart inside crh_set_transforms keeps what is valid now
  return CRH_OK;
}

int reproject_transforms_set(crh_ctx* c)
{
  c->rp_keep_restart = false;
  if (!c->rp_on || !c->rpm_on || !c->built) return CRH_OK;
  return motion_rebuild(c);
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
  // k_reproject_resolve itself, whatever table is in force: crh_bench_reproject_motion times the other kernel, and the two are compared
  auto plain = [&] { DScene S; fill_scene(c, S); launch_reproject_resolve(on, S, c->d_dn_guide, c->d_dn_ids, src, hist, R, d_out); };
  plain();                                               // the code is loaded
  hipError_t e = time_launches(on, repeats, [&] { plain(); return hipGetLastError(); }, resolve_ms);
  if (e == hipSuccess) e = time_launches(on, repeats, [&] {
    plain();
    hipError_t ec = hipGetLastError();
    if (ec == hipSuccess) ec = hipMemcpyAsync(d_hguide_cp, c->d_dn_guide, sizeof(float4) * n, hipMemcpyDeviceToDevice, on);
    if (ec == hipSuccess) ec = hipMemcpyAsync(d_hids_cp, c->d_dn_ids, sizeof(int2) * n, hipMemcpyDeviceToDevice, on);
    return ec;
  }, capture_ms);
  CRH_HIP(e);                                            // (time_launches has waited for the stream: this call's blocks may go)
  return CRH_OK;
}

void crh_reproject_motion_defaults(crh_reproject_motion_params* p)
{
  if (!p) return;
  p->max_history_moved = 16.f;
  p->max_history_static = 8.f;
}

int crh_set_reproject_motion(crh_ctx* c, const crh_reproject_motion_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) {
    if (c->rpm_on && c->rpm_flagged) reproject_drop(c);  // the history of a moved object no longer fits the plain rule
    c->rpm_on = false; c->rpm_flagged = 0;
    c->rpm_xf_hist.clear(); c->rpm_table.clear();
    return CRH_OK;
  }
  if (const char* why = motion_refused(p)) { std::string m = std::string("crh_set_reproject_motion: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  c->rpm_par = *p;
  if (c->rpm_on) return CRH_OK;
  // Switched on: with the feature off every transform change had dropped the history, so a valid history was taken under the transforms in force -- no record
  // is flagged, nothing is uploaded
  c->rpm_on = true;
  c->rpm_xf_hist = c->two_level ? c->xf : std::vector<float>();
  c->rpm_table.clear(); c->rpm_flagged = 0;
  return CRH_OK;
}

int crh_get_reproject_motion(crh_ctx* c, crh_reproject_motion_params* out, int* on, uint32_t* n_flagged)
{
  if (!c) return CRH_E_INVALID;
  if (out) *out = motion_in_force(c);
  if (on) *on = c->rpm_on ? 1 : 0;
  if (n_flagged) *n_flagged = (c->rp_on && c->built && history_valid(c) && motion_in_use(c)) ? c->rpm_flagged : 0u;
  return CRH_OK;
}

int crh_get_reproject_launches(crh_ctx* c, uint64_t* plain, uint64_t* motion)
{
  if (!c) return CRH_E_INVALID;
  if (plain) *plain = c->rp_launches[0];
  if (motion) *motion = c->rp_launches[1];
  return CRH_OK;
}

int crh_bench_reproject_motion(crh_ctx* c, uint32_t repeats, float* resolve_ms)
{
  if (!c || !repeats) return fail(c, CRH_E_INVALID, "crh_bench_reproject_motion: no repeats");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  const ReprojectRule R = rule_of(params_in_force(c));
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = ensure_guide(c)) return rc;
  hipStream_t on = cstream(c);
  CRH_HIP(hipStreamSynchronize(on));
  const uint32_t W = c->par.width, H = c->par.height;
  const size_t n = (size_t)W * H;
  DevBuf<float4> d_out, d_himg; DevBuf<void> d_table;      // this call's own blocks, released when it returns
  CRH_HIP(d_out.reserve(n));
  const float4* src = display_source(c);
  ReprojectHistory hist = history_of(c);
  if (!hist.valid) {                                     // the current view as its own history: the identity reprojection
    CRH_HIP(d_himg.reserve(n));
    CRH_HIP(hipMemcpyAsync(d_himg, src, sizeof(float4) * n, hipMemcpyDeviceToDevice, on));
    DScene S; fill_scene(c, S);
    hist.img = d_himg; hist.guide = c->d_dn_guide; hist.ids = c->d_dn_ids; hist.frame = frame_of(S); hist.valid = 1;
  }
  ReprojectMotion M;
  const crh_reproject_motion_params mp = motion_in_force(c);
  bool staged = c->rpm_staged && c->rpm_stageable; uint32_t n_staged = c->rpm_n_staged;
  if (c->rp_on && history_valid(c) && motion_in_use(c)) M = motion_of(c);
  else {                                                 // the stand-in: every object flagged with its exact identity delta
    const uint32_t nO = n_pick_objects(c);
    staged = c->rpm_staged && nO <= kReprojectStagedMax; n_staged = staged ? nO : 0u;
    std::vector<crh_reproject_delta> tab(nO);
    for (uint32_t k = 0; k < nO; ++k) { crh_reproject_delta& r = tab[k]; std::memset(&r, 0, sizeof r); r.D[0] = r.D[5] = r.D[10] = 1.f; r.flag = 1u; r.pad[0] = k; }
    if (staged) tab.insert(tab.end(), tab.begin(), tab.begin() + nO);      // the records again, in slot order: what the staged form copies into LDS
    CRH_HIP(d_table.reserve(sizeof(crh_reproject_delta) * tab.size()));
    CRH_HIP(hipMemcpyAsync(d_table, tab.data(), sizeof(crh_reproject_delta) * tab.size(), hipMemcpyHostToDevice, on));
    CRH_HIP(hipStreamSynchronize(on));                   // (`tab` is pageable and goes out of scope)
    M.table = d_table.as<ReprojectDelta>(); M.n_objects = nO; M.max_moved = mp.max_history_moved; M.max_static = mp.max_history_static; M.capped = 1;
  }
  DScene S; fill_scene(c, S);
  auto launch = [&] { launch_motion(on, S, c->d_dn_guide, c->d_dn_ids, src, hist, R, M, staged, n_staged, d_out); return hipGetLastError(); };
  hipError_t e = launch();                               // the code is loaded
  if (e == hipSuccess) e = time_launches(on, repeats, launch, resolve_ms);
  else hipStreamSynchronize(on);
  CRH_HIP(e);                                            // (the stream has been waited for: this call's blocks may go)
  return CRH_OK;
}

int crh_reproject_delta_host(const float* xf_hist, const float* xf_cur, uint32_t n_objects, void* table_out)
{
  if (!n_objects) return CRH_OK;
  if (!xf_hist || !xf_cur || !table_out) return CRH_E_INVALID;
  for (uint32_t k = 0; k < n_objects; ++k) {
    crh_reproject_delta r;
    delta_record(xf_hist + 12 * (size_t)k, xf_cur + 12 * (size_t)k, &r);
    std::memcpy((char*)table_out + sizeof r * (size_t)k, &r, sizeof r);      // (the caller's bytes need not be aligned)
  }
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

int crh_reproject_motion_host(const float* accum_rgba, const float* rays_px, const int32_t* object_px, const int32_t* triangle_px, const float* t_px,
                              const float* hist_rgba, const int32_t* hist_object, const int32_t* hist_triangle, const float* hist_t,
                              const crh_reproject_frame* hist_cam, const void* table, uint32_t n_tri, uint32_t width, uint32_t height,
                              const crh_reproject_params* p, const void* delta_table, uint32_t n_objects, const crh_reproject_motion_params* mp, float* rgba_out)
{
  if (!accum_rgba || !rays_px || !object_px || !triangle_px || !t_px || !rgba_out || !p || !width || !height || (n_tri && !table)) return CRH_E_INVALID;
  if (hist_rgba && (!hist_object || !hist_triangle || !hist_t || !hist_cam)) return CRH_E_INVALID;
  if (params_refused(p)) return CRH_E_INVALID;
  if (n_objects && !delta_table) return CRH_E_INVALID;
  if (delta_table && (!mp || motion_refused(mp))) return CRH_E_INVALID;
  const size_t n = (size_t)width * height;
  std::vector<OutlineTri> tb; std::vector<float4> in, hist, out; std::vector<ReprojectDelta> dt;      // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, table, n_tri) || aligned_copy(in, accum_rgba, n) || aligned_copy(out, nullptr, n) || aligned_copy(hist, hist_rgba, hist_rgba ? n : 0) ||
      aligned_copy(dt, delta_table, delta_table ? n_objects : 0)) return CRH_E_NOMEM;
  ReprojectMotion M;
  if (delta_table && n_objects) {
    M.table = dt.data(); M.n_objects = n_objects; M.max_moved = mp->max_history_moved; M.max_static = mp->max_history_static;
    for (const ReprojectDelta& r : dt) { if (r.flag > 2u) return CRH_E_INVALID; if (r.flag) M.capped = 1; }
  }
  crh_reproject_frame F{}; if (hist_rgba) F = *hist_cam;
  reproject_motion_host(in.data(), rays_px, object_px, triangle_px, t_px, hist_rgba ? hist.data() : nullptr, hist_object, hist_triangle, hist_t, F, tb.data(), n_tri, width, height,
                        rule_of(*p), M, out.data());
  std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
  return CRH_OK;
}

}  // extern "C"
