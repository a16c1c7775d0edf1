// crh_annotate.cpp -- annotations: the helpers an application draws over the path-traced frame -- the manipulator at the selection's pivot (ImGuizmo::Manipulate,
// reference src/ImGui/ImRaytraceControls.cxx:64), a marker at every positional light (DrawLights, :93-111), a grid, an axis triad, the selection's box -- as ONE
// primitive: a list of coloured world-space segments, projected, binned and drawn by the LDR read-outs as the last stage of the display chain, each hidden, dimmed or
// left on top where the first-hit id buffer says the scene is nearer.  The reference paints them with ImGui over the image and knows nothing of occlusion.
// Three kernels (annotate_kernels.hip); the rules have ONE copy (annotate_kernels.h), compiled for the kernels and for the host twins below.  Display state: nothing of
// the rendering state is touched.  DESIGN.md section 4.16.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "annotate_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_annot_segment) == 32, "crh_annot_segment is 32 bytes");
static_assert(sizeof(crh_annot_params) == 8, "crh_annot_params is 8 bytes");
static_assert(sizeof(AnnotRecord) == 32, "the screen record is 32 bytes");
static_assert(kAnnotOnTop == CRH_ANNOT_ON_TOP && kAnnotHide == CRH_ANNOT_HIDE && kAnnotXray == CRH_ANNOT_XRAY && kAnnotMaxSegments == CRH_ANNOT_MAX_SEGMENTS, "the constants of the header");

namespace {

std::string params_refused(const crh_annot_params* p)
{
  if (!all_finite(&p->depth_bias, 1)) return "depth_bias holds a NaN / Inf";
  if (!(p->depth_bias >= 0.f)) return "depth_bias is negative";
  if (p->hidden_alpha > 255u) return "hidden_alpha lies above 255";
  return {};
}

// why this list cannot be drawn (empty: it can); *depth: some segment has mode HIDE or XRAY
std::string list_refused(const crh_annot_segment* segs, uint32_t n, bool* depth)
{
  if (n > kAnnotMaxSegments) return "more than 65536 segments";
  bool d = false;
  for (uint32_t i = 0; i < n; ++i) {
    const crh_annot_segment& s = segs[i];
    const char* why = nullptr;
    const float f[6] = {s.a[0], s.a[1], s.a[2], s.b[0], s.b[1], s.b[2]};
    if (s.style & ~kAnnotStyleBits) why = "unknown bits in style";
    else if (annot_width(s.style) < 1u || annot_width(s.style) > kAnnotMaxWidth) why = "the width lies outside 1..8";
    else if (annot_mode(s.style) > kAnnotXray) why = "the mode is none of CRH_ANNOT_ON_TOP / _HIDE / _XRAY";
    else if (!all_finite(f, 6)) why = "a coordinate is a NaN / Inf";
    if (why) { char b[128]; snprintf(b, sizeof b, "segment %u: %s", i, why); return b; }
    d = d || annot_mode(s.style) != kAnnotOnTop;
  }
  if (depth) *depth = d;
  return {};
}

AnnotCam cam_of(const crh_camera& cam, uint32_t W, uint32_t H)
{
  const CameraFrame f = camera_frame(cam, W, H);      // what fill_scene puts into the kernels' DScene
  AnnotCam C{};
  for (int k = 0; k < 3; ++k) C.eye[k] = cam.eye[k];
  C.right[0] = f.right.x; C.right[1] = f.right.y; C.right[2] = f.right.z;
  C.up[0] = f.up.x; C.up[1] = f.up.y; C.up[2] = f.up.z;
  C.fwd[0] = f.fwd.x; C.fwd[1] = f.fwd.y; C.fwd[2] = f.fwd.z;
  C.tan_half = f.tan_half; C.aspect = f.aspect; C.ortho_scale = cam.ortho_scale; C.is_ortho = cam.is_ortho ? 1u : 0u; C.W = W; C.H = H;
  return C;
}

crh_annot_params params_in_force(const crh_ctx* c)
{
  crh_annot_params p; crh_annot_defaults(&p);
  if (c->an_on) p = c->an_par;
  return p;
}

bool drawn(const crh_ctx* c) { return c->an_on && !c->an_segs.empty() && c->built; }

// The list on the device, valid when this returns.  Replaced only after the kernels of read-backs in flight that read the old one are done; the synchronous users
// (sets 0 and 2) have waited for their streams themselves.
int ensure_list(crh_ctx* c)
{
  if (c->an_segs_gen == c->an_gen) return CRH_OK;
  int rc = pick_stream(c); if (rc) return rc;
  if ((rc = wait_overlay_readers(c))) return rc;
  const size_t bytes = sizeof(crh_annot_segment) * c->an_segs.size();
  CRH_HIP(c->d_an_segs.reserve(bytes, bytes / 4));
  CRH_HIP(hipMemcpyAsync(c->d_an_segs, c->an_segs.data(), bytes, hipMemcpyHostToDevice, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->an_segs_gen = c->an_gen;
  return CRH_OK;
}

// The records and the bins of set `set` for the list, the camera and the frame size in force, in *D: recomputed on `on` -- the one stream the set is used on -- when
// their stamp differs, in stream order: nothing waits but a block that must grow.
int ensure_derived(crh_ctx* c, hipStream_t on, int set, AnnotDraw* D)
{
  if (int rc = ensure_list(c)) return rc;
  const uint32_t W = c->par.width, H = c->par.height, n = (uint32_t)c->an_segs.size(), E = c->an_tile;
  AnnotDraw d{};
  d.n = n; d.n_words = (n + 31u) / 32u; d.tile = E; d.tiles_x = (W + E - 1u) / E; d.tiles_y = (H + E - 1u) / E;
  d.depth_bias = c->an_par.depth_bias; d.hidden_alpha = c->an_par.hidden_alpha;
  const size_t n_bins = (size_t)d.tiles_x * d.tiles_y * d.n_words;
  AnnotStamp now; now.gen = c->an_gen; now.cam = c->cam; now.w = W; now.h = H; now.tile = E;
  const bool scatter = c->an_bin_form == 2 || (c->an_bin_form == 0 && n > kAnnotGatherMax);
  now.scatter = scatter ? 1u : 0u;
  const bool stale = !(c->an_stamp[set] == now);
  if (stale) {
    c->an_stamp[set] = AnnotStamp{};
    if (int rc = grow_display_scratch(c, set == 1 ? 1 : 0, &c->d_an_rec[set], 1, sizeof(AnnotRecord) * (size_t)n)) return rc;      // (sets 0 and 2: nothing in flight)
    if (int rc = grow_display_scratch(c, set == 1 ? 1 : 0, &c->d_an_bins[set], 1, n_bins)) return rc;
  }
  d.seg = c->d_an_segs.as<const crh_annot_segment>(); d.rec = c->d_an_rec[set].as<const AnnotRecord>(); d.bins = c->d_an_bins[set];
  if (stale) {
    launch_annot_project(on, cam_of(c->cam, W, H), d.seg, n, c->d_an_rec[set].as<AnnotRecord>());
    launch_annot_bin(on, d, scatter, c->d_an_bins[set]);
    CRH_HIP(hipGetLastError());
    c->an_stamp[set] = now;
  }
  *D = d;
  return CRH_OK;
}

// The id plane and the parameter plane of the queries (set 2, the id buffer's stream), valid when this returns
int ensure_plane(crh_ctx* c)
{
  if (c->an_depth) if (int rc = ensure_ids(c)) return rc;
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = pick_stream(c)) return rc;
  AnnotDraw D;
  if (int rc = ensure_derived(c, c->pk_stream, 2, &D)) return rc;
  AnnotStamp now = c->an_stamp[2]; now.ids_gen = c->an_depth ? c->ids_gen : 0;
  if (c->an_plane_stamp == now) return CRH_OK;
  c->an_plane_stamp = AnnotStamp{};
  const size_t n_px = (size_t)c->par.width * c->par.height;
  CRH_HIP(c->d_an_ids.reserve(n_px)); CRH_HIP(c->d_an_s.reserve(n_px));      // (this stream runs synchronously: nothing reads the old blocks)
  D.hit = c->an_depth ? (const float4*)c->d_pk_hit : nullptr;
  DScene S; fill_scene(c, S);
  launch_annot_draw(c->pk_stream, S, D, nullptr, c->d_an_ids, c->d_an_s);
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->an_plane_stamp = now;
  return CRH_OK;
}

}  // namespace

namespace crh {
namespace api {

// Called by the LDR read-outs behind overlay_ldr, on the stream the chain runs on.  Feature off, an empty list or no scene: nothing is launched, nothing is computed,
// nothing is allocated -- the bytes are the chain's.
int annotate_ldr(crh_ctx* c, hipStream_t on, int set, uint8_t* d_ldr)
{
  if (!drawn(c)) return CRH_OK;
  if (c->an_depth) if (int rc = ensure_ids(c)) return rc;      // (synchronous on its own stream: every stream may read the buffer)
  CRH_HIP(hipSetDevice(c->device));
  AnnotDraw D;
  if (int rc = ensure_derived(c, on, set, &D)) return rc;
  D.hit = c->an_depth ? (const float4*)c->d_pk_hit : nullptr;
  DScene S; fill_scene(c, S);
  launch_annot_draw(on, S, D, d_ldr, nullptr, nullptr);
  CRH_HIP(hipGetLastError());
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

void crh_annot_defaults(crh_annot_params* p)
{
  if (!p) return;
  p->depth_bias = 0x1p-9f;
  p->hidden_alpha = 64u;
}

int crh_set_annotations(crh_ctx* c, const crh_annot_segment* segs, uint32_t n, const crh_annot_params* params)
{
  if (!c) return CRH_E_INVALID;
  crh_annot_params p; crh_annot_defaults(&p);
  if (params) p = *params;
  bool depth = false;
  std::string why = params_refused(&p);
  if (why.empty() && segs && n) why = list_refused(segs, n, &depth);
  if (!why.empty()) { why = "crh_set_annotations: " + why; return fail(c, CRH_E_INVALID, why.c_str()); }
  const bool on = segs && n;
  std::vector<crh_annot_segment> copy;
  if (on) { try { copy.assign(segs, segs + n); } catch (const std::bad_alloc&) { return fail(c, CRH_E_NOMEM, "no memory for the annotation list"); } }
  c->an_segs.swap(copy);      // read by the LDR read-outs and the annotation queries only
  c->an_on = on; c->an_par = p; c->an_depth = depth;
  ++c->an_gen;
  return CRH_OK;
}

int crh_get_annotations(crh_ctx* c, crh_annot_segment* segs_out, uint32_t capacity, uint32_t* n, crh_annot_params* params_out, int* on)
{
  if (!c) return CRH_E_INVALID;
  const uint32_t have = c->an_on ? (uint32_t)c->an_segs.size() : 0u;
  if (segs_out && have) std::memcpy(segs_out, c->an_segs.data(), sizeof(crh_annot_segment) * std::min(have, capacity));
  if (n) *n = have;
  if (params_out) *params_out = params_in_force(c);
  if (on) *on = c->an_on ? 1 : 0;
  return CRH_OK;
}

int crh_read_annotation_ids(crh_ctx* c, int32_t* seg_px)
{
  if (!c || !seg_px) return fail(c, CRH_E_INVALID, "crh_read_annotation_ids: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  const size_t n_px = (size_t)c->par.width * c->par.height;
  if (!drawn(c)) { std::fill(seg_px, seg_px + n_px, -1); return CRH_OK; }
  if (int rc = ensure_plane(c)) return rc;
  CRH_HIP(hipMemcpyAsync(seg_px, c->d_an_ids, 4 * n_px, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  return CRH_OK;
}

int crh_pick_annotation(crh_ctx* c, uint32_t x, uint32_t y, int32_t* segment, float* s)
{
  if (!c) return CRH_E_INVALID;
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (x >= c->par.width || y >= c->par.height) return fail(c, CRH_E_INVALID, "pixel outside the render target");
  int32_t seg = -1; float par = 0.f;
  if (drawn(c)) {
    if (int rc = ensure_plane(c)) return rc;
    const size_t p = (size_t)y * c->par.width + x;
    CRH_HIP(hipMemcpyAsync(&seg, c->d_an_ids + p, 4, hipMemcpyDeviceToHost, c->pk_stream));
    CRH_HIP(hipMemcpyAsync(&par, c->d_an_s + p, 4, hipMemcpyDeviceToHost, c->pk_stream));
    CRH_HIP(hipStreamSynchronize(c->pk_stream));
  }
  if (segment) *segment = seg;
  if (s) *s = seg < 0 ? 0.f : par;
  return CRH_OK;
}

int crh_read_annotation_records(crh_ctx* c, void* records_out)
{
  if (!c) return CRH_E_INVALID;
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!drawn(c)) return CRH_OK;
  if (!records_out) return fail(c, CRH_E_INVALID, "crh_read_annotation_records: null output");
  CRH_HIP(hipSetDevice(c->device));
  if (int rc = pick_stream(c)) return rc;
  AnnotDraw D;
  if (int rc = ensure_derived(c, c->pk_stream, 2, &D)) return rc;
  CRH_HIP(hipMemcpyAsync(records_out, D.rec, sizeof(AnnotRecord) * (size_t)D.n, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  return CRH_OK;
}

int crh_bench_annotations(crh_ctx* c, uint32_t repeats, float* project_ms, float* bin_ms, float* draw_ms)
{
  if (!c) return CRH_E_INVALID;
  if (!repeats) return fail(c, CRH_E_INVALID, "crh_bench_annotations: no repeats");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!drawn(c) || !c->d_accum) return fail(c, CRH_E_INVALID, "crh_bench_annotations: no annotation list / no accumulator");
  c->read_since_render = true;
  CRH_HIP(hipSetDevice(c->device));
  const uint32_t W = c->par.width, H = c->par.height;
  DevBuf<uint8_t> d_full;      // this call's own block, released when it returns: the frame as a read-out issued now would show it
  CRH_HIP(d_full.reserve(3 * (size_t)W * H));
  Launch L{cstream(c), c->grid, false};
  if (int rc = enqueue_display_chain(c, L, 0, 0, d_full)) { hipStreamSynchronize(L.stream); return rc; }      // (the code is loaded, set 0 is valid)
  AnnotDraw D;
  if (int rc = ensure_derived(c, L.stream, 0, &D)) { hipStreamSynchronize(L.stream); return rc; }
  D.hit = c->an_depth ? (const float4*)c->d_pk_hit : nullptr;
  DScene S; fill_scene(c, S);
  const AnnotCam cam = cam_of(c->cam, W, H);
  AnnotRecord* rec = c->d_an_rec[0].as<AnnotRecord>(); uint32_t* bins = c->d_an_bins[0]; const bool scatter = c->an_stamp[0].scatter != 0u;
  hipError_t e = time_launches(L.stream, repeats, [&] { launch_annot_project(L.stream, cam, D.seg, D.n, rec); return hipGetLastError(); }, project_ms);      // (the same values again)
  if (e == hipSuccess) e = time_launches(L.stream, repeats, [&] { launch_annot_bin(L.stream, D, scatter, bins); return hipGetLastError(); }, bin_ms);
  if (e == hipSuccess) e = time_launches(L.stream, repeats, [&] { launch_annot_draw(L.stream, S, D, d_full, nullptr, nullptr); return hipGetLastError(); }, draw_ms);
  CRH_HIP(e);                  // (the stream has been waited for: this call's block may go)
  return CRH_OK;
}

int crh_annot_project_host(const crh_camera* cam, uint32_t width, uint32_t height, const crh_annot_segment* segs, uint32_t n, void* records_out)
{
  if (!cam || !width || !height || (n && (!segs || !records_out))) return CRH_E_INVALID;
  std::vector<crh_annot_segment> sg; std::vector<AnnotRecord> rec;      // (the caller's bytes need not be aligned)
  if (aligned_copy(sg, segs, n) || aligned_copy(rec, nullptr, n)) return CRH_E_NOMEM;
  if (!list_refused(sg.data(), n, nullptr).empty()) return CRH_E_INVALID;
  annot_project_host(cam_of(*cam, width, height), sg.data(), n, rec.data());
  if (n) std::memcpy(records_out, rec.data(), sizeof(AnnotRecord) * (size_t)n);
  return CRH_OK;
}

int crh_annot_draw_host(const void* records, const crh_annot_segment* segs, uint32_t n, const crh_annot_params* params, const crh_camera* cam, uint32_t width,
                        uint32_t height, const float* rays_px, const float* t_px, uint8_t* ldr_inout, int32_t* seg_px_out)
{
  if (!cam || !width || !height || (n && (!records || !segs)) || (!ldr_inout && !seg_px_out)) return CRH_E_INVALID;
  crh_annot_params p; crh_annot_defaults(&p);
  if (params) p = *params;
  if (!params_refused(&p).empty()) return CRH_E_INVALID;
  std::vector<crh_annot_segment> sg; std::vector<AnnotRecord> rec;
  if (aligned_copy(sg, segs, n) || aligned_copy(rec, records, n)) return CRH_E_NOMEM;
  bool depth = false;
  if (!list_refused(sg.data(), n, &depth).empty()) return CRH_E_INVALID;
  if (depth && (!rays_px || !t_px)) return CRH_E_INVALID;
  annot_draw_host(rec.data(), sg.data(), n, p.depth_bias, p.hidden_alpha, cam_of(*cam, width, height), depth ? rays_px : nullptr, depth ? t_px : nullptr, ldr_inout, seg_px_out);
  return CRH_OK;
}

}  // extern "C"
