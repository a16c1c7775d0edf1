// crh_denoise.cpp -- the denoised display: an a-trous filter in front of the tone map of the LDR read-outs, guided by the first-hit id buffer and the per-triangle
// normals of the feature lines' table, so that the 1 - 4 spp frames of a camera drag lose their salt and pepper while object boundaries, creases and depth steps stay
// crisp.  The reference has no counterpart: OCCT's path tracer shows the raw accumulation (AppViewer.cxx:979-984 restarts it on every camera move, :1045-1047 shows it).
// Two kernels (denoise_kernels.hip): the guide -- per pixel what a tap needs, derived from the id buffer and the table, kept until one of them changes -- and one
// pass per level.  The rules have ONE copy (denoise_kernels.h), compiled for the kernels and for the host twin below.  Display state: nothing of the rendering
// state is touched, and only the tone map's source changes.  DESIGN.md section 4.12.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "shade_guide_kernels.h"      // (includes denoise_kernels.h) the guided pass, taken while crh_set_shade_guide is on

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_denoise_params) == 16, "crh_denoise_params is 16 bytes");
static_assert(sizeof(float4) == 16 && sizeof(int2) == 8, "the guide record is 16 + 8 bytes");

namespace {

const char* params_refused(const crh_denoise_params* p)
{
  const float f[] = {p->normal_cos, p->depth_ratio};
  if (!all_finite(f, 2)) return "normal_cos / depth_ratio hold a NaN / Inf";
  if (p->levels < 1u || p->levels > kDenoiseMaxLevels) return "levels lies outside 1..5";
  if (!(p->normal_cos > 0.f && p->normal_cos <= 1.f)) return "normal_cos lies outside (0, 1]";
  if (!(p->depth_ratio >= 1.f)) return "depth_ratio is below 1";
  if (p->until_samples < 1u || p->until_samples > (1u << 20)) return "until_samples lies outside 1..2^20";
  return nullptr;
}

crh_denoise_params params_in_force(const crh_ctx* c)
{
  crh_denoise_params p; crh_denoise_defaults(&p);
  if (c->dn_on) p = c->dn_par;
  return p;
}

DenoiseRule rule_of(const crh_denoise_params& p) { return DenoiseRule{p.levels, p.normal_cos, p.depth_ratio, (float)p.until_samples}; }      // (2^20 is exact)

// The passes of rule R from `src` through the two images of scratch set `set`, enqueued on `on`; *shown = the image the last pass wrote.
int filter(crh_ctx* c, hipStream_t on, const float4* src, int set, const DenoiseRule& R, const float4** shown)
{
  if (int rc = ensure_guide(c)) return rc;
  const bool guided = c->sg_on;                          // the shade guide (crh_shade_guide.cpp): off -- nothing of it is allocated, nothing launched
  if (guided) if (int rc = ensure_shade_plane(c)) return rc;
  const uint32_t W = c->par.width, H = c->par.height;
  const size_t n = (size_t)W * H;
  DevBuf<float4>* img = c->d_dn_img[set];
  if (int rc = grow_display_scratch(c, set, img, 2, n)) return rc;
  const float4* in = src;
  for (uint32_t k = 0; k < R.levels; ++k) {
    float4* out = img[k & 1u];
    if (guided) launch_denoise_pass_guided(on, c->d_dn_guide, c->d_dn_ids, c->d_sg_plane, in, out, W, H, k, R);
    else launch_denoise_pass(on, c->d_dn_guide, c->d_dn_ids, in, out, W, H, k, R, c->dn_staged);
    in = out;
  }
  CRH_HIP(hipGetLastError());
  *shown = in;
  return CRH_OK;
}

}  // namespace

namespace crh {
namespace api {

// The guide of the state in force, on the device, valid when this returns (computed on the side stream and waited for, as ensure_ids and the outline mask are).
int ensure_guide(crh_ctx* c)
{
  int rc = ensure_ids_and_table(c); if (rc) return rc;
  const uint32_t W = c->par.width, H = c->par.height;
  const DerivedStamp now{c->ids_gen, c->ol_table_gen, W, H, {0u, 0u}};
  if (c->dn_guide_stamp == now) return CRH_OK;
  if ((rc = wait_overlay_readers(c))) return rc;         // an asynchronous read-back may still be filtering from the guide
  c->dn_guide_stamp = DerivedStamp{};
  CRH_HIP(c->d_dn_guide.reserve((size_t)W * H)); CRH_HIP(c->d_dn_ids.reserve((size_t)W * H));      // (what read the old blocks has been waited for: the synchronous
  launch_denoise_guide(c->pk_stream, c->d_pk_obj, c->d_pk_hit, W, H, c->d_ol_table.as<const OutlineTri>(), c->ol_n_tri, c->d_dn_guide, c->d_dn_ids);      //  read-outs end with a wait, the readers just above)
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->dn_guide_stamp = now;
  return CRH_OK;
}

// Called by the LDR read-outs between the metering and the tone map, on the stream the tone map runs on.  Feature off or no scene: nothing is allocated, nothing is
// launched -- the tone map reads `src`.
// THE ACCUMULATE GUARD: the asynchronous read-out records its rb_tm event -- the one the next accumulate waits for -- after the tone map and the overlays, so it
// already covers the first pass's read of the accumulator; no event of the filter's own is needed.
int denoise_src(crh_ctx* c, hipStream_t on, const float4* src, int set, const float4** shown)
{
  *shown = src;
  if (!c->dn_on || !c->built) return CRH_OK;
  return filter(c, on, src, set, rule_of(c->dn_par), shown);
}

}  // namespace api
}  // namespace crh

extern "C" {

void crh_denoise_defaults(crh_denoise_params* p)
{
  if (!p) return;
  p->levels = 4u;
  p->normal_cos = 0.90630778704f;      // cos 25 deg
  p->depth_ratio = 1.05f;
  p->until_samples = 256u;
}

int crh_set_denoise(crh_ctx* c, const crh_denoise_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) { c->dn_on = false; return CRH_OK; }
  if (const char* why = params_refused(p)) { std::string m = std::string("crh_set_denoise: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  c->dn_par = *p; c->dn_on = true;      // read by the LDR read-outs and crh_read_denoised only
  return CRH_OK;
}

int crh_get_denoise(crh_ctx* c, crh_denoise_params* out, int* on)
{
  if (!c) return CRH_E_INVALID;
  if (out) *out = params_in_force(c);
  if (on) *on = c->dn_on ? 1 : 0;
  return CRH_OK;
}

int crh_read_denoised(crh_ctx* c, float* rgba_out)
{
  if (!c || !rgba_out) return fail(c, CRH_E_INVALID, "crh_read_denoised: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  c->read_since_render = true;
  CRH_HIP(hipSetDevice(c->device));
  const float4* shown = nullptr;
  hipStream_t on = cstream(c);
  if (int rc = reproject_src(c, on, display_source(c), 0, &shown)) return rc;      // what a read-out's filter receives (crh_reproject.cpp): the accumulator itself while that feature is off
  if (int rc = filter(c, on, shown, 0, rule_of(params_in_force(c)), &shown)) return rc;
  CRH_HIP(hipMemcpyAsync(rgba_out, shown, sizeof(float4) * (size_t)c->par.width * c->par.height, hipMemcpyDeviceToHost, on));
  CRH_HIP(hipStreamSynchronize(on));
  return CRH_OK;
}

int crh_bench_denoise(crh_ctx* c, uint32_t repeats, float* guide_ms, float* pass_ms)
{
  if (!c || !repeats || !pass_ms) return fail(c, CRH_E_INVALID, "crh_bench_denoise: null output / no repeats");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  const DenoiseRule R = rule_of(params_in_force(c));
  CRH_HIP(hipSetDevice(c->device));
  hipStream_t on = cstream(c);
  const float4* shown = nullptr;
  if (int rc = filter(c, on, display_source(c), 0, R, &shown)) return rc;      // guide and images exist, the code is loaded
  if (int rc = wait_overlay_readers(c)) return rc;                                                            // the guide is rewritten below, with what it holds
  CRH_HIP(hipStreamSynchronize(on));
  const uint32_t W = c->par.width, H = c->par.height;
  for (uint32_t k = 0; k < kDenoiseMaxLevels; ++k) pass_ms[k] = 0.f;
  CRH_HIP(time_launches(on, repeats, [&] { launch_denoise_guide(on, c->d_pk_obj, c->d_pk_hit, W, H, c->d_ol_table.as<const OutlineTri>(), c->ol_n_tri, c->d_dn_guide, c->d_dn_ids); return hipGetLastError(); }, guide_ms));
  const float4* in = display_source(c);
  for (uint32_t k = 0; k < R.levels; ++k) {          // pass k from the image pass k - 1 left, over and over: the same bytes every time
    float4* out = c->d_dn_img[0][k & 1u];
    CRH_HIP(time_launches(on, repeats, [&] { launch_denoise_pass(on, c->d_dn_guide, c->d_dn_ids, in, out, W, H, k, R, c->dn_staged); return hipGetLastError(); }, &pass_ms[k]));
    in = out;
  }
  return CRH_OK;
}

int crh_denoise_host(const float* rgba, const int32_t* object_px, const int32_t* triangle_px, const float* t_px, uint32_t width, uint32_t height, const void* table,
                     uint32_t n_tri, const crh_denoise_params* p, float* rgba_out)
{
  if (!rgba || !object_px || !triangle_px || !t_px || !rgba_out || !p || !width || !height || (n_tri && !table)) return CRH_E_INVALID;
  if (params_refused(p)) return CRH_E_INVALID;
  const size_t n = (size_t)width * height;
  std::vector<OutlineTri> tb; std::vector<float4> in, tmp, out;      // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, table, n_tri) || aligned_copy(in, rgba, n) || aligned_copy(tmp, nullptr, n) || aligned_copy(out, nullptr, n)) return CRH_E_NOMEM;
  denoise_host(object_px, triangle_px, t_px, width, height, tb.data(), n_tri, rule_of(*p), in.data(), tmp.data(), out.data());
  std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
  return CRH_OK;
}

}  // extern "C"
