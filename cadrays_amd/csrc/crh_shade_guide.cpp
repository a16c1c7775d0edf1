// crh_shade_guide.cpp -- the shade guide of the denoised display: albedo demodulation and lights in view for the a-trous filter of crh_denoise.cpp.  A per-pixel
// plane {1 / albedo of the first hit, "a positional light shows here"}, derived from the first-hit id buffer, a per-triangle table of uv and material, and the
// shading state (materials, textures, lights, spec); the guided form of the pass divides by the albedo in front of the filter, multiplies it back behind it and
// leaves the lights' discs alone.  The reference has no counterpart: OCCT's path tracer shows the raw accumulation (AppViewer.cxx:1045-1047).  Three kernels
// (shade_guide_kernels.hip): the light test, the plane, the guided pass.  The rules have ONE copy (shade_guide_kernels.h, denoise_kernels.h), compiled for the
// kernels and for the host twins below.  Display state: nothing of the rendering state is touched.  DESIGN.md section 4.14.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "shade_guide_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(crh_shade_guide_params) == 16, "crh_shade_guide_params is 16 bytes");
static_assert(sizeof(GuideTri) == 32, "the table record is 32 bytes");
static_assert(sizeof(crh_bsdf) == 8 * sizeof(float4) && sizeof(crh_light) == 2 * sizeof(float4), "a material is 8 float4, a light 2");

namespace {

const char* params_refused(const crh_shade_guide_params* p)
{
  if (!all_finite(&p->albedo_floor, 1)) return "albedo_floor is a NaN / Inf";
  if (p->demodulate > 1u || p->lights > 1u) return "demodulate / lights is neither 0 nor 1";
  if (!(p->albedo_floor > 0.f && p->albedo_floor <= 1.f)) return "albedo_floor lies outside (0, 1]";
  if (p->light_dilate > 2u) return "light_dilate lies outside 0..2";
  return nullptr;
}

crh_shade_guide_params params_in_force(const crh_ctx* c)
{
  crh_shade_guide_params p; crh_shade_guide_defaults(&p);
  if (c->sg_on) p = c->sg_par;
  return p;
}

crh_denoise_params denoise_in_force(const crh_ctx* c)
{
  crh_denoise_params p; crh_denoise_defaults(&p);
  if (c->dn_on) p = c->dn_par;
  return p;
}

ShadeGuideRule rule_of(const crh_shade_guide_params& p) { return ShadeGuideRule{p.demodulate, p.lights, p.albedo_floor, p.light_dilate}; }
DenoiseRule denoise_rule_of(const crh_denoise_params& p) { return DenoiseRule{p.levels, p.normal_cos, p.depth_ratio, (float)p.until_samples}; }

// the records of n_tri triangles (rows of 4 words: v0, v1, v2, material); uv: 2 floats per vertex, or nullptr; false: an index beyond the vertices
bool build_table(const float* uv, size_t n_vertices, const uint32_t* tri, size_t n_tri, GuideTri* out)
{
  for (size_t t = 0; t < n_tri; ++t) {
    GuideTri r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, (int32_t)tri[4 * t + 3], uv ? 1u : 0u};
    if (uv) {
      const uint32_t v0 = tri[4 * t], v1 = tri[4 * t + 1], v2 = tri[4 * t + 2];
      if (v0 >= n_vertices || v1 >= n_vertices || v2 >= n_vertices) return false;
      r.u0 = uv[2 * (size_t)v0]; r.v0 = uv[2 * (size_t)v0 + 1]; r.u1 = uv[2 * (size_t)v1]; r.v1 = uv[2 * (size_t)v1 + 1]; r.u2 = uv[2 * (size_t)v2]; r.v2 = uv[2 * (size_t)v2 + 1];
    }
    out[t] = r;
  }
  return true;
}

// The table of the geometry in force, on the device, valid when this returns (the side stream exists).
int ensure_guide_table(crh_ctx* c)
{
  if (c->sg_table_gen == c->geom_gen) return CRH_OK;
  const size_t nT = c->tri.size() / 4;
  std::vector<GuideTri> table;
  if (aligned_copy(table, nullptr, nT)) return fail(c, CRH_E_NOMEM, "no memory for the shade guide's table");
  if (!build_table(c->uv.empty() ? nullptr : c->uv.data(), c->uv.size() / 2, reinterpret_cast<const uint32_t*>(c->tri.data()), nT, table.data()))
    return fail(c, CRH_E_INVALID, "a triangle refers to a vertex that does not exist");
  if (int rc = wait_overlay_readers(c)) return rc;       // (a read-back in flight filters from a plane, not from the table; the plane kernel itself ran synchronously)
  if (int rc = side_upload(c, c->d_sg_table, table.data(), nT)) return rc;
  c->sg_n_tri = (uint32_t)nT; c->sg_table_gen = c->geom_gen;
  return CRH_OK;
}

ShadeGuideScene device_scene(const crh_ctx* c)
{
  const uint32_t n_tex = c->d_tex_desc ? (uint32_t)c->textures.size() : 0u;      // (as fill_scene counts them)
  return ShadeGuideScene{c->d_mats, (uint32_t)c->mats.size(), c->d_texels, c->d_tex_desc, n_tex, c->d_lights, (uint32_t)c->lights.size(), c->spec.texel_gamma2};
}

bool any_positional(const crh_ctx* c)
{
  for (const crh_light& l : c->lights) if (l.is_point != 0.f) return true;
  return false;
}

// the light test (when the rule asks for it and there is a positional light) and the plane, enqueued on `on`; the two blocks have room
void launch_plane(crh_ctx* c, hipStream_t on, const ShadeGuideRule& R)
{
  const uint32_t W = c->par.width, H = c->par.height;
  const bool flags = R.lights && any_positional(c);
  if (flags) { DScene S; fill_scene(c, S); launch_shade_guide_seen(on, S, c->d_pk_hit, c->d_sg_seen); }
  launch_shade_guide_plane(on, device_scene(c), c->d_pk_hit, W, H, c->d_sg_table.as<const GuideTri>(), c->sg_n_tri, flags ? (const uint8_t*)c->d_sg_seen : nullptr, R, c->d_sg_plane);
}

}  // namespace

namespace crh {
namespace api {

// The plane of the state in force, on the device, valid when this returns (computed on the side stream and waited for, as the filter's guide is).  The textures a
// setter has left for the next frame to upload are uploaded first: the plane reads the device's copies.
int ensure_shade_plane(crh_ctx* c)
{
  int rc = ensure_ids(c); if (rc) return rc;             // (checks c->built, sets the device, creates the side stream)
  CRH_HIP(hipSetDevice(c->device));
  if ((rc = pick_stream(c))) return rc;
  if ((rc = ensure_guide_table(c))) return rc;
  const crh_shade_guide_params p = params_in_force(c);
  const uint32_t W = c->par.width, H = c->par.height;
  const DerivedStamp now{c->ids_gen, c->sg_table_gen, W, H, {p.demodulate | (p.lights << 1) | (p.light_dilate << 2), crh_f2u(p.albedo_floor)}};
  if (c->sg_stamp == now && c->sg_stamp_shade == c->shade_gen) return CRH_OK;
  if ((rc = wait_overlay_readers(c))) return rc;         // an asynchronous read-back may still be filtering from the plane
  c->sg_stamp = DerivedStamp{};
  if ((rc = upload_textures(c))) return rc;              // (nothing unless crh_set_texture was called since the last frame)
  CRH_HIP(c->d_sg_plane.reserve((size_t)W * H)); CRH_HIP(c->d_sg_seen.reserve((size_t)W * H));      // (what read the old blocks has been waited for)
  if ((rc = fork_from_context(c))) return rc;            // materials and lights travel stream-ordered on the context's stream
  launch_plane(c, c->pk_stream, rule_of(p));
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->sg_stamp = now; c->sg_stamp_shade = c->shade_gen;
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

void crh_shade_guide_defaults(crh_shade_guide_params* p)
{
  if (!p) return;
  p->demodulate = 1u; p->lights = 1u;
  p->albedo_floor = 0.015625f;      // 1 / 64
  p->light_dilate = 1u;
}

int crh_set_shade_guide(crh_ctx* c, const crh_shade_guide_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) { c->sg_on = false; return CRH_OK; }
  if (const char* why = params_refused(p)) { std::string m = std::string("crh_set_shade_guide: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  c->sg_par = *p; c->sg_on = true;      // read by the denoise filter of the LDR read-outs and crh_read_denoised only
  return CRH_OK;
}

int crh_get_shade_guide(crh_ctx* c, crh_shade_guide_params* out, int* on)
{
  if (!c) return CRH_E_INVALID;
  if (out) *out = params_in_force(c);
  if (on) *on = c->sg_on ? 1 : 0;
  return CRH_OK;
}

int crh_read_shade_guide(crh_ctx* c, float* plane_out)
{
  if (!c || !plane_out) return fail(c, CRH_E_INVALID, "crh_read_shade_guide: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (int rc = ensure_shade_plane(c)) return rc;
  CRH_HIP(hipMemcpyAsync(plane_out, c->d_sg_plane, sizeof(float4) * (size_t)c->par.width * c->par.height, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  return CRH_OK;
}

int crh_read_hit_uv(crh_ctx* c, float* uv_out)
{
  if (!c || !uv_out) return fail(c, CRH_E_INVALID, "crh_read_hit_uv: null output");
  int rc = ensure_ids(c); if (rc) return rc;
  const size_t n = (size_t)c->par.width * c->par.height;
  std::vector<float> h;
  if (aligned_copy(h, nullptr, 4 * n)) return fail(c, CRH_E_NOMEM, "no memory for the hit records");
  CRH_HIP(hipMemcpyAsync(h.data(), c->d_pk_hit, 16 * n, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  for (size_t i = 0; i < n; ++i) { uv_out[2 * i] = h[4 * i + 1]; uv_out[2 * i + 1] = h[4 * i + 2]; }
  return CRH_OK;
}

int crh_bench_shade_guide(crh_ctx* c, uint32_t repeats, float* guide_ms, float* pass_ms)
{
  if (!c || !repeats || !pass_ms) return fail(c, CRH_E_INVALID, "crh_bench_shade_guide: null output / no repeats");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (!c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  const DenoiseRule R = denoise_rule_of(denoise_in_force(c));
  const ShadeGuideRule G = rule_of(params_in_force(c));
  if (int rc = ensure_guide(c)) return rc;                // the filter's guide, the plane and the code exist
  if (int rc = ensure_shade_plane(c)) return rc;
  const uint32_t W = c->par.width, H = c->par.height;
  hipStream_t on = cstream(c);
  if (int rc = grow_display_scratch(c, 0, c->d_dn_img[0], 2, (size_t)W * H)) return rc;
  if (int rc = wait_overlay_readers(c)) return rc;        // the plane is rewritten below, with what it holds
  CRH_HIP(hipStreamSynchronize(on));
  for (uint32_t k = 0; k < kDenoiseMaxLevels; ++k) pass_ms[k] = 0.f;
  CRH_HIP(time_launches(on, repeats, [&] { launch_plane(c, on, G); return hipGetLastError(); }, guide_ms));
  const float4* in = display_source(c);
  for (uint32_t k = 0; k < R.levels; ++k) {               // pass k from the image pass k - 1 left, over and over: the same bytes every time
    float4* out = c->d_dn_img[0][k & 1u];
    CRH_HIP(time_launches(on, repeats, [&] { launch_denoise_pass_guided(on, c->d_dn_guide, c->d_dn_ids, c->d_sg_plane, in, out, W, H, k, R); return hipGetLastError(); }, &pass_ms[k]));
    in = out;
  }
  return CRH_OK;
}

int crh_guide_table_host(const float* uv, uint32_t n_vertices, const uint32_t* tri, uint32_t n_tri, void* table_out)
{
  if (!tri || !table_out || !n_tri) return CRH_E_INVALID;
  std::vector<GuideTri> table;      // (table_out need not be aligned)
  if (aligned_copy(table, nullptr, n_tri)) return CRH_E_NOMEM;
  if (!build_table(uv, n_vertices, tri, n_tri, table.data())) return CRH_E_INVALID;
  std::memcpy(table_out, table.data(), sizeof(GuideTri) * (size_t)n_tri);
  return CRH_OK;
}

int crh_shade_guide_host(const crh_shade_guide_scene* s, const float* rays_px, const int32_t* triangle_px, const float* t_px, const float* uv_px, uint32_t width,
                         uint32_t height, const void* guide_table, uint32_t n_tri, const crh_shade_guide_params* p, float* plane_out)
{
  if (!s || !rays_px || !triangle_px || !t_px || !uv_px || !plane_out || !p || !width || !height || (n_tri && !guide_table)) return CRH_E_INVALID;
  if (params_refused(p)) return CRH_E_INVALID;
  if ((s->n_mats && !s->mats) || (s->n_texels && !s->texels) || (s->n_tex && !s->tex_desc) || (s->n_lights && !s->lights) || (n_tri && !s->n_mats)) return CRH_E_INVALID;
  if (!all_finite(reinterpret_cast<const float*>(s->mats), 32 * (size_t)s->n_mats)) return CRH_E_INVALID;
  for (uint32_t m = 0; m < s->n_mats; ++m) if (!(crh_abs(s->mats[m].Kd[3]) <= 16777216.0f)) return CRH_E_INVALID;      // (int)Kd.w is defined
  for (uint32_t k = 0; k < s->n_tex; ++k) {
    const uint32_t* d = s->tex_desc + 4 * (size_t)k;
    if (d[1] && (!d[2] || d[1] > 32768u || d[2] > 32768u || (uint64_t)d[0] + (uint64_t)d[1] * d[2] > s->n_texels)) return CRH_E_INVALID;
  }
  const size_t n = (size_t)width * height;
  std::vector<GuideTri> tb; std::vector<float4> mats, texels, lights, plane; std::vector<uint4> desc; std::vector<uint8_t> seen;      // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, guide_table, n_tri) || aligned_copy(mats, s->mats, 8 * (size_t)s->n_mats) || aligned_copy(texels, s->texels, s->n_texels) ||
      aligned_copy(desc, s->tex_desc, s->n_tex) || aligned_copy(lights, nullptr, 2 * (size_t)s->n_lights) || aligned_copy(plane, nullptr, n) || aligned_copy(seen, nullptr, n))
    return CRH_E_NOMEM;
  for (uint32_t i = 0; i < s->n_lights; ++i) {            // the kernels' record of a positional light: {position, 1}, {emission, radius}; a directional one is not looked at
    const crh_light& l = s->lights[i];
    if (l.is_point != 0.f) { lights[2 * i] = make_float4(l.vec[0], l.vec[1], l.vec[2], 1.f); lights[2 * i + 1] = make_float4(l.emission[0], l.emission[1], l.emission[2], l.smoothness); }
  }
  const ShadeGuideScene S{mats.data(), s->n_mats, texels.data(), desc.data(), s->n_tex, lights.data(), s->n_lights, s->gamma2};
  shade_guide_host(S, rays_px, triangle_px, t_px, uv_px, width, height, tb.data(), n_tri, rule_of(*p), seen.data(), plane.data());
  std::memcpy(plane_out, plane.data(), sizeof(float4) * n);
  return CRH_OK;
}

int crh_denoise_guided_host(const float* rgba, const int32_t* object_px, const int32_t* triangle_px, const float* t_px, uint32_t width, uint32_t height, const void* table,
                            uint32_t n_tri, const float* plane, const crh_denoise_params* p, float* rgba_out)
{
  if (!rgba || !object_px || !triangle_px || !t_px || !plane || !rgba_out || !p || !width || !height || (n_tri && !table)) return CRH_E_INVALID;
  crh_denoise_params probe = *p;      // checked as crh_denoise_host checks it: by that function itself, over one pixel
  { const float px[4] = {0.f, 0.f, 0.f, 0.f}; const int32_t id = -1; const float t0 = CRH_MAXFLOAT; float o[4];
    if (int rc = crh_denoise_host(px, &id, &id, &t0, 1u, 1u, nullptr, 0u, &probe, o)) return rc; }
  const size_t n = (size_t)width * height;
  std::vector<OutlineTri> tb; std::vector<float4> in, sg, tmp, out;      // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, table, n_tri) || aligned_copy(in, rgba, n) || aligned_copy(sg, plane, n) || aligned_copy(tmp, nullptr, n) || aligned_copy(out, nullptr, n)) return CRH_E_NOMEM;
  denoise_guided_host(object_px, triangle_px, t_px, width, height, tb.data(), n_tri, sg.data(), denoise_rule_of(*p), in.data(), tmp.data(), out.data());
  std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
  return CRH_OK;
}

}  // extern "C"
