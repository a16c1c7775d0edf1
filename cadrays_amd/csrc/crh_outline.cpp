// crh_outline.cpp -- feature lines on the display ("shaded with edges"): crisp lines along object boundaries, depth steps and creases, drawn by the LDR read-outs
// over the tone-mapped bytes from the first-hit id buffer, so that a 1-spp frame of a drag still shows the shape of a part.  The reference has no counterpart: OCCT's
// path tracer draws no edges, and src/Launcher/DataNode.cxx:286 only sets a display mode of the rasteriser.  Two kernels (outline_kernels.hip): the mask -- one byte
// per pixel, derived from the id buffer and a per-triangle table, kept until one of them changes -- and the drawing.  The rules have ONE copy (outline_kernels.h),
// compiled for the kernels and for the host twins below.  Display state: nothing of the rendering state is touched.  DESIGN.md section 4.11.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "outline_kernels.h"

using namespace crh;
using namespace crh::api;

static_assert(sizeof(OutlineTri) == 32, "the table record is 32 bytes");
static_assert(sizeof(crh_outline_params) == 20, "crh_outline_params is 20 bytes");
static_assert(kOutlineObject == CRH_OUTLINE_OBJECT && kOutlineDepth == CRH_OUTLINE_DEPTH && kOutlineCrease == CRH_OUTLINE_CREASE, "the kinds of the header");

namespace {

const char* thresholds_refused(float crease_cos, float depth_ratio)
{
  const float f[] = {crease_cos, depth_ratio};
  if (!all_finite(f, 2)) return "crease_cos / depth_ratio hold a NaN / Inf";
  if (!(crease_cos > 0.f && crease_cos <= 1.f)) return "crease_cos lies outside (0, 1]";
  if (!(depth_ratio >= 1.f)) return "depth_ratio is below 1";
  return nullptr;
}

const char* params_refused(const crh_outline_params* p)
{
  if (p->kinds & ~kOutlineAll) return "unknown bits in kinds";
  if (p->width < 1u || p->width > 3u) return "width lies outside 1..3";
  return thresholds_refused(p->crease_cos, p->depth_ratio);
}

crh_outline_params params_in_force(const crh_ctx* c)
{
  crh_outline_params p; crh_outline_defaults(&p);
  if (c->ol_on) p = c->ol_par;
  return p;
}

OutlineDraw draw_of(const crh_outline_params& p) { return OutlineDraw{p.kinds, p.width, p.rgb[0], p.rgb[1], p.rgb[2], p.alpha}; }

// the records of n_tri triangles (rows of 4 words: v0, v1, v2, material); false: an index beyond the vertices
bool build_table(const float* pos, size_t n_vertices, const uint32_t* tri, size_t n_tri, OutlineTri* out)
{
  for (size_t t = 0; t < n_tri; ++t) {
    const uint32_t v0 = tri[4 * t], v1 = tri[4 * t + 1], v2 = tri[4 * t + 2];
    if (v0 >= n_vertices || v1 >= n_vertices || v2 >= n_vertices) return false;
    out[t] = outline_record(pos + 3 * (size_t)v0, pos + 3 * (size_t)v1, pos + 3 * (size_t)v2, v0, v1, v2);
  }
  return true;
}

// The per-triangle table of the geometry in force, on the device, valid when this returns (the side stream exists).  Shared with the denoised display
// (crh_denoise.cpp), which reads the normals.
int ensure_outline_table(crh_ctx* c)
{
  if (c->ol_table_gen == c->geom_gen) return CRH_OK;
  const size_t nT = c->tri.size() / 4;                   // the first need after the geometry changed: build the table and upload it
  std::vector<OutlineTri> table;
  if (aligned_copy(table, nullptr, nT)) return fail(c, CRH_E_NOMEM, "no memory for the outline table");
  if (!build_table(c->pos.data(), c->pos.size() / 3, reinterpret_cast<const uint32_t*>(c->tri.data()), nT, table.data()))
    return fail(c, CRH_E_INVALID, "a triangle refers to a vertex that does not exist");
  if (int rc = wait_overlay_readers(c)) return rc;       // a read-back in flight draws from a mask, not from the table; the mask kernel itself ran synchronously
  if (int rc = side_upload(c, c->d_ol_table, table.data(), nT)) return rc;
  c->ol_n_tri = (uint32_t)nT; c->ol_table_gen = c->geom_gen;
  return CRH_OK;
}

}  // namespace

namespace crh {
namespace api {

int ensure_ids_and_table(crh_ctx* c)
{
  int rc = ensure_ids(c); if (rc) return rc;             // (checks c->built, sets the device, creates the side stream)
  CRH_HIP(hipSetDevice(c->device));
  if ((rc = pick_stream(c))) return rc;
  return ensure_outline_table(c);
}

}  // namespace api
}  // namespace crh

namespace {

// The mask of the state in force for these thresholds, on the device, valid when this returns (computed on the side stream and waited for, as ensure_ids does).
int ensure_mask(crh_ctx* c, float crease_cos, float depth_ratio)
{
  int rc = ensure_ids_and_table(c); if (rc) return rc;
  const uint32_t W = c->par.width, H = c->par.height;
  const DerivedStamp now{c->ids_gen, c->ol_table_gen, W, H, {crh_f2u(crease_cos), crh_f2u(depth_ratio)}};
  if (c->ol_mask_stamp == now) return CRH_OK;
  if ((rc = wait_overlay_readers(c))) return rc;         // an asynchronous read-back may still be drawing from the mask
  c->ol_mask_stamp = DerivedStamp{};
  CRH_HIP(c->d_ol_mask.reserve((size_t)W * H));          // (what read the old block has been waited for: this stream runs synchronously, the readers just above)
  launch_outline_mask(c->pk_stream, c->d_pk_obj, c->d_pk_hit, W, H, c->d_ol_table.as<const OutlineTri>(), c->ol_n_tri, crease_cos, depth_ratio, c->d_ol_mask);
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  c->ol_mask_stamp = now;
  return CRH_OK;
}

}  // namespace

namespace crh {
namespace api {

// Called by the LDR read-outs between the tone map (which includes the ShowSamplingTiles outline) and overlay_ldr, on the stream the tone map ran on.  Feature off,
// nothing to draw or no scene: nothing is launched and nothing is computed -- the bytes are the tone map's.
int outline_ldr(crh_ctx* c, hipStream_t on, uint8_t* d_ldr)
{
  if (!c->ol_on || !c->ol_par.kinds || !c->built) return CRH_OK;
  if (int rc = ensure_mask(c, c->ol_par.crease_cos, c->ol_par.depth_ratio)) return rc;
  launch_outline_draw(on, c->d_ol_mask, c->par.width, c->par.height, draw_of(c->ol_par), d_ldr);
  CRH_HIP(hipGetLastError());
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

void crh_outline_defaults(crh_outline_params* p)
{
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->kinds = kOutlineAll;
  p->crease_cos = 0.86602540378f;      // cos 30 deg
  p->depth_ratio = 1.02f;
  p->width = 1u;
  p->rgb[0] = p->rgb[1] = p->rgb[2] = 0; p->alpha = 255;
}

int crh_set_outline(crh_ctx* c, const crh_outline_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) { c->ol_on = false; return CRH_OK; }
  if (const char* why = params_refused(p)) { std::string m = std::string("crh_set_outline: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  c->ol_par = *p; c->ol_on = true;      // read by the LDR read-outs only
  return CRH_OK;
}

int crh_get_outline(crh_ctx* c, crh_outline_params* out, int* on)
{
  if (!c) return CRH_E_INVALID;
  if (out) *out = params_in_force(c);
  if (on) *on = c->ol_on ? 1 : 0;
  return CRH_OK;
}

int crh_read_outline(crh_ctx* c, uint8_t* mask_out)
{
  if (!c || !mask_out) return fail(c, CRH_E_INVALID, "crh_read_outline: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  const crh_outline_params p = params_in_force(c);
  if (int rc = ensure_mask(c, p.crease_cos, p.depth_ratio)) return rc;
  CRH_HIP(hipMemcpyAsync(mask_out, c->d_ol_mask, (size_t)c->par.width * c->par.height, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  return CRH_OK;
}

int crh_outline_table_host(const float* pos, uint32_t n_vertices, const uint32_t* tri, uint32_t n_tri, void* table_out)
{
  if (!pos || !tri || !table_out || !n_vertices || !n_tri) return CRH_E_INVALID;
  std::vector<OutlineTri> table;      // (table_out need not be aligned)
  if (aligned_copy(table, nullptr, n_tri)) return CRH_E_NOMEM;
  if (!build_table(pos, n_vertices, tri, n_tri, table.data())) return CRH_E_INVALID;
  std::memcpy(table_out, table.data(), sizeof(OutlineTri) * (size_t)n_tri);
  return CRH_OK;
}

int crh_outline_mask_host(const int32_t* object_px, const int32_t* triangle_px, const float* t_px, uint32_t width, uint32_t height, const void* table, uint32_t n_tri,
                          float crease_cos, float depth_ratio, uint8_t* mask_out)
{
  if (!object_px || !triangle_px || !t_px || !mask_out || !width || !height || (n_tri && !table)) return CRH_E_INVALID;
  if (thresholds_refused(crease_cos, depth_ratio)) return CRH_E_INVALID;
  std::vector<OutlineTri> tb;         // (the caller's bytes need not be aligned)
  if (aligned_copy(tb, table, n_tri)) return CRH_E_NOMEM;
  outline_mask_host(object_px, triangle_px, t_px, width, height, tb.data(), n_tri, crease_cos, depth_ratio, mask_out);
  return CRH_OK;
}

int crh_outline_draw_host(const uint8_t* mask, uint32_t width, uint32_t height, const crh_outline_params* p, uint8_t* ldr_inout)
{
  if (!mask || !p || !ldr_inout || !width || !height) return CRH_E_INVALID;
  if (params_refused(p)) return CRH_E_INVALID;
  outline_draw_host(mask, width, height, draw_of(*p), ldr_inout);
  return CRH_OK;
}

}  // extern "C"
