// crh_region.cpp -- what the application asks about an AREA of a rendered scene: which objects lie under a dragged rectangle or a lasso, which are visible at all,
// how much of the screen each covers, in which screen box and depth range.  The reference selects one object per click (src/Launcher/AppViewer.cxx:347-457) and has
// no counterpart; in OCCT it is AIS_InteractiveContext::Select(xmin, ymin, xmax, ymax, view) and its polyline form.  One pass over the first-hit id buffer on the
// device reduces eight integers per object (region_kernels.hip; the host twin runs the same rule and the same keys).  Nothing of the rendering state is touched
// and no selection is set: the host hands the flags of crh_region_select to crh_set_selection.  The kernel and the record are DESIGN.md section 4.10.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include <new>

#include "crh_context.h"
#include "region_kernels.h"

using namespace crh;
using namespace crh::api;

namespace {

// The region as a launch sees it: the rectangle cut to the frame, the polygon's edges in doubled units, the box outside which no edge is looked at.
const char* region_setup(uint32_t W, uint32_t H, const uint32_t* rect, const int32_t* poly, uint32_t n_poly, RegionSetup& S, std::vector<RegionEdge>& edges)
{
  std::memset(&S, 0, sizeof S);
  S.width = W; S.height = H;
  uint32_t r[4] = {0u, 0u, W, H};
  if (rect) {
    if (rect[0] > rect[2] || rect[1] > rect[3]) return "the rectangle is inverted (x0 > x1 or y0 > y1)";
    r[0] = std::min(rect[0], W); r[1] = std::min(rect[1], H); r[2] = std::min(rect[2], W); r[3] = std::min(rect[3], H);
  }
  S.rx0 = r[0]; S.ry0 = r[1]; S.rx1 = r[2]; S.ry1 = r[3];
  S.bx0 = r[0]; S.by0 = r[1]; S.bx1 = r[2]; S.by1 = r[3];
  edges.clear();
  if (!poly && !n_poly) return nullptr;
  if (!poly) return "a vertex count without vertices";
  if (n_poly < 3u || n_poly > kRegionMaxEdges) return "a polygon takes 3 to 256 vertices";
  int32_t lo[2] = {kRegionMaxCoord, kRegionMaxCoord}, hi[2] = {-kRegionMaxCoord, -kRegionMaxCoord};
  for (uint32_t k = 0; k < 2u * n_poly; ++k) {
    if (poly[k] < -kRegionMaxCoord || poly[k] > kRegionMaxCoord) return "a polygon coordinate lies beyond +-2^20";
    lo[k & 1u] = std::min(lo[k & 1u], poly[k]); hi[k & 1u] = std::max(hi[k & 1u], poly[k]);
  }
  edges.resize(n_poly);
  for (uint32_t k = 0; k < n_poly; ++k) {
    const int32_t* a = poly + 2 * (size_t)k; const int32_t* b = poly + 2 * (size_t)((k + 1u) % n_poly);
    edges[k] = RegionEdge{2 * a[0], 2 * a[1], 2 * (b[0] - a[0]), 2 * (b[1] - a[1])};
  }
  S.n_edges = n_poly;
  // a centre 2 p + 1 lies strictly between the doubled extremes 2 lo and 2 hi iff lo <= p < hi: the pixels [lo, hi) per axis, cut to the rectangle
  auto cut = [](int32_t v, uint32_t a, uint32_t b) { return v < (int32_t)0 ? a : std::min(std::max((uint32_t)v, a), b); };
  S.bx0 = cut(lo[0], r[0], r[2]); S.bx1 = cut(hi[0], r[0], r[2]); S.by0 = cut(lo[1], r[1], r[3]); S.by1 = cut(hi[1], r[1], r[3]);
  if (S.bx0 >= S.bx1 || S.by0 >= S.by1) S.bx0 = S.bx1 = S.by0 = S.by1 = 0u;
  return nullptr;
}

// a zero record means "no pixel"; minima were kept as complements, x1 / y1 as coordinate + 1, the distances as their bits
void records_to_stats(const uint32_t* rec, uint32_t n_records, crh_region_stats* out)
{
  for (uint32_t o = 0; o < n_records; ++o) {
    const uint32_t* r = rec + (size_t)kRegionRec * o;
    crh_region_stats& s = out[o];
    std::memset(&s, 0, sizeof s);
    s.pixels = r[0]; s.pixels_frame = r[1];
    if (!r[0]) continue;
    s.x0 = ~r[2]; s.y0 = ~r[3]; s.x1 = r[4]; s.y1 = r[5];
    s.t_min = r[6] ? crh_u2f(~r[6]) : 0.f; s.t_max = crh_u2f(r[7]);
  }
}

}  // namespace

extern "C" {

int crh_query_region(crh_ctx* c, const uint32_t rect[4], const int32_t* poly_xy, uint32_t n_poly, crh_region_stats* out, uint32_t n_objects)
{
  if (!c || !out) return fail(c, CRH_E_INVALID, "crh_query_region: null output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  const uint32_t nO = n_pick_objects(c);
  if (n_objects != nO) { char b[128]; snprintf(b, sizeof b, "crh_query_region: %u records for a scene of %u objects", n_objects, nO); return fail(c, CRH_E_INVALID, b); }
  RegionSetup S; std::vector<RegionEdge> edges;
  if (const char* why = region_setup(c->par.width, c->par.height, rect, poly_xy, n_poly, S, edges)) { std::string m = std::string("crh_query_region: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  int rc = ensure_ids(c); if (rc) return rc;             // (sets the device, creates the side stream; a valid buffer: nothing is launched)
  CRH_HIP(hipSetDevice(c->device));
  if ((rc = pick_stream(c))) return rc;
  const size_t n_rec = (size_t)nO + 1;
  CRH_HIP(c->d_rg_edges.reserve(sizeof(RegionEdge) * kRegionMaxEdges));
  CRH_HIP(c->d_rg_rec.reserve((size_t)kRegionRec * n_rec, (size_t)kRegionRec * 16));      // crh_add_object grows the scene one object at a time
  std::vector<uint32_t> rec((size_t)kRegionRec * n_rec, 0u);
  if (S.n_edges) CRH_HIP(hipMemcpyAsync(c->d_rg_edges, edges.data(), sizeof(RegionEdge) * S.n_edges, hipMemcpyHostToDevice, c->pk_stream));
  CRH_HIP(hipMemsetAsync(c->d_rg_rec, 0, sizeof(uint32_t) * kRegionRec * n_rec, c->pk_stream));
  // ONE workgroup per compute unit: every workgroup ends with its atomics on the records, and fewer, longer-running workgroups were faster in every form measured
  // (4 / 2 / 1 per compute unit)
  launch_region_stats(c->pk_stream, std::max(c->grid / 4, 1), c->d_pk_obj, c->d_pk_hit, c->d_rg_edges.as<const RegionEdge>(), S, nO, c->d_rg_rec);
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipMemcpyAsync(rec.data(), c->d_rg_rec, sizeof(uint32_t) * kRegionRec * n_rec, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  records_to_stats(rec.data(), (uint32_t)n_rec, out);
  return CRH_OK;
}

int crh_region_stats_host(const int32_t* object_px, const float* t_px, uint32_t width, uint32_t height, const uint32_t rect[4], const int32_t* poly_xy, uint32_t n_poly,
                          crh_region_stats* out, uint32_t n_objects)
{
  if (!object_px || !t_px || !out || !width || !height || !n_objects) return CRH_E_INVALID;
  RegionSetup S; std::vector<RegionEdge> edges;
  if (region_setup(width, height, rect, poly_xy, n_poly, S, edges)) return CRH_E_INVALID;
  std::vector<uint32_t> rec;
  try { rec.assign((size_t)kRegionRec * ((size_t)n_objects + 1), 0u); } catch (const std::bad_alloc&) { return CRH_E_NOMEM; }
  region_stats_host(object_px, t_px, edges.data(), S, n_objects, rec.data());
  records_to_stats(rec.data(), n_objects + 1u, out);
  return CRH_OK;
}

int crh_region_select(const crh_region_stats* stats, uint32_t n_objects, int mode, uint32_t min_pixels, uint8_t* selected_out)
{
  if (!stats || !selected_out || !n_objects || (mode != CRH_REGION_TOUCHED && mode != CRH_REGION_ENCLOSED)) return CRH_E_INVALID;
  const uint32_t least = min_pixels > 1u ? min_pixels : 1u;
  for (uint32_t o = 0; o < n_objects; ++o)
    selected_out[o] = (stats[o].pixels >= least && (mode == CRH_REGION_TOUCHED || stats[o].pixels == stats[o].pixels_frame)) ? 1 : 0;
  return CRH_OK;
}

}  // extern "C"
