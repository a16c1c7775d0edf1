// region_kernels.h -- region queries on the first-hit id buffer (crh_region.cpp, region_kernels.hip): the polygon rule, the per-object record and its keys -- ONE copy
// each, compiled for the gfx950 kernel and for the host twin -- and the launch wrapper.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
//
// ARITHMETIC: integers only (the rule in int64, counts, coordinates, the bits of non-negative finite floats), every field of a record a sum or a maximum: nothing
// depends on the order of arrival, so the device, the host twin and a numpy restatement agree bit for bit (tests/region_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crh_math.h"

namespace crh {

constexpr uint32_t kRegionRec = 8;             // dwords per record, ZERO = "no pixel": pixels, pixels_frame, ~x0, ~y0, x1, y1, ~bits(t_min), bits(t_max) -- two sums, six maxima
constexpr uint32_t kRegionMaxEdges = 256;      // 256 x 16 B = 4 KB
constexpr int32_t kRegionMaxCoord = 1 << 20;   // |vertex coordinate| <= 2^20 pixels: doubled 2^21, a difference 2^22, a product 2^44

struct alignas(16) RegionEdge { int32_t ax, ay, dx, dy; };   // DOUBLED units: a = (2x, 2y) of the edge's first vertex, d = b - a

// What a launch tests a pixel against.  rect = the caller's rectangle cut to the frame (possibly empty); box = rect cut to the pixels whose centre can lie inside
// the polygon (= rect without a polygon): outside it no edge is looked at.
struct RegionSetup { uint32_t width, height, rx0, ry0, rx1, ry1, bx0, by0, bx1, by1, n_edges; };

// THE RULE, even-odd, exact.  Pixel (px, py) has its centre at (cx, cy) = (2 px + 1, 2 py + 1) in doubled units -- odd, so never on the row of a vertex.  Edge a -> b
// counts iff it crosses the centre's row, (a.y < cy) != (b.y < cy), and the centre lies strictly on its left seen upwards resp. right seen downwards:
// cross * sign(b.y - a.y) > 0 with cross = (b.x - a.x)(cy - a.y) - (cx - a.x)(b.y - a.y).  Horizontal and zero-length edges (dy == 0) never cross a row.
CRH_HD bool region_edge_crosses_row(const RegionEdge& e, int32_t cy) { return (e.ay < cy) != (e.ay + e.dy < cy); }
CRH_HD bool region_edge_counts(const RegionEdge& e, int32_t cx, int32_t cy)      // for an edge that crosses the row of cy
{
  const int64_t cross = (int64_t)e.dx * (int64_t)(cy - e.ay) - (int64_t)(cx - e.ax) * (int64_t)e.dy;
  return e.dy > 0 ? cross > 0 : cross < 0;
}
CRH_HD bool region_inside_polygon(const RegionEdge* edges, uint32_t n_edges, uint32_t px, uint32_t py)
{
  const int32_t cx = 2 * (int32_t)px + 1, cy = 2 * (int32_t)py + 1;
  bool in = false;
  for (uint32_t k = 0; k < n_edges; ++k)
    if (region_edge_crosses_row(edges[k], cy) && region_edge_counts(edges[k], cx, cy)) in = !in;
  return in;
}
CRH_HD bool region_in_rect(const RegionSetup& S, uint32_t px, uint32_t py) { return px >= S.rx0 && px < S.rx1 && py >= S.ry0 && py < S.ry1; }
CRH_HD bool region_in_box(const RegionSetup& S, uint32_t px, uint32_t py) { return px >= S.bx0 && px < S.bx1 && py >= S.by0 && py < S.by1; }

// the record an object id goes to: the object's own, or the background's (index n_objects) for a miss (-1) and for any id outside [0, n_objects)
CRH_HD uint32_t region_slot(int32_t object, uint32_t n_objects) { return (object >= 0 && (uint32_t)object < n_objects) ? (uint32_t)object : n_objects; }

// rec: kRegionRec * (n_objects + 1) dwords, ZERO at launch.  object: width * height ids, row-major; hit: the id buffer's {t, u, v, triangle} plane, .x read only for
// pixels inside the region that hit something.  edges: S.n_edges of them on the device (not read when 0).  `grid` workgroups at most.
void launch_region_stats(hipStream_t stream, int grid, const int32_t* object, const float4* hit, const RegionEdge* edges, const RegionSetup& S, uint32_t n_objects, uint32_t* rec);
// the host twin: the same rule and the same keys in a plain loop over host planes (t: one float per pixel; rec zeroed by the caller)
void region_stats_host(const int32_t* object, const float* t, const RegionEdge* edges, const RegionSetup& S, uint32_t n_objects, uint32_t* rec);
// threads per workgroup, chunks of 64 pixels a wavefront has in flight per round (a frame of more than grid x 4 x kRegionLoads chunks takes a second round)
constexpr int kRegionBlock = 256, kRegionLoads = 4;

}  // namespace crh
