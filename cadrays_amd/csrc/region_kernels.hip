// region_kernels.hip -- the one pass over the first-hit id buffer behind crh_query_region (crh_region.cpp): per object the pixels inside a rectangle / polygon, the
// pixels in the whole frame, their screen box and depth range, for gfx950, and the host twin.
// (reference: the reference selects one object per click, src/Launcher/AppViewer.cxx:347-457; rubber-band and lasso selection are
// AIS_InteractiveContext::Select(xmin, ymin, xmax, ymax, view) and its polyline form in OCCT, which the application never calls)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.  Integers only (region_kernels.h): every field of a
// record is a sum or a maximum, so the record does not depend on which wavefront arrives first or on how a wavefront's pixels are grouped.
#include "region_kernels.h"

namespace crh {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // "no record": a lane beyond the row's end, a wavefront that has met no pixel yet

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_umax(uint32_t m)
{
  for (int off = 32; off > 0; off >>= 1) m = umax(m, (uint32_t)__shfl_xor((int)m, off));
  return m;
}

// THE REDUCTION.  A frame of ONE object sends every wavefront of the chip to the same eight words, and atomics on one address are served one after the other
// (DESIGN.md section 6.8 measured it on k_fit_extents; section 6.9: the first form of this kernel, which kept ONE running record per wavefront and sent it whenever
// the record changed, took 2.8 ms at 1080p on a soup whose pixels alternate between the object and the background).  So a wavefront keeps kRegionSlots running
// records in REGISTERS, spread over its lanes: lane 8 s + q of register pair h holds field q of the record in slot 8 h + s, and its tag (the record's index, kNone: empty)
// beside it.  A record lives in slot (index mod kRegionSlots).  Joining a group costs a handful of VALU instructions and no memory traffic; a record leaves for HBM
// only when another one claims its slot (eight lanes, eight words, one instruction each for the sums and the maxima, nothing waited for) and at the end.
constexpr uint32_t kRegionSlots = 32;

struct RegionTable { uint32_t tag0, tag1, tag2, tag3, val0, val1, val2, val3; };      // per lane (plain members: nothing here is indexed at run time)

// the eight lanes of a slot send their fields of record `id`; a zero field has nothing to add
__device__ __forceinline__ void region_evict(uint32_t* __restrict__ rec, uint32_t id, uint32_t v, uint32_t q)
{
  if (!v) return;
  uint32_t* r = rec + (size_t)kRegionRec * id + q;
  if (q < 2u) atomicAdd(r, v); else atomicMax(r, v);
}

__device__ __forceinline__ void region_join_part(uint32_t& tag, uint32_t& val, uint32_t* __restrict__ rec, uint32_t g, uint32_t s8, bool mine, uint32_t q, uint32_t v)
{
  const uint32_t old = (uint32_t)__builtin_amdgcn_readlane((int)tag, (int)(8u * s8));
  if (old != g && mine) {                                                    // (old != g: uniform)
    if (old != kNone) region_evict(rec, old, val, q);
    tag = g; val = 0u;
  }
  if (mine) val = q < 2u ? val + v : umax(val, v);
}

// the group of record g joins the table: f0 .. f7 are the group's eight fields, the same in every lane (a field that has nothing to say is 0); lane 8 s + q takes
// field q (scalars and selects on purpose: an array indexed by q would be spilled to LDS and read back per lane)
__device__ __forceinline__ void region_join(RegionTable& T, uint32_t* __restrict__ rec, uint32_t lane, uint32_t g, uint32_t f0, uint32_t f1, uint32_t f2, uint32_t f3,
                                            uint32_t f4, uint32_t f5, uint32_t f6, uint32_t f7)
{
  const uint32_t q = lane & 7u, slot = g & (kRegionSlots - 1u), s8 = slot & 7u;
  const uint32_t lo = (q & 1u) ? ((q & 2u) ? f3 : f1) : ((q & 2u) ? f2 : f0), hi = (q & 1u) ? ((q & 2u) ? f7 : f5) : ((q & 2u) ? f6 : f4);
  const uint32_t v = (q & 4u) ? hi : lo;
  const bool mine = (lane >> 3) == s8;
  if (slot < 8u) region_join_part(T.tag0, T.val0, rec, g, s8, mine, q, v);   // uniform
  else if (slot < 16u) region_join_part(T.tag1, T.val1, rec, g, s8, mine, q, v);
  else if (slot < 24u) region_join_part(T.tag2, T.val2, rec, g, s8, mine, q, v);
  else region_join_part(T.tag3, T.val3, rec, g, s8, mine, q, v);
}

// One pass over the WHOLE frame (pixels_frame needs every pixel).  A wavefront takes 64 consecutive pixels of ONE row per chunk -- one coalesced 256-B load of the
// object plane -- and kRegionLoads chunks per round of its grid-stride loop, all loads issued before the first is used.  Row and chunk are the same for the whole
// wavefront, so the "does this edge cross my row" half of the rule is asked once per EDGE, not per pixel: the edges sit in registers, four per lane, each lane
// asks for its own, a ballot names the few that cross, and only those cost every lane a 64-bit cross product (their values come by v_readlane: no memory is touched
// inside the pixel loop).  A chunk wholly outside rect x bbox(polygon) never looks at an edge.  t is read only where a pixel is inside the region and hit something.
//   The lanes are grouped by record -- the first remaining lane's record, a ballot of the lanes that hold it, popcounts for the two counts; the lanes of a chunk are
//   consecutive pixels of one row, so the group's box is the first and last set bit of the ballot and the row (no cross-lane traffic), and only the two depth keys
//   take a masked wave maximum.  The group joins the wavefront's table (above).  At the end the four wavefronts of the workgroup meet in LDS: entries of the same
//   record leave as one, counts added, and a key maximum is sent only where a plain look at the record says it would raise it -- the keys only grow, so a stale
//   look can cost an atomic that changes nothing and never loses one.
// Every loop bound and every branch around a cross-lane operation is uniform per wavefront.
__global__ __launch_bounds__(kRegionBlock) void k_region_stats(const int32_t* __restrict__ object, const float4* __restrict__ hit, const RegionEdge* __restrict__ edges,
                                                               RegionSetup S, uint32_t n_objects, uint32_t* __restrict__ rec)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kRegionBlock + threadIdx.x) >> 6)), n_waves = gridDim.x * (kRegionBlock / 64);
  const uint32_t cpr = (S.width + 63u) >> 6;                                 // chunks per row
  const uint64_t n_chunks = (uint64_t)cpr * S.height;                        // (< 2^32: the planes of such a frame fit in memory)
  // the polygon's edges, uniform per launch, staged ONCE in registers: lane l holds edges l, 64 + l, 128 + l, 192 + l (beyond the last: dy = 0, which crosses no row)
  RegionEdge ev[kRegionMaxEdges / 64];
#pragma unroll
  for (uint32_t m = 0; m < kRegionMaxEdges / 64u; ++m) ev[m] = (S.n_edges && lane + 64u * m < S.n_edges) ? edges[lane + 64u * m] : RegionEdge{0, 0, 0, 0};
  RegionTable T{kNone, kNone, kNone, kNone, 0u, 0u, 0u, 0u};
  for (uint64_t c0 = wave; c0 < n_chunks; c0 += (uint64_t)kRegionLoads * n_waves) {
    int32_t ob[kRegionLoads]; uint32_t row[kRegionLoads], xb[kRegionLoads]; bool live[kRegionLoads];
#pragma unroll
    for (int j = 0; j < kRegionLoads; ++j) {
      const uint64_t c = c0 + (uint64_t)j * n_waves;
      const bool ok = c < n_chunks;
      row[j] = ok ? (uint32_t)c / cpr : 0u;
      xb[j] = ok ? ((uint32_t)c - row[j] * cpr) * 64u : S.width;
      live[j] = xb[j] + lane < S.width;
      ob[j] = live[j] ? object[(size_t)row[j] * S.width + xb[j] + lane] : -1;
    }
#pragma unroll
    for (int j = 0; j < kRegionLoads; ++j) {
      const uint32_t y = row[j], x = xb[j] + lane;
      const uint32_t id = live[j] ? region_slot(ob[j], n_objects) : kNone;
      bool in = live[j] && region_in_rect(S, x, y);
      if (S.n_edges) {
        in = in && region_in_box(S, x, y);
        if (__ballot(in)) {
          const int32_t cx = 2 * (int32_t)x + 1, cy = 2 * (int32_t)y + 1;
          bool odd = false;
#pragma unroll
          for (uint32_t m = 0; m < kRegionMaxEdges / 64u; ++m) {
            unsigned long long cr = __ballot(region_edge_crosses_row(ev[m], cy));      // every lane asks for its own edges: the row is the wavefront's
            while (cr) {                                                               // ... and every lane then weighs the few edges that do cross it
              const int k = __ffsll((long long)cr) - 1;
              cr &= cr - 1ull;
              const RegionEdge e{__builtin_amdgcn_readlane(ev[m].ax, k), __builtin_amdgcn_readlane(ev[m].ay, k), __builtin_amdgcn_readlane(ev[m].dx, k), __builtin_amdgcn_readlane(ev[m].dy, k)};
              odd ^= region_edge_counts(e, cx, cy);
            }
          }
          in = in && odd;
        }
      }
      const bool with_t = in && id != n_objects;
      const uint32_t tb = with_t ? crh_f2u(hit[(size_t)y * S.width + x].x) : 0u;
      unsigned long long rem = __ballot(id != kNone);
      while (rem) {
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)id, __ffsll((long long)rem) - 1);
        const bool mine = id == g;
        const unsigned long long grp = __ballot(mine), gin = __ballot(mine && in);
        rem &= ~grp;
        uint32_t f2 = 0u, f3 = 0u, f4 = 0u, f5 = 0u, f6 = 0u, f7 = 0u;
        if (gin) {
          f2 = ~(xb[j] + (uint32_t)__ffsll((long long)gin) - 1u);
          f3 = ~y;
          f4 = xb[j] + 64u - (uint32_t)__clzll((long long)gin);
          f5 = y + 1u;
          if (g != n_objects) {
            f6 = wave_umax(mine && in ? ~tb : 0u);
            f7 = wave_umax(mine && in ? tb : 0u);
          }
        }
        region_join(T, rec, lane, g, (uint32_t)__popcll(gin), (uint32_t)__popcll(grp), f2, f3, f4, f5, f6, f7);
      }
    }
  }
  // the end: every thread arrives here (the loops above have no early exit).  Each wavefront leaves its table in LDS; the first wavefront folds the entries that
  // hold the same record (they sit in the same slot of every table) into one and sends them: thread e owns field e % 8 of the slots e / 8, 8 + e / 8, 16 + e / 8 and 24 + e / 8.
  __shared__ uint32_t s_tag[kRegionBlock / 64][kRegionSlots / 8][64], s_val[kRegionBlock / 64][kRegionSlots / 8][64];
  s_tag[threadIdx.x >> 6][0][lane] = T.tag0; s_val[threadIdx.x >> 6][0][lane] = T.val0;
  s_tag[threadIdx.x >> 6][1][lane] = T.tag1; s_val[threadIdx.x >> 6][1][lane] = T.val1;
  s_tag[threadIdx.x >> 6][2][lane] = T.tag2; s_val[threadIdx.x >> 6][2][lane] = T.val2;
  s_tag[threadIdx.x >> 6][3][lane] = T.tag3; s_val[threadIdx.x >> 6][3][lane] = T.val3;
  __syncthreads();
  if (threadIdx.x >= 64u) return;
  const uint32_t q = lane & 7u;
  uint32_t id[kRegionSlots / 8], v[kRegionSlots / 8];
#pragma unroll
  for (uint32_t h = 0; h < kRegionSlots / 8u; ++h) {
    id[h] = kNone; v[h] = 0u;
#pragma unroll
    for (int w = 0; w < kRegionBlock / 64; ++w) {
      const uint32_t tw = s_tag[w][h][lane], vw = s_val[w][h][lane];
      if (tw == kNone) continue;
      if (id[h] == kNone) id[h] = tw;
      if (tw == id[h]) v[h] = q < 2u ? v[h] + vw : umax(v[h], vw);
      else region_evict(rec, tw, vw, q);              // the wavefronts disagree about a slot's record (rare): this one goes as it is
    }
  }
  // all looks first, then what they leave: one trip to memory per workgroup, not one per record
  uint32_t seen[kRegionSlots / 8];
#pragma unroll
  for (uint32_t h = 0; h < kRegionSlots / 8u; ++h)
    seen[h] = (q >= 2u && v[h]) ? __hip_atomic_load(rec + (size_t)kRegionRec * id[h] + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
  for (uint32_t h = 0; h < kRegionSlots / 8u; ++h) {
    if (!v[h]) continue;
    uint32_t* r = rec + (size_t)kRegionRec * id[h] + q;
    if (q < 2u) atomicAdd(r, v[h]);
    else if (v[h] > seen[h]) atomicMax(r, v[h]);
  }
}

}  // namespace

void launch_region_stats(hipStream_t stream, int grid, const int32_t* object, const float4* hit, const RegionEdge* edges, const RegionSetup& S, uint32_t n_objects, uint32_t* rec)
{
  if (!S.width || !S.height) return;
  const uint64_t n_chunks = (uint64_t)((S.width + 63u) >> 6) * S.height, per_group = (uint64_t)(kRegionBlock / 64) * kRegionLoads;
  const uint64_t need = (n_chunks + per_group - 1) / per_group, most = (uint64_t)(grid > 0 ? grid : 1);
  hipLaunchKernelGGL(k_region_stats, dim3((uint32_t)(need < most ? need : most)), dim3(kRegionBlock), 0, stream, object, hit, edges, S, n_objects, rec);
}

void region_stats_host(const int32_t* object, const float* t, const RegionEdge* edges, const RegionSetup& S, uint32_t n_objects, uint32_t* rec)
{
  for (uint32_t y = 0; y < S.height; ++y)
    for (uint32_t x = 0; x < S.width; ++x) {
      const size_t i = (size_t)y * S.width + x;
      const uint32_t id = region_slot(object[i], n_objects);
      uint32_t* r = rec + (size_t)kRegionRec * id;
      ++r[1];
      if (!region_in_rect(S, x, y)) continue;
      if (S.n_edges && !(region_in_box(S, x, y) && region_inside_polygon(edges, S.n_edges, x, y))) continue;
      ++r[0];
      if (~x > r[2]) r[2] = ~x;
      if (~y > r[3]) r[3] = ~y;
      if (x + 1u > r[4]) r[4] = x + 1u;
      if (y + 1u > r[5]) r[5] = y + 1u;
      if (id == n_objects) continue;
      const uint32_t tb = crh_f2u(t[i]);
      if (~tb > r[6]) r[6] = ~tb;
      if (tb > r[7]) r[7] = tb;
    }
}

}  // namespace crh
