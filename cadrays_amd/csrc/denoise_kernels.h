// denoise_kernels.h -- the denoised display (crh_denoise.cpp, denoise_kernels.hip): an a-trous filter in front of the tone map, guided by the first-hit id buffer and
// the per-triangle normal table of the feature lines.  The similarity rule and the pixel rule -- ONE copy each, compiled for the gfx950 kernels and for the host
// twin -- the per-pixel guide record and the launch wrappers.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// ARITHMETIC: BINARY edge-stopping weights (a tap is in or out) and INTEGER spline weights; integer compares, single float32 products and sums written out without a
// fused multiply-add (the library is built with -ffp-contract=off), one float32 division per channel, no transcendental; every pixel GATHERS its own 25 taps in a
// fixed order, nothing is scattered and nothing depends on the order of arrival.  So the device, the host twin and a numpy restatement agree bit for bit
// (tests/denoise_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crh_math.h"
#include "outline_kernels.h"

namespace crh {

constexpr uint32_t kDenoiseMaxLevels = 5u;

// crh_denoise_params as the kernels take it: until = (float)until_samples
struct DenoiseRule { uint32_t levels; float normal_cos, depth_ratio, until; };

// What the rule knows of one pixel: the id buffer's object, triangle and distance, and the OBJECT-space unit normal of the triangle's table record where there is one
// (has_n: 0 <= triangle < n_tri and the record is not degenerate).
struct DenoisePx { int32_t object, triangle; float t, nx, ny, nz; bool has_n; };

CRH_HD bool denoise_finite(float v) { return (crh_f2u(v) & 0x7f800000u) != 0x7f800000u; }
CRH_HD bool denoise_finite3(const float4& c) { return denoise_finite(c.x) && denoise_finite(c.y) && denoise_finite(c.z); }

// THE SIMILARITY RULE, symmetric: the two pixels show the same object, both hit, and either the same triangle or two triangles with normals whose planes meet at
// less than the threshold angle (the outline's dot product, its order and its absolute value: meshes with inconsistent winding) and no step in first-hit distance
// (the outline's ratio test: one float32 product, rounded, then a strict compare).
CRH_HD bool denoise_similar(const DenoisePx& p, const DenoisePx& q, float normal_cos, float depth_ratio)
{
  if (p.object != q.object || p.triangle < 0 || q.triangle < 0) return false;
  if (p.triangle == q.triangle) return true;
  if (!p.has_n || !q.has_n) return false;
  const float xy = p.nx * q.nx + p.ny * q.ny;
  const float dot = xy + p.nz * q.nz;
  if (!(crh_abs(dot) >= normal_cos)) return false;
  const float lo = p.t < q.t ? p.t : q.t, hi = p.t < q.t ? q.t : p.t;
  const float scaled = lo * depth_ratio;
  return !(hi > scaled);
}

// How a pixel reads its guide: the device has the two planes k_denoise_guide compacted (a tap costs one 16-byte and one 8-byte load and nothing from the triangle
// table; a pixel without a normal carries a NaN in n.x), the host twin the three planes of crh_read_ids and the table itself.
struct DenoisePlanesDevice {
  const float4* __restrict__ guide; const int2* __restrict__ ids; const float4* __restrict__ in; uint32_t W;      // {n.x, n.y, n.z, t}, {object, triangle}, the pass's input
  __host__ __device__ __forceinline__ float4 colour(uint32_t x, uint32_t y) const { return in[(size_t)y * W + x]; }
  __host__ __device__ __forceinline__ DenoisePx at(uint32_t x, uint32_t y) const
  {
    const size_t i = (size_t)y * W + x;
    const float4 g = guide[i]; const int2 o = ids[i];
    return DenoisePx{o.x, o.y, g.w, g.x, g.y, g.z, g.x == g.x};
  }
};
struct DenoisePlanesHost {
  const int32_t* object; const int32_t* triangle; const float* t_px; const OutlineTri* table; uint32_t n_tri; const float4* in; uint32_t W;
  __host__ __device__ __forceinline__ float4 colour(uint32_t x, uint32_t y) const { return in[(size_t)y * W + x]; }
  __host__ __device__ __forceinline__ DenoisePx at(uint32_t x, uint32_t y) const
  {
    const size_t i = (size_t)y * W + x;
    DenoisePx p{object[i], triangle[i], t_px[i], 0.f, 0.f, 0.f, false};
    if (p.triangle >= 0 && (uint32_t)p.triangle < n_tri) { const OutlineTri r = table[p.triangle]; if (!r.degenerate) { p.nx = r.nx; p.ny = r.ny; p.nz = r.nz; p.has_n = true; } }
    return p;
  }
};

// ... and the LDS-staged form of steps 1 and 2 has a workgroup's tile plus its halo of all three in LDS: slot (0, 0) is frame pixel (x0, y0), which may lie outside
// the frame (such slots are never written and, as denoise_pixel checks every tap against the frame first, never read).
struct DenoisePlanesLds {
  const float4* col; const float4* gd; const int2* id; int32_t x0, y0; uint32_t pitch;
  __device__ __forceinline__ uint32_t slot(uint32_t x, uint32_t y) const { return (uint32_t)((int32_t)y - y0) * pitch + (uint32_t)((int32_t)x - x0); }
  __device__ __forceinline__ float4 colour(uint32_t x, uint32_t y) const { return col[slot(x, y)]; }
  __device__ __forceinline__ DenoisePx at(uint32_t x, uint32_t y) const
  {
    const uint32_t i = slot(x, y);
    const float4 g = gd[i]; const int2 o = id[i];
    return DenoisePx{o.x, o.y, g.w, g.x, g.y, g.z, g.x == g.x};
  }
};

// THE PIXEL RULE of pass k (step 1 << k) for pixel (x, y): the float4 of the pass's output.  P hands out the pass's input image `in` -- the accumulator for k = 0 --
// and the guide by pixel coordinates, wherever it keeps them.
//   PASS-THROUGH, all four floats bitwise: a miss (background and environment stay sharp); no sample; a colour that is not finite; or enough samples for this level,
//   !(w * 4^k < until): the coarse levels drop out first as samples arrive, and from `until` samples on the image IS the accumulator.
//   FILTER: dy = -2 .. 2 outer, dx = -2 .. 2 inner, q = (x + dx * step, y + dy * step); a tap outside the frame (nothing wraps), without a sample, with a colour that
//   is not finite or not similar to p is skipped; otherwise c = h[dy + 2] * h[dx + 2], h = {1, 4, 6, 4, 1}, an integer exact as a float, and per channel
//   sum = sum + c * in[q]: the product rounded, then the sum rounded.  The centre always counts, so the integer weight sum is >= 36.
//   OUTPUT: (sum.rgb / (float)weight sum, in[p].w): one plain division per channel.
// THE GUIDED FORM (Guided; the shade guide, shade_guide_kernels.h): P also hands out the plane G = {w.r, w.g, w.b, L} by pixel coordinates.  A pixel with G.L != 0
// passes through, a tap with G.L != 0 is skipped; a tap's channel enters as d = in[q] * G[q].w, rounded, then c * d, rounded, then the sum; the output is
// (sum / weight sum) / G[p].w: two plain divisions per channel.  A plane of (1, 1, 1, 0) gives the bytes of the unguided form, which is compiled as it was.
template <bool Guided, class Planes> CRH_HD float4 denoise_pixel_rule(const Planes& P, uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t k, const DenoiseRule& R)
{
  const float4 a = P.colour(x, y);
  const DenoisePx p = P.at(x, y);
  if (p.triangle < 0 || !(a.w > 0.f) || !denoise_finite3(a)) return a;
  if (!(a.w * (float)(1u << (2u * k)) < R.until)) return a;
  [[maybe_unused]] float gx = 1.f, gy = 1.f, gz = 1.f;
  if constexpr (Guided) { const float4 g = P.shade(x, y); if (g.w != 0.f) return a; gx = g.x; gy = g.y; gz = g.z; }
  const int32_t step = (int32_t)(1u << k);
  float sr = 0.f, sg = 0.f, sb = 0.f; uint32_t wsum = 0u;
  for (int32_t dy = -2; dy <= 2; ++dy) {
    const int32_t qy = (int32_t)y + dy * step;
    if (qy < 0 || qy >= (int32_t)H) continue;
    const uint32_t hy = dy == 0 ? 6u : ((dy == -1 || dy == 1) ? 4u : 1u);
    for (int32_t dx = -2; dx <= 2; ++dx) {
      const int32_t qx = (int32_t)x + dx * step;
      if (qx < 0 || qx >= (int32_t)W) continue;
      const float4 b = P.colour((uint32_t)qx, (uint32_t)qy);
      if (!(b.w > 0.f) || !denoise_finite3(b)) continue;
      if (!denoise_similar(p, P.at((uint32_t)qx, (uint32_t)qy), R.normal_cos, R.depth_ratio)) continue;
      float bx = b.x, by = b.y, bz = b.z;
      if constexpr (Guided) {
        const float4 g = P.shade((uint32_t)qx, (uint32_t)qy);
        if (g.w != 0.f) continue;
        bx = b.x * g.x; by = b.y * g.y; bz = b.z * g.z;
      }
      const uint32_t c = hy * (dx == 0 ? 6u : ((dx == -1 || dx == 1) ? 4u : 1u));
      const float cf = (float)c;
      const float pr = cf * bx, pg = cf * by, pb = cf * bz;
      sr = sr + pr; sg = sg + pg; sb = sb + pb;
      wsum += c;
    }
  }
  const float ws = (float)wsum;
  if constexpr (Guided) return make_float4((sr / ws) / gx, (sg / ws) / gy, (sb / ws) / gz, a.w);
  else return make_float4(sr / ws, sg / ws, sb / ws, a.w);
}
template <class Planes> CRH_HD float4 denoise_pixel(const Planes& P, uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t k, const DenoiseRule& R)
{ return denoise_pixel_rule<false>(P, x, y, W, H, k, R); }
template <class Planes> CRH_HD float4 denoise_pixel_guided(const Planes& P, uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t k, const DenoiseRule& R)
{ return denoise_pixel_rule<true>(P, x, y, W, H, k, R); }

// guide / ids: W * H records each, written for every pixel.  object / hit: the id buffer's planes; table: n_tri records on the device (not read when n_tri == 0).
void launch_denoise_guide(hipStream_t stream, const int32_t* object, const float4* hit, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float4* guide,
                          int2* ids);
// one pass: out[p] = denoise_pixel(in, p, k) for every pixel; in and out are different images of W * H float4
// staged: passes 0 and 1 (steps 1 and 2) take the LDS-staged form, the same rule over a tile and its halo in LDS; the other passes have no such form
void launch_denoise_pass(hipStream_t stream, const float4* guide, const int2* ids, const float4* in, float4* out, uint32_t W, uint32_t H, uint32_t k, const DenoiseRule& R,
                         bool staged);
// the host twin: all R.levels passes of the same rule in plain loops over host planes; tmp: W * H float4 of scratch; the result is in `out`
void denoise_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, const DenoiseRule& R,
                  const float4* in, float4* tmp, float4* out);

constexpr int kDenoiseBlock = 256;      // four wavefronts, each 64 consecutive pixels of one row
constexpr uint32_t kDenoiseTileW = 64u, kDenoiseTileH = 8u, kDenoiseMaxHalo = 4u;      // the staged form: a workgroup's tile (two rows per wavefront), the halo of step 2
constexpr uint32_t kDenoiseSlots = (kDenoiseTileW + 2u * kDenoiseMaxHalo) * (kDenoiseTileH + 2u * kDenoiseMaxHalo);      // 72 x 16 slots of 40 B: 45 KB of LDS

}  // namespace crh
