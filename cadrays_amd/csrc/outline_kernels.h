// outline_kernels.h -- feature lines on the display (crh_outline.cpp, outline_kernels.hip): the per-triangle record, the pair rule and the drawing rule -- ONE copy
// each, compiled for the gfx950 kernels and for the host twins -- and the launch wrappers.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (the reference has no counterpart: OCCT's path tracer draws no edges, src/Launcher/DataNode.cxx:286 only sets a display mode of the rasteriser)
//
// ARITHMETIC: integer compares, one float32 product and one float32 dot product written out without a fused multiply-add (the library is built with
// -ffp-contract=off), no transcendental; every pixel GATHERS its own four pairs, nothing is scattered and nothing depends on the order of arrival.  So the
// device, the host twin and a numpy restatement agree bit for bit (tests/outline_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crh_math.h"

namespace crh {

constexpr uint32_t kOutlineObject = 1u, kOutlineDepth = 2u, kOutlineCrease = 4u, kOutlineAll = 7u;      // CRH_OUTLINE_* of include/cadrays_hip.h

// One record per triangle, in the caller's triangle order (the numbering of `triangle` in the id buffer): the unit normal in OBJECT space, whether there is none,
// the three vertex indices as the context stores them.  32 B: two 16-byte loads.
struct alignas(16) OutlineTri { float nx, ny, nz; uint32_t degenerate; uint32_t v0, v1, v2, pad; };

// The record of one triangle from its three positions (float, as handed over), in double, in this order: widen; a = p1 - p0, b = p2 - p0; c = a x b, every
// product rounded, then the difference; l = sqrt((c.x c.x + c.y c.y) + c.z c.z); n = (float)(c / l) if l > 0 and finite, else n = 0 and degenerate = 1.
inline OutlineTri outline_record(const float* p0, const float* p1, const float* p2, uint32_t v0, uint32_t v1, uint32_t v2)
{
  const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
  const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double l = __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
  OutlineTri r{0.f, 0.f, 0.f, 1u, v0, v1, v2, 0u};
  if (l > 0.0 && l <= 1.7976931348623157e308) { r.nx = (float)(cx / l); r.ny = (float)(cy / l); r.nz = (float)(cz / l); r.degenerate = 0u; }
  return r;
}

// THE RULE for one pair of 4-neighbours (a, b), a left of b or above b: the kinds the pair carries (0: none).  A miss carries object -1, triangle -1 and t = 1e15,
// as the id buffer writes it.
//   OBJECT  the two objects differ.
//   otherwise, both hit, the triangles differ and both indices lie below n_tri:
//   DEPTH   no vertex index of one triangle equals one of the other (nine integer compares: indices, not positions) and hi > lo * depth_ratio, lo / hi the smaller /
//           larger t: one float32 product, rounded, then a strict compare
//   CREASE  neither record is degenerate and |(n.x m.x + n.y m.y) + n.z m.z| < crease_cos, plain float32.  The absolute value is deliberate: meshes with inconsistent
//           winding are common.
// Table records are fetched only here, for pairs of one object whose triangles differ.
CRH_HD uint32_t outline_pair_kinds(int32_t oa, int32_t ob, int32_t ta, int32_t tb, float da, float db, const OutlineTri* __restrict__ table, uint32_t n_tri, float crease_cos,
                                   float depth_ratio)
{
  if (oa != ob) return kOutlineObject;
  if (ta < 0 || tb < 0 || ta == tb || (uint32_t)ta >= n_tri || (uint32_t)tb >= n_tri) return 0u;
  const OutlineTri A = table[ta], B = table[tb];
  uint32_t k = 0u;
  const bool shared = A.v0 == B.v0 || A.v0 == B.v1 || A.v0 == B.v2 || A.v1 == B.v0 || A.v1 == B.v1 || A.v1 == B.v2 || A.v2 == B.v0 || A.v2 == B.v1 || A.v2 == B.v2;
  const float lo = da < db ? da : db, hi = da < db ? db : da;
  const float scaled = lo * depth_ratio;
  if (!shared && hi > scaled) k |= kOutlineDepth;
  const float xy = A.nx * B.nx + A.ny * B.ny;
  const float dot = xy + A.nz * B.nz;
  if (!A.degenerate && !B.degenerate && crh_abs(dot) < crease_cos) k |= kOutlineCrease;
  return k;
}

// How a pixel reads the id buffer: the device has the object plane and the 16-byte hit plane {t, u, v, triangle}, the host twin three planes.
struct OutlinePlanesDevice {
  const int32_t* __restrict__ object; const float4* __restrict__ hit;
  __host__ __device__ __forceinline__ void at(size_t i, int32_t& o, int32_t& tri, float& t) const { const float4 h = hit[i]; o = object[i]; tri = (int32_t)crh_f2u(h.w); t = h.x; }
};
struct OutlinePlanesHost {
  const int32_t* object; const int32_t* triangle; const float* t_px;
  __host__ __device__ __forceinline__ void at(size_t i, int32_t& o, int32_t& tri, float& t) const { o = object[i]; tri = triangle[i]; t = t_px[i]; }
};

// One pixel's byte, as a GATHER: the OR of the kinds of those of its up to four pairs in which IT is the marked pixel.  In a pair (a, b) with any kind the marked pixel
// is b if t[b] < t[a], else a: the line lies on the nearer surface, and on a tie (coincident faces included) it goes to a.  Nothing pairs across the frame border:
// every neighbour access is checked against the frame.
template <class Planes> CRH_HD uint32_t outline_pixel(const Planes& P, uint32_t x, uint32_t y, uint32_t W, uint32_t H, const OutlineTri* __restrict__ table, uint32_t n_tri,
                                                      float crease_cos, float depth_ratio)
{
  const size_t i = (size_t)y * W + x;
  int32_t o, tri, on, trin; float t, tn;
  P.at(i, o, tri, t);
  uint32_t m = 0u;
  if (x > 0u) {          // (left, this): this pixel is b
    P.at(i - 1u, on, trin, tn);
    if (t < tn) m |= outline_pair_kinds(on, o, trin, tri, tn, t, table, n_tri, crease_cos, depth_ratio);
  }
  if (y > 0u) {          // (above, this): this pixel is b
    P.at(i - W, on, trin, tn);
    if (t < tn) m |= outline_pair_kinds(on, o, trin, tri, tn, t, table, n_tri, crease_cos, depth_ratio);
  }
  if (x + 1u < W) {      // (this, right): this pixel is a
    P.at(i + 1u, on, trin, tn);
    if (!(tn < t)) m |= outline_pair_kinds(o, on, tri, trin, t, tn, table, n_tri, crease_cos, depth_ratio);
  }
  if (y + 1u < H) {      // (this, below): this pixel is a
    P.at(i + W, on, trin, tn);
    if (!(tn < t)) m |= outline_pair_kinds(o, on, tri, trin, t, tn, table, n_tri, crease_cos, depth_ratio);
  }
  return m;
}

// THE DRAWING RULE.  The window of a line `width` pixels wide: offsets dx, dy in [-floor((width - 1) / 2), ceil((width - 1) / 2)], cut to the frame -- the pixel itself,
// 2 x 2, 3 x 3 centred.  A pixel is drawn iff some pixel of its window carries one of the kinds that are drawn.
CRH_HD bool outline_drawn(const uint8_t* __restrict__ mask, uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t kinds, uint32_t width)
{
  const int32_t lo = -(int32_t)((width - 1u) / 2u), hi = (int32_t)(width / 2u);
  uint32_t any = 0u;
  for (int32_t dy = lo; dy <= hi; ++dy)
    for (int32_t dx = lo; dx <= hi; ++dx) {
      const int32_t qx = (int32_t)x + dx, qy = (int32_t)y + dy;
      if (qx < 0 || qy < 0 || qx >= (int32_t)W || qy >= (int32_t)H) continue;
      any |= mask[(size_t)qy * W + (uint32_t)qx];
    }
  return (any & kinds) != 0u;
}
// ... and a drawn pixel becomes the colour itself for alpha 255, else the selection interior's formula
CRH_HD uint32_t outline_blend(uint32_t ldr, uint32_t colour, uint32_t alpha) { return alpha == 255u ? colour : (ldr * (256u - alpha) + colour * alpha + 128u) >> 8; }

struct OutlineDraw { uint32_t kinds, width, r, g, b, alpha; };

// mask: W * H bytes, written for every pixel.  object / hit: the id buffer's planes; table: n_tri records on the device (not read when n_tri == 0).
void launch_outline_mask(hipStream_t stream, const int32_t* object, const float4* hit, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float crease_cos,
                         float depth_ratio, uint8_t* mask);
// ldr: W * H * 3 bytes, blended in place (a pixel reads the mask's window and its own three bytes only)
void launch_outline_draw(hipStream_t stream, const uint8_t* mask, uint32_t W, uint32_t H, const OutlineDraw& D, uint8_t* ldr);
// the host twins: the same rules in plain loops over host planes
void outline_mask_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float crease_cos,
                       float depth_ratio, uint8_t* mask);
void outline_draw_host(const uint8_t* mask, uint32_t W, uint32_t H, const OutlineDraw& D, uint8_t* ldr);

constexpr int kOutlineBlock = 256;      // four wavefronts, each 64 consecutive pixels of one row

}  // namespace crh
