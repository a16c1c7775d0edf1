// outline_kernels.hip -- feature lines on the display, for gfx950, and the host twins: k_outline_mask turns the first-hit id buffer into one byte per pixel (object,
// depth and crease edges), k_outline_draw blends the lines over the tone-mapped RGB8 bytes (crh_outline.cpp; the rules: outline_kernels.h).
// (the reference has no counterpart: OCCT's path tracer draws no edges, src/Launcher/DataNode.cxx:286 only sets a display mode of the rasteriser)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "outline_kernels.h"

namespace crh {
namespace {

// THE PLAIN FORM.  A wavefront takes 64 consecutive pixels of ONE row: the object plane arrives as one coalesced 256-B load, the hit plane as 1 KB, and the four
// neighbours are read straight from memory as k_overlay reads them (the rows above and below are the same lines another wavefront's own pixels pull through L2).
// Table records (32 B) are fetched only by a pixel that is the marked one of a same-object pair whose triangles differ.  Every neighbour access is checked against
// the frame, every table access against n_tri (outline_pixel / outline_pair_kinds).  No LDS, no cross-lane traffic, no atomics: every pixel writes its own byte.
__global__ __launch_bounds__(kOutlineBlock) void k_outline_mask(const int32_t* __restrict__ object, const float4* __restrict__ hit, uint32_t W, uint32_t H,
                                                                const OutlineTri* __restrict__ table, uint32_t n_tri, float crease_cos, float depth_ratio,
                                                                uint8_t* __restrict__ mask)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;      // chunks of 64 pixels per row
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kOutlineBlock / 64);
  const OutlinePlanesDevice P{object, hit};
  for (uint64_t c = ((uint64_t)blockIdx.x * kOutlineBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    mask[(size_t)y * W + x] = (uint8_t)outline_pixel(P, x, y, W, H, table, n_tri, crease_cos, depth_ratio);
  }
}

// One thread per pixel, the same chunks: up to nine mask bytes of the window (rows adjacent in L2), and only a drawn pixel touches its three bytes of the frame.
__global__ __launch_bounds__(kOutlineBlock) void k_outline_draw(const uint8_t* __restrict__ mask, uint32_t W, uint32_t H, OutlineDraw D, uint8_t* __restrict__ ldr)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kOutlineBlock / 64);
  for (uint64_t c = ((uint64_t)blockIdx.x * kOutlineBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W || !outline_drawn(mask, x, y, W, H, D.kinds, D.width)) continue;
    uint8_t* p = ldr + 3u * ((size_t)y * W + x);
    p[0] = (uint8_t)outline_blend(p[0], D.r, D.alpha); p[1] = (uint8_t)outline_blend(p[1], D.g, D.alpha); p[2] = (uint8_t)outline_blend(p[2], D.b, D.alpha);
  }
}

uint32_t outline_grid(uint32_t W, uint32_t H)
{
  const uint64_t n_chunks = (uint64_t)((W + 63u) >> 6) * H, per_group = kOutlineBlock / 64;
  const uint64_t need = (n_chunks + per_group - 1) / per_group;
  return (uint32_t)(need < 65535u * 16u ? need : 65535u * 16u);      // beyond that the grid-stride loop takes the rest
}

}  // namespace

void launch_outline_mask(hipStream_t stream, const int32_t* object, const float4* hit, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float crease_cos,
                         float depth_ratio, uint8_t* mask)
{
  if (!W || !H) return;
  hipLaunchKernelGGL(k_outline_mask, dim3(outline_grid(W, H)), dim3(kOutlineBlock), 0, stream, object, hit, W, H, table, n_tri, crease_cos, depth_ratio, mask);
}

void launch_outline_draw(hipStream_t stream, const uint8_t* mask, uint32_t W, uint32_t H, const OutlineDraw& D, uint8_t* ldr)
{
  if (!W || !H) return;
  hipLaunchKernelGGL(k_outline_draw, dim3(outline_grid(W, H)), dim3(kOutlineBlock), 0, stream, mask, W, H, D, ldr);
}

void outline_mask_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float crease_cos,
                       float depth_ratio, uint8_t* mask)
{
  const OutlinePlanesHost P{object, triangle, t};
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) mask[(size_t)y * W + x] = (uint8_t)outline_pixel(P, x, y, W, H, table, n_tri, crease_cos, depth_ratio);
}

void outline_draw_host(const uint8_t* mask, uint32_t W, uint32_t H, const OutlineDraw& D, uint8_t* ldr)
{
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      if (!outline_drawn(mask, x, y, W, H, D.kinds, D.width)) continue;
      uint8_t* p = ldr + 3u * ((size_t)y * W + x);
      p[0] = (uint8_t)outline_blend(p[0], D.r, D.alpha); p[1] = (uint8_t)outline_blend(p[1], D.g, D.alpha); p[2] = (uint8_t)outline_blend(p[2], D.b, D.alpha);
    }
}

}  // namespace crh
