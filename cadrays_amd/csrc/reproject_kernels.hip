// reproject_kernels.hip -- reprojected display history, for gfx950, and the host twin: k_reproject_resolve blends the image an earlier view displayed into the image
// the current view is about to display (crh_reproject.cpp; the rule: reproject_kernels.h).
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "reproject_kernels.h"

namespace crh {

#include "k_pixel_ray.h"      // pixel_centre_ray: the ONE copy, shared with k_ids.h (crh_camera_rays, the id buffer)

namespace {

// THE PLAIN FORM.  One pixel per lane, 64 consecutive pixels of ONE row per wavefront: the pixel's own colour and guide arrive coalesced (1 KB + 1 KB + 512 B per
// wavefront).  The ray is computed, not loaded.  The four taps of the history -- 16 B of colour, 16 B + 8 B of guide each -- lie next to those of the neighbouring
// lanes (a translation or a dolly moves a row of pixels to a row of the old frame, a rotation to a slanted line), so L2 and the Infinity Cache serve them; every tap
// is checked against the frame (reproject_pixel).  No LDS, no cross-lane traffic, no atomics: every pixel writes its own 16 bytes.  `out` aliases no input.
__global__ __launch_bounds__(kReprojectBlock) void k_reproject_resolve(DScene S, const float4* __restrict__ guide, const int2* __restrict__ ids, const float4* __restrict__ a,
                                                                       ReprojectHistory hist, ReprojectRule R, float4* __restrict__ out)
{
  const uint32_t W = S.width, H = S.height;
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;      // chunks of 64 pixels per row
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kReprojectBlock / 64);
  const DenoisePlanesDevice C{guide, ids, a, W};
  const DenoisePlanesDevice Hs{hist.guide, hist.ids, hist.img, W};
  for (uint64_t c = ((uint64_t)blockIdx.x * kReprojectBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    crh_v3 o, d;
    pixel_centre_ray(S, x, y, o, d);
    out[(size_t)y * W + x] = reproject_pixel(C, Hs, hist.valid != 0, x, y, W, H, o, d, hist.frame, R);
  }
}

uint32_t reproject_grid(uint32_t W, uint32_t H)
{
  const uint64_t n_chunks = (uint64_t)((W + 63u) >> 6) * H, per_group = kReprojectBlock / 64;
  const uint64_t need = (n_chunks + per_group - 1) / per_group;
  return (uint32_t)(need < 65535u * 16u ? need : 65535u * 16u);      // beyond that the grid-stride loop takes the rest
}

}  // namespace

void launch_reproject_resolve(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist, const ReprojectRule& R,
                              float4* out)
{
  if (!S.width || !S.height) return;
  hipLaunchKernelGGL(k_reproject_resolve, dim3(reproject_grid(S.width, S.height)), dim3(kReprojectBlock), 0, stream, S, guide, ids, a, hist, R, out);
}

void reproject_host(const float4* a, const float* rays, const int32_t* object, const int32_t* triangle, const float* t, const float4* hist_rgba, const int32_t* hist_object,
                    const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame& F, const OutlineTri* table, uint32_t n_tri, uint32_t W, uint32_t H,
                    const ReprojectRule& R, float4* out)
{
  const DenoisePlanesHost C{object, triangle, t, table, n_tri, a, W};
  const DenoisePlanesHost Hs{hist_object, hist_triangle, hist_t, table, n_tri, hist_rgba, W};
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const float* r = rays + 8 * ((size_t)y * W + x);
      out[(size_t)y * W + x] = reproject_pixel(C, Hs, hist_rgba != nullptr, x, y, W, H, crh_mk3(r[0], r[1], r[2]), crh_mk3(r[4], r[5], r[6]), F, R);
    }
}

}  // namespace crh
