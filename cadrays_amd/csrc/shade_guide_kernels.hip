// shade_guide_kernels.hip -- the shade guide of the denoised display, for gfx950, and the host twins: k_shade_guide_seen flags the pixels whose centre ray shows a
// positional light, k_shade_guide_plane writes per pixel the reciprocal albedo of the first hit and the dilated flag, k_denoise_pass_guided is one level of the
// a-trous filter over the demodulated image (crh_shade_guide.cpp; the rules: shade_guide_kernels.h, denoise_kernels.h).
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "shade_guide_kernels.h"

namespace crh {

#include "k_pixel_ray.h"      // pixel_centre_ray: the ONE copy, shared with k_ids.h (crh_camera_rays, the id buffer)

namespace {

constexpr int kShadeGuideBlock = 256;      // four wavefronts, each 64 consecutive pixels of one row

// One pixel per lane, 64 consecutive pixels of ONE row per wavefront.  The ray is computed, not loaded; the hit record arrives as one coalesced 1-KB load; the few
// lights are read through the scalar cache (the same address in every lane).  Every pixel writes its own byte.
__global__ __launch_bounds__(kShadeGuideBlock) void k_shade_guide_seen(DScene S, const float4* __restrict__ hit, uint8_t* __restrict__ seen)
{
  const uint32_t W = S.width, H = S.height;
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;      // chunks of 64 pixels per row
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kShadeGuideBlock / 64);
  for (uint64_t c = ((uint64_t)blockIdx.x * kShadeGuideBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    const size_t i = (size_t)y * W + x;
    const float4 h = hit[i];
    crh_v3 o, d;
    pixel_centre_ray(S, x, y, o, d);
    const float hd = (int32_t)crh_f2u(h.w) >= 0 ? h.x : CRH_MAXFLOAT;
    seen[i] = shade_guide_seen(S.lights, S.n_lights, o, d, hd) ? 1u : 0u;
  }
}

// Data movement and one texture lookup per pixel.  The hit record arrives coalesced; the table record (32 B) and the material (five 16-byte loads of a 128-B record
// that neighbouring pixels share) come through L2; the four texels of a textured pixel lie next to those of the neighbouring lanes.  Every table, material, slot and
// texel index is checked or wrapped (shade_guide_weight, shade_guide_texel); the up to 25 flag bytes of the dilation are checked against the frame.  Every pixel
// writes its own 16 bytes.
__global__ __launch_bounds__(kShadeGuideBlock) void k_shade_guide_plane(ShadeGuideScene S, const float4* __restrict__ hit, uint32_t W, uint32_t H,
                                                                        const GuideTri* __restrict__ table, uint32_t n_tri, const uint8_t* __restrict__ seen,
                                                                        ShadeGuideRule R, float4* __restrict__ plane)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kShadeGuideBlock / 64);
  for (uint64_t c = ((uint64_t)blockIdx.x * kShadeGuideBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    const size_t i = (size_t)y * W + x;
    const float4 h = hit[i];
    plane[i] = shade_guide_pixel(S, table, n_tri, (int32_t)crh_f2u(h.w), h.y, h.z, seen, x, y, W, H, R);
  }
}

// THE PLAIN GATHER FORM of the guided pass: k_denoise_pass (denoise_kernels.hip) with one more coalesced 16-byte load per tap, the plane's.  One pixel per lane, no
// LDS, no cross-lane traffic, no atomics; every tap is checked against the frame (denoise_pixel_rule).  `in` and `out` never alias.
__global__ __launch_bounds__(kDenoiseBlock) void k_denoise_pass_guided(const float4* __restrict__ guide, const int2* __restrict__ ids, const float4* __restrict__ plane,
                                                                       const float4* __restrict__ in, float4* __restrict__ out, uint32_t W, uint32_t H, uint32_t k,
                                                                       DenoiseRule R)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kDenoiseBlock / 64);
  const DenoisePlanesGuidedDevice P{{guide, ids, in, W}, plane};
  for (uint64_t c = ((uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    out[(size_t)y * W + x] = denoise_pixel_guided(P, x, y, W, H, k, R);
  }
}

uint32_t row_chunk_grid(uint32_t W, uint32_t H, int block)
{
  const uint64_t n_chunks = (uint64_t)((W + 63u) >> 6) * H, per_group = (uint64_t)block / 64;
  const uint64_t need = (n_chunks + per_group - 1) / per_group;
  return (uint32_t)(need < 65535u * 16u ? need : 65535u * 16u);      // beyond that the grid-stride loop takes the rest
}

}  // namespace

void launch_shade_guide_seen(hipStream_t stream, const DScene& S, const float4* hit, uint8_t* seen)
{
  if (!S.width || !S.height) return;
  hipLaunchKernelGGL(k_shade_guide_seen, dim3(row_chunk_grid(S.width, S.height, kShadeGuideBlock)), dim3(kShadeGuideBlock), 0, stream, S, hit, seen);
}

void launch_shade_guide_plane(hipStream_t stream, const ShadeGuideScene& S, const float4* hit, uint32_t W, uint32_t H, const GuideTri* table, uint32_t n_tri,
                              const uint8_t* seen, const ShadeGuideRule& R, float4* plane)
{
  if (!W || !H) return;
  hipLaunchKernelGGL(k_shade_guide_plane, dim3(row_chunk_grid(W, H, kShadeGuideBlock)), dim3(kShadeGuideBlock), 0, stream, S, hit, W, H, table, n_tri, seen, R, plane);
}

void launch_denoise_pass_guided(hipStream_t stream, const float4* guide, const int2* ids, const float4* plane, const float4* in, float4* out, uint32_t W, uint32_t H,
                                uint32_t k, const DenoiseRule& R)
{
  if (!W || !H) return;
  hipLaunchKernelGGL(k_denoise_pass_guided, dim3(row_chunk_grid(W, H, kDenoiseBlock)), dim3(kDenoiseBlock), 0, stream, guide, ids, plane, in, out, W, H, k, R);
}

void shade_guide_host(const ShadeGuideScene& S, const float* rays, const int32_t* triangle, const float* t, const float* uv, uint32_t W, uint32_t H, const GuideTri* table,
                      uint32_t n_tri, const ShadeGuideRule& R, uint8_t* seen, float4* plane)
{
  const size_t n = (size_t)W * H;
  for (size_t i = 0; i < n; ++i) {
    const float* r = rays + 8 * i;
    const float hd = triangle[i] >= 0 ? t[i] : CRH_MAXFLOAT;
    seen[i] = shade_guide_seen(S.lights, S.n_lights, crh_mk3(r[0], r[1], r[2]), crh_mk3(r[4], r[5], r[6]), hd) ? 1u : 0u;
  }
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      plane[i] = shade_guide_pixel(S, table, n_tri, triangle[i], uv[2 * i], uv[2 * i + 1], seen, x, y, W, H, R);
    }
}

void denoise_guided_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri,
                         const float4* plane, const DenoiseRule& R, const float4* in, float4* tmp, float4* out)
{
  // the last pass writes `out`: passes alternate between the two images, backwards from there (as denoise_host)
  for (uint32_t k = 0; k < R.levels; ++k) {
    const float4* src = k == 0 ? in : (((R.levels - k) & 1u) ? tmp : out);
    float4* dst = ((R.levels - 1u - k) & 1u) ? tmp : out;
    const DenoisePlanesGuidedHost P{{object, triangle, t, table, n_tri, src, W}, plane};
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) dst[(size_t)y * W + x] = denoise_pixel_guided(P, x, y, W, H, k, R);
  }
}

}  // namespace crh
