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

// THE MOTION FORM (per-object history deltas): the same mapping, the same loads, and per pixel the 4-byte flag of the pixel's object -- 64 lanes of a row mostly
// share one or two objects, so the flags and the 48-byte D records of a wavefront are a handful of cache lines.  Only lanes whose flag is 1 fetch D; a wavefront
// whose ballot shows no such lane skips fetch and transform (ReprojectMotion::lookup).  Every index into the table is checked against n_objects.  No LDS, no
// atomics, no scatter; `out` aliases no input.  Launched only while a record is flagged: a pure camera drag keeps k_reproject_resolve.
__global__ __launch_bounds__(kReprojectBlock) void k_reproject_resolve_motion(DScene S, const float4* __restrict__ guide, const int2* __restrict__ ids, const float4* __restrict__ a,
                                                                              ReprojectHistory hist, ReprojectRule R, ReprojectMotion M, float4* __restrict__ out)
{
  const uint32_t W = S.width, H = S.height;
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kReprojectBlock / 64);
  const DenoisePlanesDevice C{guide, ids, a, W};
  const DenoisePlanesDevice Hs{hist.guide, hist.ids, hist.img, W};
  for (uint64_t c = ((uint64_t)blockIdx.x * kReprojectBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    crh_v3 o, d;
    pixel_centre_ray(S, x, y, o, d);
    out[(size_t)y * W + x] = reproject_pixel_rule<true>(C, Hs, hist.valid != 0, x, y, W, H, o, d, hist.frame, R, M);
  }
}

// THE STAGED FORM of the motion kernel, the issue's one alternative (measured: profiles/reproject_ab.md 6.1): 4 KB of LDS per workgroup hold the flag-1 records;
// thread t copies quarter t & 3 of record t >> 2 (256 threads = 64 records x 4 float4), one barrier, then the plain mapping.  A lane reads its object's flag and
// slot in ONE 8-byte load and D from LDS, so the second dependent memory load of the plain form is an LDS read.  slot & 63 keeps any word inside the array.
struct ReprojectMotionLds {
  const ReprojectDelta* table; uint32_t n_objects; float max_moved, max_static; int capped; const ReprojectDelta* lds;
  __device__ __forceinline__ uint32_t lookup(int32_t object, float4& r0, float4& r1, float4& r2) const
  {
    uint32_t flag = 0u, slot = 0u;
    if ((uint32_t)object < n_objects) { const uint2 w = *reinterpret_cast<const uint2*>(&table[object].flag); flag = w.x; slot = w.y; }
    if (flag == 1u) { const ReprojectDelta& r = lds[slot & (kReprojectStagedMax - 1u)]; r0 = r.r0; r1 = r.r1; r2 = r.r2; }
    return flag;
  }
};

__global__ __launch_bounds__(kReprojectBlock) void k_reproject_resolve_motion_staged(DScene S, const float4* __restrict__ guide, const int2* __restrict__ ids,
                                                                                     const float4* __restrict__ a, ReprojectHistory hist, ReprojectRule R, ReprojectMotion M,
                                                                                     uint32_t n_staged, float4* __restrict__ out)
{
  __shared__ ReprojectDelta staged[kReprojectStagedMax];
  {
    const uint32_t rec = threadIdx.x >> 2, q = threadIdx.x & 3u;
    if (rec < n_staged && rec < kReprojectStagedMax) reinterpret_cast<float4*>(&staged[rec])[q] = reinterpret_cast<const float4*>(&M.table[M.n_objects + rec])[q];
  }
  __syncthreads();
  const ReprojectMotionLds L{M.table, M.n_objects, M.max_moved, M.max_static, M.capped, staged};
  const uint32_t W = S.width, H = S.height;
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kReprojectBlock / 64);
  const DenoisePlanesDevice C{guide, ids, a, W};
  const DenoisePlanesDevice Hs{hist.guide, hist.ids, hist.img, W};
  for (uint64_t c = ((uint64_t)blockIdx.x * kReprojectBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    crh_v3 o, d;
    pixel_centre_ray(S, x, y, o, d);
    out[(size_t)y * W + x] = reproject_pixel_rule<true>(C, Hs, hist.valid != 0, x, y, W, H, o, d, hist.frame, R, L);
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

void launch_reproject_resolve_motion(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist,
                                     const ReprojectRule& R, const ReprojectMotion& M, float4* out)
{
  if (!S.width || !S.height) return;
  hipLaunchKernelGGL(k_reproject_resolve_motion, dim3(reproject_grid(S.width, S.height)), dim3(kReprojectBlock), 0, stream, S, guide, ids, a, hist, R, M, out);
}

void launch_reproject_resolve_motion_staged(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist,
                                            const ReprojectRule& R, const ReprojectMotion& M, uint32_t n_staged, float4* out)
{
  if (!S.width || !S.height) return;
  hipLaunchKernelGGL(k_reproject_resolve_motion_staged, dim3(reproject_grid(S.width, S.height)), dim3(kReprojectBlock), 0, stream, S, guide, ids, a, hist, R, M,
                     n_staged > kReprojectStagedMax ? kReprojectStagedMax : n_staged, out);
}

void reproject_motion_host(const float4* a, const float* rays, const int32_t* object, const int32_t* triangle, const float* t, const float4* hist_rgba, const int32_t* hist_object,
                           const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame& F, const OutlineTri* table, uint32_t n_tri, uint32_t W, uint32_t H,
                           const ReprojectRule& R, const ReprojectMotion& M, float4* out)
{
  if (!M.table) { reproject_host(a, rays, object, triangle, t, hist_rgba, hist_object, hist_triangle, hist_t, F, table, n_tri, W, H, R, out); return; }
  const DenoisePlanesHost C{object, triangle, t, table, n_tri, a, W};
  const DenoisePlanesHost Hs{hist_object, hist_triangle, hist_t, table, n_tri, hist_rgba, W};
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const float* r = rays + 8 * ((size_t)y * W + x);
      out[(size_t)y * W + x] = reproject_pixel_rule<true>(C, Hs, hist_rgba != nullptr, x, y, W, H, crh_mk3(r[0], r[1], r[2]), crh_mk3(r[4], r[5], r[6]), F, R, M);
    }
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
