// denoise_kernels.hip -- the denoised display, for gfx950, and the host twin: k_denoise_guide compacts per pixel what the filter needs from the first-hit id buffer and
// the per-triangle table, k_denoise_pass is one level of the a-trous filter (crh_denoise.cpp; the rules: denoise_kernels.h).
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "denoise_kernels.h"

namespace crh {
namespace {

// Data movement only.  A wavefront takes 64 consecutive pixels of ONE row: the object plane arrives as one coalesced 256-B load, the hit plane as 1 KB; the table
// record (32 B) is fetched once per pixel HERE, so that no tap of any pass ever touches the table.  Every table access is checked against n_tri.  A pixel without a
// normal (a miss, an index beyond the table, a degenerate record) carries a NaN in n.x: DenoisePlanesDevice::at reads has_n from it.
__global__ __launch_bounds__(kDenoiseBlock) void k_denoise_guide(const int32_t* __restrict__ object, const float4* __restrict__ hit, uint32_t W, uint32_t H,
                                                                 const OutlineTri* __restrict__ table, uint32_t n_tri, float4* __restrict__ guide, int2* __restrict__ ids)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;      // chunks of 64 pixels per row
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kDenoiseBlock / 64);
  for (uint64_t c = ((uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    const size_t i = (size_t)y * W + x;
    const float4 h = hit[i];
    const int32_t tri = (int32_t)crh_f2u(h.w);
    float4 g = make_float4(crh_u2f(0x7fc00000u), 0.f, 0.f, h.x);
    if (tri >= 0 && (uint32_t)tri < n_tri) {
      const OutlineTri r = table[tri];
      if (!r.degenerate) { g.x = r.nx; g.y = r.ny; g.z = r.nz; }
    }
    guide[i] = g;
    ids[i] = make_int2(object[i], tri);
  }
}

// THE PLAIN GATHER FORM.  One pixel per lane, 64 consecutive pixels of a row per wavefront: the pixel's own colour and guide arrive coalesced (1 KB + 1 KB + 512 B per
// wavefront); each of the up to 25 taps is one 16-byte colour load, one 16-byte and one 8-byte guide load at a row offset shared by the whole wavefront, so the loads
// of a tap are coalesced too, and at steps 1 and 2 neighbouring lanes and the wavefronts of the rows above and below pull the same lines through L2.  Every tap is
// checked against the frame (denoise_pixel).  No LDS, no cross-lane traffic, no atomics: every pixel writes its own 16 bytes.  `in` and `out` never alias.
__global__ __launch_bounds__(kDenoiseBlock) void k_denoise_pass(const float4* __restrict__ guide, const int2* __restrict__ ids, const float4* __restrict__ in,
                                                                float4* __restrict__ out, uint32_t W, uint32_t H, uint32_t k, DenoiseRule R)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (W + 63u) >> 6;
  const uint64_t n_chunks = (uint64_t)cpr * H, n_waves = (uint64_t)gridDim.x * (kDenoiseBlock / 64);
  const DenoisePlanesDevice P{guide, ids, in, W};
  for (uint64_t c = ((uint64_t)blockIdx.x * kDenoiseBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t y = (uint32_t)(c / cpr), x = (uint32_t)(c - (uint64_t)y * cpr) * 64u + lane;
    if (x >= W) continue;
    out[(size_t)y * W + x] = denoise_pixel(P, x, y, W, H, k, R);
  }
}

// THE LDS-STAGED FORM of steps 1 and 2, where neighbouring lanes read the same taps 25 times over.  A workgroup takes a tile of 64 x 8 pixels: all 256 threads copy the
// tile and its halo of 2 * step pixels (68 x 12 or 72 x 16 slots; colour, guide and ids: 40 B per slot) from memory into LDS -- consecutive threads take consecutive
// slots of a staged row, so the copies are coalesced runs of 16-byte, 16-byte and 8-byte loads and conflict-free LDS writes -- then every wavefront filters two rows of
// the tile, 64 consecutive pixels each, out of LDS: a tap is one ds_read_b128 pair and one ds_read_b64 at consecutive addresses across the lanes.  Slots outside the
// frame are not written and not read (denoise_pixel checks the frame first).  The SAME rule function as the plain form: the bytes are the same.
__global__ __launch_bounds__(kDenoiseBlock) void k_denoise_pass_lds(const float4* __restrict__ guide, const int2* __restrict__ ids, const float4* __restrict__ in,
                                                                    float4* __restrict__ out, uint32_t W, uint32_t H, uint32_t k, DenoiseRule R)
{
  __shared__ float4 s_col[kDenoiseSlots];
  __shared__ float4 s_gd[kDenoiseSlots];
  __shared__ int2 s_id[kDenoiseSlots];
  const uint32_t halo = 2u << k, pitch = kDenoiseTileW + 2u * halo, rows = kDenoiseTileH + 2u * halo, n_slots = pitch * rows;      // k <= 1: n_slots <= kDenoiseSlots
  const uint32_t tiles_x = (W + kDenoiseTileW - 1u) / kDenoiseTileW, tiles_y = (H + kDenoiseTileH - 1u) / kDenoiseTileH;
  const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // (uniform over the workgroup: every thread reaches both barriers)
    const uint32_t ty = (uint32_t)(tile / tiles_x), tx = (uint32_t)(tile - (uint64_t)ty * tiles_x);
    const int32_t x0 = (int32_t)(tx * kDenoiseTileW) - (int32_t)halo, y0 = (int32_t)(ty * kDenoiseTileH) - (int32_t)halo;
    for (uint32_t i = threadIdx.x; i < n_slots; i += kDenoiseBlock) {
      const uint32_t sy = i / pitch, sx = i - sy * pitch;
      const int32_t fx = x0 + (int32_t)sx, fy = y0 + (int32_t)sy;
      if (fx < 0 || fy < 0 || fx >= (int32_t)W || fy >= (int32_t)H) continue;
      const size_t j = (size_t)fy * W + (uint32_t)fx;
      s_col[i] = in[j]; s_gd[i] = guide[j]; s_id[i] = ids[j];
    }
    __syncthreads();
    const DenoisePlanesLds P{s_col, s_gd, s_id, x0, y0, pitch};
    const uint32_t x = tx * kDenoiseTileW + lane;
    for (uint32_t r = 0; r < kDenoiseTileH / 4u; ++r) {
      const uint32_t y = ty * kDenoiseTileH + wave * (kDenoiseTileH / 4u) + r;
      if (x < W && y < H) out[(size_t)y * W + x] = denoise_pixel(P, x, y, W, H, k, R);
    }
    __syncthreads();      // the next tile overwrites the slots
  }
}

uint32_t denoise_grid(uint32_t W, uint32_t H)
{
  const uint64_t n_chunks = (uint64_t)((W + 63u) >> 6) * H, per_group = kDenoiseBlock / 64;
  const uint64_t need = (n_chunks + per_group - 1) / per_group;
  return (uint32_t)(need < 65535u * 16u ? need : 65535u * 16u);      // beyond that the grid-stride loop takes the rest
}

}  // namespace

void launch_denoise_guide(hipStream_t stream, const int32_t* object, const float4* hit, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, float4* guide,
                          int2* ids)
{
  if (!W || !H) return;
  hipLaunchKernelGGL(k_denoise_guide, dim3(denoise_grid(W, H)), dim3(kDenoiseBlock), 0, stream, object, hit, W, H, table, n_tri, guide, ids);
}

void launch_denoise_pass(hipStream_t stream, const float4* guide, const int2* ids, const float4* in, float4* out, uint32_t W, uint32_t H, uint32_t k, const DenoiseRule& R,
                         bool staged)
{
  if (!W || !H) return;
  if (staged && (2u << k) <= kDenoiseMaxHalo) {
    const uint64_t n_tiles = (uint64_t)((W + kDenoiseTileW - 1u) / kDenoiseTileW) * ((H + kDenoiseTileH - 1u) / kDenoiseTileH);
    hipLaunchKernelGGL(k_denoise_pass_lds, dim3((uint32_t)(n_tiles < 65535u * 16u ? n_tiles : 65535u * 16u)), dim3(kDenoiseBlock), 0, stream, guide, ids, in, out, W, H, k, R);
    return;
  }
  hipLaunchKernelGGL(k_denoise_pass, dim3(denoise_grid(W, H)), dim3(kDenoiseBlock), 0, stream, guide, ids, in, out, W, H, k, R);
}

void denoise_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri, const DenoiseRule& R,
                  const float4* in, float4* tmp, float4* out)
{
  // the last pass writes `out`: passes alternate between the two images, backwards from there
  for (uint32_t k = 0; k < R.levels; ++k) {
    const float4* src = k == 0 ? in : (((R.levels - k) & 1u) ? tmp : out);
    float4* dst = ((R.levels - 1u - k) & 1u) ? tmp : out;
    const DenoisePlanesHost P{object, triangle, t, table, n_tri, src, W};
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) dst[(size_t)y * W + x] = denoise_pixel(P, x, y, W, H, k, R);
  }
}

}  // namespace crh
