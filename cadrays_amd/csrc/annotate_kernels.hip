// annotate_kernels.hip -- world-space line annotations over the display, for gfx950, and the host twins: k_annot_project turns the list into screen records,
// k_annot_bin into one bitmask per tile, k_annot_draw blends the segments of a tile over the tone-mapped RGB8 bytes in ascending index, hidden, dimmed or left on top
// where the first-hit id buffer says the scene is nearer (crh_annotate.cpp; the rules: annotate_kernels.h).
// (no counterpart in the reference: ImGui paints the manipulator and the light markers over the image, src/ImGui/ImRaytraceControls.cxx:64, :93-111)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "annotate_kernels.h"

#include "device_types.h"

namespace crh {

#include "k_pixel_ray.h"      // pixel_centre_ray: the ONE copy, shared with k_ids.h (crh_camera_rays, the id buffer) and reproject_kernels.hip

namespace {

constexpr int kAnnotBlock = 256;

// One segment per lane: 32 B in, 32 B out, float64 in between.
__global__ __launch_bounds__(kAnnotBlock) void k_annot_project(AnnotCam cam, const crh_annot_segment* __restrict__ seg, uint32_t n, AnnotRecord* __restrict__ rec)
{
  const uint32_t i = blockIdx.x * kAnnotBlock + threadIdx.x;
  if (i >= n) return;
  const crh_annot_segment s = seg[i];
  rec[i] = annot_project(cam, s.a, s.b);
}

// THE GATHER FORM of the bins: one thread per (tile, word) tests the 32 boxes of its word and writes the word -- no atomics, no clear, every word written.
__global__ __launch_bounds__(kAnnotBlock) void k_annot_bin(AnnotDraw D, uint32_t* __restrict__ bins)
{
  const uint64_t k = (uint64_t)blockIdx.x * kAnnotBlock + threadIdx.x, total = (uint64_t)D.tiles_x * D.tiles_y * D.n_words;
  if (k >= total) return;
  const uint32_t w = (uint32_t)(k % D.n_words), tile = (uint32_t)(k / D.n_words), ty = tile / D.tiles_x, tx = tile - ty * D.tiles_x;
  uint32_t word = 0u;
  for (uint32_t j = 0; j < 32u; ++j) {
    const uint32_t i = w * 32u + j;
    if (i >= D.n) break;
    const AnnotRecord R = D.rec[i];
    if ((R.flags & 1u) && annot_box_meets(annot_box(R, annot_width(D.seg[i].style)), tx, ty, D.tile)) word |= 1u << j;
  }
  bins[k] = word;
}

// THE SCATTER FORM: one thread per segment ORs its bit into the words of the tiles its box meets (the buffer has been cleared in front).  The tile range is cut to the
// frame's tiles in float before it becomes an integer; the bits that arrive are the gather form's.
__global__ __launch_bounds__(kAnnotBlock) void k_annot_bin_scatter(AnnotDraw D, uint32_t* __restrict__ bins)
{
  const uint32_t i = blockIdx.x * kAnnotBlock + threadIdx.x;
  if (i >= D.n) return;
  const AnnotRecord R = D.rec[i];
  if (!(R.flags & 1u)) return;
  const AnnotBox B = annot_box(R, annot_width(D.seg[i].style));
  const float E = (float)D.tile, fx = (float)D.tiles_x, fy = (float)D.tiles_y;
  const float ax = B.lo_x / E - 1.0f, bx = B.hi_x / E + 1.0f, ay = B.lo_y / E - 1.0f, by = B.hi_y / E + 1.0f;
  if (!(bx >= 0.f && ax < fx && by >= 0.f && ay < fy)) return;
  const uint32_t tx0 = ax > 0.f ? (uint32_t)ax : 0u, ty0 = ay > 0.f ? (uint32_t)ay : 0u;
  const uint32_t tx1 = bx < fx - 1.0f ? (uint32_t)bx : D.tiles_x - 1u, ty1 = by < fy - 1.0f ? (uint32_t)by : D.tiles_y - 1u;
  for (uint32_t ty = ty0; ty <= ty1 && ty < D.tiles_y; ++ty)
    for (uint32_t tx = tx0; tx <= tx1 && tx < D.tiles_x; ++tx)
      if (annot_box_meets(B, tx, ty, D.tile)) atomicOr(&bins[((size_t)ty * D.tiles_x + tx) * D.n_words + (i >> 5)], 1u << (i & 31u));
}

// One workgroup per tile of E x E pixels, one pixel per lane.  The tile's words and the records they name are the same for every lane (scalar loads); a lane keeps
// its three bytes and its id in registers while the set bits pass by in ascending index, and writes them once.  Every access is checked: the pixel against the frame,
// the segment index against n; the words of a tile lie inside the buffer by construction (tile < tiles_x * tiles_y).
template <int E, bool Ids> __global__ __launch_bounds__(E * E) void k_annot_draw(DScene S, AnnotDraw D, uint8_t* __restrict__ ldr, int32_t* __restrict__ seg_px,
                                                                                 float* __restrict__ s_px)
{
  const uint32_t tile = blockIdx.x;
  if (tile >= D.tiles_x * D.tiles_y) return;
  const uint32_t ty = tile / D.tiles_x, tx = tile - ty * D.tiles_x;
  const uint32_t x = tx * E + threadIdx.x % E, y = ty * E + threadIdx.x / E;
  if (x >= S.width || y >= S.height) return;
  const size_t p = (size_t)y * S.width + x;
  float t = kAnnotMiss, zh = 0.f;
  if (D.hit) {
    crh_v3 o, d;
    pixel_centre_ray(S, x, y, o, d);
    const float fwd[3] = {S.fwd.x, S.fwd.y, S.fwd.z};
    t = D.hit[p].x;
    zh = annot_hit_depth(t, d.x, d.y, d.z, fwd, (uint32_t)S.is_ortho);
  }
  AnnotPixel P{0u, 0u, 0u, -1, 0.f};
  if (!Ids) { P.r = ldr[3 * p]; P.g = ldr[3 * p + 1]; P.b = ldr[3 * p + 2]; }
  const uint32_t* __restrict__ words = D.bins + (size_t)tile * D.n_words;
  for (uint32_t w = 0; w < D.n_words; ++w) {
    uint32_t word = words[w];
    while (word) {
      const uint32_t j = (uint32_t)__builtin_ctz(word);
      word &= word - 1u;
      const uint32_t i = w * 32u + j;
      if (i >= D.n) break;
      annot_apply(P, D.rec[i], D.seg[i], (int32_t)i, x, y, zh, t, D.depth_bias, D.hidden_alpha, (uint32_t)S.is_ortho);
    }
  }
  if (Ids) { seg_px[p] = P.seg; s_px[p] = P.s; }
  else if (P.seg >= 0) { ldr[3 * p] = (uint8_t)P.r; ldr[3 * p + 1] = (uint8_t)P.g; ldr[3 * p + 2] = (uint8_t)P.b; }
}

template <int E> void draw_with_edge(hipStream_t stream, const DScene& S, const AnnotDraw& D, uint8_t* ldr, int32_t* seg_px, float* s_px)
{
  const dim3 grid(D.tiles_x * D.tiles_y), block(E * E);
  if (ldr) hipLaunchKernelGGL((k_annot_draw<E, false>), grid, block, 0, stream, S, D, ldr, seg_px, s_px);
  else hipLaunchKernelGGL((k_annot_draw<E, true>), grid, block, 0, stream, S, D, ldr, seg_px, s_px);
}

}  // namespace

void launch_annot_project(hipStream_t stream, const AnnotCam& cam, const crh_annot_segment* seg, uint32_t n, AnnotRecord* rec)
{
  if (!n) return;
  hipLaunchKernelGGL(k_annot_project, dim3((n + kAnnotBlock - 1) / kAnnotBlock), dim3(kAnnotBlock), 0, stream, cam, seg, n, rec);
}

void launch_annot_bin(hipStream_t stream, const AnnotDraw& D, bool scatter, uint32_t* bins)
{
  const uint64_t total = (uint64_t)D.tiles_x * D.tiles_y * D.n_words;
  if (!total || !D.n) return;
  if (scatter) {
    (void)hipMemsetAsync(bins, 0, sizeof(uint32_t) * total, stream);      // (a failure stays in the stream's status: the caller reads hipGetLastError)
    hipLaunchKernelGGL(k_annot_bin_scatter, dim3((D.n + kAnnotBlock - 1) / kAnnotBlock), dim3(kAnnotBlock), 0, stream, D, bins);
  } else {
    hipLaunchKernelGGL(k_annot_bin, dim3((uint32_t)((total + kAnnotBlock - 1) / kAnnotBlock)), dim3(kAnnotBlock), 0, stream, D, bins);
  }
}

void launch_annot_draw(hipStream_t stream, const DScene& S, const AnnotDraw& D, uint8_t* ldr, int32_t* seg_px, float* s_px)
{
  if (!D.tiles_x || !D.tiles_y || (!ldr && !(seg_px && s_px))) return;
  if (D.tile == 8u) draw_with_edge<8>(stream, S, D, ldr, seg_px, s_px);
  else if (D.tile == 32u) draw_with_edge<32>(stream, S, D, ldr, seg_px, s_px);
  else draw_with_edge<16>(stream, S, D, ldr, seg_px, s_px);
}

void annot_project_host(const AnnotCam& cam, const crh_annot_segment* seg, uint32_t n, AnnotRecord* rec)
{
  for (uint32_t i = 0; i < n; ++i) rec[i] = annot_project(cam, seg[i].a, seg[i].b);
}

void annot_draw_host(const AnnotRecord* rec, const crh_annot_segment* seg, uint32_t n, float depth_bias, uint32_t hidden_alpha, const AnnotCam& cam, const float* rays_px,
                     const float* t_px, uint8_t* ldr, int32_t* seg_px)
{
  for (uint32_t y = 0; y < cam.H; ++y)
    for (uint32_t x = 0; x < cam.W; ++x) {
      const size_t p = (size_t)y * cam.W + x;
      float t = kAnnotMiss, zh = 0.f;
      if (rays_px && t_px) { t = t_px[p]; zh = annot_hit_depth(t, rays_px[8 * p + 4], rays_px[8 * p + 5], rays_px[8 * p + 6], cam.fwd, cam.is_ortho); }
      AnnotPixel P{0u, 0u, 0u, -1, 0.f};
      if (ldr) { P.r = ldr[3 * p]; P.g = ldr[3 * p + 1]; P.b = ldr[3 * p + 2]; }
      for (uint32_t i = 0; i < n; ++i) annot_apply(P, rec[i], seg[i], (int32_t)i, x, y, zh, t, depth_bias, hidden_alpha, cam.is_ortho);
      if (seg_px) seg_px[p] = P.seg;
      if (ldr && P.seg >= 0) { ldr[3 * p] = (uint8_t)P.r; ldr[3 * p + 1] = (uint8_t)P.g; ldr[3 * p + 2] = (uint8_t)P.b; }
    }
}

}  // namespace crh
