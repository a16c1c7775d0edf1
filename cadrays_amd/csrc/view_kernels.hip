// view_kernels.hip -- the viewport read-out, for gfx950, and the host twin: the finished RGB8 frame (tone map, feature lines and overlay done) resampled to the size of
// the window that shows it, the last stage of the display chain (crh_view.cpp; the rules: view_kernels.h).
// (reference: the GL texture unit scales the FBO's RGB8 colour texture to the panel, src/Launcher/AppViewer.cxx:1095-1102)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.
#include "view_kernels.h"

namespace crh {
namespace {

// THE PLAIN GATHER, the one form that ships.  A wavefront takes 64 consecutive output pixels of ONE row; each lane reads the bytes of its own taps straight from the
// frame.  Neighbouring lanes' taps are neighbouring (minify: adjacent blocks of a row; magnify: the same one or two pixels), so a wavefront's loads of one tap row fall
// into a few cache lines.  No LDS, no cross-lane traffic, no atomics: every pixel writes its own three bytes.  Every tap index is clamped to the frame
// (view_tap_index), every output pixel is checked against the view.
// An LDS-staged form -- a workgroup loads the source footprint of a 64 x 4 output tile as aligned dwords and taps from there -- was built and measured against this one:
// it gave the same bytes and was 30 - 50 % SLOWER in every regime at 1080p and at 4K (profiles/view_ab.md), so it is not here.
__global__ __launch_bounds__(kViewBlock) void k_view(const uint8_t* __restrict__ ldr, uint32_t W, ViewAxis X, ViewAxis Y, uint8_t* __restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u, cpr = (X.v + 63u) >> 6;      // chunks of 64 output pixels per row
  const uint64_t n_chunks = (uint64_t)cpr * Y.v, n_waves = (uint64_t)gridDim.x * (kViewBlock / 64);
  const ViewFrame src{ldr, W};
  for (uint64_t c = ((uint64_t)blockIdx.x * kViewBlock + threadIdx.x) >> 6; c < n_chunks; c += n_waves) {
    const uint32_t oy = (uint32_t)(c / cpr), ox = (uint32_t)(c - (uint64_t)oy * cpr) * 64u + lane;
    if (ox >= X.v) continue;
    uint32_t p[3];
    view_pixel(src, X, Y, ox, oy, p);
    uint8_t* q = out + 3u * ((size_t)oy * X.v + ox);
    q[0] = (uint8_t)p[0]; q[1] = (uint8_t)p[1]; q[2] = (uint8_t)p[2];
  }
}

}  // namespace

void launch_view(hipStream_t stream, const uint8_t* ldr, uint32_t W, uint32_t H, const ViewPlan& P, uint8_t* out)
{
  if (!W || !H || !P.X.v || !P.Y.v) return;
  const uint64_t n_chunks = (uint64_t)((P.X.v + 63u) >> 6) * P.Y.v, per_group = kViewBlock / 64;
  const uint64_t need = (n_chunks + per_group - 1) / per_group;
  const uint32_t grid = (uint32_t)(need < 65535u * 16u ? need : 65535u * 16u);      // beyond that the grid-stride loop takes the rest
  hipLaunchKernelGGL(k_view, dim3(grid), dim3(kViewBlock), 0, stream, ldr, W, P.X, P.Y, out);
}

void view_host(const uint8_t* ldr, uint32_t W, uint32_t H, const ViewPlan& P, uint8_t* out)
{
  (void)H;
  const ViewFrame src{ldr, W};
  for (uint32_t oy = 0; oy < P.Y.v; ++oy)
    for (uint32_t ox = 0; ox < P.X.v; ++ox) {
      uint32_t p[3];
      view_pixel(src, P.X, P.Y, ox, oy, p);
      uint8_t* q = out + 3u * ((size_t)oy * P.X.v + ox);
      q[0] = (uint8_t)p[0]; q[1] = (uint8_t)p[1]; q[2] = (uint8_t)p[2];
    }
}

}  // namespace crh
