// view_kernels.h -- the viewport read-out (crh_view.cpp, view_kernels.hip): the finished RGB8 frame resampled to the size of the window that shows it -- the per-axis
// tap rule, the per-pixel rule and the exact division, ONE copy each, compiled for the gfx950 kernels and for the host twin -- and the launch wrapper.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (reference: the render target has a size of its own, SettingsWidget.cxx:104-149, and the GL texture unit scales its RGB8 colour texture to the panel,
// src/Launcher/AppViewer.cxx:929-957, :1095-1102)
//
// ARITHMETIC: integers only.  Every tap weight is an integer, the weights of an axis sum to its divisor D, and a channel is the exact quotient
// (sum + (Dx Dy) div 2) div (Dx Dy) in 64 bits.  Every pixel GATHERS.  So the device, the host twin and a numpy restatement agree bit for bit
// (tests/view_reference.py); no tolerance exists anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crh_math.h"

namespace crh {

constexpr uint32_t kViewAuto = 0u, kViewNearest = 1u, kViewBilinear = 2u, kViewArea = 3u;      // CRH_VIEW_* of include/cadrays_hip.h
constexpr uint32_t kViewMaxSide = 8192u;      // of the frame and of the view: (2 i + 1) s stays below 2^28, a channel's sum below 2^37

// One axis: s source pixels starting at `off` of a frame axis of S pixels, v output pixels, the filter in force (never AUTO: view_axis resolves it), the divisor D.
struct ViewAxis { uint32_t s, v, off, S, filter, D; };

// AUTO is chosen per axis: AREA where the axis shrinks or keeps its size, else BILINEAR
CRH_HD ViewAxis view_axis(uint32_t s, uint32_t v, uint32_t off, uint32_t S, uint32_t filter)
{
  if (filter == kViewAuto) filter = s >= v ? kViewArea : kViewBilinear;
  return ViewAxis{s, v, off, S, filter, filter == kViewArea ? s : filter == kViewBilinear ? 2u * v : 1u};
}

// THE TAP RULE.  The taps of output index i: n source indices k0, k0 + 1, ... RELATIVE to the rectangle (k0 is -1 for the first pixels of a BILINEAR magnification),
// and what their weights are computed from.
//   AREA      lo = i s, hi = (i + 1) s; k from lo div v to (hi - 1) div v; weight min((k + 1) v, hi) - max(k v, lo); D = s
//   BILINEAR  n = (2 i + 1) s - v; k0 = floor(n / 2 v); f = n - k0 2 v; taps (k0, 2 v - f) and (k0 + 1, f); D = 2 v
//   NEAREST   one tap ((2 i + 1) s) div (2 v), weight 1; D = 1
struct ViewTaps { int32_t k0; uint32_t n, lo, hi; };      // lo / hi: AREA's interval; lo: BILINEAR's f
CRH_HD ViewTaps view_taps(const ViewAxis& A, uint32_t i)
{
  if (A.filter == kViewArea) {
    const uint32_t lo = i * A.s, hi = lo + A.s, k0 = lo / A.v, k1 = (hi - 1u) / A.v;
    return ViewTaps{(int32_t)k0, k1 - k0 + 1u, lo, hi};
  }
  if (A.filter == kViewBilinear) {
    const int32_t n = (int32_t)((2u * i + 1u) * A.s) - (int32_t)A.v, d = (int32_t)(2u * A.v);
    const int32_t k0 = n >= 0 ? n / d : -((d - 1 - n) / d);      // floor division
    return ViewTaps{k0, 2u, (uint32_t)(n - k0 * d), 0u};
  }
  return ViewTaps{(int32_t)(((2u * i + 1u) * A.s) / (2u * A.v)), 1u, 0u, 0u};
}
CRH_HD uint32_t view_tap_weight(const ViewAxis& A, const ViewTaps& T, uint32_t j)
{
  if (A.filter == kViewArea) {
    const uint32_t k = (uint32_t)T.k0 + j, a = k * A.v, b = a + A.v;
    return (b < T.hi ? b : T.hi) - (a > T.lo ? a : T.lo);
  }
  if (A.filter == kViewBilinear) return j ? T.lo : 2u * A.v - T.lo;
  return 1u;
}
// ... and the FRAME index of tap j: the rectangle's offset added, then clamped to the frame [0, S - 1], NOT to the rectangle -- the pixels just outside a zoom
// rectangle are real pixels.  (Only BILINEAR ever leaves the rectangle; AREA and NEAREST stay inside it.)
CRH_HD uint32_t view_tap_index(const ViewAxis& A, const ViewTaps& T, uint32_t j)
{
  const int32_t k = (int32_t)A.off + T.k0 + (int32_t)j;
  return k < 0 ? 0u : (uint32_t)k >= A.S ? A.S - 1u : (uint32_t)k;
}

// THE DIVISION: (acc + D div 2) div D, exactly, for a quotient of at most 255 and D below 2^29.  A float32 estimate of the quotient is off by less than one (its
// relative error is below 2^-21); the remainder then corrects it, so the result does not depend on how the estimate was rounded.
CRH_HD uint32_t view_div_round(uint64_t acc, uint64_t D, float inv_D)
{
  const uint64_t num = acc + (D >> 1);
  uint32_t q = (uint32_t)((float)num * inv_D);
  int64_t r = (int64_t)num - (int64_t)((uint64_t)q * D);
  while (r < 0) { --q; r += (int64_t)D; }
  while (r >= (int64_t)D) { ++q; r -= (int64_t)D; }
  return q;
}

// THE PIXEL RULE: output pixel (ox, oy), three channels, each (sum_y w_y sum_x w_x byte + (Dx Dy) div 2) div (Dx Dy).  `src.rgb(y, x, p)` hands out the three bytes of
// frame pixel (x, y) (ViewFrame: the frame in memory, on the device and on the host).
template <class Src> CRH_HD void view_pixel(const Src& src, const ViewAxis& X, const ViewAxis& Y, uint32_t ox, uint32_t oy, uint32_t out[3])
{
  const ViewTaps tx = view_taps(X, ox), ty = view_taps(Y, oy);
  uint64_t acc[3] = {0u, 0u, 0u};
  for (uint32_t jy = 0; jy < ty.n; ++jy) {
    const uint32_t wy = view_tap_weight(Y, ty, jy), sy = view_tap_index(Y, ty, jy);
    uint32_t row[3] = {0u, 0u, 0u};      // at most Dx * 255 < 2^22
    for (uint32_t jx = 0; jx < tx.n; ++jx) {
      const uint32_t wx = view_tap_weight(X, tx, jx);
      uint32_t p[3];
      src.rgb(sy, view_tap_index(X, tx, jx), p);
      row[0] += wx * p[0]; row[1] += wx * p[1]; row[2] += wx * p[2];
    }
    acc[0] += (uint64_t)wy * row[0]; acc[1] += (uint64_t)wy * row[1]; acc[2] += (uint64_t)wy * row[2];
  }
  const uint64_t D = (uint64_t)X.D * Y.D;
  const float inv = 1.0f / (float)D;
  out[0] = view_div_round(acc[0], D, inv); out[1] = view_div_round(acc[1], D, inv); out[2] = view_div_round(acc[2], D, inv);
}

// the frame in memory: W pixels per row, 3 bytes each, rows packed
struct ViewFrame {
  const uint8_t* __restrict__ ldr; uint32_t W;
  __host__ __device__ __forceinline__ void rgb(uint32_t y, uint32_t x, uint32_t p[3]) const
  {
    const uint8_t* q = ldr + 3u * ((size_t)y * W + x);
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
  }
};

// What a read-out resamples: both axes, resolved.  identity: the view IS the frame (same size, whole rectangle) under every filter -- no kernel is launched for it.
struct ViewPlan { ViewAxis X, Y; bool identity; };

constexpr int kViewBlock = 256;             // four wavefronts, each 64 consecutive output pixels of one row

// out: P.X.v * P.Y.v * 3 bytes, written for every pixel.  ldr: the frame, W x H x 3 bytes.
void launch_view(hipStream_t stream, const uint8_t* ldr, uint32_t W, uint32_t H, const ViewPlan& P, uint8_t* out);
// the host twin: the same rule in a plain loop
void view_host(const uint8_t* ldr, uint32_t W, uint32_t H, const ViewPlan& P, uint8_t* out);

}  // namespace crh
