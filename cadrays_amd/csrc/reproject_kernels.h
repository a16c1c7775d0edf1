// reproject_kernels.h -- reprojected display history (crh_reproject.cpp, reproject_kernels.hip): the image an ending view displayed is fetched by the next view through
// the first-hit point of every pixel and blended with the new accumulator, in front of the denoise filter and the tone map.  The pixel rule -- ONE copy, compiled for
// the gfx950 kernel and for the host twin -- and the launch wrappers.  The normative text is include/cadrays_hip.h ("reprojected display history").
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// ARITHMETIC: plain float32, one operation at a time and each one rounded (the library is built with -ffp-contract=off and nothing here writes CRH_FMA), the IEEE
// division and square root, floorf; every pixel GATHERS its four taps in a fixed order, nothing is scattered and nothing depends on the order of arrival.  So the
// device, the host twin and a numpy restatement agree bit for bit (tests/reproject_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cadrays_hip.h"
#include "denoise_kernels.h"
#include "device_types.h"

namespace crh {

// crh_reproject_params as the kernel takes it: until = (float)until_samples (2^20 is exact)
struct ReprojectRule { float max_history, until, normal_cos, depth_ratio; };

// A tap of the history against pixel p of the current view: the same object, a hit, and either the same triangle or two triangles whose planes meet at less than
// the threshold angle with no step between the distance the old view EXPECTED of p's point (te) and the one it saw (q.t).
CRH_HD bool reproject_match(const DenoisePx& p, const DenoisePx& q, float te, float normal_cos, float depth_ratio)
{
  if (q.object != p.object || q.triangle < 0) return false;
  if (q.triangle == p.triangle) return true;
  if (!p.has_n || !q.has_n) return false;
  const float xy = p.nx * q.nx + p.ny * q.ny;
  const float dot = xy + p.nz * q.nz;
  if (!(crh_abs(dot) >= normal_cos)) return false;
  const float lo = te < q.t ? te : q.t, hi = te < q.t ? q.t : te;
  const float scaled = lo * depth_ratio;
  return !(hi > scaled);
}

// THE PIXEL RULE for pixel (x, y) of the current view: the float4 the denoise filter / the tone map receives.  C hands out the current view's image and guide, Hs the
// history's image (its .w the effective sample count) and guide -- DenoisePlanesDevice on the device, DenoisePlanesHost in the host twin; (o, d) is the pixel-centre
// ray; F the history's camera frame.  have_history false: every pixel passes through.  Every step is the header's, in its order.
template <class PlanesC, class PlanesH>
CRH_HD float4 reproject_pixel(const PlanesC& C, const PlanesH& Hs, bool have_history, uint32_t x, uint32_t y, uint32_t W, uint32_t H, const crh_v3& o, const crh_v3& d,
                              const crh_reproject_frame& F, const ReprojectRule& R)
{
  const float4 a = C.colour(x, y);
  if (!have_history) return a;
  const DenoisePx p = C.at(x, y);
  if (p.triangle < 0 || !denoise_finite3(a) || a.w >= R.until) return a;
  // PROJECT
  const float tx = p.t * d.x, ty = p.t * d.y, tz = p.t * d.z;
  const float Px = o.x + tx, Py = o.y + ty, Pz = o.z + tz;
  const float qx = Px - F.eye[0], qy = Py - F.eye[1], qz = Pz - F.eye[2];
  const float xr0 = qx * F.right[0], xr1 = qy * F.right[1], xr2 = qz * F.right[2];
  const float yu0 = qx * F.up[0], yu1 = qy * F.up[1], yu2 = qz * F.up[2];
  const float zf0 = qx * F.fwd[0], zf1 = qy * F.fwd[1], zf2 = qz * F.fwd[2];
  const float vx = (xr0 + xr1) + xr2, vy = (yu0 + yu1) + yu2, vz = (zf0 + zf1) + zf2;
  float nx, ny, te;
  if (!F.is_ortho) {
    if (!(vz > 0.f)) return a;
    const float den = vz * F.tan_half;
    const float denx = den * F.aspect;
    ny = vy / den; nx = vx / denx;
    const float s0 = qx * qx, s1 = qy * qy, s2 = qz * qz;
    te = crh_sqrt((s0 + s1) + s2);
  } else {
    const float denx = F.ortho_scale * F.aspect;
    ny = vy / F.ortho_scale; nx = vx / denx;
    te = vz;
    if (!(te > 0.f)) return a;
  }
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
  const float ux = nx + 1.0f, uy = 1.0f - ny;
  const float mx = ux * hw, my = uy * hh;
  const float fx = mx - 0.5f, fy = my - 0.5f;
  if (!denoise_finite(fx) || !denoise_finite(fy) || !(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H)) return a;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;      // -1 .. W - 1, -1 .. H - 1
  // GATHER
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float wgt[4] = {bx * by, ax * by, bx * ay, ax * ay};
  float S = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f; bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int32_t tx_ = x0 + (j & 1), ty_ = y0 + (j >> 1);
    if (tx_ < 0 || ty_ < 0 || tx_ >= (int32_t)W || ty_ >= (int32_t)H) continue;
    const float w = wgt[j];
    if (!(w > 0.f)) continue;
    const float4 h = Hs.colour((uint32_t)tx_, (uint32_t)ty_);
    if (!(h.w > 0.f) || !denoise_finite3(h)) continue;
    if (!reproject_match(p, Hs.at((uint32_t)tx_, (uint32_t)ty_), te, R.normal_cos, R.depth_ratio)) continue;
    const float pr = w * h.x, pg = w * h.y, pb = w * h.z, pn = w * h.w;
    S = S + w; sr = sr + pr; sg = sg + pg; sb = sb + pb; sn = sn + pn;
    any = true;
  }
  if (!any) return a;
  const float hr = sr / S, hg = sg / S, hb = sb / S, hq = sn / S;
  const float hn = hq < R.max_history ? hq : R.max_history;      // fminf
  // BLEND
  if (!(a.w > 0.f)) return make_float4(hr, hg, hb, hn);
  const float W2 = a.w + hn;
  const float ar = a.x * a.w, ag = a.y * a.w, ab = a.z * a.w;
  const float br = hr * hn, bg = hg * hn, bb = hb * hn;
  return make_float4((ar + br) / W2, (ag + bg) / W2, (ab + bb) / W2, W2);
}

// What the resolve kernel reads of the history (all W * H records; never read when `valid` is 0) ...
struct ReprojectHistory { const float4* img; const float4* guide; const int2* ids; crh_reproject_frame frame; int valid; };

// out[p] = reproject_pixel(...) for every pixel of the view S describes (its camera frame and size; the pixel-centre ray of k_pixel_ray.h); `a`, the guide planes of the
// current view and `out` hold S.width * S.height records; `out` aliases none of the inputs
void launch_reproject_resolve(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist, const ReprojectRule& R,
                              float4* out);
// the host twin: the same rule in a plain loop over host planes; rays: 8 floats per pixel {o.xyz, -, d.xyz, -}; hist_rgba == nullptr: no history
void reproject_host(const float4* a, const float* rays, const int32_t* object, const int32_t* triangle, const float* t, const float4* hist_rgba, const int32_t* hist_object,
                    const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame& F, const OutlineTri* table, uint32_t n_tri, uint32_t W, uint32_t H,
                    const ReprojectRule& R, float4* out);

constexpr int kReprojectBlock = 256;      // four wavefronts, each 64 consecutive pixels of one row

}  // namespace crh
