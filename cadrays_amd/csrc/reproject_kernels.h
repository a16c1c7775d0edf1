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

// A record of THE DELTA TABLE (crh_reproject_delta) as the rule reads it: the rows of D as three float4 {D[4k], D[4k+1], D[4k+2], D[4k+3]}
// On the DEVICE pad[0] of a flag-1 record is its slot among the flag-1 records (the staged form's index into LDS); the host twin's table has zero pads.
struct ReprojectDelta { float4 r0, r1, r2; uint32_t flag, pad[3]; };
static_assert(sizeof(ReprojectDelta) == 64 && sizeof(crh_reproject_delta) == 64, "a delta record is 64 bytes");

// The table in force and the two caps; capped = a record has a non-zero flag.  lookup: the flag of `object` (0 outside the table) and, for flag 1 only, D.  On the
// device the 4-byte flag is read per lane, the 48 bytes of D only by the lanes whose flag is 1, and a wavefront whose ballot shows no such lane skips the fetch as a whole.
struct ReprojectMotion {
  const ReprojectDelta* table = nullptr; uint32_t n_objects = 0; float max_moved = 0.f, max_static = 0.f; int capped = 0;
  CRH_HD uint32_t lookup(int32_t object, float4& r0, float4& r1, float4& r2) const
  {
    uint32_t flag = 0u;
    if ((uint32_t)object < n_objects) flag = table[object].flag;
#if defined(__HIP_DEVICE_COMPILE__)
    if (__ballot(flag == 1u) == 0ull) return flag;
#endif
    if (flag == 1u) { const ReprojectDelta& r = table[object]; r0 = r.r0; r1 = r.r1; r2 = r.r2; }
    return flag;
  }
};

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
// Motion false: the rule of "reprojected display history", and M is never looked at; true: that of "per-object history deltas" with the table M describes.
// MotionT: where the table's records come from -- ReprojectMotion (memory) or the LDS-staged form of reproject_kernels.hip; the arithmetic is the same.
template <bool Motion, class PlanesC, class PlanesH, class MotionT>
CRH_HD float4 reproject_pixel_rule(const PlanesC& C, const PlanesH& Hs, bool have_history, uint32_t x, uint32_t y, uint32_t W, uint32_t H, const crh_v3& o, const crh_v3& d,
                                   const crh_reproject_frame& F, const ReprojectRule& R, const MotionT& M)
{
  const float4 a = C.colour(x, y);
  if (!have_history) return a;
  const DenoisePx p = C.at(x, y);
  if (p.triangle < 0 || !denoise_finite3(a) || a.w >= R.until) return a;
  // PROJECT
  const float tx = p.t * d.x, ty = p.t * d.y, tz = p.t * d.z;
  float Px = o.x + tx, Py = o.y + ty, Pz = o.z + tz;
  [[maybe_unused]] uint32_t flag = 0u;
  if constexpr (Motion) {
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    flag = M.lookup(p.object, r0, r1, r2);
    if (flag == 2u) return a;
    if (flag == 1u) {
      const float x0_ = r0.x * Px, x1_ = r0.y * Py, x2_ = r0.z * Pz;
      const float y0_ = r1.x * Px, y1_ = r1.y * Py, y2_ = r1.z * Pz;
      const float z0_ = r2.x * Px, z1_ = r2.y * Py, z2_ = r2.z * Pz;
      const float nx_ = ((x0_ + x1_) + x2_) + r0.w, ny_ = ((y0_ + y1_) + y2_) + r1.w, nz_ = ((z0_ + z1_) + z2_) + r2.w;
      Px = nx_; Py = ny_; Pz = nz_;
    }
  }
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
  float hn = hq < R.max_history ? hq : R.max_history;      // fminf
  if constexpr (Motion) {                                  // CAP
    if (M.capped) { const float cap = flag == 1u ? M.max_moved : M.max_static; hn = hn < cap ? hn : cap; }
  }
  // BLEND
  if (!(a.w > 0.f)) return make_float4(hr, hg, hb, hn);
  const float W2 = a.w + hn;
  const float ar = a.x * a.w, ag = a.y * a.w, ab = a.z * a.w;
  const float br = hr * hn, bg = hg * hn, bb = hb * hn;
  return make_float4((ar + br) / W2, (ag + bg) / W2, (ab + bb) / W2, W2);
}

template <class PlanesC, class PlanesH>
CRH_HD float4 reproject_pixel(const PlanesC& C, const PlanesH& Hs, bool have_history, uint32_t x, uint32_t y, uint32_t W, uint32_t H, const crh_v3& o, const crh_v3& d,
                              const crh_reproject_frame& F, const ReprojectRule& R)
{
  return reproject_pixel_rule<false>(C, Hs, have_history, x, y, W, H, o, d, F, R, ReprojectMotion{});
}

// What the resolve kernel reads of the history (all W * H records; never read when `valid` is 0) ...
struct ReprojectHistory { const float4* img; const float4* guide; const int2* ids; crh_reproject_frame frame; int valid; };

// out[p] = reproject_pixel(...) for every pixel of the view S describes (its camera frame and size; the pixel-centre ray of k_pixel_ray.h); `a`, the guide planes of the
// current view and `out` hold S.width * S.height records; `out` aliases none of the inputs
void launch_reproject_resolve(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist, const ReprojectRule& R,
                              float4* out);
// ... with THE DELTA TABLE M describes (device memory, M.n_objects records): k_reproject_resolve_motion, the same pixel-to-lane mapping.  The callers launch it only
// while a record is flagged (M.capped); without one, launch_reproject_resolve gives the same image with the plain kernel's time.
void launch_reproject_resolve_motion(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist,
                                     const ReprojectRule& R, const ReprojectMotion& M, float4* out);
// THE STAGED FORM (CRH_REPROJECT_STAGED=1, at most kReprojectStagedMax flag-1 records): the n_staged flag-1 records, which the caller keeps in slot order BEHIND the
// table's M.n_objects records, are copied into LDS by every workgroup; the lanes then read flag and slot from memory and D from LDS.  The same bytes.
void launch_reproject_resolve_motion_staged(hipStream_t stream, const DScene& S, const float4* guide, const int2* ids, const float4* a, const ReprojectHistory& hist,
                                            const ReprojectRule& R, const ReprojectMotion& M, uint32_t n_staged, float4* out);
// the host twin: the same rule in a plain loop over host planes; rays: 8 floats per pixel {o.xyz, -, d.xyz, -}; hist_rgba == nullptr: no history
void reproject_host(const float4* a, const float* rays, const int32_t* object, const int32_t* triangle, const float* t, const float4* hist_rgba, const int32_t* hist_object,
                    const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame& F, const OutlineTri* table, uint32_t n_tri, uint32_t W, uint32_t H,
                    const ReprojectRule& R, float4* out);
// ... with the table (host memory; M.table == nullptr: reproject_host)
void reproject_motion_host(const float4* a, const float* rays, const int32_t* object, const int32_t* triangle, const float* t, const float4* hist_rgba, const int32_t* hist_object,
                           const int32_t* hist_triangle, const float* hist_t, const crh_reproject_frame& F, const OutlineTri* table, uint32_t n_tri, uint32_t W, uint32_t H,
                           const ReprojectRule& R, const ReprojectMotion& M, float4* out);

constexpr uint32_t kReprojectStagedMax = 64;
constexpr int kReprojectBlock = 256;      // four wavefronts, each 64 consecutive pixels of one row

}  // namespace crh
