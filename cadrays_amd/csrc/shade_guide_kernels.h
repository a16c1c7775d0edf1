// shade_guide_kernels.h -- the shade guide of the denoised display (crh_shade_guide.cpp, shade_guide_kernels.hip): per pixel the reciprocal of the first hit's albedo
// and a flag "a positional light shows here", derived from the first-hit id buffer, and the GUIDED form of the a-trous pass that reads it: the filter works on the
// image divided by the albedo (a diffuse texture survives it) and leaves the disc of a light alone.  The plane rule, the light test, the texture lookup -- ONE copy
// each, compiled for the gfx950 kernels and for the host twins -- the per-triangle record and the launch wrappers.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (the reference has no counterpart: OCCT's path tracer shows the raw accumulation)
//
// SECOND COPIES: shade_guide_texel restates sample_texture and shade_guide_seen the positional branch of intersect_light (k_lights_env.h, part of kernels.hip, which
// this feature does not touch), operation for operation, over plain pointers instead of the kernels' DScene; tests/test_shade_guide.py pins both to the renderer.
#pragma once
#include "denoise_kernels.h"
#include "device_types.h"

namespace crh {

// per CALLER'S triangle index (what the id buffer reports; the kernels' shading and uv records are in leaf order): the three vertices' uv, the material, whether the
// geometry has texture coordinates at all
struct GuideTri { float u0, v0, u1, v1, u2, v2; int32_t material; uint32_t has_uv; };      // 32 B

// crh_shade_guide_params as the kernels take it
struct ShadeGuideRule { uint32_t demodulate, lights; float albedo_floor; uint32_t light_dilate; };

// what the plane rule reads of the scene: the material table (8 x float4 per crh_bsdf), every texture slot's texels back to back, per slot {first texel, width,
// height, 0} (width 0: an empty slot), the lights as the kernels keep them ({position, is_point}, {emission, radius} for a positional one), crh_spec.h #2
struct ShadeGuideScene {
  const float4* mats; uint32_t n_mats; const float4* texels; const uint4* tex_desc; uint32_t n_tex; const float4* lights; uint32_t n_lights; int gamma2;
};

CRH_HD float shade_guide_lerp(float a, float b, float t) { return CRH_FMA(t, b - a, a); }

// the texel of a BOUND slot (td.y != 0) at the barycentrics (bu, bv), w0 = (1 - bu) - bv, of a triangle with the record r: sample_texture's arithmetic
CRH_HD float4 shade_guide_texel(const float4* texels, const uint4 td, const GuideTri& r, float bu, float bv, float w0, float sc_s, float sc_t, int gamma2)
{
  const float ss = sc_s != 0.f ? sc_s : 1.0f, st_ = sc_t != 0.f ? sc_t : 1.0f;
  float us = CRH_FMA(r.u2, bv, CRH_FMA(r.u1, bu, r.u0 * w0)) * ss;
  float vs = CRH_FMA(r.v2, bv, CRH_FMA(r.v1, bu, r.v0 * w0)) * st_;
  if (!(crh_abs(us) < 4194304.0f)) us = 0.f;
  if (!(crh_abs(vs) < 4194304.0f)) vs = 0.f;
  float uf = (float)(int)us; if (uf > us) uf -= 1.0f;
  float vf = (float)(int)vs; if (vf > vs) vf -= 1.0f;
  const float x = CRH_FMA(us - uf, (float)td.y, -0.5f), y = CRH_FMA(1.0f - (vs - vf), (float)td.z, -0.5f);
  float xf = (float)(int)x; if (xf > x) xf -= 1.0f;
  float yf = (float)(int)y; if (yf > y) yf -= 1.0f;
  const float fx = x - xf, fy = y - yf;
  const int W = (int)td.y, H = (int)td.z;
  int x0 = (int)xf; if (x0 < 0) x0 += W; if (x0 >= W) x0 -= W;
  int x1 = x0 + 1; if (x1 >= W) x1 = 0;
  int y0 = (int)yf; if (y0 < 0) y0 += H; if (y0 >= H) y0 -= H;
  int y1 = y0 + 1; if (y1 >= H) y1 = 0;
  const float4* tb = texels + td.x;
  const float4 p00 = tb[y0 * W + x0], p10 = tb[y0 * W + x1], p01 = tb[y1 * W + x0], p11 = tb[y1 * W + x1];
  float4 t = make_float4(shade_guide_lerp(shade_guide_lerp(p00.x, p10.x, fx), shade_guide_lerp(p01.x, p11.x, fx), fy),
                         shade_guide_lerp(shade_guide_lerp(p00.y, p10.y, fx), shade_guide_lerp(p01.y, p11.y, fx), fy),
                         shade_guide_lerp(shade_guide_lerp(p00.z, p10.z, fx), shade_guide_lerp(p01.z, p11.z, fx), fy),
                         shade_guide_lerp(shade_guide_lerp(p00.w, p10.w, fx), shade_guide_lerp(p01.w, p11.w, fx), fy));
  if (gamma2) { t.x *= t.x; t.y *= t.y; t.z *= t.z; }
  return t;
}

// THE ALBEDO RULE: (w.r, w.g, w.b, 0) for a pixel whose first hit is a triangle with the record r, at the barycentrics (bu, bv): w = 1 / max(albedo, floor), the
// albedo the sum of the four lobe weights with the texture applied to Kd and Kt as k_shade applies it
CRH_HD float4 shade_guide_weight(const ShadeGuideScene& S, const GuideTri& r, float bu, float bv, float albedo_floor)
{
  if (!S.n_mats) return make_float4(1.f, 1.f, 1.f, 0.f);
  int mat = r.material; if (mat < 0 || (uint32_t)mat >= S.n_mats) mat = 0;
  const float4* mp = S.mats + 8 * mat;
  const float4 m0 = mp[0], m1 = mp[1], m2 = mp[2], m3 = mp[3], m4 = mp[4];
  float kd[3] = {m1.x, m1.y, m1.z}, kt[3] = {m3.x, m3.y, m3.z};
  const float ks[3] = {m2.x, m2.y, m2.z}, kc[3] = {m0.x, m0.y, m0.z};
  const int slot = (int)m1.w - 1;
  if (slot >= 0 && (uint32_t)slot < S.n_tex && r.has_uv) {
    const uint4 td = S.tex_desc[slot];
    if (td.y != 0u) {
      const float w0 = (1.0f - bu) - bv;
      const float4 tx = shade_guide_texel(S.texels, td, r, bu, bv, w0, m3.w, m4.w, S.gamma2);
      kd[0] = kd[0] * tx.x; kd[1] = kd[1] * tx.y; kd[2] = kd[2] * tx.z;
      if (tx.w != 1.0f) {
        const float ia = 1.0f - tx.w;
        for (int k = 0; k < 3; ++k) { kd[k] = kd[k] * tx.w; kt[k] = CRH_FMA(tx.w, kt[k], ia); }
      }
    }
  }
  float w[3];
  for (int k = 0; k < 3; ++k) {
    float m = ((kd[k] + ks[k]) + kc[k]) + kt[k];
    if (!denoise_finite(m)) m = 1.0f;
    if (!(m >= albedo_floor)) m = albedo_floor;
    w[k] = 1.0f / m;
  }
  return make_float4(w[0], w[1], w[2], 0.f);
}

// THE LIGHT TEST: does the ray (o, d), whose first hit lies at hd (CRH_MAXFLOAT: none), show a positional light?  intersect_light's positional branch.
CRH_HD bool shade_guide_seen(const float4* lights, uint32_t n_lights, crh_v3 o, crh_v3 d, float hd)
{
  for (uint32_t i = 0; i < n_lights; ++i) {
    const float4 l0 = lights[2u * i], l1 = lights[2u * i + 1u];
    if (l0.w == 0.f) continue;
    const crh_v3 tl = crh_sub3(crh_mk3(l0.x, l0.y, l0.z), o);
    const float dist = crh_len3(tl);
    if (dist < hd) {
      const float q = l1.w / dist;
      const float cm = 1.0f / crh_sqrt(CRH_FMA(q, q, 1.0f));
      if (cm < 1.0f && crh_dot3(d, tl) * (1.0f / dist) >= cm) return true;
    }
  }
  return false;
}

// ... and its dilation: some pixel of the frame within the Chebyshev distance `dilate` of (x, y) is seen (seen == nullptr: none is)
CRH_HD bool shade_guide_dilated(const uint8_t* seen, uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t dilate)
{
  if (!seen) return false;
  const int32_t r = (int32_t)dilate;
  for (int32_t dy = -r; dy <= r; ++dy) {
    const int32_t qy = (int32_t)y + dy;
    if (qy < 0 || qy >= (int32_t)H) continue;
    for (int32_t dx = -r; dx <= r; ++dx) {
      const int32_t qx = (int32_t)x + dx;
      if (qx < 0 || qx >= (int32_t)W) continue;
      if (seen[(size_t)qy * W + (uint32_t)qx]) return true;
    }
  }
  return false;
}

// THE PLANE RULE for pixel (x, y), whose id buffer record is {-, bu, bv, tri}: {w.r, w.g, w.b, L}
CRH_HD float4 shade_guide_pixel(const ShadeGuideScene& S, const GuideTri* table, uint32_t n_tri, int32_t tri, float bu, float bv, const uint8_t* seen, uint32_t x,
                                uint32_t y, uint32_t W, uint32_t H, const ShadeGuideRule& R)
{
  float4 g = make_float4(1.f, 1.f, 1.f, 0.f);
  if (R.demodulate && tri >= 0 && (uint32_t)tri < n_tri) g = shade_guide_weight(S, table[tri], bu, bv, R.albedo_floor);
  g.w = (R.lights && shade_guide_dilated(seen, x, y, W, H, R.light_dilate)) ? 1.0f : 0.0f;
  return g;
}

// the guided pass reads the plane beside what the unguided one reads
struct DenoisePlanesGuidedDevice : DenoisePlanesDevice {
  const float4* __restrict__ sg;
  __host__ __device__ __forceinline__ float4 shade(uint32_t x, uint32_t y) const { return sg[(size_t)y * W + x]; }
};
struct DenoisePlanesGuidedHost : DenoisePlanesHost {
  const float4* sg;
  __host__ __device__ __forceinline__ float4 shade(uint32_t x, uint32_t y) const { return sg[(size_t)y * W + x]; }
};

// seen: W * H bytes, 1 where the pixel-centre ray of S's camera shows a positional light of S in front of the id buffer's hit
void launch_shade_guide_seen(hipStream_t stream, const DScene& S, const float4* hit, uint8_t* seen);
// plane: W * H records, written for every pixel.  hit: the id buffer's plane; table: n_tri records on the device (not read when n_tri == 0); seen: nullptr = no
// pixel shows a light (no positional light, or lights == 0)
void launch_shade_guide_plane(hipStream_t stream, const ShadeGuideScene& S, const float4* hit, uint32_t W, uint32_t H, const GuideTri* table, uint32_t n_tri,
                              const uint8_t* seen, const ShadeGuideRule& R, float4* plane);
// one guided pass: out[p] = denoise_pixel_guided(in, p, k) for every pixel, the plain gather form (every level)
void launch_denoise_pass_guided(hipStream_t stream, const float4* guide, const int2* ids, const float4* plane, const float4* in, float4* out, uint32_t W, uint32_t H,
                                uint32_t k, const DenoiseRule& R);
// the host twins: the same rules in plain loops.  rays: 8 floats per pixel {o.xyz, -, d.xyz, -}; uv: 2 per pixel; seen: W * H bytes of scratch
void shade_guide_host(const ShadeGuideScene& S, const float* rays, const int32_t* triangle, const float* t, const float* uv, uint32_t W, uint32_t H, const GuideTri* table,
                      uint32_t n_tri, const ShadeGuideRule& R, uint8_t* seen, float4* plane);
void denoise_guided_host(const int32_t* object, const int32_t* triangle, const float* t, uint32_t W, uint32_t H, const OutlineTri* table, uint32_t n_tri,
                         const float4* plane, const DenoiseRule& R, const float4* in, float4* tmp, float4* out);

}  // namespace crh
