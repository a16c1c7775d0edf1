// annotate_kernels.h -- world-space line annotations over the display (crh_annotate.cpp, annotate_kernels.hip): the projection of a segment into its screen record,
// the pixel rule and the bin rule -- ONE copy each, compiled for the gfx950 kernels and for the host twins -- and the launch wrappers.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
// (no counterpart in the reference: the application paints its manipulator and its light markers with ImGui over the finished image, with no notion of what the scene
// hides -- src/ImGui/ImRaytraceControls.cxx:64, :93-111)
//
// ARITHMETIC: the projection in float64 from the widened floats, the pixel rule in float32; sums, differences, products, quotients, compares and min / max only, every
// one rounded on its own -- no transcendental, no fused multiply-add (the library is built with -ffp-contract=off) -- in the order written below.  Every pixel GATHERS
// the segments of its tile in ascending index; the bins only leave out segments that cannot cover a pixel of the tile, so no result depends on them.  So the device,
// the host twins and a numpy restatement agree bit for bit (tests/annotate_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cadrays_hip.h"
#include "../../include/crh_math.h"

namespace crh {

constexpr uint32_t kAnnotOnTop = 0u, kAnnotHide = 1u, kAnnotXray = 2u;      // CRH_ANNOT_* of include/cadrays_hip.h
constexpr uint32_t kAnnotMaxSegments = 65536u, kAnnotMaxWidth = 8u;
constexpr uint32_t kAnnotGatherMax = 256u;                                  // lists up to this length are binned by the gather form, longer ones by the scatter form (measured)
constexpr uint32_t kAnnotStyleBits = 0x30Fu;                                // width in bits 0-3, mode in bits 8-9
constexpr float kAnnotMiss = 1.0e15f;                                       // t of a pixel whose ray met nothing (the id buffer)

// The screen record of one segment (32 B, two 16-byte loads): the end points in continuous pixel coordinates (a pixel centre at px + 0.5, row 0 the top), the depth
// coordinate q at each -- 1 / z for a perspective camera, z for an orthographic one: linear along the SCREEN segment -- and flags bit 0: the record is valid.
struct alignas(16) AnnotRecord { float x0, y0, x1, y1, q0, q1; uint32_t flags, pad; };

// The camera as the projection reads it: camera_frame()'s basis and half-angle, the eye, the frame size
struct AnnotCam { float eye[3], right[3], up[3], fwd[3]; float tan_half, aspect, ortho_scale; uint32_t is_ortho, W, H; };

CRH_HD uint32_t annot_width(uint32_t style) { return style & 15u; }
CRH_HD uint32_t annot_mode(uint32_t style) { return (style >> 8) & 3u; }

CRH_HD double annot_dot(double x, double y, double z, const float* b) { return (x * (double)b[0] + y * (double)b[1]) + z * (double)b[2]; }
CRH_HD bool annot_finite(float v) { return v - v == 0.0f; }
CRH_HD bool annot_finite(double v) { return v - v == 0.0; }
CRH_HD double annot_clamp(double v, double lo, double hi) { v = v > lo ? v : lo; return v < hi ? v : hi; }

// One edge of Liang-Barsky: the part of [t0, t1] with p t <= q; false: none
CRH_HD bool annot_clip_edge(double p, double q, double& t0, double& t1)
{
  if (p == 0.0) return q >= 0.0;
  const double r = q / p;
  if (p < 0.0) { if (r > t1) return false; if (r > t0) t0 = r; }
  else         { if (r < t0) return false; if (r < t1) t1 = r; }
  return true;
}

// THE PROJECTION of one segment, in double from the widened floats, in this order:
//   1  v = P - eye per component;  xr = (v.x r.x + v.y r.y) + v.z r.z with r = right, yu likewise with up, z with fwd -- for both end points a, b
//   2  near clip: zmax = max(za, zb); !(zmax > 0): invalid.  zmin = zmax * 2^-16 (perspective) or 0 (orthographic).  An end point with z < zmin moves along the
//      segment to z = zmin:  u = (zmin - z) / (z_other - z);  xr += u (xr_other - xr), yu += u (yu_other - yu), z = zmin  (the other end point is the one with zmax)
//   3  kx = tan_half * aspect, ky = tan_half;  perspective: dx = z kx, dy = z ky;  orthographic: dx = ortho_scale * aspect, dy = ortho_scale
//      X = (xr / dx + 1) (W / 2),  Y = (1 - yu / dy) (H / 2);   q = 1 / z (perspective) or z (orthographic)
//   4  Liang-Barsky against the guard band [-W, 2W] x [-H, 2H], edges in the order left, right, top, bottom, over (t0, t1) = (0, 1) with D = B - A:
//      a' = A + t0 D where t0 > 0, b' = A + t1 D where t1 < 1 (else the point itself), q likewise with the same parameter; nothing left: invalid.
//      one of the six not finite: invalid.  x then min(max(x, -W), 2W), y min(max(y, -H), 2H): the sum can leave the band by its rounding (far by cancellation,
//      for end points 1e30 pixels away)
//   5  each of the six rounded to float32; any of them not finite: invalid; else flags = 1.  An invalid record is all zero.
CRH_HD AnnotRecord annot_project(const AnnotCam& C, const float* a, const float* b)
{
  const AnnotRecord none{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u, 0u};
  const double ax = (double)a[0] - (double)C.eye[0], ay = (double)a[1] - (double)C.eye[1], az = (double)a[2] - (double)C.eye[2];
  const double bx = (double)b[0] - (double)C.eye[0], by = (double)b[1] - (double)C.eye[1], bz = (double)b[2] - (double)C.eye[2];
  double xa = annot_dot(ax, ay, az, C.right), ya = annot_dot(ax, ay, az, C.up), za = annot_dot(ax, ay, az, C.fwd);
  double xb = annot_dot(bx, by, bz, C.right), yb = annot_dot(bx, by, bz, C.up), zb = annot_dot(bx, by, bz, C.fwd);
  const double zmax = za > zb ? za : zb;
  if (!(zmax > 0.0)) return none;
  const double zmin = C.is_ortho ? 0.0 : zmax * (1.0 / 65536.0);
  if (za < zmin) { const double u = (zmin - za) / (zb - za); xa = xa + u * (xb - xa); ya = ya + u * (yb - ya); za = zmin; }
  else if (zb < zmin) { const double u = (zmin - zb) / (za - zb); xb = xb + u * (xa - xb); yb = yb + u * (ya - yb); zb = zmin; }
  const double kx = (double)C.tan_half * (double)C.aspect, ky = (double)C.tan_half;
  const double hw = (double)C.W * 0.5, hh = (double)C.H * 0.5;
  double X0, Y0, X1, Y1, Q0, Q1;
  if (C.is_ortho) {
    const double dx = (double)C.ortho_scale * (double)C.aspect, dy = (double)C.ortho_scale;
    X0 = (xa / dx + 1.0) * hw; Y0 = (1.0 - ya / dy) * hh; X1 = (xb / dx + 1.0) * hw; Y1 = (1.0 - yb / dy) * hh;
    Q0 = za; Q1 = zb;
  } else {
    X0 = (xa / (za * kx) + 1.0) * hw; Y0 = (1.0 - ya / (za * ky)) * hh; X1 = (xb / (zb * kx) + 1.0) * hw; Y1 = (1.0 - yb / (zb * ky)) * hh;
    Q0 = 1.0 / za; Q1 = 1.0 / zb;
  }
  const double W = (double)C.W, H = (double)C.H, DX = X1 - X0, DY = Y1 - Y0, DQ = Q1 - Q0;
  double t0 = 0.0, t1 = 1.0;
  if (!annot_clip_edge(-DX, X0 + W, t0, t1)) return none;           // -W <= X
  if (!annot_clip_edge(DX, (W + W) - X0, t0, t1)) return none;      // X <= 2W
  if (!annot_clip_edge(-DY, Y0 + H, t0, t1)) return none;           // -H <= Y
  if (!annot_clip_edge(DY, (H + H) - Y0, t0, t1)) return none;      // Y <= 2H
  const double x1 = t1 < 1.0 ? X0 + t1 * DX : X1, y1 = t1 < 1.0 ? Y0 + t1 * DY : Y1, q1 = t1 < 1.0 ? Q0 + t1 * DQ : Q1;
  const double x0 = t0 > 0.0 ? X0 + t0 * DX : X0, y0 = t0 > 0.0 ? Y0 + t0 * DY : Y0, q0 = t0 > 0.0 ? Q0 + t0 * DQ : Q0;
  if (!(annot_finite(x0) && annot_finite(y0) && annot_finite(x1) && annot_finite(y1) && annot_finite(q0) && annot_finite(q1))) return none;
  const AnnotRecord R{(float)annot_clamp(x0, -W, W + W), (float)annot_clamp(y0, -H, H + H), (float)annot_clamp(x1, -W, W + W), (float)annot_clamp(y1, -H, H + H), (float)q0, (float)q1, 1u, 0u};
  if (!(annot_finite(R.x0) && annot_finite(R.y0) && annot_finite(R.x1) && annot_finite(R.y1) && annot_finite(R.q0) && annot_finite(R.q1))) return none;
  return R;
}

// THE PIXEL RULE, float32, for the pixel (x, y) and one valid record of a segment `width` pixels wide:   p = (x + 0.5, y + 0.5), a = (x0, y0), e = b - a,
//   l2 = e.x e.x + e.y e.y;   s = l2 > 0 ? min(max(((p.x - a.x) e.x + (p.y - a.y) e.y) / l2, 0), 1) : 0;   d = p - (a + s e);   h = width * 0.5
//   covered iff d.x d.x + d.y d.y <= h h            (*s_out = s either way)
CRH_HD bool annot_covers(const AnnotRecord& R, uint32_t width, uint32_t x, uint32_t y, float* s_out)
{
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float ex = R.x1 - R.x0, ey = R.y1 - R.y0;
  const float l2 = ex * ex + ey * ey;
  float s = 0.f;
  if (l2 > 0.f) {
    s = ((px - R.x0) * ex + (py - R.y0) * ey) / l2;
    s = s > 0.f ? s : 0.f;           // (a NaN becomes 0)
    s = s < 1.f ? s : 1.f;
  }
  const float dx = px - (R.x0 + s * ex), dy = py - (R.y0 + s * ey);
  const float h = (float)width * 0.5f;
  *s_out = s;
  return dx * dx + dy * dy <= h * h;
}

// ... and whether the scene hides the segment there (modes HIDE and XRAY):   zh = t (d . fwd), t the pixel's first-hit distance and d its pixel-centre ray's direction
// (d . fwd = (d.x f.x + d.y f.y) + d.z f.z; an orthographic ray runs along fwd: the factor is 1, zh = t);   qs = q0 + s (q1 - q0);   zb = zh (1 + depth_bias)
//   perspective: occluded iff qs zb < 1;   orthographic: occluded iff qs > zb;   a miss (t >= 1e15) never occludes
CRH_HD bool annot_occluded(const AnnotRecord& R, float s, float zh, float t, float depth_bias, uint32_t is_ortho)
{
  if (!(t < kAnnotMiss)) return false;
  const float qs = R.q0 + s * (R.q1 - R.q0);
  const float zb = zh * (1.0f + depth_bias);
  return is_ortho ? qs > zb : qs * zb < 1.0f;
}
CRH_HD float annot_hit_depth(float t, float dx, float dy, float dz, const float* fwd, uint32_t is_ortho) { return is_ortho ? t : t * ((dx * fwd[0] + dy * fwd[1]) + dz * fwd[2]); }

// The alpha a covered pixel is blended with: the segment's where it is visible or the mode is ON_TOP, (alpha hidden_alpha + 128) >> 8 for an occluded XRAY pixel;
// -1: an occluded HIDE pixel, which is skipped and does not enter the id plane
CRH_HD int32_t annot_alpha(uint32_t mode, bool occluded, uint32_t alpha, uint32_t hidden_alpha)
{
  if (mode == kAnnotOnTop || !occluded) return (int32_t)alpha;
  if (mode == kAnnotXray) return (int32_t)((alpha * hidden_alpha + 128u) >> 8);
  return -1;
}
// ... by the selection interior's formula
CRH_HD uint32_t annot_blend(uint32_t ldr, uint32_t colour, uint32_t A) { return (ldr * (256u - A) + colour * A + 128u) >> 8; }

// One pixel's state while the segments of its tile pass by in ascending index
struct AnnotPixel { uint32_t r, g, b; int32_t seg; float s; };
// One segment against one pixel: the pixel rule, then the composite.  zh / t: the pixel's scene depth (read only for modes HIDE and XRAY).
CRH_HD void annot_apply(AnnotPixel& P, const AnnotRecord& R, const crh_annot_segment& S, int32_t index, uint32_t x, uint32_t y, float zh, float t, float depth_bias,
                        uint32_t hidden_alpha, uint32_t is_ortho)
{
  if (!(R.flags & 1u)) return;
  float s;
  if (!annot_covers(R, annot_width(S.style), x, y, &s)) return;
  const uint32_t mode = annot_mode(S.style);
  const bool occluded = mode != kAnnotOnTop && annot_occluded(R, s, zh, t, depth_bias, is_ortho);
  const int32_t A = annot_alpha(mode, occluded, S.alpha, hidden_alpha);
  if (A < 0) return;
  P.r = annot_blend(P.r, S.rgb[0], (uint32_t)A); P.g = annot_blend(P.g, S.rgb[1], (uint32_t)A); P.b = annot_blend(P.b, S.rgb[2], (uint32_t)A);
  P.seg = index; P.s = s;
}

// THE BIN RULE: segment i's bit is set in a tile (edge E pixels, tile (tx, ty) covers the pixels [tx E, tx E + E) x [ty E, ty E + E)) iff its record is valid and
// its box, grown by half the width plus one pixel, meets the tile's square.  A superset of the tiles in which the pixel rule can cover a pixel.
struct AnnotBox { float lo_x, lo_y, hi_x, hi_y; };
CRH_HD AnnotBox annot_box(const AnnotRecord& R, uint32_t width)
{
  const float g = (float)width * 0.5f + 1.0f;
  return AnnotBox{(R.x0 < R.x1 ? R.x0 : R.x1) - g, (R.y0 < R.y1 ? R.y0 : R.y1) - g, (R.x0 < R.x1 ? R.x1 : R.x0) + g, (R.y0 < R.y1 ? R.y1 : R.y0) + g};
}
CRH_HD bool annot_box_meets(const AnnotBox& B, uint32_t tx, uint32_t ty, uint32_t E)
{
  const float x0 = (float)(tx * E), y0 = (float)(ty * E), x1 = (float)(tx * E + E), y1 = (float)(ty * E + E);
  return B.hi_x >= x0 && B.lo_x <= x1 && B.hi_y >= y0 && B.lo_y <= y1;
}

struct DScene;

// What the drawing needs besides the records: the list, the frame, the camera's fwd and model, the parameters, the id buffer's hit plane (NULL: no segment asks for depth)
struct AnnotDraw {
  const AnnotRecord* rec; const crh_annot_segment* seg; uint32_t n, n_words;
  const uint32_t* bins; uint32_t tile, tiles_x, tiles_y;      // n_words words per tile, row-major tiles of edge `tile` (8, 16 or 32)
  const float4* hit; float depth_bias; uint32_t hidden_alpha;
};

// records[i] = annot_project(cam, seg[i]) for i < n
void launch_annot_project(hipStream_t stream, const AnnotCam& cam, const crh_annot_segment* seg, uint32_t n, AnnotRecord* rec);
// bins: tiles_x * tiles_y * n_words words, every one written (gather form) or cleared and OR-ed into (scatter form: vector atomicOr)
void launch_annot_bin(hipStream_t stream, const AnnotDraw& D, bool scatter, uint32_t* bins);
// ldr: W * H * 3 bytes blended in place (a pixel reads and writes its own three bytes only);  or, ldr == NULL, the id plane and the parameter plane (W * H each), every
// pixel written.  S: the scene record of the view (its camera frame and size: the pixel-centre ray of k_pixel_ray.h).
void launch_annot_draw(hipStream_t stream, const DScene& S, const AnnotDraw& D, uint8_t* ldr, int32_t* seg_px, float* s_px);
// the host twins: the same functions in plain loops, no bins
void annot_project_host(const AnnotCam& cam, const crh_annot_segment* seg, uint32_t n, AnnotRecord* rec);
void annot_draw_host(const AnnotRecord* rec, const crh_annot_segment* seg, uint32_t n, float depth_bias, uint32_t hidden_alpha, const AnnotCam& cam, const float* rays_px,
                     const float* t_px, uint8_t* ldr, int32_t* seg_px);

}  // namespace crh
