/* brute_force.c -- independent geometric ground truth for the traversal tests.  TEST INFRASTRUCTURE ONLY (loaded by tests/).
 *
 * No BVH, no shared headers: every ray is tested against every triangle.
 *   bf_nearest_f64   Moeller-Trumbore in double precision (a different formula from the product's n = (v0-v2) x (v1-v0) form):
 *                    the geometric truth, compared with a tolerance.
 *   bf_nearest_f64d  the same over triangle corners given in double precision (world corners of placed objects: float vertices under a
 *                    float matrix, multiplied out in double by the test).
 *   bf_blockers_f64  per ray the nearest robust and the nearest possible blocker (double corners): the truth of an any-hit query.
 *   bf_nearest_f32   the product's triangle test (DESIGN.md section 3 "Triangle (a7)"), restated here in plain float with the
 *                    same operation order (dot = fma(z,z, fma(y,y, x*x)), cross component = fma(p,q, -(r*s))), over ALL triangles in input order, first of equal t wins the tie like a front-to-back
 *                    walk cannot promise -- so the caller compares t/u/v bit-for-bit and the triangle index modulo exact t ties.
 *                    BVH traversal == this on every ray means the quantised boxes never cull a triangle the ray hits.
 * rays: 8 floats each {o.xyz, tmax, d.xyz, -}; tri_pos: 9 floats per triangle (world space); out: {t, u, v, index (as float bits)}.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define BF_API __attribute__((visibility("default")))

/* Moeller-Trumbore for ray r over all triangles; the corners come as floats (tf) or as doubles (td), a float corner converts exactly */
static inline void bf_nearest_ray(const float* tf, const double* td, uint32_t nT, const float* rays, uint32_t r, double* out_tuv, int32_t* out_idx,
                                  double* out_margin)
{
  const double ox = rays[8 * r], oy = rays[8 * r + 1], oz = rays[8 * r + 2], tmax = rays[8 * r + 3];
  const double dx = rays[8 * r + 4], dy = rays[8 * r + 5], dz = rays[8 * r + 6];
  double best = tmax, bu = 0, bv = 0; int32_t bi = -1;
  for (uint32_t i = 0; i < nT; ++i) {
    double p[9];
    for (int k = 0; k < 9; ++k) p[k] = td ? td[9 * (size_t)i + k] : (double)tf[9 * (size_t)i + k];
    const double e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const double e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const double det = e1x * px + e1y * py + e1z * pz;
    if (det == 0.0) continue;
    const double inv = 1.0 / det;
    const double tx = ox - p[0], ty = oy - p[1], tz = oz - p[2];
    const double u = (tx * px + ty * py + tz * pz) * inv;
    if (u < 0.0 || u > 1.0) continue;
    const double qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
    const double v = (dx * qx + dy * qy + dz * qz) * inv;
    if (v < 0.0 || u + v > 1.0) continue;
    const double t = (e2x * qx + e2y * qy + e2z * qz) * inv;
    if (t >= 0.0 && t < best) { best = t; bu = u; bv = v; bi = (int32_t)i; }
  }
  out_tuv[3 * (size_t)r] = best; out_tuv[3 * (size_t)r + 1] = bu; out_tuv[3 * (size_t)r + 2] = bv; out_idx[r] = bi;
  if (out_margin) {              /* distance of the hit from the triangle's edges in barycentric units (0 = on an edge) */
    double m = bu < bv ? bu : bv; const double w = 1.0 - bu - bv; if (w < m) m = w;
    out_margin[r] = bi >= 0 ? m : 1.0;
  }
}

BF_API void bf_nearest_f64(const float* tri_pos, uint32_t nT, const float* rays, uint32_t nR, double* out_tuv, int32_t* out_idx,
                           double* out_margin)
{
#pragma omp parallel for schedule(dynamic, 64)
  for (uint32_t r = 0; r < nR; ++r) bf_nearest_ray(tri_pos, NULL, nT, rays, r, out_tuv, out_idx, out_margin);
}

BF_API void bf_nearest_f64d(const double* tri_pos, uint32_t nT, const float* rays, uint32_t nR, double* out_tuv, int32_t* out_idx,
                            double* out_margin)
{
#pragma omp parallel for schedule(dynamic, 64)
  for (uint32_t r = 0; r < nR; ++r) bf_nearest_ray(NULL, tri_pos, nT, rays, r, out_tuv, out_idx, out_margin);
}

/* Any-hit truth.  For every triangle whose plane the ray crosses at t >= 0: how far inside (+) / outside (-) the triangle does it cross, as a
 * distance d (minimum over the three edges of the in-plane distance to the edge), and the band b around an edge inside which a float walk
 * and double precision may disagree:  b = (2e-5 size + 2e-6 scene + 1e-6 |t|) / max(cos of incidence, 1e-5),  size = longest edge.
 * A ROBUST blocker has d > b, a POSSIBLE blocker d > -b.  out[2 r] = nearest t of a robust one, out[2 r + 1] of a possible one (INFINITY: none). */
BF_API void bf_blockers_f64(const double* tri_pos, uint32_t nT, const float* rays, uint32_t nR, double scene, double* out)
{
#pragma omp parallel for schedule(dynamic, 64)
  for (uint32_t r = 0; r < nR; ++r) {
    const double o[3] = {rays[8 * r], rays[8 * r + 1], rays[8 * r + 2]}, d[3] = {rays[8 * r + 4], rays[8 * r + 5], rays[8 * r + 6]};
    double t_rob = INFINITY, t_pos = INFINITY;
    for (uint32_t i = 0; i < nT; ++i) {
      const double* p = &tri_pos[9 * (size_t)i];
      const double ax = p[3] - p[0], ay = p[4] - p[1], az = p[5] - p[2], bx = p[6] - p[0], by = p[7] - p[1], bz = p[8] - p[2];
      double n[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
      const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      if (!(nl > 0.0)) continue;
      n[0] /= nl; n[1] /= nl; n[2] /= nl;
      const double dn = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
      if (dn == 0.0) continue;
      const double t = ((p[0] - o[0]) * n[0] + (p[1] - o[1]) * n[1] + (p[2] - o[2]) * n[2]) / dn;
      if (!(t >= 0.0) || t >= t_rob) continue;                         /* t_rob >= t_pos always: a robust blocker is a possible one */
      const double P[3] = {o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t};
      double dist = INFINITY, size = 0.0;
      for (int e = 0; e < 3; ++e) {
        const double* a = &p[3 * e]; const double* b = &p[3 * ((e + 1) % 3)];
        const double ex = b[0] - a[0], ey = b[1] - a[1], ez = b[2] - a[2];
        double m[3] = {n[1] * ez - n[2] * ey, n[2] * ex - n[0] * ez, n[0] * ey - n[1] * ex};      /* n x edge: in the plane, pointing inside */
        const double ml = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), el = sqrt(ex * ex + ey * ey + ez * ez);
        if (el > size) size = el;
        const double q = ((P[0] - a[0]) * m[0] + (P[1] - a[1]) * m[1] + (P[2] - a[2]) * m[2]) / (ml > 1e-300 ? ml : 1e-300);
        if (q < dist) dist = q;
      }
      const double cosi = fabs(dn);
      const double band = (2e-5 * size + 2e-6 * scene + 1e-6 * fabs(t)) / (cosi > 1e-5 ? cosi : 1e-5);
      if (dist > -band && t < t_pos) t_pos = t;
      if (dist > band) t_rob = t;
    }
    out[2 * (size_t)r] = t_rob; out[2 * (size_t)r + 1] = t_pos;
  }
}

/* the product's float formula, operation by operation; built with -ffp-contract=off */
BF_API void bf_nearest_f32(const float* tri_pos, uint32_t nT, const float* rays, uint32_t nR, float* out)
{
#pragma omp parallel for schedule(dynamic, 64)
  for (uint32_t r = 0; r < nR; ++r) {
    const float ox = rays[8 * r], oy = rays[8 * r + 1], oz = rays[8 * r + 2];
    const float dx = rays[8 * r + 4], dy = rays[8 * r + 5], dz = rays[8 * r + 6];
    float best = rays[8 * r + 3], bu = 0.f, bv = 0.f; int32_t bi = -1;
    for (uint32_t i = 0; i < nT; ++i) {
      const float* p = &tri_pos[9 * (size_t)i];
      const float e0x = p[3] - p[0], e0y = p[4] - p[1], e0z = p[5] - p[2];          /* v1 - v0 */
      const float e1x = p[0] - p[6], e1y = p[1] - p[7], e1z = p[2] - p[8];          /* v0 - v2 */
      const float nx = fmaf(e1y, e0z, -(e1z * e0y)), ny = fmaf(e1z, e0x, -(e1x * e0z)), nz = fmaf(e1x, e0y, -(e1y * e0x));     /* e1 x e0 */
      const float tox = p[0] - ox, toy = p[1] - oy, toz = p[2] - oz;
      const float inv = 1.0f / fmaf(nz, dz, fmaf(ny, dy, nx * dx));
      const float cx = fmaf(dy, toz, -(dz * toy)), cy = fmaf(dz, tox, -(dx * toz)), cz = fmaf(dx, toy, -(dy * tox));           /* d x to */
      const float t = fmaf(nz, toz, fmaf(ny, toy, nx * tox)) * inv;
      const float u = fmaf(cz, e1z, fmaf(cy, e1y, cx * e1x)) * inv;
      const float v = fmaf(cz, e0z, fmaf(cy, e0y, cx * e0x)) * inv;
      if (t >= 0.f && u >= 0.f && v >= 0.f && (u + v) <= 1.0f && t < best) { best = t; bu = u; bv = v; bi = (int32_t)i; }
    }
    float* o = &out[4 * (size_t)r];
    o[0] = best; o[1] = bu; o[2] = bv; memcpy(&o[3], &bi, 4);
  }
}
