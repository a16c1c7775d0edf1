// fit_kernels.h -- view fitting (crh_fit.cpp, fit_kernels.hip): the types and the PER-VERTEX function the gfx950 kernel and its host twin share, and the launch wrapper.
// A translation unit of its own, apart from kernels.hip: the timed kernels' object code does not change when this does.
//
// ARITHMETIC: plain float32 multiplies, adds and subtractions in the order written, one rounding each -- NO CRH_FMA ANYWHERE in this file or in fit_kernels.hip
// (-ffp-contract=off keeps the compiler from fusing on either side), so that a numpy float32 restatement gives the same bits (tests/fit_reference.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crh_math.h"

namespace crh {

struct FitFrame { float pivot[3], right[3], up[3], fwd[3], kx, ky; };      // pivot = the eye of the input camera; the frame of fill_scene; the slopes (0 / 0: orthographic)
struct FitObject { float m[12]; uint32_t on, pad[3]; };                    // per call: the object's CURRENT 3x4 transform, 1 = its extents are wanted
constexpr uint32_t kFitRec = 8;                                            // dwords per object record: six keys, the count of contributing vertices, one unused

// Order-preserving integer key of a float: all bits flipped for negatives, the sign bit flipped otherwise.  -0.0 sorts below +0.0, which a float maximum does not
// decide; key 0 belongs to no finite float and stands for "no vertex" in a zeroed record.
CRH_HD uint32_t fit_key(float f) { const uint32_t u = crh_f2u(f); return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
CRH_HD float fit_unkey(uint32_t k) { return crh_u2f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// The six values of one vertex v of an object with rows m: p = m v (world), q = p - pivot, (x, y, z) = q in the camera frame, then
// x - z kx, -x - z kx, y - z ky, -y - z ky, -z, z.  Every product is rounded, then every sum / difference.  No CRH_FMA.
CRH_HD void fit_vertex(const float* m, float v0, float v1, float v2, const FitFrame& F, float e[6])
{
  const float p0 = ((m[0] * v0 + m[1] * v1) + m[2] * v2) + m[3];
  const float p1 = ((m[4] * v0 + m[5] * v1) + m[6] * v2) + m[7];
  const float p2 = ((m[8] * v0 + m[9] * v1) + m[10] * v2) + m[11];
  const float q0 = p0 - F.pivot[0], q1 = p1 - F.pivot[1], q2 = p2 - F.pivot[2];
  const float x = (q0 * F.right[0] + q1 * F.right[1]) + q2 * F.right[2];
  const float y = (q0 * F.up[0] + q1 * F.up[1]) + q2 * F.up[2];
  const float z = (q0 * F.fwd[0] + q1 * F.fwd[1]) + q2 * F.fwd[2];
  const float zx = z * F.kx, zy = z * F.ky;
  e[0] = x - zx; e[1] = -x - zx; e[2] = y - zy; e[3] = -y - zy; e[4] = -z; e[5] = z;
}

// rec: kFitRec * n_objects dwords, ZERO at launch; verts: {x, y, z, object index as int bits}, an index outside [0, n_objects) (-1: no triangle references the
// vertex) or an object whose `on` is 0 is skipped.  `grid` workgroups at most.
void launch_fit_extents(hipStream_t stream, int grid, const float4* verts, uint32_t n, const FitObject* objs, uint32_t n_objects, const FitFrame& F, uint32_t* rec);
// the host twin: the same per-vertex function in a plain loop over host arrays (rec zeroed by the caller)
void fit_extents_host(const float* verts4, uint32_t n, const FitObject* objs, uint32_t n_objects, const FitFrame& F, uint32_t* rec);

}  // namespace crh
