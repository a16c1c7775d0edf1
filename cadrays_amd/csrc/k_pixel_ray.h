// k_pixel_ray.h -- the pixel-centre camera ray: ONE copy, included by k_ids.h (part of kernels.hip, inside namespace crh::(anonymous)) and by reproject_kernels.hip
// (inside namespace crh).  No include guard and no includes of its own: whoever includes it has device_types.h (DScene, crh_math.h) in scope, once per translation unit.

// The camera ray camera_ray() (k_raygen.h) produces with jitter (0.5, 0.5) and no lens sample, restated: camera_ray() seeds and advances the RNG on its way, and the
// rendered images must not depend on how the compiler schedules a shared helper.  Same operations in the same order for the three camera models.
__host__ __device__ __forceinline__ void pixel_centre_ray(const DScene& S, const uint32_t px, const uint32_t py, crh_v3& o, crh_v3& d)
{
  const float jx = 0.5f, jy = 0.5f;
  const float nx = CRH_FMA(((float)px + jx) / (float)S.width, 2.0f, -1.0f);
  const float ny = CRH_FMA(((float)py + jy) / (float)S.height, -2.0f, 1.0f);
  if (S.is_ortho) {
    const float sx = (nx * S.ortho_scale) * S.aspect, sy = ny * S.ortho_scale;
    o = crh_madd3(crh_madd3(S.eye, S.right, sx), S.up, sy);
    d = S.fwd;
  } else if (S.spec_raygen) {
    const float u = ((float)px + jx) / (float)S.width, v = 1.0f - ((float)py + jy) / (float)S.height;
    o = S.eye;
    d = crh_norm3(crh_lerp3(crh_lerp3(S.corner[0], S.corner[1], u), crh_lerp3(S.corner[2], S.corner[3], u), v));
  } else {
    const float sx = (nx * S.tan_half) * S.aspect, sy = ny * S.tan_half;
    o = S.eye;
    d = crh_norm3(crh_madd3(crh_madd3(S.fwd, S.right, sx), S.up, sy));
  }
}
