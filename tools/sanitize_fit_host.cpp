// sanitize_fit_host.cpp -- the host-only side of view fitting (crh_fit_extents_host, crh_fit_from_extents; cadrays_amd/csrc/crh_fit.cpp, fit_kernels.hip) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no context, nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-fit      (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; }

int main()
{
  int failures = 0;
  crh_camera cam; std::memset(&cam, 0, sizeof cam);
  cam.eye[0] = 0.31f; cam.eye[1] = -2.9f; cam.eye[2] = 0.73f; cam.dir[0] = 0.21f; cam.dir[1] = 1.0f; cam.dir[2] = -0.16f; cam.up[0] = 0.05f; cam.up[2] = 1.0f;
  cam.fovy_deg = 37.0f; cam.ortho_scale = 1.0f; cam.focal_dist = 1.0f;
  for (int ortho = 0; ortho < 2; ++ortho)
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 1000u, 100003u}) {
      const uint32_t nO = 5;
      cam.is_ortho = ortho;
      std::vector<float> v(4 * (size_t)n), xf(12 * nO, 0.f), ext(6 * nO); std::vector<uint32_t> cnt(nO);
      for (uint32_t i = 0; i < n; ++i) {
        v[4 * i] = rnd(); v[4 * i + 1] = rnd(); v[4 * i + 2] = rnd();
        const int32_t ob = (int32_t)(i % 7u) - 1;            // -1 (skipped), 0 .. 4, 5 (out of range: skipped)
        std::memcpy(&v[4 * i + 3], &ob, 4);
      }
      for (uint32_t o = 0; o < nO; ++o) { xf[12 * o] = xf[12 * o + 5] = xf[12 * o + 10] = 1.0f + 0.1f * (float)o; xf[12 * o + 3] = 0.2f * (float)o; }
      crh_fit_result fr;
      for (const float* m : {(const float*)nullptr, (const float*)xf.data()}) {
        int rc = crh_fit_extents_host(n ? v.data() : nullptr, n, m, nO, &cam, 96, 64, 0.05f, ext.data(), cnt.data(), &fr);
        if (rc != CRH_OK) { std::printf("extents n=%u -> %d\n", n, rc); ++failures; continue; }
        float e[6] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY}; uint32_t total = 0;
        for (uint32_t o = 0; o < nO; ++o) { total += cnt[o]; for (int j = 0; j < 6; ++j) if (cnt[o] && ext[6 * o + j] > e[j]) e[j] = ext[6 * o + j]; }
        crh_camera out; crh_fit_result res;
        rc = crh_fit_from_extents(e, &cam, 96, 64, 0.05f, &out, &res);
        const bool expect_ok = total >= 2;
        if ((rc == CRH_OK) != expect_ok) { std::printf("rule n=%u total=%u -> %d\n", n, total, rc); ++failures; }
        if (rc == CRH_OK && !(res.z_near > 0.f && res.z_far >= res.z_near)) { std::printf("depth range n=%u\n", n); ++failures; }
        rc = crh_fit_from_extents(e, &cam, 96, 64, 0.05f, &out, nullptr);      // the result is optional
      }
    }
  // refusals walk their own paths
  {
    float e[6] = {1, 1, 1, 1, -4, 6}; crh_camera out;
    failures += crh_fit_from_extents(e, &cam, 96, 64, -0.5f, &out, nullptr) != CRH_E_INVALID;
    failures += crh_fit_from_extents(e, &cam, 96, 64, NAN, &out, nullptr) != CRH_E_INVALID;
    failures += crh_fit_from_extents(nullptr, &cam, 96, 64, 0.1f, &out, nullptr) != CRH_E_INVALID;
    e[3] = INFINITY;
    failures += crh_fit_from_extents(e, &cam, 96, 64, 0.1f, &out, nullptr) != CRH_E_INVALID;
    failures += crh_fit_extents_host(nullptr, 0, nullptr, 0, &cam, 96, 64, 0.1f, e, nullptr, nullptr) != CRH_E_INVALID;
  }
  std::printf("sanitize_fit_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
