// sanitize_denoise_host.cpp -- the host-only side of the denoised display (crh_denoise_host; cadrays_amd/csrc/crh_denoise.cpp, denoise_kernels.h: the similarity
// rule, the pixel rule, every pass) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no context, nothing loaded into an
// interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-denoise   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)(rnd() % 20001u) * 1e-4f - 1.0f; }

struct Rec { float n[3]; uint32_t degenerate; uint32_t v[3]; uint32_t pad; };

int main()
{
  int failures = 0;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // a table from random triangles, some degenerate; exactly-sized heap blocks, so one byte too many is seen
  const uint32_t nV = 96, nT = 50;
  std::vector<float> pos(3 * nV);
  for (float& p : pos) p = rndf();
  std::vector<uint32_t> tri(4 * nT);
  for (uint32_t t = 0; t < nT; ++t) { for (int k = 0; k < 3; ++k) tri[4 * t + k] = rnd() % nV; tri[4 * t + 3] = 0; }
  tri[8] = 7; tri[9] = 7; tri[10] = 7;                     // a point
  tri[12] = 9; tri[13] = 9; tri[14] = 12;                  // two equal vertices
  std::vector<Rec> table(nT);
  failures += crh_outline_table_host(pos.data(), nV, tri.data(), nT, table.data()) != CRH_OK;
  std::vector<unsigned char> raw(sizeof(Rec) * nT + 1);    // an unaligned table block is the caller's right
  std::memcpy(raw.data() + 1, table.data(), sizeof(Rec) * nT);

  // the edge shapes: one pixel, one row, one column, frames narrower than the window of step 16, more than one 64-pixel chunk per row
  const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 300}, {67, 45}, {130, 3}};
  crh_denoise_params def; crh_denoise_defaults(&def);
  for (const auto& wh : sizes) {
    const uint32_t W = wh[0], H = wh[1];
    const size_t n = (size_t)W * H;
    std::vector<int32_t> ob(n), tr(n); std::vector<float> t(n), rgba(4 * n);
    for (size_t i = 0; i < n; ++i) {
      tr[i] = (int32_t)(rnd() % (nT + 12u)) - 4;                     // -4 .. -1 (misses and nonsense), 0 .. nT - 1, nT .. nT + 7 (beyond the table)
      if (i && rnd() % 2u) tr[i] = tr[i - 1];                        // runs
      ob[i] = tr[i] < 0 ? -1 : (int32_t)((uint32_t)tr[i] % 3u);
      t[i] = tr[i] < 0 ? 1e15f : 1.0f + (float)(rnd() % 40u) * 0.5f;
      for (int k = 0; k < 3; ++k) rgba[4 * i + k] = (float)(rnd() % 1000u) * 1e-3f;
      rgba[4 * i + 3] = (float)(rnd() % 6u);                         // unsampled pixels among them
      const uint32_t odd = rnd() % 50u;
      if (odd == 0u) rgba[4 * i] = inf; else if (odd == 1u) rgba[4 * i + 1] = nan; else if (odd == 2u) rgba[4 * i + 2] = -inf; else if (odd == 3u) rgba[4 * i + 3] = nan;
      else if (odd == 4u) rgba[4 * i] = 3.0e38f;                     // a sum that overflows is a float, not undefined behaviour
    }
    if (n > 3) { tr[n - 1] = std::numeric_limits<int32_t>::max(); tr[n - 2] = std::numeric_limits<int32_t>::min(); ob[n - 1] = ob[n - 2] = ob[n - 3]; }
    std::vector<float> out(4 * n), out_unaligned(4 * n);
    std::vector<float> rgba_off(4 * n + 1);                           // ... and so is an image aligned to its floats only, not to 16 bytes
    std::memcpy(rgba_off.data() + 1, rgba.data(), 16 * n);
    for (uint32_t levels = 1; levels <= 5; ++levels) {
      const crh_denoise_params ps[] = {{levels, def.normal_cos, def.depth_ratio, def.until_samples}, {levels, 1.0f, 1.0f, 1u}, {levels, 1e-30f, 3e38f, 1u << 20}, {levels, 0.5f, 1.5f, 4u}};
      for (const crh_denoise_params& p : ps) {
        int rc = crh_denoise_host(rgba.data(), ob.data(), tr.data(), t.data(), W, H, table.data(), nT, &p, out.data());
        if (rc != CRH_OK) { std::printf("denoise %ux%u -> %d\n", W, H, rc); ++failures; continue; }
        rc = crh_denoise_host(rgba_off.data() + 1, ob.data(), tr.data(), t.data(), W, H, raw.data() + 1, nT, &p, out_unaligned.data());
        failures += rc != CRH_OK || std::memcmp(out.data(), out_unaligned.data(), 16 * n) != 0;
        for (size_t i = 0; i < n; ++i) {
          if (std::memcmp(&out[4 * i + 3], &rgba[4 * i + 3], 4) != 0) { std::printf("a sample count that changed\n"); ++failures; break; }
          if ((tr[i] < 0 || !(rgba[4 * i + 3] > 0.f)) && std::memcmp(&out[4 * i], &rgba[4 * i], 16) != 0) { std::printf("a pixel that should pass through did not\n"); ++failures; break; }
        }
        if (p.until_samples == 1u && std::memcmp(out.data(), rgba.data(), 16 * n) != 0) { std::printf("a filter beyond until_samples\n"); ++failures; }
      }
    }
    // no table at all
    failures += crh_denoise_host(rgba.data(), ob.data(), tr.data(), t.data(), W, H, nullptr, 0, &def, out.data()) != CRH_OK;
  }
  // refusals walk their own paths
  {
    int32_t ob[4] = {0, 0, -1, 1}, tr[4] = {0, 1, -1, 2}; float t[4] = {1.f, 2.f, 1e15f, 3.f}, rgba[16] = {0}, out[16];
    crh_denoise_defaults(nullptr);
    auto refused = [&](void (*change)(crh_denoise_params&)) { crh_denoise_params p; crh_denoise_defaults(&p); change(p); return crh_denoise_host(rgba, ob, tr, t, 2, 2, table.data(), nT, &p, out) == CRH_E_INVALID ? 0 : 1; };
    failures += refused([](crh_denoise_params& q) { q.levels = 0u; });
    failures += refused([](crh_denoise_params& q) { q.levels = 6u; });
    failures += refused([](crh_denoise_params& q) { q.normal_cos = 0.f; });
    failures += refused([](crh_denoise_params& q) { q.normal_cos = 1.0000001f; });
    failures += refused([](crh_denoise_params& q) { q.normal_cos = std::numeric_limits<float>::quiet_NaN(); });
    failures += refused([](crh_denoise_params& q) { q.normal_cos = std::numeric_limits<float>::infinity(); });
    failures += refused([](crh_denoise_params& q) { q.depth_ratio = 0.5f; });
    failures += refused([](crh_denoise_params& q) { q.depth_ratio = std::numeric_limits<float>::quiet_NaN(); });
    failures += refused([](crh_denoise_params& q) { q.depth_ratio = -std::numeric_limits<float>::infinity(); });
    failures += refused([](crh_denoise_params& q) { q.until_samples = 0u; });
    failures += refused([](crh_denoise_params& q) { q.until_samples = (1u << 20) + 1u; });
    crh_denoise_params p; crh_denoise_defaults(&p);
    failures += crh_denoise_host(rgba, ob, tr, t, 2, 2, table.data(), nT, &p, out) != CRH_OK;
    failures += crh_denoise_host(nullptr, ob, tr, t, 2, 2, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, nullptr, tr, t, 2, 2, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, nullptr, t, 2, 2, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, nullptr, 2, 2, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, t, 2, 2, table.data(), nT, nullptr, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, t, 2, 2, table.data(), nT, &p, nullptr) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, t, 0, 2, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, t, 2, 0, table.data(), nT, &p, out) != CRH_E_INVALID;
    failures += crh_denoise_host(rgba, ob, tr, t, 2, 2, nullptr, nT, &p, out) != CRH_E_INVALID;
    failures += crh_set_denoise(nullptr, &p) != CRH_E_INVALID;
    failures += crh_get_denoise(nullptr, &p, nullptr) != CRH_E_INVALID;
    failures += crh_read_denoised(nullptr, out) != CRH_E_INVALID;
  }
  std::printf("sanitize_denoise_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
