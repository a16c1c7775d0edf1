// sanitize_region_host.cpp -- the host-only side of the region queries (crh_region_stats_host, crh_region_select; cadrays_amd/csrc/crh_region.cpp,
// region_kernels.hip: the polygon rule and the records) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no context,
// nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-region   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main()
{
  int failures = 0;
  const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {64, 2}, {61, 37}, {130, 67}};
  for (const auto& wh : sizes)
    for (uint32_t nO : {1u, 7u, 5000u}) {
      const uint32_t W = wh[0], H = wh[1];
      std::vector<int32_t> ob((size_t)W * H); std::vector<float> t((size_t)W * H);
      for (size_t i = 0; i < ob.size(); ++i) {
        ob[i] = (int32_t)(rnd() % (nO + 3u)) - 1;             // -1 (background), 0 .. nO - 1, nO and nO + 1 (out of range: background)
        t[i] = ob[i] < 0 ? 1e15f : (float)(rnd() % 1000u) * 0.01f;
      }
      std::vector<crh_region_stats> st((size_t)nO + 1); std::vector<uint8_t> sel(nO);
      const int32_t L = 1 << 20;
      std::vector<std::vector<int32_t>> polys = {
          {},                                                                           // none
          {1, 0, (int32_t)W - 1, (int32_t)H / 2, (int32_t)W / 3, (int32_t)H},           // a triangle
          {0, 0, (int32_t)W, (int32_t)H, (int32_t)W, 0, 0, (int32_t)H},                 // a bow-tie
          {-L, -L, L, -L + 3, (int32_t)W / 2, L},                                       // vertices at the limit: the products reach 2^44
          {L, L, -L, L, -L, -L, L, -L},
          {0, 0, 5, 0, 5, 0, 5, 5, 0, 5, 0, 0},                                         // repeated vertices, horizontal edges
      };
      std::vector<int32_t> big(512);
      for (size_t k = 0; k < 256; ++k) { big[2 * k] = (int32_t)(rnd() % (W + 8u)) - 4; big[2 * k + 1] = (int32_t)(rnd() % (H + 8u)) - 4; }
      polys.push_back(big);
      const uint32_t rects[][4] = {{0, 0, W, H}, {W / 2, H / 2, W / 2 + 1, H / 2 + 1}, {W / 3, H / 4, W + 50, H + 9}, {W + 5, H + 5, W + 20, H + 30}, {0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu}};
      for (const auto& p : polys)
        for (int r = -1; r < 5; ++r) {
          const uint32_t n_poly = (uint32_t)(p.size() / 2);
          const int rc = crh_region_stats_host(ob.data(), t.data(), W, H, r < 0 ? nullptr : rects[r], n_poly ? p.data() : nullptr, n_poly, st.data(), nO);
          if (rc != CRH_OK) { std::printf("stats %ux%u nO=%u -> %d\n", W, H, nO, rc); ++failures; continue; }
          uint64_t frame = 0;
          for (uint32_t o = 0; o <= nO; ++o) {
            frame += st[o].pixels_frame;
            if (st[o].pixels > st[o].pixels_frame || (st[o].pixels && !(st[o].x0 < st[o].x1 && st[o].y0 < st[o].y1 && st[o].x1 <= W && st[o].y1 <= H && st[o].t_min <= st[o].t_max))) {
              std::printf("record %u of %ux%u nO=%u is inconsistent\n", o, W, H, nO); ++failures;
            }
          }
          if (frame != (uint64_t)W * H) { std::printf("pixels_frame sums to %llu of %ux%u\n", (unsigned long long)frame, W, H); ++failures; }
          for (int mode : {CRH_REGION_TOUCHED, CRH_REGION_ENCLOSED})
            for (uint32_t least : {0u, 1u, 7u})
              failures += crh_region_select(st.data(), nO, mode, least, sel.data()) != CRH_OK;
        }
    }
  // refusals walk their own paths
  {
    int32_t ob[4] = {0, 0, -1, 1}; float t[4] = {1.f, 2.f, 1e15f, 3.f}; crh_region_stats st[3]; uint8_t sel[2];
    const int32_t two[4] = {0, 0, 1, 1}, far[6] = {0, 0, (1 << 20) + 1, 0, 1, 1}; std::vector<int32_t> many(2 * 257, 0);
    const uint32_t inverted[4] = {2, 0, 1, 2};
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, two, 2, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, two, 1, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, many.data(), 257, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, far, 3, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, nullptr, 3, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, inverted, nullptr, 0, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, nullptr, 0, nullptr, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(nullptr, t, 2, 2, nullptr, nullptr, 0, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, nullptr, 2, 2, nullptr, nullptr, 0, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, nullptr, 0, st, 0) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 0, 2, nullptr, nullptr, 0, st, 2) != CRH_E_INVALID;
    failures += crh_region_stats_host(ob, t, 2, 2, nullptr, nullptr, 0, st, 2) != CRH_OK;
    failures += crh_region_select(nullptr, 2, CRH_REGION_TOUCHED, 1, sel) != CRH_E_INVALID;
    failures += crh_region_select(st, 2, CRH_REGION_TOUCHED, 1, nullptr) != CRH_E_INVALID;
    failures += crh_region_select(st, 0, CRH_REGION_TOUCHED, 1, sel) != CRH_E_INVALID;
    failures += crh_region_select(st, 2, 2, 1, sel) != CRH_E_INVALID;
    failures += crh_region_select(st, 2, CRH_REGION_ENCLOSED, 1, sel) != CRH_OK;
    failures += crh_query_region(nullptr, nullptr, nullptr, 0, st, 2) != CRH_E_INVALID;
  }
  std::printf("sanitize_region_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
