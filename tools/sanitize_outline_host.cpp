// sanitize_outline_host.cpp -- the host-only side of the feature lines (crh_outline_table_host, crh_outline_mask_host, crh_outline_draw_host;
// cadrays_amd/csrc/crh_outline.cpp, outline_kernels.h: the table, the pair rule, the drawing rule) under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, no device, no context, nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-outline   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
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
  // a table of random, degenerate, huge and tiny triangles; exactly-sized heap blocks, so one byte too many is seen
  const uint32_t nV = 96, nT = 50;
  std::vector<float> pos(3 * nV);
  for (float& p : pos) p = rndf();
  const float big[9] = {3e38f, 3e38f, 3e38f, -3e38f, 3e38f, -3e38f, 1e-40f, -3e38f, 3e38f}, tiny[9] = {1e-45f, 0, 0, 0, 1e-45f, 0, 0, 0, 0};
  std::memcpy(&pos[0], big, sizeof big); std::memcpy(&pos[9], tiny, sizeof tiny);
  std::vector<uint32_t> tri(4 * nT);
  for (uint32_t t = 0; t < nT; ++t) { for (int k = 0; k < 3; ++k) tri[4 * t + k] = rnd() % nV; tri[4 * t + 3] = rnd() % 5u; }
  tri[0] = 0; tri[1] = 1; tri[2] = 2; tri[4] = 3; tri[5] = 4; tri[6] = 5;
  tri[8] = 7; tri[9] = 7; tri[10] = 7;                     // a point
  tri[12] = 9; tri[13] = 9; tri[14] = 12;                  // two equal vertices
  std::vector<Rec> table(nT);
  if (crh_outline_table_host(pos.data(), nV, tri.data(), nT, table.data()) != CRH_OK) { std::printf("table -> error\n"); ++failures; }
  if (!table[2].degenerate || !table[3].degenerate || table[0].degenerate || table[1].degenerate) { std::printf("degenerate flags are wrong\n"); ++failures; }
  for (const Rec& r : table) {
    const double l = std::sqrt((double)r.n[0] * r.n[0] + (double)r.n[1] * r.n[1] + (double)r.n[2] * r.n[2]);
    if (r.degenerate ? l != 0.0 : std::fabs(l - 1.0) > 1e-6) { std::printf("a normal of length %g\n", l); ++failures; }
  }
  // an unaligned table block is the caller's right
  std::vector<unsigned char> raw(sizeof(Rec) * nT + 1);
  failures += crh_outline_table_host(pos.data(), nV, tri.data(), nT, raw.data() + 1) != CRH_OK;
  failures += std::memcmp(raw.data() + 1, table.data(), sizeof(Rec) * nT) != 0;

  const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {64, 2}, {65, 9}, {61, 37}, {130, 67}};
  crh_outline_params def; crh_outline_defaults(&def);
  for (const auto& wh : sizes)
    for (uint32_t nO : {1u, 7u, 5000u}) {
      const uint32_t W = wh[0], H = wh[1];
      const size_t n = (size_t)W * H;
      std::vector<int32_t> ob(n), tr(n); std::vector<float> t(n);
      for (size_t i = 0; i < n; ++i) {
        tr[i] = (int32_t)(rnd() % (nT + 12u)) - 4;                     // -4 .. -1 (misses and nonsense), 0 .. nT - 1, nT .. nT + 7 (beyond the table)
        if (i && rnd() % 2u) tr[i] = tr[i - 1];                        // runs
        ob[i] = tr[i] < 0 ? -1 : (int32_t)((uint32_t)tr[i] % nO);
        t[i] = tr[i] < 0 ? 1e15f : (float)(rnd() % 40u) * 0.5f;        // equal distances, zero among them
      }
      if (n > 3) { tr[n - 1] = std::numeric_limits<int32_t>::max(); tr[n - 2] = std::numeric_limits<int32_t>::min(); ob[n - 1] = ob[n - 2] = ob[n - 3]; t[n - 1] = t[n - 2] = ob[n - 3] < 0 ? 1e15f : 2.0f; }
      std::vector<uint8_t> mask(n), mask_unaligned(n);
      const float thresholds[][2] = {{def.crease_cos, def.depth_ratio}, {1.0f, 1.0f}, {1e-30f, 3e38f}};
      for (const auto& th : thresholds) {
        int rc = crh_outline_mask_host(ob.data(), tr.data(), t.data(), W, H, table.data(), nT, th[0], th[1], mask.data());
        if (rc != CRH_OK) { std::printf("mask %ux%u -> %d\n", W, H, rc); ++failures; continue; }
        rc = crh_outline_mask_host(ob.data(), tr.data(), t.data(), W, H, raw.data() + 1, nT, th[0], th[1], mask_unaligned.data());
        failures += rc != CRH_OK || mask != mask_unaligned;
        for (uint8_t m : mask) if (m & ~7u) { std::printf("a mask byte with unknown bits\n"); ++failures; break; }
        if (nO == 1u) for (size_t i = 0; i < n; ++i) if ((mask[i] & 1u) && ob[i] < 0) { std::printf("an object line on the background\n"); ++failures; break; }
      }
      // no table at all: object lines only
      failures += crh_outline_mask_host(ob.data(), tr.data(), t.data(), W, H, nullptr, 0, 0.5f, 1.02f, mask.data()) != CRH_OK;
      for (uint8_t m : mask) if (m & 6u) { std::printf("a same-object line without a table\n"); ++failures; break; }
      crh_outline_mask_host(ob.data(), tr.data(), t.data(), W, H, table.data(), nT, def.crease_cos, def.depth_ratio, mask.data());
      std::vector<uint8_t> ldr(3 * n), before;
      for (uint8_t& b : ldr) b = (uint8_t)rnd();
      for (uint32_t width = 1; width <= 3; ++width)
        for (uint32_t alpha : {0u, 1u, 128u, 254u, 255u})
          for (uint32_t kinds : {7u, 1u, 6u, 0u}) {
            crh_outline_params p = def; p.width = width; p.alpha = (uint8_t)alpha; p.kinds = kinds; p.rgb[0] = 200; p.rgb[1] = 10; p.rgb[2] = (uint8_t)rnd();
            before = ldr;
            if (crh_outline_draw_host(mask.data(), W, H, &p, ldr.data()) != CRH_OK) { std::printf("draw %ux%u -> error\n", W, H); ++failures; }
            if ((kinds == 0u || alpha == 0u) && before != ldr) { std::printf("a draw that should change nothing did\n"); ++failures; }
          }
    }
  // refusals walk their own paths
  {
    int32_t ob[4] = {0, 0, -1, 1}, tr[4] = {0, 1, -1, 2}; float t[4] = {1.f, 2.f, 1e15f, 3.f}; uint8_t mask[4], ldr[12] = {0};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const uint32_t beyond[4] = {0, 1, nV, 0};
    failures += crh_outline_table_host(pos.data(), nV, beyond, 1, table.data()) != CRH_E_INVALID;
    failures += crh_outline_table_host(nullptr, nV, tri.data(), nT, table.data()) != CRH_E_INVALID;
    failures += crh_outline_table_host(pos.data(), nV, nullptr, nT, table.data()) != CRH_E_INVALID;
    failures += crh_outline_table_host(pos.data(), nV, tri.data(), nT, nullptr) != CRH_E_INVALID;
    failures += crh_outline_table_host(pos.data(), 0, tri.data(), nT, table.data()) != CRH_E_INVALID;
    failures += crh_outline_table_host(pos.data(), nV, tri.data(), 0, table.data()) != CRH_E_INVALID;
    for (float cc : {0.0f, -0.5f, 1.0000001f, nan, inf, -inf})
      failures += crh_outline_mask_host(ob, tr, t, 2, 2, table.data(), nT, cc, 1.02f, mask) != CRH_E_INVALID;
    for (float dr : {0.999f, 0.0f, -2.0f, nan, inf, -inf})
      failures += crh_outline_mask_host(ob, tr, t, 2, 2, table.data(), nT, 0.5f, dr, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(nullptr, tr, t, 2, 2, table.data(), nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, nullptr, t, 2, 2, table.data(), nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, nullptr, 2, 2, table.data(), nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, t, 2, 2, table.data(), nT, 0.5f, 1.02f, nullptr) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, t, 0, 2, table.data(), nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, t, 2, 0, table.data(), nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, t, 2, 2, nullptr, nT, 0.5f, 1.02f, mask) != CRH_E_INVALID;
    failures += crh_outline_mask_host(ob, tr, t, 2, 2, table.data(), nT, 1.0f, 1.0f, mask) != CRH_OK;
    crh_outline_params p;
    crh_outline_defaults(nullptr);
    auto refused = [&](void (*change)(crh_outline_params&)) { crh_outline_defaults(&p); change(p); return crh_outline_draw_host(mask, 2, 2, &p, ldr) == CRH_E_INVALID ? 0 : 1; };
    failures += refused([](crh_outline_params& q) { q.kinds = 8u; });
    failures += refused([](crh_outline_params& q) { q.width = 0u; });
    failures += refused([](crh_outline_params& q) { q.width = 4u; });
    failures += refused([](crh_outline_params& q) { q.crease_cos = 0.f; });
    failures += refused([](crh_outline_params& q) { q.crease_cos = std::numeric_limits<float>::quiet_NaN(); });
    failures += refused([](crh_outline_params& q) { q.depth_ratio = 0.5f; });
    failures += refused([](crh_outline_params& q) { q.depth_ratio = std::numeric_limits<float>::infinity(); });
    crh_outline_defaults(&p);
    failures += crh_outline_draw_host(mask, 2, 2, &p, ldr) != CRH_OK;
    failures += crh_outline_draw_host(nullptr, 2, 2, &p, ldr) != CRH_E_INVALID;
    failures += crh_outline_draw_host(mask, 2, 2, nullptr, ldr) != CRH_E_INVALID;
    failures += crh_outline_draw_host(mask, 2, 2, &p, nullptr) != CRH_E_INVALID;
    failures += crh_outline_draw_host(mask, 0, 2, &p, ldr) != CRH_E_INVALID;
    failures += crh_set_outline(nullptr, &p) != CRH_E_INVALID;
    failures += crh_get_outline(nullptr, &p, nullptr) != CRH_E_INVALID;
    failures += crh_read_outline(nullptr, mask) != CRH_E_INVALID;
  }
  std::printf("sanitize_outline_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
