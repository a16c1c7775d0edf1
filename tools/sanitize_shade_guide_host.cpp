// sanitize_shade_guide_host.cpp -- the host-only side of the shade guide of the denoised display (crh_guide_table_host, crh_shade_guide_host,
// crh_denoise_guided_host; cadrays_amd/csrc/crh_shade_guide.cpp, shade_guide_kernels.h: the texture lookup, the albedo rule, the light test, the dilation, the guided
// pass) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no context, nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-shade-guide   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)(rnd() % 20001u) * 1e-4f - 1.0f; }      // -1 .. 1
static float rnd01() { return (float)(rnd() % 10001u) * 1e-4f; }

struct GuideRec { float uv[6]; int32_t material; uint32_t has_uv; };
struct NormalRec { float n[3]; uint32_t degenerate; uint32_t v[3]; uint32_t pad; };

int main()
{
  int failures = 0;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // geometry: uv of every magnitude the lookup guards against; exactly-sized heap blocks, so one element too many is seen
  const uint32_t nV = 90, nT = 48;
  std::vector<float> pos(3 * nV), uv(2 * nV);
  for (float& p : pos) p = rndf();
  for (uint32_t v = 0; v < nV; ++v) {
    const uint32_t kind = rnd() % 8u;
    const float s = kind == 0u ? 4194304.0f : (kind == 1u ? 3.0e9f : (kind == 2u ? 1.0e-30f : 3.0f));
    uv[2 * v] = rndf() * s; uv[2 * v + 1] = rndf() * s;
  }
  uv[0] = -0.0f; uv[1] = 1.0f; uv[2] = 4194303.5f; uv[3] = -4194303.5f; uv[4] = 3.0e38f; uv[5] = -3.0e38f;
  std::vector<uint32_t> tri(4 * nT);
  for (uint32_t t = 0; t < nT; ++t) { for (int k = 0; k < 3; ++k) tri[4 * t + k] = rnd() % nV; tri[4 * t + 3] = t % 9u; }      // materials 0 .. 8: 7 and 8 lie beyond the table of 7
  tri[3] = 0xFFFFFFFFu;                                     // material -1
  std::vector<GuideRec> table(nT), table_no_uv(nT);
  failures += crh_guide_table_host(uv.data(), nV, tri.data(), nT, table.data()) != CRH_OK;
  failures += crh_guide_table_host(nullptr, 0, tri.data(), nT, table_no_uv.data()) != CRH_OK;
  failures += crh_guide_table_host(uv.data(), nV, nullptr, nT, table.data()) != CRH_E_INVALID;
  failures += crh_guide_table_host(uv.data(), nV, tri.data(), 0, table.data()) != CRH_E_INVALID;
  failures += crh_guide_table_host(uv.data(), nV, tri.data(), nT, nullptr) != CRH_E_INVALID;
  { uint32_t bad[4] = {0, 1, nV, 0}; GuideRec r; failures += crh_guide_table_host(uv.data(), nV, bad, 1, &r) != CRH_E_INVALID; }
  std::vector<unsigned char> raw(sizeof(GuideRec) * nT + 1);      // an unaligned table block is the caller's right
  std::memcpy(raw.data() + 1, table.data(), sizeof(GuideRec) * nT);

  // the scene: seven materials (plain, three textured with odd scales, one with an unbound slot, one with a slot beyond the slots, one black), three slots (1 x 1,
  // 5 x 7 with alpha below 1, one empty), three lights (one directional, one positional, one of radius 0)
  std::vector<crh_bsdf> mats(7);
  std::memset(mats.data(), 0, sizeof(crh_bsdf) * mats.size());
  for (uint32_t m = 0; m < 7u; ++m) for (int k = 0; k < 3; ++k) { mats[m].Kd[k] = rnd01(); mats[m].Ks[k] = 0.25f * rnd01(); mats[m].Kc[k] = 0.1f * rnd01(); mats[m].Kt[k] = 0.5f * rnd01(); }
  mats[1].Kd[3] = 1.f; mats[1].Kt[3] = 1.f; mats[1].Le[3] = 1.f;
  mats[2].Kd[3] = 2.f; mats[2].Kt[3] = -2.f; mats[2].Le[3] = 0.5f;
  mats[3].Kd[3] = 2.f; mats[3].Kt[3] = 1.0e30f; mats[3].Le[3] = 3.0e38f;      // a scale that overflows: the coordinate becomes 0
  mats[4].Kd[3] = 3.f;                                                         // slot 2: empty
  mats[5].Kd[3] = 100.f;                                                       // beyond the slots
  for (int k = 0; k < 3; ++k) { mats[6].Kd[k] = mats[6].Ks[k] = mats[6].Kc[k] = mats[6].Kt[k] = 0.f; }
  const uint32_t desc[12] = {0u, 1u, 1u, 0u, 1u, 5u, 7u, 0u, 0u, 0u, 0u, 0u};
  std::vector<float> texels(4 * 36);
  for (size_t i = 0; i < 36; ++i) { for (int k = 0; k < 3; ++k) texels[4 * i + k] = rnd01(); texels[4 * i + 3] = (i % 3u) ? 1.f : 0.5f; }
  crh_light lights[3];
  std::memset(lights, 0, sizeof lights);
  lights[0].vec[1] = 1.f; lights[0].smoothness = 0.3f;
  lights[1].vec[0] = 0.1f; lights[1].vec[1] = 1.5f; lights[1].vec[2] = 0.1f; lights[1].is_point = 1.f; lights[1].smoothness = 0.4f;
  lights[2].vec[0] = -0.3f; lights[2].vec[1] = 1.0f; lights[2].is_point = 1.f; lights[2].smoothness = 0.f;
  crh_shade_guide_scene scene;
  std::memset(&scene, 0, sizeof scene);
  scene.mats = mats.data(); scene.n_mats = 7; scene.texels = texels.data(); scene.n_texels = 36; scene.tex_desc = desc; scene.n_tex = 3; scene.lights = lights; scene.n_lights = 3;

  // the edge shapes: one pixel, one row, one column, frames narrower than the dilation and the window of step 16, more than one 64-pixel chunk per row
  const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 300}, {67, 45}, {130, 3}};
  crh_shade_guide_params def; crh_shade_guide_defaults(&def); crh_shade_guide_defaults(nullptr);
  crh_denoise_params dn; crh_denoise_defaults(&dn);
  for (const auto& wh : sizes) {
    const uint32_t W = wh[0], H = wh[1];
    const size_t n = (size_t)W * H;
    std::vector<int32_t> ob(n), tr(n); std::vector<float> t(n), bary(2 * n), rays(8 * n), rgba(4 * n);
    for (size_t i = 0; i < n; ++i) {
      tr[i] = (int32_t)(rnd() % (nT + 12u)) - 4;                     // -4 .. -1 (misses and nonsense), 0 .. nT - 1, nT .. nT + 7 (beyond the table)
      if (i && rnd() % 2u) tr[i] = tr[i - 1];
      ob[i] = tr[i] < 0 ? -1 : (int32_t)((uint32_t)tr[i] % 3u);
      t[i] = tr[i] < 0 ? 1e15f : 1.0f + (float)(rnd() % 40u) * 0.1f;
      bary[2 * i] = rnd01(); bary[2 * i + 1] = rnd01() * (1.f - bary[2 * i]);
      const float x = ((float)(i % W) + 0.5f) / (float)W - 0.5f, y = 0.5f - ((float)(i / W) + 0.5f) / (float)H;
      const float l = std::sqrt(x * x + 1.f + y * y);
      float* r = &rays[8 * i];
      r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; r[3] = 1e15f; r[4] = x / l; r[5] = 1.f / l; r[6] = y / l; r[7] = 0.f;
      for (int k = 0; k < 3; ++k) rgba[4 * i + k] = (float)(rnd() % 1000u) * 1e-3f;
      rgba[4 * i + 3] = (float)(rnd() % 6u);
      const uint32_t odd = rnd() % 50u;
      if (odd == 0u) rgba[4 * i] = inf; else if (odd == 1u) rgba[4 * i + 1] = nan; else if (odd == 2u) rgba[4 * i] = 3.0e38f;
    }
    if (n > 3) { tr[n - 1] = std::numeric_limits<int32_t>::max(); tr[n - 2] = std::numeric_limits<int32_t>::min(); bary[0] = nan; bary[3] = inf; rays[8 * (n - 1)] = 0.1f; rays[8 * (n - 1) + 1] = 1.5f; rays[8 * (n - 1) + 2] = 0.1f; }      // (an origin IN the light: dist == 0)
    std::vector<float> plane(4 * n), plane2(4 * n), out(4 * n);
    const crh_shade_guide_params ps[] = {def, {1u, 1u, 1.0f, 0u}, {1u, 1u, 1.0e-30f, 2u}, {0u, 1u, 0.5f, 2u}, {1u, 0u, 0.5f, 1u}, {0u, 0u, 1.0f, 0u}};
    for (int gamma2 = 0; gamma2 < 2; ++gamma2)
      for (const crh_shade_guide_params& p : ps) {
        scene.gamma2 = gamma2;
        int rc = crh_shade_guide_host(&scene, rays.data(), tr.data(), t.data(), bary.data(), W, H, table.data(), nT, &p, plane.data());
        if (rc != CRH_OK) { std::printf("plane %ux%u -> %d\n", W, H, rc); ++failures; continue; }
        rc = crh_shade_guide_host(&scene, rays.data(), tr.data(), t.data(), bary.data(), W, H, raw.data() + 1, nT, &p, plane2.data());
        failures += rc != CRH_OK || std::memcmp(plane.data(), plane2.data(), 16 * n) != 0;
        for (size_t i = 0; i < n; ++i) {
          const float* g = &plane[4 * i];
          const float top = 1.0f / p.albedo_floor;
          if (!(g[0] > 0.f && g[0] <= top && g[1] > 0.f && g[1] <= top && g[2] > 0.f && g[2] <= top) || (g[3] != 0.f && g[3] != 1.f)) { std::printf("a weight outside (0, 1 / floor] or a flag that is no flag\n"); ++failures; break; }
          if ((!p.demodulate || tr[i] < 0 || (uint32_t)tr[i] >= nT) && (g[0] != 1.f || g[1] != 1.f || g[2] != 1.f)) { std::printf("a pixel without a record that is demodulated\n"); ++failures; break; }
          if (!p.lights && g[3] != 0.f) { std::printf("a flag with lights off\n"); ++failures; break; }
        }
        failures += crh_shade_guide_host(&scene, rays.data(), tr.data(), t.data(), bary.data(), W, H, table_no_uv.data(), nT, &p, plane2.data()) != CRH_OK;
        for (uint32_t levels = 1; levels <= 5; levels += 2) {
          const crh_denoise_params q{levels, dn.normal_cos, dn.depth_ratio, dn.until_samples};
          rc = crh_denoise_guided_host(rgba.data(), ob.data(), tr.data(), t.data(), W, H, nullptr, 0, plane.data(), &q, out.data());
          if (rc != CRH_OK) { std::printf("guided %ux%u -> %d\n", W, H, rc); ++failures; continue; }
          for (size_t i = 0; i < n; ++i)
            if ((tr[i] < 0 || !(rgba[4 * i + 3] > 0.f) || plane[4 * i + 3] != 0.f) && std::memcmp(&out[4 * i], &rgba[4 * i], 16) != 0) { std::printf("a pixel that should pass through did not\n"); ++failures; break; }
        }
      }
    // no table, no textures, no lights
    crh_shade_guide_scene bare; std::memset(&bare, 0, sizeof bare); bare.mats = mats.data(); bare.n_mats = 1;
    failures += crh_shade_guide_host(&bare, rays.data(), tr.data(), t.data(), bary.data(), W, H, nullptr, 0, &def, plane.data()) != CRH_OK;
    // the plane of ones gives the unguided filter
    std::vector<float> ones(4 * n), plain(4 * n);
    for (size_t i = 0; i < n; ++i) { ones[4 * i] = ones[4 * i + 1] = ones[4 * i + 2] = 1.f; ones[4 * i + 3] = 0.f; }
    failures += crh_denoise_host(rgba.data(), ob.data(), tr.data(), t.data(), W, H, nullptr, 0, &dn, plain.data()) != CRH_OK;
    failures += crh_denoise_guided_host(rgba.data(), ob.data(), tr.data(), t.data(), W, H, nullptr, 0, ones.data(), &dn, out.data()) != CRH_OK;
    if (std::memcmp(plain.data(), out.data(), 16 * n) != 0) { std::printf("the plane of ones changed the filter\n"); ++failures; }
  }
  // refusals walk their own paths
  {
    int32_t tr[4] = {0, 1, -1, 2}, ob[4] = {0, 0, -1, 1}; float t[4] = {1.f, 2.f, 1e15f, 3.f}, bary[8] = {0}, rays[32] = {0}, rgba[16] = {0}, plane[16], out[16];
    for (int i = 0; i < 4; ++i) rays[8 * i + 5] = 1.f;
    scene.gamma2 = 0;
    auto refused = [&](void (*change)(crh_shade_guide_params&)) { crh_shade_guide_params p; crh_shade_guide_defaults(&p); change(p); return crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) == CRH_E_INVALID ? 0 : 1; };
    failures += refused([](crh_shade_guide_params& q) { q.demodulate = 2u; });
    failures += refused([](crh_shade_guide_params& q) { q.lights = 0xFFFFFFFFu; });
    failures += refused([](crh_shade_guide_params& q) { q.albedo_floor = 0.f; });
    failures += refused([](crh_shade_guide_params& q) { q.albedo_floor = 1.0000001f; });
    failures += refused([](crh_shade_guide_params& q) { q.albedo_floor = -1.f; });
    failures += refused([](crh_shade_guide_params& q) { q.albedo_floor = std::numeric_limits<float>::quiet_NaN(); });
    failures += refused([](crh_shade_guide_params& q) { q.albedo_floor = std::numeric_limits<float>::infinity(); });
    failures += refused([](crh_shade_guide_params& q) { q.light_dilate = 3u; });
    crh_shade_guide_params p; crh_shade_guide_defaults(&p);
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_OK;
    failures += crh_shade_guide_host(nullptr, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, nullptr, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, nullptr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, nullptr, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, nullptr, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 0, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 0, table.data(), nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 2, nullptr, nT, &p, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 2, table.data(), nT, nullptr, plane) != CRH_E_INVALID;
    failures += crh_shade_guide_host(&scene, rays, tr, t, bary, 2, 2, table.data(), nT, &p, nullptr) != CRH_E_INVALID;
    crh_shade_guide_scene s2 = scene;
    s2.n_texels = 35;                                       // slot 1 reaches one texel beyond
    failures += crh_shade_guide_host(&s2, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    s2 = scene; s2.n_mats = 0;
    failures += crh_shade_guide_host(&s2, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    s2 = scene; s2.lights = nullptr;
    failures += crh_shade_guide_host(&s2, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    std::vector<crh_bsdf> m2 = mats; m2[2].Ks[1] = nan; s2 = scene; s2.mats = m2.data();
    failures += crh_shade_guide_host(&s2, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    m2 = mats; m2[2].Kd[3] = 3.0e9f; s2.mats = m2.data();   // a slot no int holds
    failures += crh_shade_guide_host(&s2, rays, tr, t, bary, 2, 2, table.data(), nT, &p, plane) != CRH_E_INVALID;
    crh_denoise_params q; crh_denoise_defaults(&q);
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 0, plane, &q, out) != CRH_OK;
    failures += crh_denoise_guided_host(nullptr, ob, tr, t, 2, 2, nullptr, 0, plane, &q, out) != CRH_E_INVALID;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 0, nullptr, &q, out) != CRH_E_INVALID;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 0, plane, nullptr, out) != CRH_E_INVALID;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 0, plane, &q, nullptr) != CRH_E_INVALID;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 0, 2, nullptr, 0, plane, &q, out) != CRH_E_INVALID;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 3, plane, &q, out) != CRH_E_INVALID;
    q.levels = 6u;
    failures += crh_denoise_guided_host(rgba, ob, tr, t, 2, 2, nullptr, 0, plane, &q, out) != CRH_E_INVALID;
    failures += crh_set_shade_guide(nullptr, &p) != CRH_E_INVALID;
    failures += crh_get_shade_guide(nullptr, &p, nullptr) != CRH_E_INVALID;
    failures += crh_read_shade_guide(nullptr, out) != CRH_E_INVALID;
    failures += crh_read_hit_uv(nullptr, out) != CRH_E_INVALID;
    failures += crh_bench_shade_guide(nullptr, 1, nullptr, out) != CRH_E_INVALID;
  }
  std::printf("sanitize_shade_guide_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
