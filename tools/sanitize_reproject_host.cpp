// sanitize_reproject_host.cpp -- the host-only side of the reprojected display history (crh_reproject_host, crh_reproject_frame_host; cadrays_amd/csrc/crh_reproject.cpp,
// reproject_kernels.h: the projection, the gather, the blend; and the per-object history deltas: crh_reproject_delta_host, crh_reproject_motion_host) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no context,
// nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-reproject   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
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
  const uint32_t nV = 96, nT = 50;
  std::vector<float> pos(3 * nV);
  for (float& p : pos) p = rndf();
  std::vector<uint32_t> tri(4 * nT);
  for (uint32_t t = 0; t < nT; ++t) { for (int k = 0; k < 3; ++k) tri[4 * t + k] = rnd() % nV; tri[4 * t + 3] = 0; }
  tri[8] = 7; tri[9] = 7; tri[10] = 7;                     // a degenerate record
  std::vector<Rec> table(nT);
  failures += crh_outline_table_host(pos.data(), nV, tri.data(), nT, table.data()) != CRH_OK;
  std::vector<unsigned char> raw(sizeof(Rec) * nT + 1);    // an unaligned table block is the caller's right
  std::memcpy(raw.data() + 1, table.data(), sizeof(Rec) * nT);

  // cameras: the view in force looks down +y; the histories' views are near it, far from it, behind it, orthographic, and one frame is nonsense (zeros, NaN)
  crh_camera now{}; now.eye[1] = -4.f; now.dir[1] = 1.f; now.up[2] = 1.f; now.fovy_deg = 50.f;
  std::vector<crh_reproject_frame> frames;
  for (int k = 0; k < 5; ++k) {
    crh_camera c = now;
    if (k == 1) { c.eye[0] = 0.3f; c.dir[0] = 0.05f; }
    if (k == 2) { c.dir[1] = -1.f; }
    if (k == 3) { c.is_ortho = 1; c.ortho_scale = 2.5f; c.eye[2] = 0.2f; }
    if (k == 4) { c.eye[0] = 3.f; c.dir[0] = -0.6f; c.fovy_deg = 120.f; }
    crh_reproject_frame F;
    failures += crh_reproject_frame_host(&c, 7, 5, &F) != CRH_OK;
    frames.push_back(F);
  }
  { crh_reproject_frame F; std::memset(&F, 0, sizeof F); frames.push_back(F); F.tan_half = nan; F.eye[0] = inf; F.aspect = -1.f; frames.push_back(F); }

  // the edge shapes: one pixel, one row, one column, more than one 64-pixel chunk per row; exactly-sized heap blocks, so one element too many is seen
  const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 300}, {67, 45}, {130, 3}};
  crh_reproject_params def; crh_reproject_defaults(&def);
  for (const auto& wh : sizes) {
    const uint32_t W = wh[0], H = wh[1];
    const size_t n = (size_t)W * H;
    std::vector<int32_t> ob(n), tr(n), hob(n), htr(n); std::vector<float> t(n), ht(n), rgba(4 * n), hist(4 * n), rays(8 * n);
    auto fill = [&](std::vector<int32_t>& o, std::vector<int32_t>& r, std::vector<float>& d, std::vector<float>& img) {
      for (size_t i = 0; i < n; ++i) {
        r[i] = (int32_t)(rnd() % (nT + 12u)) - 4;                      // -4 .. -1 (misses and nonsense), 0 .. nT - 1, nT .. nT + 7 (beyond the table)
        if (i && rnd() % 2u) r[i] = r[i - 1];
        o[i] = r[i] < 0 ? -1 : (int32_t)((uint32_t)r[i] % 3u);
        d[i] = r[i] < 0 ? 3.4e38f : 2.0f + (float)(rnd() % 40u) * 0.1f;
        for (int k = 0; k < 3; ++k) img[4 * i + k] = (float)(rnd() % 1000u) * 1e-3f;
        img[4 * i + 3] = (float)(rnd() % 6u);
        const uint32_t odd = rnd() % 40u;
        if (odd == 0u) img[4 * i] = inf; else if (odd == 1u) img[4 * i + 1] = nan; else if (odd == 2u) img[4 * i + 2] = -inf; else if (odd == 3u) img[4 * i + 3] = nan;
        else if (odd == 4u) img[4 * i] = 3.0e38f; else if (odd == 5u) img[4 * i + 3] = inf; else if (odd == 6u) d[i] = nan; else if (odd == 7u) d[i] = -1.0f;
      }
      if (n > 3) { r[n - 1] = std::numeric_limits<int32_t>::max(); r[n - 2] = std::numeric_limits<int32_t>::min(); o[n - 1] = o[n - 2] = o[n - 3]; }
    };
    fill(ob, tr, t, rgba); fill(hob, htr, ht, hist);
    for (size_t i = 0; i < n; ++i) {                                   // rays of a pinhole at `now`, a few of them nonsense
      const float u = ((float)(i % W) + 0.5f) / (float)W * 2.f - 1.f, v = 1.f - ((float)(i / W) + 0.5f) / (float)H * 2.f;
      float d[3] = {0.45f * u, 1.f, 0.45f * v};
      const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      float* r = &rays[8 * i];
      r[0] = now.eye[0]; r[1] = now.eye[1]; r[2] = now.eye[2]; r[3] = 3.4e38f; r[4] = d[0] / l; r[5] = d[1] / l; r[6] = d[2] / l; r[7] = 0.f;
      const uint32_t odd = rnd() % 60u;
      if (odd == 0u) r[4] = nan; else if (odd == 1u) r[0] = inf; else if (odd == 2u) r[5] = 3.0e38f;
    }
    std::vector<float> out(4 * n), out_unaligned(4 * n), rgba_off(4 * n + 1), hist_off(4 * n + 1);
    std::memcpy(rgba_off.data() + 1, rgba.data(), 16 * n); std::memcpy(hist_off.data() + 1, hist.data(), 16 * n);      // images aligned to their floats only
    const crh_reproject_params ps[] = {def, {1.0f, 1u, 1.0f, 1.0f}, {1024.0f, 1u << 20, 1e-30f, 3e38f}, {2.5f, 4u, 0.5f, 1.5f}};
    for (const crh_reproject_frame& F : frames)
      for (const crh_reproject_params& p : ps) {
        int rc = crh_reproject_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &F, table.data(), nT, W, H, &p, out.data());
        if (rc != CRH_OK) { std::printf("reproject %ux%u -> %d\n", W, H, rc); ++failures; continue; }
        rc = crh_reproject_host(rgba_off.data() + 1, rays.data(), ob.data(), tr.data(), t.data(), hist_off.data() + 1, hob.data(), htr.data(), ht.data(), &F, raw.data() + 1, nT, W, H, &p,
                                out_unaligned.data());
        failures += rc != CRH_OK || std::memcmp(out.data(), out_unaligned.data(), 16 * n) != 0;
        for (size_t i = 0; i < n; ++i)
          if ((tr[i] < 0 || rgba[4 * i + 3] >= (float)p.until_samples) && std::memcmp(&out[4 * i], &rgba[4 * i], 16) != 0) { std::printf("a pixel that should pass through did not\n"); ++failures; break; }
      }
    // per-object history deltas: the table of crh_reproject_delta_host (exactly-sized blocks, an unaligned copy) through crh_reproject_motion_host; the objects
    // of `fill` are 0 .. 2, so a table of two records leaves object 2 outside it; an unflagged table and no table give crh_reproject_host's bytes
    {
      const float xh[36] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      const float xc[36] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.9f, -0.2f, 0, 0.3f, 0.2f, 0.9f, 0, -0.1f, 0, 0, 1.1f, 0.05f, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3};
      std::vector<crh_reproject_delta> dt(3), zero(3);
      std::vector<unsigned char> dt_off(sizeof(crh_reproject_delta) * 3 + 1);
      failures += crh_reproject_delta_host(xh, xc, 3, dt.data()) != CRH_OK || crh_reproject_delta_host(xh, xc, 3, dt_off.data() + 1) != CRH_OK;
      failures += std::memcmp(dt.data(), dt_off.data() + 1, sizeof(crh_reproject_delta) * 3) != 0;
      failures += dt[0].flag != 0u || dt[1].flag != 1u || dt[2].flag != 2u;
      failures += crh_reproject_delta_host(xh, xh, 3, zero.data()) != CRH_OK || zero[0].flag || zero[1].flag || zero[2].flag;
      const crh_reproject_motion_params mps[] = {{16.f, 8.f}, {1.f, 1024.f}, {1024.f, 1.f}, {2.5f, 1.5f}};
      std::vector<float> plain(4 * n), moved(4 * n);
      for (const crh_reproject_frame& F : frames) {
        failures += crh_reproject_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &F, table.data(), nT, W, H, &def, plain.data()) != CRH_OK;
        for (const crh_reproject_motion_params& mp : mps) {
          for (uint32_t nO = 1; nO <= 3; ++nO) {
            int rc = crh_reproject_motion_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &F, table.data(), nT, W, H, &def,
                                               dt.data(), nO, &mp, out.data());
            if (rc != CRH_OK) { std::printf("reproject motion %ux%u -> %d\n", W, H, rc); ++failures; continue; }
            rc = crh_reproject_motion_host(rgba_off.data() + 1, rays.data(), ob.data(), tr.data(), t.data(), hist_off.data() + 1, hob.data(), htr.data(), ht.data(), &F, raw.data() + 1, nT, W, H,
                                           &def, dt_off.data() + 1, nO, &mp, out_unaligned.data());
            failures += rc != CRH_OK || std::memcmp(out.data(), out_unaligned.data(), 16 * n) != 0;
            if (nO == 3)
              for (size_t i = 0; i < n; ++i)
                if ((tr[i] < 0 || ob[i] == 2) && std::memcmp(&out[4 * i], &rgba[4 * i], 16) != 0) { std::printf("a pixel of an object without history did not pass through\n"); ++failures; break; }
          }
          failures += crh_reproject_motion_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &F, table.data(), nT, W, H, &def,
                                                zero.data(), 3, &mp, moved.data()) != CRH_OK || std::memcmp(moved.data(), plain.data(), 16 * n) != 0;
        }
        failures += crh_reproject_motion_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &F, table.data(), nT, W, H, &def,
                                              nullptr, 0, nullptr, moved.data()) != CRH_OK || std::memcmp(moved.data(), plain.data(), 16 * n) != 0;
      }
      // the refusals of the new entry points
      const crh_reproject_motion_params good = mps[0], bad_lo = {0.5f, 8.f}, bad_hi = {16.f, 1025.f}, bad_nan = {nan, 8.f}, bad_inf = {16.f, inf};
      auto call = [&](const void* d, uint32_t nO, const crh_reproject_motion_params* mp) {
        return crh_reproject_motion_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &frames[0], table.data(), nT, W, H, &def, d, nO, mp, out.data());
      };
      failures += call(dt.data(), 3, &good) != CRH_OK;
      failures += call(nullptr, 3, &good) != CRH_E_INVALID || call(dt.data(), 3, nullptr) != CRH_E_INVALID;
      failures += call(dt.data(), 3, &bad_lo) != CRH_E_INVALID || call(dt.data(), 3, &bad_hi) != CRH_E_INVALID || call(dt.data(), 3, &bad_nan) != CRH_E_INVALID || call(dt.data(), 3, &bad_inf) != CRH_E_INVALID;
      std::vector<crh_reproject_delta> three = dt; three[1].flag = 3u;
      failures += call(three.data(), 3, &good) != CRH_E_INVALID;
      failures += crh_reproject_delta_host(nullptr, xc, 3, dt.data()) != CRH_E_INVALID || crh_reproject_delta_host(xh, nullptr, 3, dt.data()) != CRH_E_INVALID;
      failures += crh_reproject_delta_host(xh, xc, 3, nullptr) != CRH_E_INVALID || crh_reproject_delta_host(nullptr, nullptr, 0, nullptr) != CRH_OK;
      const float odd[24] = {nan, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1e30f, 0, 0, 0, 0, 1e30f, 0, 0, 0, 0, 1e30f, inf};
      const float tiny[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1e-30f, 0, 0, 0, 0, 1e-30f, 0, 0, 0, 0, 1e-30f, 0};
      crh_reproject_delta two[2];
      failures += crh_reproject_delta_host(odd, tiny, 2, two) != CRH_OK || two[0].flag != 2u || two[1].flag != 2u;
      failures += crh_reproject_delta_host(tiny, odd, 2, two) != CRH_OK || two[0].flag != 2u || two[1].flag != 2u;
      crh_reproject_motion_params got; crh_reproject_motion_defaults(&got); crh_reproject_motion_defaults(nullptr);
      failures += !(got.max_history_moved == 16.f) || crh_set_reproject_motion(nullptr, &got) != CRH_E_INVALID || crh_get_reproject_motion(nullptr, &got, nullptr, nullptr) != CRH_E_INVALID;
      failures += crh_bench_reproject_motion(nullptr, 1, nullptr) != CRH_E_INVALID;
    }
    // no table at all, and no history at all: the accumulator, bitwise
    failures += crh_reproject_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), hist.data(), hob.data(), htr.data(), ht.data(), &frames[0], nullptr, 0, W, H, &def, out.data()) != CRH_OK;
    failures += crh_reproject_host(rgba.data(), rays.data(), ob.data(), tr.data(), t.data(), nullptr, nullptr, nullptr, nullptr, nullptr, table.data(), nT, W, H, &def, out.data()) != CRH_OK;
    failures += std::memcmp(out.data(), rgba.data(), 16 * n) != 0;
  }
  // refusals walk their own paths
  {
    int32_t ob[4] = {0, 0, -1, 1}, tr[4] = {0, 1, -1, 2}; float t[4] = {1.f, 2.f, 3.4e38f, 3.f}, rgba[16] = {0}, rays[32] = {0}, out[16];
    const crh_reproject_frame& F = frames[0];
    crh_reproject_defaults(nullptr);
    auto refused = [&](void (*change)(crh_reproject_params&)) {
      crh_reproject_params p; crh_reproject_defaults(&p); change(p);
      return crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) == CRH_E_INVALID ? 0 : 1;
    };
    failures += refused([](crh_reproject_params& q) { q.max_history = 0.5f; });
    failures += refused([](crh_reproject_params& q) { q.max_history = 1025.f; });
    failures += refused([](crh_reproject_params& q) { q.max_history = std::numeric_limits<float>::quiet_NaN(); });
    failures += refused([](crh_reproject_params& q) { q.until_samples = 0u; });
    failures += refused([](crh_reproject_params& q) { q.until_samples = (1u << 20) + 1u; });
    failures += refused([](crh_reproject_params& q) { q.normal_cos = 0.f; });
    failures += refused([](crh_reproject_params& q) { q.normal_cos = 1.0000001f; });
    failures += refused([](crh_reproject_params& q) { q.normal_cos = std::numeric_limits<float>::infinity(); });
    failures += refused([](crh_reproject_params& q) { q.depth_ratio = 0.5f; });
    failures += refused([](crh_reproject_params& q) { q.depth_ratio = -std::numeric_limits<float>::infinity(); });
    crh_reproject_params p; crh_reproject_defaults(&p);
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_OK;
    failures += crh_reproject_host(nullptr, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, nullptr, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, nullptr, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, nullptr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, nullptr, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, nullptr, tr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, nullptr, t, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, nullptr, &F, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, nullptr, table.data(), nT, 2, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, nullptr, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 2, &p, nullptr) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 0, 2, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, table.data(), nT, 2, 0, &p, out) != CRH_E_INVALID;
    failures += crh_reproject_host(rgba, rays, ob, tr, t, rgba, ob, tr, t, &F, nullptr, nT, 2, 2, &p, out) != CRH_E_INVALID;
    crh_camera bad = now; bad.dir[0] = std::numeric_limits<float>::quiet_NaN();
    crh_reproject_frame G;
    failures += crh_reproject_frame_host(&bad, 4, 4, &G) != CRH_E_INVALID;
    failures += crh_reproject_frame_host(nullptr, 4, 4, &G) != CRH_E_INVALID;
    failures += crh_reproject_frame_host(&now, 4, 4, nullptr) != CRH_E_INVALID;
    failures += crh_reproject_frame_host(&now, 0, 4, &G) != CRH_E_INVALID;
    failures += crh_set_reproject(nullptr, &p) != CRH_E_INVALID;
    failures += crh_get_reproject(nullptr, &p, nullptr, nullptr) != CRH_E_INVALID;
    failures += crh_read_reprojected(nullptr, out) != CRH_E_INVALID;
    failures += crh_bench_reproject(nullptr, 1, nullptr, nullptr) != CRH_E_INVALID;
  }
  std::printf("sanitize_reproject_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
