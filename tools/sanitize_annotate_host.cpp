// sanitize_annotate_host.cpp -- the host-only side of the annotations (crh_annot_project_host, crh_annot_draw_host; cadrays_amd/csrc/crh_annotate.cpp,
// annotate_kernels.h: the projection, the pixel rule, the composite) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no
// context, nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-annotate   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)(rnd() % 20001u) * 1e-4f - 1.0f; }

struct Rec { float x0, y0, x1, y1, q0, q1; uint32_t flags, pad; };

static crh_camera camera(bool ortho, float fov)
{
  crh_camera c; std::memset(&c, 0, sizeof c);
  c.eye[0] = 0.25f; c.eye[1] = -3.0f; c.eye[2] = 0.5f;
  c.dir[0] = 0.3f; c.dir[1] = 1.0f; c.dir[2] = -0.2f;
  c.up[2] = 1.0f; c.fovy_deg = fov; c.is_ortho = ortho ? 1 : 0; c.ortho_scale = 1.5f; c.focal_dist = 1.0f;
  return c;
}

int main()
{
  int failures = 0;
  const float extremes[] = {0.f, -0.f, 1e-45f, -1e-45f, 1e-38f, 1.f, -1.f, 3e38f, -3e38f, 1e20f, -1e20f};
  const uint32_t nE = sizeof extremes / sizeof extremes[0];
  const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {16, 16}, {67, 45}, {130, 70}};
  for (bool ortho : {false, true})
    for (float fov : {1.0f, 45.0f, 170.0f})
      for (const auto& wh : sizes)
        for (uint32_t n : {0u, 1u, 33u, 257u}) {
          const uint32_t W = wh[0], H = wh[1];
          const size_t px = (size_t)W * H;
          const crh_camera cam = camera(ortho, fov);
          // exactly-sized heap blocks, so one byte too many is seen
          std::vector<crh_annot_segment> segs(n);
          for (uint32_t i = 0; i < n; ++i) {
            crh_annot_segment& s = segs[i];
            for (int k = 0; k < 3; ++k) {
              s.a[k] = i % 3u == 0u ? extremes[rnd() % nE] : rndf() * 4.0f;
              s.b[k] = i % 5u == 0u ? s.a[k] : (i % 7u == 0u ? extremes[rnd() % nE] : s.a[k] + rndf());
              s.rgb[k] = (uint8_t)rnd();
            }
            s.alpha = (uint8_t)rnd();
            s.style = CRH_ANNOT_STYLE(1u + rnd() % 8u, rnd() % 3u);
          }
          std::vector<Rec> rec(n);
          if (crh_annot_project_host(&cam, W, H, segs.data(), n, rec.data()) != CRH_OK) { std::printf("project %ux%u n %u -> error\n", W, H, n); ++failures; continue; }
          for (const Rec& r : rec) {
            if (r.flags > 1u || r.pad) { std::printf("a record with unknown flags\n"); ++failures; break; }
            if (!r.flags) continue;
            const bool inside = r.x0 >= -(float)W && r.x0 <= 2.f * W && r.x1 >= -(float)W && r.x1 <= 2.f * W && r.y0 >= -(float)H && r.y0 <= 2.f * H && r.y1 >= -(float)H && r.y1 <= 2.f * H;
            if (!inside || !std::isfinite(r.q0) || !std::isfinite(r.q1)) { std::printf("a valid record outside the guard band or with a depth that is not finite\n"); ++failures; break; }
          }
          // an unaligned record block and an unaligned list are the caller's right
          std::vector<unsigned char> raw_rec(sizeof(Rec) * n + 1), raw_seg(sizeof(crh_annot_segment) * n + 1);
          if (n) std::memcpy(raw_seg.data() + 1, segs.data(), sizeof(crh_annot_segment) * n);
          failures += crh_annot_project_host(&cam, W, H, reinterpret_cast<const crh_annot_segment*>(raw_seg.data() + 1), n, raw_rec.data() + 1) != CRH_OK;
          failures += n && std::memcmp(raw_rec.data() + 1, rec.data(), sizeof(Rec) * n) != 0;
          std::vector<float> rays(8 * px), t(px);
          for (size_t i = 0; i < px; ++i) {
            for (int k = 0; k < 8; ++k) rays[8 * i + k] = rndf();
            t[i] = rnd() % 4u == 0u ? 1e15f : (float)(rnd() % 60u) * 0.1f;     // misses, zero and equal distances
          }
          std::vector<uint8_t> ldr(3 * px), ldr2; std::vector<int32_t> ids(px), ids2(px);
          for (uint8_t& b : ldr) b = (uint8_t)rnd();
          ldr2 = ldr;
          crh_annot_params p; crh_annot_defaults(&p);
          if (crh_annot_draw_host(rec.data(), segs.data(), n, &p, &cam, W, H, rays.data(), t.data(), ldr.data(), ids.data()) != CRH_OK) { std::printf("draw %ux%u n %u -> error\n", W, H, n); ++failures; continue; }
          failures += crh_annot_draw_host(raw_rec.data() + 1, reinterpret_cast<const crh_annot_segment*>(raw_seg.data() + 1), n, nullptr, &cam, W, H, rays.data(), t.data(), ldr2.data(), ids2.data()) != CRH_OK;
          failures += ldr != ldr2 || ids != ids2;
          for (int32_t s : ids) if (s < -1 || s >= (int32_t)n) { std::printf("an id outside the list\n"); ++failures; break; }
          failures += crh_annot_draw_host(rec.data(), segs.data(), n, &p, &cam, W, H, rays.data(), t.data(), nullptr, ids2.data()) != CRH_OK || ids != ids2;
          p.depth_bias = 3e38f; p.hidden_alpha = 0u;
          failures += crh_annot_draw_host(rec.data(), segs.data(), n, &p, &cam, W, H, rays.data(), t.data(), ldr2.data(), nullptr) != CRH_OK;
        }
  // refusals walk their own paths
  {
    const crh_camera cam = camera(false, 45.f);
    crh_annot_segment s; std::memset(&s, 0, sizeof s); s.b[1] = 1.f; s.style = CRH_ANNOT_STYLE(1u, CRH_ANNOT_ON_TOP);
    Rec r; uint8_t ldr[12] = {0}; int32_t ids[4]; float rays[32] = {0}, t[4] = {1.f, 2.f, 1e15f, 3.f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    failures += crh_annot_project_host(&cam, 2, 2, &s, 1, &r) != CRH_OK;
    failures += crh_annot_project_host(nullptr, 2, 2, &s, 1, &r) != CRH_E_INVALID;
    failures += crh_annot_project_host(&cam, 0, 2, &s, 1, &r) != CRH_E_INVALID;
    failures += crh_annot_project_host(&cam, 2, 0, &s, 1, &r) != CRH_E_INVALID;
    failures += crh_annot_project_host(&cam, 2, 2, nullptr, 1, &r) != CRH_E_INVALID;
    failures += crh_annot_project_host(&cam, 2, 2, &s, 1, nullptr) != CRH_E_INVALID;
    failures += crh_annot_project_host(&cam, 2, 2, nullptr, 0, nullptr) != CRH_OK;
    for (uint32_t style : {0u, 9u, 15u, 0x301u, 0x401u, 0x11u, 0x80000001u}) { crh_annot_segment q = s; q.style = style; failures += crh_annot_project_host(&cam, 2, 2, &q, 1, &r) != CRH_E_INVALID; }
    for (float v : {nan, inf, -inf}) { crh_annot_segment q = s; q.a[2] = v; failures += crh_annot_project_host(&cam, 2, 2, &q, 1, &r) != CRH_E_INVALID; q = s; q.b[0] = v; failures += crh_annot_draw_host(&r, &q, 1, nullptr, &cam, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID; }
    failures += crh_annot_draw_host(&r, &s, 1, nullptr, &cam, 2, 2, nullptr, nullptr, ldr, ids) != CRH_OK;
    failures += crh_annot_draw_host(&r, &s, 1, nullptr, &cam, 2, 2, nullptr, nullptr, nullptr, nullptr) != CRH_E_INVALID;
    failures += crh_annot_draw_host(nullptr, &s, 1, nullptr, &cam, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID;
    failures += crh_annot_draw_host(&r, nullptr, 1, nullptr, &cam, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID;
    failures += crh_annot_draw_host(&r, &s, 1, nullptr, nullptr, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID;
    failures += crh_annot_draw_host(&r, &s, 1, nullptr, &cam, 0, 2, rays, t, ldr, ids) != CRH_E_INVALID;
    crh_annot_segment hid = s; hid.style = CRH_ANNOT_STYLE(2u, CRH_ANNOT_HIDE);
    failures += crh_annot_draw_host(&r, &hid, 1, nullptr, &cam, 2, 2, nullptr, t, ldr, ids) != CRH_E_INVALID;      // depth asked for, no planes
    failures += crh_annot_draw_host(&r, &hid, 1, nullptr, &cam, 2, 2, rays, nullptr, ldr, ids) != CRH_E_INVALID;
    failures += crh_annot_draw_host(&r, &hid, 1, nullptr, &cam, 2, 2, rays, t, ldr, ids) != CRH_OK;
    for (float bias : {-1e-6f, nan, inf}) { crh_annot_params p; crh_annot_defaults(&p); p.depth_bias = bias; failures += crh_annot_draw_host(&r, &s, 1, &p, &cam, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID; }
    { crh_annot_params p; crh_annot_defaults(&p); p.hidden_alpha = 256u; failures += crh_annot_draw_host(&r, &s, 1, &p, &cam, 2, 2, rays, t, ldr, ids) != CRH_E_INVALID; }
    crh_annot_defaults(nullptr);
    failures += crh_set_annotations(nullptr, &s, 1, nullptr) != CRH_E_INVALID;
    failures += crh_get_annotations(nullptr, nullptr, 0, nullptr, nullptr, nullptr) != CRH_E_INVALID;
    failures += crh_read_annotation_ids(nullptr, ids) != CRH_E_INVALID;
    failures += crh_pick_annotation(nullptr, 0, 0, nullptr, nullptr) != CRH_E_INVALID;
    failures += crh_read_annotation_records(nullptr, &r) != CRH_E_INVALID;
    failures += crh_bench_annotations(nullptr, 1, nullptr, nullptr, nullptr) != CRH_E_INVALID;
  }
  std::printf("sanitize_annotate_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
