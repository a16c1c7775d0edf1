// sanitize_view_host.cpp -- the host-only side of the viewport read-out (crh_view_host, crh_view_fit, crh_view_to_frame; cadrays_amd/csrc/crh_view.cpp,
// view_kernels.h: the tap rule, the pixel rule, the exact division) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no device, no
// context, nothing loaded into an interpreter.
// Build and run:  make -C cadrays_amd/csrc sanitize-view   (links the library's own translation units, host code compiled with -fsanitize=address,undefined)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/cadrays_hip.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static crh_view_params params(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t filter)
{
  crh_view_params p; std::memset(&p, 0, sizeof p);
  p.width = w; p.height = h; p.src[0] = x0; p.src[1] = y0; p.src[2] = x1; p.src[3] = y1; p.filter = filter;
  return p;
}

int main()
{
  int failures = 0;
  // frames and views in exactly-sized heap blocks, so one byte too many -- read or written -- is seen
  const uint32_t frames[][2] = {{1, 1}, {3, 3}, {37, 23}, {64, 5}, {67, 23}, {8192, 1}, {1, 8192}};
  const uint32_t views[][2] = {{1, 1}, {37, 23}, {18, 11}, {19, 12}, {74, 46}, {53, 31}, {37, 1}, {1, 23}, {111, 5}, {8192, 1}, {1, 8192}};
  for (const auto& wh : frames) {
    const uint32_t W = wh[0], H = wh[1];
    std::vector<uint8_t> ldr(3 * (size_t)W * H), full(ldr.size(), 255);
    for (uint8_t& b : ldr) b = (uint8_t)rnd();
    const uint32_t rects[][4] = {{0, 0, 0, 0}, {0, 0, W, H}, {W - 1, H - 1, W, H}, {W / 3, H / 3, W / 3 + (W + 1) / 2, H / 3 + (H + 1) / 2}, {0, 0, 1, 1}};
    for (const auto& v : views)
      for (const auto& r : rects)
        for (uint32_t filter = 0; filter <= 3; ++filter) {
          const crh_view_params p = params(v[0], v[1], r[0], r[1], r[2], r[3], filter);
          std::vector<uint8_t> out(3 * (size_t)v[0] * v[1]);
          int rc = crh_view_host(ldr.data(), W, H, &p, out.data());
          if (rc != CRH_OK) { std::printf("view %ux%u of %ux%u -> %d\n", v[0], v[1], W, H, rc); ++failures; continue; }
          rc = crh_view_host(full.data(), W, H, &p, out.data());
          for (uint8_t b : out) if (b != 255) { std::printf("a frame of 255 gave %u\n", b); ++failures; break; }
          failures += rc != CRH_OK;
          // the mapping of the corners and of a few pixels inside: always a pixel of the rectangle
          const uint32_t x0 = r[2] ? r[0] : 0, y0 = r[2] ? r[1] : 0, x1 = r[2] ? r[2] : W, y1 = r[2] ? r[3] : H;
          for (int k = 0; k < 6; ++k) {
            const uint32_t vx = k == 0 ? 0 : k == 1 ? v[0] - 1 : rnd() % v[0], vy = k == 0 ? 0 : k == 1 ? v[1] - 1 : rnd() % v[1];
            uint32_t fx = ~0u, fy = ~0u;
            if (crh_view_to_frame(&p, W, H, vx, vy, &fx, &fy) != CRH_OK || fx < x0 || fx >= x1 || fy < y0 || fy >= y1) { std::printf("to_frame left the rectangle\n"); ++failures; }
          }
        }
    // the identity: the frame itself under every filter
    for (uint32_t filter = 0; filter <= 3; ++filter) {
      const crh_view_params p = params(W, H, 0, 0, 0, 0, filter);
      std::vector<uint8_t> out(ldr.size());
      failures += crh_view_host(ldr.data(), W, H, &p, out.data()) != CRH_OK || out != ldr;
    }
  }
  // the largest sums: an 8192-wide row of 255 reduced to one pixel, and magnified to 8192 from a 2-pixel ramp
  {
    std::vector<uint8_t> row(3 * 8192u, 255), one(3), wide(3 * 8192u), ramp = {0, 0, 0, 100, 100, 100};
    crh_view_params p = params(1, 1, 0, 0, 0, 0, CRH_VIEW_AREA);
    failures += crh_view_host(row.data(), 8192, 1, &p, one.data()) != CRH_OK || one[0] != 255 || one[2] != 255;
    p = params(8192, 1, 0, 0, 0, 0, CRH_VIEW_BILINEAR);
    failures += crh_view_host(ramp.data(), 2, 1, &p, wide.data()) != CRH_OK || wide[0] != 0 || wide[3 * 8191u] != 100;
    p = params(4, 1, 0, 0, 0, 0, CRH_VIEW_BILINEAR);
    uint8_t four[12];
    failures += crh_view_host(ramp.data(), 2, 1, &p, four) != CRH_OK || four[0] != 0 || four[3] != 25 || four[6] != 75 || four[9] != 100;
  }
  // the letterbox: both branches, the extremes
  {
    crh_view_params p;
    const uint32_t sides[] = {1, 2, 37, 360, 640, 1080, 1920, 2048, 8191, 8192};
    for (uint32_t W : sides) for (uint32_t H : sides) for (uint32_t aw : sides) for (uint32_t ah : sides) {
      if (crh_view_fit(W, H, aw, ah, &p) != CRH_OK || p.width < 1 || p.height < 1 || p.width > aw || p.height > ah || p.filter != CRH_VIEW_AUTO || p.reserved ||
          p.src[0] || p.src[1] || p.src[2] || p.src[3]) { std::printf("fit %ux%u into %ux%u -> %ux%u\n", W, H, aw, ah, p.width, p.height); ++failures; }
    }
    failures += crh_view_fit(1920, 1080, 900, 700, &p) != CRH_OK || p.width != 900 || p.height != 506;
    failures += crh_view_fit(1920, 1080, 1800, 700, &p) != CRH_OK || p.width != 1244 || p.height != 700;
  }
  // refusals walk their own paths
  {
    uint8_t ldr[3 * 6 * 4] = {0}, out[3 * 5 * 5];
    uint32_t fx, fy;
    crh_view_params ok = params(5, 5, 0, 0, 0, 0, 0), p;
    failures += crh_view_host(ldr, 6, 4, &ok, out) != CRH_OK;
    failures += crh_view_host(nullptr, 6, 4, &ok, out) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 6, 4, nullptr, out) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 6, 4, &ok, nullptr) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 0, 4, &ok, out) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 6, 0, &ok, out) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 8193, 4, &ok, out) != CRH_E_INVALID;
    failures += crh_view_host(ldr, 6, 8193, &ok, out) != CRH_E_INVALID;
    const crh_view_params bad[] = {params(0, 5, 0, 0, 0, 0, 0), params(5, 0, 0, 0, 0, 0, 0), params(8193, 5, 0, 0, 0, 0, 0), params(5, 8193, 0, 0, 0, 0, 0),
                                   params(5, 5, 2, 1, 2, 3, 0), params(5, 5, 1, 3, 4, 3, 0), params(5, 5, 4, 1, 2, 3, 0), params(5, 5, 0, 0, 7, 4, 0),
                                   params(5, 5, 0, 0, 6, 5, 0), params(5, 5, 6, 0, 9, 4, 0), params(5, 5, 0, 0, 0, 3, 0), params(5, 5, 0xFFFFFFFFu, 0, 1, 1, 0),
                                   params(5, 5, 0, 0, 0, 0, 4), params(5, 5, 0, 0, 0, 0, 0xFFFFFFFFu)};
    for (const crh_view_params& b : bad) {
      failures += crh_view_host(ldr, 6, 4, &b, out) != CRH_E_INVALID;
      failures += crh_view_to_frame(&b, 6, 4, 0, 0, &fx, &fy) != CRH_E_INVALID;
    }
    p = ok; p.reserved = 1;
    failures += crh_view_host(ldr, 6, 4, &p, out) != CRH_E_INVALID;
    failures += crh_view_to_frame(&p, 6, 4, 0, 0, &fx, &fy) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 6, 4, 4, 4, &fx, &fy) != CRH_OK || fx != 5 || fy != 3;
    failures += crh_view_to_frame(nullptr, 6, 4, 0, 0, &fx, &fy) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 6, 4, 0, 0, nullptr, &fy) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 6, 4, 0, 0, &fx, nullptr) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 6, 4, 5, 0, &fx, &fy) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 6, 4, 0, 5, &fx, &fy) != CRH_E_INVALID;
    failures += crh_view_to_frame(&ok, 0, 4, 0, 0, &fx, &fy) != CRH_E_INVALID;
    failures += crh_view_fit(6, 4, 10, 10, nullptr) != CRH_E_INVALID;
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t v : {0u, 8193u}) {
        uint32_t a[4] = {6, 4, 10, 10}; a[k] = v;
        failures += crh_view_fit(a[0], a[1], a[2], a[3], &p) != CRH_E_INVALID;
      }
    // the calls on a context refuse a null context before anything else
    failures += crh_read_view(nullptr, &ok, out) != CRH_E_INVALID;
    failures += crh_read_view_begin(nullptr, &ok) != CRH_E_INVALID;
    failures += crh_read_view_end(nullptr, out) != CRH_E_INVALID;
    float ms;
    failures += crh_bench_view(nullptr, &ok, 1, &ms) != CRH_E_INVALID;
  }
  std::printf("sanitize_view_host: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
