// k_ids.h -- part of kernels.hip (ONE translation unit: included there inside namespace crh::(anonymous), after k_accumulate).  The first-hit id buffer behind
// crh_pick / crh_read_ids and the hover / selection overlay of the LDR read-out (crh_pick.cpp):
//   k_first_hit_rays     the pixel-centre camera ray of every pixel (or of a caller's pixel list: crh_camera_rays), 8 floats each in crh_trace_nearest's layout
//   k_trace_rays<false, false, TWO>   (k_packets.h, unchanged) traces them: the engine, the split-scene walk and the disabled records are crh_trace_nearest's
//   k_first_hit_resolve  {t, u, v, triangle} from block order to row-major pixel order + the object of the triangle
//   k_overlay            outline / interior tint of the selected and the hovered objects over the tone-mapped bytes
// Nothing here draws from the RNG or touches path state, queues, the accumulator or the counters of crh_stats.

#include "k_pixel_ray.h"      // pixel_centre_ray: the pixel-centre camera ray, shared with reproject_kernels.hip

// Ray slot <-> pixel of the id pass: 8x8-pixel blocks, row-major over ceil(W/8) x ceil(H/8), so that one wavefront of the traversal kernel owns one block
// (slot_pixel's mapping inside a tile, without the tiles: the id buffer is never sharded).  Slots of a partial block that fall outside the image repeat the
// nearest edge pixel: an ordinary ray whose answer k_first_hit_resolve drops.
__device__ __forceinline__ bool ids_slot_pixel(uint32_t slot, uint32_t W, uint32_t H, uint32_t& px, uint32_t& py)
{
  const uint32_t bx = (W + 7u) >> 3, blk = slot >> 6, l = slot & 63u;
  px = (blk % bx) * 8u + (l & 7u);
  py = (blk / bx) * 8u + (l >> 3);
  return px < W && py < H;
}

// xy == nullptr: ray `i` belongs to slot i of the whole target (n = 64 * blocks); else to pixel (xy[2i], xy[2i+1]) -- validated by the host
__global__ __launch_bounds__(kBlock) void k_first_hit_rays(DScene S, const uint32_t* __restrict__ xy, uint32_t n, float4* __restrict__ rays)
{
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    uint32_t px, py;
    if (xy) { px = xy[2u * i]; py = xy[2u * i + 1u]; }
    else { ids_slot_pixel(i, S.width, S.height, px, py); px = min(px, S.width - 1u); py = min(py, S.height - 1u); }
    v3 o, d;
    pixel_centre_ray(S, px, py, o, d);
    rays[2u * i] = mk4(o, CRH_MAXFLOAT);
    rays[2u * i + 1u] = mk4(d, 0.f);
  }
}

// hit_slot: what k_trace_rays wrote per slot, {t, u, v, caller's triangle index as int bits (-1: miss, t = tmax)}.  tri_obj == nullptr: a scene handed over without
// objects -- every hit is object 0.
__global__ __launch_bounds__(kBlock) void k_first_hit_resolve(uint32_t W, uint32_t H, uint32_t n_slots, const float4* __restrict__ hit_slot, const int32_t* __restrict__ tri_obj,
                                                               uint32_t n_tri_obj, float4* __restrict__ hit_px, int32_t* __restrict__ obj_px)
{
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_slots; i += gridDim.x * kBlock) {
    uint32_t px, py;
    if (!ids_slot_pixel(i, W, H, px, py)) continue;
    const float4 h = hit_slot[i];
    const int tri = __float_as_int(h.w);
    const int32_t ob = tri < 0 ? -1 : (tri_obj ? ((uint32_t)tri < n_tri_obj ? tri_obj[tri] : -1) : 0);
    const uint32_t p = py * W + px;
    hit_px[p] = h;
    obj_px[p] = ob;
  }
}

// Hover / selection overlay over the tone-mapped RGB8 frame; integer arithmetic only (tests restate it in numpy).  A pixel is MARKED for a set when its object is in
// the set; a marked pixel is an OUTLINE pixel when it lies on the image border or one of its 4 neighbours is not marked for the same set; outline pixels take the
// set's colour, other marked pixels (ldr * (256 - a) + colour * a + 128) >> 8.  The selection first, the hovered object second.  Neighbour ids come straight from the
// object plane (4 B per pixel, read only by marked pixels, rows adjacent in L2): at 1080p the whole kernel moves ~14 MB, an LDS tile with an apron would save
// at most the 4 neighbour reads of the marked pixels.
struct OverlaySet { const uint8_t* flags; uint32_t n_flags; int32_t one; uint32_t r, g, b, a; };      // flags == nullptr: the set is the single object `one` (-1: empty)
__device__ __forceinline__ bool overlay_marked(const OverlaySet& s, int32_t ob)
{
  if (ob < 0) return false;
  return s.flags ? ((uint32_t)ob < s.n_flags && s.flags[ob] != 0) : ob == s.one;
}
__device__ __forceinline__ void overlay_apply(const OverlaySet& s, const int32_t* __restrict__ obj, uint32_t W, uint32_t H, uint32_t px, uint32_t py, uint32_t c[3])
{
  const uint32_t i = py * W + px;
  if (!overlay_marked(s, obj[i])) return;
  const bool outline = px == 0u || py == 0u || px == W - 1u || py == H - 1u || !overlay_marked(s, obj[i - 1u]) || !overlay_marked(s, obj[i + 1u]) ||
                       !overlay_marked(s, obj[i - W]) || !overlay_marked(s, obj[i + W]);
  const uint32_t col[3] = {s.r, s.g, s.b};
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = outline ? col[k] : (c[k] * (256u - s.a) + col[k] * s.a + 128u) >> 8;
}
__global__ __launch_bounds__(kBlock) void k_overlay(uint8_t* __restrict__ ldr, const int32_t* __restrict__ obj, uint32_t W, uint32_t H, OverlaySet sel, OverlaySet hov)
{
  const uint32_t n = W * H;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const int32_t ob = obj[i];
    const bool ms = overlay_marked(sel, ob), mh = overlay_marked(hov, ob);
    if (!ms && !mh) continue;
    const uint32_t px = i % W, py = i / W;
    uint32_t c[3] = {ldr[3u * i], ldr[3u * i + 1u], ldr[3u * i + 2u]};
    if (ms) overlay_apply(sel, obj, W, H, px, py, c);
    if (mh) overlay_apply(hov, obj, W, H, px, py, c);
    ldr[3u * i] = (uint8_t)c[0]; ldr[3u * i + 1u] = (uint8_t)c[1]; ldr[3u * i + 2u] = (uint8_t)c[2];
  }
}
