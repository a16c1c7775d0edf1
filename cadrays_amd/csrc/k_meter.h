// k_meter.h -- part of kernels.hip (ONE translation unit: included there inside namespace crh::(anonymous), after k_ids).  Auto exposure: the display pass meters
// the image it is about to tone-map (crh_readback.cpp; the rule is DESIGN.md section 3):
//   k_luma_histogram   256-bin histogram of the pixel luminances, four bins per octave, binned on the float's bits
//   k_meter            ONE thread: exposure and white point from the histogram (meter_rule below -- the host entry point crh_meter_from_histogram runs the same function)
//   k_tonemap          (k_accumulate.h) takes the two values from the metering block instead of its arguments
// All counts are integers: the histogram does not depend on the order in which workgroups arrive.  Nothing here touches path state, queues, the accumulator or
// the counters of crh_stats.

// bin of a luminance l >= 0 (never NaN: a sum of non-negative terms): 0 for l == 0; else four bins per octave from 2^-32 on -- the lower edge of bin q is the float
// whose bits are (q + 379) << 21 (mantissa 1, 1.25, 1.5, 1.75); denormals and everything below 2^-32 fall in bin 1, +inf and everything from 1.75 x 2^31 on in bin 255
__host__ __device__ __forceinline__ uint32_t luma_bin(float l)
{
  if (l == 0.f) return 0u;
  const int q = (int)(crh_f2u(l) >> 21) - 379;
  return (uint32_t)(q < 1 ? 1 : (q > 255 ? 255 : q));
}

// The rule.  Integer sums are exact, the one division is IEEE double, one rounding to float, then the gain expression of k_tonemap: every step gives the same bits on
// the host and on the device.  N = lit pixels, mean = mean log2 luminance over the bin centres (bin i is centred at (2i - 1) / 8 - 32).
__host__ __device__ inline void meter_rule(const uint32_t* hist, const MeterRule& R, float& exposure, float& white_point, uint32_t& white_bin, uint32_t& n_lit)
{
  uint64_t N = 0, M = 0;
  for (uint32_t i = 1; i < 256u; ++i) { N += hist[i]; M += (uint64_t)hist[i] * (uint64_t)(2u * i - 1u); }
  n_lit = (uint32_t)N;
  exposure = R.exposure_in; white_point = R.white_in; white_bin = 0u;
  if (!N) return;                                        // nothing lit: the display values in force
  const double mean = (double)M / (8.0 * (double)N) - 32.0;
  double e = (double)R.key_stops - mean;
  e = e < (double)R.min_stops ? (double)R.min_stops : e;
  e = e > (double)R.max_stops ? (double)R.max_stops : e;
  exposure = (float)e;
  if (!R.white_permille) return;                         // the display white point stays
  const uint64_t target = ((uint64_t)R.white_permille * N + 999u) / 1000u;
  uint64_t run = 0; uint32_t b = 255u;
  for (uint32_t i = 1; i < 256u; ++i) { run += hist[i]; if (run >= target) { b = i; break; } }
  const float E = crh_u2f((b + 380u) << 21);            // upper edge of bin b
  white_point = crh_clamp(E * crh_exp(exposure * 0.69314718056f), R.white_min, R.white_max);
  white_bin = b;
}

// Pixels [x0, x0 + rw) x [y0, y0 + rh) of the width-wide image `src` (the host has cut the rectangle to the image).  Grid-stride, four float4 loads in flight per
// lane; one LDS histogram per wavefront, filled with LDS atomics (worst case a constant image: all 64 lanes on one word); after the barrier thread i adds the sum
// of the four copies of bin i to the block in HBM -- one atomic per non-empty bin and workgroup.  M->hist and M->n_unsampled are zero at launch.
__global__ __launch_bounds__(kBlock) void k_luma_histogram(const float4* __restrict__ src, uint32_t width, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, DMeter* __restrict__ M)
{
  __shared__ uint32_t s_h[kBlock / 64][256];
  __shared__ uint32_t s_uns;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) s_h[w][threadIdx.x] = 0u;
  if (threadIdx.x == 0) s_uns = 0u;
  __syncthreads();
  uint32_t* mine = s_h[threadIdx.x >> 6];
  const uint32_t n = rw * rh, stride = gridDim.x * kBlock;
  const bool rows = rw != width;                         // (x0 is 0 when the rectangle is as wide as the image)
  uint32_t uns = 0u;                                     // the same in every lane of a wavefront
  for (uint32_t b0 = blockIdx.x * kBlock; b0 < n; b0 += 4u * stride) {      // uniform per workgroup
    float4 a[4]; bool live[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t idx = b0 + j * stride + threadIdx.x;
      live[j] = idx < n;
      const size_t pi = rows ? (size_t)(y0 + idx / rw) * width + x0 + idx % rw : (size_t)y0 * width + idx;
      a[j] = live[j] ? src[pi] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const bool sampled = a[j].w > 0.f;                 // a NaN count is no sample either
      uns += (uint32_t)__popcll(__ballot(live[j] && !sampled));
      if (live[j] && sampled) {
        // the channels as the tone map sanitises them: NaN and everything <= 0 (-0.0 included) is 0
        const float r = a[j].x > 0.f ? a[j].x : 0.f, g = a[j].y > 0.f ? a[j].y : 0.f, b = a[j].z > 0.f ? a[j].z : 0.f;
        const float l = CRH_FMA(0.0722f, b, CRH_FMA(0.7152f, g, 0.2126f * r));      // k_tile_error's luminance
        atomicAdd(&mine[luma_bin(l)], 1u);
      }
    }
  }
  if (lane_id() == 0 && uns) atomicAdd(&s_uns, uns);
  __syncthreads();
  uint32_t sum = 0u;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) sum += s_h[w][threadIdx.x];
  if (sum) atomicAdd(&M->hist[threadIdx.x], sum);
  if (threadIdx.x == 0 && s_uns) atomicAdd(&M->n_unsampled, s_uns);
}
static_assert(kBlock == 256, "k_luma_histogram: thread i owns bin i");

// ONE thread runs the rule: 2 x 255 short dependent iterations, 16 us, most of it serial arithmetic -- bringing the bins into LDS with a whole
// workgroup first was measured and changed nothing
__global__ void k_meter(DMeter* __restrict__ M, MeterRule R)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float e, w; uint32_t wb, nl;
  meter_rule(M->hist, R, e, w, wb, nl);
  M->n_lit = nl; M->white_bin = wb; M->metered[0] = e; M->metered[1] = w;
}
