// fit_kernels.hip -- the one pass over the vertices behind crh_fit_view (crh_fit.cpp): six maxima and a vertex count per object, for gfx950, and the host twin.
// (reference: V3d_View::FitAll / ZFitAll as the application drives them, src/Launcher/AppViewer.cxx:704, 764-767, 788, 886)
//
// A translation unit of its own: nothing here is part of kernels.hip, whose object code stays what it is.  Plain float32, NO CRH_FMA anywhere (fit_kernels.h):
// every value is a maximum of per-vertex values that do not depend on the order of arrival, so the device, the host twin and a numpy restatement agree bit for bit.
#include "fit_kernels.h"

namespace crh {
namespace {

constexpr int kFitBlock = 256;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Add maxima and a count to a record.  Every wavefront of the grid ends up here with the SAME few addresses, and atomics on one address are served one
// after the other (measured: 4096 wavefronts x 7 atomics = 0.33 ms of a 0.35 ms pass over 3 M vertices), so a maximum is sent only where it would raise what
// the record holds -- a plain look first; the keys only grow, so a stale look can cost an atomic that changes nothing and never loses one.
__device__ __forceinline__ void fit_merge(uint32_t* __restrict__ r, const uint32_t k[6], uint32_t cnt)
{
#pragma unroll
  for (int j = 0; j < 6; ++j)
    if (k[j] > __hip_atomic_load(&r[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&r[j], k[j]);
  atomicAdd(&r[6], cnt);
}

// lane 0 of the wavefront adds the wavefront's running maxima (the same in every lane) to the record of object `ob`
__device__ __forceinline__ void fit_flush(uint32_t* __restrict__ rec, int ob, const uint32_t k[6], uint32_t cnt)
{
  if (ob < 0 || !cnt || (threadIdx.x & 63u)) return;
  fit_merge(rec + (size_t)kFitRec * (uint32_t)ob, k, cnt);
}

// Grid-stride, one vertex per lane per round; the loop bounds are the same for every lane of a wavefront, so the cross-lane operations always see all 64 lanes.
// A lane that contributes nothing (tail, unreferenced vertex, object not wanted) holds key 0 = "no vertex", the identity of the key maximum.
//   all contributing lanes of the wavefront hold ONE object (an object's vertices are contiguous: the normal case): __shfl_xor reduction, the result joins the
//     wavefront's running maxima in registers; they go to the record (fit_merge) only when the object changes and at the end -- where the four wavefronts of
//     the workgroup first meet in LDS, so that one object costs one count atomic per workgroup;
//   otherwise (the wavefront straddles objects): fit_merge per contributing lane.
// Maxima of keys and a sum of integers: the record does not depend on which branch ran.
__global__ __launch_bounds__(kFitBlock) void k_fit_extents(const float4* __restrict__ verts, uint32_t n, const FitObject* __restrict__ objs, uint32_t n_objects, FitFrame F,
                                                           uint32_t* __restrict__ rec)
{
  const uint32_t lane = threadIdx.x & 63u, wave0 = blockIdx.x * kFitBlock + (threadIdx.x & ~63u), stride = gridDim.x * kFitBlock;
  int cur = -1; uint32_t run[6] = {0u, 0u, 0u, 0u, 0u, 0u}, run_n = 0u;      // the same in every lane
  for (uint64_t base = wave0; base < n; base += stride) {                    // (64 bits: base + stride may pass 2^32)
    const uint64_t i = base + lane;
    int ob = -1; uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (i < n) {
      const float4 v = verts[i];
      const int o = (int)crh_f2u(v.w);
      if (o >= 0 && (uint32_t)o < n_objects && objs[o].on) {
        float e[6];
        fit_vertex(objs[o].m, v.x, v.y, v.z, F, e);
#pragma unroll
        for (int j = 0; j < 6; ++j) k[j] = fit_key(e[j]);
        ob = o;
      }
    }
    const unsigned long long live = __ballot(ob >= 0);
    if (!live) continue;
    const int first = __shfl(ob, __ffsll(live) - 1);
    if (!__ballot(ob >= 0 && ob != first)) {
      if (first != cur) {
        fit_flush(rec, cur, run, run_n);
        cur = first; run_n = 0u;
#pragma unroll
        for (int j = 0; j < 6; ++j) run[j] = 0u;
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        uint32_t m = k[j];
        for (int off = 32; off > 0; off >>= 1) m = umax(m, (uint32_t)__shfl_xor((int)m, off));
        run[j] = umax(run[j], m);
      }
      run_n += (uint32_t)__popcll(live);
    } else if (ob >= 0) {
      fit_merge(rec + (size_t)kFitRec * (uint32_t)ob, k, 1u);
    }
  }
  // the end: every thread arrives here (the loops above have no early exit).  Each wavefront leaves its running maxima in LDS; thread 0 folds neighbours that
  // hold the same object into one and sends what is left.
  __shared__ uint32_t s_run[kFitBlock / 64][8];
  if (lane == 0u) {
    uint32_t* mine = s_run[threadIdx.x >> 6];
#pragma unroll
    for (int j = 0; j < 6; ++j) mine[j] = run[j];
    mine[6] = run_n; mine[7] = (uint32_t)cur;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  int ob = -1; uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u}, cnt = 0u;
  for (int w = 0; w < kFitBlock / 64; ++w) {
    const uint32_t* theirs = s_run[w];
    if (!theirs[6]) continue;
    if ((int)theirs[7] != ob) {
      fit_flush(rec, ob, k, cnt);
      ob = (int)theirs[7]; cnt = 0u;
#pragma unroll
      for (int j = 0; j < 6; ++j) k[j] = 0u;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) k[j] = umax(k[j], theirs[j]);
    cnt += theirs[6];
  }
  fit_flush(rec, ob, k, cnt);
}

}  // namespace

void launch_fit_extents(hipStream_t stream, int grid, const float4* verts, uint32_t n, const FitObject* objs, uint32_t n_objects, const FitFrame& F, uint32_t* rec)
{
  if (!n || !n_objects) return;
  const uint64_t need = ((uint64_t)n + kFitBlock - 1) / kFitBlock;
  const uint32_t g = (uint32_t)(need < (uint64_t)(grid > 0 ? grid : 1) ? need : (uint64_t)(grid > 0 ? grid : 1));
  hipLaunchKernelGGL(k_fit_extents, dim3(g), dim3(kFitBlock), 0, stream, verts, n, objs, n_objects, F, rec);
}

void fit_extents_host(const float* verts4, uint32_t n, const FitObject* objs, uint32_t n_objects, const FitFrame& F, uint32_t* rec)
{
  for (uint32_t i = 0; i < n; ++i) {
    const float* v = verts4 + 4 * (size_t)i;
    const int o = (int)crh_f2u(v[3]);
    if (o < 0 || (uint32_t)o >= n_objects || !objs[o].on) continue;
    float e[6];
    fit_vertex(objs[o].m, v[0], v[1], v[2], F, e);
    uint32_t* r = rec + (size_t)kFitRec * (uint32_t)o;
    for (int j = 0; j < 6; ++j) { const uint32_t k = fit_key(e[j]); if (k > r[j]) r[j] = k; }
    ++r[6];
  }
}

}  // namespace crh
