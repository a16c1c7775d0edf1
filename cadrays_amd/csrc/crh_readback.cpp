// crh_readback.cpp -- HDR / LDR read-back (synchronous and asynchronous), accumulator checkpoints, statistics, kernel timing
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include "crh_context.h"
#include "view_kernels.h"

using namespace crh;
using namespace crh::api;

// ---- auto exposure (crh_set_auto_exposure): the metering in front of an LDR read-out's tone map.  Block 0 belongs to the synchronous read-out, 1 / 2 to the two
// read-back slots, 3 to crh_measure_exposure.
static bool meter_params_ok(const crh_meter_params* p)
{
  const float f[] = {p->key_stops, p->min_stops, p->max_stops, p->white_min, p->white_max};
  return all_finite(f, sizeof f / sizeof f[0]) && p->min_stops <= p->max_stops && p->white_min <= p->white_max && p->white_permille <= 1000u;
}
static MeterRule meter_rule_of(const crh_meter_params& p, float exposure_in, float white_in)
{
  return MeterRule{p.key_stops, p.min_stops, p.max_stops, p.white_permille, p.white_min, p.white_max, exposure_in, white_in};
}
// memset + k_luma_histogram + k_meter on L.stream over the image the tone map is about to read; the rectangle is cut to the target, an empty one is the whole frame
static void meter_image(crh_ctx* c, const Launch& L, const float4* src, const crh_meter_params& p, DMeter* block)
{
  const uint32_t W = c->par.width, H = c->par.height;
  uint32_t x0 = std::min(p.rect[0], W), y0 = std::min(p.rect[1], H), x1 = std::min(p.rect[2], W), y1 = std::min(p.rect[3], H);
  if (x1 <= x0 || y1 <= y0) { x0 = 0; y0 = 0; x1 = W; y1 = H; }
  launch_meter(L, src, W, x0, y0, x1 - x0, y1 - y0, meter_rule_of(p, c->par.exposure, c->par.white_point), block);
}
// what launch_tonemap takes as `metered`: nullptr (auto exposure off: the code path and bytes of a context that never heard of it) or the block just filled
static const float* meter_in_front(crh_ctx* c, const Launch& L, const float4* src, int block)
{
  if (!c->meter_on || !c->d_meter) return nullptr;
  meter_image(c, L, src, c->meter_par, c->d_meter + block);
  return c->d_meter[block].metered;
}
static int ensure_meter_blocks(crh_ctx* c)
{
  if (c->d_meter) return CRH_OK;
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(c->d_meter.reserve(4));
  return CRH_OK;
}

// THE DISPLAY CHAIN: everything between the image a read-out shows and the RGB8 bytes at d_ldr, enqueued on L.stream -- the one place where a
// display feature is inserted.  `set`: the scratch images of the denoise filter and the reprojection (0: the context's stream, 1: the read-back stream); `block`: the
// metering block.  The caller owns the stream: nothing here calls cstream().
namespace crh {
namespace api {

int enqueue_display_chain(crh_ctx* c, const Launch& L, int set, int block, uint8_t* d_ldr)
{
  const uint32_t n = c->par.width * c->par.height;
  const uint32_t ts = c->par.tile_size, n_tiles = ((c->par.width + ts - 1) / ts) * ((c->par.height + ts - 1) / ts);
  const bool tiles = c->show_tiles && c->adaptive && c->picked_valid && c->d_picked.cap() >= n_tiles;      // ShowSamplingTiles: d_picked was written by the device-side tile draw of the last iteration
  const float4* src = display_source(c);
  const float* metered = meter_in_front(c, L, src, block);                // auto exposure meters the UNFILTERED image ...
  const float4* shown;
  if (int rc = reproject_src(c, L.stream, src, set, &shown)) return rc;   // ... reprojected display history (crh_reproject.cpp) and ...
  if (int rc = denoise_src(c, L.stream, shown, set, &shown)) return rc;   // ... the denoised display (crh_denoise.cpp): `src` itself, and nothing at all, while the feature is off
  launch_tonemap(L, shown, d_ldr, n, c->par.tonemap_mode, c->par.exposure, c->par.white_point, c->spec.display_gamma22, tiles ? c->d_picked : nullptr, c->par.width, ts, metered);
  if (int rc = outline_ldr(c, L.stream, d_ldr)) return rc;                // feature lines (crh_outline.cpp): nothing at all while the feature is off
  if (int rc = overlay_ldr(c, L.stream, d_ldr)) return rc;                // hover / selection (crh_pick.cpp): nothing at all when neither is set
  return annotate_ldr(c, L.stream, set, d_ldr);                           // annotations (crh_annotate.cpp): LAST, and nothing at all while there is no list
}

// Asynchronous read-back of the frame as submitted so far -- LDR (tone-mapped RGB8), HDR (linear float RGB) or a VIEW of the LDR frame (crh_view.cpp: the frame goes
// to the scratch image of set 1 and the slot receives its resample): display chain / unpack + device-to-host copy run on a stream of their own into one of two
// device / pinned-host buffer pairs while the next Redraw()s are already rendering; only the NEXT accumulate waits (for the kernels that read the accumulator: rb_tm
// is recorded BEHIND the chain and IN FRONT of a view's resample, which reads the scratch image only), nothing else does.
int read_begin(crh_ctx* c, ReadKind kind, const ViewPlan* view)
{
  if (!c || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  if (c->rb_outstanding >= 2) return fail(c, CRH_E_INVALID, "two read-backs are already in flight (crh_read_ldr_end / crh_read_hdr_end / crh_read_view_end first)");
  CRH_HIP(hipSetDevice(c->device));
  const uint32_t n = c->par.width * c->par.height;
  const bool resample = kind == kReadView && view && !view->identity;
  const size_t bytes = resample ? 3 * (size_t)view->X.v * view->Y.v : (kind == kReadHdr ? 12 : 3) * (size_t)n;
  if (!c->rb_stream) {
    CRH_HIP(hipStreamCreateWithFlags(&c->rb_stream, hipStreamNonBlocking));
    CRH_HIP(hipEventCreateWithFlags(&c->rb_fork, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) { CRH_HIP(hipEventCreateWithFlags(&c->rb_tm[k], hipEventDisableTiming)); CRH_HIP(hipEventCreateWithFlags(&c->rb_done[k], hipEventDisableTiming)); }
  }
  if (bytes > c->d_rb[0].cap() || bytes > c->h_rb[0].cap() || bytes > c->d_rb[1].cap() || bytes > c->h_rb[1].cap()) {
    CRH_HIP(hipStreamSynchronize(c->rb_stream));
    if (c->rb_outstanding) return fail(c, CRH_E_INVALID, "the read-back buffers must grow while a read-back is in flight (crh_read_*_end first)");
    for (int k = 0; k < 2; ++k) { CRH_HIP(c->d_rb[k].release()); CRH_HIP(c->h_rb[k].release()); }
    for (int k = 0; k < 2; ++k) { CRH_HIP(c->d_rb[k].reserve(bytes)); CRH_HIP(c->h_rb[k].reserve(bytes)); }
  }
  if (resample) if (int rc = grow_display_scratch(c, 1, &c->d_vw_full[1], 1, 3 * (size_t)n)) return rc;
  const uint32_t slot = c->rb_head & 1u;
  // everything submitted so far comes first: the frames in flight on the pipeline streams (not joined, they stay in flight) and
  // whatever sits on the context's stream
  for (int k = 0; k < 8; ++k) if (c->pipe.pipe_pending[k]) CRH_HIP(hipStreamWaitEvent(c->rb_stream, c->lane_join[k], 0));
  CRH_HIP(hipEventRecord(c->rb_fork, c->stream_));
  CRH_HIP(hipStreamWaitEvent(c->rb_stream, c->rb_fork, 0));
  Launch L{c->rb_stream, c->grid, false};
  if (kind == kReadHdr) launch_hdr(L, display_source(c), c->d_rb[slot].as<float>(), n);
  else if (int rc = enqueue_display_chain(c, L, 1, 1 + (int)slot, resample ? c->d_vw_full[1] : c->d_rb[slot])) return rc;      // rb_tm below covers every read of the accumulator, the history and the guide
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipEventRecord(c->rb_tm[slot], c->rb_stream));
  if (resample) if (int rc = view_resample(c, c->rb_stream, c->d_vw_full[1], *view, c->d_rb[slot])) return rc;
  CRH_HIP(hipMemcpyAsync(c->h_rb[slot], c->d_rb[slot], bytes, hipMemcpyDeviceToHost, c->rb_stream));
  CRH_HIP(hipEventRecord(c->rb_done[slot], c->rb_stream));
  c->rb_bytes[slot] = bytes; c->rb_kind[slot] = kind;
  c->rb_guard = c->rb_tm[slot]; c->rb_guard_pending = true;
  ++c->rb_head; ++c->rb_outstanding;
  return CRH_OK;
}

int read_end(crh_ctx* c, void* out, ReadKind kind)
{
  if (!c || !out) return fail(c, CRH_E_INVALID, "null output");
  if (!c->rb_outstanding) return fail(c, CRH_E_INVALID, "no read-back in flight (crh_read_*_begin first)");
  CRH_HIP(hipSetDevice(c->device));
  const uint32_t slot = (c->rb_head - c->rb_outstanding) & 1u;          // the oldest one
  if (c->rb_kind[slot] != kind) return fail(c, CRH_E_INVALID, "the oldest read-back in flight is of another kind (LDR / HDR / view): end it with its own call");
  CRH_HIP(hipEventSynchronize(c->rb_done[slot]));
  std::memcpy(out, c->h_rb[slot], c->rb_bytes[slot]);
  --c->rb_outstanding;
  return CRH_OK;
}

}  // namespace api
}  // namespace crh

extern "C" {

int crh_read_hdr(crh_ctx* c, float* out)
{
  if (c) c->read_since_render = true;
  if (!c || !out || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator / null output");
  CRH_HIP(hipSetDevice(c->device));
  const uint32_t n = c->par.width * c->par.height;
  CRH_HIP(c->d_scratch.reserve(sizeof(float) * 3 * (size_t)n));
  Launch L{cstream(c), c->grid, false};
  launch_hdr(L, display_source(c), c->d_scratch.as<float>(), n);
  CRH_HIP(hipMemcpyAsync(out, c->d_scratch, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  return CRH_OK;
}

int crh_read_ldr(crh_ctx* c, uint8_t* out)
{
  if (c) c->read_since_render = true;
  if (!c || !out || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator / null output");
  CRH_HIP(hipSetDevice(c->device));
  const size_t bytes = 3 * (size_t)c->par.width * c->par.height;
  CRH_HIP(c->d_scratch.reserve(bytes));
  Launch L{cstream(c), c->grid, false};
  if (int rc = enqueue_display_chain(c, L, 0, 0, c->d_scratch.as<uint8_t>())) return rc;
  CRH_HIP(hipMemcpyAsync(out, c->d_scratch, bytes, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  return CRH_OK;
}

int crh_read_ldr_begin(crh_ctx* c) { return read_begin(c, kReadLdr, nullptr); }
int crh_read_ldr_end(crh_ctx* c, uint8_t* out) { return read_end(c, out, kReadLdr); }
int crh_read_hdr_begin(crh_ctx* c) { return read_begin(c, kReadHdr, nullptr); }
int crh_read_hdr_end(crh_ctx* c, float* out) { return read_end(c, out, kReadHdr); }

// ---- display state without a restart, auto exposure (reference: the exposure / white point sliders and the tone-mapping combo only write fields the display pass
// reads, SettingsWidget.cxx:343-404).  None of these calls do_reset.
int crh_set_display(crh_ctx* c, int tonemap_mode, float exposure, float white_point)
{
  if (!c) return CRH_E_INVALID;
  const float f[] = {exposure, white_point};
  if (!all_finite(f, 2)) return fail(c, CRH_E_INVALID, "exposure / white point hold a NaN / Inf");
  c->par.tonemap_mode = tonemap_mode; c->par.exposure = exposure; c->par.white_point = white_point;      // read by the tone map only
  return CRH_OK;
}

int crh_get_display(crh_ctx* c, int* tonemap_mode, float* exposure, float* white_point, int* auto_on)
{
  if (!c) return CRH_E_INVALID;
  if (tonemap_mode) *tonemap_mode = c->par.tonemap_mode;
  if (exposure) *exposure = c->par.exposure;
  if (white_point) *white_point = c->par.white_point;
  if (auto_on) *auto_on = c->meter_on ? 1 : 0;
  return CRH_OK;
}

void crh_meter_defaults(crh_meter_params* p)
{
  if (!p) return;
  p->key_stops = -2.47393118833f;      // log2(0.18)
  p->min_stops = -10.0f; p->max_stops = 10.0f;
  p->white_permille = 990u; p->white_min = 1.0f; p->white_max = 10.0f;
  p->rect[0] = p->rect[1] = p->rect[2] = p->rect[3] = 0u;
}

int crh_meter_from_histogram(const uint32_t hist[256], const crh_meter_params* p, float gain_exposure_in, float* exposure, float* white_point, uint32_t* white_bin)
{
  if (!hist || !p || !exposure || !white_point) return CRH_E_INVALID;
  const float in[] = {gain_exposure_in, *white_point};
  if (!meter_params_ok(p) || !all_finite(in, 2)) return CRH_E_INVALID;
  uint32_t wb = 0, n_lit = 0;
  meter_rule_host(hist, meter_rule_of(*p, gain_exposure_in, *white_point), exposure, white_point, &wb, &n_lit);
  if (white_bin) *white_bin = wb;
  return CRH_OK;
}

int crh_set_auto_exposure(crh_ctx* c, const crh_meter_params* p)
{
  if (!c) return CRH_E_INVALID;
  if (!p) { c->meter_on = false; return CRH_OK; }
  if (!meter_params_ok(p)) return fail(c, CRH_E_INVALID, "meter params: NaN / Inf, min_stops > max_stops, white_min > white_max or white_permille > 1000");
  if (int rc = ensure_meter_blocks(c)) return rc;
  c->meter_par = *p; c->meter_on = true;
  return CRH_OK;
}

int crh_measure_exposure(crh_ctx* c, const crh_meter_params* p, crh_meter_result* out)
{
  if (c) c->read_since_render = true;
  if (!c || !out || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator / null output");
  crh_meter_params def; crh_meter_defaults(&def);
  if (!p) p = &def;
  if (!meter_params_ok(p)) return fail(c, CRH_E_INVALID, "meter params: NaN / Inf, min_stops > max_stops, white_min > white_max or white_permille > 1000");
  if (int rc = ensure_meter_blocks(c)) return rc;
  CRH_HIP(hipSetDevice(c->device));
  Launch L{cstream(c), c->grid, false};
  meter_image(c, L, display_source(c), *p, c->d_meter + 3);
  CRH_HIP(hipGetLastError());
  DMeter h;
  CRH_HIP(hipMemcpyAsync(&h, c->d_meter + 3, sizeof h, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  std::memcpy(out->hist, h.hist, sizeof out->hist);
  out->n_unsampled = h.n_unsampled; out->n_lit = h.n_lit; out->exposure = h.metered[0]; out->white_point = h.metered[1]; out->white_bin = h.white_bin;
  return CRH_OK;
}

int crh_save_accum(crh_ctx* c, float* out, uint32_t* frames_done)
{
  if (c) c->read_since_render = true;
  if (!c || !out || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator / null output");
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  CRH_HIP(hipMemcpyAsync(out, display_source(c), sizeof(float4) * (size_t)c->par.width * c->par.height, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  if (frames_done) *frames_done = c->frames_done;
  return CRH_OK;
}

int crh_load_accum(crh_ctx* c, const float* in, uint32_t frames_done)
{
  if (!c || !in || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator / null input");
  if (c->adaptive) return fail(c, CRH_E_INVALID, "checkpoints do not carry the adaptive sampler's second moments");
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  CRH_HIP(hipMemcpyAsync(c->d_accum, in, sizeof(float4) * (size_t)c->par.width * c->par.height, hipMemcpyHostToDevice, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  c->frames_done = frames_done; c->pending_n = 0; c->assembled_valid = false; reproject_drop(c);
  return CRH_OK;
}

int crh_accum_device_ptr(crh_ctx* c, void** p, uint64_t* nbytes)
{
  if (!c || !p || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  *p = c->d_accum; if (nbytes) *nbytes = sizeof(float4) * (uint64_t)c->par.width * c->par.height;
  return CRH_OK;
}

int crh_get_stats(crh_ctx* c, crh_stats* out)
{
  if (c) c->read_since_render = true;
  if (!c || !out) return fail(c, CRH_E_INVALID, "null stats");
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  drain_events(c);
  DCounters h;
  CRH_HIP(hipMemcpyAsync(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  out->rays_nearest = h.rays_nearest; out->rays_any = h.rays_any; out->nodes_nearest = h.nodes_nearest; out->tris_nearest = h.tris_nearest;
  out->nodes_any = h.nodes_any; out->tris_any = h.tris_any; out->shaded_hits = h.shaded_hits; out->samples = h.samples;
  out->seconds = c->seconds_acc;
  return check_device_error(c);
}

int crh_get_packet_stats(crh_ctx* c, uint64_t* packet_rays, uint64_t* fallback_rays)
{
  if (!c) return CRH_E_INVALID;
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  drain_events(c);
  DCounters h;
  CRH_HIP(hipMemcpyAsync(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  if (packet_rays) *packet_rays = h.packet_rays;
  if (fallback_rays) *fallback_rays = h.packet_fallback;
  return CRH_OK;
}

int crh_get_kernel_timing(crh_ctx* c, double* trace_ms_total, uint64_t* trace_launches, double* all_ms_total)
{
  if (!c) return CRH_E_INVALID;
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  drain_events(c);
  if (trace_ms_total) *trace_ms_total = c->trace_ms_acc;
  if (trace_launches) *trace_launches = c->trace_launches;
  if (all_ms_total) *all_ms_total = c->all_ms_acc;
  return CRH_OK;
}

}  // extern "C"
