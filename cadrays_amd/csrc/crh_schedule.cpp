// crh_schedule.cpp -- the per-iteration wavefront schedule: lanes, batches, frame pipelining, look-ahead, adaptive iterations
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h;
// the rules -- what is cut, planned and ordered how -- are the pure functions of crh_plan.h: this file enqueues what they answer)
#include "crh_context.h"

using namespace crh;
using namespace crh::api;

namespace {

// One wavefront schedule: `ns` samples of `nt` tiles (ids at d_tiles, seeds at d_seeds) on one stream and one slice of the path state.
struct Lane { hipStream_t stream; DPaths P; DQueues Q; int grid, grid_trace; bool timed; const uint32_t* n_tiles_dev = nullptr; bool donate = false;
              bool frame = false; int grid_frame = 0;         // frame: the whole batch in one launch of the frame kernel (k_frame.h) with grid_frame workgroups
              const uint32_t* h_seeds = nullptr;              // ... whose <= 16 frame seeds travel by value (d_seeds == nullptr)
              hipEvent_t tune_e0 = nullptr, tune_e1 = nullptr;      // ... bracketed by these two events when the feeder count is being tuned (crh_context.h FeedTune)
              uint32_t* tile_cost = nullptr; };                     // ... and whose accumulate adds the rays its paths traced to the per-tile sums (crh_context.h TileOrder)

// A lane's slice [base, ...) of every path-state array (queue entries are positions relative to the slice) and its own counter block
void slice(Lane& ln, const DPaths& P, const DQueues& Q, size_t base, uint32_t* counts)
{
  ln.P.ray_o[0] = P.ray_o[0] + base; ln.P.ray_o[1] = P.ray_o[1] + base; ln.P.ray_d[0] = P.ray_d[0] + base; ln.P.ray_d[1] = P.ray_d[1] + base;
  ln.P.thr[0] = P.thr[0] + base; ln.P.thr[1] = P.thr[1] + base; ln.P.hit = P.hit + base; ln.P.rad = P.rad + base;
  ln.P.sh_o = P.sh_o + base; ln.P.sh_d = P.sh_d + base; ln.P.sh_c = P.sh_c + base; ln.P.stamp = P.stamp;
  ln.Q.q[0] = Q.q[0] + base; ln.Q.q[1] = Q.q[1] + base; ln.Q.q_sh = Q.q_sh + base; ln.Q.q2 = Q.q2 + base; ln.Q.q2_sh = Q.q2_sh + base; ln.Q.counts = counts;
}

// crh_stats.seconds: the device time of a span of work on one stream, between two events that wait in render_ev until someone asks for the times
struct Span { hipEvent_t e0, e1; };
Span span_begin(crh_ctx* c, hipStream_t on) { const Span s{get_event(c), get_event(c)}; hipEventRecord(s.e0, on); return s; }
void span_end(crh_ctx* c, const Span& s, hipStream_t on) { hipEventRecord(s.e1, on); c->render_ev.emplace_back(s.e0, s.e1); }

// the event pairs of a measurement that have finished: into its running means, the events back to the pool
void harvest(crh_ctx* c, plan::Tally<hipEvent_t>& t)
{
  t.harvest([](hipEvent_t e1) { return hipEventQuery(e1) != hipErrorNotReady; },
            [](hipEvent_t e0, hipEvent_t e1, float* ms) { return hipEventElapsedTime(ms, e0, e1) == hipSuccess; },
            [c](hipEvent_t e) { c->ev_pool.push_back(e); });
}

// May this batch take the frame kernel?  Small, not counted, not timed per kernel, slots that fit the bits the kernel keeps them in.
bool frame_ok(const crh_ctx* c, uint64_t total)
{ return c->frame_kernel && !c->counters_on && !c->timing_on && total <= c->lane_max_paths && total < (uint64_t)kFrameMaxPaths && frame_launchable(!c->inst.empty()); }
int frame_grid(const crh_ctx* c, const DScene& S, uint32_t share = 1u)
{
  const int res = frame_resident_grid(c->clamp_grid ? c->cus : 0, S.two_level != 0);
  const int want = c->frame_grid > 0 ? std::min(c->frame_grid, res) : res;
  return std::max(std::min(res, 32), want / (int)std::max(1u, share));
}

int run_lane(crh_ctx* c, const Lane& ln, const DScene& S, const uint32_t* d_tiles, uint32_t nt, const uint32_t* d_seeds, uint32_t ns, int seed_per_tile,
             bool accumulate, hipEvent_t before_accumulate = nullptr, hipEvent_t before_accumulate2 = nullptr, hipEvent_t before_accumulate3 = nullptr)
{
  Launch L{ln.stream, ln.grid, c->counters_on};
  Launch LT{ln.stream, ln.grid_trace, c->counters_on, c->clamp_grid ? c->cus : 0, ln.donate && !c->counters_on};
  // wide batches (a wavefront = >= 16 consecutive samples of one pixel): the camera rays are walked as packets (kernels.hip, k_trace_packets)
  // (small batches -- a wavefront = an 8 x 8 pixel block -- lose with packets: 468 -> 391 Redraw/s, profiles/r4/ab_camera_ray_packets.txt)
  LT.packets = c->packets > 0 && !c->counters_on && !ln.donate && std::min<uint32_t>(ns & (0u - ns), 64u) >= (uint32_t)c->packets;

  if (ln.frame) {
    // the frame kernel: camera rays, every bounce's traversal, shading and shadow rays of this batch in ONE launch (k_frame.h); its two control words live behind
    // the queue counters of this lane (zero when allocated, left zero by every launch)
    Launch LF{ln.stream, ln.grid_frame, false, c->clamp_grid ? c->cus : 0};
    if (ln.tune_e0) hipEventRecord(ln.tune_e0, ln.stream);
    launch_frame(LF, S, ln.P, ln.Q.counts + 12, d_tiles, nt, d_seeds, ns, seed_per_tile, ln.n_tiles_dev, c->frame_live, c->frame_chunk, c->frame_low_water, c->frame_feeders, c->frame_claim_step, c->frame_starve, c->d_counters, ln.h_seeds, c->d_api_cursor + 8, c->frame_help | (c->frame_help_low << 16));      // + 8: the context's device error word (crh_context.cpp check_device_error)
    if (ln.tune_e1) hipEventRecord(ln.tune_e1, ln.stream);
  } else {
  launch_raygen(L, S, ln.P, ln.Q, 0, d_tiles, nt, d_seeds, ns, seed_per_tile, ln.n_tiles_dev, ln.h_seeds);
  int qin = 0;
  for (uint32_t b = 0; b < S.max_depth; ++b) {
    const Launch& T = LT;
    if (ln.timed && c->timing_on) {
      hipEvent_t e0 = get_event(c), e1 = get_event(c);
      hipEventRecord(e0, ln.stream);
      launch_trace_nearest(T, S, ln.P, ln.Q, qin, b, c->d_counters);
      hipEventRecord(e1, ln.stream);
      c->trace_ev.emplace_back(e0, e1);
    } else launch_trace_nearest(T, S, ln.P, ln.Q, qin, b, c->d_counters);
    launch_shade(L, S, ln.P, ln.Q, qin, b, c->d_counters);
    if (S.n_lights > 0) launch_trace_any(T, S, ln.P, ln.Q, c->d_counters);
    qin = 1 - qin;
  }
  }
  if (accumulate && before_accumulate) CRH_HIP(hipStreamWaitEvent(ln.stream, before_accumulate, 0));      // samples are folded in in frame order
  if (accumulate && before_accumulate2) CRH_HIP(hipStreamWaitEvent(ln.stream, before_accumulate2, 0));    // ... and not while a read-back tone-maps the accumulator
  if (accumulate && before_accumulate3) CRH_HIP(hipStreamWaitEvent(ln.stream, before_accumulate3, 0));    // ... and after a restart has zeroed it
  if (accumulate) launch_accumulate(L, S, ln.P, c->d_accum, c->adaptive ? c->d_m2 : nullptr, d_tiles, nt, 0, ns, ns, c->d_counters, ln.n_tiles_dev, ln.frame && ns == 1u ? ln.tile_cost : nullptr);
  CRH_HIP(hipGetLastError());
  return CRH_OK;
}

int ensure_lanes(crh_ctx* c)
{
  if (c->d_lane_counts) return CRH_OK;
  for (uint32_t k = 0; k < 8u; ++k) {      // tile ranges of one batch (n_lanes <= 8), or frames in flight (pipe_depth <= 8)
    CRH_HIP(hipStreamCreateWithFlags(&c->lane_stream[k], hipStreamNonBlocking));
    CRH_HIP(hipEventCreateWithFlags(&c->lane_join[k], hipEventDisableTiming));
  }
  CRH_HIP(hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming));
  CRH_HIP(c->d_lane_counts.reserve(kCounts * 8));
  CRH_HIP(hipMemsetAsync(c->d_lane_counts, 0, kCounts * sizeof(uint32_t) * 8, cstream(c)));
  return CRH_OK;
}

// One batch: `ns` samples of `nt` tiles whose ids sit at d_tiles; seeds at d_seeds.
int run_batch(crh_ctx* c, const DScene& S, const uint32_t* d_tiles, uint32_t nt, const uint32_t* d_seeds, uint32_t ns, int seed_per_tile = 0,
              bool accumulate = true)
{
  c->pending_n = 0;                                  // the path buffer is about to be overwritten
  c->paths.stamp = next_stamp(c);                    // lanes copy it; a look-ahead batch is folded in later by launch_accumulate(c->paths, ...)
  const uint32_t tpp = S.tile_size * S.tile_size;
  const uint64_t total = (uint64_t)nt * tpp * ns;
  // two ranges pay from about a frame's worth of paths (2 M: 173 -> 182 Redraw/s); below that one schedule with a small grid is
  // faster (128 tiles per call: 303 vs 284 calls/s)
  const uint32_t K = total >= (1u << 20) ? std::min<uint32_t>(c->n_lanes, nt / 4u) : 1u;
  const bool frame = frame_ok(c, total);
  if (frame || K < 2 || total > c->lane_max_paths || !accumulate || c->counters_on) {
    const bool small = total <= c->lane_max_paths && !c->counters_on;      // small batches get grids that follow their size (crh_plan.h small_grid)
    Lane one{cstream(c), c->paths, c->queues, small ? plan::small_grid(total, c->grid, 2048) : c->grid, small ? plan::small_grid(total, c->grid_trace, 2048) : c->grid_trace, true};
    one.donate = small && c->donate;
    one.frame = frame; one.grid_frame = frame ? frame_grid(c, S) : 0;
    return run_lane(c, one, S, d_tiles, nt, d_seeds, ns, seed_per_tile, accumulate);
  }
  // small batch: K tile ranges on K streams, each with its own slice [base, base + n_k * tpp * ns) of every path-state array
  // and its own counter block; fork from / join into the context's stream
  int rc = ensure_lanes(c); if (rc) return rc;
  CRH_HIP(hipEventRecord(c->lane_fork, cstream(c)));
  size_t base = 0;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t t0 = (uint32_t)((uint64_t)nt * k / K), t1 = (uint32_t)((uint64_t)nt * (k + 1) / K);
    Lane ln; ln.stream = c->lane_stream[k]; ln.timed = false; ln.donate = c->donate;
    ln.grid = plan::small_grid(total / K, c->grid, 2048);
    ln.grid_trace = plan::small_grid(total / K, c->grid_trace, 2048);
    slice(ln, c->paths, c->queues, base, c->d_lane_counts + kCounts * k);
    CRH_HIP(hipStreamWaitEvent(ln.stream, c->lane_fork, 0));
    rc = run_lane(c, ln, S, d_tiles + t0, t1 - t0, seed_per_tile ? d_seeds + t0 : d_seeds, ns, seed_per_tile, true); if (rc) return rc;
    CRH_HIP(hipEventRecord(c->lane_join[k], ln.stream));
    CRH_HIP(hipStreamWaitEvent(cstream(c), c->lane_join[k], 0));
    base += (size_t)(t1 - t0) * tpp * ns;
  }
  return CRH_OK;
}

int validate_tiles(crh_ctx* c, const uint32_t* tiles, uint32_t nt)
{
  const uint32_t all = plan::tile_count(c->par.width, c->par.height, c->par.tile_size);
  std::vector<uint8_t> seen(all, 0);          // a tile listed twice would be accumulated by two threads at once
  for (uint32_t i = 0; i < nt; ++i) {
    if (tiles[i] >= all) return fail(c, CRH_E_INVALID, "tile id out of range");
    if (seen[tiles[i]]) return fail(c, CRH_E_INVALID, "duplicate tile id");
    seen[tiles[i]] = 1;
  }
  return CRH_OK;
}

// Tile ids to the device, stream-ordered behind any kernels still reading the old ones, through pinned staging: a Redraw() does not wait for the previous
// one (an unchanged tile list is not sent again).  d_list: where this call's list sits.
int resident_tile_list(crh_ctx* c, const uint32_t* tiles, uint32_t nt, uint32_t*& d_list)
{
  if (nt > c->d_tile_ids.cap()) c->h_tile_ids.clear();
  int rc = grow_u32(c, c->d_tile_ids, nt); if (rc) return rc;
  // Round 6: TWO lists stay on the device -- crh_render hands over the image's tiles either row-major or most-expensive-first (crh_context.h TileOrder), by what
  // is in flight; switching between two resident lists costs nothing, and a frame in flight keeps reading the one it was launched with.  A third list replaces the
  // one the previous call did not use (through the context's stream: behind every frame that still reads it).
  if (c->h_tile_ids.size() == nt && std::memcmp(c->h_tile_ids.data(), tiles, sizeof(uint32_t) * nt) == 0) { d_list = c->d_tile_ids; c->tile_list_last = 0; }
  else if (c->h_tile_ids2.size() == nt && std::memcmp(c->h_tile_ids2.data(), tiles, sizeof(uint32_t) * nt) == 0) { d_list = c->d_tile_ids2; c->tile_list_last = 1; }
  else if (c->tile_list_last == 0 && !c->h_tile_ids.empty()) {      // the first list is the one in use: the new one goes to the second
    if ((rc = grow_u32(c, c->d_tile_ids2, nt))) return rc;
    if ((rc = stage_copy(c, c->d_tile_ids2, tiles, sizeof(uint32_t) * nt))) return rc;
    c->h_tile_ids2.assign(tiles, tiles + nt); d_list = c->d_tile_ids2; c->tile_list_last = 1;
  } else {
    if ((rc = stage_copy(c, c->d_tile_ids, tiles, sizeof(uint32_t) * nt))) return rc;
    c->h_tile_ids.assign(tiles, tiles + nt); d_list = c->d_tile_ids; c->tile_list_last = 0;
  }
  return CRH_OK;
}

// path budget of this call: crh_set_path_budget's, cut to what the device has free when the state would have to grow (196 B per slot; a shared or smaller
// device gets the narrower batches the budget table of cadrays_hip.h prices at a few percent, not a hipMalloc error -- ADVICE r4)
uint32_t call_budget(const crh_ctx* c, uint32_t nt, uint32_t tpp, uint32_t ns)
{
  uint32_t budget = c->max_paths;
  const uint64_t slots_wanted = (uint64_t)nt * tpp * ns * ((c->pipeline && ns <= 16u && (uint64_t)nt * tpp * ns <= c->lane_max_paths) ? c->pipe_depth : 1u);      // a pipelined frame holds pipe_depth slices
  if (slots_wanted > c->path_cap) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const uint64_t fit = (uint64_t)((double)(fr + (size_t)c->path_cap * 196u) * 0.85) / 196u;
      if (fit < budget) budget = (uint32_t)std::max<uint64_t>(fit, std::min<uint64_t>(budget, 1u << 20));
    }
  }
  return budget;
}

// per-tile ray sums of this accumulation (crh_context.h TileOrder), indexed by tile id: allocated for the image's tiles
int tile_cost_sums(crh_ctx* c, Lane& ln)
{
  crh_ctx::TileOrder& to = c->tile_order;
  const uint32_t all_tiles = plan::tile_count(c->par.width, c->par.height, c->par.tile_size);
  if (to.n != all_tiles) {
    CRH_HIP(hipStreamSynchronize(cstream(c)));
    to.n = 0;                                               // (no count is in force until both blocks have the new one)
    CRH_HIP(to.d_cost.release()); CRH_HIP(to.h_cost.release());      // blocks of exactly this size, a smaller one too
    CRH_HIP(to.d_cost.reserve(all_tiles)); CRH_HIP(hipMemsetAsync(to.d_cost, 0, sizeof(uint32_t) * all_tiles, cstream(c)));      // (never the NULL stream: once it exists every launch on the context's streams pays for it -- the drag loop lost 2.3 % to one hipMemset here)
    CRH_HIP(to.h_cost.reserve(all_tiles));
    to.n = all_tiles; to.pending = false; to.dirty = false; to.cls.clear(); to.order.clear();
  }
  if (to.streak >= 2u && to.verdict != 2u) { ln.tile_cost = to.d_cost; to.dirty = true; ++to.frames_collected; }      // (a host that keeps frames in flight gets no new list anyway: nothing is collected for it)
  return CRH_OK;
}

// the feeder count by measurement (crh_context.h FeedTune): collect the frame kernels that have finished, then either take the next measurement or the verdict
void tune_feeders(crh_ctx* c, Lane& ln)
{
  crh_ctx::FeedTune& ft = c->feed_tune;
  harvest(c, ft.t);
  if (!ft.chosen && ft.t.n[0] >= 8u && ft.t.n[1] >= 8u) { ft.chosen = ft.t.mean(1) < 0.95 * ft.t.mean(0) ? 4u : 3u; ft.t.invalidate(); }
  if (ft.chosen) { c->frame_feeders = ft.chosen; return; }
  const uint32_t block = ft.frames / 6u, which = (block + 1u) & 1u;      // blocks: warm-up (4, not measured), 3, 4, 3, 4, ...
  c->frame_feeders = which ? 4u : 3u;
  if (block != 0u && ft.frames % 6u != 0u && ft.t.pend.size() < 64u) {     // (the first frame of a block runs beside a frame of the other setting; the first block after
                                                                           // a build touches the path state for the first time)
    ln.tune_e0 = get_event(c); ln.tune_e1 = get_event(c);
    ft.t.pend.push_back({ln.tune_e0, ln.tune_e1, (int)which});
  }
  ++ft.frames;
}

// What a frame-kernel frame of the pipeline measures on its way: per-tile ray sums, the feeder count, sorted against row-major tiles
int arm_measurements(crh_ctx* c, Lane& ln, uint32_t ns, uint32_t running)
{
  crh_ctx::TileOrder& to = c->tile_order;
  if (to.on && ns == 1u) { int rc = tile_cost_sums(c, ln); if (rc) return rc; }
  if (c->feed_tune.on) tune_feeders(c, ln);
  if (to.on && to.tag_next >= 0) {      // this lone frame is a sample of the sorted-against-row-major measurement (choose_tile_list decided which list it got)
    if (!ln.tune_e0 && running == 0u && to.t.pend.size() < 32u) {
      ln.tune_e0 = get_event(c); ln.tune_e1 = get_event(c);
      to.t.pend.push_back({ln.tune_e0, ln.tune_e1, to.tag_next});
    }
    to.tag_next = -1;
  }
  return CRH_OK;
}

struct PipeProbe {      // what plan_frame asks the device: one event query each
  crh_ctx* c;
  bool frame_done(uint32_t j) const { return hipEventQuery(c->lane_join[j]) != hipErrorNotReady; }
  bool resized_done() const { return hipEventQuery(c->pipe_resized) != hipErrorNotReady; }
};

// One frame of the pipeline (crh_plan.h plan_frame says on which stream and slice, behind what): plan, arm the measurements, enqueue.
int render_pipelined_frame(crh_ctx* c, const uint32_t* d_list, uint32_t nt, uint32_t first, uint32_t ns, uint64_t total, bool frame_able, bool host_runs_ahead)
{
  const uint32_t depth = c->pipe_depth;               // streams / path-state slices the frames rotate through
  int rc = ensure_paths(c, (uint32_t)(depth * total)); if (rc) return rc;
  rc = ensure_lanes(c); if (rc) return rc;
  uint32_t seeds[16];
  plan::frame_seeds(c->par.seed, first, ns, seeds);
  DScene S; fill_scene(c, S);
  const plan::FramePlan fp = plan::plan_frame(c->pipe, {total, depth, c->frame_pipe_depth, c->stream_uses, c->counter_epoch, frame_able, host_runs_ahead}, PipeProbe{c});
  if (fp.fork) CRH_HIP(hipEventRecord(c->lane_fork, c->stream_));      // raw: no join
  Lane ln; ln.stream = c->lane_stream[fp.k]; ln.timed = false; ln.donate = c->donate; ln.h_seeds = seeds;
  const auto now = std::chrono::steady_clock::now();
  const bool burst = c->pipe_last_submit.time_since_epoch().count() != 0 && now - c->pipe_last_submit < std::chrono::microseconds(300);
  c->pipe_last_submit = now;
  const plan::PipeGrids g = plan::pipe_grids({c->grid, c->grid_trace, c->pipe_grid_min, c->pipe_grid_min_shade, c->pipe_div, total, fp.running, fp.own_running, depth, c->frame_pipe_depth, fp.frame, burst});
  ln.grid = g.grid; ln.grid_trace = g.grid_trace;
  ln.frame = fp.frame; ln.grid_frame = fp.frame ? frame_grid(c, S, g.share) : 0;
  if (fp.frame && (rc = arm_measurements(c, ln, ns, fp.running))) return rc;
  slice(ln, c->paths, c->queues, fp.base, c->d_lane_counts + kCounts * fp.k);
  ln.P.stamp = next_stamp(c);      // this frame's own stamp
  if (fp.fork) CRH_HIP(hipStreamWaitEvent(ln.stream, c->lane_fork, 0));
  for (uint32_t j = 0; j < 8u; ++j) if (fp.wait_joins >> j & 1u) CRH_HIP(hipStreamWaitEvent(ln.stream, c->lane_join[j], 0));
  if (fp.wait_counters_zeroed) { const hipEvent_t z = c->counters_zeroed[c->counter_epoch & 3u]; if (z) CRH_HIP(hipStreamWaitEvent(ln.stream, z, 0)); }
  if (fp.resized == plan::FramePlan::kRecord) {
    if (!c->pipe_resized) CRH_HIP(hipEventCreateWithFlags(&c->pipe_resized, hipEventDisableTiming));
    CRH_HIP(hipEventRecord(c->pipe_resized, ln.stream));
  } else if (fp.resized == plan::FramePlan::kWait) CRH_HIP(hipStreamWaitEvent(ln.stream, c->pipe_resized, 0));
  c->pending_n = 0;
  const Span span = span_begin(c, ln.stream);                 // crh_stats.seconds: device time of this frame (frames in flight overlap)
  const hipEvent_t guard = c->rb_guard_pending ? c->rb_guard : nullptr; c->rb_guard_pending = false;      // later frames are ordered behind this one's accumulate
  const hipEvent_t after_reset = c->reset_pending ? c->reset_ev : nullptr; c->reset_pending = false;      // (it followed the joins of every earlier frame)
  rc = run_lane(c, ln, S, d_list, nt, nullptr, ns, 0, true, fp.after_prev ? c->lane_join[fp.prev] : nullptr, guard, after_reset); if (rc) return rc;
  span_end(c, span, ln.stream);
  CRH_HIP(hipEventRecord(c->lane_join[fp.k], ln.stream));
  plan::frame_submitted(c->pipe, fp.k);
  rc = trim_events(c);                                        // every 4096 frames: waits for the device once
  c->read_since_render = false;
  return rc;
}

// The call as batches of `group` tiles x `spb` samples on the context's stream, one after the other
int render_batches(crh_ctx* c, const uint32_t* d_list, uint32_t nt, uint32_t first, uint32_t ns, uint32_t group, uint32_t spb)
{
  int rc = grow_u32(c, c->d_seeds, ns); if (rc) return rc;
  {
    std::vector<uint32_t> seeds(ns);
    plan::frame_seeds(c->par.seed, first, ns, seeds.data());
    if ((rc = stage_copy(c, c->d_seeds, seeds.data(), sizeof(uint32_t) * ns))) return rc;
  }
  rc = ensure_paths(c, group * c->par.tile_size * c->par.tile_size * spb); if (rc) return rc;
  DScene S; fill_scene(c, S);
  const Span span = span_begin(c, cstream(c));
  for (uint32_t t0 = 0; t0 < nt; t0 += group) {
    const uint32_t g = std::min(group, nt - t0);
    for (uint32_t s0 = 0; s0 < ns; s0 += spb) {
      rc = run_batch(c, S, d_list + t0, g, c->d_seeds + s0, std::min(spb, ns - s0));
      if (rc) return rc;
    }
  }
  span_end(c, span, cstream(c));
  rc = trim_events(c);
  c->read_since_render = false;      // from here on, only a call other than the next render sets it again
  return rc;
}

int render_impl(crh_ctx* c, const uint32_t* tiles, uint32_t nt, uint32_t first, uint32_t ns)
{
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  if (ns == 0 || nt == 0) return CRH_OK;
  CRH_HIP(hipSetDevice(c->device));
  int rc = upload_textures(c); if (rc) return rc;
  if ((rc = validate_tiles(c, tiles, nt))) return rc;
  uint32_t* d_list = nullptr;
  if ((rc = resident_tile_list(c, tiles, nt, d_list))) return rc;
  const uint32_t tpp = c->par.tile_size * c->par.tile_size;
  const uint32_t budget = call_budget(c, nt, tpp, ns);
  const plan::CallCut cut = plan::cut_call(nt, tpp, ns, budget, c->packets, c->counters_on, c->lane_max_paths);
  const uint64_t total = (uint64_t)nt * tpp * ns;
  // Measured on C3 at 1080p, 1 spp per call: free-running 232 -> 326 Redraw/s (C2: 323 -> 442); a host that reads every frame back
  // would get 187 instead of 225 (one schedule per frame is slower than two tile ranges when nothing overlaps it), so a
  // read-back / synchronisation since the last render selects the two-range schedule for this frame.
  const bool host_runs_ahead = !c->read_since_render;
  // Small whole-frame batches -- one Redraw() each -- are pipelined (crh_plan.h plan_frame).  Two kinds of frame travel through the same pipeline:
  //   * the FRAME KERNEL (k_frame.h, one launch): the fastest way through a chip that is empty or nearly so -- a lone frame (2.98 ms against 4.26 staged on C3),
  //     and the frames of a host that shows every frame or restarts with every frame (AppViewer.cxx:979-984: the camera drag);
  //   * the STAGED form (a launch per stage and bounce; the stages of eight frames in flight overlap one another): the higher throughput once the host runs far
  //     ahead -- 467-480 Redraw/s against 406-426 with frame kernels only.
  // Neither kind waits for the context's stream unless something was enqueued there that its tracing reads (seeds travel by value, a restart's memsets gate the
  // accumulate only).
  const bool frame_able = frame_ok(c, total);
  if (c->pipeline && (host_runs_ahead || frame_able) && !c->counters_on && !c->timing_on && !c->adaptive && cut.group == nt && cut.spb == ns && ns <= 16u && total >= (1u << 20) &&
      total <= c->lane_max_paths && (uint64_t)c->pipe_depth * total <= budget)      // `budget`: the device's free memory counts here too
    return render_pipelined_frame(c, d_list, nt, first, ns, total, frame_able, host_runs_ahead);
  return render_batches(c, d_list, nt, first, ns, cut.group, cut.spb);
}

// ---- adaptive screen sampling (reference: AdaptiveScreenSampling / NbRayTracingTiles, SettingsWidget.cxx:427-477) ----------
int tile_stats(crh_ctx* c, std::vector<float>& err, std::vector<uint32_t>& cnt)
{
  const uint32_t nt = plan::tile_count(c->par.width, c->par.height, c->par.tile_size);
  if (nt > c->d_tile_err.cap() || nt > c->d_tile_cnt.cap()) {
    CRH_HIP(hipStreamSynchronize(cstream(c)));
    c->picked_valid = false;                                // the sampler allocates its three again at this size
    CRH_HIP(c->d_tile_cdf.release()); CRH_HIP(c->d_picked.release()); CRH_HIP(c->d_adapt_n.release());
    CRH_HIP(c->d_tile_err.reserve(nt)); CRH_HIP(c->d_tile_cnt.reserve(nt));
  }
  DScene S; fill_scene(c, S);
  Launch L{cstream(c), c->grid, false};
  launch_tile_error(L, S, c->d_accum, c->d_m2, c->d_tile_err, c->d_tile_cnt, nt);
  err.resize(nt); cnt.resize(nt);
  CRH_HIP(hipMemcpyAsync(err.data(), c->d_tile_err, sizeof(float) * nt, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipMemcpyAsync(cnt.data(), c->d_tile_cnt, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  return CRH_OK;
}

// One adaptive iteration: draw `adaptive_tiles` tiles with probability proportional to their error estimate (inverse CDF
// driven by the base-2 radical inverse of a running pick counter), render +1 sample on the distinct tiles drawn.  Everything --
// error estimate, running sum, draws, tile list, per-tile seeds -- happens in HBM, stream-ordered: the host only advances the
// pick counter, so a GUI loop of crh_render(1) calls never waits for the device (the reference offers this mode as its
// responsiveness feature, SettingsWidget.cxx:427-477).
int adaptive_iteration(crh_ctx* c)
{
  int rc = upload_textures(c); if (rc) return rc;
  const uint32_t ts = c->par.tile_size, tpp = ts * ts;
  const uint32_t nt = plan::tile_count(c->par.width, c->par.height, ts);
  const uint32_t most = std::min(c->adaptive_tiles, nt);                // distinct tiles one iteration can draw
  if (nt > c->d_tile_err.cap() || nt > c->d_tile_cnt.cap() || nt > c->d_tile_cdf.cap() || nt > c->d_picked.cap() || !c->d_adapt_n) {
    CRH_HIP(hipStreamSynchronize(cstream(c)));
    CRH_HIP(c->d_tile_err.reserve(nt)); CRH_HIP(c->d_tile_cnt.reserve(nt));
    CRH_HIP(c->d_tile_cdf.reserve(nt)); CRH_HIP(c->d_picked.reserve(nt)); CRH_HIP(c->d_adapt_n.reserve(16));
  }
  if ((rc = grow_u32(c, c->d_tile_ids, most))) return rc;
  if ((rc = grow_u32(c, c->d_seeds, most))) return rc;
  c->h_tile_ids.clear();                                                // the device is about to write its own list there
  rc = ensure_paths(c, most * tpp); if (rc) return rc;
  DScene S; fill_scene(c, S);
  const Span span = span_begin(c, cstream(c));
  Launch L{cstream(c), c->grid, false};
  launch_tile_error(L, S, c->d_accum, c->d_m2, c->d_tile_err, c->d_tile_cnt, nt);
  launch_adaptive_pick(L, c->d_tile_err, c->d_tile_cnt, nt, c->adaptive_picks, c->adaptive_tiles, c->par.seed, c->d_tile_cdf, c->d_picked,
                       c->d_tile_ids, c->d_seeds, c->d_adapt_n);
  c->adaptive_picks += c->adaptive_tiles; c->picked_valid = true;
  c->pending_n = 0;
  c->paths.stamp = next_stamp(c);
  Lane ln{cstream(c), c->paths, c->queues, plan::small_grid((uint64_t)most * tpp, c->grid, 1024), plan::small_grid((uint64_t)most * tpp, c->grid_trace, 2048), true};      // grids follow the batch (run_batch)
  ln.n_tiles_dev = c->d_adapt_n; ln.donate = c->donate;
  ln.frame = frame_ok(c, (uint64_t)most * tpp); ln.grid_frame = ln.frame ? std::min(frame_grid(c, S), (int)std::max<uint64_t>(64u, (uint64_t)most * tpp / 512u)) : 0;
  rc = run_lane(c, ln, S, c->d_tile_ids, most, c->d_seeds, 1, 1, true); if (rc) return rc;
  span_end(c, span, cstream(c));
  return trim_events(c);
}

int render_adaptive(crh_ctx* c, uint32_t n)
{
  CRH_HIP(hipSetDevice(c->device));
  for (uint32_t i = 0; i < n; ++i) { int rc = adaptive_iteration(c); if (rc) return rc; }
  c->frames_done += n;
  return CRH_OK;
}

// look-ahead: one wide batch of `lookahead` frames is traced at once; each call folds in only the samples it asked for
// (ramp -- crh_set_lookahead_auto: the first frame after a restart is ONE sample, what the user sees while dragging, then batches of 4, 16, ... k_max)
int render_lookahead(crh_ctx* c, const std::vector<uint32_t>& all, uint32_t n, bool ramp, uint32_t k_max)
{
  const uint32_t ts = c->par.tile_size, nt = (uint32_t)all.size();
  CRH_HIP(hipSetDevice(c->device));
  while (n > 0) {
    if (c->pending_n == 0 || c->pending_first != c->frames_done || c->pending_tiles != nt) {
      uint32_t k = c->lookahead;
      if (ramp) {
        if (n >= k_max) {                                                   // the caller asks for a whole batch itself: nothing to speculate on,
          int rcn = render_impl(c, all.data(), nt, c->frames_done, n); if (rcn) return rcn;      // and render_impl cuts it into the widest batches that fit
          c->frames_done += n; n = 0; c->ramp_k = k_max;
          break;
        }
        k = std::max(c->ramp_k, n);                                         // a call that asks for n samples at once is not cut finer than that
        c->ramp_k = std::min(4u * k, k_max);
        if (k == 1) {                                                       // right after a restart: a plain frame
          int rc1 = render_impl(c, all.data(), nt, c->frames_done, 1); if (rc1) return rc1;
          c->frames_done += 1; n -= 1;
          continue;
        }
      }
      int rc = upload_textures(c); if (rc) return rc;
      if ((rc = grow_u32(c, c->d_tile_ids, nt))) return rc;
      if ((rc = grow_u32(c, c->d_seeds, k))) return rc;
      std::vector<uint32_t> seeds(k);
      plan::frame_seeds(c->par.seed, c->frames_done, k, seeds.data());
      c->h_tile_ids.clear();
      CRH_HIP(hipMemcpyAsync(c->d_tile_ids, all.data(), sizeof(uint32_t) * nt, hipMemcpyHostToDevice, cstream(c)));
      CRH_HIP(hipMemcpyAsync(c->d_seeds, seeds.data(), sizeof(uint32_t) * k, hipMemcpyHostToDevice, cstream(c)));
      CRH_HIP(hipStreamSynchronize(cstream(c)));
      if ((rc = ensure_paths(c, nt * ts * ts * k))) return rc;
      DScene S; fill_scene(c, S);
      const Span span = span_begin(c, cstream(c));
      if ((rc = run_batch(c, S, c->d_tile_ids, nt, c->d_seeds, k, 0, false))) return rc;
      span_end(c, span, cstream(c));
      if ((rc = trim_events(c))) return rc;
      c->pending_first = c->frames_done; c->pending_n = k; c->pending_off = 0; c->pending_tiles = nt;
    }
    const uint32_t m = std::min(n, c->pending_n);
    DScene S; fill_scene(c, S);
    Launch L{cstream(c), c->grid, false};
    launch_accumulate(L, S, c->paths, c->d_accum, nullptr, c->d_tile_ids, nt, c->pending_off, m, c->pending_off + c->pending_n, c->d_counters);      // the batch held pending_off + pending_n samples
    CRH_HIP(hipGetLastError());
    c->pending_off += m; c->pending_n -= m; c->pending_first += m; c->frames_done += m; n -= m;
  }
  return CRH_OK;
}

// the order the tiles are claimed in (crh_context.h TileOrder): most rays of the last accumulation first -- for a host whose frames start on an idle chip (six
// calls in a row found nothing in flight: a viewer that waits for every frame; a drag loop with a gap now and then does not get there).  With frames in flight the drain overlaps the next frame anyway, the row-major
// list keeps neighbouring tiles together (sorted: drag loop -4 % on C3 / C2) and a new list would wait for the frames that read the old one.
// `all`: the image's tiles row-major on entry, the list this crh_render(n) hands to render_impl on return.
void choose_tile_list(crh_ctx* c, std::vector<uint32_t>& all, uint32_t n)
{
  crh_ctx::TileOrder& to = c->tile_order;
  const uint32_t nt = (uint32_t)all.size();
  if (!to.on || to.n != nt || n != 1u) return;         // (one sample per pixel: the frame kernel's regime; a wide batch keeps the row-major list -- its tile groups want neighbours)
  const bool busy = c->pipe.last_running != 0u;        // what the previous pipelined frame found in flight when it was submitted (no event queries of its own here:
                                                       // four more hipEventQuery calls per frame cost the drag loop 2 - 3 %)
  to.streak = busy ? 0u : std::min(to.streak + 1u, 1000u);
  if (to.streak >= 6u && to.pending && hipEventQuery(to.copied) == hipSuccess) {
    to.pending = false;
    if (plan::order_tiles(to.h_cost, nt, to.cls, to.order)) ++to.reorders;
  }
  bool sorted = false;
  if (to.streak >= 6u && to.order.size() == nt) {
    harvest(c, to.t);                                  // frame kernels of the measurement that have finished
    if (!to.verdict && to.t.n[0] >= 5u && to.t.n[1] >= 5u) { to.verdict = to.t.mean(0) < 0.98 * to.t.mean(1) ? 1u : 2u; to.t.invalidate(); }
    to.tag_next = -1;
    if (to.verdict) sorted = to.verdict == 1u;
    else if (c->feed_tune.on && !c->feed_tune.chosen) sorted = true;      // one measurement at a time: the feeder count first
    else { const uint32_t which = to.trials++ & 1u; sorted = which == 0u; to.tag_next = (int)which; }
  }
  if (sorted) { all = to.order; ++to.calls_sorted; } else ++to.calls_row_major;
}

}  // namespace

extern "C" {

int crh_render(crh_ctx* c, uint32_t n)
{
  if (!c) return CRH_E_INVALID;
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  c->assembled_valid = false;                            // reads show this context's own accumulator again
  if (c->adaptive) return render_adaptive(c, n);
  const uint32_t ts = c->par.tile_size, nt = plan::tile_count(c->par.width, c->par.height, ts);
  std::vector<uint32_t> all(nt);
  for (uint32_t i = 0; i < nt; ++i) all[i] = i;
  const bool ramp = c->lookahead_auto > 1;
  const uint32_t k_max = ramp ? c->lookahead_auto : c->lookahead;
  if (k_max > 1 && (uint64_t)nt * ts * ts * k_max <= c->max_paths) return render_lookahead(c, all, n, ramp, k_max);
  choose_tile_list(c, all, n);
  int rc = render_impl(c, all.data(), nt, c->frames_done, n);
  if (rc == CRH_OK) c->frames_done += n;
  return rc;
}

int crh_render_tiles(crh_ctx* c, const uint32_t* tiles, uint32_t nt, uint32_t first, uint32_t ns)
{
  if (!c || (nt && !tiles)) return fail(c, CRH_E_INVALID, "null tile list");
  c->assembled_valid = false;
  return render_impl(c, tiles, nt, first, ns);
}

int crh_set_adaptive(crh_ctx* c, int on, uint32_t tiles_per_iteration)
{
  if (!c || (on && tiles_per_iteration == 0)) return fail(c, CRH_E_INVALID, "tiles_per_iteration must be > 0");
  c->adaptive = on != 0; if (on) c->adaptive_tiles = tiles_per_iteration;
  return do_reset(c);                                   // like every rendering-parameter change, restarts accumulation
}

int crh_set_show_tiles(crh_ctx* c, int on)
{
  if (!c) return CRH_E_INVALID;
  c->show_tiles = on != 0;                              // display-only: accumulation goes on
  return CRH_OK;
}

int crh_set_lookahead(crh_ctx* c, uint32_t frames)
{
  if (!c || frames == 0) return fail(c, CRH_E_INVALID, "lookahead must be >= 1");
  c->lookahead = frames; c->pending_n = 0;
  return CRH_OK;
}

int crh_set_lookahead_auto(crh_ctx* c, uint32_t max_frames)
{
  if (!c) return CRH_E_INVALID;
  c->lookahead_auto = max_frames; c->ramp_k = 1; c->pending_n = 0;
  return CRH_OK;
}

int crh_set_schedule(crh_ctx* c, int mode)
{
  if (!c || mode < CRH_SCHEDULE_AUTO || mode > CRH_SCHEDULE_STAGED) return fail(c, CRH_E_INVALID, "schedule must be CRH_SCHEDULE_AUTO / _WIDE / _SMALL / _STAGED");
  if (c->schedule == CRH_SCHEDULE_AUTO) { c->auto_lane_max_paths = c->lane_max_paths; c->auto_donate = c->donate; c->auto_pipeline = c->pipeline; c->auto_frame_kernel = c->frame_kernel; }
  c->schedule = mode; c->pending_n = 0;
  c->read_since_render = true;                           // the next frame is not pipelined behind frames of the other schedule
  // WIDE: no batch counts as small (run_batch: one stream, full grids, plain kernels; render_impl: no frame pipelining; adaptive
  // iterations: plain kernels).  SMALL: every batch up to the path budget does (the frame kernel takes those below 2^25 slots, the staged form the rest).
  // STAGED: like SMALL, in the staged form only (lanes / pipelined launches per stage and bounce, the donating kernels) -- the schedule the frame kernel replaced.
  c->lane_max_paths = mode == CRH_SCHEDULE_WIDE ? 0u : (mode == CRH_SCHEDULE_SMALL || mode == CRH_SCHEDULE_STAGED ? (1u << 30) : c->auto_lane_max_paths);
  c->frame_kernel = mode == CRH_SCHEDULE_STAGED ? false : c->auto_frame_kernel;
  c->donate = mode == CRH_SCHEDULE_WIDE ? false : c->auto_donate;
  c->pipeline = mode == CRH_SCHEDULE_WIDE ? false : c->auto_pipeline;
  return CRH_OK;
}

int crh_set_pipeline_depth(crh_ctx* c, uint32_t frames)
{
  if (!c || frames < 2u || frames > 8u) return fail(c, CRH_E_INVALID, "pipeline depth must be in 2 .. 8 frames");
  if (frames > pipeline_capacity()) {
    char b[320]; snprintf(b, sizeof b, "pipeline depth %u needs GPU_MAX_HW_QUEUES >= %u in the environment before the process's first HIP call: this process has %d "
                          "hardware queues, i.e. at most %u frames in flight (crh_query_pipeline_capacity)", frames, frames + 2u, hw_queues(), pipeline_capacity());
    return fail(c, CRH_E_INVALID, b);
  }
  CRH_HIP(hipSetDevice(c->device));
  CRH_HIP(hipStreamSynchronize(cstream(c)));            // the frames in flight own slices of the path state laid out for the old depth
  c->pipe_depth = frames; c->pipe.pipe_seq = 0; c->pipe.pipe_total = 0;
  return CRH_OK;
}

int crh_get_tile_stats(crh_ctx* c, float* err, uint32_t* counts, uint32_t* n_tiles)
{
  if (!c || !c->d_accum) return fail(c, CRH_E_INVALID, "no accumulator");
  CRH_HIP(hipSetDevice(c->device));
  std::vector<float> e; std::vector<uint32_t> n;
  int rc = tile_stats(c, e, n); if (rc) return rc;
  if (n_tiles) *n_tiles = (uint32_t)e.size();
  if (err) std::memcpy(err, e.data(), sizeof(float) * e.size());
  if (counts) std::memcpy(counts, n.data(), sizeof(uint32_t) * n.size());
  return CRH_OK;
}

int crh_enable_counters(crh_ctx* c, int on) { if (!c) return CRH_E_INVALID; c->counters_on = on != 0; return CRH_OK; }

int crh_enable_kernel_timing(crh_ctx* c, int on) { if (!c) return CRH_E_INVALID; c->timing_on = on != 0; return CRH_OK; }

}  // extern "C"
