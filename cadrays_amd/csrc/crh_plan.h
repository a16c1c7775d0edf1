// crh_plan.h -- the RULES of the frame schedule as pure functions over small plain structs: which stream, slice, waits and grids a Redraw() gets, how a
// wide call is cut, in which order a lone frame's tiles are claimed.  Plain C++17: no HIP header, no crh_ctx -- crh_schedule.cpp asks here and only executes
// the answer, and tests/schedule_plan_model.cpp checks the same code on the CPU (an ordering model of the pipeline, pinned values of the formulas).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <vector>

namespace crh {
namespace plan {

// frame seeds: Bullard generator restarted at `seed`, frame i uses next() >> 2; out[0 .. n) = the seeds of frames first .. first + n - 1
inline void frame_seeds(uint32_t seed, uint32_t first, uint32_t n, uint32_t* out)
{
  uint32_t hi = seed, lo = seed ^ 0x49616E42u;
  for (uint32_t i = 0; i < first + n; ++i) { hi = (hi >> 2) + (hi << 2); hi += lo; lo += hi; if (i >= first) out[i - first] = hi >> 2; }
}

inline uint32_t tile_count(uint32_t width, uint32_t height, uint32_t tile_size) { return ((width + tile_size - 1) / tile_size) * ((height + tile_size - 1) / tile_size); }

// A wide request that does not fit one batch is cut into TILE groups first and sample batches second: as many of the call's samples per batch as fit
// (multiples of 64, so that a wavefront is 64 samples of one pixel and the camera rays walk as packets; at most kBatchSamples), the tiles per batch follow
// (at least kBatchMinTiles).  The more samples of a pixel travel together, the more of their later bounces start from the same few triangles and the
// smaller the part of the tree a batch touches: on the 10 M-triangle tree at 4K 32 / 64 / 128 / 256 samples per batch give 2956 / 3301 / 3382 / 3410
// Mrays/s, on the 1 M-triangle one at 1080p 128 / 256 / 512 / 1024 give 4089 / 4145 / 4204 / 4224 (profiles/r4/ab_batch_shape.txt).  Samples of a pixel
// are folded in in the same order whatever the cut, so the frame does not change by a bit.
constexpr uint32_t kBatchSamples = 1024u, kBatchMinTiles = 256u;
struct CallCut { uint32_t group, spb; };      // tiles per batch, samples per batch
inline CallCut cut_call(uint32_t nt, uint32_t tpp, uint32_t ns, uint32_t budget, int packets, bool counters_on, uint32_t lane_max_paths)
{
  const uint32_t cap_tiles = std::max<uint32_t>(1u, budget / tpp);
  uint32_t group = std::min(nt, cap_tiles);
  uint32_t spb = std::max<uint32_t>(1u, std::min(ns, budget / (group * tpp)));
  if (packets > 0 && packets <= 64 && !counters_on && ns >= 64u && (uint64_t)nt * tpp * ns > lane_max_paths) {
    uint32_t want = std::min<uint32_t>(ns & ~63u, kBatchSamples);
    const uint32_t min_group = std::min<uint32_t>(nt, kBatchMinTiles);
    while (want > 64u && budget / (want * tpp) < min_group) want = (want / 2u) & ~63u;
    if (want >= 64u && budget / (want * tpp) >= 1u) {
      group = std::min(nt, budget / (want * tpp));
      spb = want;
      if (group == nt) spb = std::max<uint32_t>(want, std::min(ns, budget / (group * tpp)) & ~63u);
    }
  }
  return {group, spb};
}

// A persistent grid far larger than the batch only queues wavefronts for work fetches that return nothing (one cursor word
// sustains ~88 atomics/us: 6144 wavefronts = 70 us per launch): small batches get grids that follow their size.  Measured on
// C3 at 1080p, 1 spp per call: traversal grids of 1536 / 1024 / 768 / 512 workgroups -> 163 / 174 / 173 / 165 Redraw/s; 128
// tiles per call: 257 / 275 / 284 / 293 calls/s.
inline int small_grid(uint64_t paths, int full, int per) { return (int)std::min<uint64_t>((uint64_t)full, std::max<uint64_t>(512u, paths / (uint64_t)per)); }

// ---- the grids of a pipelined frame
struct PipeGridAsk {
  int grid, grid_trace, pipe_grid_min, pipe_grid_min_shade, pipe_div; uint64_t total;
  uint32_t running; bool own_running;      // frames found running at submission (FramePlan); this stream's own last frame among them
  uint32_t depth, frame_pipe_depth; bool frame, burst;      // frame: takes the frame kernel; burst: the previous frame was submitted under 300 us ago
};
struct PipeGrids { int grid, grid_trace; uint32_t share; };      // streaming grid, traversal grid, the frames a frame kernel shares the chip with
inline PipeGrids pipe_grids(const PipeGridAsk& a)
{
  PipeGrids g;
  g.grid = (int)std::min<uint64_t>((uint64_t)a.grid, std::max<uint64_t>((uint64_t)a.pipe_grid_min_shade, a.total / 2048u));
  // staged traversal grid of this frame: the chip's resident workgroups (6 per CU) shared among the frames that are in flight RIGHT NOW -- a host that runs far
  // ahead has pipe_depth of them (eight: 192 workgroups each), one that waits for every other frame's read-back has two or three (512 each); measured
  // optima at 3 / 4 / 6 / 8 frames in flight: 512 / 384 / 256 / 192-256 (profiles/r3/interactive_counters.txt)
  uint32_t in_flight = 1u + a.running - (a.own_running ? 1u : 0u);
  // a host that submitted the previous frame a moment ago is not waiting for anything: the pipeline is about to fill (counting what is in flight NOW
  // would give the first frames of a burst grids for a nearly empty chip: eight of them, 2900 workgroups)
  if (!a.frame && a.burst) in_flight = std::max(in_flight, a.depth);
  const uint64_t share = std::min<uint64_t>(512u, std::max<uint64_t>((uint64_t)a.pipe_grid_min, (uint64_t)a.grid_trace / in_flight));
  g.grid_trace = (int)std::min<uint64_t>((uint64_t)a.grid_trace, std::max<uint64_t>(share, a.total / (uint64_t)a.pipe_div));
  // frame kernel: one workgroup fills a compute unit, so the frames in flight share the chip by compute units (every frame asking for all of them was
  // measured: the second frame's workgroups then wait for whole workgroups of the first to leave -- 368 against 399 Redraw/s)
  g.share = std::min(in_flight, std::max(1u, a.frame_pipe_depth));
  return g;
}

// ---- the frame pipeline: what the rules below remember from one Redraw() to the next (a member of the context's ScheduleState)
struct PipeState {
  uint32_t pipe_seq = 0;             // pipelined frames submitted: frame n runs on stream n % depth and in slice [k * total, (k + 1) * total) of the path state
  uint64_t pipe_total = 0;           // batch size of the frames in flight (their path-state slices are laid out by it)
  uint32_t pipe_last_depth = 0;      // frames in flight the last pipelined frame was submitted with
  bool pipe_resized_pending = false; // the event "the last frame of the PREVIOUS batch size is done" has not been seen complete
  uint64_t lane_stream_uses[8] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};      // the count of context-stream uses at which each pipeline stream last forked from it
  uint32_t lane_counter_epoch[8] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};                    // the accumulation whose counter block each pipeline stream has waited for
  bool pipe_pending[8] = {false, false, false, false, false, false, false, false};      // a frame was submitted on that pipeline stream and the context's stream has not joined it
  bool pipe_running[8] = {false, false, false, false, false, false, false, false};      // ... and has not been seen finished (the frames-in-flight estimate)
  uint32_t last_running = 0;         // frames in flight when the last pipelined frame was submitted
};

// The context's stream joins lazily: whoever wants to enqueue on it, or wait for it, first makes it wait (wait(k): for lane_join[k]) for the frames still in flight.
template <class Wait> inline void join_pending(PipeState& p, Wait&& wait)
{
  for (uint32_t k = 0; k < 8u; ++k) if (p.pipe_pending[k]) { wait(k); p.pipe_pending[k] = false; }
}

struct FrameAsk {
  uint64_t total; uint32_t depth, frame_pipe_depth;      // paths of this frame; streams / path-state slices the frames rotate through; frame kernels that may run at a time
  uint64_t stream_uses; uint32_t counter_epoch;          // of the context, as they stand
  bool frame_able, host_runs_ahead;                      // the batch may take the frame kernel; nothing read or synchronised since the last render
};
struct FramePlan {
  uint32_t k, prev;                    // this frame's stream, the previous frame's
  size_t base;                         // first path slot of this frame's slice
  bool fork;                           // record lane_fork on the context's stream, the tracing waits for it
  bool frame;                          // the frame kernel (else the staged form)
  uint32_t wait_joins;                 // bit j: the tracing waits for lane_join[j]
  bool wait_counters_zeroed;           // ... and for counters_zeroed[counter_epoch & 3]
  enum Resized { kNone, kRecord, kWait } resized;      // ... then records pipe_resized on its stream, or waits for it
  bool after_prev;                     // the accumulate waits for lane_join[prev]
  uint32_t running; bool own_running;  // frames still running right now; this stream's own last frame among them
};

// Small whole-frame batches -- one Redraw() each -- are pipelined: frame n + 1 starts tracing on another stream and another slice of the path state while frame n
// finishes; accumulation stays in frame order.  probe.frame_done(j): has the frame last submitted on stream j finished?  probe.resized_done(): is pipe_resized
// complete?  Both are asked only when the answer is needed (the library: one hipEventQuery each).
template <class Probe> inline FramePlan plan_frame(PipeState& p, const FrameAsk& a, Probe&& probe)
{
  FramePlan f{};
  f.k = p.pipe_seq % a.depth; f.prev = (p.pipe_seq + a.depth - 1u) % a.depth;
  ++p.pipe_seq;
  f.base = (size_t)f.k * a.total;
  // What this frame's TRACING must wait for: whatever was enqueued on the context's stream since this pipeline stream last forked from it -- scene uploads, a new
  // tile list, a read-back's kernels.  A restart's memsets are not among them (do_reset): the first frame after crh_reset starts at once, only its accumulate
  // waits (reset_ev).  Per pipeline stream: the frame after the one that forked runs on ANOTHER stream and must see the same uploads.
  f.fork = a.stream_uses != p.lane_stream_uses[f.k];
  if (f.fork) p.lane_stream_uses[f.k] = a.stream_uses;
  // frames still running right now (this stream's own last frame included: this one queues behind it)
  for (uint32_t j = 0; j < 8u; ++j) if (p.pipe_running[j]) { if (probe.frame_done(j)) p.pipe_running[j] = false; else ++f.running; }
  p.last_running = f.running; f.own_running = p.pipe_running[f.k];
  // A frame takes the frame kernel when fewer than frame_pipe_depth frames are still running at its submission.
  f.frame = a.frame_able && (f.running < a.frame_pipe_depth || !a.host_runs_ahead);
  // a frame kernel wants compute units of its own: at most frame_pipe_depth of them run at a time (the frame submitted that many frames ago comes first;
  // measured with three in flight on halves of the chip: 272 against 379 frames/s in the drag loop)
  if (f.frame && a.frame_pipe_depth < a.depth) {
    const uint32_t j = (f.k + a.depth - std::max(1u, a.frame_pipe_depth)) % a.depth;
    if (p.pipe_running[j]) f.wait_joins |= 1u << j;
  }
  // this stream's first frame of an accumulation: the counter block was zeroed one restart ago, stream-ordered
  f.wait_counters_zeroed = p.lane_counter_epoch[f.k] != a.counter_epoch;
  p.lane_counter_epoch[f.k] = a.counter_epoch;
  // the frames in flight own path-state slices [k * total, (k + 1) * total): a batch of ANOTHER size (crh_render_tiles with another
  // sample count or tile list) would lay its slice across theirs -- it starts only when they are all done (joined into the context's stream or not)
  if (a.total != p.pipe_total || a.depth != p.pipe_last_depth) {
    for (uint32_t j = 0; j < 8u; ++j) if (p.pipe_running[j]) f.wait_joins |= 1u << j;
    p.pipe_total = a.total; p.pipe_last_depth = a.depth;
    // ... and so must every LATER frame of the new size: its slice may lie across a slice of the old size too, and it runs on another stream (round 6,
    // tests/hunts/tile_order_sequences.py seed 166: crh_render(2) followed at once by three one-sample frames -- the third one's slice [6.5 M, 7.6 M) lay inside the
    // two-sample frame's [6.5 M, 8.7 M) and nothing made it wait: a GPU memory fault).  One event, recorded behind the waits above, says "the old size is gone".
    f.resized = FramePlan::kRecord; p.pipe_resized_pending = true;
  } else if (p.pipe_resized_pending) {
    if (!probe.resized_done()) f.resized = FramePlan::kWait;
    else p.pipe_resized_pending = false;
  }
  f.after_prev = p.pipe_pending[f.prev];      // samples are folded in in frame order
  return f;
}
inline void frame_submitted(PipeState& p, uint32_t k) { p.pipe_pending[k] = true; p.pipe_running[k] = true; }      // lane_join[k] has been recorded behind the frame

// ---- the order a lone frame's tiles are claimed in (crh_context.h TileOrder).  cost[t]: rays of tile t in the last accumulation.  The classes only say WHEN to
// make a new list (noise between two frames of one view does not): false, and nothing written, while they are what `cls` holds.
inline bool order_tiles(const uint32_t* cost, uint32_t nt, std::vector<uint8_t>& cls, std::vector<uint32_t>& order)
{
  uint64_t sum = 0; for (uint32_t t = 0; t < nt; ++t) sum += cost[t];
  if (!sum) return false;
  const double mean = (double)sum / nt;
  std::vector<uint8_t> now(nt);
  for (uint32_t t = 0; t < nt; ++t) { const double x = cost[t] / mean; now[t] = x >= 2.0 ? 0 : x >= 1.25 ? 1 : x >= 0.75 ? 2 : x >= 0.4 ? 3 : 4; }
  if (now == cls) return false;
  // most rays first, row-major among equals: a counting sort over 256 levels of the cost (five classes in row-major order inside each class gain nothing
  // -- 2.27 against 2.30 ms on CAD1M -- the sorted list 2.16: profiles/r6/lone_frame.md 2c)
  uint32_t top = 1; for (uint32_t t = 0; t < nt; ++t) top = std::max(top, cost[t]);
  uint32_t at[258]; std::memset(at, 0, sizeof at);
  auto level = [&](uint32_t t) { return 255u - (uint32_t)(((uint64_t)cost[t] * 255u) / top); };      // 0 = the most expensive
  for (uint32_t t = 0; t < nt; ++t) ++at[level(t) + 1u];
  for (int k = 1; k < 258; ++k) at[k] += at[k - 1];
  order.resize(nt);
  for (uint32_t t = 0; t < nt; ++t) order[at[level(t)]++] = t;
  cls.swap(now);
  return true;
}

// ---- a two-sided measurement: event pairs (e0, e1) around the launches of setting 0 or 1 wait here until they have finished, then add to two running means
template <class Event> struct Tally {
  struct Pend { Event e0, e1; int which; };      // which < 0: bracketed a launch that no longer counts
  std::deque<Pend> pend; double ms[2] = {0.0, 0.0}; uint32_t n[2] = {0, 0};
  double mean(int which) const { return ms[which] / n[which]; }
  void invalidate() { for (Pend& q : pend) q.which = -1; }
  void restart() { n[0] = n[1] = 0; ms[0] = ms[1] = 0.0; invalidate(); }
  // done(e1): has the pair finished?  elapsed(e0, e1, &ms): its time, false if there is none.  release(e): the event goes back to its pool.
  template <class Done, class Elapsed, class Release> void harvest(Done&& done, Elapsed&& elapsed, Release&& release)
  {
    while (!pend.empty() && done(pend.front().e1)) {
      const Pend q = pend.front(); pend.pop_front();
      float t = 0.f;
      if (q.which >= 0 && elapsed(q.e0, q.e1, &t)) { ms[q.which] += t; ++n[q.which]; }
      release(q.e0); release(q.e1);
    }
  }
};

}  // namespace plan
}  // namespace crh
