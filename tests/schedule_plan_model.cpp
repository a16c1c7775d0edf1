// schedule_plan_model.cpp -- the CPU check of cadrays_amd/csrc/crh_plan.h (run by tests/test_schedule_plan.py under ASan + UBSan; includes nothing else of the library):
//   (a) an ordering model of the frame pipeline: what plan_frame / join_pending decide is executed on a graph of stream-ordered nodes, as crh_schedule.cpp executes it on
//       HIP streams, and the orderings the path state and the accumulator depend on are checked -- exhaustively over short call sequences, then over random long ones;
//   (b) pinned values of the pure formulas (computed from the expressions as they stood inline in crh_schedule.cpp before crh_plan.h existed);
//   (c) order_tiles on small cases.
// Arguments: the 16 frame seeds of seed 1 (tests/golden/math.npz).  Exit status 0 and a last line "ok ..." when everything holds.
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "crh_plan.h"

using namespace crh::plan;

static int g_failures = 0;
static void fail(const std::string& what) { if (++g_failures <= 10) fprintf(stderr, "FAIL %s\n", what.c_str()); }
#define EXPECT(cond, what) do { if (!(cond)) fail(std::string(what) + "  [" #cond "]"); } while (0)

// ================================================================================================ (a) the ordering model
// A node is one piece of device work (or, `marker`, a recorded event); it starts after the node before it on its stream and after every event its stream was made to
// wait for.  `done`: the fake device has finished it -- only ever together with everything in front of it; an event is done exactly when what it follows is.
// a happens before b: a is in front of b in the graph, or a was done when b was submitted.
constexpr int kMaxNodes = 384;
constexpr uint64_t kA = 1089536u;      // 1216 x 896 at one sample: the smallest frame the pipeline takes
enum Stream { kContext = 8, kReadback = 9, kStreams = 10 };
struct Node { std::bitset<kMaxNodes> in_front; int pred[12], n_pred = 0; bool marker = false, done = false; int born = 0, done_at = 0; };
struct Frame { int T, A, J; uint64_t base, total; };

struct Model {
  // the configuration and the context's fields of the same names
  uint32_t depth = 3, frame_pipe_depth = 2; bool frame_able = true; uint64_t path_cap = 0;
  PipeState pipe; uint64_t stream_uses = 0; uint32_t counter_epoch = 0;
  bool read_since_render = true, reset_pending = false, rb_guard_pending = false, lanes = false;
  int lane_join[8] = {-1, -1, -1, -1, -1, -1, -1, -1}, lane_fork = -1, pipe_resized = -1, reset_ev = -1, rb_guard = -1, counters_zeroed[4] = {-1, -1, -1, -1};
  // the graph
  std::vector<Node> nodes; int tail[kStreams]; int waits[kStreams][12], n_waits[kStreams] = {}; int now = 0;
  std::vector<Frame> frames; std::vector<int> inputs, restarts, readbacks;      // nodes on the context's stream a frame's tracing reads; restarts no frame has followed yet
  std::string config; char calls[64]; int n_calls = 0;                           // the calls so far, for messages
  uint32_t probes_frame = 0, probes_resized = 0;

  Model() { for (int& t : tail) t = -1; }
  void note(char call) { if (n_calls < 64) calls[n_calls++] = call; }
  std::string trace() const
  {
    std::string t = " " + config;
    for (int i = 0; i < n_calls; ++i) {
      const char c = calls[i];
      t += c == 'u' ? " use" : c == 'r' ? " restart" : c == 'w' ? " wide" : c == 'b' ? " readback" : c == 'f' ? " finish-oldest" : c == 'F' ? " finish-all" : c == 'g' ? " grow" :
           c >= '1' && c <= '3' ? std::string(" frame") + c : std::string(" depth") + (char)(c - 'A' + '0');
    }
    return t;
  }

  // ---- streams and events
  int add(int s, bool marker)
  {
    Node n; n.marker = marker; n.born = ++now;
    if (tail[s] >= 0) n.pred[n.n_pred++] = tail[s];
    for (int i = 0; i < n_waits[s]; ++i) if (n.n_pred < 12) n.pred[n.n_pred++] = waits[s][i]; else fail("model: too many waits on one node");
    n_waits[s] = 0;
    bool all_done = true;
    for (int i = 0; i < n.n_pred; ++i) { n.in_front |= nodes[n.pred[i]].in_front; n.in_front.set(n.pred[i]); all_done = all_done && nodes[n.pred[i]].done; }
    if (marker && all_done) { n.done = true; n.done_at = now; }
    if ((int)nodes.size() >= kMaxNodes) { fail("model: sequence too long for kMaxNodes"); exit(2); }
    nodes.push_back(n); tail[s] = (int)nodes.size() - 1;
    return tail[s];
  }
  void wait(int s, int event) { if (event >= 0 && n_waits[s] < 12) waits[s][n_waits[s]++] = event; }      // hipStreamWaitEvent (an event never recorded: no wait)
  int record(int s) { return add(s, true); }                                       // hipEventRecord
  void settle() { for (Node& n : nodes) if (n.marker && !n.done) { bool all = true; for (int i = 0; i < n.n_pred; ++i) all = all && nodes[n.pred[i]].done; if (all) { n.done = true; n.done_at = now; } } }
  void finish(int x)                                                               // the device has finished x: and so everything in front of it
  {
    ++now;
    for (int i = 0; i <= x; ++i) if ((i == x || nodes[x].in_front[i]) && !nodes[i].done) { nodes[i].done = true; nodes[i].done_at = now; }
    settle();
  }
  bool before(int a, int b) const { return nodes[b].in_front[a] || (nodes[a].done && nodes[a].done_at <= nodes[b].born); }

  // ---- the context's stream as crh_context.h cstream() hands it out
  int cstream()
  {
    join_pending(pipe, [&](uint32_t k) { wait(kContext, lane_join[k]); });
    if (rb_guard_pending) { wait(kContext, rb_guard); rb_guard_pending = false; }
    read_since_render = true; ++stream_uses;
    return kContext;
  }
  void sync_context() { const int s = cstream(); finish(record(s)); }             // hipStreamSynchronize(cstream(c))

  // ---- the operations
  void use_context() { note('u'); inputs.push_back(add(cstream(), false)); }      // an upload, a new tile list: something a frame's tracing reads
  void restart()                                                                     // do_reset
  {
    note('r');
    const uint64_t uses = stream_uses;
    const int cs = cstream();
    restarts.push_back(add(cs, false));                                              // the accumulator's memsets
    reset_ev = record(cs); reset_pending = true;
    const uint32_t next = (++counter_epoch + 1u) & 3u;
    add(cs, false); counters_zeroed[next] = record(cs);                              // the counter block of the restart after this one
    stream_uses = uses;                                                              // none of this is input of a frame's tracing
  }
  void wide(uint64_t size)                                                           // render_batches: one batch on the context's stream that owns [0, size) of the path state
  {
    if (size > path_cap) { sync_context(); path_cap = size; }
    const int w = add(cstream(), false);
    for (const Frame& f : frames) if (f.base < size) EXPECT(before(f.J, w), "invariant 1 (wide batch over a frame in flight) after" + trace());
    inputs.push_back(w);
    read_since_render = false;
  }
  void readback()                                                                    // crh_read_ldr_begin: tone map on a stream of its own behind everything submitted so far
  {
    note('b');
    for (int k = 0; k < 8; ++k) if (pipe.pipe_pending[k]) wait(kReadback, lane_join[k]);
    wait(kReadback, record(kContext));
    const int r = add(kReadback, false);
    for (const Frame& f : frames) EXPECT(before(f.A, r), "read-back shows every frame submitted before it, after" + trace());
    readbacks.push_back(r);
    rb_guard = record(kReadback); rb_guard_pending = true;
  }
  void finish_oldest() { note('f'); for (const Frame& f : frames) if (!nodes[f.J].done) { finish(f.A); return; } }
  void finish_all() { note('F'); ++now; for (Node& n : nodes) if (!n.done) { n.done = true; n.done_at = now; } }
  void set_depth(uint32_t d) { note((char)('A' + d)); sync_context(); depth = d; pipe.pipe_seq = 0; pipe.pipe_total = 0; }      // crh_set_pipeline_depth
  void grow_paths() { note('g'); sync_context(); }                           // ensure_paths when the buffers must grow

  struct Probe {
    Model* m;
    bool frame_done(uint32_t j) { ++m->probes_frame; return m->nodes[m->lane_join[j]].done; }
    bool resized_done() { ++m->probes_resized; return m->nodes[m->pipe_resized].done; }
  };

  void frame(uint32_t mult)                                                          // one Redraw() of mult samples: render_impl with a frame the pipeline takes
  {
    note((char)('0' + mult));
    const uint64_t total = mult * kA;
    const bool host_runs_ahead = !read_since_render;
    if (!(host_runs_ahead || frame_able)) { wide(total); return; }                  // the two-range schedule on the context's stream
    if (depth * total > path_cap) { sync_context(); path_cap = depth * total; }     // ensure_paths
    if (!lanes) { inputs.push_back(add(cstream(), false)); lanes = true; }          // ensure_lanes: the lanes' counter blocks are zeroed on the context's stream
    uint32_t were_running = 0; for (bool r : pipe.pipe_running) were_running += r ? 1u : 0u;
    const bool may_ask_resized = pipe.pipe_resized_pending && total == pipe.pipe_total && depth == pipe.pipe_last_depth;
    probes_frame = probes_resized = 0;
    const FramePlan fp = plan_frame(pipe, {total, depth, frame_pipe_depth, stream_uses, counter_epoch, frame_able, host_runs_ahead}, Probe{this});
    EXPECT(probes_frame == were_running && probes_resized <= (may_ask_resized ? 1u : 0u), "plan_frame asks about each running frame once and about pipe_resized only while it is pending, after" + trace());
    EXPECT(fp.k < depth && fp.prev < depth && fp.k != fp.prev && fp.base == fp.k * total && (uint64_t)fp.base + total <= path_cap, "stream and slice of the frame after" + trace());
    // the execution, as render_pipelined_frame enqueues it
    const int s = (int)fp.k;
    if (fp.fork) { lane_fork = record(kContext); wait(s, lane_fork); }
    for (uint32_t j = 0; j < 8u; ++j) if (fp.wait_joins >> j & 1u) wait(s, lane_join[j]);
    if (fp.wait_counters_zeroed) wait(s, counters_zeroed[counter_epoch & 3u]);
    if (fp.resized == FramePlan::kRecord) pipe_resized = record(s);
    else if (fp.resized == FramePlan::kWait) wait(s, pipe_resized);
    Frame f; f.base = fp.base; f.total = total;
    f.T = add(s, false);
    if (fp.after_prev) wait(s, lane_join[fp.prev]);
    if (rb_guard_pending) { wait(s, rb_guard); rb_guard_pending = false; }
    if (reset_pending) { wait(s, reset_ev); reset_pending = false; }
    f.A = add(s, false);
    f.J = lane_join[fp.k] = record(s);
    frame_submitted(pipe, fp.k);
    read_since_render = false;
    // what must hold
    for (const Frame& e : frames) {
      if (e.base < f.base + f.total && f.base < e.base + e.total) EXPECT(before(e.J, f.T), "invariant 1 (overlapping slices are ordered) after" + trace());
      EXPECT(before(e.A, f.A), "invariant 2 (accumulation in frame order) after" + trace());
    }
    for (int n : inputs) EXPECT(before(n, f.T), "invariant 3 (tracing behind its inputs on the context's stream) after" + trace());
    for (int n : restarts) EXPECT(before(n, f.A), "invariant 4 (accumulate behind the restart) after" + trace());
    restarts.clear();
    for (int n : readbacks) EXPECT(before(n, f.A), "accumulate behind a read-back's tone map, after" + trace());
    frames.push_back(f);
  }

  enum { kOps = 13 };
  void op(int i)
  {
    switch (i) {
      case 0: case 1: case 2: frame((uint32_t)i + 1u); break;
      case 3: use_context(); break;
      case 4: restart(); break;
      case 5: note('w'); wide(16u * kA); break;
      case 6: finish_oldest(); break;
      case 7: finish_all(); break;
      case 8: set_depth(2); break;
      case 9: set_depth(3); break;
      case 10: set_depth(8); break;
      case 11: grow_paths(); break;
      default: readback(); break;
    }
  }
};

static uint64_t g_sequences = 0;
static void exhaust(const Model& m, const std::vector<int>& ops, int left)      // every sequence of `left` calls out of `ops`
{
  if (left == 0 || g_failures) { ++g_sequences; return; }
  for (int i : ops) { Model n = m; n.op(i); exhaust(n, ops, left - 1); }
}

static Model configured(uint32_t depth, bool frame_able, bool roomy)
{
  Model m; m.depth = depth; m.frame_able = frame_able; m.path_cap = roomy ? 64u * kA : 0u;      // roomy: the path state never has to grow (growing waits for the device)
  m.config = "[depth " + std::to_string(depth) + (frame_able ? ", frame kernel" : ", staged") + (roomy ? ", roomy]" : "]");
  return m;
}

static void ordering_model()
{
  // the sequence of tests/hunts/tile_order_sequences.py seed 166: one frame of two samples, then three of one, nothing finished in between (the pipeline stood at its
  // fourth stream: the third one-sample frame's slice [6 A, 7 A) lies inside the two-sample frame's [6 A, 8 A))
  for (int fa = 0; fa < 2; ++fa) {
    Model m = configured(8, fa != 0, true); m.config += " seed 166:"; m.pipe.pipe_seq = 3; m.read_since_render = false;
    m.frame(2); m.frame(1); m.frame(1); m.frame(1);
    EXPECT(m.frames[3].base == 6u * kA && m.frames[0].base == 6u * kA && !m.nodes[m.frames[0].J].done, "the seed-166 sequence lays the fourth frame's slice inside the first one's");
  }
  {   // the first frame after a restart traces at once: it is not planned to wait for the memsets
    Model m = configured(2, true, true);      // (two streams, both have forked from the context's stream before)
    m.frame(1); m.frame(1); m.restart(); const int r = m.restarts.back(); m.frame(1);
    EXPECT(!m.before(r, m.frames.back().T) && m.before(r, m.frames.back().A), "invariant 4: the first frame after a restart waits with its accumulate only");
  }
  // every sequence of four calls; of five without the calls that wait for the device; of six frames, restarts, uploads and finished frames where nothing has to grow
  for (uint32_t depth : {2u, 3u, 8u}) for (int fa = 0; fa < 2; ++fa) for (int roomy = 0; roomy < 2; ++roomy) {
    const Model m = configured(depth, fa != 0, roomy != 0);
    exhaust(m, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, 4);
    exhaust(m, {0, 1, 2, 3, 4, 6, 12}, 5);
    if (roomy) exhaust(m, {0, 1, 3, 4, 6}, 6);
  }
  // longer walks: fixed seed; frames three times as likely as anything else, so that the pipeline fills
  std::mt19937 rng(20250166u);
  for (int walk = 0; walk < 400 && !g_failures; ++walk) {
    const uint32_t depths[3] = {2u, 3u, 8u}, pick = (uint32_t)rng();
    Model m = configured(depths[pick % 3u], (pick & 4u) != 0, (pick & 8u) != 0);
    m.frame_pipe_depth = 1u + rng() % 3u;
    for (int step = 0; step < 48; ++step) { const uint32_t r = rng() % 39u; m.op(r < 26u ? (int)(r % 3u) : (int)(r - 26u)); }
    ++g_sequences;
  }
}

// ================================================================================================ (b) pinned values
struct SmallGridRow { uint64_t paths; int full, per, want; };
static const SmallGridRow kSmallGrid[] = {
  {262144ull, 1024, 1024, 512},
  {262144ull, 1024, 2048, 512},
  {262144ull, 1536, 1024, 512},
  {262144ull, 1536, 2048, 512},
  {1048576ull, 1024, 1024, 1024},
  {1048576ull, 1024, 2048, 512},
  {1048576ull, 1536, 1024, 1024},
  {1048576ull, 1536, 2048, 512},
  {1089536ull, 1024, 1024, 1024},
  {1089536ull, 1024, 2048, 532},
  {1089536ull, 1536, 1024, 1064},
  {1089536ull, 1536, 2048, 532},
  {2073600ull, 1024, 1024, 1024},
  {2073600ull, 1024, 2048, 1012},
  {2073600ull, 1536, 1024, 1536},
  {2073600ull, 1536, 2048, 1012},
  {3145728ull, 1024, 1024, 1024},
  {3145728ull, 1024, 2048, 1024},
  {3145728ull, 1536, 1024, 1536},
  {3145728ull, 1536, 2048, 1536},
  {8388608ull, 1024, 1024, 1024},
  {8388608ull, 1024, 2048, 1024},
  {8388608ull, 1536, 1024, 1536},
  {8388608ull, 1536, 2048, 1536},
};
// grid 1024, grid_trace 1536, floors 192 / 512, pipe_div 4096
struct PipeGridRow { uint64_t total; uint32_t running; int own_running; uint32_t depth, frame_pipe_depth; int frame, burst, grid, grid_trace; uint32_t share; };
static const PipeGridRow kPipeGrid[] = {
  {1089536ull, 0, 0, 3, 2u, 0, 0, 532, 512, 1u},
  {1089536ull, 1, 1, 3, 2u, 0, 0, 532, 512, 1u},
  {1089536ull, 0, 0, 8, 2u, 0, 1, 532, 266, 2u},
  {1089536ull, 0, 0, 3, 2u, 1, 1, 532, 512, 1u},
  {1089536ull, 1, 0, 3, 2u, 0, 0, 532, 512, 2u},
  {1089536ull, 2, 0, 3, 2u, 0, 0, 532, 512, 2u},
  {1089536ull, 3, 1, 3, 2u, 0, 0, 532, 512, 2u},
  {1089536ull, 2, 0, 8, 2u, 0, 1, 532, 266, 2u},
  {1089536ull, 2, 0, 3, 2u, 1, 1, 532, 512, 2u},
  {1089536ull, 3, 0, 3, 2u, 0, 0, 532, 384, 2u},
  {1089536ull, 5, 0, 3, 2u, 0, 0, 532, 266, 2u},
  {1089536ull, 6, 1, 3, 2u, 0, 0, 532, 266, 2u},
  {1089536ull, 5, 0, 8, 2u, 0, 1, 532, 266, 2u},
  {1089536ull, 5, 0, 3, 2u, 1, 1, 532, 266, 2u},
  {1089536ull, 7, 0, 3, 2u, 0, 0, 532, 266, 2u},
  {2073600ull, 0, 0, 3, 2u, 0, 0, 1012, 512, 1u},
  {2073600ull, 1, 1, 3, 2u, 0, 0, 1012, 512, 1u},
  {2073600ull, 0, 0, 8, 2u, 0, 1, 1012, 506, 2u},
  {2073600ull, 0, 0, 3, 2u, 1, 1, 1012, 512, 1u},
  {2073600ull, 1, 0, 3, 2u, 0, 0, 1012, 512, 2u},
  {2073600ull, 2, 0, 3, 2u, 0, 0, 1012, 512, 2u},
  {2073600ull, 3, 1, 3, 2u, 0, 0, 1012, 512, 2u},
  {2073600ull, 2, 0, 8, 2u, 0, 1, 1012, 506, 2u},
  {2073600ull, 2, 0, 3, 2u, 1, 1, 1012, 512, 2u},
  {2073600ull, 3, 0, 3, 2u, 0, 0, 1012, 506, 2u},
  {2073600ull, 5, 0, 3, 2u, 0, 0, 1012, 506, 2u},
  {2073600ull, 6, 1, 3, 2u, 0, 0, 1012, 506, 2u},
  {2073600ull, 5, 0, 8, 2u, 0, 1, 1012, 506, 2u},
  {2073600ull, 5, 0, 3, 2u, 1, 1, 1012, 506, 2u},
  {2073600ull, 7, 0, 3, 2u, 0, 0, 1012, 506, 2u},
  {8294400ull, 0, 0, 3, 2u, 0, 0, 1024, 1536, 1u},
  {8294400ull, 1, 1, 3, 2u, 0, 0, 1024, 1536, 1u},
  {8294400ull, 0, 0, 8, 2u, 0, 1, 1024, 1536, 2u},
  {8294400ull, 0, 0, 3, 2u, 1, 1, 1024, 1536, 1u},
  {8294400ull, 1, 0, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 2, 0, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 3, 1, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 2, 0, 8, 2u, 0, 1, 1024, 1536, 2u},
  {8294400ull, 2, 0, 3, 2u, 1, 1, 1024, 1536, 2u},
  {8294400ull, 3, 0, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 5, 0, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 6, 1, 3, 2u, 0, 0, 1024, 1536, 2u},
  {8294400ull, 5, 0, 8, 2u, 0, 1, 1024, 1536, 2u},
  {8294400ull, 5, 0, 3, 2u, 1, 1, 1024, 1536, 2u},
  {8294400ull, 7, 0, 3, 2u, 0, 0, 1024, 1536, 2u},
};
struct CutRow { uint32_t nt, tpp, ns, budget; int packets, counters_on; uint32_t lane_max_paths, group, spb; };
static const CutRow kCut[] = {
  {2040u, 1024u, 1u, 536870912u, 64, 0, 12582912u, 2040u, 1u},
  {2040u, 1024u, 16u, 536870912u, 64, 0, 12582912u, 2040u, 16u},
  {2040u, 1024u, 16u, 16777216u, 64, 0, 12582912u, 2040u, 8u},
  {2040u, 1024u, 16u, 536870912u, 0, 0, 12582912u, 2040u, 16u},
  {2040u, 1024u, 16u, 536870912u, 64, 1, 12582912u, 2040u, 16u},
  {2040u, 1024u, 16u, 1048576u, 64, 0, 12582912u, 1024u, 1u},
  {2040u, 1024u, 63u, 536870912u, 64, 0, 12582912u, 2040u, 63u},
  {2040u, 1024u, 64u, 536870912u, 64, 0, 12582912u, 2040u, 64u},
  {2040u, 1024u, 96u, 536870912u, 64, 0, 12582912u, 2040u, 64u},
  {2040u, 1024u, 512u, 536870912u, 64, 0, 12582912u, 1024u, 512u},
  {2040u, 1024u, 512u, 16777216u, 64, 0, 12582912u, 256u, 64u},
  {2040u, 1024u, 512u, 536870912u, 0, 0, 12582912u, 2040u, 257u},
  {2040u, 1024u, 512u, 536870912u, 64, 1, 12582912u, 2040u, 257u},
  {2040u, 1024u, 512u, 1048576u, 64, 0, 12582912u, 16u, 64u},
  {2040u, 1024u, 700u, 536870912u, 64, 0, 12582912u, 819u, 640u},
  {2040u, 1024u, 700u, 16777216u, 64, 0, 12582912u, 256u, 64u},
  {2040u, 1024u, 700u, 536870912u, 0, 0, 12582912u, 2040u, 257u},
  {2040u, 1024u, 700u, 536870912u, 64, 1, 12582912u, 2040u, 257u},
  {2040u, 1024u, 700u, 1048576u, 64, 0, 12582912u, 16u, 64u},
  {2040u, 1024u, 4096u, 536870912u, 64, 0, 12582912u, 512u, 1024u},
  {32400u, 64u, 1u, 536870912u, 64, 0, 12582912u, 32400u, 1u},
  {32400u, 64u, 16u, 536870912u, 64, 0, 12582912u, 32400u, 16u},
  {32400u, 64u, 16u, 16777216u, 64, 0, 12582912u, 32400u, 8u},
  {32400u, 64u, 16u, 536870912u, 0, 0, 12582912u, 32400u, 16u},
  {32400u, 64u, 16u, 536870912u, 64, 1, 12582912u, 32400u, 16u},
  {32400u, 64u, 16u, 1048576u, 64, 0, 12582912u, 16384u, 1u},
  {32400u, 64u, 63u, 536870912u, 64, 0, 12582912u, 32400u, 63u},
  {32400u, 64u, 64u, 536870912u, 64, 0, 12582912u, 32400u, 64u},
  {32400u, 64u, 96u, 536870912u, 64, 0, 12582912u, 32400u, 64u},
  {32400u, 64u, 512u, 536870912u, 64, 0, 12582912u, 16384u, 512u},
  {32400u, 64u, 512u, 16777216u, 64, 0, 12582912u, 512u, 512u},
  {32400u, 64u, 512u, 536870912u, 0, 0, 12582912u, 32400u, 258u},
  {32400u, 64u, 512u, 536870912u, 64, 1, 12582912u, 32400u, 258u},
  {32400u, 64u, 512u, 1048576u, 64, 0, 12582912u, 256u, 64u},
  {32400u, 64u, 700u, 536870912u, 64, 0, 12582912u, 13107u, 640u},
  {32400u, 64u, 700u, 16777216u, 64, 0, 12582912u, 409u, 640u},
  {32400u, 64u, 700u, 536870912u, 0, 0, 12582912u, 32400u, 258u},
  {32400u, 64u, 700u, 536870912u, 64, 1, 12582912u, 32400u, 258u},
  {32400u, 64u, 700u, 1048576u, 64, 0, 12582912u, 256u, 64u},
  {32400u, 64u, 4096u, 536870912u, 64, 0, 12582912u, 8192u, 1024u},
  {510u, 4096u, 1u, 536870912u, 64, 0, 12582912u, 510u, 1u},
  {510u, 4096u, 16u, 536870912u, 64, 0, 12582912u, 510u, 16u},
  {510u, 4096u, 16u, 16777216u, 64, 0, 12582912u, 510u, 8u},
  {510u, 4096u, 16u, 536870912u, 0, 0, 12582912u, 510u, 16u},
  {510u, 4096u, 16u, 536870912u, 64, 1, 12582912u, 510u, 16u},
  {510u, 4096u, 16u, 1048576u, 64, 0, 12582912u, 256u, 1u},
  {510u, 4096u, 63u, 536870912u, 64, 0, 12582912u, 510u, 63u},
  {510u, 4096u, 64u, 536870912u, 64, 0, 12582912u, 510u, 64u},
  {510u, 4096u, 96u, 536870912u, 64, 0, 12582912u, 510u, 64u},
  {510u, 4096u, 512u, 536870912u, 64, 0, 12582912u, 256u, 512u},
  {510u, 4096u, 512u, 16777216u, 64, 0, 12582912u, 64u, 64u},
  {510u, 4096u, 512u, 536870912u, 0, 0, 12582912u, 510u, 257u},
  {510u, 4096u, 512u, 536870912u, 64, 1, 12582912u, 510u, 257u},
  {510u, 4096u, 512u, 1048576u, 64, 0, 12582912u, 4u, 64u},
  {510u, 4096u, 700u, 536870912u, 64, 0, 12582912u, 409u, 320u},
  {510u, 4096u, 700u, 16777216u, 64, 0, 12582912u, 64u, 64u},
  {510u, 4096u, 700u, 536870912u, 0, 0, 12582912u, 510u, 257u},
  {510u, 4096u, 700u, 536870912u, 64, 1, 12582912u, 510u, 257u},
  {510u, 4096u, 700u, 1048576u, 64, 0, 12582912u, 4u, 64u},
  {510u, 4096u, 4096u, 536870912u, 64, 0, 12582912u, 256u, 512u},
};

static void pinned_values(int argc, char** argv)
{
  for (const SmallGridRow& r : kSmallGrid) EXPECT(small_grid(r.paths, r.full, r.per) == r.want, "small_grid(" + std::to_string(r.paths) + ", " + std::to_string(r.full) + ", " + std::to_string(r.per) + ")");
  for (const PipeGridRow& r : kPipeGrid) {
    const PipeGrids g = pipe_grids({1024, 1536, 192, 512, 4096, r.total, r.running, r.own_running != 0, r.depth, r.frame_pipe_depth, r.frame != 0, r.burst != 0});
    EXPECT(g.grid == r.grid && g.grid_trace == r.grid_trace && g.share == r.share, "pipe_grids(total " + std::to_string(r.total) + ", running " + std::to_string(r.running) + ") = " +
           std::to_string(g.grid) + " / " + std::to_string(g.grid_trace) + " / " + std::to_string(g.share));
  }
  for (const CutRow& r : kCut) {
    const CallCut cut = cut_call(r.nt, r.tpp, r.ns, r.budget, r.packets, r.counters_on != 0, r.lane_max_paths);
    EXPECT(cut.group == r.group && cut.spb == r.spb, "cut_call(" + std::to_string(r.nt) + ", " + std::to_string(r.tpp) + ", " + std::to_string(r.ns) + ", " + std::to_string(r.budget) + ") = (" +
           std::to_string(cut.group) + ", " + std::to_string(cut.spb) + ")");
  }
  EXPECT(tile_count(1920, 1080, 32) == 2040u && tile_count(1216, 896, 32) == 1064u && tile_count(3840, 2160, 8) == 129600u && tile_count(65, 33, 32) == 6u && tile_count(64, 64, 32) == 4u, "tile_count");
  uint32_t golden[16], got[16];
  EXPECT(argc == 17, "usage: schedule_plan_model <the 16 frame seeds of seed 1>");
  for (int i = 0; i < 16 && i + 1 < argc; ++i) golden[i] = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
  frame_seeds(1, 0, 16, got);
  for (int i = 0; i < 16 && argc == 17; ++i) EXPECT(got[i] == golden[i], "frame_seeds(1, 0, 16)[" + std::to_string(i) + "] = " + std::to_string(got[i]));
  for (uint32_t seed : {0u, 1u, 7u, 0xFFFFFFFFu, 0x49616E42u}) for (uint32_t first : {0u, 1u, 5u, 100u}) for (uint32_t n : {0u, 1u, 16u, 37u}) {
    std::vector<uint32_t> whole(first + n + 1u), part(n + 1u, 0xDEADBEEFu);
    frame_seeds(seed, 0, first + n, whole.data()); frame_seeds(seed, first, n, part.data());
    EXPECT(std::equal(part.begin(), part.begin() + n, whole.begin() + first) && part[n] == 0xDEADBEEFu, "frame_seeds(s, first, n) is the tail of frame_seeds(s, 0, first + n)");
  }
}

// ================================================================================================ (c) order_tiles, and the tally
static void tile_order_and_tally()
{
  std::mt19937 rng(7u);
  for (uint32_t nt : {1u, 2u, 7u, 64u, 1064u}) for (int kind = 0; kind < 4; ++kind) {
    std::vector<uint32_t> cost(nt);
    for (uint32_t t = 0; t < nt; ++t) cost[t] = kind == 0 ? 1000u : kind == 1 ? (uint32_t)(rng() % 5u) * 100u : kind == 2 ? (uint32_t)rng() : t == nt / 2u ? 0xFFFFFFFFu : (uint32_t)(rng() % 1000u);
    if (kind == 1) cost[0] = 400u;      // never all zero
    std::vector<uint8_t> cls; std::vector<uint32_t> order;
    EXPECT(order_tiles(cost.data(), nt, cls, order) && cls.size() == nt && order.size() == nt, "order_tiles makes a first list");
    std::vector<uint8_t> seen(nt, 0); bool permutation = order.size() == nt;
    for (uint32_t t : order) { if (t >= nt || seen[t]) { permutation = false; break; } seen[t] = 1; }
    EXPECT(permutation, "order_tiles: a permutation");
    if (!permutation) continue;
    uint32_t top = 1; for (uint32_t c : cost) top = std::max(top, c);
    EXPECT(cost[order[0]] == top || (uint64_t)cost[order[0]] * 255u / top == 255u, "order_tiles: the most expensive tile first");
    bool sorted = true;
    for (uint32_t i = 1; i < nt; ++i) {
      const uint64_t a = (uint64_t)cost[order[i - 1]] * 255u / top, b = (uint64_t)cost[order[i]] * 255u / top;      // the 256 levels the list is sorted by
      sorted = sorted && (a > b || (a == b && order[i - 1] < order[i]));
      if (cost[order[i - 1]] == cost[order[i]]) sorted = sorted && order[i - 1] < order[i];                           // equal costs stay row-major
    }
    EXPECT(sorted, "order_tiles: descending cost, row-major among equals");
    const std::vector<uint32_t> first = order; const std::vector<uint8_t> first_cls = cls;
    std::vector<uint32_t> noisy = cost;
    if (kind == 0) for (uint32_t& c : noisy) c += (uint32_t)(rng() % 50u);      // +- 5 % around the mean: no tile changes its class
    EXPECT(!order_tiles(noisy.data(), nt, cls, order) && order == first && cls == first_cls, "order_tiles: unchanged classes leave the list alone");
  }
  {
    std::vector<uint32_t> zero(16, 0u), order{3u, 1u}; std::vector<uint8_t> cls;
    EXPECT(!order_tiles(zero.data(), 16, cls, order) && order.size() == 2u && cls.empty(), "order_tiles: nothing traced, nothing ordered");
    const uint32_t cost[6] = {5u, 900u, 5u, 900u, 0u, 300u};
    EXPECT(order_tiles(cost, 6, cls, order) && order == std::vector<uint32_t>({1u, 3u, 5u, 0u, 2u, 4u}), "order_tiles: 5 900 5 900 0 300");
  }
  {   // events are numbers here; the even ones have finished, event e0 = 10 * k bracketed k ms
    Tally<int> t;
    t.pend.push_back({10, 2, 0}); t.pend.push_back({30, 4, 1}); t.pend.push_back({50, 6, -1}); t.pend.push_back({70, 7, 0}); t.pend.push_back({90, 8, 1});
    std::vector<int> released;
    auto harvest = [&] { t.harvest([](int e1) { return e1 % 2 == 0; }, [](int e0, int, float* ms) { *ms = e0 / 10.f; return e0 != 30; }, [&](int e) { released.push_back(e); }); };
    harvest();
    EXPECT(t.pend.size() == 2u && t.n[0] == 1u && t.n[1] == 0u && t.ms[0] == 1.0 && released == std::vector<int>({10, 2, 30, 4, 50, 6}), "Tally::harvest stops at the first pair still running");
    t.pend.front().e1 = 12; t.invalidate(); harvest();
    EXPECT(t.pend.empty() && t.n[0] == 1u && t.n[1] == 0u && released.size() == 10u, "Tally::invalidate: pending pairs no longer count");
    t.restart();
    EXPECT(t.n[0] == 0u && t.ms[0] == 0.0, "Tally::restart");
  }
}

int main(int argc, char** argv)
{
  ordering_model();
  pinned_values(argc, argv);
  tile_order_and_tally();
  if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
  printf("ok: %llu call sequences, %zu + %zu + %zu pinned rows\n", (unsigned long long)g_sequences, sizeof kSmallGrid / sizeof *kSmallGrid, sizeof kPipeGrid / sizeof *kPipeGrid, sizeof kCut / sizeof *kCut);
  return 0;
}
