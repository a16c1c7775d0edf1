// crh_context.h -- the context behind the C ABI of libcadrays_hip.so (include/cadrays_hip.h) and the helpers its translation units share.
//
//   crh_context.cpp    create / destroy, device-memory and event helpers, accumulator, crh_reset / crh_sync, the CRH_* environment table
//   crh_devmem.h       who owns device / pinned memory: Buf<T, Mem>, a pointer and its capacity that change together (no HIP, no context); the two HIP
//                      memory policies, DevBuf<T> and PinnedBuf<T> are below; checked on the CPU by tests/devmem_model.cpp
//   crh_scene.cpp      geometry, transforms, materials, lights, environment, textures, camera, params, spec; crh_build; the kernels' DScene
//   crh_plan.h         the RULES of the schedule as pure functions (no HIP, no context): frame seeds, the cut of a wide call, grids, the frame pipeline's plan,
//                      the tile order, the two-sided measurement tally; checked on the CPU by tests/schedule_plan_model.cpp
//   crh_schedule.cpp   the wavefront schedule: lanes, batches, frame pipelining, look-ahead, adaptive iterations -- asks crh_plan.h, enqueues the HIP work;
//                      crh_render / crh_render_tiles
//   crh_readback.cpp   HDR / LDR read-back (synchronous and asynchronous) and THE DISPLAY CHAIN both LDR read-outs enqueue (metering, reprojection, denoise filter,
//                      tone map, feature lines, overlay: enqueue_display_chain), accumulator checkpoints, statistics and kernel timing
//   crh_reduce.cpp     crh_reduce (RCCL over xGMI, or peer copies on one device)
//   crh_pick.cpp       the first-hit id buffer: camera rays, pick, id read-back, selection / hover state and bounds, the overlay of the LDR read-out
//   crh_fit.cpp        fit the view to the displayed / chosen objects: vertex extents on the device (fit_kernels.hip), the closed-form rule, the host-only twins
//   crh_region.cpp     region queries on the id buffer: rectangle / lasso selection, visible objects (region_kernels.hip), the host-only twin
//   crh_outline.cpp    feature lines on the LDR read-out: object, depth and crease edges from the id buffer (outline_kernels.hip), the host-only twins
//   crh_denoise.cpp    the denoised display: an id-guided a-trous filter in front of the LDR read-outs' tone map (denoise_kernels.hip), the host-only twin
//   crh_shade_guide.cpp  the shade guide of the denoised display: per pixel 1 / albedo and "a light shows here", the guided pass (shade_guide_kernels.hip), the
//                      host-only twins
//   crh_reproject.cpp  reprojected display history: the image an ending view displayed, blended into the next view's in front of the denoise filter
//                      (reproject_kernels.hip), the capture in crh_set_camera, the host-only twin
//   crh_view.cpp       the viewport read-out: the finished RGB8 frame resampled to the window's size as the LAST stage of the display chain (view_kernels.hip),
//                      the letterbox fit, the window-to-frame mapping, the host-only twin
//   crh_annotate.cpp   annotations: world-space line segments projected, binned and drawn over the frame as the last stage of the display chain, hidden or
//                      dimmed where the id buffer says the scene is nearer (annotate_kernels.hip), the queries, the host-only twins
//   crh_debug.cpp      API-level ray tracing, micro-benchmarks and the math / BSDF test hooks
//
// Shared by those, below: display_source (the image a read-out shows), grow_display_scratch, geometry_changed / geom_gen and side_upload (the tables derived from the
// geometry), DerivedStamp (what the outline mask and the denoise guide were computed from), camera_frame (the ONE copy of the camera basis), time_launches, aligned_copy
//
// This is the code that sits behind CADRays' `myInternal->View->Redraw()` (reference src/Launcher/AppViewer.cxx:1047).  There is NO CPU fallback:
// every entry point that renders or traces launches the gfx950 kernels and reports CRH_E_DEVICE when the HIP runtime refuses.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // types only: the library is loaded with dlopen on the first multi-device crh_reduce

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cadrays_hip.h"
#include "../../include/crh_xform.h"
#include "bvh_builder.h"
#include "crh_devmem.h"
#include "crh_plan.h"
#include "kernels.h"

namespace crh {

// ---- device and pinned host memory: the ONLY callers of the HIP allocator (crh_devmem.h; tests/test_cpu_host.py checks that).  A context's buffers are members
// of these types: they are released with it.  Synchronisation is not theirs: whoever makes a buffer grow first waits for what may still read it.
struct DeviceMem {
  using status = hipError_t; static constexpr status ok = hipSuccess;
  static status alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static status free(void* p) { return hipFree(p); }
};
struct PinnedMem {
  using status = hipError_t; static constexpr status ok = hipSuccess;
  static status alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static status free(void* p) { return hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

// ---- host copies of the inputs (what the setters received; crh_build and the per-frame setters work from these)
struct HostInputs {
  std::vector<float> pos, nrm, uv;
  std::vector<int32_t> tri;
  std::vector<crh_bsdf> mats;
  std::vector<crh_light> lights;
  std::vector<float> env; uint32_t envW = 0, envH = 0;
  struct HostTex { std::vector<float> rgba; uint32_t w = 0, h = 0; };
  std::vector<HostTex> textures; bool textures_dirty = false;
  crh_camera cam{};
  crh_params par{};
  crh_spec spec = CRH_SPEC_DEFAULTS;      // include/crh_spec.h
};

// ---- two-level mode (per-object transforms) and the static / moved split (reference: the gizmo moves ONE object per drag,
// ImRaytraceControls.cxx:64,88): every object is baked into one world-space tree with the transform it has when the scene is built; an object that is
// moved away from that placement has its triangles there disabled and gets an object tree of its own (built on first need, kept); nothing else is ever
// rebuilt by crh_set_transforms but the top-level tree
struct TwoLevelState {
  bool two_level = false; uint32_t nO = 0;
  std::vector<float> xf; std::vector<int32_t> tri_obj;
  std::vector<uint8_t> hidden;            // per object: 1 = erased from the view (crh_set_visibility); empty = all displayed
  std::vector<float> xf0, pos_w, nrm_w;   // the transforms the scene was built with; per vertex: position / unit normal under its object's build-time transform (what the static tree holds)
  struct Inst { float fwd[12], inv[12], bmin[3], bmax[3]; uint32_t root, obj; };
  std::vector<Inst> inst;                 // the objects rendered as instances RIGHT NOW, ascending object index (empty: the scene is one world-space tree)
  uint32_t n_blas_nodes = 0, root = 0;    // nodes of the static tree + the object trees built so far (the top-level tree follows them); entry point of the walk
  struct Obj { bool static0 = false, built = false, is_inst = false, in_static = false; uint32_t root = 0, first = 0, ntri = 0; float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0}; };
  std::vector<Obj> objs; std::vector<uint32_t> obj_tris, static_pos, pos_obj;   // pos_obj: object of the triangle at a leaf position >= n_static
  uint32_t n_static = 0, n_static_live = 0, n_pos = 0; float sbmin[3] = {0, 0, 0}, sbmax[3] = {0, 0, 0};
  uint32_t root2 = 0xFFFFFFFFu; float tlas_lo[3] = {0, 0, 0}, tlas_hi[3] = {0, 0, 0};
  size_t cap_pos = 0;                     // leaf positions the triangle / shading / uv / vertex arrays ALL have room for (each array knows its own size)
  DevBuf<void> d_patch;
  int split_passes = -1;                  // CRH_SPLIT_PASSES: -1 auto, 0 one walk, 1 two passes
  DevBuf<float4> d_ibox;                  // spheres around the instances' world boxes when there are at most kMaxIBox (the "does the ray come near a moved object" test)
  float usph[4] = {0.f, 0.f, 0.f, 0.f};  // ... and around the bounds of all of them
  DevBuf<float4> d_inst;
};

// ---- the built scene: host tree + leaf-ordered records, and their residency in HBM
struct BuiltScene {
  QBvh bvh;
  std::vector<float> h_tris;      // 12 floats per triangle, leaf order
  bool built = false;
  DevBuf<float4> d_pnodes;        // packet nodes of a single-level scene (128 B per node; kernels.hip k_expand_packet_nodes)
  DevBuf<float4> d_nodes, d_tris, d_shade, d_mats, d_lights, d_env;
  DevBuf<float4> d_uvs, d_texels; DevBuf<uint4> d_tex_desc;
  DevBuf<float4> d_verts;         // two-level scenes: object-space vertices per leaf position (shading of instance hits)
  // setters called every GUI frame (material-editor drags MaterialEditor.cxx:331-337, manipulator moves ImRaytraceControls.cxx:58-89)
  // reuse their device allocations and copy through a small ring of pinned staging buffers on the context's
  // stream: no hipFree / hipMalloc, no device-wide synchronisation, kernels still in flight keep reading the old bytes
  struct Stage { PinnedBuf<void> p; hipEvent_t ev = nullptr; bool used = false; } stage[4];
  uint32_t stage_next = 0;
};

// ---- accumulator, the frame assembled by crh_reduce, adaptive sampler state
struct FrameState {
  DevBuf<float4> d_accum; uint32_t accumW = 0, accumH = 0;
  DevBuf<float> d_m2;               // running mean of squared luminance (adaptive sampling only)
  // crh_reduce: the frame assembled from all shards lives beside the root's own accumulator (rendering continues into that)
  DevBuf<float4> d_assembled, d_peer_stage; uint32_t assembledW = 0, assembledH = 0; bool assembled_valid = false;
  std::vector<ncclComm_t> comms; std::vector<crh_ctx*> comm_ctxs;      // RCCL communicators of the last multi-device group (kept on the root)
  DevBuf<float> d_tile_err; DevBuf<uint32_t> d_tile_cnt;      // per tile of the image
  bool show_tiles = false; bool picked_valid = false;                                   // ShowSamplingTiles: d_picked marks the tiles of the last adaptive iteration
  DevBuf<float> d_tile_cdf; DevBuf<uint8_t> d_picked; DevBuf<uint32_t> d_adapt_n;   // adaptive sampler state in HBM (running sum, drawn-tile mask, tile count)
  bool adaptive = false; uint32_t adaptive_tiles = 128; uint32_t adaptive_picks = 0;   // NbRayTracingTiles, Halton index
  uint32_t frames_done = 0;       // whole-frame iterations since reset (crh_render continues from here)
};

// ---- path state, queues and the launch schedule
struct ScheduleState {
  // speculative look-ahead for the +1-spp-per-Redraw boundary: frames [pending_first, pending_first + pending_n) are traced
  // and wait in the path buffer (batch sample index pending_off ...) to be folded in by the next crh_render calls
  uint32_t lookahead = 1, pending_first = 0, pending_n = 0, pending_off = 0, pending_tiles = 0;
  uint32_t lookahead_auto = 0, ramp_k = 1;               // crh_set_lookahead_auto: the batch grows 1, 4, 16, ... after every restart of the accumulation
  DPaths paths{}; DQueues queues{}; uint32_t path_cap = 0;      // what the kernels take by value: raw pointers into path_store / d_queue_counts (path_slots())
  DevBuf<void> path_store[16]; DevBuf<uint32_t> d_queue_counts;
  uint32_t stamp_counter = 0;        // DPaths::stamp of the last batch traced (never 0: the radiance buffer is zeroed when it is allocated)
  DevBuf<uint32_t> d_tile_ids;
  DevBuf<uint32_t> d_tile_ids2; int tile_list_last = 0;      // render_impl keeps two lists resident (round 6: row-major and sorted)
  DevBuf<uint32_t> d_seeds;
  // Counters of the CURRENT accumulation (crh_stats counts since the last restart).  Four blocks, used in turn: crh_reset moves on to the next one -- zeroed one
  // restart earlier, stream-ordered -- instead of zeroing the one in use, so the first frame after a restart need not wait for the frames of the old accumulation
  // that are still in flight to have added their last counts (render_impl, frame pipeline).
  DCounters* d_counters = nullptr; DevBuf<DCounters> d_counters_ring; uint32_t counter_epoch = 0; hipEvent_t counters_zeroed[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t reset_ev = nullptr; bool reset_pending = false;       // crh_reset's memsets of the accumulator: the next frame's ACCUMULATE waits for them, its tracing does not
  uint64_t stream_uses = 0;                                        // cstream() calls (anything enqueued on the context's stream)
  DevBuf<uint32_t> d_api_cursor;      // work cursor of the API-level trace kernels
  DevBuf<void> d_scratch;
  bool clamp_grid = true;   // persistent traversal grids are clamped to what the register budget keeps resident (kernels.hip, resident_grid)
  int packets = 64;         // smallest run of consecutive samples per pixel (sample_group) from which wide batches walk their camera rays as wavefront packets (kernels.hip, k_trace_packets): 64 = a wavefront is ONE pixel (C3 +3.3 % at 128 spp per batch, +1.6 % at 64); with two / four pixels per wavefront (32 / 16 samples each) the shared walk loses (C3 -2 % / -5.6 %); CRH_PACKETS=<n> sets the threshold, 0 switches packets off
  bool donate = true;       // small batches use the work-donating traversal kernels (kernels.hip, DON); CRH_DONATE=0 switches them off
                            // (measured with plain kernels + wider grids for the first 1-4 bounces: 232 -> 232 / 226 / 222 / 218 Redraw/s: donate from bounce 0)
  // Small batches (one Redraw() = +1 spp of one frame, AppViewer.cxx:1045-1047) are launch- and drain-bound: every traversal
  // launch ends with the longest rays of a few wavefronts while the rest of the chip idles.  Such a batch is cut into `n_lanes`
  // tile ranges that run the same wavefront schedule on their own streams and their own slice of the path state, so one
  // range's drain phases overlap the others' busy phases.  Pixels, seeds and the per-pixel accumulation order do not change.
  // Measured on C3 at 1080p, 1 spp per call (tools/bench_interactive.py): 1 / 2 / 4 / 8 ranges -> 162 / 175 / 114 / 84 Redraw/s: two
  // concurrent schedules overlap, more of them only add launches that each end in their own ~0.4 ms drain.
  uint32_t n_lanes = 2, lane_max_paths = 12u << 20;
  hipStream_t lane_stream[8] = {}; hipEvent_t lane_fork = nullptr, lane_join[8] = {}; DevBuf<uint32_t> d_lane_counts;
  std::vector<uint32_t> h_tile_ids;      // what d_tile_ids holds (an unchanged tile list is not uploaded again)
  std::vector<uint32_t> h_tile_ids2;     // ... and d_tile_ids2
  // frame pipelining: consecutive small whole batches (one Redraw() each) rotate through pipe_depth streams and path-state slices, so
  // the drain-bound late bounces of frame n overlap the throughput-bound first bounces of frame n + 1; accumulation stays in
  // frame order (an event between consecutive accumulate launches); the rules: crh_plan.h plan_frame
  bool pipeline = true; int pipe_div = 4096;
  plan::PipeState pipe;            // what the pipeline's rules remember from frame to frame (crh_plan.h plan_frame)
  hipEvent_t pipe_resized = nullptr;      // complete when the last frame of the PREVIOUS batch size is done (plan_frame)
  std::chrono::steady_clock::time_point pipe_last_submit{};      // when the previous pipelined frame was submitted
  int pipe_grid_min = 192, pipe_grid_min_shade = 512;      // floors of a pipelined frame's traversal / streaming grids
  uint32_t pipe_depth = 3;         // frames in flight: 2 / 3 / 4 -> 323 / 391 / 312 Redraw/s on C3, 448 / 558 / 453 on C2
  bool read_since_render = true;   // a host that looks at every frame (read-back / sync between Redraws) gets the two-range schedule instead
  // path slots per batch (196 B each = 105 GB of the 288 GB; allocated on demand, so small renders stay small).  Every launch of
  // the wavefront schedule ends in a drain phase whose length does not depend on the launch's size (~0.24 ms per launch on C3), so
  // the batch is made as wide as the memory comfortably allows: 32 M / 64 M / 128 M / 256 M / 512 M slots -> 2745 / 2960 / 3114 /
  // 3205 / 3243 Mrays/s on C3 in round 2; round 4, 512 samples per call: 128 M / 256 M / 512 M / 1 G -> 3981 / 4132 / 4204 / 4180
  uint32_t max_paths = 512u << 20;
  // The frame kernel (k_frame.h): a small batch in ONE launch -- every workgroup streams its own paths through ray generation, traversal and shading, no
  // launch boundary between bounces.  Takes the place of the staged small-batch schedule (lanes / pipelined launches per bounce) wherever a batch is small,
  // not counted and not timed per kernel; CRH_FRAME_KERNEL=0 or crh_set_schedule(CRH_SCHEDULE_STAGED) keeps the staged form (the reference of the sequence tests).
  bool frame_kernel = true, auto_frame_kernel = true;
  uint32_t frame_live = 4096, frame_chunk = 128;    // paths a workgroup (16 wavefronts, one per compute unit) keeps alive at most; path slots a wavefront claims at a time
                                                    // (round 6, with the miss ring: chunk 128 / 192 / 256 / 512 -> lone frame on C3 2.85 / 2.97 / 2.95 / 3.46 ms, profiles/r6/lone_frame.md)
  uint32_t frame_low_water = 512;                   // a feeder wavefront claims the next chunk once fewer rays than this wait in the workgroup's ring
  uint32_t frame_starve = 1u << 20;                 // a feeder shades fewer than 64 hits only while fewer rays than this wait in the ring
  uint32_t frame_feeders = 3, frame_claim_step = 0;    // wavefronts that only shade and generate (round 6: 2 / 3 / 4 / 5 -> 3.07 / 2.85 / 2.92 / 3.39 ms lone frame on C3, 3.0 / 2.60 / 2.30 / 2.31 on the CAD-like scene,
                                                    // whose short walks leave more shading and generating per traced ray: CRH_FRAME_FEED=4 there); tracer w takes rays only
                                                       // while >= w * claim_step wait: 0 / 16 / 32 / 64 -> 2.90 / 2.95 / 3.13 / 3.46 ms -- the shared rings gather the late bounces by themselves
  // The feeder count is chosen by measurement (round 6) unless CRH_FRAME_FEED fixes it: scenes with short walks (tessellated parts, 13.6 node visits per ray) want 4
  // feeders -- lone frame 2.62 -> 2.36 ms, drag 425 -> 507 frames/s on CAD1M -- triangle soups 3 (4 costs them 1 - 2 %).  After every crh_build (and a change of the
  // target size or the depth) the first pipelined frame-kernel frames run in blocks of 6 -- a warm-up block, then 3 / 4 / 3 / 4 feeders; the device time of each
  // frame KERNEL (its own event pair, first frame of a block left out) decides: 4 if that is >= 5 % faster, else 3 (CAD1M: 16 %; the soups: within +- 3 %).  No image depends on the count (tests/test_frame_kernel.py).
  struct FeedTune {
    bool on = true; uint32_t chosen = 0, frames = 0;
    plan::Tally<hipEvent_t> t;      // [0]: 3 feeders, [1]: 4
    void restart() { chosen = 0; frames = 0; t.restart(); }
  } feed_tune;
  // The ORDER in which a lone frame's tiles are claimed (round 6; CRH_TILE_ORDER=0: row-major as up to round 5).  Whatever the frame kernel claims last runs out its
  // bounces on an emptying chip (the drain is 0.43 of a lone frame); pixels do not depend on the order (the RNG is seeded per pixel).  k_accumulate sums the rays
  // each tile's paths traced (frame-kernel frames of a host that waits for its frames only); a restart copies the sums to the host and zeroes them; crh_render
  // then lists the tiles most-rays-first -- for a host whose frames start on an idle chip (six calls in a row with nothing in flight); otherwise row-major.
  // Both lists stay resident on the device (render_impl).  Measured (profiles/r6/lone_frame.md 2c, tile_order_product_ab.txt): lone frame -6 % on CAD1M, -2 % on
  // C2, +-1 % on C3; the drag, display and free-running loops unchanged.
  struct TileOrder {
    bool on = true;
    DevBuf<uint32_t> d_cost; PinnedBuf<uint32_t> h_cost; uint32_t n = 0;        // per tile id: rays since the last restart (device), the last restart's copy (pinned host)
    hipEvent_t copied = nullptr; bool pending = false, dirty = false;           // a copy is under way; frames have added to d_cost since the last copy
    std::vector<uint8_t> cls; std::vector<uint32_t> order;                      // the classes the current list was made from; the list (empty: row-major)
    uint64_t reorders = 0, calls_sorted = 0, calls_row_major = 0, frames_collected = 0; uint32_t streak = 0;      // streak: crh_render calls in a row that found no frame in flight
    // ... and whether the sorted list pays on THIS scene is measured, once per crh_build (a soup that does not fit the caches loses more by the scattered tiles than
    // the shorter drain gives back: C5's lone 4K frame 10.9 -> 12.1 ms): once a sorted list exists and the feeder count is settled, lone frames take the two lists
    // in turn, each frame kernel between two events; sorted stays if its mean is >= 2 % shorter.  verdict: 0 measuring, 1 sorted, 2 row-major.
    uint32_t verdict = 0, trials = 0; int tag_next = -1;
    plan::Tally<hipEvent_t> t;      // [0]: sorted, [1]: row-major
    void remeasure() { verdict = 0; trials = 0; tag_next = -1; t.restart(); }
  } tile_order;
  uint32_t frame_help = 256;                        // a tracer wavefront shades a batch itself once this many hit records wait
  uint32_t frame_help_low = 0;                      // ... and prefers a full shading batch to tracing while fewer rays than this wait (CRH_FRAME_HELP_LOW)
  int frame_grid = 0;                               // workgroups of a lone frame (0: what is resident, 4 per CU)
  uint32_t frame_pipe_depth = 2;                    // a pipelined frame takes the frame kernel while fewer than this many frames are running, and at most this many frame
                                                    // kernels run at a time (they share the chip by compute units); beyond it the staged form carries the deeper pipeline
  int schedule = CRH_SCHEDULE_AUTO; uint32_t auto_lane_max_paths = 12u << 20; bool auto_donate = true, auto_pipeline = true;   // crh_set_schedule
};

// ---- asynchronous read-back (crh_read_ldr_begin / _end, crh_read_hdr_begin / _end): tone map + device-to-host copy of the frame as submitted so far run on
// their own stream into one of two device / pinned-host buffer pairs while the next Redraw()s are already rendering; only the NEXT
// accumulate waits (for the tone map, which reads the accumulator), nothing else does.  A read-back is of one of three KINDS -- the LDR frame, the HDR frame, a view
// of the LDR frame (crh_view.cpp) -- which share the two slots; the oldest in flight is ended by the call of its own kind.
enum ReadKind : uint8_t { kReadLdr = 0, kReadHdr = 1, kReadView = 2 };
struct ViewPlan;      // view_kernels.h
struct ReadbackState {
  hipStream_t rb_stream = nullptr; hipEvent_t rb_fork = nullptr, rb_tm[2] = {nullptr, nullptr}, rb_done[2] = {nullptr, nullptr};
  DevBuf<uint8_t> d_rb[2]; PinnedBuf<uint8_t> h_rb[2]; size_t rb_bytes[2] = {0, 0}; ReadKind rb_kind[2] = {kReadLdr, kReadLdr};
  uint32_t rb_head = 0, rb_outstanding = 0; bool rb_guard_pending = false; hipEvent_t rb_guard = nullptr;
  // auto exposure (crh_set_auto_exposure; kernels in k_meter.h): while on, every LDR read-out meters the image in front of its tone map, on the stream it uses anyway.
  // Four metering blocks (allocated on first need): [0] the synchronous read-out, [1] / [2] the two read-back slots, [3] crh_measure_exposure -- the context's
  // stream and the read-back stream never share one.  The display values themselves are par.tonemap_mode / exposure / white_point: only the tone map reads them.
  bool meter_on = false; crh_meter_params meter_par{}; DevBuf<DMeter> d_meter;
};

// ---- what a buffer DERIVED from the id buffer and the per-triangle table (the outline mask, the denoise guide) was computed from: it is stale when the stamp of the
// state in force differs.  ids_gen and table_gen of a computed buffer are never 0, so a default stamp means "none".
struct DerivedStamp {
  uint64_t ids_gen = 0, table_gen = 0; uint32_t w = 0, h = 0, par[2] = {0u, 0u};
  bool operator==(const DerivedStamp& o) const { return ids_gen == o.ids_gen && table_gen == o.table_gen && w == o.w && h == o.h && par[0] == o.par[0] && par[1] == o.par[1]; }
};

// ---- the first-hit id buffer (crh_pick.cpp): DERIVED state -- object / triangle / distance under every pixel centre for the camera, target size, geometry, transforms,
// visibility flags and tree in force.  do_reset and crh_set_camera clear ids_valid; the buffer is computed on the first pick / id read-back / overlaid LDR read-out after
// that, on a stream of its own (crh_render never launches it), kept on the device, and a further crh_pick is one 16-byte copy.  Selection and hover are plain host
// state; only the LDR read-out looks at them.
struct PickState {
  hipStream_t pk_stream = nullptr; hipEvent_t pk_fork = nullptr;
  DevBuf<float4> d_pk_rays, d_pk_hit_slot;                                                   // per ray slot (8x8-block order): the ray, what the traversal kernel answered
  DevBuf<float4> d_pk_hit; DevBuf<int32_t> d_pk_obj;                                         // per pixel, row-major: {t, u, v, caller's triangle index}, object
  DevBuf<int32_t> d_pk_tri_obj; uint64_t pk_tri_obj_gen = 0;                                 // c->tri_obj on the device, and the geom_gen it was uploaded at (on first need after a change)
  DevBuf<uint32_t> d_pk_cursor; DevBuf<DCounters> d_pk_counters;                             // work cursor and counter block of the id pass (crh_stats never sees its rays)
  bool ids_valid = false; uint32_t ids_w = 0, ids_h = 0;
  uint64_t ids_gen = 0;                                                                      // bumped whenever ensure_ids recomputes: what is derived from the buffer (the outline mask) knows when it is stale
  std::vector<uint8_t> sel; bool sel_any = false; uint8_t sel_rgb[3] = {0, 0, 0}; uint32_t sel_alpha = 0;
  DevBuf<uint8_t> d_sel; bool sel_dirty = false;
  int32_t hover = -1; uint8_t hov_rgb[3] = {0, 0, 0}; uint32_t hov_alpha = 0;
};

// ---- view fitting (crh_fit.cpp): one float4 {x, y, z, object} per vertex on the device, built from pos / tri / tri_obj and uploaded by the FIRST crh_fit_view after
// the geometry changed (a host that never fits pays no memory and no time); the per-call object table and the records the kernel fills
struct FitState {
  DevBuf<float4> d_fit_verts; uint32_t fit_n = 0; uint64_t fit_verts_gen = 0;      // (the geom_gen the array was built from)
  DevBuf<void> d_fit_objs; DevBuf<uint32_t> d_fit_rec;      // room for the same number of objects in both
};

// ---- region queries (crh_region.cpp): the polygon's edges and the per-object records of ONE call, allocated on first need (a host that never asks pays nothing)
struct RegionState {
  DevBuf<void> d_rg_edges; DevBuf<uint32_t> d_rg_rec;      // kRegionMaxEdges edges; kRegionRec words per record (objects + background)
};

// ---- feature lines (crh_outline.cpp): display state like the selection -- only the LDR read-out looks at it.  The per-triangle table (32 B: object-space normal and
// vertex indices) is DERIVED from pos / tri and uploaded by the first call that needs it after the geometry changed; the mask (one byte per pixel) is derived from the
// id buffer and the table and kept while neither, nor the frame size, nor the two thresholds change.  A host that never switches the feature on pays nothing.
struct OutlineState {
  bool ol_on = false; crh_outline_params ol_par{};
  DevBuf<void> d_ol_table; uint32_t ol_n_tri = 0; uint64_t ol_table_gen = 0;      // (the geom_gen the table was built from)
  DevBuf<uint8_t> d_ol_mask; DerivedStamp ol_mask_stamp;                          // what the mask was computed from: par = the bits of crease_cos, depth_ratio
};

// ---- denoised display (crh_denoise.cpp): display state like the feature lines -- only the tone map of an LDR read-out (and crh_read_denoised) looks at it.  The guide
// (per pixel {n.xyz, t} and {object, triangle}) is DERIVED from the id buffer and the per-triangle table of the feature lines and kept while neither, nor the frame
// size, changes.  Two ping-pong images per SET: set 0 serves the synchronous read-outs on the context's stream, set 1 the read-back stream, whose two slots are serial
// in stream order and so share it.  A host that never switches the feature on pays nothing.
struct DenoiseState {
  bool dn_on = false; crh_denoise_params dn_par{};
  DevBuf<float4> d_dn_guide; DevBuf<int2> d_dn_ids; DerivedStamp dn_guide_stamp;      // what the guide was computed from (par stays 0)
  DevBuf<float4> d_dn_img[2][2];
  bool dn_staged = true;            // steps 1 and 2 take the LDS-staged kernel (denoise_kernels.hip): 67 - 72 against 77 - 85 us per pass at 1080p; CRH_DENOISE_STAGED=0: the plain gather; the same bytes either way
};

// ---- shade guide of the denoised display (crh_shade_guide.cpp): display state like the filter it serves.  The per-triangle table (32 B: uv of the three vertices,
// material) is DERIVED from uv / tri and uploaded by the first call that needs it after the geometry changed; the plane (per pixel {1 / albedo, light flag}) and the
// flag bytes it is dilated from are derived from the id buffer, the table and the SHADING -- materials, textures, lights, spec: shade_gen, bumped by their setters --
// and kept while none of them, nor the frame size, nor the parameters change.  A host that never switches the feature on pays nothing.
struct ShadeGuideState {
  bool sg_on = false; crh_shade_guide_params sg_par{};
  DevBuf<void> d_sg_table; uint32_t sg_n_tri = 0; uint64_t sg_table_gen = 0;      // (the geom_gen the table was built from)
  DevBuf<float4> d_sg_plane; DevBuf<uint8_t> d_sg_seen;
  DerivedStamp sg_stamp; uint64_t sg_stamp_shade = 0;      // what the plane was computed from: par = the parameter bits; the shade_gen
  uint64_t shade_gen = 1;                                  // THE SHADING GENERATION
};

// ---- reprojected display history (crh_reproject.cpp): display state like the denoised display -- only the LDR read-outs (and crh_read_reprojected) look at it.  The
// HISTORY is what crh_set_camera captured of the view that ended: two images (a capture reads one and writes the other), a copy of that view's guide planes, its camera
// frame.  One output image per SET, as the denoise filter has them: set 0 the context's stream, set 1 the read-back stream.  A host that never switches the feature on
// pays nothing.
struct ReprojectState {
  bool rp_on = false; crh_reproject_params rp_par{};
  DevBuf<float4> d_rp_hist[2]; uint32_t rp_cur = 0;                   // rp_cur: the image that holds the valid history
  DevBuf<float4> d_rp_hguide; DevBuf<int2> d_rp_hids; crh_reproject_frame rp_frame{}; uint32_t rp_w = 0, rp_h = 0;
  bool rp_valid = false;          // a history exists (for the frame size rp_w x rp_h)
  bool rp_fresh = false;          // ... and was captured since the last restart: the crh_reset that follows keeps it
  bool rp_captured = false;       // a capture has been made since the last restart
  bool rp_from_reset = false;     // do_reset is being reached through crh_reset
  DevBuf<float4> d_rp_out[2];
  // per-object history deltas (crh_set_reproject_motion): X_hist = the transforms in force when the history was captured; the table derived from (X_hist, c->xf),
  // rebuilt whenever either changes and uploaded, stream-ordered on the context's stream, only while a record is flagged.  Never switched on: nothing allocated.
  bool rpm_on = false; crh_reproject_motion_params rpm_par{};
  std::vector<float> rpm_xf_hist; std::vector<crh_reproject_delta> rpm_table; uint32_t rpm_flagged = 0;
  DevBuf<void> d_rpm_table;
  bool rp_keep_restart = false;   // do_reset is being reached through a crh_set_transforms that keeps the history
  bool rpm_staged = false;        // CRH_REPROJECT_STAGED=1: the LDS-staged form of the motion kernel while at most 64 records have flag 1 (measured, not the default: DESIGN.md section 6.12)
  uint32_t rpm_n_staged = 0; bool rpm_stageable = false;      // flag-1 records uploaded in slot order behind the table; whether they are at most 64
  uint64_t rp_launches[2] = {0, 0};      // k_reproject_resolve / k_reproject_resolve_motion launched by read-outs and captures (crh_get_reproject_launches)
};

// ---- viewport read-out (crh_view.cpp): the full RGB8 frame a view is resampled FROM, one scratch image per SET as the denoise filter has them -- set 0 the context's
// stream, set 1 the read-back stream, which orders two views in flight by itself.  Nothing else is kept: the parameters travel with every call.  A host that never
// asks for a view pays nothing.
struct ViewState {
  DevBuf<uint8_t> d_vw_full[2];
};

// ---- annotations (crh_annotate.cpp): display state like the selection -- only the LDR read-outs (and the annotation queries) look at it.  The list lives on the host
// and, from the first read-out that draws it, on the device.  The records and the per-tile bins are DERIVED from the list, the camera and the frame size: one pair per
// SET -- 0 the context's stream, 1 the read-back stream, as the denoise filter has them, 2 the id buffer's stream for the queries -- each with the stamp of what it was
// computed from, recomputed in stream order by the first use after a change.  A host that never hands over a list pays nothing.
struct AnnotStamp {
  uint64_t gen = 0; crh_camera cam{}; uint32_t w = 0, h = 0, tile = 0, scatter = 0; uint64_t ids_gen = 0;      // gen 0: none
  bool operator==(const AnnotStamp& o) const { return gen == o.gen && !std::memcmp(&cam, &o.cam, sizeof cam) && w == o.w && h == o.h && tile == o.tile && scatter == o.scatter && ids_gen == o.ids_gen; }
};
struct AnnotateState {
  bool an_on = false; crh_annot_params an_par{}; std::vector<crh_annot_segment> an_segs;
  uint64_t an_gen = 0;            // THE LIST'S GENERATION: bumped by every crh_set_annotations that is accepted
  bool an_depth = false;          // some segment has mode HIDE or XRAY: the drawing reads the id buffer
  DevBuf<void> d_an_segs; uint64_t an_segs_gen = 0;      // (the generation the device copy holds)
  DevBuf<void> d_an_rec[3]; DevBuf<uint32_t> d_an_bins[3]; AnnotStamp an_stamp[3];
  DevBuf<int32_t> d_an_ids; DevBuf<float> d_an_s; AnnotStamp an_plane_stamp;      // the id plane and the parameter plane of the queries
  uint32_t an_tile = 16;          // the tile edge of the drawing kernel (CRH_ANNOT_TILE=8|16|32): 16 draws fastest, 8 costs 1.3 - 1.5 times as much
  int an_bin_form = 0;            // the binning form: 0 by the list's length -- gather (a thread per tile and word) up to kAnnotGatherMax segments, scatter (a thread per segment,
                                  // atomicOr) above: the gather form costs 3 (1080p) / 13 (4K) us per word of the list, the scatter form 16 - 120 us whatever the length --
                                  // 1 gather, 2 scatter (CRH_ANNOT_BIN=gather|scatter); the same bits either way
};

// ---- counters and timing
struct TimingState {
  bool counters_on = false, timing_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> render_ev, trace_ev;
  std::vector<hipEvent_t> ev_pool;
  double seconds_acc = 0.0, trace_ms_acc = 0.0, all_ms_acc = 0.0; uint64_t trace_launches = 0;
};

}  // namespace crh

struct crh_ctx : crh::HostInputs, crh::TwoLevelState, crh::BuiltScene, crh::FrameState, crh::ScheduleState, crh::ReadbackState, crh::PickState, crh::FitState, crh::RegionState, crh::OutlineState, crh::DenoiseState, crh::ShadeGuideState, crh::ReprojectState, crh::ViewState, crh::AnnotateState, crh::TimingState {
  int device = 0;
  uint64_t geom_gen = 1;  // THE GEOMETRY GENERATION: geometry_changed() bumps it; every table derived from pos / tri / tri_obj remembers the one it was built from (0: none yet)
  hipStream_t stream_ = nullptr;   // use cstream(c): it first joins frames still in flight on the pipeline streams
  int cus = 0;            // compute units (0: unknown)
  int grid = 1024;        // streaming / shading kernels: 4 workgroups per CU = what k_shade's 128 VGPRs keep resident; every workgroup of the
                          // persistent loops then starts at once and the next bounce's queue keeps the block-major order.  Measured, workgroups
                          // 512 / 768 / 1024 / 1280 / 2048: C5 2842 / 2874 / 2925 / 2839 / 2813, C3 3507 / 3688 / 3807 / 3787 / 3777, C2 4649 / 4849 / 4967 / 4975 / 4941 Mrays/s
  int grid_trace = 1536;  // traversal kernels: 6 workgroups (= 6 waves/SIMD) per CU -- measured: 4 / 5 / 6 / 7 / 8 per CU -> 3300 / 3424 /
                          // 3448 / 3448 / 3443 Mrays/s on C3 (more rays in flight enlarge the working set the 4 MB-per-XCD L2s hold)
  std::string err;
};

// The context's stream.  Small whole-frame batches rotate through the pipeline streams (crh_plan.h plan_frame) and are joined lazily:
// whoever wants to enqueue on, or wait for, the context's stream first makes it wait for the frames still in flight.
static inline hipStream_t cstream(crh_ctx* c)
{
  crh::plan::join_pending(c->pipe, [c](uint32_t k) { hipStreamWaitEvent(c->stream_, c->lane_join[k], 0); });
  if (c->rb_guard_pending) { hipStreamWaitEvent(c->stream_, c->rb_guard, 0); c->rb_guard_pending = false; }      // an asynchronous read-back still tone-maps the accumulator
  c->read_since_render = true;      // something other than the next frame used the stream (render_impl clears this when it is done)
  ++c->stream_uses;
  return c->stream_;
}

#define CRH_HIP(call)                                                                             \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) {                                            \
      char b_[512]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      c->err = b_; return CRH_E_DEVICE; } } while (0)

namespace crh {
namespace api {

// ---- crh_context.cpp
int fail(crh_ctx* c, int code, const char* msg);
bool all_finite(const float* v, size_t n, float limit = 3.0e38f);
int stage_copy(crh_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t on = nullptr);
hipEvent_t get_event(crh_ctx* c);
void drain_events(crh_ctx* c);
int check_device_error(crh_ctx* c);      // CRH_E_DEVICE + message if a frame-kernel workgroup gave up (crh_context.cpp)
int trim_events(crh_ctx* c);
void discard_events(crh_ctx* c);
int ensure_paths(crh_ctx* c, uint32_t need);
uint32_t next_stamp(crh_ctx* c);     // DPaths::stamp for the batch about to be traced
int alloc_accum(crh_ctx* c);
int do_reset(crh_ctx* c);
int build_threads_env();      // CRH_BUILD_THREADS (0: every usable CPU)
int hw_queues();              // GPU_MAX_HW_QUEUES as this library found it when it was loaded (default 4)
uint32_t pipeline_capacity(); // frames crh_set_pipeline_depth accepts in this process: min(8, max(3, hw_queues - 2))

// Every copy and memset goes through the context's own stream: it is created non-blocking, so work on the null stream (plain
// hipMemset / hipMemcpy) is NOT ordered with it -- a hipMemset of the queue counters on the null stream used to land in the middle
// of the first batch of a fresh context when other contexts kept the device busy (lost and doubled paths).
//
// Refresh a device array in place: the allocation is kept (and grown with head-room only when it is too small), the bytes travel
// stream-ordered.  Large blocks (environment maps, whole node arrays) are copied straight from the caller's memory and waited for.
template <class T> int dev_put(crh_ctx* c, DevBuf<T>& d, const void* src, size_t bytes, size_t headroom = 0)
{
  if (bytes > d.bytes() || !d) {
    CRH_HIP(hipStreamSynchronize(cstream(c)));          // kernels in flight may still read the old allocation
    CRH_HIP(d.reserve((std::max<size_t>(bytes + headroom, 256) + d.elem - 1) / d.elem));
  }
  if (bytes <= (4u << 20)) return stage_copy(c, d, src, bytes);
  CRH_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, cstream(c)));
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  return CRH_OK;
}

// Room for n words in a device array that kernels on the context's stream may still read (the old contents are gone when it had to grow)
inline int grow_u32(crh_ctx* c, DevBuf<uint32_t>& d, size_t n)
{
  if (n <= d.cap()) return CRH_OK;
  CRH_HIP(hipStreamSynchronize(cstream(c)));
  CRH_HIP(d.reserve(n));
  return CRH_OK;
}

// The image a read-out shows: the frame crh_reduce assembled while it is valid, else this context's own accumulator
inline const float4* display_source(const crh_ctx* c) { return c->assembled_valid ? c->d_assembled : c->d_accum; }

// Room for n elements (pixels; bytes of an RGB8 image) in each of the `count` display scratch images at d, which belong to scratch set `set`.  Set 0 is read and written on the context's stream by calls
// that end with a wait for it: nothing is in flight.  Set 1 belongs to the read-back stream, which is waited for before a block goes.
template <class T> int grow_display_scratch(crh_ctx* c, int set, DevBuf<T>* d, int count, size_t n)
{
  bool room = true;
  for (int k = 0; k < count; ++k) room = room && d[k].cap() >= n;
  if (room) return CRH_OK;
  if (set == 1) CRH_HIP(hipStreamSynchronize(c->rb_stream));
  for (int k = 0; k < count; ++k) CRH_HIP(d[k].reserve(n));
  return CRH_OK;
}

// pos / tri / tri_obj changed (crh_set_geometry, crh_add_object, crh_build -- nowhere else): every table derived from them is stale
inline void geometry_changed(crh_ctx* c) { ++c->geom_gen; }

// n records from the host into a derived device table on the side stream (pick_stream first): grown with a quarter of head-room (crh_add_object grows the scene a
// little at a time) and waited for, so `src` may be a temporary
template <class Rec, class T> int side_upload(crh_ctx* c, DevBuf<T>& d, const Rec* src, size_t n)
{
  constexpr size_t per = sizeof(Rec) / DevBuf<T>::elem;
  CRH_HIP(d.reserve(per * n, per * (n / 4)));
  if (n) CRH_HIP(hipMemcpyAsync(d, src, sizeof(Rec) * n, hipMemcpyHostToDevice, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  return CRH_OK;
}

// Time `repeats` calls of launch() -- it enqueues on `on` and returns the HIP status -- between two events: their mean in *mean_ms.  Whatever went wrong, `on` has been
// waited for when this returns: the events, and the call-local buffers the launches used, may go.
template <class F> hipError_t time_launches(hipStream_t on, uint32_t repeats, F&& launch, float* mean_ms)
{
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.f;
  hipError_t e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipEventRecord(e0, on);
  for (uint32_t r = 0; r < repeats && e == hipSuccess; ++r) e = launch();
  if (e == hipSuccess) e = hipEventRecord(e1, on);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  const hipError_t e2 = hipStreamSynchronize(on);
  if (e0) hipEventDestroy(e0);
  if (e1) hipEventDestroy(e1);
  if (mean_ms) *mean_ms = ms / (float)repeats;
  return e != hipSuccess ? e : e2;
}

// The host twins: n elements of aligned storage in v, filled from the caller's bytes at src, which need not be aligned (nullptr: left zeroed)
template <class T> int aligned_copy(std::vector<T>& v, const void* src, size_t n)
{
  try { v.resize(n); } catch (const std::bad_alloc&) { return CRH_E_NOMEM; }
  if (src && n) std::memcpy(v.data(), src, sizeof(T) * n);
  return CRH_OK;
}

// THE CAMERA FRAME of `cam` over a W x H target: the one copy of these expressions -- the kernels' DScene (fill_scene), the view fit (crh_fit.cpp) and the frame a
// reprojection history keeps (crh_reproject.cpp) must agree to the bit (tests/test_display_chain.py)
struct CameraFrame { crh_v3 fwd, right, up; float tan_half, aspect; };
inline CameraFrame camera_frame(const crh_camera& cam, uint32_t W, uint32_t H)
{
  CameraFrame f;
  f.fwd = crh_norm3(crh_mk3(cam.dir[0], cam.dir[1], cam.dir[2]));
  f.right = crh_norm3(crh_cross3(f.fwd, crh_mk3(cam.up[0], cam.up[1], cam.up[2])));
  f.up = crh_cross3(f.right, f.fwd);
  float s, cs; crh_sincos((cam.fovy_deg * 0.5f) * (CRH_PI / 180.0f), &s, &cs);
  f.tan_half = s / cs;
  f.aspect = cam.aspect > 0.f ? cam.aspect : (float)W / (float)H;
  return f;
}

// ---- crh_scene.cpp
void fill_scene(const crh_ctx* c, DScene& S);
int upload_textures(crh_ctx* c);

// ---- crh_pick.cpp
int overlay_ldr(crh_ctx* c, hipStream_t on, uint8_t* d_ldr);      // hover / selection over the tone-mapped bytes at d_ldr, enqueued on `on`; nothing at all when neither is set
void clear_selection(crh_ctx* c);
uint32_t n_pick_objects(const crh_ctx* c);      // a scene handed over without objects is one object, 0
int ensure_ids(crh_ctx* c);                     // the id buffer of the state in force, computed if a change has invalidated it; synchronous on its own stream
int pick_stream(crh_ctx* c);                    // the side stream of the id buffer, of crh_fit_view and of crh_query_region, created on first need
int fork_from_context(crh_ctx* c);              // ... made to start behind what the setters have put on the context's stream
int wait_overlay_readers(crh_ctx* c);
// ---- crh_outline.cpp
int outline_ldr(crh_ctx* c, hipStream_t on, uint8_t* d_ldr);      // feature lines over the tone-mapped bytes at d_ldr, enqueued on `on`, BEFORE overlay_ldr; nothing at all while the feature is off
int ensure_ids_and_table(crh_ctx* c);                              // what the outline mask and the denoise guide are derived from, valid on return: ensure_ids, the device set, the side stream, the per-triangle table of the geometry in force
// ---- crh_denoise.cpp
// The image the tone map of an LDR read-out reads, in *shown: `src` itself while the feature is off or there is no scene (nothing is allocated, nothing is launched),
// else the filtered image of scratch set `set` (0: the context's stream, 1: the read-back stream), its passes enqueued on `on`.  Called just BEFORE launch_tonemap,
// after the metering, which keeps reading `src`.
int denoise_src(crh_ctx* c, hipStream_t on, const float4* src, int set, const float4** shown);
int ensure_guide(crh_ctx* c);      // the guide (d_dn_guide, d_dn_ids) of the state in force, computed if stale; synchronous on the side stream
// ---- crh_shade_guide.cpp
int ensure_shade_plane(crh_ctx* c);      // the plane (d_sg_plane) of the state and the parameters in force (the defaults while off), computed if stale; synchronous on the side stream
inline void shading_changed(crh_ctx* c) { ++c->shade_gen; }      // crh_set_materials, crh_set_texture, crh_set_lights, crh_set_spec -- nowhere else
// ---- crh_reproject.cpp
// The image the denoise filter / the tone map of an LDR read-out receives, in *shown: `src` itself while the feature is off, there is no scene or no valid history
// (nothing is allocated, nothing is launched), else the resolved image of set `set` (0: the context's stream, 1: the read-back stream), enqueued on `on`.  Called just
// BEFORE denoise_src, after the metering, which keeps reading `src`.
int reproject_src(crh_ctx* c, hipStream_t on, const float4* src, int set, const float4** shown);
int reproject_capture(crh_ctx* c, const crh_camera* next);      // crh_set_camera, BEFORE `next` replaces the camera in force: the header's LIFE CYCLE
// crh_set_transforms on a built scene, BEFORE `xf` replaces the transforms in force (per-object history deltas, LIFE CYCLE): the capture, and rp_keep_restart for the
// restart that follows; nothing at all unless both features are on.  reproject_transforms_set: behind apply_objects, whatever it returned -- the table of the new
// transforms, and the mark cleared.
int reproject_transforms_begin(crh_ctx* c, const float* xf);
int reproject_transforms_set(crh_ctx* c);
// do_reset: a restart reached through crh_reset keeps a fresh history, one reached through such a crh_set_transforms a valid one, any other drops it; either way a
// new capture may follow
inline void reproject_restart(crh_ctx* c)
{
  const bool keep = (c->rp_from_reset && c->rp_fresh) || c->rp_keep_restart;
  c->rp_from_reset = c->rp_fresh = c->rp_captured = c->rp_keep_restart = false;
  if (!keep) c->rp_valid = false;
}
inline void reproject_drop(crh_ctx* c) { c->rp_valid = c->rp_fresh = false; }      // the setters that change the picture without a restart of their own
// ---- crh_readback.cpp
// THE DISPLAY CHAIN: everything between the image a read-out shows and the RGB8 bytes of the FRAME at d_ldr, enqueued on L.stream (set: the scratch images, block: the
// metering block).  A view read-out resamples what this wrote (crh_view.cpp): that stage comes last, behind the overlay.
int enqueue_display_chain(crh_ctx* c, const Launch& L, int set, int block, uint8_t* d_ldr);
// the asynchronous read-backs of all three kinds (view: the plan of a kReadView, else NULL) and the end of the oldest one
int read_begin(crh_ctx* c, ReadKind kind, const ViewPlan* view);
int read_end(crh_ctx* c, void* out, ReadKind kind);
// ---- crh_view.cpp
// The resample of the frame at d_full (W x H of the parameters in force) into d_out, enqueued on `on`
int view_resample(crh_ctx* c, hipStream_t on, const uint8_t* d_full, const ViewPlan& P, uint8_t* d_out);
// ---- crh_annotate.cpp
// Annotations over the finished bytes of the FRAME at d_ldr, enqueued on `on` (set: whose records and bins), LAST in the display chain, behind overlay_ldr; nothing at
// all while the feature is off, the list is empty or there is no scene
int annotate_ldr(crh_ctx* c, hipStream_t on, int set, uint8_t* d_ldr);
// ---- crh_reduce.cpp
void release_comms(crh_ctx* c);
int reduce_fake_devices(crh_ctx* const* ctxs, uint32_t n, uint32_t root);      // crh_reduce.cpp: the RCCL branch of crh_reduce on contexts that share a device (test hook)

}  // namespace api
}  // namespace crh
