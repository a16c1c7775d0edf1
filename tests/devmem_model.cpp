// devmem_model.cpp -- the owning buffer type of cadrays_amd/csrc/crh_devmem.h against a memory policy that records what is live and can be told to refuse
// its k-th allocation.  No HIP, no context.  The script below makes the calls the library makes (growing, equal and smaller sizes, head-room, the
// keep-the-front growth of crh_add_object, release, move, scope exit), among them the five sequences that used to leave a capacity beside a null or freed
// pointer; it runs once clean and once for every allocation of the clean run refused.  After EVERY step: null exactly when empty, the live blocks are exactly
// the buffers' blocks; a reserve that has room calls no allocator; a refused reserve leaves an empty buffer, a refused reserve_keep the old block, untouched and
// with no copy made; whatever comes after the refusal succeeds; at exit nothing is live.  tests/test_devmem.py builds this with ASan + UBSan: the blocks are real
// ones and every successful call writes all the elements it asked for.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "crh_devmem.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s (%s:%d) refuse_at=%ld step=%ld\n", #x, __FILE__, __LINE__, Fake::refuse_at, g_steps); abort(); } } while (0)

static long g_steps = 0;

struct Fake {
  using status = int; static constexpr status ok = 0; static constexpr status refused = 2;
  static std::set<void*> live; static long allocs, frees, refuse_at; static bool fired;
  static status alloc(void** p, size_t bytes)
  {
    ++allocs;
    if (allocs == refuse_at) { fired = true; *p = nullptr; return refused; }
    *p = malloc(bytes ? bytes : 1);      // distinct blocks, and ASan watches their bounds
    live.insert(*p);
    return ok;
  }
  static status free(void* p)
  {
    ++frees;
    if (!live.erase(p)) { fprintf(stderr, "FAILED release of a block that is not live (refuse_at=%ld step=%ld)\n", refuse_at, g_steps); abort(); }
    ::free(p);
    return ok;
  }
};
std::set<void*> Fake::live; long Fake::allocs = 0, Fake::frees = 0, Fake::refuse_at = 0; bool Fake::fired = false;

struct Rec16 { uint32_t w[4]; };
template <class T> using FBuf = crh::Buf<T, Fake>;

// every buffer in scope, as {pointer, capacity} readers
struct View { const void* (*p)(const void*); size_t (*cap)(const void*); const void* self; };
static std::vector<View> g_bufs;
template <class T> struct Watched {
  FBuf<T> b;
  Watched() { g_bufs.push_back({[](const void* s) -> const void* { return (T*)*(const FBuf<T>*)s; }, [](const void* s) { return ((const FBuf<T>*)s)->cap(); }, &b}); }
  ~Watched() { for (size_t i = 0; i < g_bufs.size(); ++i) if (g_bufs[i].self == &b) { g_bufs.erase(g_bufs.begin() + (long)i); break; } }
};

static void invariants()
{
  ++g_steps;
  std::set<void*> held;
  for (const View& v : g_bufs) {
    const void* p = v.p(v.self);
    CHECK((p == nullptr) == (v.cap(v.self) == 0));
    if (p) CHECK(held.insert((void*)p).second);      // no block belongs to two buffers
  }
  CHECK(held == Fake::live);
}

template <class T> static void touch(FBuf<T>& b, size_t n) { if (n) std::memset(b.template as<char>(), 0x5a, n * b.elem); }

// reserve as a call site makes it: false = the call returns its error (CRH_HIP)
template <class T> static bool reserve(FBuf<T>& b, size_t n, size_t headroom = 0)
{
  const size_t cap0 = b.cap(); const long a0 = Fake::allocs, f0 = Fake::frees; const bool after_refusal = Fake::fired;
  const int s = b.reserve(n, headroom);
  invariants();
  if (n <= cap0) { CHECK(s == Fake::ok && Fake::allocs == a0 && Fake::frees == f0 && b.cap() == cap0); touch(b, n); return true; }
  CHECK(Fake::allocs == a0 + 1 && Fake::frees == f0 + (cap0 ? 1 : 0));
  if (s != Fake::ok) { CHECK(!after_refusal && (T*)b == nullptr && b.cap() == 0); return false; }
  CHECK(b.cap() == n + headroom && (T*)b != nullptr);
  touch(b, n + headroom);
  return true;
}

static long g_copies = 0;
static bool reserve_keep(FBuf<Rec16>& b, size_t n, size_t keep)
{
  const size_t cap0 = b.cap(); Rec16* const p0 = b; const long a0 = Fake::allocs, c0 = g_copies; const bool after_refusal = Fake::fired;
  for (size_t i = 0; i < keep; ++i) p0[i].w[0] = (uint32_t)(7u * i + 1u);
  const int s = b.reserve_keep(n, keep, [](Rec16* to, const Rec16* from, size_t k) { ++g_copies; std::memcpy(to, from, k * sizeof(Rec16)); return Fake::ok; });
  invariants();
  if (n <= cap0) { CHECK(s == Fake::ok && Fake::allocs == a0 && g_copies == c0 && (Rec16*)b == p0); return true; }
  if (s != Fake::ok) { CHECK(!after_refusal && (Rec16*)b == p0 && b.cap() == cap0 && g_copies == c0); for (size_t i = 0; i < keep; ++i) CHECK(p0[i].w[0] == (uint32_t)(7u * i + 1u)); return false; }
  CHECK(b.cap() == n && (Rec16*)b != p0 && g_copies == c0 + ((p0 && keep) ? 1 : 0));
  for (size_t i = 0; i < keep; ++i) CHECK(b[i].w[0] == (uint32_t)(7u * i + 1u));
  touch(b, n);
  return true;
}

template <class T> static void release(FBuf<T>& b) { CHECK(b.release() == Fake::ok); invariants(); CHECK((T*)b == nullptr && b.cap() == 0); }

// ---- the calls of the library, as far as memory goes
struct Ctx {
  Watched<void> scratch;                                  // crh_read_hdr / crh_read_ldr / the debug hooks
  Watched<uint32_t> tile_ids, tile_ids2, seeds;           // grow_u32
  Watched<float> tile_err, tile_cdf; Watched<uint32_t> tile_cnt, adapt_n; Watched<uint8_t> picked;      // tile_stats / adaptive_iteration
  Watched<uint8_t> d_rb[2], h_rb[2];                      // read_begin
  Watched<Rec16> tris, shade, uvs, verts; size_t cap_pos = 0, n_pos = 0;      // crh_build / crh_add_object
  Watched<void> path[3];                                  // ensure_paths / crh_set_path_budget
  Watched<Rec16> mats;                                    // dev_put
};

static bool read_ldr(Ctx& c, size_t n) { return reserve(c.scratch.b, 3 * n); }
static bool render(Ctx& c, size_t nt, size_t ns)
{
  if (!reserve(c.tile_ids.b, nt)) return false;
  if (nt & 1u) { if (!reserve(c.tile_ids2.b, nt)) return false; }
  return reserve(c.seeds.b, ns);
}
static bool tile_stats(Ctx& c, size_t nt)
{
  if (nt > c.tile_err.b.cap() || nt > c.tile_cnt.b.cap()) {
    release(c.tile_cdf.b); release(c.picked.b); release(c.adapt_n.b);
    if (!reserve(c.tile_err.b, nt) || !reserve(c.tile_cnt.b, nt)) return false;
  }
  return true;
}
static bool adaptive(Ctx& c, size_t nt)
{
  return reserve(c.tile_err.b, nt) && reserve(c.tile_cnt.b, nt) && reserve(c.tile_cdf.b, nt) && reserve(c.picked.b, nt) && reserve(c.adapt_n.b, 16);
}
static bool read_begin(Ctx& c, size_t bytes)
{
  if (bytes > c.d_rb[0].b.cap() || bytes > c.h_rb[0].b.cap() || bytes > c.d_rb[1].b.cap() || bytes > c.h_rb[1].b.cap()) {
    for (int k = 0; k < 2; ++k) { release(c.d_rb[k].b); release(c.h_rb[k].b); }
    for (int k = 0; k < 2; ++k) if (!reserve(c.d_rb[k].b, bytes) || !reserve(c.h_rb[k].b, bytes)) return false;
  }
  for (int k = 0; k < 2; ++k) { touch(c.d_rb[k].b, bytes); touch(c.h_rb[k].b, bytes); }
  return true;
}
static bool build(Ctx& c, size_t n_pos, bool uv)
{
  c.cap_pos = 0;
  const size_t cap = 2 * n_pos;
  release(c.tris.b); if (!reserve(c.tris.b, 4 * cap)) return false;
  release(c.shade.b); if (!reserve(c.shade.b, 4 * cap)) return false;
  release(c.uvs.b); if (uv && !reserve(c.uvs.b, 2 * cap)) return false;
  release(c.verts.b); if (!reserve(c.verts.b, 3 * cap)) return false;
  c.cap_pos = cap; c.n_pos = n_pos;
  return true;
}
static void scene_is_renderable(Ctx& c)      // every array holds what cap_pos promises
{
  CHECK(c.tris.b.cap() >= 4 * c.cap_pos && c.shade.b.cap() >= 4 * c.cap_pos && c.verts.b.cap() >= 3 * c.cap_pos && (!c.uvs.b || c.uvs.b.cap() >= 2 * c.cap_pos) && c.n_pos <= c.cap_pos);
  touch(c.tris.b, 4 * c.cap_pos); touch(c.shade.b, 4 * c.cap_pos); touch(c.verts.b, 3 * c.cap_pos); if (c.uvs.b) touch(c.uvs.b, 2 * c.cap_pos);
}
static bool add_object(Ctx& c, size_t nT)
{
  if (!c.cap_pos) return false;                            // (not built)
  if (c.n_pos + nT > c.cap_pos) {
    const size_t cap = c.n_pos + 2 * nT + c.cap_pos / 4;
    const bool ok = reserve_keep(c.tris.b, 4 * cap, 4 * c.n_pos) && reserve_keep(c.shade.b, 4 * cap, 4 * c.n_pos) && (!c.uvs.b || reserve_keep(c.uvs.b, 2 * cap, 2 * c.n_pos)) &&
                    reserve_keep(c.verts.b, 3 * cap, 3 * c.n_pos);
    scene_is_renderable(c);                                // refused half-way: some arrays grown, cap_pos as before
    if (!ok) return false;
    c.cap_pos = cap;
  }
  c.n_pos += nT;
  scene_is_renderable(c);
  return true;
}
static bool ensure_paths(Ctx& c, size_t need) { for (int i = 0; i < 3; ++i) if (!reserve(c.path[i].b, 16 * need)) return false; return true; }
static void path_budget_down(Ctx& c) { for (int i = 0; i < 3; ++i) release(c.path[i].b); }
static bool set_materials(Ctx& c, size_t n)                // dev_put: grows with head-room, and allocates 256 bytes for nothing at all
{
  if (n > c.mats.b.cap() || !c.mats.b) { if (!reserve(c.mats.b, n ? n + 16 : 16)) return false; }
  return true;
}

static void script()
{
  g_steps = 0;
  {
    Ctx c; invariants();
    // 1. the scratch buffer: grows, is refused, and the read-out of the EARLIER size must not find the old capacity beside a null pointer
    read_ldr(c, 64); read_ldr(c, 200); read_ldr(c, 64); read_ldr(c, 200); read_ldr(c, 10);
    // 2. the word arrays: a refused growth, then a call that the old capacity would have let through
    render(c, 5, 1); render(c, 41, 16); render(c, 5, 1); render(c, 41, 16); render(c, 40, 2);
    // 3. the tile statistics: the pair and the sampler's three, both entry points, both directions
    tile_stats(c, 4); adaptive(c, 4); tile_stats(c, 35); tile_stats(c, 35); adaptive(c, 35); adaptive(c, 4); tile_stats(c, 70); tile_stats(c, 4); adaptive(c, 70);
    // 4. the read-back pairs: refused growth, then a read-back of the earlier size
    read_begin(c, 300); read_begin(c, 1200); read_begin(c, 300); read_begin(c, 1200); read_begin(c, 100);
    // 5. the four leaf-ordered arrays behind ONE logical capacity
    add_object(c, 3);                                      // (before any build: refused by the caller)
    build(c, 10, true); build(c, 10, true);
    for (int i = 0; i < 6; ++i) add_object(c, 9);
    build(c, 6, false); build(c, 6, false);
    for (int i = 0; i < 4; ++i) add_object(c, 5);
    // the path state both ways, dev_put, temporaries of one call, moves
    ensure_paths(c, 100); ensure_paths(c, 100); path_budget_down(c); ensure_paths(c, 30); ensure_paths(c, 100); ensure_paths(c, 100);
    set_materials(c, 0); set_materials(c, 3); set_materials(c, 40); set_materials(c, 40); set_materials(c, 2);
    for (int i = 0; i < 2; ++i) { Watched<uint32_t> xy; Watched<Rec16> rays; if (reserve(xy.b, 14) && reserve(rays.b, 14)) touch(rays.b, 14); }      // crh_camera_rays
    invariants();
    {
      Watched<uint32_t> a, b;
      reserve(a.b, 9); reserve(b.b, 3);
      b.b = std::move(a.b); invariants();                  // the target's old block goes, the source is empty
      CHECK((uint32_t*)a.b == nullptr && a.b.cap() == 0);
      reserve(a.b, 2); reserve(a.b, 2);
      Watched<uint32_t> d; d.b = FBuf<uint32_t>(std::move(b.b)); invariants();
      CHECK((uint32_t*)b.b == nullptr && ((uint32_t*)d.b == nullptr) == (d.b.cap() == 0));
      FBuf<uint32_t>& self = d.b; d.b = std::move(self); invariants();
    }
    invariants();
  }
  CHECK(g_bufs.empty());
  CHECK(Fake::live.empty());                               // scope exit released the rest
}

int main()
{
  Fake::refuse_at = 0; script();
  const long n_allocs = Fake::allocs, clean_steps = g_steps;
  CHECK(!Fake::fired && n_allocs > 60);
  for (long k = 1; k <= n_allocs; ++k) {
    Fake::allocs = Fake::frees = 0; Fake::fired = false; Fake::refuse_at = k;
    script();
    CHECK(Fake::fired);
  }
  printf("ok: %ld allocations in the clean run (%ld steps), each refused in turn\n", n_allocs, clean_steps);
  return 0;
}
