/* crh_spec.h -- the places where this project's frozen algorithm spec DELIBERATELY departs from what the
 * OCCT 7.3-era GLSL path tracer is recollected to do ([OCCT-ext]: no OCCT source, header or shader is on
 * disk, so neither the recollection nor the departure can be verified here -- parity against the real renderer is UNPINNED).
 *
 * Every departure is a named switch, so that somebody with an OCCT build can flip them one at a time and measure which
 * setting the real renderer agrees with (tools/occt_pin/ is the kit for that).  The DEFAULT of every switch is the behaviour
 * all committed golden vectors were generated with; product (cadrays_amd/csrc) and CPU oracle (oracle/) honour the same
 * switches through the same struct, and tests/test_spec_switches.py keeps them bit-identical with every switch flipped.
 *
 *  #  switch                         default (this spec)                          alternative (OCCT as recollected)
 *  1  crh_spec.uniform_32bit         u = (state >> 8) * 2^-24  in [0, 1)          u = float(state) * 2^-32, rounds to 1.0 for the top 128 states
 *                                     -- never 1.0, so sqrt(1 - u), the light pick and the lobe pick need no guard
 *  2  crh_spec.texel_gamma2          texels handed over are LINEAR float data      the lookup squares the FILTERED texel (pow(rgb, 2): the shader's
 *                                     (the file readers square 8-bit images on       stand-in for sRGB decoding of 8-bit env maps / diffuse maps);
 *                                     the host, before filtering)                    callers then hand over the raw image values in [0, 1]
 *  3  crh_spec.mis_single_lobe       MIS weight of a BSDF-sampled ray uses the     pdf of the SAMPLED lobe times its selection probability only
 *                                     mixture pdf over all non-delta lobes           (what SampleBsdfLayered returns); NEE still evaluates the mixture,
 *                                     (weights of the two strategies sum to 1)       so the two weights no longer sum to one where lobes overlap
 *  4  CRH_SPEC_ORDER_EXACT (build)   child order key = entry-distance bits with    exact entry distance, ties by slot (a full float compare per
 *                                     the slot index in the two low mantissa bits    comparator); changes visit counters and the winner among hits at
 *                                     (one 32-bit integer sort key per child)        EQUAL t only -- compile-time because it sits in the traversal loop
 *  5  CRH_BVH_LEAF_SIZE (format)     one triangle per leaf (crh_bvh_format.h: a    OCCT's builder stops at ~5 triangles (Appendix A "(?)").  NOT a
 *                                     leaf reference IS a triangle index; measured   switch: fixed by the node format, and image-neutral -- the nearest
 *                                     +14 % on the 1 M-triangle soup) hit does not depend on the tree, only the winner among equal t
 *  6  crh_spec.eps_rule              eps = max(1e-6, 1e-5 * |scene diagonal|)      eps = max(1e-6, 1e-4 * scene radius), radius = |diagonal| / 2
 *                                     (crh_params.scene_epsilon > 0 overrides both)
 *  7  crh_spec.eta_no_dielectric     specular transmission under a coat that is    any other index for that case (e.g. 1.5, the material editor's
 *                                     NOT a dielectric is index-matched: eta = 1     default glass index, MaterialEditor.cxx:789-806)
 *  -- round 4: the Appendix-A "(?)" choices that were constants, so that the kit spans every recollected choice (round-3 verdict item 5) --
 *  9  crh_spec.rr_start_bounce       Russian roulette from bounce 3 on             any other first bounce (0 = from the camera ray's first hit on)
 * 10  crh_spec.rr_survival_cap       survival probability min(luma(W), 0.95)       any other cap in (0, 1]  (1 = no cap)
 * 11  crh_spec.min_contribution      an NEE sample is traced when a channel of     any other threshold >= 0 (Appendix A: MIN_CONTRIBUTION = vec3(1e-2) "(?)")
 *                                     its MIS-weighted contribution exceeds 1e-2
 * 12  crh_spec.min_throughput        a path goes on while a channel of its         any other threshold >= 0 (Appendix A: MIN_THROUGHPUT = vec3(1e-3) "(?)")
 *                                     throughput exceeds 1e-3
 * 13  crh_spec.raygen_bilinear       0: d = norm(fwd + right * ndc.x * tan(fovy/2)  1: bilinear blend of the four frustum-corner directions by the pixel's
 *                                     * aspect + up * ndc.y * tan(fovy/2))           position in [0,1]^2, then normalised (SURVEY a2 / Appendix A GenerateRay) --
 *                                                                                    the corners unnormalised: the same direction up to rounding;
 *                                                                                    2: the corner directions NORMALISED before the blend (what a shader gets
 *                                                                                    when the host uploads unit vectors): rays bend towards the image centre
 * 14  crh_spec.env_orientation       lat-long lookup u = (atan2(d.y, d.x) + pi) /   1: Appendix A's FetchEnvironment: u = atan2(d.y, d.x) / (2 pi) (wraps),
 *                                     (2 pi), v = acos(d.z) / pi (row 0 = zenith)    v = acos(-d.z) / pi -- the map turned by half a turn and upside down
 *  -- round 6: the first switch whose default is backed by an OUTPUT OF THE REAL RENDERER (the icons under data/materials, tests/golden/icon_features.json) --
 * 15  crh_spec.display_gamma22       display value = sqrt(v): gamma 2.  The 25      1: v ^ (1 / 2.2), this project's default up to round 5 (SURVEY Appendix A's
 *                                     icons OCCT rendered from preview.tcl show a    recollection of Display.fs).  The icons refute it: 2.2 would put the tile
 *                                     lit 0.85 tile over its 0.45 neighbour at       ratio at 1.335
 *                                     1.365 .. 1.382 = (0.85 / 0.45) ^ (1 / gamma)
 *                                     with gamma 1.97 .. 2.04 on every icon
 *     (not a switch) the display rule before the gamma: NaN / negative -> 0, times 2^exposure, in filmic mode hable(v) / hable(white point) with the curve's
 *     input cut at 2^60 -- it saturates, so +inf and anything whose square overflows is drawn white, as in linear mode -- then clamp to [0, 1]
 *
 * Reference evidence that these are the knobs that matter: the only numbers CADRays itself pins are the BSDF / light / camera /
 * parameter vectors of its input contract (cadrays_hip.h cites them line by line); everything in the table is arithmetic inside
 * OCCT's shaders, reached through V3d_View::Redraw() (src/Launcher/AppViewer.cxx:1047).
 */
#ifndef CRH_SPEC_H
#define CRH_SPEC_H

#include <stdint.h>

typedef struct crh_spec {
  uint32_t size;                /* sizeof(crh_spec) AS THE CALLER KNOWS IT: a caller built against an older, shorter struct passes its own size and the
                                 * fields it does not know take their defaults (crh_spec_normalise); a size larger than this library's is refused */
  int32_t  uniform_32bit;       /* #1 */
  int32_t  texel_gamma2;        /* #2 */
  int32_t  mis_single_lobe;     /* #3 */
  int32_t  eps_rule;            /* #6: 0 = 1e-5 * diagonal, 1 = 1e-4 * radius */
  float    eta_no_dielectric;   /* #7: 1e-2 .. 1e3; default 1 */
  /* ---- round 4 (size 24 -> 48) */
  int32_t  rr_start_bounce;     /* #9: 0 .. 32; default 3 */
  float    rr_survival_cap;     /* #10: (0, 1]; default 0.95 */
  float    min_contribution;    /* #11: >= 0; default 1e-2 */
  float    min_throughput;      /* #12: >= 0; default 1e-3 */
  int32_t  raygen_bilinear;     /* #13: 0 tan form, 1 blend of unnormalised corners, 2 blend of normalised corners */
  int32_t  env_orientation;     /* #14: 0 / 1 */
  /* ---- round 6 (size 48 -> 52) */
  int32_t  display_gamma22;     /* #15: 0 = sqrt (gamma 2, what the reference's icons show), 1 = v^(1/2.2) */
} crh_spec;

#define CRH_SPEC_DEFAULTS {(uint32_t)sizeof(crh_spec), 0, 0, 0, 0, 1.0f, 3, 0.95f, 1.0e-2f, 1.0e-3f, 0, 0, 0}
#define CRH_SPEC_SIZE_R3 24u    /* the struct of round 3: {size .. eta_no_dielectric} */
#define CRH_SPEC_SIZE_R5 48u    /* rounds 4 - 5: {.. env_orientation} */

/* What crh_set_spec (product) and the oracle's twin both do with a caller's struct: copy the first min(in->size, sizeof) bytes over the defaults,
 * check the ranges, turn the flags into 0 / 1.  Returns 0, or -1 with *why (a static string) set.  Input contract, shared like the structs. */
static inline int crh_spec_normalise(const crh_spec* in, crh_spec* out, const char** why)
{
  static const crh_spec defaults = CRH_SPEC_DEFAULTS;
  const char* dummy; if (!why) why = &dummy;
  if (!in || !out) { *why = "null spec"; return -1; }
  if (in->size < CRH_SPEC_SIZE_R3 || in->size > (uint32_t)sizeof(crh_spec) || (in->size & 3u)) { *why = "crh_spec.size is neither this library's struct nor an older one"; return -1; }
  crh_spec s = defaults;
  { const unsigned char* src = (const unsigned char*)in; unsigned char* dst = (unsigned char*)&s; for (uint32_t i = 4; i < in->size; ++i) dst[i] = src[i]; }
  s.size = (uint32_t)sizeof(crh_spec);
  if (!(s.eta_no_dielectric >= 1.0e-2f && s.eta_no_dielectric <= 1.0e3f)) { *why = "eta_no_dielectric must be in 1e-2 .. 1e3"; return -1; }
  if (s.rr_start_bounce < 0 || s.rr_start_bounce > 32) { *why = "rr_start_bounce must be in 0 .. 32"; return -1; }
  if (!(s.rr_survival_cap > 0.f && s.rr_survival_cap <= 1.0f)) { *why = "rr_survival_cap must be in (0, 1]"; return -1; }
  if (!(s.min_contribution >= 0.f && s.min_contribution <= 3.0e38f) || !(s.min_throughput >= 0.f && s.min_throughput <= 3.0e38f)) { *why = "min_contribution / min_throughput must be finite and >= 0"; return -1; }
  if (s.raygen_bilinear < 0 || s.raygen_bilinear > 2) { *why = "raygen_bilinear must be 0, 1 or 2"; return -1; }
  if (s.env_orientation < 0 || s.env_orientation > 1) { *why = "env_orientation must be 0 or 1"; return -1; }
  s.display_gamma22 = s.display_gamma22 != 0;
  s.uniform_32bit = s.uniform_32bit != 0; s.texel_gamma2 = s.texel_gamma2 != 0; s.mis_single_lobe = s.mis_single_lobe != 0; s.eps_rule = s.eps_rule != 0;
  *out = s;
  return 0;
}

/* What crh_get_spec (product) and the oracle's twin do: `out->size` is IN / OUT -- the caller sets it to sizeof(crh_spec) AS IT KNOWS THE STRUCT
 * (24 for a caller built against round 3's header) and exactly that many bytes are written: the switches the caller's struct has room for, nothing
 * past it; size stays the caller's.  size == 0 -- a zero-initialised struct, which round 3's contract allowed -- means "the oldest struct":
 * CRH_SPEC_SIZE_R3 bytes are written (every struct this header ever declared has room for them) and size is SET to 24 so that the caller can see
 * how far the answer goes.  Any other size that is neither this library's nor an older struct's (below CRH_SPEC_SIZE_R3, above sizeof(crh_spec),
 * not a multiple of 4) is refused and nothing is written.  Returns 0 / -1 with *why set. */
static inline int crh_spec_export(const crh_spec* have, crh_spec* out, const char** why)
{
  const char* dummy; if (!why) why = &dummy;
  if (!have || !out) { *why = "null spec"; return -1; }
  uint32_t n = out->size;
  if (n == 0u) n = out->size = CRH_SPEC_SIZE_R3;
  if (n < CRH_SPEC_SIZE_R3 || n > (uint32_t)sizeof(crh_spec) || (n & 3u)) { *why = "crh_spec.size must hold the caller's sizeof(crh_spec) before crh_get_spec (24 .. this library's, a multiple of 4)"; return -1; }
  { const unsigned char* src = (const unsigned char*)have; unsigned char* dst = (unsigned char*)out; for (uint32_t i = 4; i < n; ++i) dst[i] = src[i]; }
  return 0;
}

/* #4: build-time (traversal inner loop).  0 = quantised key (default), 1 = exact distance order, ties by slot. */
#ifndef CRH_SPEC_ORDER_EXACT
#define CRH_SPEC_ORDER_EXACT 0
#endif

/* #8: build-time.  Child order of ANY-HIT (shadow-ray) traversal: 0 = near to far like nearest-hit rays (default; what OCCT's
 * SceneAnyHit is recollected to do, it shares the ordered walk), 1 = slot order -- an occlusion query needs no order, and the walk
 * then needs no sort (round-2 verdict item 3).  Changes the any-hit visit counters only: visibility is order-independent. */
#ifndef CRH_SPEC_ANYHIT_SLOT_ORDER
#define CRH_SPEC_ANYHIT_SLOT_ORDER 0
#endif

#endif /* CRH_SPEC_H */
