// crh_fit.cpp -- fit the view to the displayed or chosen objects: V3d_View::FitAll / ZFitAll as the application drives them (reference src/Launcher/AppViewer.cxx:704,
// 764-767, 788, 886).  One pass over the vertices on the device reduces six maxima per object (fit_kernels.hip; the host twin runs the same per-vertex function), a
// closed-form rule in double turns the maxima of the chosen objects into a camera.  Nothing of the rendering state is touched and nothing restarts: the host hands
// the fitted camera to crh_set_camera itself.  The arithmetic is DESIGN.md section 4.9.
// (one of the translation units behind include/cadrays_hip.h; the context, the shared helpers and the map of the files: crh_context.h)
#include <cmath>

#include "crh_context.h"
#include "fit_kernels.h"

using namespace crh;
using namespace crh::api;

namespace {

struct FitSetup { FitFrame F; float tan_half, aspect; };

bool finite_camera(const crh_camera& cam)
{
  const float v[] = {cam.eye[0], cam.eye[1], cam.eye[2], cam.dir[0], cam.dir[1], cam.dir[2], cam.up[0], cam.up[1], cam.up[2], cam.fovy_deg, cam.aspect, cam.ortho_scale,
                     cam.aperture_radius, cam.focal_dist};
  return all_finite(v, sizeof v / sizeof v[0]);
}

// The frame and the slopes.  right / up / fwd, tan_half and aspect are camera_frame's (crh_context.h), as fill_scene's are; kx and ky in double, rounded once.
const char* fit_setup(const crh_camera& cam, uint32_t W, uint32_t H, float margin, FitSetup& S)
{
  if (!(margin >= 0.f && margin <= 0.9f)) return "margin outside [0, 0.9]";
  if (!finite_camera(cam)) return "the camera holds a NaN / Inf";
  if (!(cam.aspect > 0.f) && (!W || !H)) return "aspect <= 0 needs a target size";
  const CameraFrame cf = camera_frame(cam, W, H);
  const crh_v3 fwd = cf.fwd, right = cf.right, up = cf.up;
  S.tan_half = cf.tan_half; S.aspect = cf.aspect;
  FitFrame& F = S.F;
  for (int a = 0; a < 3; ++a) F.pivot[a] = cam.eye[a];
  F.right[0] = right.x; F.right[1] = right.y; F.right[2] = right.z;
  F.up[0] = up.x; F.up[1] = up.y; F.up[2] = up.z;
  F.fwd[0] = fwd.x; F.fwd[1] = fwd.y; F.fwd[2] = fwd.z;
  if (cam.is_ortho) { F.kx = F.ky = 0.f; }
  else {
    F.kx = (float)(((double)S.tan_half * (double)S.aspect) * (1.0 - (double)margin));
    F.ky = (float)((double)S.tan_half * (1.0 - (double)margin));
    if (!(F.kx > 0.f && F.ky > 0.f) || !all_finite(&F.kx, 1) || !all_finite(&F.ky, 1)) return "the field of view leaves no positive slope";
  }
  const float fr[] = {right.x, right.y, right.z, up.x, up.y, up.z, fwd.x, fwd.y, fwd.z, S.aspect};
  if (!all_finite(fr, 10)) return "the camera frame is not finite";
  return nullptr;
}

void frame_to_result(const FitSetup& S, crh_fit_result& r)
{
  std::memset(&r, 0, sizeof r);
  for (int a = 0; a < 3; ++a) { r.right[a] = S.F.right[a]; r.up[a] = S.F.up[a]; r.fwd[a] = S.F.fwd[a]; }
  r.kx = S.F.kx; r.ky = S.F.ky;
}

// The rule: double arithmetic on the float32 extents, every output rounded to float32 once (the header states it; tests/fit_reference.py restates it).
const char* fit_rule(const float e[6], const FitSetup& S, const crh_camera& cam, float margin, uint32_t n_vertices, crh_camera* cam_out, crh_fit_result* out)
{
  if (!all_finite(e, 6)) return "an extent is NaN / Inf";
  const double R = e[0], L = e[1], U = e[2], D = e[3], N = e[4], Fz = e[5];
  const double ex = (R - L) / 2.0, ey = (U - D) / 2.0;
  double ez, half = 0.0; int binding;
  if (!cam.is_ortho) {
    const double zx = -(R + L) / (2.0 * (double)S.F.kx), zy = -(U + D) / (2.0 * (double)S.F.ky), clear = -N - (Fz + N) / 16.0;
    ez = zx; binding = 0;
    if (zy < ez) { ez = zy; binding = 1; }
    if (clear < ez) { ez = clear; binding = 2; }
  } else {
    const double hv = (U + D) / 2.0, hh = (R + L) / (2.0 * (double)S.aspect);
    binding = hv >= hh ? 1 : 0;
    half = (hv >= hh ? hv : hh) / (1.0 - (double)margin);
    const double depth = Fz + N, wide = 2.0 * half;
    ez = -N - (depth >= wide ? depth : wide);
  }
  const double zn = -N - ez, zf = Fz - ez;
  crh_camera o = cam;
  for (int a = 0; a < 3; ++a)
    o.eye[a] = (float)((((double)S.F.pivot[a] + ex * (double)S.F.right[a]) + ey * (double)S.F.up[a]) + ez * (double)S.F.fwd[a]);
  if (cam.is_ortho) o.ortho_scale = (float)half;
  const float chk[] = {o.eye[0], o.eye[1], o.eye[2], o.ortho_scale, (float)zn, (float)zf};
  if (!all_finite(chk, 6) || !std::isfinite(ez)) return "the fitted camera is not finite";
  if (!(zn > 0.0)) return "all chosen vertices coincide (z_near <= 0)";
  *cam_out = o;
  if (out) {
    frame_to_result(S, *out);
    for (int j = 0; j < 6; ++j) out->extents[j] = e[j];
    out->z_near = (float)zn; out->z_far = (float)zf; out->n_vertices = n_vertices; out->binding = binding;
  }
  return nullptr;
}

void records_to_extents(const uint32_t* rec, uint32_t nO, float* extents_out, uint32_t* counts_out)
{
  for (uint32_t o = 0; o < nO; ++o) {
    const uint32_t* r = rec + (size_t)kFitRec * o;
    if (extents_out) for (int j = 0; j < 6; ++j) extents_out[6 * (size_t)o + j] = r[6] ? fit_unkey(r[j]) : -INFINITY;
    if (counts_out) counts_out[o] = r[6];
  }
}

// {x, y, z, object as int bits} per vertex from the context's host arrays: the object of the triangles that reference it (every vertex belongs to ONE object,
// crh_set_geometry checks it; object 0 for a scene handed over without objects), -1 where no triangle does
void build_fit_verts(const crh_ctx* c, std::vector<float>& v4)
{
  const size_t nV = c->pos.size() / 3, nT = c->tri.size() / 4;
  std::vector<int32_t> owner(nV, -1);
  const bool objs = !c->tri_obj.empty();
  for (size_t t = 0; t < nT; ++t)
    for (int k = 0; k < 3; ++k) owner[(size_t)c->tri[4 * t + k]] = objs ? c->tri_obj[t] : 0;
  v4.resize(4 * nV);
  for (size_t i = 0; i < nV; ++i) {
    v4[4 * i] = c->pos[3 * i]; v4[4 * i + 1] = c->pos[3 * i + 1]; v4[4 * i + 2] = c->pos[3 * i + 2];
    std::memcpy(&v4[4 * i + 3], &owner[i], 4);
  }
}

void fill_objects(std::vector<FitObject>& tab, const float* xf, uint32_t nO)
{
  static const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  tab.resize(nO);
  for (uint32_t o = 0; o < nO; ++o) {
    std::memcpy(tab[o].m, xf ? xf + 12 * (size_t)o : I, sizeof I);
    tab[o].on = 1u; tab[o].pad[0] = tab[o].pad[1] = tab[o].pad[2] = 0u;
  }
}

}  // namespace

extern "C" {

int crh_fit_view(crh_ctx* c, const crh_camera* cam_in, const uint8_t* chosen, uint32_t n_objects, float margin, crh_camera* cam_out, crh_fit_result* out, float* extents_out)
{
  if (!c || !cam_out) return fail(c, CRH_E_INVALID, "crh_fit_view: null camera output");
  if (!c->built) return fail(c, CRH_E_NOTBUILT, "crh_build has not been called");
  const uint32_t nO = n_pick_objects(c);
  if (n_objects != nO) { char b[128]; snprintf(b, sizeof b, "crh_fit_view: %u flags for a scene of %u objects", n_objects, nO); return fail(c, CRH_E_INVALID, b); }
  const crh_camera cam = cam_in ? *cam_in : c->cam;
  FitSetup S;
  if (const char* why = fit_setup(cam, c->par.width, c->par.height, margin, S)) { std::string m = std::string("crh_fit_view: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  std::vector<FitObject> tab;
  fill_objects(tab, c->tri_obj.empty() ? nullptr : c->xf.data(), nO);
  std::vector<uint8_t> want(nO);
  for (uint32_t o = 0; o < nO; ++o) {
    want[o] = chosen ? (chosen[o] ? 1 : 0) : ((c->hidden.size() == nO && c->hidden[o]) ? 0 : 1);      // NULL: every displayed object
    tab[o].on = (want[o] || extents_out) ? 1u : 0u;
  }
  CRH_HIP(hipSetDevice(c->device));
  int rc = pick_stream(c); if (rc) return rc;
  if (c->fit_verts_gen != c->geom_gen) {                 // the first fit after the geometry changed: build the array and upload it
    std::vector<float> v4; build_fit_verts(c, v4);
    if ((rc = side_upload(c, c->d_fit_verts, reinterpret_cast<const float4*>(v4.data()), v4.size() / 4))) return rc;
    c->fit_n = (uint32_t)(v4.size() / 4); c->fit_verts_gen = c->geom_gen;
  }
  CRH_HIP(c->d_fit_objs.reserve(sizeof(FitObject) * nO, sizeof(FitObject) * 16)); CRH_HIP(c->d_fit_rec.reserve((size_t)kFitRec * nO, (size_t)kFitRec * 16));
  std::vector<uint32_t> rec((size_t)kFitRec * nO, 0u);
  CRH_HIP(hipMemcpyAsync(c->d_fit_objs, tab.data(), sizeof(FitObject) * nO, hipMemcpyHostToDevice, c->pk_stream));
  CRH_HIP(hipMemsetAsync(c->d_fit_rec, 0, sizeof(uint32_t) * kFitRec * nO, c->pk_stream));
  launch_fit_extents(c->pk_stream, c->grid, c->d_fit_verts, c->fit_n, c->d_fit_objs.as<const FitObject>(), nO, S.F, c->d_fit_rec);
  CRH_HIP(hipGetLastError());
  CRH_HIP(hipMemcpyAsync(rec.data(), c->d_fit_rec, sizeof(uint32_t) * kFitRec * nO, hipMemcpyDeviceToHost, c->pk_stream));
  CRH_HIP(hipStreamSynchronize(c->pk_stream));
  if (extents_out) records_to_extents(rec.data(), nO, extents_out, nullptr);
  uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u}, n = 0u;    // the key maximum over the chosen objects' records
  for (uint32_t o = 0; o < nO; ++o) {
    const uint32_t* r = &rec[(size_t)kFitRec * o];
    if (!want[o] || !r[6]) continue;
    for (int j = 0; j < 6; ++j) if (r[j] > k[j]) k[j] = r[j];
    n += r[6];
  }
  if (!n) return fail(c, CRH_E_INVALID, "crh_fit_view: no chosen object has a vertex");
  float e[6]; for (int j = 0; j < 6; ++j) e[j] = fit_unkey(k[j]);
  if (const char* why = fit_rule(e, S, cam, margin, n, cam_out, out)) { std::string m = std::string("crh_fit_view: ") + why; return fail(c, CRH_E_INVALID, m.c_str()); }
  return CRH_OK;
}

int crh_fit_extents_host(const float* verts4, uint32_t n_vertices, const float* obj_xform, uint32_t n_objects, const crh_camera* cam, uint32_t width, uint32_t height,
                         float margin, float* extents_out, uint32_t* counts_out, crh_fit_result* frame_out)
{
  if ((n_vertices && !verts4) || !n_objects || !cam || !extents_out) return CRH_E_INVALID;
  if (obj_xform && !all_finite(obj_xform, 12 * (size_t)n_objects)) return CRH_E_INVALID;
  FitSetup S;
  if (fit_setup(*cam, width, height, margin, S)) return CRH_E_INVALID;
  std::vector<FitObject> tab;
  fill_objects(tab, obj_xform, n_objects);
  std::vector<uint32_t> rec((size_t)kFitRec * n_objects, 0u);
  fit_extents_host(verts4, n_vertices, tab.data(), n_objects, S.F, rec.data());
  records_to_extents(rec.data(), n_objects, extents_out, counts_out);
  if (frame_out) frame_to_result(S, *frame_out);
  return CRH_OK;
}

int crh_fit_from_extents(const float extents[6], const crh_camera* cam, uint32_t width, uint32_t height, float margin, crh_camera* cam_out, crh_fit_result* out)
{
  if (!extents || !cam || !cam_out) return CRH_E_INVALID;
  FitSetup S;
  if (fit_setup(*cam, width, height, margin, S)) return CRH_E_INVALID;
  return fit_rule(extents, S, *cam, margin, 0u, cam_out, out) ? CRH_E_INVALID : CRH_OK;
}

}  // extern "C"
