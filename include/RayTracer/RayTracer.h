// RayTracer/RayTracer.h -- source-compatible rt::RayTracer (reference RayTracer/RayTracer.h:14-41).
//
// Same class name, base, public methods, parameter order, types and units as the reference,
// implemented header-only over the C ABI of librt_mi355x.so (../rt_mi355x.h): link with
// -lrt_mi355x.  Nothing throws (the reference swallows every failure, RayTracerImpl.cu:42-45,
// 307-314); LastError() tells what went wrong.  Methods below the marker are additive.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../Common/Color.h"
#include "../Common/Math.h"
#include "../Common/Sptr.h"
#include "../rt_mi355x.h"
#include "RaytracerCallback.h"

namespace rt {

class RayTracer : public ISptr<RayTracer> {
public:
  RayTracer(const math::uvec2& imageSize, const math::vec3& cameraPosition, const math::vec2& cameraAngles,
            const float fov, const float focalLength, const float aperture)
      : RayTracer(imageSize, cameraPosition, cameraAngles, fov, focalLength, aperture, nullptr) {}

  ~RayTracer() { rt_tracer_destroy(mImpl); }
  RayTracer(const RayTracer&) = delete;
  RayTracer& operator=(const RayTracer&) = delete;

  void Trace(const uint32_t iterationCount, const uint32_t samplesPerIteration, const uint32_t updateInterval) {
    if (mImpl) rt_tracer_trace(mImpl, iterationCount, samplesPerIteration, updateInterval);
  }
  void Stop() { rt_tracer_stop(mImpl); }
  void Resize(const math::uvec2& size) {
    const uint32_t s[2] = {size.x, size.y};
    if (mImpl) rt_tracer_resize(mImpl, s);
  }
  void SetCameraParameters(const float fov, const float focalLength, const float aperture) {
    rt_tracer_set_camera_parameters(mImpl, fov, focalLength, aperture);
  }
  void RotateCamera(const math::vec2& angles) {
    const float a[2] = {angles.x, angles.y};
    rt_tracer_rotate_camera(mImpl, a);
  }
  void UploadScene(const std::vector<float4>& hostData) {
    static_assert(sizeof(float4) == sizeof(rt_float4), "float4 layout");
    if (mImpl) rt_tracer_upload_scene(mImpl, reinterpret_cast<const rt_float4*>(hostData.data()), hostData.size());
  }
  // (the render thread may be inside OnUpdate/OnFinished meanwhile: the std::function is swapped under a
  //  mutex and the trampolines call a copy)
  void SetUpdateCallback(rt::CallBackFunction callback) {
    const bool on = static_cast<bool>(callback);
    { std::lock_guard<std::mutex> lk(mCallbackMutex); mUpdate = std::move(callback); }
    rt_tracer_set_update_callback(mImpl, on ? &RayTracer::OnUpdate : nullptr, this);
  }
  void SetFinishedCallback(rt::CallBackFunction callback) {
    const bool on = static_cast<bool>(callback);
    { std::lock_guard<std::mutex> lk(mCallbackMutex); mFinished = std::move(callback); }
    rt_tracer_set_finished_callback(mImpl, on ? &RayTracer::OnFinished : nullptr, this);
  }

  // ---- additive extensions (not in the reference) ---------------------------------------
  RayTracer(const math::uvec2& imageSize, const math::vec3& cameraPosition, const math::vec2& cameraAngles,
            const float fov, const float focalLength, const float aperture, const rt_options* options)
      : mImpl(nullptr) {
    const uint32_t size[2] = {imageSize.x, imageSize.y};
    const float pos[3] = {cameraPosition.x, cameraPosition.y, cameraPosition.z};
    const float ang[2] = {cameraAngles.x, cameraAngles.y};
    rt_tracer_create_ex(size, pos, ang, fov, focalLength, aperture, options, &mImpl);
  }
  // The frame sharded in row bands over several GPUs of this process, band k on devices[k] (the reference
  // pins device 0, OpenGLView/GLCanvas.cpp:259-260); same methods, the callbacks receive the whole frame.
  RayTracer(const math::uvec2& imageSize, const math::vec3& cameraPosition, const math::vec2& cameraAngles,
            const float fov, const float focalLength, const float aperture, const std::vector<int>& devices,
            const rt_options* options = nullptr)
      : mImpl(nullptr) {
    const uint32_t size[2] = {imageSize.x, imageSize.y};
    const float pos[3] = {cameraPosition.x, cameraPosition.y, cameraPosition.z};
    const float ang[2] = {cameraAngles.x, cameraAngles.y};
    const std::vector<int32_t> devs(devices.begin(), devices.end());
    rt_tracer_create_multi(size, pos, ang, fov, focalLength, aperture, options, devs.data(),
                           static_cast<uint32_t>(devs.size()), &mImpl);
  }
  bool Valid() const { return mImpl != nullptr; }
  bool Wait() { return mImpl && rt_tracer_wait(mImpl) == 1; }
  void SetSeed(uint64_t seed) { if (mImpl) rt_tracer_set_seed(mImpl, seed); }
  void UploadSpheres(const std::vector<float4>& spheres) {
    if (mImpl) rt_tracer_upload_spheres(mImpl, reinterpret_cast<const rt_float4*>(spheres.data()), spheres.size());
  }
  // (v0, e0 = v1-v0, e1 = v2-v0) rows with packed vertex normals in .w (Documentation/gpu.meshes.txt:16-34;
  // pack with rt::pack, Common/NormalPacking.h); smooth shading needs RT_FLAG_SMOOTH_NORMALS in rt_options
  void UploadSceneEdges(const std::vector<float4>& hostData) {
    if (mImpl) rt_tracer_upload_scene_edges(mImpl, reinterpret_cast<const rt_float4*>(hostData.data()), hostData.size());
  }
  bool ReadRenderBuffer(std::vector<float>& rgba) {
    if (!mImpl) return false;
    rgba.resize(rt_tracer_buffer_bytes(mImpl, RT_BUF_RENDER) / sizeof(float));
    return rt_tracer_read_buffer(mImpl, RT_BUF_RENDER, rgba.data(), rgba.size() * sizeof(float)) == RT_OK;
  }
  bool ReadSampleCounts(std::vector<uint32_t>& counts) {
    if (!mImpl) return false;
    counts.resize(rt_tracer_buffer_bytes(mImpl, RT_BUF_COUNTS) / sizeof(uint32_t));
    return rt_tracer_read_buffer(mImpl, RT_BUF_COUNTS, counts.data(), counts.size() * sizeof(uint32_t)) == RT_OK;
  }
  // Ray queries (rt_mi355x.h "ray queries"): the tracer's arithmetic and hit rule; rays are origin, direction pairs used as
  // given.  hits[i].prim = triangle index, n_tris + sphere index, or RT_PRIM_NONE.
  bool Intersect(const std::vector<math::vec3>& rays, std::vector<rt_hit>& hits) {
    static_assert(sizeof(math::vec3) == 3 * sizeof(float), "vec3 layout");
    hits.resize(rays.size() / 2);
    return mImpl && rays.size() % 2 == 0 &&
           rt_tracer_intersect(mImpl, reinterpret_cast<const float*>(rays.data()), hits.size(), hits.data()) == RT_OK;
  }
  // Visibility (rt_mi355x.h, rt_tracer_occluded): segs holds 8 floats per ray -- origin, direction (used as given), tmin, tmax;
  // occluded[i] = 1 when anything in the scene is hit with tmin <= t <= tmax.  Independent of the hit rule.
  bool Occluded(const std::vector<float>& segs, std::vector<uint8_t>& occluded) {
    occluded.resize(segs.size() / 8);
    return mImpl && segs.size() % 8 == 0 && rt_tracer_occluded(mImpl, segs.data(), occluded.size(), occluded.data()) == RT_OK;
  }
  // Exposure (rt_mi355x.h, rt_tracer_exposure): points holds 8 floats per point -- origin, unit normal, tmin, tmax; dirs 4 floats
  // per direction {x, y, z, -}, 1 .. RT_MAX_DIRS of them, in the frame of each point's normal (z along it) or, with world,
  // used as given.  Bit j of masks[i] is set when direction j from point i is open: Occluded would answer 0 for that segment.
  // A vector whose size does not fit, no direction or more than RT_MAX_DIRS: false, masks untouched.
  bool Exposure(const std::vector<float>& points, const std::vector<float>& dirs, std::vector<uint64_t>& masks, bool world = false) {
    if (!mImpl || points.size() % 8 != 0 || dirs.size() % 4 != 0 || dirs.empty() || dirs.size() / 4 > RT_MAX_DIRS) return false;
    masks.resize(points.size() / 8);
    return rt_tracer_exposure(mImpl, points.data(), masks.size(), dirs.data(), static_cast<uint32_t>(dirs.size() / 4),
                              world ? RT_EXPOSURE_WORLD : RT_EXPOSURE_LOCAL, masks.data()) == RT_OK;
  }
  // The same, returning the masks: empty when the vectors were rejected or the call failed (LastError()).
  std::vector<uint64_t> Exposure(const std::vector<float>& points, const std::vector<float>& dirs, bool world = false) {
    std::vector<uint64_t> masks;
    if (!Exposure(points, dirs, masks, world)) masks.clear();
    return masks;
  }
  // A cosine-weighted Fibonacci set on the hemisphere z > 0 for Exposure's local frame, 4 floats {x, y, z, 0} per sample:
  // sample k at r^2 = (k + 1/2) / samples, phi = (k + 1/2) * pi * (3 - sqrt(5)), in double, rounded to float once.
  static std::vector<float> HemisphereDirections(uint32_t samples) {
    std::vector<float> d(static_cast<size_t>(samples) * 4, 0.0f);
    for (uint32_t k = 0; k < samples; ++k) {
      const double h = static_cast<double>(k) + 0.5, r2 = h / static_cast<double>(samples);
      const double phi = h * (3.141592653589793238462643383279502884 * (3.0 - std::sqrt(5.0))), r = std::sqrt(r2);
      d[4 * k] = static_cast<float>(r * std::cos(phi));
      d[4 * k + 1] = static_cast<float>(r * std::sin(phi));
      d[4 * k + 2] = static_cast<float>(std::sqrt(1.0 - r2));
    }
    return d;
  }
  // All hits (rt_mi355x.h, rt_tracer_intersect_all): the same segments; row i of hits (maxHits records) holds the ray's first
  // counts[i] <= maxHits in-interval hits in ascending (t, prim) order, then records {0, 0, 0, RT_PRIM_NONE}.  counts[i] ==
  // maxHits: there may be more.  1 <= maxHits <= RT_MAX_HITS.  A segment vector whose size is no multiple of 8: false, the
  // outputs untouched.
  bool IntersectAll(const std::vector<float>& segs, uint32_t maxHits, std::vector<rt_hit>& hits, std::vector<uint32_t>& counts) {
    if (!mImpl || segs.size() % 8 != 0 || maxHits == 0 || maxHits > RT_MAX_HITS) return false;
    const size_t n = segs.size() / 8;
    hits.resize(n * maxHits);
    counts.resize(n);
    return rt_tracer_intersect_all(mImpl, segs.data(), n, maxHits, hits.data(), counts.data()) == RT_OK;
  }
  // Point query (rt_mi355x.h, rt_tracer_closest_point): pts holds 4 floats per point -- x, y, z and the SQUARED search radius
  // (+inf = unbounded); hits[i].t = the squared distance to the nearest surface point, u, v its barycentrics (the point is
  // v0 + u*e1 + v*e2 of triangle prim), prim = RT_PRIM_NONE when nothing lies within the radius.  A vector whose size is no
  // multiple of 4: false, hits untouched.
  bool ClosestPoint(const std::vector<float>& pts, std::vector<rt_hit>& hits) {
    if (!mImpl || pts.size() % 4 != 0) return false;
    hits.resize(pts.size() / 4);
    return rt_tracer_closest_point(mImpl, pts.data(), hits.size(), hits.data()) == RT_OK;
  }
  // The same, returning the hits: empty when the vector was rejected or the call failed (LastError()).
  std::vector<rt_hit> ClosestPoint(const std::vector<float>& pts) {
    std::vector<rt_hit> hits;
    if (!ClosestPoint(pts, hits)) hits.clear();
    return hits;
  }
  // The k nearest primitives (rt_mi355x.h, rt_tracer_closest_all): the same points; row i of hits (maxHits records) holds the
  // point's counts[i] <= maxHits nearest primitives within its radius in ascending (t, prim) order, then records {0, 0, 0,
  // RT_PRIM_NONE}; record 0 is ClosestPoint's answer.  counts[i] == maxHits: there may be more -- call again with after[i] =
  // the row's last record.  after: empty (no cursor) or one record per point.  1 <= maxHits <= RT_MAX_HITS.  A point vector
  // whose size is no multiple of 4, or an after of another length: false, the outputs untouched.
  bool ClosestAll(const std::vector<float>& pts, uint32_t maxHits, std::vector<rt_hit>& hits, std::vector<uint32_t>& counts,
                  const std::vector<rt_hit>& after = std::vector<rt_hit>()) {
    if (!mImpl || pts.size() % 4 != 0 || maxHits == 0 || maxHits > RT_MAX_HITS) return false;
    const size_t n = pts.size() / 4;
    if (!after.empty() && after.size() != n) return false;
    hits.resize(n * maxHits);
    counts.resize(n);
    return rt_tracer_closest_all(mImpl, pts.data(), after.empty() ? nullptr : after.data(), n, maxHits, hits.data(), counts.data()) == RT_OK;
  }
  // The same, returning the rows (n * maxHits records): empty when the arguments were rejected or the call failed.
  std::vector<rt_hit> ClosestAll(const std::vector<float>& pts, uint32_t maxHits) {
    std::vector<rt_hit> hits;
    std::vector<uint32_t> counts;
    if (!ClosestAll(pts, maxHits, hits, counts)) hits.clear();
    return hits;
  }
  // Region query (rt_mi355x.h, rt_tracer_overlap): boxes holds 8 floats per box, lo.x lo.y lo.z _ hi.x hi.y hi.z _ (the pads are
  // never read).  Row i of prims (maxHits ints) holds the min(counts[i], maxHits) lowest primitives that touch box i in
  // ascending order, then RT_PRIM_NONE; counts[i] is their TOTAL behind the cursor, so counts[i] > maxHits means there are more
  // -- call again with after[i] = the row's last prim.  after: empty (no cursor) or one int per box.  0 <= maxHits <=
  // RT_MAX_HITS (0: counts only).  A box vector whose size is no multiple of 8, or an after of another length: false, the
  // outputs untouched.
  bool Overlap(const std::vector<float>& boxes, uint32_t maxHits, std::vector<int32_t>& prims, std::vector<uint32_t>& counts,
               const std::vector<int32_t>& after = std::vector<int32_t>()) {
    return Region(rt_tracer_overlap, 8, boxes, maxHits, prims, counts, after);
  }
  // The same, returning the counts: empty when the arguments were rejected or the call failed (LastError()).
  std::vector<uint32_t> Overlap(const std::vector<float>& boxes, uint32_t maxHits = 0) {
    std::vector<int32_t> prims;
    std::vector<uint32_t> counts;
    if (!Overlap(boxes, maxHits, prims, counts)) counts.clear();
    return counts;
  }
  // Triangle-shaped region query (rt_mi355x.h, rt_tracer_overlap_triangles): tris holds 12 floats per query triangle, P0.xyz _
  // P1.xyz _ P2.xyz _ (the pads are never read).  prims, counts, after and maxHits are Overlap's: row i holds the
  // min(counts[i], maxHits) lowest primitives that touch triangle i, then RT_PRIM_NONE; counts[i] is their TOTAL behind the
  // cursor.  Closed: touching counts, and a query corner bit-equal to a corner of a scene triangle's record always touches it; a
  // query with a non-finite coordinate touches nothing.  A vector whose size is no multiple of 12, or an after of another
  // length: false, the outputs untouched.
  bool OverlapTriangles(const std::vector<float>& tris, uint32_t maxHits, std::vector<int32_t>& prims, std::vector<uint32_t>& counts,
                        const std::vector<int32_t>& after = std::vector<int32_t>()) {
    return Region(rt_tracer_overlap_triangles, 12, tris, maxHits, prims, counts, after);
  }
  // The same, returning the counts: empty when the arguments were rejected or the call failed (LastError()).
  std::vector<uint32_t> OverlapTriangles(const std::vector<float>& tris, uint32_t maxHits = 0) {
    std::vector<int32_t> prims;
    std::vector<uint32_t> counts;
    if (!OverlapTriangles(tris, maxHits, prims, counts)) counts.clear();
    return counts;
  }
  // Triangle distance (rt_mi355x.h, rt_tracer_triangle_distance): tris holds 12 floats per query triangle, P0.xyz d2max P1.xyz _
  // P2.xyz _ -- OverlapTriangles' layout with the SQUARED search radius in the first pad (+inf = unbounded).  hits[i] is
  // ClosestPoint's record for the nearest primitive of triangle i (t = the squared distance, u, v on the scene's triangle prim,
  // RT_PRIM_NONE when nothing lies within the radius); witness[i] is the nearest point ON THE QUERY triangle and the index of
  // the candidate that found it (-1: none).  (t, u, v) is ClosestPoint's answer for the point witness[i] on that prim, bit for
  // bit.  A vector whose size is no multiple of 12: false, the outputs untouched.
  bool TriangleDistance(const std::vector<float>& tris, std::vector<rt_hit>& hits, std::vector<rt_witness>& witness) {
    if (!mImpl || tris.size() % 12 != 0) return false;
    hits.resize(tris.size() / 12);
    witness.resize(tris.size() / 12);
    return rt_tracer_triangle_distance(mImpl, tris.data(), hits.size(), hits.data(), witness.data()) == RT_OK;
  }
  // The same, returning the hits: empty when the vector was rejected or the call failed (LastError()).
  std::vector<rt_hit> TriangleDistance(const std::vector<float>& tris) {
    std::vector<rt_hit> hits;
    std::vector<rt_witness> witness;
    if (!TriangleDistance(tris, hits, witness)) hits.clear();
    return hits;
  }
  // Hexahedron-shaped region query (rt_mi355x.h, rt_tracer_overlap_hexahedra): hexa holds 32 floats per region, eight rows
  // C_k.xyz _ (the pads are never read) in box-like order: bit 0 of k is the side along the region's first direction, bit 1 the
  // second, bit 2 the third -- an oriented or sheared box, a frustum (C0..C3 the near rectangle, C4..C7 the far one), a pyramid,
  // a segment.  prims, counts, after and maxHits are Overlap's: row i holds the min(counts[i], maxHits) lowest primitives that
  // touch region i, then RT_PRIM_NONE; counts[i] is their TOTAL behind the cursor.  Closed: touching counts; a region with a
  // non-finite coordinate touches nothing.  A vector whose size is no multiple of 32, or an after of another length: false,
  // the outputs untouched.
  bool OverlapHexahedra(const std::vector<float>& hexa, uint32_t maxHits, std::vector<int32_t>& prims, std::vector<uint32_t>& counts,
                        const std::vector<int32_t>& after = std::vector<int32_t>()) {
    return Region(rt_tracer_overlap_hexahedra, 32, hexa, maxHits, prims, counts, after);
  }
  // The same, returning the counts: empty when the arguments were rejected or the call failed (LastError()).
  std::vector<uint32_t> OverlapHexahedra(const std::vector<float>& hexa, uint32_t maxHits = 0) {
    std::vector<int32_t> prims;
    std::vector<uint32_t> counts;
    if (!OverlapHexahedra(hexa, maxHits, prims, counts)) counts.clear();
    return counts;
  }
  // Section query (rt_mi355x.h, rt_tracer_section): planes holds 8 floats per plane or slab, n.x n.y n.z d0 d1 _ _ _ (the pads are
  // never read): the region d0 <= n.x <= d1, a plane when d0 == d1, a half-space when one end is infinite; n is used as given.
  // prims, counts, after and maxHits are Overlap's: row i holds the min(counts[i], maxHits) lowest primitives slab i cuts, then
  // RT_PRIM_NONE; counts[i] is their TOTAL behind the cursor.  Closed: touching counts; a non-finite normal, a NaN or d0 > d1
  // cuts nothing.  A vector whose size is no multiple of 8, or an after of another length: false, the outputs untouched.
  bool Section(const std::vector<float>& planes, uint32_t maxHits, std::vector<int32_t>& prims, std::vector<uint32_t>& counts,
               const std::vector<int32_t>& after = std::vector<int32_t>()) {
    return Region(rt_tracer_section, 8, planes, maxHits, prims, counts, after);
  }
  // The same, returning the counts: empty when the arguments were rejected or the call failed (LastError()).
  std::vector<uint32_t> Section(const std::vector<float>& planes, uint32_t maxHits = 0) {
    std::vector<int32_t> prims;
    std::vector<uint32_t> counts;
    if (!Section(planes, maxHits, prims, counts)) counts.clear();
    return counts;
  }
  // Where the plane n.x = d0 (side 0) or d1 (side 1) cuts the prims Section returned (rt_mi355x.h, rt_tracer_section_segments):
  // prims holds perPlane ints per plane (a row of Section with maxHits = perPlane); cuts[j] is the rt_cut of prims[j] --
  // RT_CUT_SEGMENT from p0 to p1, RT_CUT_TOUCH, RT_CUT_COPLANAR, RT_CUT_CIRCLE or RT_CUT_NONE.  Sizes that do not fit: false,
  // cuts untouched.
  bool SectionSegments(const std::vector<float>& planes, const std::vector<int32_t>& prims, uint32_t perPlane, uint32_t side,
                       std::vector<rt_cut>& cuts) {
    if (!mImpl || planes.size() % 8 != 0 || perPlane == 0 || prims.size() != planes.size() / 8 * perPlane) return false;
    std::vector<rt_cut> out(prims.size());
    if (rt_tracer_section_segments(mImpl, planes.data(), prims.data(), planes.size() / 8, perPlane, side, out.data()) != RT_OK) return false;
    cuts.swap(out);
    return true;
  }
  // Swept query (rt_mi355x.h, rt_tracer_sphere_cast): sweeps holds 8 floats per sweep -- origin, direction (used as given), the
  // sphere's radius, tmax; the centre runs along o + t*d for 0 <= t <= tmax.  hits[i].t = the time of first contact, u, v the
  // barycentrics of the contact point on triangle prim (0, 0 for a sphere), prim = RT_PRIM_NONE when nothing is touched.  A
  // reported contact is within RT_SWEEP_SLACK * (max|c| + r) of touching.  A vector whose size is no multiple of 8: false,
  // hits untouched.
  bool SphereCast(const std::vector<float>& sweeps, std::vector<rt_hit>& hits) {
    if (!mImpl || sweeps.size() % 8 != 0) return false;
    hits.resize(sweeps.size() / 8);
    return rt_tracer_sphere_cast(mImpl, sweeps.data(), hits.size(), hits.data()) == RT_OK;
  }
  // The same, returning the hits: empty when the vector was rejected or the call failed (LastError()).
  std::vector<rt_hit> SphereCast(const std::vector<float>& sweeps) {
    std::vector<rt_hit> hits;
    if (!SphereCast(sweeps, hits)) hits.clear();
    return hits;
  }
  // Signed point query (rt_mi355x.h, rt_tracer_signed_distance): the same points; hits is ClosestPoint's answer bit for bit,
  // sides[i].s > 0 in front of the nearest surface (outside a closed, outward-wound mesh), < 0 behind it, 0 on it or undecided;
  // sides[i].feature names the face, vertex or edge that holds the nearest point (RT_FEATURE_SPHERE for a sphere,
  // RT_FEATURE_NONE with s = 0 when nothing lies within the radius).  The signed distance is copysign(sqrt(hits[i].t),
  // sides[i].s).  A vector whose size is no multiple of 4: false, the outputs untouched.
  bool SignedDistance(const std::vector<float>& pts, std::vector<rt_hit>& hits, std::vector<rt_side>& sides) {
    if (!mImpl || pts.size() % 4 != 0) return false;
    hits.resize(pts.size() / 4);
    sides.resize(pts.size() / 4);
    return rt_tracer_signed_distance(mImpl, pts.data(), hits.size(), hits.data(), sides.data()) == RT_OK;
  }
  // The same, returning the sides: empty when the vector was rejected or the call failed (LastError()).
  std::vector<rt_side> SignedDistance(const std::vector<float>& pts) {
    std::vector<rt_hit> hits;
    std::vector<rt_side> sides;
    if (!SignedDistance(pts, hits, sides)) sides.clear();
    return sides;
  }
  // The sides of records the caller has: hits holds perPoint records per point (1 for ClosestPoint's answers, maxHits for
  // ClosestAll's rows; unfilled records come back as {0, RT_FEATURE_NONE}).  Sizes that do not fit: false, sides untouched.
  bool ClosestSides(const std::vector<float>& pts, const std::vector<rt_hit>& hits, std::vector<rt_side>& sides) {
    if (!mImpl || pts.size() % 4 != 0) return false;
    const size_t n = pts.size() / 4;
    if (n == 0) { if (!hits.empty()) return false; sides.clear(); return true; }
    if (hits.size() % n != 0 || hits.size() / n == 0 || hits.size() / n > RT_MAX_HITS) return false;
    sides.resize(hits.size());
    return rt_tracer_closest_sides(mImpl, pts.data(), hits.data(), n, static_cast<uint32_t>(hits.size() / n), sides.data()) == RT_OK;
  }
  // The pinhole ray of a full-image pixel; `ray` (origin, direction) when asked for: the hit point is o + t * d.
  bool Pick(const math::uvec2& pixel, rt_hit& hit) { return Pick(pixel, hit, nullptr); }
  bool Pick(const math::uvec2& pixel, rt_hit& hit, math::vec3 ray[2]) {
    const uint32_t px[2] = {pixel.x, pixel.y};
    float r[6];
    if (!mImpl || rt_tracer_pick(mImpl, px, 1, &hit, r) != RT_OK) return false;
    if (ray) { ray[0] = math::vec3(r[0], r[1], r[2]); ray[1] = math::vec3(r[3], r[4], r[5]); }
    return true;
  }
  // Click to focus: the focal length becomes the distance to what the pixel sees (fov and aperture unchanged).
  bool FocusAt(const math::uvec2& pixel, float* focalLength = nullptr) {
    return mImpl && rt_tracer_focus_at(mImpl, pixel.x, pixel.y, focalLength) == RT_OK;
  }
  // Opt-in BVH for Intersect / Pick / FocusAt (rt_tracer_set_query_accel; false = the default scan).  Same answers for every
  // ray whose scan winner is well conditioned (rt_mi355x.h, "ray queries"); the tree is built by the next query.
  bool SetQueryAcceleration(bool bvh) { return mImpl && rt_tracer_set_query_accel(mImpl, bvh ? RT_QUERY_BVH : RT_QUERY_SCAN) == RT_OK; }
  struct QueryAccel { bool bvh, valid; uint64_t nodes, leaves, depth, alwaysTested, buildMicroseconds, deviceBytes; };
  QueryAccel QueryAccelInfo() const {
    uint64_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mImpl) (void)rt_tracer_query_accel_info(mImpl, o);
    return QueryAccel{o[0] == RT_QUERY_BVH, o[1] != 0, o[2], o[3], o[4], o[5], o[6], o[7]};
  }
  // What an upload does to that tree (rt_tracer_set_query_accel_update): false = the next query builds a new one on the host
  // (default); true = an upload of the same number of triangles keeps the topology and the next query refits the boxes on the
  // device.  Same contracts either way; QueryAccelUpdateInfo().cost against costBuilt tells how far the tree has degraded.
  bool SetQueryAccelUpdate(bool refit) { return mImpl && rt_tracer_set_query_accel_update(mImpl, refit ? RT_ACCEL_REFIT : RT_ACCEL_REBUILD) == RT_OK; }
  bool RebuildQueryAccel() { return mImpl && rt_tracer_query_accel_rebuild(mImpl) == RT_OK; }
  struct QueryAccelUpdate { bool refit; uint64_t refits, fallbacks, refitMicroseconds; double cost, costBuilt; };
  QueryAccelUpdate QueryAccelUpdateInfo() const {
    uint64_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mImpl) (void)rt_tracer_query_accel_update_info(mImpl, o);
    QueryAccelUpdate u{o[0] == RT_ACCEL_REFIT, o[1], o[2], o[3], 0.0, 0.0};
    std::memcpy(&u.cost, &o[4], sizeof(double));
    std::memcpy(&u.costBuilt, &o[5], sizeof(double));
    return u;
  }
  std::string LastError() const { return mImpl ? rt_tracer_last_error(mImpl) : rt_last_error(); }
  rt_tracer* Handle() const { return mImpl; }

private:
  static void OnUpdate(uint32_t* image, size_t size, void* self) {
    RayTracer* const me = static_cast<RayTracer*>(self);
    rt::CallBackFunction f;
    { std::lock_guard<std::mutex> lk(me->mCallbackMutex); f = me->mUpdate; }
    if (f) f(image, size);
  }
  static void OnFinished(uint32_t* image, size_t size, void* self) {
    RayTracer* const me = static_cast<RayTracer*>(self);
    rt::CallBackFunction f;
    { std::lock_guard<std::mutex> lk(me->mCallbackMutex); f = me->mFinished; }
    if (f) f(image, size);
  }
  // the three region queries: `floats` per query, one C entry point each
  bool Region(int (*query)(rt_tracer*, const float*, const int32_t*, size_t, uint32_t, int32_t*, uint32_t*), size_t floats,
              const std::vector<float>& queries, uint32_t maxHits, std::vector<int32_t>& prims, std::vector<uint32_t>& counts,
              const std::vector<int32_t>& after) {
    if (!mImpl || queries.size() % floats != 0 || maxHits > RT_MAX_HITS) return false;
    const size_t n = queries.size() / floats;
    if (!after.empty() && after.size() != n) return false;
    prims.resize(n * maxHits);
    counts.resize(n);
    return query(mImpl, queries.data(), after.empty() ? nullptr : after.data(), n, maxHits, maxHits != 0 ? prims.data() : nullptr,
                 counts.data()) == RT_OK;
  }

  rt_tracer* mImpl;
  std::mutex mCallbackMutex;
  rt::CallBackFunction mUpdate, mFinished;
};

}  // namespace rt
