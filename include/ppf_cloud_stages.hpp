/*
 * ppf_cloud_stages.hpp — header-only C++ wrapper of the device-resident cloud stages (ppf_cloud_* / ppf_prep_* in
 * ppf_hip.h): the PCL half of the reference's ppf::CloudProcessor (/root/reference/include/CloudProcessing.h)
 *
 *   Deprojection       :262      ->  Cloud::fromDepth(depth, rows, cols, fx, fy, ppx, ppy) / fromDepthU16(..., scale, ...)
 *   (nothing: pcl::IntegralImageNormalEstimation would be it) ->  Cloud::fromDepth(depth, rows, cols, normalParams, fx, ...)  (with normals and curvature)
 *   SceneCropping      :263-339  ->  Cloud::crop(box, depth, rows, cols, fx, fy, ppx, ppy)
 *   Subsampling        :361-380  ->  Cloud::voxelGrid(leaf)
 *   OutlierProcessing  :341-360  ->  Cloud::outlierRemoval(meanK, stddevMul)
 *   NormalEstimation   :381-405  ->  Cloud::normals(k)
 *   EdgeExtraction     :406-427  ->  Cloud::edges(curvatureThreshold)
 *   PointCloudXYZNormalToMat :163-190 -> Cloud::toMat()   (an N x 6 ppf_match_3d::Mat for PPF3DDetector / ICP)
 *   (nothing: pcl::SACSegmentation would be it)    ->  Cloud::removePlanes(params) / Cloud::applyPlanes(planes)  (the table or wall taken out)
 *   (nothing: pcl::EuclideanClusterExtraction would be it) ->  Cloud::clusters(params, info, intr, ...)  (a plane-free cloud split into objects and their boxes)
 *   (nothing: pcl::RegionGrowing would be it)              ->  Cloud::regions(params, info, intr, ...)   (a cloud with normals split into smooth surface regions)
 *   all of the above for every box of a frame  ->  Cloud::prepareFrame(boxes, n, depth, ...)  (one (object, edge) pair per box)
 *   Matching_S2B + ICP for every detection     ->  Cloud::matchFrame(models, modelClouds, dets, ...)  (ICP in one launch sequence)
 *   `// TODO: Pose Validation` (:477-479, :530-532) -> Cloud::verifyFrame(modelClouds, dets, poses, depth, ...)  (scores, best pose)
 *                                                     Cloud::verifyFrameRendered(...)  (the same with self-occlusion)
 *   transformPCPose -> writePLY of the result       ->  Cloud::renderFrame(modelClouds, poses, best, ...)  (depth, label images)
 *   `return *resultsSub[0];` per box (:480, :533)   ->  Cloud::selectFrame(modelClouds, poses, depth, ...)  (one consistent set per frame)
 *   (nothing: the reference stops at the ICP pose)  ->  Cloud::refineFrame(modelClouds, poses, depth, ...)  (poses fitted to the depth image)
 *   k4a::transformation::depth_image_to_color_camera (k4a_grabber.h:339, :391) -> DepthMap::registerDepth / registerDepthU16
 *                                                     (a raw sensor depth frame aligned to the colour camera; Cloud::fromDepth takes it)
 *   (nothing: a sensor pipeline's depth clean-up)     ->  filterDepth / filterDepthU16 / DepthMap::registerFiltered
 *   (nothing: the frames of a fixed camera fused)     ->  DepthHistory::push / pushU16
 *   (nothing: the camera stands still there)          ->  depthMotion / depthMotionU16 / DepthOdometry::push  (the camera's motion between two depth frames)
 *   (nothing: the boxes come from YOLO)               ->  segmentDepth / segmentDepthU16  (the depth image's surfaces as labels and boxes)
 *   EdgeExtraction    :406 (on a depth-normals cloud) ->  depthEdges / depthEdgesU16  (the image's occluding and boundary pixels: mask and edge cloud)
 *   (nothing: the labels come from YOLO)              ->  Recognizer::recognize  (per proposal cloud the trained models it can be a view of)
 *
 * Every stage returns a new Cloud that stays in HBM; only toMat()/download() copy to the host.  A maintainer replaces
 * the bodies of those CloudProcessor methods by these one-liners; pcl::PointCloud<PointXYZ> goes
 * in through Cloud::fromXYZ(&cloud.points[0].x, cloud.size(), 4) (PointXYZ is 4 floats wide).
 */
#ifndef PPF_CLOUD_STAGES_HPP
#define PPF_CLOUD_STAGES_HPP

#include <memory>
#include <utility>
#include <vector>

#include "ppf_match_3d.hpp"

namespace ppfhip {
namespace prep {

/* ppf_depth_params of an image of `format` (PPF_DEPTH_F32: metres; PPF_DEPTH_U16: units of `scale` metres) kept inside zMin..zMax */
inline ppf_depth_params depthParams(int format, double scale, float zMin, float zMax, int flags = 0) {
  ppf_depth_params p;
  ppf_default_depth_params(&p);
  p.format = format;
  p.flags = flags;
  p.depth_scale = scale;
  p.z_min = zMin;
  p.z_max = zMax;
  return p;
}

class Cloud {
 public:
  Cloud() {}
  /* rows of `cols` (3 or 6) floats, `strideFloats` apart */
  static Cloud fromRows(const float* rows, int n, int strideFloats, int cols) {
    ppf_cloud* c = nullptr;
    ppf_match_3d::check(ppf_cloud_upload(rows, n, strideFloats, PPF_NOFF_MAT, cols, &c));
    return Cloud(c);
  }
  static Cloud fromXYZ(const float* xyz, int n, int strideFloats = 3) { return fromRows(xyz, n, strideFloats, 3); }
  /* the same with the curvature an upload leaves zero: n floats (ppf_cloud_set_curvature) */
  static Cloud fromRows(const float* rows, int n, int strideFloats, int cols, const float* curvature) {
    const Cloud c = fromRows(rows, n, strideFloats, cols);
    ppf_match_3d::check(ppf_cloud_set_curvature(c.h_.get(), curvature, n));
    return c;
  }
  /* an N x 3 or N x 6 float32 Mat (cv::Mat when OpenCV is present: rows read through step1()) */
  static Cloud fromMat(const ppf_match_3d::Mat& m) {
    return fromRows(m.ptr<float>(0), m.rows, ppf_match_3d::detail::stride_of(m), m.cols >= 6 ? 6 : 3);
  }

  /* Deprojection (:262, an empty stub in the reference): the scene cloud of a HOST depth image, back-projected on the
   * device (ppf_cloud_from_depth).  float32 metres; rows x y z 0 0 0 of every pixel with a finite z > 0 in [zMin, zMax]
   * (zMax 0: no upper bound), row-major pixel order.  fp64: the fp64 formula instead of Camera::back_projection's
   * rounding.  rowPitchBytes 0: packed rows. */
  static Cloud fromDepth(const float* depth, int rows, int cols, double fx, double fy, double ppx, double ppy, float zMin = 0.f,
                         float zMax = 0.f, bool fp64 = false, size_t rowPitchBytes = 0) {
    return fromDepthImage(depth, PPF_DEPTH_F32, 0.001, rows, cols, fx, fy, ppx, ppy, zMin, zMax, fp64, rowPitchBytes);
  }
  /* the same from a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
  static Cloud fromDepthU16(const uint16_t* depth, int rows, int cols, double scale, double fx, double fy, double ppx, double ppy,
                            float zMin = 0.f, float zMax = 0.f, bool fp64 = false, size_t rowPitchBytes = 0) {
    return fromDepthImage(depth, PPF_DEPTH_U16, scale, rows, cols, fx, fy, ppx, ppy, zMin, zMax, fp64, rowPitchBytes);
  }
  static ppf_depth_normal_params defaultDepthNormalParams() {
    ppf_depth_normal_params p;
    ppf_default_depth_normal_params(&p);
    return p;
  }
  /* the same clouds with the normal and curvature of a plane fit over each pixel's (2 radius + 1)^2 image window
   * (ppf_cloud_from_depth_normals): what crop, removePlanes, clusters, edges and toMat carry.  A pixel with fewer than
   * min_neighbours neighbours gets NaNs, or with PPF_DEPTH_NORMALS_DROP no row. */
  static Cloud fromDepth(const float* depth, int rows, int cols, const ppf_depth_normal_params& normals, double fx, double fy,
                         double ppx, double ppy, float zMin = 0.f, float zMax = 0.f, bool fp64 = false, size_t rowPitchBytes = 0) {
    return fromDepthImage(depth, PPF_DEPTH_F32, 0.001, rows, cols, fx, fy, ppx, ppy, zMin, zMax, fp64, rowPitchBytes, &normals);
  }
  static Cloud fromDepthU16(const uint16_t* depth, int rows, int cols, double scale, const ppf_depth_normal_params& normals, double fx,
                            double fy, double ppx, double ppy, float zMin = 0.f, float zMax = 0.f, bool fp64 = false,
                            size_t rowPitchBytes = 0) {
    return fromDepthImage(depth, PPF_DEPTH_U16, scale, rows, cols, fx, fy, ppx, ppy, zMin, zMax, fp64, rowPitchBytes, &normals);
  }

  static ppf_mesh_sample_params defaultMeshSampleParams() {
    ppf_mesh_sample_params p;
    ppf_default_mesh_sample_params(&p);
    return p;
  }
  /* A model cloud sampled from a triangle mesh (ppf_cloud_from_mesh): on average one row per spacing^2 of surface, without
   * the rows none of 26 views can see and with the normals turned outward; what train takes once downloaded.  vertices:
   * nVertices rows of vstride floats, x y z first and, with normalOffset >= 0, a normal there; triangles: nTriangles index
   * triples.  params == 0: defaultMeshSampleParams() (spacing 4 mm, face normals, visibility and orient on). */
  static Cloud fromMesh(const float* vertices, int nVertices, int vstride, int normalOffset, const int32_t* triangles, int nTriangles,
                        const ppf_mesh_sample_params* params = 0, ppf_mesh_sample_stats* stats = 0) {
    const ppf_mesh_sample_params mp = params ? *params : defaultMeshSampleParams();
    ppf_cloud* c = nullptr;
    ppf_match_3d::check(ppf_cloud_from_mesh(vertices, nVertices, vstride, normalOffset, triangles, nTriangles, &mp, &c, stats));
    return Cloud(c);
  }

  bool empty() const { return size() == 0; }
  int size() const {
    if (!h_) return 0;
    int n = 0;
    ppf_match_3d::check(ppf_cloud_size(h_.get(), &n));
    return n;
  }
  const ppf_cloud* handle() const { return h_.get(); }

  /* box = {x, y, width, height} of the detection; depth: host image rows x cols, metres */
  Cloud crop(const int box[4], const float* depth, int depthRows, int depthCols, double fx, double fy, double ppx, double ppy) const {
    const double intr[4] = {fx, fy, ppx, ppy};
    ppf_cloud* o = nullptr;
    ppf_match_3d::check(ppf_prep_crop(need(), box, depth, depthRows, depthCols, intr, &o));
    return Cloud(o);
  }
  Cloud voxelGrid(double leaf) const { ppf_cloud* o = nullptr; ppf_match_3d::check(ppf_prep_voxel_grid(need(), leaf, &o)); return Cloud(o); }
  Cloud outlierRemoval(int meanK = 50, double stddevMul = 1.5) const {
    ppf_cloud* o = nullptr;
    ppf_match_3d::check(ppf_prep_outlier_removal(need(), meanK, stddevMul, &o));
    return Cloud(o);
  }
  Cloud normals(int k = 30) const { ppf_cloud* o = nullptr; ppf_match_3d::check(ppf_prep_normals(need(), k, &o)); return Cloud(o); }
  Cloud edges(float curvatureThreshold) const { ppf_cloud* o = nullptr; ppf_match_3d::check(ppf_prep_edges(need(), curvatureThreshold, &o)); return Cloud(o); }

  static ppf_plane_params defaultPlaneParams() {
    ppf_plane_params p;
    ppf_default_plane_params(&p);
    return p;
  }
  /* The support planes (the table, a wall) of every cloud found and removed in one call (ppf_prep_planes), the step before
   * crop / prepareFrame: up to params->max_planes rounds of a seeded hypothesis search per cloud, each cloud's result what a
   * call with it alone gives.  Returns the kept rows per cloud, still in HBM.  info (optional): [clouds][max_planes] rows;
   * labels (optional): per cloud one byte per input row (0 kept, 1 + p inlier of plane p, 0x80 | (1 + p) behind plane p).
   * params == 0: defaultPlaneParams(). */
  static std::vector<Cloud> removePlanes(const std::vector<const Cloud*>& clouds, const ppf_plane_params* params = 0,
                                         std::vector<ppf_plane_info>* info = 0, std::vector<std::vector<uint8_t> >* labels = 0,
                                         ppf_plane_stats* stats = 0) {
    const ppf_plane_params p = orDefaults(params, ppf_default_plane_params);
    const size_t nc = clouds.size();
    const size_t planes = p.max_planes >= 1 && p.max_planes <= PPF_PLANE_MAX_PLANES ? (size_t)p.max_planes : 1;
    std::vector<const ppf_cloud*> in(nc + 1, (const ppf_cloud*)0);
    std::vector<ppf_cloud*> out(nc + 1, (ppf_cloud*)0);
    std::vector<ppf_plane_info> rows(nc * planes + 1);
    std::vector<uint8_t*> lab(nc + 1, (uint8_t*)0);
    for (size_t i = 0; i < nc; i++) {
      if (!clouds[i]) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::removePlanes: a cloud is missing");
      in[i] = clouds[i]->need();
    }
    if (labels) {
      labels->assign(nc, std::vector<uint8_t>());
      for (size_t i = 0; i < nc; i++) {
        (*labels)[i].assign((size_t)clouds[i]->size() + 1, 0);
        lab[i] = &(*labels)[i][0];
      }
    }
    ppf_match_3d::check(ppf_prep_planes(&in[0], (int)nc, &p, &out[0], &rows[0], labels ? &lab[0] : 0, stats));
    std::vector<Cloud> kept;
    for (size_t i = 0; i < nc; i++) kept.push_back(Cloud(out[i]));
    if (labels)
      for (size_t i = 0; i < nc; i++) (*labels)[i].pop_back();
    if (info) info->assign(rows.begin(), rows.begin() + (std::ptrdiff_t)(nc * planes));
    return kept;
  }
  /* this cloud without its support planes: info receives max_planes rows, labels one byte per row */
  Cloud removePlanes(const ppf_plane_params* params = 0, std::vector<ppf_plane_info>* info = 0, std::vector<uint8_t>* labels = 0,
                     ppf_plane_stats* stats = 0) const {
    std::vector<std::vector<uint8_t> > lab;
    const std::vector<Cloud> kept = removePlanes(std::vector<const Cloud*>(1, this), params, info, labels ? &lab : 0, stats);
    if (labels) labels->swap(lab[0]);
    return kept[0];
  }
  /* the rows of a companion cloud (a detection's edge cloud) that the planes removePlanes reported do not remove
   * (ppf_prep_planes_apply): the same predicate and params */
  Cloud applyPlanes(const std::vector<ppf_plane_info>& planes, const ppf_plane_params* params = 0) const {
    const ppf_plane_params p = orDefaults(params, ppf_default_plane_params);
    ppf_cloud* o = nullptr;
    ppf_match_3d::check(ppf_prep_planes_apply(need(), planes.empty() ? 0 : &planes[0], (int)planes.size(), &p, &o));
    return Cloud(o);
  }

  static ppf_cluster_params defaultClusterParams() {
    ppf_cluster_params p;
    ppf_default_cluster_params(&p);
    return p;
  }
  /* This cloud -- plane-free, so after removePlanes -- split into its object clusters (ppf_prep_clusters): the connected
   * components of "two rows are no farther apart than params->tolerance" (fp64, <=) with min_size .. max_size rows, the largest
   * first (equal sizes: the smaller first row first), at most params->max_clusters of them, each a cloud still in HBM with its
   * rows in ascending row index.  info (optional): one row per returned cluster; with intr = {fx, fy, ppx, ppy} and the image
   * size its box_xywh is the cluster's image box, what prepareFrame takes as a detection's box.  labels (optional): per row the
   * rank of its cluster or -1.  counts (optional): {clusters returned, valid components, all components}.
   * params == 0: defaultClusterParams(). */
  std::vector<Cloud> clusters(const ppf_cluster_params* params = 0, std::vector<ppf_cluster_info>* info = 0, const double* intr = 0,
                              int imageRows = 0, int imageCols = 0, std::vector<int32_t>* labels = 0, int32_t* counts = 0,
                              ppf_cluster_stats* stats = 0) const {
    const ppf_cluster_params p = orDefaults(params, ppf_default_cluster_params);
    const size_t slots = p.max_clusters >= 1 && p.max_clusters <= PPF_CLUSTER_MAX_CLUSTERS ? (size_t)p.max_clusters : 1;
    const ppf_cloud* in[1] = {need()};
    std::vector<ppf_cloud*> out(slots, (ppf_cloud*)0);
    std::vector<ppf_cluster_info> rows(slots);
    std::vector<int32_t> lab((size_t)size() + 1, -1);
    int32_t* labp[1] = {&lab[0]};
    int32_t cnt[3] = {0, 0, 0};
    ppf_match_3d::check(ppf_prep_clusters(in, 1, &p, intr, imageRows, imageCols, &out[0], &rows[0], cnt, labels ? labp : 0, stats));
    std::vector<Cloud> found;
    for (int32_t r = 0; r < cnt[0]; r++) found.push_back(Cloud(out[(size_t)r]));
    if (info) info->assign(rows.begin(), rows.begin() + cnt[0]);
    if (labels) { lab.pop_back(); labels->swap(lab); }
    if (counts) { counts[0] = cnt[0]; counts[1] = cnt[1]; counts[2] = cnt[2]; }
    return found;
  }

  static ppf_region_params defaultRegionParams() {
    ppf_region_params p;
    ppf_default_region_params(&p);
    return p;
  }
  /* This cloud, with the normals and curvature it carries (fromDepth with ppf_depth_normal_params, or normals()), split into
   * its smooth surface regions (ppf_prep_regions): what cuts objects that touch, where clusters() leaves
   * one blob.  Rows of curvature <= params->curvature_threshold are smooth; two smooth rows are linked iff they are no farther
   * apart than params->tolerance and the dot product of their normals is >= params->normal_cos (fp64; with
   * PPF_REGION_UNORIENTED its absolute value); a region is a connected component of the links plus the other (border) rows
   * whose nearest linkable smooth row is in it.  Sizes, order, info, labels and the boxes are clusters()', except that
   * info.first_row is the region's smallest smooth row.  counts (optional): {regions returned, valid components, all
   * components, border rows attached}.  params == 0: defaultRegionParams(). */
  std::vector<Cloud> regions(const ppf_region_params* params = 0, std::vector<ppf_cluster_info>* info = 0, const double* intr = 0,
                             int imageRows = 0, int imageCols = 0, std::vector<int32_t>* labels = 0, int32_t* counts = 0,
                             ppf_cluster_stats* stats = 0) const {
    const ppf_region_params p = orDefaults(params, ppf_default_region_params);
    const size_t slots = p.max_regions >= 1 && p.max_regions <= PPF_CLUSTER_MAX_CLUSTERS ? (size_t)p.max_regions : 1;
    const ppf_cloud* in[1] = {need()};
    std::vector<ppf_cloud*> out(slots, (ppf_cloud*)0);
    std::vector<ppf_cluster_info> rows(slots);
    std::vector<int32_t> lab((size_t)size() + 1, -1);
    int32_t* labp[1] = {&lab[0]};
    int32_t cnt[4] = {0, 0, 0, 0};
    ppf_match_3d::check(ppf_prep_regions(in, 1, &p, intr, imageRows, imageCols, &out[0], &rows[0], cnt, labels ? labp : 0, stats));
    std::vector<Cloud> found;
    for (int32_t r = 0; r < cnt[0]; r++) found.push_back(Cloud(out[(size_t)r]));
    if (info) info->assign(rows.begin(), rows.begin() + cnt[0]);
    if (labels) { lab.pop_back(); labels->swap(lab); }
    if (counts) { counts[0] = cnt[0]; counts[1] = cnt[1]; counts[2] = cnt[2]; counts[3] = cnt[3]; }
    return found;
  }

  static ppf_frame_params defaultFrameParams() {
    ppf_frame_params p;
    ppf_default_frame_params(&p);
    return p;
  }
  /* every stage above for all nBoxes boxes {x, y, width, height} of a frame in one call (ppf_prep_frame): one (object,
   * edge) pair of to-Mat clouds per box, still in HBM, bit-identical to crop -> ... -> toMat per box.  params NULL =
   * defaultFrameParams(); stageRows (optional) receives [nBoxes][4] rows after crop, voxel grid, outlier removal, edges. */
  std::vector<std::pair<Cloud, Cloud> > prepareFrame(const int* boxesXYWH, int nBoxes, const float* depth, int depthRows, int depthCols,
                                                     double fx, double fy, double ppx, double ppy, const ppf_frame_params* params = 0,
                                                     std::vector<int>* stageRows = 0, ppf_frame_stats* stats = 0) const {
    const double intr[4] = {fx, fy, ppx, ppy};
    const ppf_frame_params prm = params ? *params : defaultFrameParams();
    const size_t nb = nBoxes > 0 ? (size_t)nBoxes : 0;
    std::vector<ppf_cloud*> objs(nb + 1, (ppf_cloud*)0), edges(nb + 1, (ppf_cloud*)0);
    std::vector<int32_t> rows(nb * 4 + 1, 0);
    ppf_match_3d::check(ppf_prep_frame(need(), boxesXYWH, nBoxes, depth, depthRows, depthCols, intr, &prm, &objs[0], &edges[0], &rows[0],
                                       stats));
    std::vector<std::pair<Cloud, Cloud> > out;
    for (size_t i = 0; i < nb; i++) out.push_back(std::make_pair(Cloud(objs[i]), Cloud(edges[i])));
    if (stageRows) stageRows->assign(rows.begin(), rows.begin() + nb * 4);
    return out;
  }

  /* Matching_S2B (edge cloud given) or Matching, then the ICP of the top poses, for every detection of a frame in one call
   * (ppf_match_frame): the ICP of all detections runs as one launch sequence.  models[i] == 0 or an empty object cloud
   * skips detection i (its list stays empty); modelClouds[i] is the model's full cloud (ICP source, Cloud::fromMat of the
   * trained Mat).  Returns per detection its refined poses in match rank order (the reference keeps element 0), each
   * bit-identical to match + ICP of that detection alone.  Match parameters: ppf_default_match_params with the two
   * relative steps; ICP: ppf_default_icp_params. */
  static std::vector<std::vector<ppf_match_3d::Pose3D> > matchFrame(const std::vector<const ppf_model*>& models,
                                                                     const std::vector<const Cloud*>& modelClouds,
                                                                     const std::vector<std::pair<Cloud, Cloud> >& dets,
                                                                     double relativeSceneSampleStep = 0.05, double relativeSceneDistance = 0.05,
                                                                     int top = 5, std::vector<std::vector<int> >* iterations = 0,
                                                                     ppf_match_frame_stats* stats = 0) {
    const size_t nd = dets.size();
    if (models.size() != nd || modelClouds.size() != nd)
      throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::matchFrame: one model and one model cloud per detection");
    std::vector<ppf_frame_detection> d(nd + 1);
    for (size_t i = 0; i < nd; i++) {
      const bool live = models[i] && modelClouds[i] && dets[i].first.handle();
      d[i].model = live ? models[i] : 0;
      d[i].model_cloud = live ? modelClouds[i]->handle() : 0;
      d[i].scene = live ? dets[i].first.handle() : 0;
      d[i].edge = live ? dets[i].second.handle() : 0;
    }
    ppf_match_params mp;
    ppf_default_match_params(&mp);
    mp.relative_scene_sample_step = relativeSceneSampleStep;
    mp.relative_scene_distance = relativeSceneDistance;
    ppf_icp_params ip;
    ppf_default_icp_params(&ip);
    const size_t t = top > 0 ? (size_t)top : 0;
    std::vector<ppf_pose> poses(nd * t + 1);
    std::vector<int> n(nd + 1, 0);
    std::vector<int32_t> it(nd * t + 1, 0);
    ppf_match_3d::check(ppf_match_frame(&d[0], (int)nd, &mp, &ip, top, &poses[0], &n[0], &it[0], stats));
    std::vector<std::vector<ppf_match_3d::Pose3D> > out(nd);
    if (iterations) iterations->assign(nd, std::vector<int>());
    for (size_t i = 0; i < nd; i++)
      for (int k = 0; k < n[i]; k++) {
        out[i].push_back(ppf_match_3d::Pose3D(poses[i * t + (size_t)k]));
        if (iterations) (*iterations)[i].push_back(it[i * t + (size_t)k]);
      }
    return out;
  }
  /* Pose validation, the reference's TODO after `return *resultsSub[0];` (CloudProcessing.h:477-479, :530-532), for every
   * detection of a frame in one call (ppf_verify_frame): each of poses[i] (what matchFrame returns) moves modelClouds[i] and
   * is scored against dets[i].first and, with depth != 0, against the depth image (rows x cols float32 metres, the
   * intrinsics prepareFrame took).  Returns per detection one ppf_pose_score per pose; best (optional) receives per
   * detection the index of the highest score (the lowest index among equal ones, -1 without poses).  params == 0:
   * ppf_default_verify_params.  A detection with no poses, no model cloud or no object cloud is not scored. */
  static std::vector<std::vector<ppf_pose_score> > verifyFrame(const std::vector<const Cloud*>& modelClouds,
                                                               const std::vector<std::pair<Cloud, Cloud> >& dets,
                                                               const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses,
                                                               const float* depth, int rows, int cols, double fx, double fy, double ppx,
                                                               double ppy, const ppf_verify_params* params = 0,
                                                               std::vector<int>* best = 0, ppf_verify_stats* stats = 0) {
    const size_t nd = dets.size();
    if (modelClouds.size() != nd || poses.size() != nd)
      throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::verifyFrame: one model cloud and one pose list per detection");
    const PoseTable t(modelClouds, &dets, poses);
    const size_t top = t.top;
    const ppf_verify_params p = orDefaults(params, ppf_default_verify_params);
    const double intr[4] = {fx, fy, ppx, ppy};
    std::vector<ppf_pose_score> sc(nd * top + 1);
    std::vector<int> b(nd + 1, -1);
    ppf_match_3d::check(ppf_verify_frame(&t.d[0], (int)nd, &t.recs[0], &t.n[0], (int)top, depth, rows, cols, depth ? intr : 0, &p, &sc[0], &b[0],
                                         stats));
    if (best) best->assign(b.begin(), b.begin() + (std::ptrdiff_t)nd);
    return t.perDetection(sc);
  }
  /* verifyFrame with self-occlusion (ppf_verify_frame_rendered): a model row counts only where it is visible in a surfel
   * z-buffer of its own pose, rows x cols with the intrinsics prepareFrame took.  depth may be 0 (no depth test); the image
   * size is then still what the render draws into.  rparams == 0: ppf_default_render_params.  PPF_VERIFY_ALL_ROWS is
   * refused.  Otherwise as verifyFrame. */
  static std::vector<std::vector<ppf_pose_score> > verifyFrameRendered(const std::vector<const Cloud*>& modelClouds,
                                                                       const std::vector<std::pair<Cloud, Cloud> >& dets,
                                                                       const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses,
                                                                       const float* depth, int rows, int cols, double fx, double fy,
                                                                       double ppx, double ppy, const ppf_verify_params* params = 0,
                                                                       const ppf_render_params* rparams = 0, std::vector<int>* best = 0,
                                                                       ppf_verify_stats* stats = 0) {
    const size_t nd = dets.size();
    if (modelClouds.size() != nd || poses.size() != nd)
      throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::verifyFrameRendered: one model cloud and one pose list per detection");
    const PoseTable t(modelClouds, &dets, poses);
    const size_t top = t.top;
    const ppf_verify_params p = orDefaults(params, ppf_default_verify_params);
    const ppf_render_params rp = orDefaults(rparams, ppf_default_render_params);
    const double intr[4] = {fx, fy, ppx, ppy};
    std::vector<ppf_pose_score> sc(nd * top + 1);
    std::vector<int> b(nd + 1, -1);
    ppf_match_3d::check(ppf_verify_frame_rendered(&t.d[0], (int)nd, &t.recs[0], &t.n[0], (int)top, depth, rows, cols, intr, &p, &rp, &sc[0],
                                                  &b[0], stats));
    if (best) best->assign(b.begin(), b.begin() + (std::ptrdiff_t)nd);
    return t.perDetection(sc);
  }
  /* Depth and instance-label images of one chosen pose per detection (ppf_render_frame), in place of the reference's
   * transformPCPose -> writePLY dump: poses[i][which[i]] moves modelClouds[i] (which[i] < 0, or no model cloud: not drawn;
   * the best of verifyFrame / verifyFrameRendered plugs in), drawn as surfel disks into one rows x cols z-buffer.
   * depthOut (metres, 0 where empty) and labelOut (the detection index, -1 where empty) are resized to rows x cols; either
   * may be 0.  rparams == 0: ppf_default_render_params. */
  static void renderFrame(const std::vector<const Cloud*>& modelClouds, const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses,
                          const std::vector<int>& which, int rows, int cols, double fx, double fy, double ppx, double ppy,
                          std::vector<float>* depthOut, std::vector<int32_t>* labelOut, const ppf_render_params* rparams = 0,
                          ppf_render_stats* stats = 0) {
    const size_t nd = poses.size();
    if (modelClouds.size() != nd || which.size() != nd)
      throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::renderFrame: one model cloud and one pose index per detection");
    const PoseTable t(modelClouds, 0, poses);
    std::vector<int> w(nd + 1, -1);
    for (size_t i = 0; i < nd; i++) {
      const bool live = modelClouds[i] && modelClouds[i]->handle() && which[i] >= 0;
      if (live && (size_t)which[i] >= poses[i].size())
        throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::renderFrame: which[i] is past the detection's poses");
      w[i] = live ? which[i] : -1;
    }
    const ppf_render_params rp = orDefaults(rparams, ppf_default_render_params);
    const double intr[4] = {fx, fy, ppx, ppy};
    const size_t npx = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
    if (depthOut) depthOut->assign(npx, 0.f);
    if (labelOut) labelOut->assign(npx, -1);
    ppf_match_3d::check(ppf_render_frame(&t.d[0], (int)nd, &t.recs[0], &w[0], (int)t.top, rows, cols, intr, &rp,
                                         depthOut && npx ? &(*depthOut)[0] : 0, labelOut && npx ? &(*labelOut)[0] : 0, stats));
  }
  /* One consistent set among all poses of all detections of a frame (ppf_select_frame): duplicates and the
   * same object seen through overlapping boxes are suppressed, a second instance inside one box is kept.  Returns the
   * selected (detection, k) pairs in selection order.  depth is required; top is the longest pose list, and the flat index
   * of pose k of detection i is i * top + k (suppressed_by in the info rows, the values of labelOut).  scores (what either
   * verify entry returned) ranks by their score instead of the explained share.  info, when given, gets one row per pose;
   * depthOut / labelOut are resized to rows x cols, either may be 0.  params == 0 / rparams == 0: the defaults. */
  static std::vector<std::pair<int, int> > selectFrame(const std::vector<const Cloud*>& modelClouds,
                                                       const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses, const float* depth,
                                                       int rows, int cols, double fx, double fy, double ppx, double ppy,
                                                       const ppf_select_params* params = 0, const ppf_render_params* rparams = 0,
                                                       const std::vector<std::vector<ppf_pose_score> >* scores = 0,
                                                       std::vector<std::vector<ppf_select_info> >* info = 0, std::vector<float>* depthOut = 0,
                                                       std::vector<int32_t>* labelOut = 0, ppf_select_stats* stats = 0) {
    const size_t nd = poses.size();
    if (modelClouds.size() != nd || (scores && scores->size() != nd))
      throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::selectFrame: one model cloud (and one score list) per detection");
    const PoseTable t(modelClouds, 0, poses);
    const size_t top = t.top;
    std::vector<ppf_pose_score> sc(nd * top + 1);
    for (size_t i = 0; scores && i < nd; i++) {
      if ((*scores)[i].size() < (size_t)t.n[i]) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::selectFrame: fewer scores than poses");
      for (int k = 0; k < t.n[i]; k++) sc[i * top + (size_t)k] = (*scores)[i][(size_t)k];
    }
    const ppf_select_params p = orDefaults(params, ppf_default_select_params);
    const ppf_render_params rp = orDefaults(rparams, ppf_default_render_params);
    const double intr[4] = {fx, fy, ppx, ppy};
    const size_t npx = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
    if (depthOut) depthOut->assign(npx, 0.f);
    if (labelOut) labelOut->assign(npx, -1);
    std::vector<ppf_select_info> rowsOut(nd * top + 1);
    std::vector<int> sel(nd * top + 1, -1);
    int nSel = 0;
    ppf_match_3d::check(ppf_select_frame(&t.d[0], (int)nd, &t.recs[0], &t.n[0], (int)top, scores ? &sc[0] : 0, depth, rows, cols, intr, &rp, &p,
                                         &rowsOut[0], &sel[0], &nSel, depthOut && npx ? &(*depthOut)[0] : 0,
                                         labelOut && npx ? &(*labelOut)[0] : 0, stats));
    if (info) *info = t.perDetection(rowsOut);
    std::vector<std::pair<int, int> > out;
    for (int r = 0; r < nSel; r++) out.push_back(std::make_pair(sel[(size_t)r] / (int)top, sel[(size_t)r] % (int)top));
    return out;
  }
  /* Every pose of every detection refined on the depth image itself by projective point-to-plane steps (ppf_refine_frame,
   * DESIGN.md §17): to polish what selectFrame kept at full depth resolution, or to carry the poses of the last frame into
   * this frame's image without matching again.  Returns per detection its refined poses (a pose whose refinement was
   * stopped by a guard comes back as given); info, when given, gets one row per pose.  depth is required.
   * params == 0: ppf_default_refine_params.  A detection without a model cloud is not refined: its poses come back as given. */
  static std::vector<std::vector<ppf_match_3d::Pose3D> > refineFrame(const std::vector<const Cloud*>& modelClouds,
                                                                     const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses,
                                                                     const float* depth, int rows, int cols, double fx, double fy,
                                                                     double ppx, double ppy, const ppf_refine_params* params = 0,
                                                                     std::vector<std::vector<ppf_refine_info> >* info = 0,
                                                                     ppf_refine_stats* stats = 0) {
    const size_t nd = poses.size();
    if (modelClouds.size() != nd) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud::refineFrame: one model cloud per detection");
    const PoseTable t(modelClouds, 0, poses);
    const ppf_refine_params p = orDefaults(params, ppf_default_refine_params);
    const double intr[4] = {fx, fy, ppx, ppy};
    std::vector<ppf_pose> out(nd * t.top + 1);
    std::vector<ppf_refine_info> rowsOut(nd * t.top + 1);
    ppf_match_3d::check(ppf_refine_frame(&t.d[0], (int)nd, &t.recs[0], &t.n[0], (int)t.top, depth, rows, cols, intr, &p, &out[0], &rowsOut[0],
                                         stats));
    if (info) *info = t.perDetection(rowsOut);
    std::vector<std::vector<ppf_match_3d::Pose3D> > refined(nd);
    for (size_t i = 0; i < nd; i++) {
      if (t.n[i] == 0) refined[i] = poses[i]; /* not refined: as given */
      for (int k = 0; k < t.n[i]; k++) refined[i].push_back(ppf_match_3d::Pose3D(out[i * t.top + (size_t)k]));
    }
    return refined;
  }
  /* the N x 6 CV_32FC1-shaped Mat of PointCloudXYZNormalToMat (normals re-normalised) */
  ppf_match_3d::Mat toMat() const {
    ppf_cloud* o = nullptr;
    ppf_match_3d::check(ppf_prep_to_mat(need(), &o));
    Cloud tmp(o);
    const int n = tmp.size();
    ppf_match_3d::Mat m = ppf_match_3d::detail::new_cloud(n, 6);
    if (n) ppf_match_3d::check(ppf_cloud_download(tmp.handle(), m.ptr<float>(0), nullptr, n));
    return m;
  }
  /* rows (n x 6) and curvature (n) as they are on the device */
  void download(std::vector<float>& rows6, std::vector<float>& curvature) const {
    const int n = size();
    rows6.assign((size_t)n * 6, 0.f);
    curvature.assign((size_t)n, 0.f);
    if (n) ppf_match_3d::check(ppf_cloud_download(h_.get(), rows6.data(), curvature.data(), n));
  }

 private:
  /* the tables every stage after matchFrame takes: one ppf_frame_detection, `top` (the longest list, at least 1) pose records
   * and one pose count per detection, each padded by one element so that &v[0] is valid without detections.  A detection is
   * live with a model cloud, poses and, where dets is given, an object cloud; the others get no handles and count 0.
   * renderFrame draws by which[i], not by n: a live detection it does not draw (which[i] < 0) keeps its handle here, and
   * ppf_render_frame reads neither handle nor poses of a detection whose which is -1. */
  struct PoseTable {
    size_t top;
    std::vector<ppf_frame_detection> d;
    std::vector<ppf_pose> recs;
    std::vector<int> n;
    PoseTable(const std::vector<const Cloud*>& modelClouds, const std::vector<std::pair<Cloud, Cloud> >* dets,
              const std::vector<std::vector<ppf_match_3d::Pose3D> >& poses)
        : top(1), d(poses.size() + 1), n(poses.size() + 1, 0) {
      for (size_t i = 0; i < poses.size(); i++) top = poses[i].size() > top ? poses[i].size() : top;
      recs.resize(poses.size() * top + 1);
      for (size_t i = 0; i < poses.size(); i++) {
        const bool live = modelClouds[i] && modelClouds[i]->handle() && (!dets || (*dets)[i].first.handle()) && !poses[i].empty();
        d[i].model = 0;
        d[i].edge = 0;
        d[i].model_cloud = live ? modelClouds[i]->handle() : 0;
        d[i].scene = live && dets ? (*dets)[i].first.handle() : 0;
        n[i] = live ? (int)poses[i].size() : 0;
        for (int k = 0; k < n[i]; k++) recs[i * top + (size_t)k] = poses[i][(size_t)k].record();
      }
    }
    /* flat[i * top + k] -> out[i][k], the n[i] rows of each detection */
    template <class T>
    std::vector<std::vector<T> > perDetection(const std::vector<T>& flat) const {
      std::vector<std::vector<T> > out(n.size() - 1);
      for (size_t i = 0; i < out.size(); i++)
        out[i].assign(flat.begin() + (std::ptrdiff_t)(i * top), flat.begin() + (std::ptrdiff_t)(i * top + (size_t)n[i]));
      return out;
    }
  };
  template <class P>
  static P orDefaults(const P* given, void (*defaults)(P*)) { P p; if (given) p = *given; else defaults(&p); return p; }
  friend class DepthVolume; /* its extract() returns a Cloud */
  friend std::vector<uint8_t> depthEdgesImage(const void* depth, int format, double scale, int rows, int cols, const double* intr,
                                              const Cloud* normals, const ppf_depth_edge_params* params, Cloud* edgeCloud, float zMin,
                                              float zMax, bool fp64, size_t rowPitchBytes, ppf_depth_edge_stats* stats); /* fills a Cloud */
  explicit Cloud(ppf_cloud* c) : h_(c, [](ppf_cloud* p) { ppf_cloud_release(p); }) {}
  static Cloud fromDepthImage(const void* depth, int format, double scale, int rows, int cols, double fx, double fy, double ppx,
                              double ppy, float zMin, float zMax, bool fp64, size_t rowPitchBytes,
                              const ppf_depth_normal_params* normals = 0) {
    const ppf_depth_params p = depthParams(format, scale, zMin, zMax, fp64 ? PPF_DEPTH_FP64 : 0);
    const double intr[4] = {fx, fy, ppx, ppy};
    ppf_cloud* c = nullptr;
    ppf_match_3d::check(normals ? ppf_cloud_from_depth_normals(depth, rows, cols, rowPitchBytes, intr, &p, normals, &c)
                                : ppf_cloud_from_depth(depth, rows, cols, rowPitchBytes, intr, &p, &c));
    return Cloud(c);
  }
  const ppf_cloud* need() const {
    if (!h_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Cloud: empty handle");
    return h_.get();
  }
  std::shared_ptr<ppf_cloud> h_;
};

/* ppf_depth_filter: the depth image without its unsupported ("flying") pixels and smoothed inside each
 * surface, float32 metres, packed rows x cols, 0 where nothing is written: what Cloud::fromDepth and every frame stage take. */
inline ppf_depth_filter_params defaultDepthFilterParams() {
  ppf_depth_filter_params p;
  ppf_default_depth_filter_params(&p);
  return p;
}
inline std::vector<float> filterDepthImage(const void* depth, int format, double scale, int rows, int cols, const ppf_depth_filter_params* params,
                                           float zMin, float zMax, size_t rowPitchBytes, ppf_depth_filter_stats* stats) {
  const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
  const ppf_depth_filter_params fp = params ? *params : defaultDepthFilterParams();
  std::vector<float> out((rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0) + 1);
  ppf_match_3d::check(ppf_depth_filter(depth, rows, cols, rowPitchBytes, &dp, &fp, &out[0], stats));
  out.resize(out.size() - 1);
  return out;
}
/* float32 metres in; rowPitchBytes 0: packed rows; params 0: the defaults */
inline std::vector<float> filterDepth(const float* depth, int rows, int cols, const ppf_depth_filter_params* params = 0, float zMin = 0.f,
                                      float zMax = 0.f, size_t rowPitchBytes = 0, ppf_depth_filter_stats* stats = 0) {
  return filterDepthImage(depth, PPF_DEPTH_F32, 0.001, rows, cols, params, zMin, zMax, rowPitchBytes, stats);
}
/* a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
inline std::vector<float> filterDepthU16(const uint16_t* depth, int rows, int cols, double scale, const ppf_depth_filter_params* params = 0,
                                         float zMin = 0.f, float zMax = 0.f, size_t rowPitchBytes = 0, ppf_depth_filter_stats* stats = 0) {
  return filterDepthImage(depth, PPF_DEPTH_U16, scale, rows, cols, params, zMin, zMax, rowPitchBytes, stats);
}

/* ppf_depth_history: the last `window` depth images of a fixed camera, resident on the device; push takes the
 * next frame and returns the fused image (float32 metres, packed rows x cols, 0 where nothing is written), which filterDepth,
 * Cloud::fromDepth and every frame stage take.  format: PPF_DEPTH_F32 (push) or PPF_DEPTH_U16 (pushU16, z = d * scale metres).
 * Copies share the history. */
class DepthHistory {
 public:
  static ppf_depth_history_params defaultParams() {
    ppf_depth_history_params p;
    ppf_default_depth_history_params(&p);
    return p;
  }
  DepthHistory() : rows_(0), cols_(0) {}
  DepthHistory(int rows, int cols, const ppf_depth_history_params* params = 0, int format = PPF_DEPTH_F32, double scale = 0.001,
               float zMin = 0.f, float zMax = 0.f)
      : rows_(rows), cols_(cols) {
    const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
    const ppf_depth_history_params hp = params ? *params : defaultParams();
    ppf_depth_history* h = nullptr;
    ppf_match_3d::check(ppf_depth_history_create(rows, cols, &dp, &hp, &h));
    h_ = std::shared_ptr<ppf_depth_history>(h, [](ppf_depth_history* p) { ppf_depth_history_release(p); });
  }
  int rows() const { return rows_; }
  int cols() const { return cols_; }
  ppf_depth_history* handle() const { return h_.get(); }

  /* float32 metres in; rowPitchBytes 0: packed rows; state: 0, or it receives the packed rows x cols state image */
  std::vector<float> push(const float* depth, std::vector<uint8_t>* state = 0, ppf_depth_history_stats* stats = 0, size_t rowPitchBytes = 0) {
    return run(depth, state, stats, rowPitchBytes);
  }
  /* a 16-bit sensor image, for a history made with PPF_DEPTH_U16 */
  std::vector<float> pushU16(const uint16_t* depth, std::vector<uint8_t>* state = 0, ppf_depth_history_stats* stats = 0,
                             size_t rowPitchBytes = 0) {
    return run(depth, state, stats, rowPitchBytes);
  }
  /* forget every frame */
  void reset() { ppf_match_3d::check(ppf_depth_history_reset(need())); }
  ppf_depth_history_desc info() const {
    ppf_depth_history_desc d;
    ppf_match_3d::check(ppf_depth_history_info(need(), &d));
    return d;
  }

 private:
  ppf_depth_history* need() const {
    if (!h_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::DepthHistory: empty handle");
    return h_.get();
  }
  std::vector<float> run(const void* depth, std::vector<uint8_t>* state, ppf_depth_history_stats* stats, size_t rowPitchBytes) {
    const size_t n = (size_t)rows_ * (size_t)cols_;
    std::vector<float> out(n + 1);
    std::vector<uint8_t> st(state ? n + 1 : 1);
    ppf_match_3d::check(ppf_depth_history_push(need(), depth, rowPitchBytes, &out[0], state ? &st[0] : 0, stats));
    out.resize(n);
    if (state) {
      st.resize(n);
      state->swap(st);
    }
    return out;
  }
  std::shared_ptr<ppf_depth_history> h_;
  int rows_, cols_;
};

/* ppf_depth_motion: the camera's rigid motion between two depth images of one size and format.  T (16 doubles,
 * row-major) takes a static point's coordinates in the previous camera frame to the current one: a pose of the previous frame
 * is T * pose in the current one.  status is the status of the last level reached; PPF_MOTION_LOST or PPF_MOTION_STEP: not
 * found, T is the start. */
struct DepthMotion {
  double T[16];
  int status;
  ppf_depth_motion_level levels[PPF_MOTION_MAX_LEVELS];
  ppf_depth_motion_stats stats;
  bool found() const { return status != PPF_MOTION_LOST && status != PPF_MOTION_STEP; }
};
inline ppf_depth_motion_params defaultDepthMotionParams() {
  ppf_depth_motion_params p;
  ppf_default_depth_motion_params(&p);
  return p;
}
inline DepthMotion depthMotionImage(const void* prev, const void* cur, int format, double scale, int rows, int cols, const double* intr,
                                    const ppf_depth_motion_params* params, const double* init16, float zMin, float zMax,
                                    size_t prevPitchBytes, size_t curPitchBytes) {
  const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
  const ppf_depth_motion_params mp = params ? *params : defaultDepthMotionParams();
  DepthMotion m;
  ppf_match_3d::check(ppf_depth_motion(prev, prevPitchBytes, cur, curPitchBytes, rows, cols, intr, &dp, &mp, init16, m.T, m.levels, &m.stats));
  m.status = m.stats.status;
  return m;
}
/* float32 metres in; intr = {fx, fy, ppx, ppy}; params 0: the defaults; init16 0: the identity; a pitch of 0: packed rows */
inline DepthMotion depthMotion(const float* prev, const float* cur, int rows, int cols, const double* intr,
                               const ppf_depth_motion_params* params = 0, const double* init16 = 0, float zMin = 0.f, float zMax = 0.f,
                               size_t prevPitchBytes = 0, size_t curPitchBytes = 0) {
  return depthMotionImage(prev, cur, PPF_DEPTH_F32, 0.001, rows, cols, intr, params, init16, zMin, zMax, prevPitchBytes, curPitchBytes);
}
/* two 16-bit sensor images: z = d * scale metres (0.001 for millimetres) */
inline DepthMotion depthMotionU16(const uint16_t* prev, const uint16_t* cur, int rows, int cols, double scale, const double* intr,
                                  const ppf_depth_motion_params* params = 0, const double* init16 = 0, float zMin = 0.f, float zMax = 0.f,
                                  size_t prevPitchBytes = 0, size_t curPitchBytes = 0) {
  return depthMotionImage(prev, cur, PPF_DEPTH_U16, scale, rows, cols, intr, params, init16, zMin, zMax, prevPitchBytes, curPitchBytes);
}

/* Frame-to-frame camera tracking on float32 depth images: push keeps a copy of the frame, runs depthMotion from the frame kept
 * before it and accumulates pose(), which takes the first frame's camera coordinates to the current frame's (T * pose, summed as
 * ppf_mat44_mul sums it).  When the motion is not found pose() stays where it was, and the new frame becomes the next previous
 * frame only with keepOnFailure. */
class DepthOdometry {
 public:
  DepthOdometry(int rows, int cols, const double* intr, const ppf_depth_motion_params* params = 0, float zMin = 0.f, float zMax = 0.f)
      : rows_(rows), cols_(cols), mp_(params ? *params : defaultDepthMotionParams()), zMin_(zMin), zMax_(zMax), frames_(0) {
    for (int i = 0; i < 4; i++) intr_[i] = intr[i];
    reset();
  }
  void reset() {
    prev_.clear();
    frames_ = 0;
    for (int i = 0; i < 16; i++) pose_[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
  const double* pose() const { return pose_; }
  int frames() const { return frames_; }
  /* the first push only keeps the frame: the identity, status PPF_MOTION_NONE */
  DepthMotion push(const float* depth, bool keepOnFailure = false) {
    const size_t n = (size_t)rows_ * (size_t)cols_;
    DepthMotion m;
    if (prev_.empty()) {
      m = DepthMotion();
      for (int i = 0; i < 16; i++) m.T[i] = (i % 5 == 0) ? 1.0 : 0.0;
      m.status = PPF_MOTION_NONE;
      prev_.assign(depth, depth + n);
      frames_ = 1;
      return m;
    }
    m = depthMotion(&prev_[0], depth, rows_, cols_, intr_, &mp_, 0, zMin_, zMax_);
    if (m.found()) {
      double next[16];
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
          double s = 0;
          for (int k = 0; k < 4; k++) s += m.T[i * 4 + k] * pose_[k * 4 + j];
          next[i * 4 + j] = s;
        }
      for (int i = 0; i < 16; i++) pose_[i] = next[i];
    }
    if (m.found() || keepOnFailure) prev_.assign(depth, depth + n);
    frames_++;
    return m;
  }

 private:
  int rows_, cols_;
  ppf_depth_motion_params mp_;
  float zMin_, zMax_;
  int frames_;
  double intr_[4], pose_[16];
  std::vector<float> prev_;
};

/* what DepthVolume::mesh returns (ppf_depth_volume_mesh): vertices are rows x y z nx ny nz in world coordinates (a
 * normal of 0 0 0 where the volume gives none), triangles three vertex indices each, counter-clockwise seen from free space:
 * what Cloud::fromMesh(&vertices[0], nVertices(), 6, 3, &triangles[0], nTriangles(), ...) takes. */
struct VolumeMesh {
  std::vector<float> vertices;
  std::vector<int32_t> triangles;
  int nVertices() const { return (int)(vertices.size() / 6); }
  int nTriangles() const { return (int)(triangles.size() / 3); }

  /* ppf_volume_mesh_components: the mesh's connected pieces ranked by area, and the mesh of those that are kept */
  static ppf_mesh_component_params defaultComponentParams() {
    ppf_mesh_component_params p;
    ppf_default_mesh_component_params(&p);
    return p;
  }
  /* a mesh from any arrays, checked as ppf_volume_mesh_upload checks them: rows of vstride floats that begin with x y z, the
   * normal at normalOffset (-1: none, the rows get 0 0 0) */
  static VolumeMesh fromArrays(const float* verts, int nVerts, int vstride, int normalOffset, const int32_t* tris, int nTris) {
    ppf_volume_mesh* m = nullptr;
    ppf_match_3d::check(ppf_volume_mesh_upload(verts, nVerts, vstride, normalOffset, tris, nTris, &m));
    return download(m);
  }
  /* info: 0, or it receives the records of the maxInfo largest components, largest first; labels: 0, or it receives every
   * vertex's rank (-1: no triangle names it).  This mesh is not changed */
  VolumeMesh components(const ppf_mesh_component_params* params = 0, std::vector<ppf_mesh_component_info>* info = 0, int maxInfo = 64,
                        std::vector<int32_t>* labels = 0, ppf_mesh_component_stats* stats = 0) const {
    ppf_mesh_component_params cp;
    if (params) cp = *params; else ppf_default_mesh_component_params(&cp);
    ppf_volume_mesh* in = nullptr;
    ppf_match_3d::check(ppf_volume_mesh_upload(vertices.empty() ? 0 : &vertices[0], nVertices(), 6, 3, triangles.empty() ? 0 : &triangles[0],
                                               nTriangles(), &in));
    std::shared_ptr<ppf_volume_mesh> hold(in, [](ppf_volume_mesh* p) { ppf_volume_mesh_release(p); });
    const int cap = info && maxInfo > 0 ? maxInfo : 0;
    std::vector<ppf_mesh_component_info> rec((size_t)cap + 1);
    std::vector<int32_t> lab(labels ? (size_t)nVertices() + 1 : 1);
    ppf_mesh_component_stats st;
    ppf_volume_mesh* out = nullptr;
    ppf_match_3d::check(ppf_volume_mesh_components(in, &cp, &out, labels ? &lab[0] : 0, cap ? &rec[0] : 0, cap, &st));
    const VolumeMesh kept = download(out);
    if (info) {
      rec.resize((size_t)(st.n_components < cap ? st.n_components : cap));
      info->swap(rec);
    }
    if (labels) {
      lab.resize((size_t)nVertices());
      labels->swap(lab);
    }
    if (stats) *stats = st;
    return kept;
  }
  /* the k largest pieces among those of at least minTriangles triangles */
  VolumeMesh largest(int k = 1, int minTriangles = 1, std::vector<ppf_mesh_component_info>* info = 0, ppf_mesh_component_stats* stats = 0) const {
    ppf_mesh_component_params cp = defaultComponentParams();
    cp.rank_hi = k;
    cp.min_triangles = minTriangles;
    return components(&cp, info, 64, 0, stats);
  }

 private:
  /* the arrays of a device mesh, which is released */
  static VolumeMesh download(ppf_volume_mesh* m) {
    std::shared_ptr<ppf_volume_mesh> hold(m, [](ppf_volume_mesh* p) { ppf_volume_mesh_release(p); });
    ppf_volume_mesh_desc d;
    ppf_match_3d::check(ppf_volume_mesh_info(m, &d));
    VolumeMesh out;
    out.vertices.resize((size_t)d.n_vertices * 6);
    out.triangles.resize((size_t)d.n_triangles * 3);
    ppf_match_3d::check(ppf_volume_mesh_read(m, out.vertices.empty() ? 0 : &out.vertices[0], (size_t)d.n_vertices,
                                             out.triangles.empty() ? 0 : &out.triangles[0], (size_t)d.n_triangles));
    return out;
  }
};

/* ppf_depth_volume: a truncated signed distance volume on the device that posed depth images are fused into.
 * A pose is 16 doubles, row-major, world -> camera, as DepthOdometry::pose() is; intr = {fx, fy, ppx, ppy}.  integrate adds a
 * frame seen from a pose; raycast gives the volume's float32 depth image (0 where no surface is hit) from any pose, which
 * filterDepth, Cloud::fromDepth, depthMotion and every frame stage take; extract returns the zero surface as a Cloud with
 * normals, which train takes.  Copies share the volume. */
class DepthVolume {
 public:
  static ppf_depth_volume_params defaultParams() {
    ppf_depth_volume_params p;
    ppf_default_depth_volume_params(&p);
    return p;
  }
  DepthVolume() {}
  explicit DepthVolume(const ppf_depth_volume_params& params) {
    ppf_depth_volume* v = nullptr;
    ppf_match_3d::check(ppf_depth_volume_create(&params, &v));
    h_ = std::shared_ptr<ppf_depth_volume>(v, [](ppf_depth_volume* p) { ppf_depth_volume_release(p); });
  }
  ppf_depth_volume* handle() const { return h_.get(); }
  void reset() { ppf_match_3d::check(ppf_depth_volume_reset(need())); }
  ppf_depth_volume_desc info() const {
    ppf_depth_volume_desc d;
    ppf_match_3d::check(ppf_depth_volume_info(need(), &d));
    return d;
  }
  /* float32 metres in; rowPitchBytes 0: packed rows */
  ppf_depth_volume_integrate_stats integrate(const float* depth, int rows, int cols, const double* intr, const double* pose16, float zMin = 0.f,
                                             float zMax = 0.f, size_t rowPitchBytes = 0) {
    return run(depth, PPF_DEPTH_F32, 0.001, rows, cols, intr, pose16, zMin, zMax, rowPitchBytes);
  }
  /* a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
  ppf_depth_volume_integrate_stats integrateU16(const uint16_t* depth, int rows, int cols, double scale, const double* intr,
                                                const double* pose16, float zMin = 0.f, float zMax = 0.f, size_t rowPitchBytes = 0) {
    return run(depth, PPF_DEPTH_U16, scale, rows, cols, intr, pose16, zMin, zMax, rowPitchBytes);
  }
  /* the packed rows x cols depth image; normals: 0, or it receives the packed rows x cols x 3 normals in camera coordinates */
  std::vector<float> raycast(int rows, int cols, const double* intr, const double* pose16, const ppf_depth_volume_raycast_params* params = 0,
                             std::vector<float>* normals = 0, ppf_depth_volume_raycast_stats* stats = 0) const {
    ppf_depth_volume_raycast_params rp;
    if (params) rp = *params; else ppf_default_depth_volume_raycast_params(&rp);
    const size_t n = (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0);
    std::vector<float> out(n + 1), nr(normals ? n * 3 + 1 : 1);
    ppf_match_3d::check(ppf_depth_volume_raycast(need(), rows, cols, intr, pose16, &rp, &out[0], normals ? &nr[0] : 0, stats));
    out.resize(n);
    if (normals) {
      nr.resize(n * 3);
      normals->swap(nr);
    }
    return out;
  }
  Cloud extract(const ppf_depth_volume_extract_params* params = 0, ppf_depth_volume_extract_stats* stats = 0) const {
    ppf_depth_volume_extract_params ep;
    if (params) ep = *params; else ppf_default_depth_volume_extract_params(&ep);
    ppf_cloud* c = nullptr;
    ppf_match_3d::check(ppf_depth_volume_extract(need(), &ep, &c, stats));
    return Cloud(c);
  }
  /* every voxel, x fastest: nx * ny * nz records */
  std::vector<ppf_depth_volume_voxel> read() const {
    const ppf_depth_volume_desc d = info();
    std::vector<ppf_depth_volume_voxel> out((size_t)d.dims[0] * (size_t)d.dims[1] * (size_t)d.dims[2]);
    ppf_match_3d::check(ppf_depth_volume_read(need(), &out[0], out.size()));
    return out;
  }
  /* the inverse of read: nx * ny * nz records replace every voxel (w in 0 .. max_weight, d finite in [-1, 1]) */
  void write(const std::vector<ppf_depth_volume_voxel>& records) {
    ppf_match_3d::check(ppf_depth_volume_write(need(), records.empty() ? 0 : &records[0], records.size()));
  }
  /* the zero surface as a triangle mesh by marching tetrahedra, downloaded */
  VolumeMesh mesh(int minWeight = 1, ppf_depth_volume_mesh_stats* stats = 0) const {
    ppf_depth_volume_mesh_params mp;
    ppf_default_depth_volume_mesh_params(&mp);
    mp.min_weight = minWeight;
    ppf_volume_mesh* m = nullptr;
    ppf_match_3d::check(ppf_depth_volume_mesh(need(), &mp, &m, stats));
    std::shared_ptr<ppf_volume_mesh> hold(m, [](ppf_volume_mesh* p) { ppf_volume_mesh_release(p); });
    ppf_volume_mesh_desc d;
    ppf_match_3d::check(ppf_volume_mesh_info(m, &d));
    VolumeMesh out;
    out.vertices.resize((size_t)d.n_vertices * 6);
    out.triangles.resize((size_t)d.n_triangles * 3);
    ppf_match_3d::check(ppf_volume_mesh_read(m, out.vertices.empty() ? 0 : &out.vertices[0], (size_t)d.n_vertices,
                                             out.triangles.empty() ? 0 : &out.triangles[0], (size_t)d.n_triangles));
    return out;
  }

 private:
  ppf_depth_volume* need() const {
    if (!h_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::DepthVolume: empty handle");
    return h_.get();
  }
  ppf_depth_volume_integrate_stats run(const void* depth, int format, double scale, int rows, int cols, const double* intr, const double* pose16,
                                       float zMin, float zMax, size_t rowPitchBytes) {
    const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
    ppf_depth_volume_integrate_stats st;
    ppf_match_3d::check(ppf_depth_volume_integrate(need(), depth, rows, cols, rowPitchBytes, intr, &dp, pose16, &st));
    return st;
  }
  std::shared_ptr<ppf_depth_volume> h_;
};

/* Frame-to-model camera tracking and fusion on float32 depth images: the first push integrates the frame at the identity; every
 * later push raycasts the volume from pose(), runs depthMotion(prev = that image, cur = the frame), sets pose() to T * pose()
 * (summed as ppf_mat44_mul sums it) and integrates the frame there.  When the motion is not found, pose() and the volume stay as
 * they were.  modelDepth() is the last raycast image.  The volume's world is the first frame's camera. */
class DepthFusion {
 public:
  DepthFusion(int rows, int cols, const double* intr, const DepthVolume& volume, const ppf_depth_motion_params* motion = 0,
              const ppf_depth_volume_raycast_params* raycast = 0, float zMin = 0.f, float zMax = 0.f)
      : rows_(rows), cols_(cols), vol_(volume), mp_(motion ? *motion : defaultDepthMotionParams()), zMin_(zMin), zMax_(zMax), frames_(0) {
    for (int i = 0; i < 4; i++) intr_[i] = intr[i];
    if (raycast) rp_ = *raycast; else ppf_default_depth_volume_raycast_params(&rp_);
    for (int i = 0; i < 16; i++) pose_[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
  const double* pose() const { return pose_; }
  int frames() const { return frames_; }
  const std::vector<float>& modelDepth() const { return model_; }
  DepthVolume& volume() { return vol_; }
  /* updated: 0, or it receives the integration's counters (zero when nothing was integrated) */
  DepthMotion push(const float* depth, ppf_depth_volume_integrate_stats* updated = 0) {
    DepthMotion m = DepthMotion();
    ppf_depth_volume_integrate_stats st = ppf_depth_volume_integrate_stats();
    if (frames_ == 0) {
      for (int i = 0; i < 16; i++) m.T[i] = (i % 5 == 0) ? 1.0 : 0.0;
      m.status = PPF_MOTION_NONE;
      st = vol_.integrate(depth, rows_, cols_, intr_, pose_, zMin_, zMax_);
    } else {
      model_ = vol_.raycast(rows_, cols_, intr_, pose_, &rp_);
      m = depthMotion(&model_[0], depth, rows_, cols_, intr_, &mp_, 0, zMin_, zMax_);
      if (m.found()) {
        double next[16];
        for (int i = 0; i < 4; i++)
          for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += m.T[i * 4 + k] * pose_[k * 4 + j];
            next[i * 4 + j] = s;
          }
        for (int i = 0; i < 16; i++) pose_[i] = next[i];
        st = vol_.integrate(depth, rows_, cols_, intr_, pose_, zMin_, zMax_);
      }
    }
    frames_++;
    if (updated) *updated = st;
    return m;
  }

 private:
  int rows_, cols_;
  DepthVolume vol_;
  ppf_depth_motion_params mp_;
  ppf_depth_volume_raycast_params rp_;
  float zMin_, zMax_;
  int frames_;
  double intr_[4], pose_[16];
  std::vector<float> model_;
};

/* ppf_depth_segments: the depth image's connected surfaces labelled in image space.  Returns the label image
 * (packed rows x cols: a pixel's segment rank, largest segment 0, or -1) and fills `info` with one record per segment, whose
 * box_xywh is what Cloud::prepareFrame takes as a box.  normals: 0 (depth alone decides), or the cloud Cloud::fromDepth gives
 * for this image with ppf_depth_normal_params (no PPF_DEPTH_NORMALS_DROP) and the same zMin / zMax. */
inline ppf_segment_params defaultSegmentParams() {
  ppf_segment_params p;
  ppf_default_segment_params(&p);
  return p;
}
inline std::vector<int32_t> segmentDepthImage(const void* depth, int format, double scale, int rows, int cols, const Cloud* normals,
                                              const ppf_segment_params* params, std::vector<ppf_segment_info>& info, float zMin, float zMax,
                                              size_t rowPitchBytes, int32_t* counts, ppf_segment_stats* stats) {
  const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
  const ppf_segment_params sp = params ? *params : defaultSegmentParams();
  const int slots = sp.max_segments >= 1 && sp.max_segments <= PPF_CLUSTER_MAX_CLUSTERS ? sp.max_segments : 1;
  std::vector<int32_t> labels((rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0) + 1);
  int32_t local[3] = {0, 0, 0};
  info.assign((size_t)slots, ppf_segment_info());
  ppf_match_3d::check(ppf_depth_segments(depth, rows, cols, rowPitchBytes, &dp, normals ? normals->handle() : 0, &sp, &labels[0], &info[0],
                                         counts ? counts : local, stats));
  info.resize((size_t)(counts ? counts : local)[0]);
  labels.resize(labels.size() - 1);
  return labels;
}
/* float32 metres in; rowPitchBytes 0: packed rows; params 0: the defaults; counts: 0 or {segments, valid, all components} */
inline std::vector<int32_t> segmentDepth(const float* depth, int rows, int cols, std::vector<ppf_segment_info>& info, const Cloud* normals = 0,
                                         const ppf_segment_params* params = 0, float zMin = 0.f, float zMax = 0.f, size_t rowPitchBytes = 0,
                                         int32_t* counts = 0, ppf_segment_stats* stats = 0) {
  return segmentDepthImage(depth, PPF_DEPTH_F32, 0.001, rows, cols, normals, params, info, zMin, zMax, rowPitchBytes, counts, stats);
}
/* a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
inline std::vector<int32_t> segmentDepthU16(const uint16_t* depth, int rows, int cols, double scale, std::vector<ppf_segment_info>& info,
                                            const Cloud* normals = 0, const ppf_segment_params* params = 0, float zMin = 0.f, float zMax = 0.f,
                                            size_t rowPitchBytes = 0, int32_t* counts = 0, ppf_segment_stats* stats = 0) {
  return segmentDepthImage(depth, PPF_DEPTH_U16, scale, rows, cols, normals, params, info, zMin, zMax, rowPitchBytes, counts, stats);
}

/* ppf_depth_edges: where the depth image says a surface ends.  Returns the mask (packed rows x cols: the OR of
 * PPF_EDGE_OCCLUDING, _OCCLUDED, _BOUNDARY and, with normals, _CURVATURE; 0 at pixels that are not kept) and, when edgeCloud is
 * given, fills it with the pixels whose mask meets params->select in row-major order: what matchS2B and the frame stages take
 * as the edge cloud.  normals: 0, or the cloud Cloud::fromDepth gives for this image with ppf_depth_normal_params (no
 * PPF_DEPTH_NORMALS_DROP) and the same zMin / zMax; the edge cloud's rows are then that cloud's rows and intr is not read.
 * Without normals the rows are x y z 0 0 0 and intr = {fx, fy, ppx, ppy} is needed for a cloud. */
inline ppf_depth_edge_params defaultDepthEdgeParams() {
  ppf_depth_edge_params p;
  ppf_default_depth_edge_params(&p);
  return p;
}
inline std::vector<uint8_t> depthEdgesImage(const void* depth, int format, double scale, int rows, int cols, const double* intr,
                                            const Cloud* normals, const ppf_depth_edge_params* params, Cloud* edgeCloud, float zMin,
                                            float zMax, bool fp64, size_t rowPitchBytes, ppf_depth_edge_stats* stats) {
  const ppf_depth_params dp = depthParams(format, scale, zMin, zMax, fp64 ? PPF_DEPTH_FP64 : 0);
  const ppf_depth_edge_params ep = params ? *params : defaultDepthEdgeParams();
  std::vector<uint8_t> mask((rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0) + 1);
  ppf_cloud* c = nullptr;
  ppf_match_3d::check(ppf_depth_edges(depth, rows, cols, rowPitchBytes, intr, &dp, normals ? normals->handle() : 0, &ep, &mask[0],
                                      edgeCloud ? &c : 0, stats));
  if (edgeCloud) *edgeCloud = Cloud(c);
  mask.resize(mask.size() - 1);
  return mask;
}
/* float32 metres in; rowPitchBytes 0: packed rows; params 0: the defaults; edgeCloud 0: the mask alone */
inline std::vector<uint8_t> depthEdges(const float* depth, int rows, int cols, const double* intr = 0, const Cloud* normals = 0,
                                       const ppf_depth_edge_params* params = 0, Cloud* edgeCloud = 0, float zMin = 0.f, float zMax = 0.f,
                                       bool fp64 = false, size_t rowPitchBytes = 0, ppf_depth_edge_stats* stats = 0) {
  return depthEdgesImage(depth, PPF_DEPTH_F32, 0.001, rows, cols, intr, normals, params, edgeCloud, zMin, zMax, fp64, rowPitchBytes, stats);
}
/* a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
inline std::vector<uint8_t> depthEdgesU16(const uint16_t* depth, int rows, int cols, double scale, const double* intr = 0,
                                          const Cloud* normals = 0, const ppf_depth_edge_params* params = 0, Cloud* edgeCloud = 0,
                                          float zMin = 0.f, float zMax = 0.f, bool fp64 = false, size_t rowPitchBytes = 0,
                                          ppf_depth_edge_stats* stats = 0) {
  return depthEdgesImage(depth, PPF_DEPTH_U16, scale, rows, cols, intr, normals, params, edgeCloud, zMin, zMax, fp64, rowPitchBytes, stats);
}

/* ppf_recognizer / ppf_recognize_frame: which trained models a proposal cloud can be a view of, from the models'
 * quantised pair-feature keys.  Built once from trained detectors (ppf_match_3d::PPF3DDetector::handle(), PPF_FEATURE_PPF models
 * only), which it keeps alive; copies share the recogniser.  recognize() returns per cloud its candidates, best first, at most
 * params.top of them; a null pointer in `clouds` or an empty Cloud has none. */
class Recognizer {
 public:
  Recognizer() : n_models_(0) {}
  explicit Recognizer(const std::vector<const ppf_model*>& models) : n_models_((int)models.size()) {
    ppf_recognizer* r = nullptr;
    ppf_match_3d::check(ppf_recognizer_create(models.empty() ? 0 : &models[0], (int)models.size(), &r));
    h_ = std::shared_ptr<ppf_recognizer>(r, [](ppf_recognizer* p) { ppf_recognizer_release(p); });
  }
  static ppf_recognize_params defaultParams() {
    ppf_recognize_params p;
    ppf_default_recognize_params(&p);
    return p;
  }
  int models() const { return n_models_; }
  const ppf_recognizer* handle() const { return h_.get(); }
  ppf_recognizer_info modelInfo(int i) const {
    ppf_recognizer_info info;
    ppf_match_3d::check(ppf_recognizer_model_info(need(), i, &info));
    return info;
  }
  /* model i's key set: 4 int32 a key, in lexicographic order */
  std::vector<int32_t> keys(int i) const {
    int n = 0;
    (void)ppf_recognizer_keys(need(), i, 0, 0, &n); /* PPF_ERR_CAPACITY: n is the size */
    std::vector<int32_t> out((size_t)n * 4 + 4);
    ppf_match_3d::check(ppf_recognizer_keys(need(), i, &out[0], n + 1, &n));
    out.resize((size_t)n * 4);
    return out;
  }
  /* nUsed: 0 or the used rows per cloud; counts: 0 or per cloud and model {n_known, n_keys_hit} */
  std::vector<std::vector<ppf_recognize_score> > recognize(const std::vector<const Cloud*>& clouds, const ppf_recognize_params* params = 0,
                                                           std::vector<int32_t>* nUsed = 0, std::vector<uint64_t>* counts = 0,
                                                           ppf_recognize_stats* stats = 0) const {
    const ppf_recognize_params p = params ? *params : defaultParams();
    const size_t n = clouds.size(), top = p.top >= 1 && p.top <= PPF_RECOGNIZE_MAX_TOP ? (size_t)p.top : 1;
    std::vector<const ppf_cloud*> handles(n + 1, (const ppf_cloud*)0);
    for (size_t i = 0; i < n; i++) handles[i] = clouds[i] ? clouds[i]->handle() : 0;
    std::vector<ppf_recognize_score> ranked(n * top + 1);
    std::vector<int32_t> nRanked(n + 1, 0), used(n + 1, 0);
    std::vector<uint64_t> cnt(n * (size_t)n_models_ * 2 + 1, 0);
    ppf_match_3d::check(ppf_recognize_frame(need(), &handles[0], (int)n, &p, &used[0], &cnt[0], &ranked[0], &nRanked[0], stats));
    std::vector<std::vector<ppf_recognize_score> > out(n);
    for (size_t i = 0; i < n; i++) out[i].assign(ranked.begin() + i * top, ranked.begin() + i * top + nRanked[i]);
    if (nUsed) nUsed->assign(used.begin(), used.begin() + n);
    if (counts) counts->assign(cnt.begin(), cnt.begin() + n * (size_t)n_models_ * 2);
    return out;
  }

 private:
  const ppf_recognizer* need() const {
    if (!h_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::Recognizer: empty handle");
    return h_.get();
  }
  std::shared_ptr<ppf_recognizer> h_;
  int n_models_;
};

/* A resident registration map (ppf_depth_map), built once per calibration as k4a::transformation is: registerDepth draws a
 * raw depth frame of the depth camera into the pixel grid of the colour camera (float32 metres, 0 where nothing was drawn),
 * which is what Cloud::fromDepth and every frame stage take with fx(), fy(), ppx(), ppy().  R9 (row-major) and t3 (metres)
 * take a point of the depth camera's frame into the colour camera's.  Copies share the map. */
class DepthMap {
 public:
  DepthMap() : cam_(), rows_(0), cols_(0) {}
  DepthMap(const ppf_camera& depthCam, int depthRows, int depthCols, const ppf_camera& colorCam, int colorRows, int colorCols,
           const double R9[9], const double t3[3])
      : cam_(colorCam), rows_(colorRows), cols_(colorCols) {
    ppf_depth_map* m = nullptr;
    ppf_match_3d::check(ppf_depth_map_create(&depthCam, depthRows, depthCols, &colorCam, colorRows, colorCols, R9, t3, &m));
    h_ = std::shared_ptr<ppf_depth_map>(m, [](ppf_depth_map* p) { ppf_depth_map_release(p); });
  }
  static ppf_camera pinhole(double fx, double fy, double cx, double cy) {
    ppf_camera c;
    ppf_default_camera(&c, fx, fy, cx, cy);
    return c;
  }
  int rows() const { return rows_; } /* of the aligned image */
  int cols() const { return cols_; }
  double fx() const { return cam_.fx; }
  double fy() const { return cam_.fy; }
  double ppx() const { return cam_.cx; }
  double ppy() const { return cam_.cy; }
  const ppf_depth_map* handle() const { return h_.get(); }

  /* float32 metres in, the aligned rows() x cols() image out; rowPitchBytes 0: packed rows */
  std::vector<float> registerDepth(const float* depth, float zMin = 0.f, float zMax = 0.f, size_t rowPitchBytes = 0,
                                   const ppf_register_params* params = 0, ppf_register_stats* stats = 0) const {
    return run(depth, PPF_DEPTH_F32, 0.001, zMin, zMax, rowPitchBytes, params, stats);
  }
  /* a 16-bit sensor image: z = d * scale metres (0.001 for millimetres) */
  std::vector<float> registerDepthU16(const uint16_t* depth, double scale, float zMin = 0.f, float zMax = 0.f, size_t rowPitchBytes = 0,
                                      const ppf_register_params* params = 0, ppf_register_stats* stats = 0) const {
    return run(depth, PPF_DEPTH_U16, scale, zMin, zMax, rowPitchBytes, params, stats);
  }
  /* registerDepth, then filterDepth on the aligned image */
  std::vector<float> registerFiltered(const float* depth, const ppf_depth_filter_params* filter = 0, float zMin = 0.f, float zMax = 0.f) const {
    return filterDepth(&registerDepth(depth, zMin, zMax)[0], rows_, cols_, filter, zMin, zMax);
  }
  /* a detector's boxes {x, y, w, h} on the raw colour image (camera `raw`, with its distortion) in this map's colour camera */
  std::vector<int> mapBoxes(const ppf_camera& raw, const int* boxesXYWH, int n) const {
    std::vector<int> out((size_t)(n > 0 ? n : 0) * 4 + 1, 0);
    ppf_match_3d::check(ppf_camera_map_boxes(&raw, &cam_, rows_, cols_, boxesXYWH, n, &out[0]));
    out.resize((size_t)(n > 0 ? n : 0) * 4);
    return out;
  }

 private:
  std::vector<float> run(const void* depth, int format, double scale, float zMin, float zMax, size_t rowPitchBytes,
                         const ppf_register_params* params, ppf_register_stats* stats) const {
    if (!h_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "prep::DepthMap: empty handle");
    const ppf_depth_params dp = depthParams(format, scale, zMin, zMax);
    ppf_register_params rp;
    if (params) rp = *params; else ppf_default_register_params(&rp);
    std::vector<float> out((size_t)rows_ * (size_t)cols_ + 1);
    ppf_match_3d::check(ppf_depth_register(h_.get(), depth, rowPitchBytes, &dp, &rp, &out[0], stats));
    out.resize((size_t)rows_ * (size_t)cols_);
    return out;
  }
  std::shared_ptr<ppf_depth_map> h_;
  ppf_camera cam_;
  int rows_, cols_;
};

}  // namespace prep
}  // namespace ppfhip

#endif /* PPF_CLOUD_STAGES_HPP */
