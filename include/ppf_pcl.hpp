/*
 * ppf_pcl.hpp — header-only facade with the shape of PCL's PPF pipeline
 * (pcl::PPFEstimation / pcl::PPFHashMapSearch / pcl::PPFRegistration), which BASELINE.json's north_star names,
 * over the same C-ABI (ppf_hip.h).  The reference itself never calls these classes (it uses PCL only
 * for I/O, cropping, voxel grid, outlier removal and normals; its PPF calls go to OpenCV's PPF3DDetector, see
 * ppf_match_3d.hpp), so this header exists for code written against the PCL names:
 *
 *     PPFEstimation<PointNormal, PointNormal, PPFSignature> est;
 *     est.setInputCloud(model); est.setInputNormals(model); est.compute(*model_ppf);
 *     PPFHashMapSearch::Ptr search(new PPFHashMapSearch(12.0f / 180.0f * M_PI, 0.05f));
 *     search->setInputFeatureCloud(model_ppf);
 *     PPFRegistration<PointNormal, PointNormal> reg;
 *     reg.setSceneReferencePointSamplingRate(10);
 *     reg.setPositionClusteringThreshold(0.2f); reg.setRotationClusteringThreshold(30.0f / 180.0f * M_PI);
 *     reg.setSearchMethod(search); reg.setInputSource(model); reg.setInputTarget(scene);
 *     reg.align(output);  reg.getFinalTransformation();
 *
 * SEMANTICS (stated, not hidden): these classes switch the engine's PCL policy flags on -- the pair feature is
 * pcl::computePairFeatures' (ppf_train_params.feature = PPF_FEATURE_DARBOUX, keys floor(f / step)), the model table is
 * keyed on the exact quantised feature (key_equality = PPF_KEY_EXACT, PPFHashMapSearch's hash map with key equality),
 * a reference point is paired with the scene points within model_diameter / 2
 * (ppf_match_params.pair_radius, PPFRegistration's kd-tree radius search), alpha differences are wrapped into
 * [-pi, pi] and binned over 2*pi (alpha_range_2pi), and poses cluster on the angle of their relative rotation
 * (rot_metric_relative).  What remains different from PCL proper: fp64 arithmetic where PCL computes in float (pairs within
 * rounding of a bin edge can land in the neighbouring bin), and the engine's reference frame / alpha convention (the
 * reference's library's, applied to model and scene alike, so alpha differences agree).  Point types only need members
 * x, y, z, normal_x, normal_y, normal_z (pcl::PointNormal qualifies); clouds only need `.points` or to be a
 * std::vector of such points, and are handed to the engine WHERE THEY ARE (stride 12 floats, normals at float 4 for
 * pcl::PointNormal): no host-side repack.  Normals are used as given, as PCL does (the reference's Mat adaptor
 * re-normalises them; ppf_prep_to_mat is that step on the device).  Compiles without PCL and without Eigen.
 */
#ifndef PPF_PCL_HPP
#define PPF_PCL_HPP

#include <array>
#include <cmath>
#include <cstddef>
#include <functional>
#include <memory>
#include <utility>
#include <type_traits>
#include <vector>

#include "ppf_detmath.h" /* ppf_cos: RegionGrowing's smoothness threshold as a cosine, the same bits on every machine */
#include "ppf_match_3d.hpp"

namespace ppfhip {
namespace pcl_shaped {

/* pcl::PointNormal's storage for builds without PCL: 48 bytes, x y z 1 | normal_x normal_y normal_z 0 | curvature pad pad pad
 * (PCL aligns the struct to 16 bytes; the float positions are what matters here) */
struct PointNormal {
  float x, y, z, pad0;
  float normal_x, normal_y, normal_z, pad1;
  float curvature, pad2[3];
  PointNormal() : x(0), y(0), z(0), pad0(1.f), normal_x(0), normal_y(0), normal_z(0), pad1(0), curvature(0), pad2{0, 0, 0} {}
  PointNormal(float x_, float y_, float z_, float nx, float ny, float nz)
      : x(x_), y(y_), z(z_), pad0(1.f), normal_x(nx), normal_y(ny), normal_z(nz), pad1(0), curvature(0), pad2{0, 0, 0} {}
};

struct PPFSignature {
  float f1, f2, f3, f4, alpha_m;
};

template <class PointT>
struct PointCloud {
  std::vector<PointT> points;
  std::size_t size() const { return points.size(); }
  typedef std::shared_ptr<PointCloud<PointT>> Ptr;
  typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
};

namespace detail {
template <class C> auto pts(const C& c) -> decltype(c.points) const& { return c.points; }
template <class P> const std::vector<P>& pts(const std::vector<P>& v) { return v; }
template <class C> auto pts_mut(C& c) -> decltype(c.points)& { return c.points; }
template <class P> std::vector<P>& pts_mut(std::vector<P>& v) { return v; }

/* A cloud of PointNormal-like points as the C-ABI's (pointer, rows, stride, normal_offset): the caller's storage itself
 * when the point type keeps x y z and normal_x normal_y normal_z as two runs of three consecutive floats (pcl::PointNormal
 * does: stride 12, normal offset 4), so nothing is repacked on the host -- unlike the reference's
 * PointCloudXYZNormalToMat (CloudProcessing.h:163-190), which copies every point into an N x 6 Mat first.  Any other
 * point type is copied into N x 6 rows.  A view holds the caller's smart pointer, not an address: `refresh()` takes pointer
 * and row count from the cloud AS IT IS THEN, so points that were resized or reallocated between setInputCloud() and
 * compute() / align() -- legal in PCL, which reads through the cloud pointer at compute time -- are read where they are now. */
struct RowsView {
  const float* p = nullptr;
  int n = 0, stride = 6, noff = PPF_NOFF_MAT;
  std::shared_ptr<void> keep;             /* the caller's cloud pointer, or the copied rows */
  std::function<void(RowsView&)> resolve; /* fills p / n / stride / noff from the cloud */
  void refresh() { if (resolve) resolve(*this); }
};

template <class CloudPtr>
RowsView view_of(const CloudPtr& cloud) {
  RowsView v;
  v.resolve = [cloud](RowsView& r) {
    const auto& p = pts(*cloud);
    typedef typename std::decay<decltype(p[0])>::type PointT;
    r.n = (int)p.size();
    r.p = nullptr;
    if (p.empty()) return;
    /* member offsets in bytes from the point's first byte (no pointer arithmetic across members) */
    const char* b0 = reinterpret_cast<const char*>(&p[0]);
    const std::ptrdiff_t ox = reinterpret_cast<const char*>(&p[0].x) - b0, oy = reinterpret_cast<const char*>(&p[0].y) - b0,
                         oz = reinterpret_cast<const char*>(&p[0].z) - b0, nx = reinterpret_cast<const char*>(&p[0].normal_x) - b0,
                         ny = reinterpret_cast<const char*>(&p[0].normal_y) - b0, nz = reinterpret_cast<const char*>(&p[0].normal_z) - b0;
    const std::ptrdiff_t F = (std::ptrdiff_t)sizeof(float);
    if (sizeof(PointT) % sizeof(float) == 0 && oy == ox + F && oz == ox + 2 * F && nx >= ox + 3 * F && (nx - ox) % F == 0 && ny == nx + F &&
        nz == nx + 2 * F && (std::size_t)(nz + F) <= sizeof(PointT)) {
      r.p = reinterpret_cast<const float*>(b0 + ox);
      r.stride = (int)(sizeof(PointT) / sizeof(float));
      r.noff = (int)((nx - ox) / F);
      r.keep = std::make_shared<CloudPtr>(cloud); /* a copy of the caller's smart pointer: the points stay where they are */
      return;
    }
    auto rows = std::make_shared<std::vector<float>>(p.size() * 6);
    for (std::size_t i = 0; i < p.size(); i++) {
      float* d = &(*rows)[i * 6];
      d[0] = p[i].x; d[1] = p[i].y; d[2] = p[i].z;
      d[3] = p[i].normal_x; d[4] = p[i].normal_y; d[5] = p[i].normal_z;
    }
    r.p = rows->data();
    r.stride = 6;
    r.noff = PPF_NOFF_MAT;
    r.keep = rows;
  };
  v.refresh();
  return v;
}
}  // namespace detail

/* The feature cloud of the PCL pipeline: PPFEstimation::compute fills `points` with the N x N PPFSignature rows PCL
 * materialises (row i*N + j = pair (i, j): pcl::computePairFeatures' f1..f4 and alpha_m; rows i == j are NaN), computed on
 * the device (ppf_pair_features).  PPFHashMapSearch trains from the model rows, which travel along as a view. */
struct PPFFeatureCloud {
  std::vector<PPFSignature> points;
  detail::RowsView model;
  std::size_t size() const { return points.size(); }
  typedef std::shared_ptr<PPFFeatureCloud> Ptr;
};

template <class PointInT, class PointNT, class PointOutT = PPFSignature>
class PPFEstimation {
 public:
  template <class CloudPtr> void setInputCloud(const CloudPtr& cloud) { model_ = detail::view_of(cloud); }
  template <class CloudPtr> void setInputNormals(const CloudPtr&) {} /* normals travel with the points */
  void compute(PPFFeatureCloud& out) {
    model_.refresh(); /* the cloud as it is now */
    out.model = model_;
    const std::size_t n = (std::size_t)model_.n;
    out.points.assign(n * n, PPFSignature());
    if (n) {
      static_assert(sizeof(PPFSignature) == 5 * sizeof(float), "PPFSignature must be five packed floats");
      ppf_match_3d::check(ppf_pair_features(model_.p, model_.n, model_.stride, model_.noff, PPF_FEATURE_DARBOUX,
                                            reinterpret_cast<float*>(out.points.data()), n * n));
    }
  }

 private:
  detail::RowsView model_;
};

class PPFHashMapSearch {
 public:
  typedef std::shared_ptr<PPFHashMapSearch> Ptr;
  PPFHashMapSearch(float angle_discretization_step = 12.0f / 180.0f * 3.14159265358979f,
                   float distance_discretization_step = 0.01f)
      : angle_step_(angle_discretization_step), dist_step_(distance_discretization_step) {}

  /* trains the device table: the model rows are used as they are (PCL does not resample the model), the distance
   * step is PCL's absolute step expressed relative to the model's bbox diagonal */
  void setInputFeatureCloud(const PPFFeatureCloud::Ptr& features) {
    features->model.refresh();
    const detail::RowsView& mv = features->model;
    if (!mv.p || mv.n < 2) throw ppf_match_3d::Error(PPF_ERR_INVALID, "PPFHashMapSearch: empty feature cloud");
    const float* r = mv.p;
    const int n = mv.n;
    const std::size_t st = (std::size_t)mv.stride;
    float lo[3] = {r[0], r[1], r[2]}, hi[3] = {r[0], r[1], r[2]};
    for (int i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], r[(size_t)i * st + k]); hi[k] = std::max(hi[k], r[(size_t)i * st + k]); }
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    diameter_ = std::sqrt(dx * dx + dy * dy + dz * dz);
    ppf_train_params tp;
    ppf_default_train_params(&tp);
    tp.presampled = 1;
    tp.feature = PPF_FEATURE_DARBOUX; /* PPFEstimation's four values */
    tp.key_equality = PPF_KEY_EXACT; /* nearestNeighborSearch() returns the model pairs with the SAME quantised feature */
    tp.distance_from_distance_step = 1;
    tp.relative_distance_step = dist_step_ / diameter_;
    tp.relative_sampling_step = tp.relative_distance_step; /* only feeds the default clustering threshold */
    tp.num_angles = 2.0 * 3.14159265358979311600 / angle_step_;
    ppf_model* m = nullptr;
    ppf_match_3d::check(ppf_model_train(r, n, mv.stride, mv.noff, &tp, &m)); /* pcl::PointNormal storage as it is: stride 12, normals at 4 */
    model_.reset(m, [](ppf_model* p) { ppf_model_release(p); });
  }
  /* the model pairs (i, j) filed under the quantised (f1, f2, f3, f4): PCL's hash-map lookup with key equality */
  void nearestNeighborSearch(float& f1, float& f2, float& f3, float& f4, std::vector<std::pair<std::size_t, std::size_t>>& indices) {
    if (!model_) throw ppf_match_3d::Error(PPF_ERR_NOT_TRAINED, "PPFHashMapSearch: no feature cloud set");
    const float f[4] = {f1, f2, f3, f4};
    int n = 0;
    ppf_match_3d::check(ppf_model_nearest_pairs(model_.get(), f, nullptr, 0, &n));
    std::vector<uint32_t> ij((std::size_t)std::max(n, 1) * 2);
    ppf_match_3d::check(ppf_model_nearest_pairs(model_.get(), f, ij.data(), std::max(n, 1), &n));
    indices.clear();
    indices.reserve((std::size_t)n);
    for (int q = 0; q < n; q++) indices.push_back(std::make_pair((std::size_t)ij[2 * q], (std::size_t)ij[2 * q + 1]));
  }
  float getAngleDiscretizationStep() const { return angle_step_; }
  float getDistanceDiscretizationStep() const { return dist_step_; }
  float getModelDiameter() const { return diameter_; }
  const ppf_model* handle() const { return model_.get(); }

 private:
  float angle_step_, dist_step_, diameter_ = 0.f;
  std::shared_ptr<ppf_model> model_;
};

template <class PointSource, class PointTarget>
class PPFRegistration {
 public:
  typedef std::array<float, 16> Matrix4f; /* row-major 4x4, model -> scene */
  struct PoseWithVotes {
    Matrix4f pose;
    unsigned votes;
  };

  void setSearchMethod(const PPFHashMapSearch::Ptr& search) { search_ = search; }
  void setSceneReferencePointSamplingRate(unsigned rate) { rate_ = rate ? rate : 1; }
  void setPositionClusteringThreshold(float t) { pos_thr_ = t; }
  void setRotationClusteringThreshold(float t) { rot_thr_ = t; }
  template <class CloudPtr> void setInputSource(const CloudPtr& model) { source_ = detail::view_of(model); } /* voted from the search method's table; align() moves THIS cloud */
  template <class CloudPtr> void setInputTarget(const CloudPtr& scene) { scene_ = detail::view_of(scene); }

  /* computeTransformation(): votes, clusters; keeps every clustered pose, best first */
  template <class CloudT> void align(CloudT& output) {
    if (!search_ || !search_->handle()) throw ppf_match_3d::Error(PPF_ERR_NOT_TRAINED, "PPFRegistration: no trained search method");
    ppf_match_params mp;
    ppf_default_match_params(&mp);
    mp.presampled = 1; /* PCL votes on the target cloud as given */
    mp.relative_scene_sample_step = 1.0 / (double)rate_;
    mp.position_threshold = pos_thr_;
    mp.rotation_threshold = rot_thr_;
    mp.pair_radius = 0.5 * (double)search_->getModelDiameter(); /* the radius search of computeTransformation() */
    mp.rot_metric_relative = 1;                                 /* posesWithinErrorBounds(): angle of the relative rotation */
    mp.alpha_range_2pi = 1;                                     /* alpha wrapped into [-pi, pi], bins of the angle discretisation step */
    scene_.refresh(); /* the target as it is now */
    const int n = scene_.n;
    if (!scene_.p || n <= 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, "PPFRegistration: no target cloud");
    std::vector<ppf_pose> out((size_t)n / rate_ + 8);
    int n_out = 0;
    ppf_match_3d::check(ppf_match(search_->handle(), scene_.p, n, scene_.stride, scene_.noff, nullptr, 0, 6, PPF_NOFF_MAT, &mp, out.data(),
                                  (int)out.size(), &n_out));
    results_.clear();
    for (int i = 0; i < n_out; i++) {
      PoseWithVotes p;
      for (int k = 0; k < 16; k++) p.pose[(size_t)k] = (float)out[(size_t)i].pose[k];
      p.votes = out[(size_t)i].num_votes;
      results_.push_back(p);
    }
    converged_ = n_out > 0;
    /* PCL: `output` = the input source transformed by the final transformation (the source itself when nothing was found) */
    source_.refresh();
    auto& op = detail::pts_mut(output);
    op.resize((std::size_t)std::max(source_.n, 0));
    if (source_.p && source_.n > 0) {
      const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      std::vector<float> rows((std::size_t)source_.n * 6);
      ppf_match_3d::check(ppf_transform_pc_pose(source_.p, source_.n, source_.stride, source_.noff, n_out > 0 ? out[0].pose : ident, rows.data()));
      for (int i = 0; i < source_.n; i++) {
        const float* r = &rows[(std::size_t)i * 6];
        op[(std::size_t)i].x = r[0]; op[(std::size_t)i].y = r[1]; op[(std::size_t)i].z = r[2];
        op[(std::size_t)i].normal_x = r[3]; op[(std::size_t)i].normal_y = r[4]; op[(std::size_t)i].normal_z = r[5];
      }
    }
  }
  bool hasConverged() const { return converged_; }
  Matrix4f getFinalTransformation() const {
    if (results_.empty()) return Matrix4f{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    return results_[0].pose;
  }
  const std::vector<PoseWithVotes>& getBestPoseCandidates() const { return results_; }

 private:
  PPFHashMapSearch::Ptr search_;
  unsigned rate_ = 5;
  float pos_thr_ = -1.f, rot_thr_ = -1.f;
  detail::RowsView scene_, source_;
  std::vector<PoseWithVotes> results_;
  bool converged_ = false;
};

/* pcl::PointXYZ's storage for builds without PCL (16 bytes: x y z 1) */
struct PointXYZ {
  float x, y, z, pad0;
  PointXYZ() : x(0), y(0), z(0), pad0(1.f) {}
  PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_), pad0(1.f) {}
};

struct PointIndices {
  std::vector<int> indices;
};

/* pcl::EuclideanClusterExtraction over ppf_prep_clusters: the connected components of "two points are no
 * farther apart than the cluster tolerance" with MinClusterSize .. MaxClusterSize points (PCL's defaults 1 and 25000), the largest
 * first, as PCL sorts them.  Point types only need members x, y, z.  What differs from PCL, stated: the indices inside a cluster
 * are ascending (PCL's are in the order its search visited them); clusters of equal size come in the order of their smallest
 * index; the predicate is (dx*dx + dy*dy) + dz*dz <= tolerance * tolerance in fp64 on the float coordinates (PCL compares a
 * float squared distance from its k-d tree), so parity with PCL is unpinned, as for every other stage; at most 256 clusters, the
 * largest, are returned per call; points that are not finite belong to no cluster; a search method is not needed and none is
 * taken. */
template <class PointT>
class EuclideanClusterExtraction {
 public:
  void setClusterTolerance(double tolerance) { tolerance_ = tolerance; }
  double getClusterTolerance() const { return tolerance_; }
  void setMinClusterSize(int n) { min_ = n; }
  int getMinClusterSize() const { return min_; }
  void setMaxClusterSize(int n) { max_ = n; }
  int getMaxClusterSize() const { return max_; }
  template <class CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    read_ = [cloud](std::vector<float>& xyz) {
      const auto& p = detail::pts(*cloud);
      xyz.resize(p.size() * 3);
      for (std::size_t i = 0; i < p.size(); i++) { xyz[i * 3] = p[i].x; xyz[i * 3 + 1] = p[i].y; xyz[i * 3 + 2] = p[i].z; }
    };
  }
  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    if (!read_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "EuclideanClusterExtraction: no input cloud");
    std::vector<float> xyz;
    read_(xyz); /* the cloud as it is now, as PCL reads through the pointer at extract() */
    const int n = (int)(xyz.size() / 3);
    ppf_cluster_params p;
    ppf_default_cluster_params(&p);
    p.tolerance = (float)tolerance_;
    p.min_size = min_;
    p.max_size = max_;
    p.max_clusters = PPF_CLUSTER_MAX_CLUSTERS;
    ppf_cloud* in = nullptr;
    xyz.push_back(0.f);
    ppf_match_3d::check(ppf_cloud_upload(&xyz[0], n, 3, PPF_NOFF_MAT, 3, &in));
    std::shared_ptr<ppf_cloud> hold(in, [](ppf_cloud* c) { ppf_cloud_release(c); });
    const ppf_cloud* ins[1] = {in};
    std::vector<ppf_cloud*> out((std::size_t)PPF_CLUSTER_MAX_CLUSTERS, (ppf_cloud*)nullptr);
    std::vector<ppf_cluster_info> info((std::size_t)PPF_CLUSTER_MAX_CLUSTERS);
    std::vector<int32_t> labels((std::size_t)n + 1, -1);
    int32_t* labp[1] = {&labels[0]};
    int32_t counts[3] = {0, 0, 0};
    ppf_match_3d::check(ppf_prep_clusters(ins, 1, &p, nullptr, 0, 0, &out[0], &info[0], counts, labp, nullptr));
    for (std::size_t k = 0; k < out.size(); k++)
      if (out[k]) ppf_cloud_release(out[k]); /* the labels are what this surface hands out */
    clusters.resize((std::size_t)counts[0]);
    for (int r = 0; r < counts[0]; r++) clusters[(std::size_t)r].indices.reserve((std::size_t)info[(std::size_t)r].n_rows);
    for (int i = 0; i < n; i++)
      if (labels[(std::size_t)i] >= 0) clusters[(std::size_t)labels[(std::size_t)i]].indices.push_back(i);
  }

 private:
  double tolerance_ = 0.0;
  int min_ = 1, max_ = 25000;
  std::function<void(std::vector<float>&)> read_;
};

/* pcl::Normal's storage for builds without PCL (32 bytes: normal_x normal_y normal_z 0 | curvature pad pad pad) */
struct Normal {
  float normal_x, normal_y, normal_z, pad0;
  float curvature, pad1[3];
  Normal() : normal_x(0), normal_y(0), normal_z(0), pad0(0), curvature(0), pad1{0, 0, 0} {}
  Normal(float nx, float ny, float nz, float c = 0.f) : normal_x(nx), normal_y(ny), normal_z(nz), pad0(0), curvature(c), pad1{0, 0, 0} {}
};

/* pcl::RegionGrowing over ppf_prep_regions.  Points need members x, y, z; normals normal_x, normal_y,
 * normal_z and curvature (pcl::Normal qualifies).  setSmoothnessThreshold takes radians, as PCL does, and becomes normal_cos by
 * ppf_detmath's cosine; setCurvatureThreshold, setMinClusterSize and setMaxClusterSize are PCL's (a maximum
 * of 0, the default here, means no bound).  What differs from PCL, stated:
 *   - the neighbourhood is a radius, setDistanceThreshold (metres; default 0.01), not the k nearest (setNumberOfNeighbours does
 *     not exist here, and no search method is taken);
 *   - the normals are compared by the signed cosine, dot >= cos(threshold), unless setUnorientedFlag(true) makes it |dot| as
 *     PCL's always is;
 *   - component semantics instead of seed order: two smooth points (curvature <= the threshold) are linked iff they are
 *     within the distance and their normals agree, a region is a connected component of the links, and a point above the
 *     curvature threshold joins the region of the nearest smooth point it is within the distance of and agrees with, carrying
 *     no link itself.  PCL grows from seeds in curvature order and lets such a point join without becoming a seed, so where
 *     two regions touch PCL's answer depends on which seed came first; this one does not.  PCL's residual test is not there;
 *   - the indices inside a region are ascending, regions come largest first (equal sizes: by their smallest smooth index), at
 *     most 256 per call; points or normals that are not finite belong to no region. */
template <class PointT, class NormalT>
class RegionGrowing {
 public:
  void setDistanceThreshold(double metres) { tolerance_ = metres; }
  double getDistanceThreshold() const { return tolerance_; }
  void setSmoothnessThreshold(float radians) { theta_ = radians; }
  float getSmoothnessThreshold() const { return theta_; }
  void setCurvatureThreshold(float c) { curvature_ = c; }
  float getCurvatureThreshold() const { return curvature_; }
  void setMinClusterSize(int n) { min_ = n; }
  int getMinClusterSize() const { return min_; }
  void setMaxClusterSize(int n) { max_ = n; }
  int getMaxClusterSize() const { return max_; }
  void setUnorientedFlag(bool on) { unoriented_ = on; }
  template <class CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    points_ = [cloud](std::vector<float>& rows) {
      const auto& p = detail::pts(*cloud);
      rows.assign(p.size() * 6, 0.f);
      for (std::size_t i = 0; i < p.size(); i++) { rows[i * 6] = p[i].x; rows[i * 6 + 1] = p[i].y; rows[i * 6 + 2] = p[i].z; }
    };
  }
  template <class NormalsPtr> void setInputNormals(const NormalsPtr& normals) {
    normals_ = [normals](std::vector<float>& rows, std::vector<float>& curv) {
      const auto& q = detail::pts(*normals);
      if (q.size() * 6 != rows.size()) throw ppf_match_3d::Error(PPF_ERR_INVALID, "RegionGrowing: the normals are not as many as the points");
      curv.resize(q.size());
      for (std::size_t i = 0; i < q.size(); i++) {
        rows[i * 6 + 3] = q[i].normal_x; rows[i * 6 + 4] = q[i].normal_y; rows[i * 6 + 5] = q[i].normal_z;
        curv[i] = q[i].curvature;
      }
    };
  }
  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    if (!points_ || !normals_) throw ppf_match_3d::Error(PPF_ERR_INVALID, "RegionGrowing: no input cloud or no input normals");
    std::vector<float> rows, curv;
    points_(rows); /* the clouds as they are now, as PCL reads through the pointers at extract() */
    normals_(rows, curv);
    const int n = (int)curv.size();
    ppf_region_params p;
    ppf_default_region_params(&p);
    p.tolerance = (float)tolerance_;
    p.normal_cos = (float)ppf_cos((double)theta_);
    p.curvature_threshold = curvature_;
    p.min_size = min_;
    p.max_size = max_;
    p.max_regions = PPF_CLUSTER_MAX_CLUSTERS;
    p.flags = unoriented_ ? PPF_REGION_UNORIENTED : 0;
    ppf_cloud* in = nullptr;
    rows.push_back(0.f);
    curv.push_back(0.f);
    ppf_match_3d::check(ppf_cloud_upload(&rows[0], n, 6, PPF_NOFF_MAT, 6, &in));
    std::shared_ptr<ppf_cloud> hold(in, [](ppf_cloud* c) { ppf_cloud_release(c); });
    ppf_match_3d::check(ppf_cloud_set_curvature(in, &curv[0], n));
    const ppf_cloud* ins[1] = {in};
    std::vector<ppf_cloud*> out((std::size_t)PPF_CLUSTER_MAX_CLUSTERS, (ppf_cloud*)nullptr);
    std::vector<ppf_cluster_info> info((std::size_t)PPF_CLUSTER_MAX_CLUSTERS);
    std::vector<int32_t> labels((std::size_t)n + 1, -1);
    int32_t* labp[1] = {&labels[0]};
    int32_t counts[4] = {0, 0, 0, 0};
    ppf_match_3d::check(ppf_prep_regions(ins, 1, &p, nullptr, 0, 0, &out[0], &info[0], counts, labp, nullptr));
    for (std::size_t k = 0; k < out.size(); k++)
      if (out[k]) ppf_cloud_release(out[k]); /* the labels are what this surface hands out */
    clusters.resize((std::size_t)counts[0]);
    for (int r = 0; r < counts[0]; r++) clusters[(std::size_t)r].indices.reserve((std::size_t)info[(std::size_t)r].n_rows);
    for (int i = 0; i < n; i++)
      if (labels[(std::size_t)i] >= 0) clusters[(std::size_t)labels[(std::size_t)i]].indices.push_back(i);
  }

 private:
  double tolerance_ = 0.01;
  float theta_ = 30.0f / 180.0f * 3.14159265f; /* PCL's default */
  float curvature_ = 0.05f;                    /* PCL's default */
  int min_ = 1, max_ = 0;
  bool unoriented_ = false;
  std::function<void(std::vector<float>&)> points_;
  std::function<void(std::vector<float>&, std::vector<float>&)> normals_;
};

}  // namespace pcl_shaped
}  // namespace ppfhip

#endif /* PPF_PCL_HPP */
