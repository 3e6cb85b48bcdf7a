/*
 * ppf_verify_host.h — host side of ppf_verify_frame: score every refined pose of every detection of a frame against its
 * object cloud and, optionally, the depth image (what the reference leaves as `// TODO: Pose Validation`,
 * CloudProcessing.h:477-479, :530-532).  Kernels: ppf_verify_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h
 * (FrameRun, FRAME_LAUNCH, frame_scan, stage_entry) and ppf_posetable_host.h (the checks, clears and score scatter of a pose table).
 *
 * Per call with at least one pose: three uploads (the detection and job tables, the depth image when given), then
 * k_vfy_grid_count, a five-launch scan, k_vfy_grid_scatter, k_vfy_score, k_vfy_finish -- nine launches whatever the number
 * of detections -- and one read-back, the score rows.  The slot offsets of every detection's grid follow from the cloud
 * sizes the host already knows, so building the grids needs no read-back.  Scratch comes from the block cache (FrameRun).
 */
namespace {

/* the arguments of both verify entries, in the order their errors win */
ppf_status verify_check(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top, const float* depth,
                        int depth_rows, int depth_cols, const double* intr, const ppf_verify_params* p, ppf_pose_score* scores, int* best,
                        const char* who) {
  ppf_status s = table_check_sizes(n_dets, top, who);
  if (s != PPF_OK) return s;
  if (!p) return fail(PPF_ERR_INVALID, "%s: params is NULL", who);
  if ((s = table_check_rows(dets, n_dets, poses, n_poses, top, scores && best, "scores and best", true, who)) != PPF_OK) return s;
  if (!(std::isfinite(p->inlier_dist) && p->inlier_dist > 0.f)) return fail(PPF_ERR_INVALID, "%s: inlier_dist must be finite and > 0", who);
  if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f)) return fail(PPF_ERR_INVALID, "%s: normal_cos must be in [-1, 1]", who);
  if (!(std::isfinite(p->depth_tol) && p->depth_tol > 0.f)) return fail(PPF_ERR_INVALID, "%s: depth_tol must be finite and > 0", who);
  if (p->model_step < 1) return fail(PPF_ERR_INVALID, "%s: model_step must be >= 1", who);
  if (p->flags & ~(PPF_VERIFY_ALL_ROWS | PPF_VERIFY_NORMALS)) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  return depth ? image_check(depth_rows, depth_cols, intr, false, who) : PPF_OK;
}

/* what the scoring needs on the device: the detection and job tables and every live detection's grid */
struct VfyTables {
  std::vector<VfyJob> hj;
  VfyDet* d_dets = nullptr;
  VfyJob* d_jobs = nullptr;
  uint32_t* start = nullptr;
  float4* pts = nullptr;
  int nd = 0, nj = 0, max_nb = 1;
  double inv_h = 0.0;
};

/* the tables (uploaded) and the grids (k_vfy_grid_count, frame_scan, k_vfy_grid_scatter): seven launches, no read-back */
ppf_status verify_tables(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                         const ppf_verify_params* p, const char* who, VfyTables& t, FrameRun& fr) {
  /* live detections (with poses) and their slots; the jobs */
  std::vector<VfyDet> hd;
  std::vector<VfyJob>& hj = t.hj;
  std::vector<int> det_of((size_t)n_dets, -1);
  size_t slots = 0, rows = 0;
  int max_scene = 0, max_nb = 1;
  for (int i = 0; i < n_dets; i++) {
    if (n_poses[i] == 0) continue;
    VfyDet d;
    d.rows = dets[i].scene->rows.p;
    d.n = dets[i].scene->n;
    const uint32_t s = next_pow2((uint32_t)std::max(64, 2 * d.n));
    d.slot_off = (uint32_t)slots;
    d.slot_mask = s - 1;
    d.row_off = (uint32_t)rows;
    slots += s;
    rows += (size_t)d.n;
    max_scene = std::max(max_scene, d.n);
    det_of[i] = (int)hd.size();
    hd.push_back(d);
    const int n_model = dets[i].model_cloud->n;
    const int n_rows = (int)(((long long)n_model + p->model_step - 1) / p->model_step);
    for (int k = 0; k < n_poses[i]; k++) {
      VfyJob j;
      std::memcpy(j.T, poses[(size_t)i * top + k].pose, sizeof(j.T));
      j.model = dets[i].model_cloud->rows.p;
      j.scene = d.rows;
      j.n_rows = n_rows;
      j.nb = (n_rows + VFY_BLOCK - 1) / VFY_BLOCK;
      j.det = det_of[i];
      j.pad = 0;
      max_nb = std::max(max_nb, j.nb);
      hj.push_back(j);
    }
  }
  if (slots + 1 > 0xffffffffull || rows > 0xffffffffull) return fail(PPF_ERR_CAPACITY, "%s: the scene clouds are too large", who);
  t.nd = (int)hd.size();
  t.nj = (int)hj.size();
  t.max_nb = max_nb;
  uint32_t *counts, *rank;
  ppf_status s = fr.get(t.nd, &t.d_dets, t.nj, &t.d_jobs, slots + 1, &counts, slots + 1, &t.start, rows, &rank, rows, &t.pts);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(t.d_dets, hd.data(), hd.size() * sizeof(VfyDet), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t.d_jobs, hj.data(), hj.size() * sizeof(VfyJob), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(counts, 0, (slots + 1) * sizeof(uint32_t), nullptr));
  t.inv_h = 1.0 / ((double)p->inlier_dist * VFY_CELL_MARGIN);
  const dim3 grid_rows(grid_for((size_t)max_scene, 256).x, (unsigned)t.nd);
  FRAME_LAUNCH(fr, k_vfy_grid_count, grid_rows, dim3(256), t.d_dets, t.inv_h, counts, rank);
  if ((s = frame_scan(fr, counts, t.start, slots + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_vfy_grid_scatter, grid_rows, dim3(256), t.d_dets, t.inv_h, t.start, rank, t.pts);
  return PPF_OK;
}

/* the scoring arguments of the tables; depth (a device image) may be NULL, intr then too */
VfyArgs verify_args(const VfyTables& t, const float* d_depth, int depth_rows, int depth_cols, const double* intr, const ppf_verify_params* p) {
  VfyArgs a;
  a.dets = t.d_dets;
  a.jobs = t.d_jobs;
  a.slot_start = t.start;
  a.pts = t.pts;
  a.depth = d_depth;
  a.rows = d_depth ? depth_rows : 0;
  a.cols = d_depth ? depth_cols : 0;
  a.fx = d_depth ? intr[0] : 0.0;
  a.fy = d_depth ? intr[1] : 0.0;
  a.ppx = d_depth ? intr[2] : 0.0;
  a.ppy = d_depth ? intr[3] : 0.0;
  a.inv_h = t.inv_h;
  a.r2 = p->inlier_dist * p->inlier_dist;
  a.normal_cos = p->normal_cos;
  a.depth_tol = p->depth_tol;
  a.step = p->model_step;
  a.all_rows = (p->flags & PPF_VERIFY_ALL_ROWS) ? 1 : 0;
  a.normals = (p->flags & PPF_VERIFY_NORMALS) ? 1 : 0;
  a.max_nb = t.max_nb;
  return a;
}

/* the scratch of the scoring that follows the tables: the partial sums, the score rows, the depth image when given */
ppf_status verify_scratch(FrameRun& fr, const VfyTables& t, const float* depth, int depth_rows, int depth_cols, VfyPartial** part,
                          ppf_pose_score** d_out, float** d_depth) {
  const ppf_status s = fr.get((size_t)t.nj * t.max_nb, part, t.nj, d_out);
  if (s != PPF_OK || !depth) return s;
  return frame_upload_depth(fr, depth, depth_rows, depth_cols, d_depth);
}

/* grids -> scores -> the one wait; dev[j] = the score row of job j on the host.  st gets the counts of a failed run too */
ppf_status verify_run(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top, const float* depth,
                      int depth_rows, int depth_cols, const double* intr, const ppf_verify_params* p, std::vector<ppf_pose_score>& dev,
                      ppf_verify_stats& st) {
  static const char* who = "ppf_verify_frame";
  FrameRun fr;
  ppf_pose_score* d_out = nullptr;
  auto run = [&]() -> ppf_status {
    VfyTables t;
    VfyPartial* part;
    float* d_depth = nullptr;
    ppf_status s;
    if ((s = verify_tables(dets, n_dets, poses, n_poses, top, p, who, t, fr)) != PPF_OK ||
        (s = verify_scratch(fr, t, depth, depth_rows, depth_cols, &part, &d_out, &d_depth)) != PPF_OK)
      return s;
    const VfyArgs a = verify_args(t, d_depth, depth_rows, depth_cols, intr, p);
    FRAME_LAUNCH(fr, k_vfy_score, dim3((unsigned)t.max_nb, (unsigned)t.nj), dim3(VFY_BLOCK), a, part);
    FRAME_LAUNCH(fr, k_vfy_finish, dim3((unsigned)t.nj), dim3(64), t.d_jobs, part, t.max_nb, depth ? 1 : 0, d_out);
    HIPCHK(hipGetLastError());
    dev.resize((size_t)t.nj);
    return PPF_OK;
  };
  const ppf_status ran = run(); /* before d_out and dev are read */
  const ppf_status s = fr.finish(who, ran, {{"scores", d_out, dev.size() * sizeof(ppf_pose_score), dev.data()}});
  fr.report(st);
  return s;
}

}  // namespace

extern "C" {

void ppf_default_verify_params(ppf_verify_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->inlier_dist = 0.005f;
  p->normal_cos = 0.5f;
  p->depth_tol = 0.01f;
  p->model_step = 1;
  p->flags = 0;
}

ppf_status ppf_verify_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const float* depth, int depth_rows, int depth_cols, const double* intr, const ppf_verify_params* params,
                            ppf_pose_score* scores, int* best, ppf_verify_stats* stats) {
  static const char* who = "ppf_verify_frame";
  /* on any error every score row is zero and every best[i] is -1: clear what the valid part of the arguments lets us reach.
   * The stats of a failed call keep n_dets and the launch counts of the run */
  auto clear = [&](ppf_verify_stats& st, bool failed) {
    if (failed) return;
    std::memset(&st, 0, sizeof(st));
    table_clear_scores(n_dets, top, scores, best);
  };
  return stage_entry(stats, clear, [&](ppf_verify_stats& st) -> ppf_status {
    ppf_status s = verify_check(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, scores, best, who);
    if (s != PPF_OK) return s;
    st.n_dets = n_dets;
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    int n_jobs;
    if ((s = table_check_models(dets, n_dets, n_poses, TABLE_N_POSES, who, &n_jobs)) != PPF_OK || n_jobs == 0) return s;
    std::vector<ppf_pose_score> dev;
    if ((s = verify_run(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, dev, st)) != PPF_OK) return s;
    table_scatter_scores(dev, n_dets, n_poses, top, scores, best);
    st.n_jobs = n_jobs;
    return PPF_OK;
  });
}

}  // extern "C"
