/*
 * ppf_refine_host.h — host side of ppf_refine_frame: projective point-to-plane refinement of every pose of every detection
 * of a frame against the depth image.  Kernel: ppf_refine_kernels.h.  Included by ppf_hip.hip after
 * ppf_icp_host.h (icp_set_pose), ppf_stage_host.h (FrameRun, FRAME_LAUNCH, stage_entry) and ppf_posetable_host.h (the checks
 * of a pose table, the depth upload).
 *
 * Per call with at least one pose and max_iters > 0: two uploads (the job table, the depth image), one launch
 * (k_rfn_refine: a persistent workgroup per pose runs the centre, every iteration and the info row) and one read-back (the
 * matrices and info rows), whatever the number of detections.  Scratch comes from the block cache (FrameRun).
 */
namespace {

ppf_status refine_check(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top, const float* depth,
                        int depth_rows, int depth_cols, const double* intr, const ppf_refine_params* p, ppf_pose* out, const char* who) {
  ppf_status s = table_check_sizes(n_dets, top, who);
  if (s != PPF_OK) return s;
  if (!p) return fail(PPF_ERR_INVALID, "%s: params is NULL", who);
  if ((s = table_check_rows(dets, n_dets, poses, n_poses, top, out != nullptr, "out", false, who)) != PPF_OK) return s;
  if (!(std::isfinite(p->depth_gate) && p->depth_gate > 0.f)) return fail(PPF_ERR_INVALID, "%s: depth_gate must be finite and > 0", who);
  if (!(std::isfinite(p->max_step_rot) && p->max_step_rot > 0.f)) return fail(PPF_ERR_INVALID, "%s: max_step_rot must be finite and > 0", who);
  if (!(std::isfinite(p->max_step_trans) && p->max_step_trans > 0.f))
    return fail(PPF_ERR_INVALID, "%s: max_step_trans must be finite and > 0", who);
  if (!(std::isfinite(p->eps_rot) && p->eps_rot >= 0.f)) return fail(PPF_ERR_INVALID, "%s: eps_rot must be finite and >= 0", who);
  if (!(std::isfinite(p->eps_trans) && p->eps_trans >= 0.f)) return fail(PPF_ERR_INVALID, "%s: eps_trans must be finite and >= 0", who);
  if (!(p->min_pair_share >= 0.f && p->min_pair_share <= 1.f)) return fail(PPF_ERR_INVALID, "%s: min_pair_share must be in [0, 1]", who);
  if (p->min_pairs < 6) return fail(PPF_ERR_INVALID, "%s: min_pairs must be >= 6", who);
  if (p->max_iters < 0 || p->max_iters > 100) return fail(PPF_ERR_INVALID, "%s: max_iters must be in [0, 100]", who);
  if (p->model_step < 1) return fail(PPF_ERR_INVALID, "%s: model_step must be >= 1", who);
  if (p->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  if (!depth) return fail(PPF_ERR_INVALID, "%s: depth is NULL", who);
  return image_check(depth_rows, depth_cols, intr, false, who);
}

/* out = poses and every info row zero, where the size arguments let us reach them (out may be poses itself) */
void refine_clear(int n_dets, int top, const ppf_pose* poses, ppf_pose* out, ppf_refine_info* info) {
  if (!table_sized(n_dets, top)) return;
  const size_t n = (size_t)n_dets * top;
  if (out && poses && out != poses) std::memmove(out, poses, n * sizeof(ppf_pose));
  if (info) std::memset(info, 0, n * sizeof(ppf_refine_info));
}

/* the job table -> k_rfn_refine -> the one wait; dev[j] = the matrix and info row of job j, (i, k) order.  st gets the counts
 * of a failed run too */
ppf_status refine_run(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top, const float* depth,
                      int depth_rows, int depth_cols, const double* intr, const ppf_refine_params* p, std::vector<RfnOut>& dev,
                      ppf_refine_stats& st) {
  FrameRun fr;
  std::vector<RfnJob> hj;
  size_t n_parts = 0;
  for (int i = 0; i < n_dets; i++) {
    const int n_model = dets[i].model_cloud ? dets[i].model_cloud->n : 0;
    const int n_rows = (int)(((long long)n_model + p->model_step - 1) / p->model_step);
    for (int k = 0; k < n_poses[i]; k++) {
      RfnJob j;
      std::memcpy(j.T, poses[(size_t)i * top + k].pose, sizeof(j.T));
      j.model = dets[i].model_cloud->rows.p;
      j.n_rows = n_rows;
      j.pad = 0;
      j.o_parts = n_parts;
      n_parts += (size_t)((n_rows + ICP_CHUNK - 1) / ICP_CHUNK) * ICP_ENTRIES;
      hj.push_back(j);
    }
  }
  RfnArgs a;
  RfnJob* d_jobs;
  float* d_depth;
  ppf_status s = fr.get(hj.size(), &d_jobs, n_parts, &a.parts, hj.size(), &a.out);
  if (s == PPF_OK) s = frame_upload_depth(fr, depth, depth_rows, depth_cols, &d_depth);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(d_jobs, hj.data(), hj.size() * sizeof(RfnJob), hipMemcpyHostToDevice));
  a.jobs = d_jobs;
  a.depth = d_depth;
  a.rows = depth_rows;
  a.cols = depth_cols;
  a.fx = intr[0]; a.fy = intr[1]; a.ppx = intr[2]; a.ppy = intr[3];
  a.max_rot2 = (double)p->max_step_rot * (double)p->max_step_rot;
  a.max_trans2 = (double)p->max_step_trans * (double)p->max_step_trans;
  a.eps_rot2 = (double)p->eps_rot * (double)p->eps_rot;
  a.eps_trans2 = (double)p->eps_trans * (double)p->eps_trans;
  a.gate = p->depth_gate;
  a.min_pair_share = p->min_pair_share;
  a.min_pairs = p->min_pairs;
  a.max_iters = p->max_iters;
  a.step = p->model_step;
  auto run = [&]() -> ppf_status {
    FRAME_LAUNCH(fr, k_rfn_refine, dim3((unsigned)hj.size()), dim3(RFN_BLOCK), a);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run();
  dev.resize(hj.size()); /* while the kernel runs */
  s = fr.finish("ppf_refine_frame", ran, {{"results", a.out, hj.size() * sizeof(RfnOut), dev.data()}});
  fr.report(st);
  return s;
}

}  // namespace

extern "C" {

void ppf_default_refine_params(ppf_refine_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->depth_gate = 0.02f;
  p->max_step_rot = 0.35f;
  p->max_step_trans = 0.03f;
  p->eps_rot = 1e-5f;
  p->eps_trans = 1e-5f;
  p->min_pair_share = 0.25f;
  p->min_pairs = 16;
  p->max_iters = 20;
  p->model_step = 1;
  p->flags = 0;
}

ppf_status ppf_refine_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const float* depth, int depth_rows, int depth_cols, const double* intr, const ppf_refine_params* params,
                            ppf_pose* out, ppf_refine_info* info, ppf_refine_stats* stats) {
  static const char* who = "ppf_refine_frame";
  /* on any error out is a copy of poses and every info row is zero: what the valid part of the arguments lets us reach.  The
   * stats of a failed call keep n_dets and the launch counts of the run */
  auto clear = [&](ppf_refine_stats& st, bool failed) {
    if (failed) return;
    std::memset(&st, 0, sizeof(st));
    refine_clear(n_dets, top, poses, out, info);
  };
  return stage_entry(stats, clear, [&](ppf_refine_stats& st) -> ppf_status {
    ppf_status s = refine_check(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, out, who);
    if (s != PPF_OK) return s;
    st.n_dets = n_dets;
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    int n_jobs;
    if ((s = table_check_models(dets, n_dets, n_poses, TABLE_N_POSES, who, &n_jobs)) != PPF_OK) return s;
    if (n_jobs > 0 && params->max_iters == 0) {
      /* nothing is evaluated: the poses as given */
      for (int i = 0; i < n_dets; i++)
        for (int k = 0; k < n_poses[i] && info; k++) {
          ppf_refine_info& r = info[(size_t)i * top + k];
          r.status = PPF_REFINE_MAX_ITERS;
          r.n_rows = (int32_t)(((long long)dets[i].model_cloud->n + params->model_step - 1) / params->model_step);
        }
    } else if (n_jobs > 0) {
      std::vector<RfnOut> dev;
      if ((s = refine_run(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, dev, st)) != PPF_OK) return s;
      size_t j = 0;
      for (int i = 0; i < n_dets; i++)
        for (int k = 0; k < n_poses[i]; k++, j++) {
          ppf_pose& o = out[(size_t)i * top + k];
          /* a pose no step was applied to keeps its record (the matrix is the one given); only the residual is new */
          if (dev[j].info.iterations > 0) icp_set_pose(&o, dev[j].T, (double)dev[j].info.rmse_last);
          else o.residual = (double)dev[j].info.rmse_last;
          if (info) info[(size_t)i * top + k] = dev[j].info;
        }
    }
    st.n_jobs = n_jobs;
    return PPF_OK;
  });
}

}  // extern "C"
