/*
 * ppf_match_frame_host.h — host side of ppf_match_frame: match (or match_S2B) every detection of a frame, then refine the
 * top poses of all detections in ONE segmented ICP launch sequence (the reference matches and refines detection after
 * detection, CloudProcessing.h:495-523).  Included by ppf_hip.hip after ppf_icp_host.h and ppf_prep_host.h (ppf_cloud,
 * HostLoan, icp_batch_run_jobs, icp_append_pose).
 *
 * Match phase: each detection borrows a warm context of its model (HostLoan) and goes through ppf_match_device /
 * ppf_workspace_results, as ppf_match_clouds does.  Up to FRAME_MATCH_INFLIGHT detections are enqueued before the first
 * of them is read back, so matches on different contexts overlap; the read-backs of this phase grow with K.
 * ICP phase: the first min(top, matches) poses of every detection become the jobs of one segmented ICP call
 * (ppf_icp_host.h): each job has its own model cloud, scene cloud and level schedule, and its launches are the same
 * whatever the number of jobs, up to ICP_GROUP_JOBS of them.
 */
namespace {

constexpr int FRAME_MATCH_MAX_DETS = 256;
constexpr int FRAME_MATCH_MAX_TOP = 16;
constexpr int FRAME_MATCH_INFLIGHT = 8; /* detections enqueued ahead of the first read-back (bounds the contexts a call opens) */

bool frame_det_live(const ppf_frame_detection& d) {
  return d.model && d.scene->n > 0 && (!d.edge || d.edge->n > 0);
}

ppf_status frame_match_segmented(const ppf_frame_detection* dets, int n_dets, const ppf_match_params* mp, const ppf_icp_params* ip,
                                 int top, ppf_pose* out, int* n_out, int32_t* icp_iterations, ppf_match_frame_stats* st) {
  const int sync0 = g_host_syncs;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int> live;
  for (int i = 0; i < n_dets; i++)
    if (frame_det_live(dets[i])) live.push_back(i);
  std::vector<int> found((size_t)n_dets, 0);
  for (size_t w0 = 0; w0 < live.size(); w0 += FRAME_MATCH_INFLIGHT) {
    const size_t w1 = std::min(live.size(), w0 + FRAME_MATCH_INFLIGHT);
    std::vector<std::unique_ptr<HostLoan>> loans;
    for (size_t q = w0; q < w1; q++) {
      const ppf_frame_detection& d = dets[live[q]];
      loans.emplace_back(new HostLoan(d.model));
      HostLoan& loan = *loans.back();
      ppf_status s = loan.open();
      if (s == PPF_OK) s = ppf_workspace_enable_timing(&loan.c->ws, 0);
      if (s == PPF_OK)
        s = ppf_match_device(d.model, &loan.c->ws, d.scene->rows.p, d.scene->n, 6, 3, d.edge ? d.edge->rows.p : nullptr, d.edge ? d.edge->n : 0,
                             6, 3, mp, loan.c->stream);
      if (s != PPF_OK) return s;
    }
    for (size_t q = w0; q < w1; q++) {
      const int i = live[q];
      HostLoan& loan = *loans[q - w0];
      int n = 0;
      ppf_status s = ppf_workspace_results(&loan.c->ws, nullptr, nullptr, 0, nullptr, nullptr, 0, &n, nullptr);
      if (s != PPF_OK) return s;
      const int k = std::min(top, n);
      if (k > 0) {
        std::vector<ppf_pose> all((size_t)n);
        if ((s = ppf_workspace_results(&loan.c->ws, nullptr, nullptr, 0, nullptr, all.data(), n, &n, nullptr)) != PPF_OK) return s;
        memcpy(out + (size_t)i * top, all.data(), (size_t)k * sizeof(ppf_pose));
      }
      found[i] = k;
      loan.ok = true;
    }
  }
  const auto t1 = std::chrono::steady_clock::now();
  st->ms_match = std::chrono::duration<float, std::milli>(t1 - t0).count();
  st->n_host_syncs += g_host_syncs - sync0;
  /* every detection's poses are the jobs of one segmented ICP call */
  std::vector<IcpJobSpec> specs;
  std::vector<ppf_pose*> job_pose;
  for (int i = 0; i < n_dets; i++) {
    if (found[i] == 0) continue;
    st->n_matched++;
    const ppf_frame_detection& d = dets[i];
    for (int k = 0; k < found[i]; k++) {
      ppf_pose* p = out + (size_t)i * top + k;
      specs.push_back(IcpJobSpec{d.model_cloud->rows.p, d.model_cloud->n, 6, 3, d.scene->rows.p, d.scene->n, 6, 3, p->pose});
      job_pose.push_back(p);
    }
  }
  st->n_icp_jobs = (int)specs.size();
  if (!specs.empty()) {
    const size_t J = specs.size();
    std::vector<double> inc(J * 16), res(J);
    std::vector<int> it(J);
    IcpRunCount cnt;
    const ppf_status s = icp_batch_run_jobs(specs.data(), (int)J, *ip, nullptr, inc.data(), res.data(), it.data(), cnt);
    st->n_icp_launches = cnt.launches;
    st->n_icp_passes = cnt.passes;
    st->n_host_syncs += cnt.syncs;
    if (s != PPF_OK) return s;
    for (size_t j = 0; j < J; j++) {
      icp_append_pose(job_pose[j], inc.data() + j * 16, res[j]);
      if (icp_iterations) icp_iterations[job_pose[j] - out] = it[j];
    }
  }
  st->ms_icp = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
  for (int i = 0; i < n_dets; i++) n_out[i] = found[i];
  return PPF_OK;
}

}  // namespace

extern "C" {

ppf_status ppf_match_frame(const ppf_frame_detection* dets, int n_dets, const ppf_match_params* mp, const ppf_icp_params* ip, int top,
                           ppf_pose* out, int* n_out, int32_t* icp_iterations, ppf_match_frame_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  ppf_match_frame_stats local;
  ppf_match_frame_stats& st = stats ? *stats : local;
  std::memset(&st, 0, sizeof(st));
  if (n_dets < 0 || n_dets > FRAME_MATCH_MAX_DETS)
    return fail(PPF_ERR_INVALID, "ppf_match_frame: n_dets must be in [0, %d]", FRAME_MATCH_MAX_DETS);
  if (n_out)
    for (int i = 0; i < n_dets; i++) n_out[i] = 0;
  if (top < 1 || top > FRAME_MATCH_MAX_TOP) return fail(PPF_ERR_INVALID, "ppf_match_frame: top must be in [1, %d]", FRAME_MATCH_MAX_TOP);
  if (!mp || !ip) return fail(PPF_ERR_INVALID, "ppf_match_frame: parameters are NULL");
  if (n_dets > 0 && (!dets || !out || !n_out)) return fail(PPF_ERR_INVALID, "ppf_match_frame: dets, out and n_out must not be NULL");
  if (!(mp->relative_scene_sample_step <= 1 && mp->relative_scene_sample_step > 0) || (!mp->presampled && !(mp->relative_scene_distance > 0)) ||
      mp->ref_stride < 1 || mp->ref_offset < 0)
    return fail(PPF_ERR_INVALID, "ppf_match_frame: bad match parameters");
  if (ip->iterations < 0 || ip->num_levels < 0 || ip->num_levels > 30 || !(ip->tolerance >= 0))
    return fail(PPF_ERR_INVALID, "ppf_match_frame: bad ICP parameters");
  for (int i = 0; i < n_dets; i++) {
    if (!dets[i].model) continue;
    if (!dets[i].scene || !dets[i].model_cloud)
      return fail(PPF_ERR_INVALID, "ppf_match_frame: detection %d has a model but no scene or model cloud", i);
  }
  st.n_dets = n_dets;
  /* the device check comes before any use of a handle */
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_match_frame: no HIP device (this engine has no CPU fallback)");
  for (int i = 0; i < n_dets; i++)
    if (dets[i].model && dets[i].model_cloud->n <= 0) return fail(PPF_ERR_INVALID, "ppf_match_frame: detection %d has an empty model cloud", i);
  std::memset(out, 0, (size_t)n_dets * top * sizeof(ppf_pose));
  if (icp_iterations) std::memset(icp_iterations, 0, (size_t)n_dets * top * sizeof(int32_t));
  ppf_status s = PPF_OK;
  if (n_dets > 0) s = frame_match_segmented(dets, n_dets, mp, ip, top, out, n_out, icp_iterations, &st);
  if (s != PPF_OK)
    for (int i = 0; i < n_dets; i++) n_out[i] = 0;
  st.ms_wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return s;
}

}  // extern "C"
