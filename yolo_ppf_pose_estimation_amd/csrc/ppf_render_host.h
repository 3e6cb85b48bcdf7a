/*
 * ppf_render_host.h — host side of ppf_verify_frame_rendered (pose verification with self-occlusion) and ppf_render_frame
 * (depth and instance-label images of the chosen poses).  Kernels: ppf_render_kernels.h.  Included by ppf_hip.hip after
 * ppf_stage_host.h (FrameRun, FRAME_LAUNCH, stage_entry), ppf_posetable_host.h (the checks, job table and clears of a pose table)
 * and ppf_verify_host.h (verify_check, verify_tables, verify_scratch, verify_args).
 *
 * ppf_verify_frame_rendered, per call with at least one pose: the verify tables and grids (seven launches), then
 * k_rnd_window and the first read-back (each job's window), the window table upload, k_rnd_splat into one scratch of the
 * summed window sizes, k_rnd_vfy_score, k_vfy_finish and the second read-back (the score rows): eleven launches whatever
 * the number of detections.
 * ppf_render_frame, per call with at least one chosen pose: one upload of the job table, k_rnd_splat_frame into a
 * rows x cols u64 buffer, k_rnd_resolve, one read-back of both images.  Scratch comes from the block cache (FrameRun).
 */
namespace {

ppf_status render_params_check(const ppf_render_params* rp, const char* who) {
  if (!rp) return fail(PPF_ERR_INVALID, "%s: rparams is NULL", who);
  if (!(std::isfinite(rp->splat_radius) && rp->splat_radius > 0.f)) return fail(PPF_ERR_INVALID, "%s: splat_radius must be finite and > 0", who);
  if (!(std::isfinite(rp->visible_tol) && rp->visible_tol > 0.f)) return fail(PPF_ERR_INVALID, "%s: visible_tol must be finite and > 0", who);
  if (rp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)rp->flags);
  return PPF_OK;
}

RndCam render_cam(int rows, int cols, const double* intr, const ppf_render_params* rp) {
  RndCam c;
  c.rows = rows;
  c.cols = cols;
  c.fx = intr[0];
  c.fy = intr[1];
  c.ppx = intr[2];
  c.ppy = intr[3];
  c.r = (double)rp->splat_radius;
  c.tol = rp->visible_tol;
  return c;
}

/* each job's window from its box {-u0, -v0, u1, v1}, at its offset in one scratch of the summed sizes; returns that sum */
unsigned long long render_windows(const std::vector<int>& box, std::vector<RndWin>& win) {
  win.resize(box.size() / 4);
  unsigned long long total = 0;
  for (size_t j = 0; j < win.size(); j++) {
    const int* b = &box[j * 4];
    RndWin& w = win[j];
    w.u0 = -b[0];
    w.v0 = -b[1];
    const bool empty = b[2] < w.u0 || b[3] < w.v0; /* a job without a rendered row keeps the preset */
    w.w = empty ? 0 : b[2] - w.u0 + 1;
    w.h = empty ? 0 : b[3] - w.v0 + 1;
    if (empty) w.u0 = w.v0 = 0;
    w.off = total;
    total += (unsigned long long)w.w * (unsigned long long)w.h;
  }
  return total;
}

/* every job drawn alone: its window of the image, and its z-buffer there at its offset in one scratch */
struct RndWindows {
  std::vector<RndWin> win; /* the host's copy of d_win */
  RndWin* d_win = nullptr;
  uint32_t* zbuf = nullptr;
  RndCam cam;
};

/* job upload, k_rnd_window, one read-back (each job's box), the window table upload, k_rnd_splat; max_n as
 * table_render_jobs returns it */
ppf_status render_job_windows(FrameRun& fr, const std::vector<RndJob>& jobs, int max_n, int rows, int cols, const double* intr,
                              const ppf_render_params* rp, RndWindows& o) {
  const size_t nj = jobs.size();
  RndJob* d_jobs;
  int* d_box;
  ppf_status s = fr.get(nj, &d_jobs, nj, &o.d_win, nj * 4, &d_box);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(d_jobs, jobs.data(), nj * sizeof(RndJob), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(d_box, 0x80, nj * 4 * sizeof(int), nullptr));
  o.cam = render_cam(rows, cols, intr, rp);
  const dim3 grid_jobs(grid_for((size_t)max_n, RND_BLOCK).x, (unsigned)nj);
  FRAME_LAUNCH(fr, k_rnd_window, grid_jobs, dim3(RND_BLOCK), d_jobs, o.cam, d_box);
  HIPCHK(hipGetLastError());
  std::vector<int> box(nj * 4);
  if ((s = fr.read(box.data(), d_box, box.size() * sizeof(int))) != PPF_OK) return s;
  const unsigned long long total = render_windows(box, o.win);
  s = fr.get((size_t)total, &o.zbuf);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(o.d_win, o.win.data(), nj * sizeof(RndWin), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(o.zbuf, 0xff, (size_t)std::max<unsigned long long>(total, 1) * sizeof(uint32_t), nullptr));
  FRAME_LAUNCH(fr, k_rnd_splat, grid_jobs, dim3(RND_BLOCK), d_jobs, o.d_win, o.cam, o.zbuf);
  return PPF_OK;
}

/* tables and grids -> windows (read-back 1) -> per-job renders -> scores (the end); dev[j] = the score row of job j.  st gets
 * the counts of a failed run too */
ppf_status verify_rendered_run(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                               const float* depth, int rows, int cols, const double* intr, const ppf_verify_params* p,
                               const ppf_render_params* rp, std::vector<ppf_pose_score>& dev, ppf_verify_stats& st) {
  static const char* who = "ppf_verify_frame_rendered";
  FrameRun fr;
  ppf_pose_score* d_out = nullptr;
  auto run = [&]() -> ppf_status {
    VfyTables t;
    ppf_status s = verify_tables(dets, n_dets, poses, n_poses, top, p, who, t, fr);
    if (s != PPF_OK) return s;
    /* the render jobs: the same poses, every model row */
    std::vector<RndJob> rj;
    const int max_n = table_render_jobs(dets, n_dets, poses, n_poses, TABLE_N_POSES, top, LABEL_DET, rj);
    VfyPartial* part;
    float* d_depth = nullptr;
    RndWindows w;
    if ((s = verify_scratch(fr, t, depth, rows, cols, &part, &d_out, &d_depth)) != PPF_OK ||
        (s = render_job_windows(fr, rj, max_n, rows, cols, intr, rp, w)) != PPF_OK)
      return s;
    const VfyArgs a = verify_args(t, d_depth, rows, cols, intr, p);
    RndView rv;
    rv.wins = w.d_win;
    rv.zbuf = w.zbuf;
    rv.c = w.cam;
    FRAME_LAUNCH(fr, k_rnd_vfy_score, dim3((unsigned)t.max_nb, (unsigned)t.nj), dim3(VFY_BLOCK), a, rv, part);
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

/* the job table -> both images drawn -> the one wait, which brings them home.  st gets the counts of a failed run too */
ppf_status render_frame_run(const std::vector<RndJob>& jobs, int max_n, int rows, int cols, const double* intr, const ppf_render_params* rp,
                            float* depth_out, int32_t* label_out, ppf_render_stats& st) {
  const size_t npx = (size_t)rows * cols;
  FrameRun fr;
  RndJob* d_jobs;
  unsigned long long* zbuf;
  float* img; /* depth then label, one read-back */
  ppf_status s = fr.get(jobs.size(), &d_jobs, npx, &zbuf, 2 * npx, &img);
  if (s != PPF_OK) return s;
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(RndJob), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(zbuf, 0xff, npx * sizeof(unsigned long long), nullptr));
    const RndCam cam = render_cam(rows, cols, intr, rp);
    FRAME_LAUNCH(fr, k_rnd_splat_frame, dim3(grid_for((size_t)max_n, RND_BLOCK).x, (unsigned)jobs.size()), dim3(RND_BLOCK), d_jobs, cam, zbuf);
    FRAME_LAUNCH(fr, k_rnd_resolve, grid_for(npx, 256), dim3(256), zbuf, npx, img, (int32_t*)(img + npx));
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run();
  std::vector<float> host(2 * npx); /* filled while the kernels run */
  s = fr.finish("ppf_render_frame", ran, {{"images", img, 2 * npx * sizeof(float), host.data()}});
  fr.report(st);
  if (s != PPF_OK) return s;
  if (depth_out) std::memcpy(depth_out, host.data(), npx * sizeof(float));
  if (label_out) std::memcpy(label_out, host.data() + npx, npx * sizeof(int32_t));
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_render_params(ppf_render_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->splat_radius = 0.003f;
  p->visible_tol = 0.005f;
  p->flags = 0;
}

ppf_status ppf_verify_frame_rendered(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                                     const float* depth, int depth_rows, int depth_cols, const double* intr,
                                     const ppf_verify_params* params, const ppf_render_params* rparams, ppf_pose_score* scores,
                                     int* best, ppf_verify_stats* stats) {
  static const char* who = "ppf_verify_frame_rendered";
  auto clear = [&](ppf_verify_stats& st, bool failed) { /* as ppf_verify_frame */
    if (failed) return;
    std::memset(&st, 0, sizeof(st));
    table_clear_scores(n_dets, top, scores, best);
  };
  return stage_entry(stats, clear, [&](ppf_verify_stats& st) -> ppf_status {
    ppf_status s = verify_check(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, scores, best, who);
    if (s != PPF_OK) return s;
    if (params->flags & PPF_VERIFY_ALL_ROWS)
      return fail(PPF_ERR_INVALID, "%s: PPF_VERIFY_ALL_ROWS has no meaning against one view's z-buffer", who);
    if ((s = image_check(depth_rows, depth_cols, intr, true, who)) != PPF_OK || (s = render_params_check(rparams, who)) != PPF_OK) return s;
    st.n_dets = n_dets;
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    int n_jobs;
    if ((s = table_check_models(dets, n_dets, n_poses, TABLE_N_POSES, who, &n_jobs)) != PPF_OK || n_jobs == 0) return s;
    std::vector<ppf_pose_score> dev;
    if ((s = verify_rendered_run(dets, n_dets, poses, n_poses, top, depth, depth_rows, depth_cols, intr, params, rparams, dev, st)) != PPF_OK)
      return s;
    table_scatter_scores(dev, n_dets, n_poses, top, scores, best);
    st.n_jobs = n_jobs;
    return PPF_OK;
  });
}

ppf_status ppf_render_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* which, int top, int rows,
                            int cols, const double* intr, const ppf_render_params* rparams, float* depth_out, int32_t* label_out,
                            ppf_render_stats* stats) {
  static const char* who = "ppf_render_frame";
  /* on any error the given images are empty: clear what the size arguments let us reach.  The stats of a failed call keep
   * n_dets and the launch counts of the run */
  auto clear = [&](ppf_render_stats& st, bool failed) {
    if (!failed) std::memset(&st, 0, sizeof(st));
    table_clear_images(rows, cols, depth_out, label_out);
  };
  return stage_entry(stats, clear, [&](ppf_render_stats& st) -> ppf_status {
    ppf_status s;
    if ((s = table_check_sizes(n_dets, top, who)) != PPF_OK || (s = image_check(rows, cols, intr, true, who)) != PPF_OK ||
        (s = render_params_check(rparams, who)) != PPF_OK)
      return s;
    if (n_dets > 0 && (!dets || !poses || !which)) return fail(PPF_ERR_INVALID, "%s: dets, poses and which must not be NULL", who);
    for (int i = 0; i < n_dets; i++) {
      if (which[i] < -1 || which[i] >= top) return fail(PPF_ERR_INVALID, "%s: which[%d] = %d is outside [-1, top)", who, i, which[i]);
      if (which[i] >= 0 && !dets[i].model_cloud) return fail(PPF_ERR_INVALID, "%s: detection %d is chosen but has no model cloud", who, i);
    }
    st.n_dets = n_dets;
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    int n_jobs;
    if ((s = table_check_models(dets, n_dets, which, TABLE_WHICH, who, &n_jobs)) != PPF_OK || n_jobs == 0) return s;
    std::vector<RndJob> jobs;
    const int max_n = table_render_jobs(dets, n_dets, poses, which, TABLE_WHICH, top, LABEL_DET, jobs);
    if ((s = render_frame_run(jobs, max_n, rows, cols, intr, rparams, depth_out, label_out, st)) != PPF_OK) return s;
    st.n_jobs = n_jobs;
    return PPF_OK;
  });
}

}  // extern "C"
