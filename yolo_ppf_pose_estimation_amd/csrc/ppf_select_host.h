/*
 * ppf_select_host.h — host side of ppf_select_frame: one consistent set of poses among all hypotheses of a frame
 * (DESIGN.md §16).  Kernels: ppf_select_kernels.h, and k_rnd_window / k_rnd_splat / k_rnd_resolve of ppf_render_kernels.h.
 * Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, FRAME_LAUNCH, stage_entry), ppf_posetable_host.h (the checks, job
 * table, depth upload and clears of a pose table) and ppf_render_host.h (render_params_check, render_job_windows).
 *
 * Per call with at least one hypothesis: the uploads (job table, depth image, scores when given), k_rnd_window and the
 * first read-back (each job's window), the window and mask tables, k_rnd_splat, k_sel_mask, k_sel_key, k_sel_overlap,
 * k_sel_greedy, k_sel_report, with an image asked for k_sel_paint and k_rnd_resolve, and the second read-back (info rows,
 * the selection, the images, one block): seven or nine launches whatever the number of detections.  Pair storage is the
 * conflict bit matrix, n_jobs^2 / 8 bytes (2 MiB at the 4,096 hypotheses a call can hold).  Scratch comes from the block
 * cache (FrameRun).
 */
namespace {

static_assert(SEL_MAX_JOBS == FRAME_MATCH_MAX_DETS * FRAME_MATCH_MAX_TOP, "k_sel_greedy sorts every hypothesis of a call in LDS");

/* what the second read-back brings home */
struct SelResult {
  std::vector<ppf_select_info> info; /* per job */
  std::vector<int> selected;         /* per job: flat indices in selection order, then -1 */
  int n_selected = 0, n_eligible = 0;
};

/* st gets the counts of a failed run too */
ppf_status select_run(const std::vector<RndJob>& jobs, int max_n, const std::vector<float>* score, const float* depth, int rows, int cols,
                      const double* intr, const ppf_render_params* rp, const ppf_select_params* p, float* depth_out, int32_t* label_out,
                      SelResult& res, ppf_select_stats& st) {
  FrameRun fr;
  const int nj = (int)jobs.size();
  const size_t npx = (size_t)rows * cols;
  const bool images = depth_out || label_out;
  std::vector<int> flat((size_t)nj);
  for (int q = 0; q < nj; q++) flat[(size_t)q] = jobs[(size_t)q].label;
  SelMask* d_mask;
  int *d_flat, *d_counts, *d_sup;
  float *d_depth, *d_score = nullptr;
  unsigned long long* d_skey;
  uint32_t* d_conf;
  const int cw = (nj + 31) / 32;
  /* the results in one block: info rows, selected, {n_selected, n_eligible}, then the two images */
  const size_t info_b = (size_t)nj * sizeof(ppf_select_info), sel_b = (size_t)nj * sizeof(int);
  const size_t head_b = (info_b + sel_b + 2 * sizeof(int) + 7) & ~(size_t)7;
  const size_t out_b = head_b + (images ? 2 * npx * sizeof(float) : 0);
  unsigned char* d_out;
  ppf_status s = fr.get(nj, &d_mask, nj, &d_flat, (size_t)nj * 2, &d_counts, nj, &d_sup, nj, &d_skey, (size_t)nj * cw, &d_conf, out_b, &d_out);
  if (s == PPF_OK) s = frame_upload_depth(fr, depth, rows, cols, &d_depth);
  if (s == PPF_OK && score) s = fr.get(nj, &d_score);
  if (s != PPF_OK) return s;
  ppf_select_info* d_info = (ppf_select_info*)d_out;
  int* d_sel = (int*)(d_out + info_b);
  int* d_count = d_sel + nj;
  float* d_img = (float*)(d_out + head_b);
  HIPCHK(hipMemcpy(d_flat, flat.data(), (size_t)nj * sizeof(int), hipMemcpyHostToDevice));
  if (score) HIPCHK(hipMemcpy(d_score, score->data(), (size_t)nj * sizeof(float), hipMemcpyHostToDevice));
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)nj * 2 * sizeof(int), nullptr));
    HIPCHK(hipMemsetAsync(d_sup, 0xff, (size_t)nj * sizeof(int), nullptr));
    HIPCHK(hipMemsetAsync(d_conf, 0, (size_t)nj * cw * sizeof(uint32_t), nullptr));
    HIPCHK(hipMemsetAsync(d_sel, 0xff, sel_b, nullptr));
    HIPCHK(hipMemsetAsync(d_count, 0, 2 * sizeof(int), nullptr));
    /* each job's window and z-buffer (read-back 1), then its mask at its offset in a scratch of the summed sizes */
    RndWindows rw;
    ppf_status r = render_job_windows(fr, jobs, max_n, rows, cols, intr, rp, rw);
    if (r != PPF_OK) return r;
    std::vector<SelMask> mask((size_t)nj);
    unsigned long long words = 0, max_px = 1, max_words = 1;
    for (int q = 0; q < nj; q++) {
      const RndWin& w = rw.win[(size_t)q];
      SelMask& m = mask[(size_t)q];
      m.wc0 = w.u0 >> 6;
      m.ww = w.w > 0 ? ((w.u0 + w.w - 1) >> 6) - m.wc0 + 1 : 0;
      m.off = words;
      const unsigned long long mw = (unsigned long long)m.ww * (unsigned long long)w.h;
      words += mw;
      max_px = std::max(max_px, (unsigned long long)w.w * (unsigned long long)w.h);
      max_words = std::max(max_words, mw);
    }
    unsigned long long *bits, *frame = nullptr;
    r = fr.get((size_t)words, &bits);
    if (r == PPF_OK && images) r = fr.get(npx, &frame);
    if (r != PPF_OK) return r;
    HIPCHK(hipMemcpy(d_mask, mask.data(), mask.size() * sizeof(SelMask), hipMemcpyHostToDevice));
    FRAME_LAUNCH(fr, k_sel_mask, dim3(grid_for((size_t)max_words, SEL_MASK_WORDS).x, (unsigned)nj), dim3(SEL_BLOCK), rw.d_win, d_mask, rw.zbuf, d_depth, cols,
                 p->depth_tol, bits, d_counts);
    SelGate g;
    g.min_score = p->min_score;
    g.min_pixels = p->min_pixels;
    FRAME_LAUNCH(fr, k_sel_key, grid_for((size_t)nj, SEL_BLOCK), dim3(SEL_BLOCK), d_counts, d_score, nj, g, d_info, d_skey);
    FRAME_LAUNCH(fr, k_sel_overlap, dim3(grid_for((size_t)nj, SEL_WAVES).x, (unsigned)nj), dim3(SEL_BLOCK), rw.d_win, d_mask, bits, d_skey, d_info, nj,
                 (double)p->max_overlap, d_conf, cw);
    FRAME_LAUNCH(fr, k_sel_greedy, dim3(1), dim3(SEL_GREEDY_BLOCK), d_skey, nj, d_conf, cw, d_flat, d_info, d_sel, d_count, d_sup);
    FRAME_LAUNCH(fr, k_sel_report, grid_for((size_t)nj, SEL_WAVES), dim3(SEL_BLOCK), rw.d_win, d_mask, bits, d_sup, nj, d_info);
    if (images) {
      HIPCHK(hipMemsetAsync(frame, 0xff, npx * sizeof(unsigned long long), nullptr));
      FRAME_LAUNCH(fr, k_sel_paint, dim3(grid_for((size_t)max_px, SEL_BLOCK).x, (unsigned)nj), dim3(SEL_BLOCK), rw.d_win, rw.zbuf, d_info, d_flat, cols,
                   frame);
      FRAME_LAUNCH(fr, k_rnd_resolve, grid_for(npx, 256), dim3(256), frame, npx, d_img, (int32_t*)(d_img + npx));
    }
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run();
  std::vector<unsigned char> host(out_b); /* filled while the kernels run */
  s = fr.finish("ppf_select_frame", ran, {{"results", d_out, out_b, host.data()}});
  fr.report(st);
  if (s != PPF_OK) return s;
  res.info.resize((size_t)nj);
  res.selected.resize((size_t)nj);
  std::memcpy(res.info.data(), host.data(), info_b);
  std::memcpy(res.selected.data(), host.data() + info_b, sel_b);
  int count[2];
  std::memcpy(count, host.data() + info_b + sel_b, sizeof(count));
  res.n_selected = count[0];
  res.n_eligible = count[1];
  if (depth_out) std::memcpy(depth_out, host.data() + head_b, npx * sizeof(float));
  if (label_out) std::memcpy(label_out, host.data() + head_b + npx * sizeof(float), npx * sizeof(int32_t));
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_select_params(ppf_select_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->depth_tol = 0.01f;
  p->max_overlap = 0.25f;
  p->min_score = 0.f;
  p->min_pixels = 1;
  p->flags = 0;
}

ppf_status ppf_select_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const ppf_pose_score* scores, const float* depth, int depth_rows, int depth_cols, const double* intr,
                            const ppf_render_params* rparams, const ppf_select_params* params, ppf_select_info* info, int* selected,
                            int* n_selected, float* depth_out, int32_t* label_out, ppf_select_stats* stats) {
  static const char* who = "ppf_select_frame";
  /* on any error the outputs are empty: clear what the size arguments let us reach.  The stats of a failed call keep n_dets
   * and the launch counts of the run */
  const size_t n_flat = table_sized(n_dets, top) ? (size_t)n_dets * top : 0;
  auto clear = [&](ppf_select_stats& st, bool failed) {
    if (!failed) std::memset(&st, 0, sizeof(st));
    if (info && n_flat) std::memset(info, 0, n_flat * sizeof(ppf_select_info));
    if (selected && n_flat) std::fill(selected, selected + n_flat, -1);
    if (n_selected) *n_selected = 0;
    table_clear_images(depth_rows, depth_cols, depth_out, label_out);
  };
  return stage_entry(stats, clear, [&](ppf_select_stats& st) -> ppf_status {
    ppf_status s = table_check_sizes(n_dets, top, who);
    if (s != PPF_OK) return s;
    if (!params) return fail(PPF_ERR_INVALID, "%s: params is NULL", who);
    if (!n_selected) return fail(PPF_ERR_INVALID, "%s: n_selected is NULL", who);
    if ((s = table_check_rows(dets, n_dets, poses, n_poses, top, info && selected, "info and selected", false, who)) != PPF_OK) return s;
    if (!(std::isfinite(params->depth_tol) && params->depth_tol > 0.f)) return fail(PPF_ERR_INVALID, "%s: depth_tol must be finite and > 0", who);
    if (!(params->max_overlap >= 0.f && params->max_overlap <= 1.f)) return fail(PPF_ERR_INVALID, "%s: max_overlap must be in [0, 1]", who);
    if (!std::isfinite(params->min_score)) return fail(PPF_ERR_INVALID, "%s: min_score must be finite", who);
    if (params->min_pixels < 1) return fail(PPF_ERR_INVALID, "%s: min_pixels must be >= 1", who);
    if (params->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)params->flags);
    if (!depth) return fail(PPF_ERR_INVALID, "%s: depth is NULL (the depth image is required)", who);
    if ((s = image_check(depth_rows, depth_cols, intr, true, who)) != PPF_OK || (s = render_params_check(rparams, who)) != PPF_OK) return s;
    st.n_dets = n_dets;
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    int n_jobs;
    if ((s = table_check_models(dets, n_dets, n_poses, TABLE_N_POSES, who, &n_jobs)) != PPF_OK || n_jobs == 0) return s;
    std::vector<RndJob> jobs; /* labelled with the flat index: what label_out shows */
    const int max_n = table_render_jobs(dets, n_dets, poses, n_poses, TABLE_N_POSES, top, LABEL_FLAT, jobs);
    std::vector<float> key; /* the given scores in job order */
    for (int i = 0; scores && i < n_dets; i++)
      for (int k = 0; k < n_poses[i]; k++) key.push_back(scores[(size_t)i * top + k].score);
    SelResult res;
    s = select_run(jobs, max_n, scores ? &key : nullptr, depth, depth_rows, depth_cols, intr, rparams, params, depth_out, label_out, res, st);
    if (s != PPF_OK) return s;
    for (size_t q = 0; q < jobs.size(); q++) info[(size_t)jobs[q].label] = res.info[q];
    std::copy(res.selected.begin(), res.selected.end(), selected);
    *n_selected = res.n_selected;
    st.n_jobs = n_jobs;
    st.n_eligible = res.n_eligible;
    st.n_selected = res.n_selected;
    return PPF_OK;
  });
}

}  // extern "C"
