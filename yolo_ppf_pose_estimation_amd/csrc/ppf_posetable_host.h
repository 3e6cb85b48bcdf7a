/*
 * ppf_posetable_host.h — what the stages on a frame's pose table share on the host: ppf_verify_frame,
 * ppf_verify_frame_rendered, ppf_render_frame and ppf_select_frame all take dets[n_dets], poses[n_dets * top] and one
 * count per detection (n_poses[i] poses, or which[i], the one chosen pose or -1).  Here: the argument checks, the render
 * job table, the depth upload, the output clears and the score scatter.  Included by ppf_hip.hip after ppf_frame_host.h
 * (FrameRun) and ppf_match_frame_host.h (the limits of ppf_match_frame), before the stage headers ppf_verify_host.h,
 * ppf_render_host.h and ppf_select_host.h.
 *
 * An entry keeps its own order of checks (which error wins when two are present is part of its contract), so the checks
 * come as pieces: table_check_sizes first in every entry, then the entry's own, table_check_rows, image_check.
 */
namespace {

/* true when n_dets x top is a table an entry may clear on error */
bool table_sized(int n_dets, int top) { return n_dets > 0 && n_dets <= FRAME_MATCH_MAX_DETS && top >= 1 && top <= FRAME_MATCH_MAX_TOP; }

ppf_status table_check_sizes(int n_dets, int top, const char* who) {
  if (n_dets < 0 || n_dets > FRAME_MATCH_MAX_DETS) return fail(PPF_ERR_INVALID, "%s: n_dets must be in [0, %d]", who, FRAME_MATCH_MAX_DETS);
  if (top < 1 || top > FRAME_MATCH_MAX_TOP) return fail(PPF_ERR_INVALID, "%s: top must be in [1, %d]", who, FRAME_MATCH_MAX_TOP);
  return PPF_OK;
}

/* the tables of an entry that takes n_poses: present (outs = its per-table outputs are, `names` says which they are), every
 * count in [0, top], and every detection with poses has its model cloud (and its scene, where the entry reads it) */
ppf_status table_check_rows(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top, bool outs,
                            const char* names, bool need_scene, const char* who) {
  if (n_dets > 0 && (!dets || !poses || !n_poses || !outs)) return fail(PPF_ERR_INVALID, "%s: dets, poses, n_poses, %s must not be NULL", who, names);
  for (int i = 0; i < n_dets; i++) {
    if (n_poses[i] < 0 || n_poses[i] > top) return fail(PPF_ERR_INVALID, "%s: n_poses[%d] = %d is outside [0, top]", who, i, n_poses[i]);
    if (n_poses[i] > 0 && (!dets[i].model_cloud || (need_scene && !dets[i].scene)))
      return fail(PPF_ERR_INVALID, "%s: detection %d has poses but no model cloud%s", who, i, need_scene ? " or scene" : "");
  }
  return PPF_OK;
}

/* what counts[i] is: the number of poses of detection i (all are taken), or which[i], the one pose taken (-1: none) */
enum TableCounts { TABLE_N_POSES, TABLE_WHICH };
/* what a render job is labelled with: its detection index i, or its flat index i * top + k */
enum JobLabel { LABEL_DET, LABEL_FLAT };

/* the first and one past the last pose taken of detection i */
int table_k0(const int* counts, int i, TableCounts c) { return c == TABLE_WHICH ? std::max(counts[i], 0) : 0; }
int table_k1(const int* counts, int i, TableCounts c) { return c == TABLE_WHICH ? counts[i] + 1 : counts[i]; }

/* after the device check: no detection with a pose has an empty model cloud; n_jobs = the poses of the table */
ppf_status table_check_models(const ppf_frame_detection* dets, int n_dets, const int* counts, TableCounts c, const char* who,
                              int* n_jobs) {
  *n_jobs = 0;
  for (int i = 0; i < n_dets; i++) {
    const int n = table_k1(counts, i, c) - table_k0(counts, i, c);
    if (n > 0 && dets[i].model_cloud->n <= 0) return fail(PPF_ERR_INVALID, "%s: detection %d has an empty model cloud", who, i);
    *n_jobs += n;
  }
  return PPF_OK;
}

/* a depth image and its intrinsics: rows x cols > 0, at most INT32_MAX pixels, fx and fy finite, ppx and ppy finite.
 * drawn: something is rendered into an image of this size, so fx and fy must be > 0; otherwise the image is only sampled
 * and they may be negative, not zero.  The texts are those of the two checks this one replaces. */
ppf_status image_check(int rows, int cols, const double* intr, bool drawn, const char* who) {
  if (rows <= 0 || cols <= 0) return fail(PPF_ERR_INVALID, "%s: the %s is %d x %d", who, drawn ? "image" : "depth image", rows, cols);
  if ((long long)rows * cols > 0x7fffffffLL) return fail(PPF_ERR_INVALID, "%s: %d x %d pixels exceed INT32_MAX", who, rows, cols);
  if (!intr) return fail(PPF_ERR_INVALID, drawn ? "%s: intr is NULL" : "%s: a depth image needs intr", who);
  const bool ok = std::isfinite(intr[0]) && std::isfinite(intr[1]) && (drawn ? intr[0] > 0.0 && intr[1] > 0.0 : intr[0] != 0.0 && intr[1] != 0.0);
  if (!ok) return fail(PPF_ERR_INVALID, "%s: fx and fy must be finite and %s", who, drawn ? "> 0" : "non-zero");
  if (!std::isfinite(intr[2]) || !std::isfinite(intr[3])) return fail(PPF_ERR_INVALID, "%s: ppx and ppy must be finite", who);
  return PPF_OK;
}

/* the render jobs of the table in (i, k) order, every model row, labelled as `label` says.  Returns the largest model
 * cloud (at least 1), what sizes a launch over the jobs' rows. */
int table_render_jobs(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* counts, TableCounts c, int top,
                      JobLabel label, std::vector<RndJob>& jobs) {
  int max_n = 1;
  for (int i = 0; i < n_dets; i++)
    for (int k = table_k0(counts, i, c); k < table_k1(counts, i, c); k++) {
      RndJob j;
      std::memcpy(j.T, poses[(size_t)i * top + k].pose, sizeof(j.T));
      j.model = dets[i].model_cloud->rows.p;
      j.n = dets[i].model_cloud->n;
      j.label = label == LABEL_FLAT ? i * top + k : i;
      max_n = std::max(max_n, j.n);
      jobs.push_back(j);
    }
  return max_n;
}

ppf_status frame_upload_depth(FrameRun& fr, const float* depth, int rows, int cols, float** d_depth) {
  const size_t npx = (size_t)rows * cols;
  ppf_status s = fr.get(npx, d_depth);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(*d_depth, depth, npx * sizeof(float), hipMemcpyHostToDevice));
  return PPF_OK;
}

/* every score row zero and every best[i] = -1, where the size arguments let us reach them */
void table_clear_scores(int n_dets, int top, ppf_pose_score* scores, int* best) {
  if (!table_sized(n_dets, top)) return;
  if (scores) std::memset(scores, 0, (size_t)n_dets * top * sizeof(ppf_pose_score));
  if (best) std::fill(best, best + n_dets, -1);
}

/* empty images (depth 0, label -1), where the size arguments let us reach them */
void table_clear_images(int rows, int cols, float* depth_out, int32_t* label_out) {
  if (rows <= 0 || cols <= 0 || (long long)rows * cols > 0x7fffffffLL) return;
  const size_t npx = (size_t)rows * cols;
  if (depth_out) std::memset(depth_out, 0, npx * sizeof(float));
  if (label_out) std::fill(label_out, label_out + npx, -1);
}

/* dev[j] = the score row of job j, (i, k) order -> scores[i * top + k]; best[i] = the first row of the highest score */
void table_scatter_scores(const std::vector<ppf_pose_score>& dev, int n_dets, const int* n_poses, int top, ppf_pose_score* scores, int* best) {
  size_t j = 0;
  for (int i = 0; i < n_dets; i++)
    for (int k = 0; k < n_poses[i]; k++) {
      scores[(size_t)i * top + k] = dev[j++];
      if (best[i] < 0 || scores[(size_t)i * top + k].score > scores[(size_t)i * top + best[i]].score) best[i] = k;
    }
}

}  // namespace
