/*
 * ppf_frame_host.h — ppf_prep_frame: the six preparation stages for every box of a frame in one launch sequence (the
 * reference's CloudProcessor returns one cloud per detection from every stage, CloudProcessing.h:263-427).  It is the
 * chain of the segmented stage functions of ppf_prep_host.h (frame_crop ... frame_to_mat; the per-cloud ppf_prep_*
 * entries are the same functions with one segment).  Kernels: ppf_prep_kernels.h.  Included by ppf_hip.hip after
 * ppf_stage_host.h (FrameRun) and ppf_prep_host.h.
 *
 * Each stage works on the concatenation of the K boxes' clouds, with a device table {off, n} per segment.  Counts stay
 * on the device; the host reads back three times, the same for every K (boxes that crop nothing: the first, and the end's
 * wait with nothing to read):
 *   1. after the crop: the cropped total (sizes the voxel grid's buffers)
 *   2. after the voxel grid: cells per box, the finite total and the overflow flag (sizes everything after it, and
 *      fails the call before any output exists)
 *   3. at the end (FrameRun::finish): rows per box and stage, and where each box's rows lie in the shared output block.
 * Scans run a fixed three-level launch sequence and the voxel sort a fixed number of digit passes, so the launch
 * count does not depend on K either.  The one upload (the K crop-plane sets) happens before any device work.
 */
namespace {

ppf_status frame_run(FrameRun& fr, const ppf_cloud* scene, const CropPlanes* h_planes, int K, const ppf_frame_params& prm,
                     ppf_cloud** objects, ppf_cloud** edges, int32_t* stage_rows) {
  SegCloud crop, vox, sor, nrm, edge;
  std::vector<uint32_t> rep((size_t)K * 6, 0u);
  uint32_t* d_rep = nullptr;
  std::shared_ptr<DevBuf<float>> blk;
  int V = 0;
  auto run = [&]() -> ppf_status {
    ppf_status s;
    if ((s = frame_crop(fr, scene->rows.p, scene->curv.p, scene->n, h_planes, K, nullptr, &crop)) != PPF_OK) return s; /* host sync 1 */
    if (crop.cap == 0) return PPF_OK;
    uint32_t overflow;
    if ((s = frame_voxel(fr, crop, prm.leaf, nullptr, &vox, &overflow)) != PPF_OK) return s; /* host sync 2 */
    if (overflow != 0xFFFFFFFFu)
      return fail(PPF_ERR_INVALID, "ppf_prep_frame: box %u: leaf size is too small for the cloud (index overflow)", overflow);
    V = vox.cap;
    s = fr.get((size_t)K * 6, &d_rep);
    if (s != PPF_OK) return s;
    if (V == 0) {
      /* every box lost all its points in the voxel grid: its crop counts are the only non-zero numbers */
      FRAME_LAUNCH(fr, k_frame_report, dim3(1), dim3(FRAME_MAX_BOXES), crop.seg, crop.seg, crop.seg, crop.seg, K, d_rep);
      HIPCHK(hipGetLastError());
      return PPF_OK;
    }
    if ((s = frame_outliers(fr, vox, prm.mean_k, prm.stddev_mul, nullptr, &sor, nullptr)) != PPF_OK ||
        (s = frame_normals(fr, sor, prm.normal_k, nullptr, &nrm, nullptr)) != PPF_OK ||
        (s = frame_edges(fr, nrm, prm.curvature_threshold, nullptr, &edge)) != PPF_OK)
      return s;
    /* PointCloudXYZNormalToMat into the one output block: [object rows | object curvature | edge rows | edge curvature] */
    blk.reset(new DevBuf<float>());
    HIPCHK(blk->reserve((size_t)V * 14));
    float* const b = blk->p;
    if ((s = frame_to_mat(fr, nrm, b, b + (size_t)V * 6)) != PPF_OK || (s = frame_to_mat(fr, edge, b + (size_t)V * 7, b + (size_t)V * 13)) != PPF_OK)
      return s;
    FRAME_LAUNCH(fr, k_frame_report, dim3(1), dim3(FRAME_MAX_BOXES), crop.seg, vox.seg, sor.seg, edge.seg, K, d_rep);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run(); /* before d_rep is read */
  const ppf_status s = fr.finish("ppf_prep_frame", ran, {{"report", d_rep, rep.size() * sizeof(uint32_t), d_rep ? rep.data() : nullptr}}); /* host sync 3 */
  if (s != PPF_OK) return s;
  if (V == 0)
    for (int b = 0; b < K; b++) for (int c = 1; c < 6; c++) rep[(size_t)b * 6 + c] = 0;
  /* ---- the handles: views into the shared block (none is created before every check has passed) ---- */
  std::vector<std::unique_ptr<ppf_cloud>> obj(K), edg(K);
  for (int b = 0; b < K; b++) {
    const uint32_t* r = &rep[(size_t)b * 6];
    for (int w = 0; w < 2; w++) {
      if (w == 1 && !edges) continue;
      std::unique_ptr<ppf_cloud>& c = w == 0 ? obj[b] : edg[b];
      c.reset(new ppf_cloud());
      c->n = (int)(w == 0 ? r[2] : r[3]);
      if (blk) {
        c->shared = blk;
        const size_t off = w == 0 ? r[4] : r[5];
        c->rows.p = blk->p + (size_t)(w == 0 ? 0 : 7) * V + off * 6;
        c->curv.p = blk->p + (size_t)(w == 0 ? 6 : 13) * V + off;
      } else {
        HIPCHK(c->rows.reserve(6));
        HIPCHK(c->curv.reserve(1));
      }
    }
  }
  for (int b = 0; b < K; b++) {
    objects[b] = obj[b].release();
    if (edges) edges[b] = edg[b].release();
    if (stage_rows)
      for (int c = 0; c < 4; c++) stage_rows[(size_t)b * 4 + c] = (int32_t)rep[(size_t)b * 6 + c];
  }
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_frame_params(ppf_frame_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->leaf = 0.003;
  p->mean_k = 50;
  p->stddev_mul = 1.0;
  p->normal_k = 30;
  p->curvature_threshold = 0.03f;
}

ppf_status ppf_prep_frame(const ppf_cloud* scene, const int* boxes_xywh, int n_boxes, const float* depth, int depth_rows, int depth_cols,
                          const double* intr, const ppf_frame_params* params, ppf_cloud** objects, ppf_cloud** edges, int32_t* stage_rows,
                          ppf_frame_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!objects) return fail(PPF_ERR_INVALID, "ppf_prep_frame: objects is NULL");
  if (n_boxes < 0 || n_boxes > FRAME_MAX_BOXES) return fail(PPF_ERR_INVALID, "ppf_prep_frame: n_boxes must be in [0, %d]", FRAME_MAX_BOXES);
  for (int b = 0; b < n_boxes; b++) {
    objects[b] = nullptr;
    if (edges) edges[b] = nullptr;
  }
  if (!scene || (n_boxes && !boxes_xywh) || !depth || !intr || !params || depth_rows <= 0 || depth_cols <= 0)
    return fail(PPF_ERR_INVALID, "ppf_prep_frame: bad argument (NULL pointer or empty depth image)");
  const ppf_frame_params& prm = *params;
  if (!((float)prm.leaf > 0.f)) return fail(PPF_ERR_INVALID, "ppf_prep_frame: leaf size must be positive");
  if (prm.mean_k < 1 || prm.mean_k + 1 > KNN_MAX_K) return fail(PPF_ERR_INVALID, "ppf_prep_frame: meanK must be in [1, %d]", KNN_MAX_K - 1);
  if (prm.normal_k < 1 || prm.normal_k > KNN_MAX_K) return fail(PPF_ERR_INVALID, "ppf_prep_frame: k must be in [1, %d]", KNN_MAX_K);
  /* the device check comes before any use of the scene handle */
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_prep_frame: no HIP device (this engine has no CPU fallback)");
  std::vector<CropPlanes> planes((size_t)std::max(n_boxes, 1));
  for (int b = 0; b < n_boxes; b++)
    if (!crop_planes(boxes_xywh + (size_t)b * 4, depth, depth_rows, depth_cols, intr, &planes[b]))
      return fail(PPF_ERR_INVALID, "ppf_prep_frame: box %d outside the depth image", b);
  FrameRun fr;
  ppf_status s = n_boxes ? frame_run(fr, scene, planes.data(), n_boxes, prm, objects, edges, stage_rows) : PPF_OK;
  if (stats) {
    stats->n_boxes = n_boxes;
    fr.report(*stats);
    stats->ms_wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return s;
}

}  // extern "C"
