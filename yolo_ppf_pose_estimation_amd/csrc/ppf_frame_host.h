/*
 * ppf_frame_host.h — host side of ppf_prep_frame: the six preparation stages for every box of a frame in one launch
 * sequence (the reference's CloudProcessor returns one cloud per detection from every stage, CloudProcessing.h:263-427).
 * Kernels: the segmented section of ppf_prep_kernels.h.  Included by ppf_hip.hip after ppf_prep_host.h (ppf_cloud,
 * crop_planes, grid_for).
 *
 * Each stage works on the concatenation of the K boxes' clouds, with a device table {off, n} per segment.  Counts stay
 * on the device; the host reads back three times, the same for every K:
 *   1. after the crop: the cropped total (sizes the voxel grid's buffers)
 *   2. after the voxel grid: cells per box, the finite total and the overflow flag (sizes everything after it, and
 *      fails the call before any output exists)
 *   3. at the end: rows per box and stage, and where each box's rows lie in the shared output block.
 * Scans run a fixed three-level launch sequence and the voxel sort a fixed number of digit passes, so the launch
 * count does not depend on K either.  The one upload (the K crop-plane sets) happens before any device work.
 */
namespace {

/* scratch of one frame call, from the block cache; it lives until the call returns (after the last read-back) */
struct FrameRun {
  int launches = 0, syncs = 0;
  struct Holder {
    virtual ~Holder() {}
  };
  template <class T>
  struct Buf : Holder {
    DevBuf<T> b;
  };
  std::vector<std::unique_ptr<Holder>> keep;
  template <class T>
  ppf_status get(size_t n, T** out) {
    std::unique_ptr<Buf<T>> h(new Buf<T>());
    HIPCHK(h->b.reserve(std::max<size_t>(n, 1)));
    *out = h->b.p;
    keep.push_back(std::move(h));
    return PPF_OK;
  }
  /* a blocking read-back (counted) */
  ppf_status read(void* dst, const void* src, size_t bytes) {
    syncs++;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PPF_OK;
  }
};

#define FRAME_LAUNCH(fr, kern, grid, block, ...) \
  do {                                           \
    kern<<<(grid), (block)>>>(__VA_ARGS__);      \
    (fr).launches++;                             \
  } while (0)

/* exclusive scan of n u32 in five launches whatever n is (device_exclusive_scan picks its launches by n and waits for
 * its scratch; here the scratch lives in `fr`) */
ppf_status frame_scan(FrameRun& fr, const uint32_t* in, uint32_t* out, size_t n) {
  const size_t nb1 = std::max<size_t>((n + 1023) / 1024, 1), nb2 = (nb1 + 1023) / 1024;
  uint32_t *s1, *s1x, *s2, *s2x;
  ppf_status s;
  if ((s = fr.get(nb1, &s1)) != PPF_OK || (s = fr.get(nb1, &s1x)) != PPF_OK || (s = fr.get(nb2, &s2)) != PPF_OK ||
      (s = fr.get(nb2, &s2x)) != PPF_OK)
    return s;
  FRAME_LAUNCH(fr, k_scan_block, dim3((unsigned)nb1), dim3(256), in, out, s1, n);
  FRAME_LAUNCH(fr, k_scan_block, dim3((unsigned)nb2), dim3(256), s1, s1x, s2, nb1);
  FRAME_LAUNCH(fr, k_scan_one, dim3(1), dim3(1024), s2, s2x, nb2);
  FRAME_LAUNCH(fr, k_scan_add, grid_for(nb1, 256), dim3(256), s1x, s2x, nb1);
  FRAME_LAUNCH(fr, k_scan_add, grid_for(n, 256), dim3(256), out, s1x, n);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* grid cells a segment of up to n points can need (cloud_knn's grid: at most G + 1 cells per axis) */
size_t frame_knn_cells_bound(uint32_t n) {
  const int G = std::max(1, std::min(128, (int)(std::sqrt((double)n) / PPF_KNN_GDIV)));
  return (size_t)(G + 1) * (G + 1) * (G + 1);
}

/* exact neighbour lists of every row of a segmented cloud (rows: cap x 6, the segment table on the device; nb[s] = an
 * upper bound of segment s's size): idx / d2 [cap][kstride], segment-local indices, k_eff(s) entries per row
 * (mode 0: SOR, k = meanK; mode 1: normals); q4 = xyz by row */
ppf_status frame_knn(FrameRun& fr, const float* rows, int cap, const FrameSeg* seg, int K, const std::vector<uint32_t>& nb, int mode,
                     int k, int kstride, float4** q4, int** idx, float** d2, int** keff, uint32_t** chunk_base) {
  size_t cells_cap = 0;
  for (int s = 0; s < K; s++) cells_cap += frame_knn_cells_bound(nb[s]);
  uint32_t *mm, *cell_base, *keys, *cell_count, *cell_begin;
  KnnGrid* grids;
  float4* pts;
  ppf_status s;
  if ((s = fr.get((size_t)K * 6, &mm)) != PPF_OK || (s = fr.get(K, &grids)) != PPF_OK || (s = fr.get(K + 1, &cell_base)) != PPF_OK ||
      (s = fr.get(K, keff)) != PPF_OK || (s = fr.get(K + 1, chunk_base)) != PPF_OK || (s = fr.get(cap, &keys)) != PPF_OK ||
      (s = fr.get(cells_cap + 1, &cell_count)) != PPF_OK || (s = fr.get(cells_cap + 1, &cell_begin)) != PPF_OK ||
      (s = fr.get(cap, &pts)) != PPF_OK || (s = fr.get(cap, q4)) != PPF_OK || (s = fr.get((size_t)cap * kstride, idx)) != PPF_OK ||
      (s = fr.get((size_t)cap * kstride, d2)) != PPF_OK)
    return s;
  FRAME_LAUNCH(fr, k_frame_bounds, dim3(K), dim3(256), rows, seg, mm, (uint32_t*)nullptr);
  FRAME_LAUNCH(fr, k_frame_knn_grids, dim3(1), dim3(FRAME_MAX_BOXES), mm, seg, K, mode, k, (double)PPF_KNN_GDIV, grids, cell_base, *keff,
               *chunk_base);
  FRAME_LAUNCH(fr, k_frame_fill_u32, grid_for(cells_cap + 1, 256), dim3(256), cell_count, cells_cap + 1, 0u);
  FRAME_LAUNCH(fr, k_frame_knn_keys, grid_for(cap, 256), dim3(256), rows, cap, seg, K, grids, cell_base, *keff, keys, cell_count);
  HIPCHK(hipGetLastError());
  if ((s = frame_scan(fr, cell_count, cell_begin, cells_cap + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_knn_scatter, grid_for(cap, 256), dim3(256), rows, cap, seg, K, keys, cell_begin, cell_count, pts, *q4);
  FRAME_LAUNCH(fr, k_frame_knn, grid_for(cap, KNN_WAVES), dim3(KNN_WAVES * 64), pts, cell_begin, grids, cell_base, seg, K, *keff, cap,
               kstride, *idx, *d2);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* segmented ordered compaction of rows/curv (cap rows, flags[0..cap]) into out; seg_out = the result's table */
ppf_status frame_compact(FrameRun& fr, const float* rows, const float* curv, int cap, uint32_t* flags, const FrameSeg* seg, int K,
                         float* out_rows, float* out_curv, FrameSeg* seg_out) {
  uint32_t* pos;
  ppf_status s;
  if ((s = fr.get((size_t)cap + 1, &pos)) != PPF_OK) return s;
  if ((s = frame_scan(fr, flags, pos, (size_t)cap + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_gather, grid_for(cap, 256), dim3(256), rows, curv, cap, flags, pos, seg, K, out_rows, out_curv, seg_out);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

ppf_status frame_run(FrameRun& fr, const ppf_cloud* scene, const CropPlanes* h_planes, int K, const ppf_frame_params& prm,
                     ppf_cloud** objects, ppf_cloud** edges, int32_t* stage_rows) {
  ppf_status s;
  const int n = scene->n;
  /* ---- SceneCropping: flags (box, point) -> one scan -> box-major ordered gather ---- */
  CropPlanes* planes;
  uint32_t *cflags, *cpos;
  FrameSeg *seg_c, *seg_v, *seg_o, *seg_e;
  if ((s = fr.get(K, &planes)) != PPF_OK || (s = fr.get((size_t)K * n + 1, &cflags)) != PPF_OK ||
      (s = fr.get((size_t)K * n + 1, &cpos)) != PPF_OK || (s = fr.get(K, &seg_c)) != PPF_OK || (s = fr.get(K, &seg_v)) != PPF_OK ||
      (s = fr.get(K, &seg_o)) != PPF_OK || (s = fr.get(K, &seg_e)) != PPF_OK)
    return s;
  HIPCHK(hipMemcpy(planes, h_planes, (size_t)K * sizeof(CropPlanes), hipMemcpyHostToDevice));
  FRAME_LAUNCH(fr, k_frame_crop_flags, dim3(grid_for(n, 256).x, K), dim3(256), scene->rows.p, n, K, planes, cflags);
  HIPCHK(hipGetLastError());
  if ((s = frame_scan(fr, cflags, cpos, (size_t)K * n + 1)) != PPF_OK) return s;
  uint32_t n_crop = 0;
  if ((s = fr.read(&n_crop, cpos + (size_t)K * n, sizeof(uint32_t))) != PPF_OK) return s; /* host sync 1 */
  std::vector<uint32_t> rep((size_t)K * 6, 0u);
  const int C = (int)n_crop;
  float *crows, *ccurv;
  if (C > 0) {
    if ((s = fr.get((size_t)C * 6, &crows)) != PPF_OK || (s = fr.get(C, &ccurv)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_frame_crop_gather, dim3(grid_for(n, 256).x, K), dim3(256), scene->rows.p, scene->curv.p, n, cflags, cpos, crows,
                 ccurv, seg_c);
    HIPCHK(hipGetLastError());
  }
  /* ---- Subsampling: per-segment bounds and PCL grid, sort by (segment, cell) in fixed digit passes, runs ---- */
  std::vector<uint32_t> head((size_t)K + 3, 0u); /* {cells, finite points, overflow box, cells per box[K]} */
  uint32_t *vals_sorted = nullptr, *starts = nullptr;
  if (C > 0) {
    uint32_t *mm, *fin, *err, *k1, *k2, *v1, *v2, *lkey, *skey, *rflags, *runid, *out;
    VoxelGridDims* dims;
    if ((s = fr.get((size_t)K * 6, &mm)) != PPF_OK || (s = fr.get(K, &fin)) != PPF_OK || (s = fr.get(1, &err)) != PPF_OK ||
        (s = fr.get(K, &dims)) != PPF_OK || (s = fr.get(C, &k1)) != PPF_OK || (s = fr.get(C, &k2)) != PPF_OK ||
        (s = fr.get(C, &v1)) != PPF_OK || (s = fr.get(C, &v2)) != PPF_OK || (s = fr.get(C, &lkey)) != PPF_OK ||
        (s = fr.get(C, &skey)) != PPF_OK || (s = fr.get((size_t)C + 1, &rflags)) != PPF_OK || (s = fr.get((size_t)C + 1, &runid)) != PPF_OK ||
        (s = fr.get(C, &starts)) != PPF_OK || (s = fr.get((size_t)K + 3, &out)) != PPF_OK)
      return s;
    FRAME_LAUNCH(fr, k_frame_bounds, dim3(K), dim3(256), crows, seg_c, mm, fin);
    FRAME_LAUNCH(fr, k_frame_voxel_dims, dim3(1), dim3(FRAME_MAX_BOXES), mm, fin, K, 1.0f / (float)prm.leaf, dims, err);
    FRAME_LAUNCH(fr, k_frame_voxel_keys, grid_for(C, 256), dim3(256), crows, C, seg_c, K, dims, k1, lkey, skey, v1);
    HIPCHK(hipGetLastError());
    /* stable LSD passes: the local cell index (< 2^31; non-finite points ~0), then the segment */
    const int nblk = (C + RS_BLOCK - 1) / RS_BLOCK;
    uint32_t *hist, *offs;
    if ((s = fr.get((size_t)256 * nblk, &hist)) != PPF_OK || (s = fr.get((size_t)256 * nblk, &offs)) != PPF_OK) return s;
    uint32_t *ka = k1, *va = v1, *kb = k2, *vb = v2;
    for (int pass = 0; pass < 5; pass++) {
      const int shift = pass < 4 ? pass * 8 : 0;
      if (pass == 4) FRAME_LAUNCH(fr, k_frame_gather_u32, grid_for(C, 256), dim3(256), skey, va, C, ka);
      FRAME_LAUNCH(fr, k_rs_hist, dim3(nblk), dim3(RS_BLOCK), ka, C, shift, nblk, hist);
      HIPCHK(hipGetLastError());
      if ((s = frame_scan(fr, hist, offs, (size_t)256 * nblk)) != PPF_OK) return s;
      FRAME_LAUNCH(fr, k_rs_scatter, dim3(nblk), dim3(RS_BLOCK), ka, va, C, shift, nblk, offs, kb, vb);
      HIPCHK(hipGetLastError());
      std::swap(ka, kb); std::swap(va, vb);
    }
    vals_sorted = va;
    FRAME_LAUNCH(fr, k_frame_voxel_runs, grid_for((size_t)C + 1, 256), dim3(256), va, lkey, skey, C, rflags);
    HIPCHK(hipGetLastError());
    if ((s = frame_scan(fr, rflags, runid, (size_t)C + 1)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_seg_starts, grid_for(C, 256), dim3(256), rflags, runid, C, starts);
    FRAME_LAUNCH(fr, k_frame_voxel_table, dim3(1), dim3(FRAME_MAX_BOXES), fin, K, runid, err, seg_v, out);
    HIPCHK(hipGetLastError());
    if ((s = fr.read(head.data(), out, head.size() * sizeof(uint32_t))) != PPF_OK) return s; /* host sync 2 */
    if (head[2] != 0xFFFFFFFFu)
      return fail(PPF_ERR_INVALID, "ppf_prep_frame: box %u: leaf size is too small for the cloud (index overflow)", head[2]);
  }
  const int V = (int)head[0];
  std::vector<uint32_t> n_vox(head.begin() + 3, head.end());
  std::shared_ptr<DevBuf<float>> blk;
  if (V > 0) {
    float *vrows, *vcurv;
    if ((s = fr.get((size_t)V * 6, &vrows)) != PPF_OK || (s = fr.get(V, &vcurv)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_prep_voxel_sum, grid_for(V, 64), dim3(64), crows, vals_sorted, starts, V, (int)head[1], vrows, vcurv);
    HIPCHK(hipGetLastError());
    /* ---- OutlierProcessing: kNN(meanK + 1) per segment, per-segment chunk sums and threshold, compaction ---- */
    float4* q4;
    int *idx, *keff;
    float *d2, *dist, *orows, *ocurv;
    uint32_t *chunk_base, *oflags;
    double *parts, *thr;
    const int mk = prm.mean_k, cap_chunks = (V + 63) / 64 + K;
    if ((s = frame_knn(fr, vrows, V, seg_v, K, n_vox, 0, mk, mk + 1, &q4, &idx, &d2, &keff, &chunk_base)) != PPF_OK) return s;
    if ((s = fr.get(V, &dist)) != PPF_OK || (s = fr.get((size_t)cap_chunks * 2, &parts)) != PPF_OK || (s = fr.get(K, &thr)) != PPF_OK ||
        (s = fr.get((size_t)V + 1, &oflags)) != PPF_OK || (s = fr.get((size_t)V * 6, &orows)) != PPF_OK || (s = fr.get(V, &ocurv)) != PPF_OK)
      return s;
    FRAME_LAUNCH(fr, k_frame_sor_dist, grid_for(V, 256), dim3(256), d2, V, seg_v, K, mk, dist);
    FRAME_LAUNCH(fr, k_frame_sor_chunks, grid_for(cap_chunks, 64), dim3(64), dist, cap_chunks, seg_v, K, chunk_base, parts);
    FRAME_LAUNCH(fr, k_frame_sor_threshold, dim3(K), dim3(64), parts, seg_v, chunk_base, prm.stddev_mul, thr);
    FRAME_LAUNCH(fr, k_frame_sor_flags, grid_for((size_t)V + 1, 256), dim3(256), dist, V, seg_v, K, thr, oflags);
    HIPCHK(hipGetLastError());
    if ((s = frame_compact(fr, vrows, vcurv, V, oflags, seg_v, K, orows, ocurv, seg_o)) != PPF_OK) return s;
    /* ---- NormalEstimation: kNN(min(k, n_s)) per segment, plane fits ---- */
    const int nk = prm.normal_k;
    float4* q4n;
    int *idxn, *keffn;
    float *d2n, *nrows, *ncurv, *erows, *ecurv;
    uint32_t *chunk_unused, *eflags;
    if ((s = frame_knn(fr, orows, V, seg_o, K, n_vox, 1, nk, nk, &q4n, &idxn, &d2n, &keffn, &chunk_unused)) != PPF_OK) return s;
    if ((s = fr.get((size_t)V * 6, &nrows)) != PPF_OK || (s = fr.get(V, &ncurv)) != PPF_OK || (s = fr.get((size_t)V + 1, &eflags)) != PPF_OK ||
        (s = fr.get((size_t)V * 6, &erows)) != PPF_OK || (s = fr.get(V, &ecurv)) != PPF_OK)
      return s;
    FRAME_LAUNCH(fr, k_frame_normals, grid_for(V, 64), dim3(64), orows, V, seg_o, K, idxn, nk, keffn, q4n, nrows, ncurv);
    /* ---- EdgeExtraction: segmented compaction on curvature ---- */
    FRAME_LAUNCH(fr, k_frame_curv_flags, grid_for((size_t)V + 1, 256), dim3(256), ncurv, V, seg_o, K, prm.curvature_threshold, eflags);
    HIPCHK(hipGetLastError());
    if ((s = frame_compact(fr, nrows, ncurv, V, eflags, seg_o, K, erows, ecurv, seg_e)) != PPF_OK) return s;
    /* ---- PointCloudXYZNormalToMat into the one output block: [object rows | object curvature | edge rows | edge curvature] ---- */
    blk.reset(new DevBuf<float>());
    HIPCHK(blk->reserve((size_t)V * 14));
    float* const b = blk->p;
    FRAME_LAUNCH(fr, k_frame_to_mat, grid_for(V, 256), dim3(256), nrows, ncurv, V, seg_o, K, b, b + (size_t)V * 6);
    FRAME_LAUNCH(fr, k_frame_to_mat, grid_for(V, 256), dim3(256), erows, ecurv, V, seg_e, K, b + (size_t)V * 7, b + (size_t)V * 13);
    uint32_t* d_rep;
    if ((s = fr.get((size_t)K * 6, &d_rep)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_frame_report, dim3(1), dim3(FRAME_MAX_BOXES), seg_c, seg_v, seg_o, seg_e, K, d_rep);
    HIPCHK(hipGetLastError());
    if ((s = fr.read(rep.data(), d_rep, rep.size() * sizeof(uint32_t))) != PPF_OK) return s; /* host sync 3 */
  } else if (C > 0) {
    /* every box lost all its points in the voxel grid: its crop counts are the only non-zero numbers */
    uint32_t* d_rep;
    if ((s = fr.get((size_t)K * 6, &d_rep)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_frame_report, dim3(1), dim3(FRAME_MAX_BOXES), seg_c, seg_c, seg_c, seg_c, K, d_rep);
    HIPCHK(hipGetLastError());
    if ((s = fr.read(rep.data(), d_rep, rep.size() * sizeof(uint32_t))) != PPF_OK) return s;
    for (int b = 0; b < K; b++) for (int c = 1; c < 6; c++) rep[(size_t)b * 6 + c] = 0;
  }
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
    stats->n_launches = fr.launches;
    stats->n_host_syncs = fr.syncs;
    stats->ms_wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return s;
}

}  // extern "C"
