/*
 * ppf_prep_host.h — host side of the stages that produce the matcher's input (row N4): the device-resident ppf_cloud,
 * the segmented stage functions (crop, voxel grid, outlier removal, normals, edges, to-Mat over K segments of one
 * concatenated cloud; frame_knn and frame_compact beneath them), the C-ABI entry points ppf_cloud_* and
 * ppf_prep_* (each stage function with one segment) and the resident ppf_match_clouds / ppf_icp_refine_clouds.
 * ppf_prep_frame chains the same functions for all boxes of a frame (ppf_frame_host.h).  Kernels: ppf_prep_kernels.h.
 * Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, FRAME_LAUNCH, frame_scan, frame_sort, grid_for; one translation
 * unit: shares DevBuf, fail(), HIPCHK and the scan and radix-sort kernels).
 */
/* ============================================================================================ */
/* Pre-processing stages (row N4; kernels in ppf_prep_kernels.h)                                  */
/* ============================================================================================ */
struct ppf_cloud {
  DevBuf<float> rows; /* n x 6: x y z nx ny nz */
  DevBuf<float> curv; /* n */
  int n = 0;
  /* the outputs of ppf_prep_frame share one block: rows.p / curv.p then point into it and do not own it; the last
   * cloud released returns it to the block cache */
  std::shared_ptr<DevBuf<float>> shared;
  ppf_cloud() = default;
  ppf_cloud(const ppf_cloud&) = delete;
  ppf_cloud& operator=(const ppf_cloud&) = delete;
  ~ppf_cloud() {
    if (shared) { rows.p = nullptr; curv.p = nullptr; }
  }
};

/* cells per axis of the neighbour-search grid = sqrt(n) / PPF_KNN_GDIV.  Swept in round 4 (normals(30) / SOR(50) on the reference's
 * 10,395 / 11,369-point clouds and on 50,000 points): 6.0: 0.280 / 0.359 / 1.27 / 1.39 ms; 4.5: 0.255 / 0.350 / 1.09 / 1.22;
 * 4.0: 0.252 / 0.353 / 1.07 / 1.19; 3.0: 0.253 / 0.382 / 1.01 / 1.17; 2.0: 0.330 / 0.530 -- finer cells, fewer candidates per
 * step of the merge network, until the cube has to grow a second time for most queries.  The result does not depend on it. */
#ifndef PPF_KNN_GDIV
#define PPF_KNN_GDIV 4.0
#endif
namespace {

ppf_status cloud_reserve(ppf_cloud* c, int n) {
  c->n = n;
  HIPCHK(c->rows.reserve((size_t)std::max(n, 1) * 6));
  HIPCHK(c->curv.reserve((size_t)std::max(n, 1)));
  return PPF_OK;
}
ppf_status cloud_alloc(std::unique_ptr<ppf_cloud>& c, int n) {
  c.reset(new ppf_cloud());
  return cloud_reserve(c.get(), n);
}

ppf_status prep_check(const char* who, const ppf_cloud* in, ppf_cloud** out) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!in) return fail(PPF_ERR_INVALID, "%s: cloud is NULL", who);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  return PPF_OK;
}

/* SceneCropping's five half-spaces for box {x, y, w, h} from the HOST depth image (CloudProcessing.h:263-339): +-30 px,
 * mean corner depth, corners pushed 0.15 m back.  false: the box lies outside the image.  ppf_prep_crop and
 * ppf_prep_frame both call it. */
bool crop_planes(const int* box_xywh, const float* depth, int depth_rows, int depth_cols, const double* intr, CropPlanes* out) {
  double left = box_xywh[0] - 30; if (left < 0) left = 0;
  double top = box_xywh[1] - 30; if (top < 0) top = 0;
  double right = box_xywh[0] + box_xywh[2] + 30; if (right >= depth_cols) right = depth_cols - 1;
  double bottom = box_xywh[1] + box_xywh[3] + 30; if (bottom >= depth_rows) bottom = depth_rows - 1;
  const int il = (int)left, it = (int)top, ir = (int)right, ib = (int)bottom;
  if (il < 0 || it < 0 || ir >= depth_cols || ib >= depth_rows || il > ir || it > ib) return false;
  const float d1 = depth[(size_t)it * depth_cols + il], d2 = depth[(size_t)it * depth_cols + ir],
              d3 = depth[(size_t)ib * depth_cols + il], d4 = depth[(size_t)ib * depth_cols + ir];
  const float davg = (d1 + d2 + d3 + d4) / 4;
  const double fx = intr[0], fy = intr[1], ppx = intr[2], ppy = intr[3];
  auto back_project = [&](int u, int v, float* o) { /* Camera::back_projection_bbox, Camera.h:50-61 */
    o[0] = (float)((double)((float)((double)u - ppx) * davg) / fx);
    o[1] = (float)((double)((float)((double)v - ppy) * davg) / fy);
    o[2] = (float)((double)davg + 0.15); /* corners pushed 0.15 m back, :292-295 */
  };
  float c[4][3];
  back_project(il, it, c[0]); back_project(il, ib, c[1]); back_project(ir, it, c[2]); back_project(ir, ib, c[3]);
  CropPlanes& pl = *out;
  pl.z_base = c[0][2];
  const double ctr[3] = {((double)c[0][0] + c[1][0] + c[2][0] + c[3][0]) / 4, ((double)c[0][1] + c[1][1] + c[2][1] + c[3][1]) / 4, (double)pl.z_base};
  const int face[4][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}};
  for (int f = 0; f < 4; f++) {
    const float* a = c[face[f][0]]; const float* b = c[face[f][1]];
    pl.n[f][0] = (double)a[1] * b[2] - (double)a[2] * b[1];
    pl.n[f][1] = (double)a[2] * b[0] - (double)a[0] * b[2];
    pl.n[f][2] = (double)a[0] * b[1] - (double)a[1] * b[0];
    const double sgn = pl.n[f][0] * ctr[0] + pl.n[f][1] * ctr[1] + pl.n[f][2] * ctr[2];
    if (sgn < 0) { pl.n[f][0] = -pl.n[f][0]; pl.n[f][1] = -pl.n[f][1]; pl.n[f][2] = -pl.n[f][2]; }
  }
  return true;
}

/* ---- the segmented stages (FrameRun, frame_scan and frame_sort: ppf_stage_host.h) ------------------------------- */
/* by a 32-bit key, then by segment (skey[row], below 256): a segment's rows end up together, in key order, equal keys in row
 * order.  Five passes and one gather */
ppf_status frame_sort_segmented(FrameRun& fr, uint32_t*& ka, uint32_t*& va, uint32_t*& kb, uint32_t*& vb, int n, uint32_t* hist,
                                uint32_t* offs, const uint32_t* skey) {
  static const int shifts[5] = {0, 8, 16, 24, 0};
  ppf_status s;
  if ((s = frame_sort(fr, ka, va, kb, vb, n, hist, offs, shifts, 4)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_gather_u32, grid_for(n, 256), dim3(256), skey, va, n, ka);
  return frame_sort(fr, ka, va, kb, vb, n, hist, offs, shifts + 4, 1);
}

/* a segmented cloud on the device: K segments, contiguous and in order, in the first rows of `cap` (>= their total);
 * the table {off, n} lives on the device, nb[s] is what the host knows: an upper bound of segment s's size */
struct SegCloud {
  const float* rows = nullptr; /* cap x 6 */
  const float* curv = nullptr; /* cap */
  int cap = 0;
  const FrameSeg* seg = nullptr;
  int K = 0;
  std::vector<uint32_t> nb;
};

/* where a stage writes its n result rows: scratch of the run, or the fresh cloud `own` that the caller hands out */
ppf_status frame_rows(FrameRun& fr, ppf_cloud* own, int n, float** rows, float** curv) {
  if (!own) return fr.get((size_t)n * 6, rows, n, curv);
  const ppf_status s = cloud_reserve(own, n);
  if (s != PPF_OK) return s;
  *rows = own->rows.p;
  *curv = own->curv.p;
  return PPF_OK;
}

/* SceneCropping of n unsegmented rows for K boxes: flags (box, point) -> one scan -> box-major ordered gather.  One
 * read-back: the cropped total (out->cap) */
ppf_status frame_crop(FrameRun& fr, const float* rows, const float* curv, int n, const CropPlanes* h_planes, int K, ppf_cloud* own,
                      SegCloud* out) {
  CropPlanes* planes;
  uint32_t *cflags, *cpos;
  FrameSeg* seg_c;
  ppf_status s = fr.get(K, &planes, (size_t)K * n + 1, &cflags, (size_t)K * n + 1, &cpos, K, &seg_c);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(planes, h_planes, (size_t)K * sizeof(CropPlanes), hipMemcpyHostToDevice));
  FRAME_LAUNCH(fr, k_frame_crop_flags, dim3(grid_for(n, 256).x, K), dim3(256), rows, n, K, planes, cflags);
  HIPCHK(hipGetLastError());
  if ((s = frame_scan(fr, cflags, cpos, (size_t)K * n + 1)) != PPF_OK) return s;
  uint32_t n_crop = 0;
  if ((s = fr.read(&n_crop, cpos + (size_t)K * n, sizeof(uint32_t))) != PPF_OK) return s;
  const int C = (int)n_crop;
  float *crows = nullptr, *ccurv = nullptr;
  if ((C > 0 || own) && (s = frame_rows(fr, own, C, &crows, &ccurv)) != PPF_OK) return s;
  if (C > 0) {
    FRAME_LAUNCH(fr, k_frame_crop_gather, dim3(grid_for(n, 256).x, K), dim3(256), rows, curv, n, cflags, cpos, crows, ccurv, seg_c);
    HIPCHK(hipGetLastError());
  }
  *out = SegCloud{crows, ccurv, C, seg_c, K, std::vector<uint32_t>((size_t)K, n_crop)};
  return PPF_OK;
}

/* Subsampling of a non-empty segmented cloud: per-segment bounds and PCL grid, sort by (segment, cell) in fixed digit
 * passes, runs, one thread per cell.  Non-finite rows take no part.  One read-back: {cells, finite points, overflow
 * box, cells per box}.  *overflow = the first box whose cell index would overflow (then nothing is written), ~0 = none */
ppf_status frame_voxel(FrameRun& fr, const SegCloud& in, double leaf, ppf_cloud* own, SegCloud* out, uint32_t* overflow) {
  const int C = in.cap, K = in.K;
  uint32_t *mm, *fin, *err, *k1, *k2, *v1, *v2, *lkey, *skey, *rflags, *runid, *starts, *d_head;
  VoxelGridDims* dims;
  FrameSeg* seg_v;
  ppf_status s = fr.get((size_t)K * 6, &mm, K, &fin, 1, &err, K, &dims, C, &k1, C, &k2, C, &v1, C, &v2, C, &lkey, C, &skey, (size_t)C + 1, &rflags,
                        (size_t)C + 1, &runid, C, &starts, (size_t)K + 3, &d_head, K, &seg_v);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_bounds, dim3(K), dim3(256), in.rows, in.seg, mm, fin);
  FRAME_LAUNCH(fr, k_frame_voxel_dims, dim3(1), dim3(FRAME_MAX_BOXES), mm, fin, K, 1.0f / (float)leaf, dims, err);
  FRAME_LAUNCH(fr, k_frame_voxel_keys, grid_for(C, 256), dim3(256), in.rows, C, in.seg, K, dims, k1, lkey, skey, v1);
  HIPCHK(hipGetLastError());
  /* by the local cell index (< 2^31; non-finite points ~0), then by the segment */
  const int nblk = (C + RS_BLOCK - 1) / RS_BLOCK;
  uint32_t *hist, *offs;
  s = fr.get((size_t)256 * nblk, &hist, (size_t)256 * nblk, &offs);
  if (s != PPF_OK) return s;
  uint32_t *ka = k1, *va = v1, *kb = k2, *vb = v2;
  if ((s = frame_sort_segmented(fr, ka, va, kb, vb, C, hist, offs, skey)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_voxel_runs, grid_for((size_t)C + 1, 256), dim3(256), va, lkey, skey, C, rflags);
  HIPCHK(hipGetLastError());
  if ((s = frame_scan(fr, rflags, runid, (size_t)C + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_seg_starts, grid_for(C, 256), dim3(256), rflags, runid, C, starts);
  FRAME_LAUNCH(fr, k_frame_voxel_table, dim3(1), dim3(FRAME_MAX_BOXES), fin, K, runid, err, seg_v, d_head);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> head((size_t)K + 3);
  if ((s = fr.read(head.data(), d_head, head.size() * sizeof(uint32_t))) != PPF_OK) return s;
  if ((*overflow = head[2]) != 0xFFFFFFFFu) return PPF_OK;
  const int V = (int)head[0];
  float *vrows, *vcurv;
  if ((s = frame_rows(fr, own, V, &vrows, &vcurv)) != PPF_OK) return s;
  if (V > 0) {
    FRAME_LAUNCH(fr, k_prep_voxel_sum, grid_for(V, 64), dim3(64), in.rows, va, starts, V, (int)head[1], vrows, vcurv);
    HIPCHK(hipGetLastError());
  }
  *out = SegCloud{vrows, vcurv, V, seg_v, K, std::vector<uint32_t>(head.begin() + 3, head.end())};
  return PPF_OK;
}

/* grid cells a segment of up to n points can need (k_frame_knn_grids: at most G + 1 cells per axis) */
size_t frame_knn_cells_bound(uint32_t n) {
  const int G = std::max(1, std::min(128, (int)(std::sqrt((double)n) / PPF_KNN_GDIV)));
  return (size_t)(G + 1) * (G + 1) * (G + 1);
}

/* exact neighbour lists of every row of a segmented cloud: idx / d2 [cap][kstride], segment-local indices, keff[s]
 * entries per row (mode 0: SOR, k = meanK; mode 1: normals); q4 = xyz by row; fin[s] = segment s's finite rows.  A
 * segment that holds a non-finite row is not searched (keff[s] = 0) */
struct FrameKnn {
  float4* q4;
  int *idx, *keff;
  float* d2;
  uint32_t *chunk_base, *fin;
};
ppf_status frame_knn(FrameRun& fr, const SegCloud& in, int mode, int k, int kstride, FrameKnn* out) {
  const int cap = in.cap, K = in.K;
  size_t cells_cap = 0;
  uint32_t nb_max = 0;
  for (int s = 0; s < K; s++) {
    cells_cap += frame_knn_cells_bound(in.nb[s]);
    nb_max = std::max(nb_max, in.nb[s]);
  }
  /* a frame segment is a crop of about 10^4 rows, a single cloud may hold any number: 4,096 rows per workgroup */
  const unsigned bounds_wgs = std::max(1u, std::min(32u, (nb_max + 4095u) / 4096u));
  uint32_t *zeroed, *cell_base, *keys, *cell_begin;
  KnnGrid* grids;
  float4* pts;
  ppf_status s = fr.get(cells_cap + 1 + (size_t)K * 7, &zeroed, K, &grids, K + 1, &cell_base, K, &out->keff, K + 1, &out->chunk_base, cap, &keys,
                        cells_cap + 1, &cell_begin, cap, &pts, cap, &out->q4, (size_t)cap * kstride, &out->idx, (size_t)cap * kstride, &out->d2);
  if (s != PPF_OK) return s;
  /* one fill zeroes the cell counts and, behind them, the bounds that the workgroups of a segment combine */
  uint32_t *const cell_count = zeroed, *const mm = zeroed + cells_cap + 1;
  out->fin = mm + (size_t)K * 6;
  FRAME_LAUNCH(fr, k_frame_fill_u32, grid_for(cells_cap + 1 + (size_t)K * 7, 256), dim3(256), zeroed, cells_cap + 1 + (size_t)K * 7, 0u);
  FRAME_LAUNCH(fr, k_frame_bounds, dim3(K, bounds_wgs), dim3(256), in.rows, in.seg, mm, out->fin);
  FRAME_LAUNCH(fr, k_frame_knn_grids, dim3(1), dim3(FRAME_MAX_BOXES), mm, out->fin, in.seg, K, mode, k, (double)PPF_KNN_GDIV, grids, cell_base,
               out->keff, out->chunk_base);
  FRAME_LAUNCH(fr, k_frame_knn_keys, grid_for(cap, 256), dim3(256), in.rows, cap, in.seg, K, grids, cell_base, out->keff, keys, cell_count);
  HIPCHK(hipGetLastError());
  if ((s = frame_scan(fr, cell_count, cell_begin, cells_cap + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_knn_scatter, grid_for(cap, 256), dim3(256), in.rows, cap, in.seg, K, keys, cell_begin, cell_count, pts, out->q4);
  FRAME_LAUNCH(fr, k_frame_knn, grid_for(cap, KNN_WAVES), dim3(KNN_WAVES * 64), pts, cell_begin, grids, cell_base, in.seg, K, out->keff, cap,
               kstride, out->idx, out->d2);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* segmented ordered compaction of the rows whose flag is set (flags[0..cap]).  Scratch of the run is sized for the
 * worst case; a cloud of its own takes what is kept, at the price of one read-back */
ppf_status frame_compact(FrameRun& fr, const SegCloud& in, const uint32_t* flags, ppf_cloud* own, SegCloud* out) {
  uint32_t* pos;
  FrameSeg* seg_out;
  float *orows, *ocurv;
  ppf_status s = fr.get((size_t)in.cap + 1, &pos, in.K, &seg_out);
  if (s != PPF_OK) return s;
  if ((s = frame_scan(fr, flags, pos, (size_t)in.cap + 1)) != PPF_OK) return s;
  uint32_t kept = (uint32_t)in.cap;
  if (own && (s = fr.read(&kept, pos + in.cap, sizeof(uint32_t))) != PPF_OK) return s;
  if ((s = frame_rows(fr, own, (int)kept, &orows, &ocurv)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_gather, grid_for(in.cap, 256), dim3(256), in.rows, in.curv, in.cap, flags, pos, in.seg, in.K, orows, ocurv, seg_out);
  HIPCHK(hipGetLastError());
  *out = SegCloud{orows, ocurv, (int)kept, seg_out, in.K, in.nb};
  return PPF_OK;
}

/* OutlierProcessing: kNN(meanK + 1) per segment, per-segment chunk sums and threshold, compaction.  *fin (optional) =
 * the finite rows per segment, on the device */
ppf_status frame_outliers(FrameRun& fr, const SegCloud& in, int mean_k, double stddev_mul, ppf_cloud* own, SegCloud* out,
                          const uint32_t** fin) {
  const int V = in.cap, K = in.K, cap_chunks = (V + 63) / 64 + K;
  FrameKnn nn;
  float* dist;
  uint32_t* oflags;
  double *parts, *thr;
  ppf_status s;
  if ((s = frame_knn(fr, in, 0, mean_k, mean_k + 1, &nn)) != PPF_OK) return s;
  s = fr.get(V, &dist, (size_t)cap_chunks * 2, &parts, K, &thr, (size_t)V + 1, &oflags);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_sor_dist, grid_for(V, 256), dim3(256), nn.d2, V, in.seg, K, nn.keff, mean_k, dist);
  FRAME_LAUNCH(fr, k_frame_sor_chunks, grid_for(cap_chunks, 64), dim3(64), dist, cap_chunks, in.seg, K, nn.chunk_base, parts);
  FRAME_LAUNCH(fr, k_frame_sor_threshold, dim3(K), dim3(64), parts, in.seg, nn.chunk_base, stddev_mul, thr);
  FRAME_LAUNCH(fr, k_frame_sor_flags, grid_for((size_t)V + 1, 256), dim3(256), dist, V, in.seg, K, thr, oflags);
  HIPCHK(hipGetLastError());
  if (fin) *fin = nn.fin;
  return frame_compact(fr, in, oflags, own, out);
}

/* NormalEstimation: kNN(min(k, n_s)) per segment, plane fits; the rows keep their places */
ppf_status frame_normals(FrameRun& fr, const SegCloud& in, int k, ppf_cloud* own, SegCloud* out, const uint32_t** fin) {
  FrameKnn nn;
  float *nrows, *ncurv;
  ppf_status s;
  if ((s = frame_knn(fr, in, 1, k, k, &nn)) != PPF_OK) return s;
  if ((s = frame_rows(fr, own, in.cap, &nrows, &ncurv)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_normals, grid_for(in.cap, 64), dim3(64), in.rows, in.cap, in.seg, in.K, nn.idx, k, nn.keff, nn.q4, nrows, ncurv);
  HIPCHK(hipGetLastError());
  if (fin) *fin = nn.fin;
  *out = in;
  out->rows = nrows;
  out->curv = ncurv;
  return PPF_OK;
}

/* EdgeExtraction: segmented compaction on curvature */
ppf_status frame_edges(FrameRun& fr, const SegCloud& in, float curvature_threshold, ppf_cloud* own, SegCloud* out) {
  uint32_t* eflags;
  const ppf_status s = fr.get((size_t)in.cap + 1, &eflags);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_curv_flags, grid_for((size_t)in.cap + 1, 256), dim3(256), in.curv, in.cap, in.seg, in.K, curvature_threshold, eflags);
  HIPCHK(hipGetLastError());
  return frame_compact(fr, in, eflags, own, out);
}

/* PointCloudXYZNormalToMat: rows with the normals re-normalised, the curvature beside them */
ppf_status frame_to_mat(FrameRun& fr, const SegCloud& in, float* out_rows, float* out_curv) {
  FRAME_LAUNCH(fr, k_frame_to_mat, grid_for(in.cap, 256), dim3(256), in.rows, in.curv, in.cap, in.seg, in.K, out_rows, out_curv);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* ---- one cloud = one segment ----------------------------------------------------------------------------------- */
/* the table {0, n} over a handle's rows (a view into a shared block included: only rows.p / curv.p are read) */
ppf_status one_segment(FrameRun& fr, const ppf_cloud* in, SegCloud* c) {
  FrameSeg* seg;
  ppf_status s = fr.get(1, &seg);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_frame_fill_u32, dim3(1), dim3(256), &seg->off, (size_t)1, 0u); /* two fills cost less than a blocking upload */
  FRAME_LAUNCH(fr, k_frame_fill_u32, dim3(1), dim3(256), &seg->n, (size_t)1, (uint32_t)in->n);
  HIPCHK(hipGetLastError());
  *c = SegCloud{in->rows.p, in->curv.p, in->n, seg, 1, std::vector<uint32_t>(1, (uint32_t)in->n)};
  return PPF_OK;
}

/* the segmented search skips a segment that holds non-finite rows; a single cloud reports it.  `finite` is the count the
 * stage's closing wait brought back */
ppf_status prep_all_finite(uint32_t finite, int n) {
  if (finite != (uint32_t)n) return fail(PPF_ERR_INVALID, "neighbour search: the cloud holds non-finite points (crop or voxel-grid it first)");
  return PPF_OK;
}

ppf_status prep_empty(ppf_cloud** out) {
  std::unique_ptr<ppf_cloud> c;
  ppf_status s = cloud_alloc(c, 0);
  if (s == PPF_OK) *out = c.release();
  return s;
}

}  // namespace

extern "C" {

ppf_status ppf_cloud_upload(const float* rows, int n, int stride, int noff, int cols, ppf_cloud** out) {
  if (!out) return fail(PPF_ERR_INVALID, "ppf_cloud_upload: out is NULL");
  *out = nullptr;
  if (!rows || n < 0 || (cols != 3 && cols != 6) || stride < cols || (cols == 6 && bad_layout(stride, noff)))
    return fail(PPF_ERR_INVALID, "ppf_cloud_upload: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_cloud_upload: no HIP device (this engine has no CPU fallback)");
  std::unique_ptr<ppf_cloud> c;
  ppf_status s = cloud_alloc(c, n);
  if (s != PPF_OK) return s;
  if (n) {
    DevBuf<float> raw;
    HIPCHK(raw.reserve((size_t)n * stride));
    HIPCHK(hipMemcpy(raw.p, rows, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
    k_prep_pack<<<grid_for(n, 256), dim3(256)>>>(raw.p, n, stride, noff, cols, c->rows.p, c->curv.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
  }
  *out = c.release();
  return PPF_OK;
}
ppf_status ppf_cloud_set_curvature(ppf_cloud* c, const float* curvature, int n) {
  if (!c || !curvature || n != c->n) return fail(PPF_ERR_INVALID, "ppf_cloud_set_curvature: NULL, or n is not the cloud's row count");
  if (n) HIPCHK(hipMemcpy(c->curv.p, curvature, (size_t)n * sizeof(float), hipMemcpyHostToDevice)); /* after every kernel queued so far */
  return PPF_OK;
}
ppf_status ppf_cloud_release(ppf_cloud* c) {
  if (c) (void)hipDeviceSynchronize(); /* its rows return to the block cache: no kernel may still be reading them */
  delete c;
  return PPF_OK;
}
ppf_status ppf_cloud_size(const ppf_cloud* c, int* n) {
  if (!c || !n) return fail(PPF_ERR_INVALID, "ppf_cloud_size: NULL");
  *n = c->n;
  return PPF_OK;
}
ppf_status ppf_cloud_download(const ppf_cloud* c, float* rows6, float* curvature, int cap_rows) {
  if (!c) return fail(PPF_ERR_INVALID, "ppf_cloud_download: NULL");
  if (cap_rows < c->n) return fail(PPF_ERR_CAPACITY, "ppf_cloud_download: need %d rows, have %d", c->n, cap_rows);
  if (rows6 && c->n) HIPCHK(hipMemcpy(rows6, c->rows.p, (size_t)c->n * 6 * sizeof(float), hipMemcpyDeviceToHost));
  if (curvature && c->n) HIPCHK(hipMemcpy(curvature, c->curv.p, (size_t)c->n * sizeof(float), hipMemcpyDeviceToHost));
  return PPF_OK;
}
ppf_status ppf_cloud_device_rows(const ppf_cloud* c, const float** d_rows6, int* n) {
  if (!c || !d_rows6 || !n) return fail(PPF_ERR_INVALID, "ppf_cloud_device_rows: NULL");
  *d_rows6 = c->rows.p;
  *n = c->n;
  return PPF_OK;
}

/* Each stage below is the one-segment case of the segmented stage above: the table is {0, n} over the handle's rows,
 * scratch comes from a FrameRun, and the last kernel writes into the fresh cloud that is returned. */

/* SceneCropping (CloudProcessing.h:263-339) for one bounding box */
ppf_status ppf_prep_crop(const ppf_cloud* in, const int* box_xywh, const float* depth, int depth_rows, int depth_cols,
                         const double* intr, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_crop", in, out);
  if (s != PPF_OK) return s;
  if (!box_xywh || !depth || !intr || depth_rows <= 0 || depth_cols <= 0) return fail(PPF_ERR_INVALID, "ppf_prep_crop: bad argument");
  CropPlanes pl;
  if (!crop_planes(box_xywh, depth, depth_rows, depth_cols, intr, &pl)) return fail(PPF_ERR_INVALID, "ppf_prep_crop: box outside the depth image");
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud res;
  if ((s = fr.finish("ppf_prep_crop", frame_crop(fr, in->rows.p, in->curv.p, in->n, &pl, 1, c.get(), &res), {})) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

/* Subsampling (:361-380): pcl::VoxelGrid with a cubic leaf */
ppf_status ppf_prep_voxel_grid(const ppf_cloud* in, double leaf, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_voxel_grid", in, out);
  if (s != PPF_OK) return s;
  if (!((float)leaf > 0.f)) return fail(PPF_ERR_INVALID, "ppf_prep_voxel_grid: leaf size must be positive");
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud seg, res;
  auto run = [&]() -> ppf_status {
    uint32_t overflow;
    ppf_status r;
    if ((r = one_segment(fr, in, &seg)) != PPF_OK || (r = frame_voxel(fr, seg, leaf, c.get(), &res, &overflow)) != PPF_OK) return r;
    if (overflow != 0xFFFFFFFFu) return fail(PPF_ERR_INVALID, "ppf_prep_voxel_grid: leaf size is too small for the cloud (index overflow)");
    return PPF_OK;
  };
  if ((s = fr.finish("ppf_prep_voxel_grid", run(), {})) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

/* exact k nearest neighbours of every point (debug / parity surface): idx and d2 are [n][k]; missing = -1 / 0 */
ppf_status ppf_prep_knn(const ppf_cloud* in, int k, int* idx, float* d2) {
  if (!in || !idx || !d2 || k < 1 || k > KNN_MAX_K) return fail(PPF_ERR_INVALID, "ppf_prep_knn: bad argument (k <= %d)", KNN_MAX_K);
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_prep_knn: no HIP device (this engine has no CPU fallback)");
  const int n = in->n, ke = std::min(k, n);
  if (n == 0) return PPF_OK;
  FrameRun fr;
  SegCloud seg;
  FrameKnn nn = {};
  std::vector<int> hi((size_t)n * ke);
  std::vector<float> hd((size_t)n * ke);
  uint32_t finite = 0;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    return r != PPF_OK ? r : frame_knn(fr, seg, 1, k, ke, &nn);
  };
  const ppf_status ran = run(); /* before nn is read */
  ppf_status s = fr.finish("ppf_prep_knn", ran, {{"finite rows", nn.fin, sizeof(finite), &finite},
                                                 {"indices", nn.idx, hi.size() * sizeof(int), hi.data()},
                                                 {"distances", nn.d2, hd.size() * sizeof(float), hd.data()}});
  if (s != PPF_OK || (s = prep_all_finite(finite, n)) != PPF_OK) return s;
  for (int i = 0; i < n; i++)
    for (int m = 0; m < k; m++) {
      idx[(size_t)i * k + m] = m < ke ? hi[(size_t)i * ke + m] : -1;
      d2[(size_t)i * k + m] = m < ke ? hd[(size_t)i * ke + m] : 0.f;
    }
  return PPF_OK;
}

/* OutlierProcessing (:341-360): pcl::StatisticalOutlierRemoval(meanK, stddevMul) */
ppf_status ppf_prep_outlier_removal(const ppf_cloud* in, int mean_k, double stddev_mul, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_outlier_removal", in, out);
  if (s != PPF_OK) return s;
  if (mean_k < 1 || mean_k + 1 > KNN_MAX_K) return fail(PPF_ERR_INVALID, "ppf_prep_outlier_removal: meanK must be in [1, %d]", KNN_MAX_K - 1);
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud seg, res;
  const uint32_t* fin = nullptr;
  uint32_t finite = 0;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    return r != PPF_OK ? r : frame_outliers(fr, seg, mean_k, stddev_mul, c.get(), &res, &fin);
  };
  /* with n <= meanK nothing is measured and every row is kept; the search's launches still run, with k_eff = 0 and no cells */
  const bool searched = in->n > mean_k;
  const ppf_status ran = run(); /* before fin is read */
  s = fr.finish("ppf_prep_outlier_removal", ran, {{"finite rows", fin, sizeof(finite), searched ? &finite : nullptr}});
  if (s != PPF_OK || (searched && (s = prep_all_finite(finite, in->n)) != PPF_OK)) return s;
  *out = c.release();
  return PPF_OK;
}

/* NormalEstimation (:381-405): k nearest neighbours, plane fit, normal towards the camera, curvature */
ppf_status ppf_prep_normals(const ppf_cloud* in, int k, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_normals", in, out);
  if (s != PPF_OK) return s;
  if (k < 1 || k > KNN_MAX_K) return fail(PPF_ERR_INVALID, "ppf_prep_normals: k must be in [1, %d]", KNN_MAX_K);
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud seg, res;
  const uint32_t* fin = nullptr;
  uint32_t finite = 0;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    return r != PPF_OK ? r : frame_normals(fr, seg, k, c.get(), &res, &fin);
  };
  const ppf_status ran = run(); /* before fin is read */
  s = fr.finish("ppf_prep_normals", ran, {{"finite rows", fin, sizeof(finite), &finite}});
  if (s != PPF_OK || (s = prep_all_finite(finite, in->n)) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

/* EdgeExtraction (:406-427): points whose curvature exceeds the threshold */
ppf_status ppf_prep_edges(const ppf_cloud* in, float curvature_threshold, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_edges", in, out);
  if (s != PPF_OK) return s;
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud seg, res;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    return r != PPF_OK ? r : frame_edges(fr, seg, curvature_threshold, c.get(), &res);
  };
  if ((s = fr.finish("ppf_prep_edges", run(), {})) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

/* PointCloudXYZNormalToMat (:163-190): the N x 6 rows the detector consumes, normals re-normalised */
ppf_status ppf_prep_to_mat(const ppf_cloud* in, ppf_cloud** out) {
  ppf_status s = prep_check("ppf_prep_to_mat", in, out);
  if (s != PPF_OK) return s;
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c;
  FrameRun fr;
  SegCloud seg;
  if ((s = cloud_alloc(c, in->n)) != PPF_OK) return s;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    return r != PPF_OK ? r : frame_to_mat(fr, seg, c->rows.p, c->curv.p);
  };
  if ((s = fr.finish("ppf_prep_to_mat", run(), {})) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

/* ---- the PPF calls on device-resident clouds: the whole chain after the detector's boxes without host copies --- */
ppf_status ppf_match_clouds(const ppf_model* m, const ppf_cloud* scene, const ppf_cloud* edge, const ppf_match_params* params,
                            ppf_pose* out, int cap, int* n_out) {
  if (!n_out) return fail(PPF_ERR_INVALID, "ppf_match_clouds: n_out is NULL");
  *n_out = 0;
  if (!scene) return fail(PPF_ERR_INVALID, "ppf_match_clouds: scene is NULL");
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_match_clouds: no HIP device (this engine has no CPU fallback)");
  ppf_status s = check_match_args(m, scene->rows.p, scene->n, 6, 3, edge ? edge->rows.p : nullptr, edge ? edge->n : 0, 6, 3, params);
  if (s != PPF_OK) return s;
  /* a warm context of the model (ppf_match_host.h); the clouds are resident, so nothing is staged.  The stages that made
   * them ran on the default stream and waited for it before returning. */
  HostLoan loan(m);
  if ((s = loan.open()) != PPF_OK) return s;
  if ((s = ppf_workspace_enable_timing(&loan.c->ws, 0)) != PPF_OK) return s;
  s = ppf_match_device(m, &loan.c->ws, scene->rows.p, scene->n, 6, 3, edge ? edge->rows.p : nullptr, edge ? edge->n : 0, 6, 3, params,
                       loan.c->stream);
  if (s == PPF_OK) s = ppf_workspace_results(&loan.c->ws, nullptr, nullptr, 0, nullptr, out, cap, n_out, nullptr);
  loan.ok = s == PPF_OK || s == PPF_ERR_CAPACITY;
  return s;
}

ppf_status ppf_icp_refine_clouds(const ppf_cloud* model, const ppf_cloud* scene, const ppf_icp_params* params, ppf_pose* poses_io,
                                 int n_poses, int* iterations_out) {
  if (!model || !scene) return fail(PPF_ERR_INVALID, "ppf_icp_refine_clouds: cloud is NULL");
  return ppf_icp_refine_device(model->rows.p, model->n, 6, 3, scene->rows.p, scene->n, 6, 3, params, poses_io, n_poses, iterations_out, nullptr);
}

}  // extern "C"
