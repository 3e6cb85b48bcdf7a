/*
 * ppf_cluster_host.h — host side of ppf_prep_clusters: the connected blobs of up to 256 plane-free clouds in one pass
 * (DESIGN.md §20).  Kernels: ppf_cluster_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, frame_scan,
 * frame_sort, stage_entry) and ppf_prep_host.h (ppf_cloud, frame_sort_segmented).
 *
 * Per call: one upload of the segment table before any device work, then k_clu_bounds, k_clu_grid, k_clu_keys, the sort by
 * (segment, cell) (five digit passes of seven launches and one gather), k_clu_runs, the scan, k_clu_cells, k_clu_link,
 * k_clu_flatten, k_clu_valid, the ranking's sort (the same five passes), k_clu_rank, k_clu_labels, the gather's sort (three
 * passes), k_clu_gather and k_clu_reduce: 110 launches whatever the clouds hold, none when no cloud has a row.
 * The sequence is cut in three shared pieces (clu_begin, clu_cells, clu_rank) that ppf_prep_regions runs too, around kernels
 * of its own (ppf_region_host.h), inside the same call (clu_run: the table, the run, the one wait, clu_results) and the same
 * entry body (clu_entry).
 * Nothing the device counts (cells, components, clusters) comes to the host before the end: grids are sized for the rows and
 * workgroups past a device-side count leave.  The host waits once, for the cluster heads, the reductions, the counts, the
 * grids and the labels; the outputs are views into one block sized for the input, so nothing is allocated after that wait.
 */
#ifndef PPF_CLUSTER_HOST_H
#define PPF_CLUSTER_HOST_H

namespace {

ppf_status cluster_params_check(const char* who, const ppf_cluster_params* p) {
  if (!p) return fail(PPF_ERR_INVALID, "%s: the params are NULL", who);
  if (!(std::isfinite(p->tolerance) && p->tolerance > 0.f)) return fail(PPF_ERR_INVALID, "%s: tolerance must be finite and > 0", who);
  if (p->min_size < 1) return fail(PPF_ERR_INVALID, "%s: min_size is %d (>= 1)", who, p->min_size);
  if (p->max_size < 0) return fail(PPF_ERR_INVALID, "%s: max_size is %d (>= 0; 0: no bound)", who, p->max_size);
  if (p->max_clusters < 1 || p->max_clusters > PPF_CLUSTER_MAX_CLUSTERS)
    return fail(PPF_ERR_INVALID, "%s: max_clusters is %d (1..%d)", who, p->max_clusters, PPF_CLUSTER_MAX_CLUSTERS);
  if (p->flags) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  return PPF_OK;
}

/* the smallest float tolerance whose grid holds an extent in CLU_AXIS cells */
float cluster_smallest_tolerance(double extent) {
  float t = (float)(extent / ((double)CLU_AXIS * CLU_CELL));
  auto fits = [&](float v) { return v > 0.f && clu_axis_cells(0.0, extent, (double)v * CLU_CELL) <= (uint32_t)CLU_AXIS; };
  while (!fits(t)) t = std::nextafter(t, INFINITY);
  while (fits(std::nextafter(t, 0.f))) t = std::nextafter(t, 0.f);
  return t;
}

/* What ppf_prep_clusters and ppf_prep_regions (ppf_region_host.h) share: the segment table, the scratch, one zeroed block
 * (the bounds, the counts, the cluster heads, the reductions and `extra` words of the entry's own) and the output block.
 * clu_begin runs up to the sort by (segment, cell), the entry its k_*_runs, clu_cells the scan and the table of cells, the
 * entry its link and flatten passes (root[], size[] final), clu_rank the ranking and the gather; after the one wait
 * clu_results reads what came back. */
struct CluWork {
  const char* who;
  int K, MC, n;
  size_t N;
  std::vector<CluSeg> tab;
  CluSeg* d_tab;
  CluGrid* d_grid;
  float4* pts;
  unsigned long long* ckey;
  uint32_t *zero, *lkey, *skey, *ka, *va, *kb, *vb, *hist, *offs, *parent, *size, *root, *flags, *runid, *cstart;
  int32_t *rank, *d_labels;
  size_t z_mm, z_fin, z_cnt, z_head, z_acc, z_extra, z_words;
  dim3 rows_grid, rows1_grid;
  double tol;
};

/* the segment table, before any device work.  w.N == 0 on PPF_OK: no cloud has a row, nothing is to be done */
ppf_status clu_table(CluWork& w, const char* who, const ppf_cloud* const* in, int K, int MC) {
  w.who = who;
  w.K = K;
  w.MC = MC;
  w.tab.resize((size_t)K);
  size_t N = 0;
  for (int i = 0; i < K; i++) {
    w.tab[i] = CluSeg{in[i]->rows.p, in[i]->curv.p, (uint32_t)N, (uint32_t)in[i]->n};
    N += (size_t)in[i]->n;
    if (N >= 0x7fffffffull) return fail(PPF_ERR_INVALID, "%s: the clouds hold more than INT32_MAX rows together", who);
  }
  w.N = N;
  return PPF_OK;
}

/* the scratch, the upload of the table and the launches up to the sort by (segment, cell); w.N > 0 */
template <bool NORMALS>
ppf_status clu_begin(FrameRun& fr, CluWork& w, DevBuf<float>& blk, float tolerance, size_t extra) {
  const int K = w.K, MC = w.MC;
  const size_t N = w.N;
  const int n = w.n = (int)N, nblk = (n + RS_BLOCK - 1) / RS_BLOCK;
  const size_t slots = (size_t)K * MC;
  uint32_t *k1, *k2, *v1, *v2;
  w.z_mm = 0; w.z_fin = w.z_mm + (size_t)K * 6; w.z_cnt = w.z_fin + K; w.z_head = w.z_cnt + (size_t)K * 2; w.z_acc = w.z_head + slots * 2;
  w.z_extra = w.z_acc + slots * CLU_ACC;
  w.z_words = (w.z_extra + extra + 3) & ~(size_t)3;
  const ppf_status s = fr.get(K, &w.d_tab, K, &w.d_grid, w.z_words, &w.zero, N, &w.pts, N + 1, &w.ckey, N, &w.lkey, N, &w.skey, N, &k1, N, &k2, N, &v1,
                              N, &v2, (size_t)256 * nblk, &w.hist, (size_t)256 * nblk, &w.offs, N, &w.parent, N, &w.size, N, &w.root, N + 1, &w.flags,
                              N + 1, &w.runid, N + 2, &w.cstart, N, &w.rank, N, &w.d_labels);
  if (s != PPF_OK) return s;
  HIPCHK(blk.reserve(N * 7)); /* [rows | curvature] */
  HIPCHK(hipMemcpy(w.d_tab, w.tab.data(), w.tab.size() * sizeof(CluSeg), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(w.zero, 0, w.z_words * sizeof(uint32_t), nullptr));
  uint32_t *mm = w.zero + w.z_mm, *fin = w.zero + w.z_fin;

  const dim3 b256(CLU_BLOCK);
  w.rows_grid = grid_for(N, CLU_BLOCK);
  w.rows1_grid = grid_for(N + 1, CLU_BLOCK);
  w.tol = (double)tolerance;
  const double h = w.tol * CLU_CELL;
  FRAME_LAUNCH(fr, k_clu_bounds<NORMALS>, dim3((unsigned)K, CLU_BOUNDS_WGS), b256, w.d_tab, mm, fin);
  FRAME_LAUNCH(fr, k_clu_grid, dim3(1), dim3(FRAME_MAX_BOXES), mm, fin, K, h, w.d_grid);
  FRAME_LAUNCH(fr, k_clu_keys<NORMALS>, w.rows_grid, b256, w.d_tab, K, (uint32_t)N, w.d_grid, w.lkey, k1, w.skey, v1, w.parent, w.size);
  HIPCHK(hipGetLastError());
  w.ka = k1; w.va = v1; w.kb = k2; w.vb = v2;
  return frame_sort_segmented(fr, w.ka, w.va, w.kb, w.vb, n, w.hist, w.offs, w.skey);
}

/* after the entry's k_*_runs (w.va: the sorted order; flags): the scan of the run starts and the table of occupied cells */
ppf_status clu_cells(FrameRun& fr, CluWork& w) {
  ppf_status s;
  if ((s = frame_scan(fr, w.flags, w.runid, w.N + 1)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_clu_cells, w.rows1_grid, dim3(CLU_BLOCK), (uint32_t)w.N, w.va, w.lkey, w.skey, w.flags, w.runid, w.ckey, w.cstart);
  return PPF_OK;
}

/* root[] and size[] are final: the ranking, the labels, the gather into blk and the reductions */
ppf_status clu_rank(FrameRun& fr, CluWork& w, DevBuf<float>& blk, int min_size, int max_size, const double* intr, int image_rows,
                    int image_cols) {
  const int K = w.K, MC = w.MC, n = w.n;
  const size_t N = w.N;
  CluSeg* d_tab = w.d_tab;
  uint32_t *skey = w.skey, *hist = w.hist, *offs = w.offs, *size = w.size, *root = w.root;
  uint32_t *&ka = w.ka, *&va = w.va, *&kb = w.kb, *&vb = w.vb;
  int32_t *rank = w.rank, *d_labels = w.d_labels;
  uint32_t *cnt = w.zero + w.z_cnt, *acc = w.zero + w.z_acc;
  int32_t* head = reinterpret_cast<int32_t*>(w.zero + w.z_head);
  const dim3 b256(CLU_BLOCK), rows_grid = w.rows_grid;
  CluIntr cam = {0.0, 0.0, 0.0, 0.0, image_rows, image_cols, intr ? 1 : 0};
  if (intr) { cam.fx = intr[0]; cam.fy = intr[1]; cam.ppx = intr[2]; cam.ppy = intr[3]; }
  ppf_status s;

  FRAME_LAUNCH(fr, k_clu_valid, rows_grid, b256, d_tab, K, (uint32_t)N, root, size, (uint32_t)min_size, (uint32_t)max_size, ka, va, cnt);
  HIPCHK(hipGetLastError());
  if ((s = frame_sort_segmented(fr, ka, va, kb, vb, n, hist, offs, skey)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_clu_rank, rows_grid, b256, d_tab, K, (uint32_t)N, va, cnt, size, MC, rank, head);
  FRAME_LAUNCH(fr, k_clu_labels, rows_grid, b256, (uint32_t)N, skey, root, rank, d_labels, ka, va);
  HIPCHK(hipGetLastError());
  static const int shifts3[3] = {0, 8, 16};
  if ((s = frame_sort(fr, ka, va, kb, vb, n, hist, offs, shifts3, 3)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_clu_gather, rows_grid, b256, d_tab, (uint32_t)N, ka, va, blk.p, blk.p + N * 6);
  FRAME_LAUNCH(fr, k_clu_reduce, rows_grid, b256, d_tab, (uint32_t)N, ka, va, cam, MC, acc);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* after the one wait: z is the zeroed block and grid the grids as the device left them, lab the labels when any were asked
 * for.  counts: [K][stride] = {output, valid, all, then the entry's `extra` words per cloud} */
ppf_status clu_results(const CluWork& w, const std::vector<uint32_t>& z, const std::vector<CluGrid>& grid, const std::vector<int32_t>& lab,
                       const std::shared_ptr<DevBuf<float>>& blk, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts, int stride,
                       int32_t* const* labels) {
  const char* who = w.who;
  const int K = w.K, MC = w.MC;
  const size_t N = w.N, slots = (size_t)K * MC, z_mm = w.z_mm, z_cnt = w.z_cnt, z_head = w.z_head, z_acc = w.z_acc;
  const std::vector<CluSeg>& tab = w.tab;
  const bool want_labels = !lab.empty();
  for (int i = 0; i < K; i++) {
    if (grid[i].ok) continue;
    const uint32_t* m = &z[z_mm + (size_t)i * 6];
    double ext = 0.0;
    for (int k = 0; k < 3; k++) ext = std::max(ext, (double)ordered_to_float(m[3 + k]) - (double)ordered_to_float(~m[k]));
    return fail(PPF_ERR_INVALID, "%s: in[%d] spans %g m, %u cells of its grid on an axis (at most %d); the smallest tolerance that fits is %.9g",
                who, i, ext, std::max(grid[i].cells[0], std::max(grid[i].cells[1], grid[i].cells[2])), CLU_AXIS,
                (double)cluster_smallest_tolerance(ext));
  }
  std::vector<std::unique_ptr<ppf_cloud>> res(slots);
  size_t at = 0; /* the clusters lie in the block one after the other, in (cloud, rank) order */
  for (int i = 0; i < K; i++) {
    const uint32_t valid = z[z_cnt + (size_t)i * 2], all = z[z_cnt + (size_t)i * 2 + 1], shown = std::min(valid, (uint32_t)MC);
    counts[i * stride] = (int32_t)shown;
    counts[i * stride + 1] = (int32_t)valid;
    counts[i * stride + 2] = (int32_t)all;
    for (int k = 3; k < stride; k++) counts[i * stride + k] = (int32_t)z[w.z_extra + (size_t)i * (stride - 3) + (k - 3)];
    for (uint32_t r = 0; r < shown; r++) {
      const size_t slot = (size_t)i * MC + r;
      ppf_cluster_info& ci = info[slot];
      const uint32_t* a = &z[z_acc + slot * CLU_ACC];
      ci.n_rows = (int32_t)z[z_head + slot * 2];
      ci.first_row = (int32_t)z[z_head + slot * 2 + 1];
      for (int k = 0; k < 3; k++) {
        ci.lo[k] = ordered_to_float(~a[k]);
        ci.hi[k] = ordered_to_float(a[3 + k]);
      }
      if (a[7]) { /* a row with z > 0 gave a pixel */
        const int32_t u0 = (int32_t)~a[6], u1 = (int32_t)a[7] - 1, v0 = (int32_t)~a[8], v1p = (int32_t)a[9] - 1;
        ci.box_xywh[0] = u0; ci.box_xywh[1] = v0; ci.box_xywh[2] = u1 - u0; ci.box_xywh[3] = v1p - v0;
      }
      res[slot].reset(new ppf_cloud());
      res[slot]->n = ci.n_rows;
      res[slot]->shared = blk;
      res[slot]->rows.p = blk->p + at * 6;
      res[slot]->curv.p = blk->p + N * 6 + at;
      at += (size_t)ci.n_rows;
    }
    if (want_labels && labels[i] && tab[i].n) std::memcpy(labels[i], lab.data() + tab[i].off, (size_t)tab[i].n * sizeof(int32_t));
  }
  for (size_t k = 0; k < slots; k++) out[k] = res[k].release();
  return PPF_OK;
}

/* One call of ppf_prep_clusters or ppf_prep_regions: the table, the scratch and the launches (clu_begin, the entry's `link`
 * -- its k_*_runs, clu_cells, its link and flatten passes -- and clu_rank), the one wait, the results.
 * link(fr, w) -> ppf_status */
template <bool NORMALS, class Link>
ppf_status clu_run(const char* who, const ppf_cloud* const* in, int K, int MC, float tolerance, size_t extra, int min_size, int max_size,
                   const double* intr, int image_rows, int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts, int stride,
                   int32_t* const* labels, ppf_cluster_stats& st, Link link) {
  CluWork w{};
  ppf_status s = clu_table(w, who, in, K, MC);
  if (s != PPF_OK || w.N == 0) return s; /* no cloud has a row: no cluster, no launch */
  FrameRun fr;
  std::shared_ptr<DevBuf<float>> blk(new DevBuf<float>());
  auto run = [&]() -> ppf_status {
    ppf_status r;
    if ((r = clu_begin<NORMALS>(fr, w, *blk, tolerance, extra)) != PPF_OK || (r = link(fr, w)) != PPF_OK) return r;
    return clu_rank(fr, w, *blk, min_size, max_size, intr, image_rows, image_cols);
  };
  const ppf_status ran = run(); /* before w is read */
  bool want_labels = false;
  for (int i = 0; labels && i < K; i++) want_labels = want_labels || labels[i];
  std::vector<uint32_t> z(ran == PPF_OK ? w.z_words : 0);
  std::vector<CluGrid> grid((size_t)K);
  std::vector<int32_t> lab(want_labels ? w.N : 0);
  s = fr.finish(who, ran, {{"counters", w.zero, z.size() * sizeof(uint32_t), z.data()},
                           {"grids", w.d_grid, grid.size() * sizeof(CluGrid), grid.data()},
                           {"labels", w.d_labels, w.N * sizeof(int32_t), want_labels ? lab.data() : nullptr}});
  if (s != PPF_OK || (s = clu_results(w, z, grid, lab, blk, out, info, counts, stride, labels)) != PPF_OK) return s;
  fr.report(st);
  return PPF_OK;
}

/* between clu_begin and clu_rank: the runs of the sorted order, the table of cells, the links and the flattening */
ppf_status clusters_link(FrameRun& fr, CluWork& w) {
  const dim3 b256(CLU_BLOCK);
  FRAME_LAUNCH(fr, k_clu_runs, w.rows1_grid, b256, w.d_tab, w.K, (uint32_t)w.N, w.va, w.lkey, w.skey, w.pts, w.flags);
  HIPCHK(hipGetLastError());
  const ppf_status s = clu_cells(fr, w);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_clu_link, dim3((unsigned)w.N), dim3(64), w.pts, w.ckey, w.cstart, w.runid + w.N, w.tol * w.tol, w.parent);
  FRAME_LAUNCH(fr, k_clu_flatten, w.rows_grid, b256, (uint32_t)w.N, w.lkey, w.parent, w.root, w.size);
  return PPF_OK;
}

/* The body of the C entries ppf_prep_clusters and ppf_prep_regions: one stage_entry whose clear zeroes the stats and the
 * outputs, around the argument checks in the order the entries document and `run`.
 * max_shown: the entry's max_clusters / max_regions clamped to 1 .. PPF_CLUSTER_MAX_CLUSTERS (1: no params), the length of a
 * cloud's part of out and info; stride: the words a cloud has in counts.  check_params() -> ppf_status;
 * run(st) -> ppf_status is the entry's clu_run */
template <class Check, class Run>
ppf_status clu_entry(const char* who, const ppf_cloud* const* in, int n_clouds, int max_shown, int stride, const double* intr, int image_rows,
                     int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts, ppf_cluster_stats* stats, Check check_params,
                     Run run) {
  const bool count_ok = n_clouds >= 0 && n_clouds <= FRAME_MAX_BOXES;
  const size_t slots = count_ok ? (size_t)n_clouds * (size_t)max_shown : 0;
  auto clear = [&](ppf_cluster_stats& st, bool) {
    std::memset(&st, 0, sizeof(st));
    for (size_t k = 0; out && k < slots; k++) out[k] = nullptr;
    if (info && slots) std::memset(info, 0, slots * sizeof(ppf_cluster_info));
    if (counts && count_ok && n_clouds) std::memset(counts, 0, (size_t)n_clouds * stride * sizeof(int32_t));
  };
  return stage_entry(stats, clear, [&](ppf_cluster_stats& st) -> ppf_status {
    if (!count_ok) return fail(PPF_ERR_INVALID, "%s: n_clouds is %d (0..%d)", who, n_clouds, FRAME_MAX_BOXES);
    if (!in || !out || !info || !counts) return fail(PPF_ERR_INVALID, "%s: in, out, info and counts must not be NULL", who);
    const ppf_status s = check_params();
    if (s != PPF_OK) return s;
    if (intr) {
      for (int k = 0; k < 4; k++)
        if (!std::isfinite(intr[k])) return fail(PPF_ERR_INVALID, "%s: the intrinsics are not finite", who);
      if (image_rows < 1 || image_cols < 1) return fail(PPF_ERR_INVALID, "%s: the image is %d x %d", who, image_rows, image_cols);
    }
    for (int i = 0; i < n_clouds; i++)
      if (!in[i]) return fail(PPF_ERR_INVALID, "%s: in[%d] is NULL", who, i);
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    st.n_clouds = n_clouds;
    return n_clouds > 0 ? run(st) : PPF_OK;
  });
}
inline int clu_max_shown(int max_components) { return std::min(std::max(max_components, 1), PPF_CLUSTER_MAX_CLUSTERS); }

}  // namespace

extern "C" {

void ppf_default_cluster_params(ppf_cluster_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->tolerance = 0.02f;
  p->min_size = 100;
  p->max_size = 0;
  p->max_clusters = 64;
}

ppf_status ppf_prep_clusters(const ppf_cloud* const* in, int n_clouds, const ppf_cluster_params* p, const double* intr, int image_rows,
                             int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts, int32_t* const* labels,
                             ppf_cluster_stats* stats) {
  static const char* who = "ppf_prep_clusters";
  return clu_entry(
      who, in, n_clouds, p ? clu_max_shown(p->max_clusters) : 1, 3, intr, image_rows, image_cols, out, info, counts, stats,
      [&]() { return cluster_params_check(who, p); },
      [&](ppf_cluster_stats& st) {
        return clu_run<false>(who, in, n_clouds, p->max_clusters, p->tolerance, 0, p->min_size, p->max_size, intr, image_rows, image_cols, out, info,
                              counts, 3, labels, st, clusters_link);
      });
}

}  // extern "C"

#endif /* PPF_CLUSTER_HOST_H */
