/*
 * ppf_region_host.h — host side of ppf_prep_regions: the smooth surface regions of up to 256 clouds in one pass (DESIGN.md
 * §22).  Kernels: ppf_region_kernels.h.  Included by ppf_hip.hip after ppf_cluster_host.h, whose clu_begin, clu_cells and
 * clu_rank it runs around its own four kernels, inside that file's call (clu_run) and entry body (clu_entry).
 *
 * Per call: clu_begin<true> (k_clu_bounds, k_clu_grid and k_clu_keys over the eligible rows, the sort by (segment, cell)),
 * k_reg_runs, clu_cells, k_reg_link, k_reg_flatten, k_reg_attach, clu_rank: 111 launches whatever the clouds hold -- one more
 * than ppf_prep_clusters, the attach pass -- and none when no cloud has a row.  One upload before any device work, one wait.
 */
#ifndef PPF_REGION_HOST_H
#define PPF_REGION_HOST_H

namespace {

ppf_status region_params_check(const char* who, const ppf_region_params* p) {
  if (!p) return fail(PPF_ERR_INVALID, "%s: the params are NULL", who);
  if (!(std::isfinite(p->tolerance) && p->tolerance > 0.f)) return fail(PPF_ERR_INVALID, "%s: tolerance must be finite and > 0", who);
  if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f)) return fail(PPF_ERR_INVALID, "%s: normal_cos must lie in -1..1", who);
  if (!(p->curvature_threshold >= 0.f)) return fail(PPF_ERR_INVALID, "%s: curvature_threshold must be >= 0 (+inf: every eligible row is smooth)", who);
  if (p->min_size < 1) return fail(PPF_ERR_INVALID, "%s: min_size is %d (>= 1)", who, p->min_size);
  if (p->max_size < 0) return fail(PPF_ERR_INVALID, "%s: max_size is %d (>= 0; 0: no bound)", who, p->max_size);
  if (p->max_regions < 1 || p->max_regions > PPF_CLUSTER_MAX_CLUSTERS)
    return fail(PPF_ERR_INVALID, "%s: max_regions is %d (1..%d)", who, p->max_regions, PPF_CLUSTER_MAX_CLUSTERS);
  if (p->flags & ~PPF_REGION_UNORIENTED) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  return PPF_OK;
}

/* between clu_begin<true> and clu_rank, as clusters_link */
ppf_status regions_link(FrameRun& fr, CluWork& w, const ppf_region_params& p) {
  float4* nrm;
  ppf_status s = fr.get(w.N, &nrm);
  if (s != PPF_OK) return s;
  const dim3 b256(CLU_BLOCK);
  const double tol2 = w.tol * w.tol, cosv = (double)p.normal_cos;
  const int unoriented = (p.flags & PPF_REGION_UNORIENTED) ? 1 : 0;
  FRAME_LAUNCH(fr, k_reg_runs, w.rows1_grid, b256, w.d_tab, (uint32_t)w.N, w.va, w.lkey, w.skey, p.curvature_threshold, w.pts, nrm, w.flags);
  HIPCHK(hipGetLastError());
  if ((s = clu_cells(fr, w)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_reg_link, dim3((unsigned)w.N), dim3(64), w.pts, nrm, w.ckey, w.cstart, w.runid + w.N, tol2, cosv, unoriented, w.parent);
  FRAME_LAUNCH(fr, k_reg_flatten, w.rows_grid, b256, (uint32_t)w.N, w.pts, nrm, w.parent, w.root, w.size);
  FRAME_LAUNCH(fr, k_reg_attach, w.rows_grid, b256, (uint32_t)w.N, w.pts, nrm, w.lkey, w.skey, w.ckey, w.cstart, w.runid + w.N, tol2, cosv,
               unoriented, w.root, w.size, w.zero + w.z_extra);
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_region_params(ppf_region_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->tolerance = 0.01f;
  p->normal_cos = 0.9659258f;
  p->curvature_threshold = 0.03f;
  p->min_size = 100;
  p->max_size = 0;
  p->max_regions = 64;
}

ppf_status ppf_prep_regions(const ppf_cloud* const* in, int n_clouds, const ppf_region_params* p, const double* intr, int image_rows,
                            int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts, int32_t* const* labels,
                            ppf_cluster_stats* stats) {
  static const char* who = "ppf_prep_regions";
  return clu_entry(
      who, in, n_clouds, p ? clu_max_shown(p->max_regions) : 1, 4, intr, image_rows, image_cols, out, info, counts, stats,
      [&]() { return region_params_check(who, p); },
      [&](ppf_cluster_stats& st) {
        return clu_run<true>(who, in, n_clouds, p->max_regions, p->tolerance, (size_t)n_clouds /* attached border rows */, p->min_size, p->max_size,
                             intr, image_rows, image_cols, out, info, counts, 4, labels, st,
                             [&](FrameRun& fr, CluWork& w) { return regions_link(fr, w, *p); });
      });
}

}  // extern "C"

#endif /* PPF_REGION_HOST_H */
