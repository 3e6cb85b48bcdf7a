/*
 * ppf_plane_host.h — host side of ppf_prep_planes and ppf_prep_planes_apply: the support planes of up to 256 clouds found
 * and removed in one pass.  Kernels: ppf_plane_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h
 * (FrameRun, frame_scan, stage_entry) and ppf_prep_host.h (ppf_cloud, frame_compact, one_segment).
 *
 * Per call: one upload of the segment table before any device work, then k_pln_load, per round
 *   k_pln_hyp, k_pln_count, k_pln_best, [k_pln_sum<3>, k_pln_finish<3>, k_pln_sum<6>, k_pln_finish<6>, k_pln_recount,
 *   k_pln_choose unless PPF_PLANE_NO_REFIT,] k_pln_flags, the five launches of the scan, k_pln_compact
 * and k_pln_gather: 2 + 16 * max_planes launches, 2 + 10 * max_planes without the refit, whatever the clouds hold.  The
 * rows left per cloud never come to the host between rounds.  The host blocks twice: in that upload, before anything is
 * launched, and once for the results (the info rows, the labels and the rows kept per cloud); n_host_syncs counts waits
 * for the device, which is the second.  The outputs are views into one block sized for the input (a cloud keeps its place in it), so nothing
 * is allocated after that wait.  Scratch comes from the block cache.
 */
#ifndef PPF_PLANE_HOST_H
#define PPF_PLANE_HOST_H

namespace {

ppf_status plane_params_check(const char* who, const ppf_plane_params* p) {
  if (!p) return fail(PPF_ERR_INVALID, "%s: the params are NULL", who);
  if (!(std::isfinite(p->distance_threshold) && p->distance_threshold > 0.f))
    return fail(PPF_ERR_INVALID, "%s: distance_threshold must be finite and > 0", who);
  if (p->n_hypotheses < 1 || p->n_hypotheses > PPF_PLANE_MAX_HYPOTHESES)
    return fail(PPF_ERR_INVALID, "%s: n_hypotheses is %d (1..%d)", who, p->n_hypotheses, PPF_PLANE_MAX_HYPOTHESES);
  if (p->max_planes < 1 || p->max_planes > PPF_PLANE_MAX_PLANES)
    return fail(PPF_ERR_INVALID, "%s: max_planes is %d (1..%d)", who, p->max_planes, PPF_PLANE_MAX_PLANES);
  if (p->min_inliers < 3) return fail(PPF_ERR_INVALID, "%s: min_inliers is %d (>= 3)", who, p->min_inliers);
  if (!(std::isfinite(p->min_inlier_share) && p->min_inlier_share >= 0.f && p->min_inlier_share <= 1.f))
    return fail(PPF_ERR_INVALID, "%s: min_inlier_share must lie in [0, 1]", who);
  if (p->flags & ~(PPF_PLANE_NO_REFIT | PPF_PLANE_REMOVE_BEHIND)) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  return PPF_OK;
}

ppf_status planes_run(const ppf_cloud* const* in, int K, const ppf_plane_params& p, ppf_cloud** out, ppf_plane_info* info,
                      uint8_t* const* labels, ppf_plane_stats& st) {
  static const char* who = "ppf_prep_planes";
  const int R = p.max_planes, H = p.n_hypotheses;
  std::vector<PlnSeg> tab((size_t)K);
  size_t N = 0, T = 0;
  for (int i = 0; i < K; i++) {
    tab[i] = PlnSeg{in[i]->rows.p, in[i]->curv.p, (uint32_t)N, (uint32_t)in[i]->n, (uint32_t)T, 0u};
    N += (size_t)in[i]->n;
    T += ((size_t)in[i]->n + PLN_TILE - 1) / PLN_TILE;
    if (N >= 0x7fffffffull) return fail(PPF_ERR_INVALID, "%s: the clouds hold more than INT32_MAX rows together", who);
  }
  std::vector<std::unique_ptr<ppf_cloud>> res((size_t)K);
  if (N == 0) { /* nothing to search: K empty clouds, the info rows stay zero */
    for (int i = 0; i < K; i++) {
      ppf_status s = cloud_alloc(res[i], 0);
      if (s != PPF_OK) return s;
    }
    for (int i = 0; i < K; i++) out[i] = res[i].release();
    return PPF_OK;
  }
  PlnSeg* d_tab;
  PlnWork* d_work;
  ppf_plane_info* d_info;
  float4 *lpa, *lpb;
  uint8_t* d_labels;
  double *hyp, *part, *ta, *tb;
  uint32_t *cnt, *flags, *pos;
  const size_t tree = (T / 64 + (size_t)K + 1) * 6;
  FrameRun fr;
  std::shared_ptr<DevBuf<float>> blk(new DevBuf<float>());
  ppf_status s = fr.get(K, &d_tab, K, &d_work, (size_t)K * R, &d_info, N, &lpa, N, &lpb, N, &d_labels, (size_t)K * H * 4, &hyp, (size_t)K * H, &cnt,
                        T * 6, &part, tree, &ta, tree, &tb, N + 1, &flags, N + 1, &pos);
  if (s != PPF_OK) return s;
  HIPCHK(blk->reserve(N * 7)); /* [rows | curvature] */
  HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(PlnSeg), hipMemcpyHostToDevice));
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemsetAsync(d_work, 0, (size_t)K * sizeof(PlnWork), nullptr));
    HIPCHK(hipMemsetAsync(d_info, 0, (size_t)K * R * sizeof(ppf_plane_info), nullptr));
    const dim3 tiles((unsigned)T), blk256(PLN_BLOCK), hyp_blocks((unsigned)((H + PLN_BLOCK - 1) / PLN_BLOCK));
    const double thr = (double)p.distance_threshold;
    const int behind = (p.flags & PPF_PLANE_REMOVE_BEHIND) ? 1 : 0;
    FRAME_LAUNCH(fr, k_pln_load, tiles, blk256, d_tab, K, lpa, d_labels, d_work);
    for (int r = 0; r < R; r++) {
      FRAME_LAUNCH(fr, k_pln_hyp, dim3(hyp_blocks.x, (unsigned)K), blk256, d_tab, d_work, lpa, r, p.seed, H, hyp, cnt);
      FRAME_LAUNCH(fr, k_pln_count, dim3((unsigned)(T * PLN_SPANS), hyp_blocks.x), blk256, d_tab, K, d_work, lpa, hyp, H, thr, cnt);
      FRAME_LAUNCH(fr, k_pln_best, dim3((unsigned)K), blk256, d_work, hyp, cnt, H, (int)p.min_inliers, (double)p.min_inlier_share, r, R, d_info);
      if (!(p.flags & PPF_PLANE_NO_REFIT)) {
        FRAME_LAUNCH(fr, k_pln_sum<3>, tiles, blk256, d_tab, K, d_work, lpa, thr, part);
        FRAME_LAUNCH(fr, k_pln_finish<3>, dim3((unsigned)K), blk256, d_tab, d_work, part, ta, tb);
        FRAME_LAUNCH(fr, k_pln_sum<6>, tiles, blk256, d_tab, K, d_work, lpa, thr, part);
        FRAME_LAUNCH(fr, k_pln_finish<6>, dim3((unsigned)K), blk256, d_tab, d_work, part, ta, tb);
        FRAME_LAUNCH(fr, k_pln_recount, tiles, blk256, d_tab, K, d_work, lpa, thr);
        FRAME_LAUNCH(fr, k_pln_choose, dim3(1), dim3(FRAME_MAX_BOXES), d_work, K, r, R, d_info);
      }
      FRAME_LAUNCH(fr, k_pln_flags, tiles, blk256, d_tab, K, d_work, lpa, thr, behind, r, R, (uint32_t)N, flags, d_labels, d_info);
      HIPCHK(hipGetLastError());
      const ppf_status q = frame_scan(fr, flags, pos, N + 1);
      if (q != PPF_OK) return q;
      FRAME_LAUNCH(fr, k_pln_compact, tiles, blk256, d_tab, K, d_work, lpa, flags, pos, lpb);
      std::swap(lpa, lpb);
    }
    FRAME_LAUNCH(fr, k_pln_gather, tiles, blk256, d_tab, K, d_work, lpa, blk->p, blk->p + N * 6);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run();
  /* the one wait: the rows kept per cloud, the info rows, the labels (their host arrays are made while the kernels run) */
  std::vector<PlnWork> work((size_t)K);
  bool want_labels = false;
  for (int i = 0; labels && i < K; i++) want_labels = want_labels || labels[i];
  std::vector<uint8_t> lab(want_labels ? N : 0);
  s = fr.finish(who, ran, {{"work", d_work, work.size() * sizeof(PlnWork), work.data()},
                             {"info", d_info, (size_t)K * R * sizeof(ppf_plane_info), info},
                             {"labels", d_labels, N, want_labels ? lab.data() : nullptr}});
  if (s != PPF_OK) return s;
  for (int i = 0; i < K; i++) {
    res[i].reset(new ppf_cloud());
    res[i]->n = (int)work[i].m;
    res[i]->shared = blk;
    res[i]->rows.p = blk->p + (size_t)tab[i].off * 6;
    res[i]->curv.p = blk->p + N * 6 + tab[i].off;
    if (want_labels && labels[i] && tab[i].n) std::memcpy(labels[i], lab.data() + tab[i].off, tab[i].n);
  }
  for (int i = 0; i < K; i++) out[i] = res[i].release();
  fr.report(st);
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_plane_params(ppf_plane_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->distance_threshold = 0.005f;
  p->n_hypotheses = 256;
  p->seed = 1u;
  p->max_planes = 1;
  p->min_inliers = 100;
  p->min_inlier_share = 0.10f;
}

ppf_status ppf_prep_planes(const ppf_cloud* const* in, int n_clouds, const ppf_plane_params* p, ppf_cloud** out, ppf_plane_info* info,
                           uint8_t* const* labels, ppf_plane_stats* stats) {
  static const char* who = "ppf_prep_planes";
  const bool count_ok = n_clouds >= 0 && n_clouds <= FRAME_MAX_BOXES;
  const size_t info_rows = count_ok ? (size_t)n_clouds * (size_t)(p ? std::min(std::max(p->max_planes, 1), PPF_PLANE_MAX_PLANES) : 1) : 0;
  auto clear = [&](ppf_plane_stats& st, bool) {
    std::memset(&st, 0, sizeof(st));
    for (int i = 0; out && count_ok && i < n_clouds; i++) out[i] = nullptr;
    if (info && info_rows) std::memset(info, 0, info_rows * sizeof(ppf_plane_info));
  };
  return stage_entry(stats, clear, [&](ppf_plane_stats& st) -> ppf_status {
    if (!count_ok) return fail(PPF_ERR_INVALID, "%s: n_clouds is %d (0..%d)", who, n_clouds, FRAME_MAX_BOXES);
    if (!in || !out || !info) return fail(PPF_ERR_INVALID, "%s: in, out and info must not be NULL", who);
    const ppf_status s = plane_params_check(who, p);
    if (s != PPF_OK) return s;
    for (int i = 0; i < n_clouds; i++)
      if (!in[i]) return fail(PPF_ERR_INVALID, "%s: in[%d] is NULL", who, i);
    if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
    st.n_clouds = n_clouds;
    return n_clouds > 0 ? planes_run(in, n_clouds, *p, out, info, labels, st) : PPF_OK;
  });
}

ppf_status ppf_prep_planes_apply(const ppf_cloud* in, const ppf_plane_info* planes, int n_planes, const ppf_plane_params* p,
                                 ppf_cloud** out) {
  static const char* who = "ppf_prep_planes_apply";
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!in) return fail(PPF_ERR_INVALID, "%s: cloud is NULL", who);
  if (n_planes < 0 || n_planes > PPF_PLANE_MAX_PLANES) return fail(PPF_ERR_INVALID, "%s: n_planes is %d (0..%d)", who, n_planes, PPF_PLANE_MAX_PLANES);
  if (n_planes > 0 && !planes) return fail(PPF_ERR_INVALID, "%s: planes is NULL", who);
  ppf_status s = plane_params_check(who, p);
  if (s != PPF_OK) return s;
  PlnPlanes pl;
  pl.n = 0;
  for (int k = 0; k < n_planes; k++) {
    if (planes[k].status != PPF_PLANE_REMOVED) continue;
    const double P[4] = {planes[k].n[0], planes[k].n[1], planes[k].n[2], planes[k].d};
    for (double v : P)
      if (!std::isfinite(v)) return fail(PPF_ERR_INVALID, "%s: planes[%d] is not finite", who, k);
    std::memcpy(pl.P[pl.n++], P, sizeof(P));
  }
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if (in->n == 0) return prep_empty(out);
  std::unique_ptr<ppf_cloud> c(new ppf_cloud());
  FrameRun fr;
  SegCloud seg, res;
  uint32_t* flags;
  s = fr.get((size_t)in->n + 1, &flags);
  if (s != PPF_OK) return s;
  auto run = [&]() -> ppf_status {
    const ppf_status r = one_segment(fr, in, &seg);
    if (r != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_pln_apply_flags, grid_for((size_t)in->n + 1, PLN_BLOCK), dim3(PLN_BLOCK), in->rows.p, in->n, pl, (double)p->distance_threshold,
                 (p->flags & PPF_PLANE_REMOVE_BEHIND) ? 1 : 0, flags);
    HIPCHK(hipGetLastError());
    return frame_compact(fr, seg, flags, c.get(), &res);
  };
  if ((s = fr.finish(who, run(), {})) != PPF_OK) return s;
  *out = c.release();
  return PPF_OK;
}

}  // extern "C"

#endif /* PPF_PLANE_HOST_H */
