/*
 * ppf_edge_host.h — host side of ppf_depth_edges / ppf_depth_edges_device: a depth image's occluding, occluded and boundary
 * edges as a mask and as the edge cloud the matching stages take.  Kernels: ppf_edge_kernels.h.  Included by
 * ppf_hip.hip after ppf_segment_host.h; uses ppf_stage_host.h (FrameRun, frame_scan, stage_entry) and ppf_depthimage_host.h
 * (the image checks, the bindings, depth_outputs_check, depth_typed).
 *
 * Per call, all on the caller's stream (FrameRun::st), whatever the image holds:
 *   mask only                 a 32-byte clear of the counters, k_depth_edges: 1 launch, 1 wait
 *   normals                   + the scan of the runs' kept counts (5) and k_edge_select: 7 launches, 1 wait
 *   cloud                     + the scan of the runs' selected counts (5), the sizing wait, k_edge_write: 7 launches, 2 waits
 *   normals and cloud         13 launches, 2 waits
 * The sizing wait brings the counters and the cloud's row count; a normals cloud of the wrong row count is refused at the
 * call's first wait.  Scratch (the uploaded image, the work bytes, the run counts, the counters) comes from the block cache.
 */
#ifndef PPF_EDGE_HOST_H
#define PPF_EDGE_HOST_H

namespace {

/* every argument check of both entries, before any device work; fills the kernel arguments (img, pitch and buffers excepted) */
ppf_status edge_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const double* intr, const ppf_depth_params* dp,
                      const ppf_cloud* normals, const ppf_depth_edge_params* ep, const uint8_t* edges, ppf_cloud** out_cloud, DepthArgs* a,
                      EdgeArgs* ea) {
  if (out_cloud) *out_cloud = nullptr;
  if (!edges && !out_cloud) return fail(PPF_ERR_INVALID, "%s: edges and out_cloud are both NULL", who);
  if (!ep) return fail(PPF_ERR_INVALID, "%s: the edge params are NULL", who);
  const bool need_intr = out_cloud && !normals;
  if (need_intr && !intr) return fail(PPF_ERR_INVALID, "%s: intr must not be NULL for a cloud without normals", who);
  ppf_status s = depth_pixels_check(who, depth, rows, cols, pitch, dp, DEPTH_FLAGS_FP64, a);
  if (s != PPF_OK || (need_intr && (s = depth_intr_check(who, intr, a)) != PPF_OK) || (s = depth_z_check(who, dp)) != PPF_OK) return s;
  if (!(std::isfinite(ep->depth_abs) && ep->depth_abs >= 0.f) || !(std::isfinite(ep->depth_quad) && ep->depth_quad >= 0.f))
    return fail(PPF_ERR_INVALID, "%s: depth_abs and depth_quad must be finite and >= 0", who);
  if (ep->max_gap < 0 || ep->max_gap > PPF_DEPTH_EDGE_MAX_GAP)
    return fail(PPF_ERR_INVALID, "%s: max_gap %d is outside 0..%d", who, ep->max_gap, PPF_DEPTH_EDGE_MAX_GAP);
  if (!(ep->curvature_threshold >= 0.f)) return fail(PPF_ERR_INVALID, "%s: curvature_threshold must be >= 0 (+inf allowed)", who);
  if (ep->select == 0 || (ep->select & ~(int32_t)EDGE_CLASSES))
    return fail(PPF_ERR_INVALID, "%s: select 0x%x is not a non-zero subset of the four edge bits", who, (unsigned)ep->select);
  if (ep->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown edge flags 0x%x", who, (unsigned)ep->flags);
  ea->rows = rows;
  ea->tiles_x = (int)(((long long)cols + EDGE_TW - 1) / EDGE_TW);
  ea->tiles_y = (int)(((long long)rows + EDGE_TH - 1) / EDGE_TH);
  ea->max_gap = ep->max_gap;
  ea->select = ep->select;
  ea->mark = normals ? 1 : 0;
  ea->final_ = normals ? 0 : 1;
  ea->depth_abs = (double)ep->depth_abs;
  ea->depth_quad = (double)ep->depth_quad;
  ea->curvature_threshold = ep->curvature_threshold;
  ea->nrm_rows = normals ? normals->rows.p : nullptr;
  ea->nrm_curv = normals ? normals->curv.p : nullptr;
  ea->nrm_n = normals ? (uint32_t)normals->n : 0u;
  ea->counters = ea->run_kept = ea->run_sel = nullptr;
  return PPF_OK;
}

/* The whole call on fr.st from the first launch to the cloud: a.img and a.pitch are set by the caller; d_mask receives the
 * final mask (the caller's buffer, or scratch of the caller's when the cloud needs one).  c[] are the counters as the device
 * left them; they are read at the sizing wait of a cloud call, else by the caller's fr.finish through *counters. */
ppf_status edge_enqueue(const char* who, FrameRun& fr, const DepthArgs& a, EdgeArgs ea, int format, const ppf_cloud* normals, uint8_t* d_mask,
                        bool want_cloud, uint32_t** counters, uint32_t* c, std::unique_ptr<ppf_cloud>& cloud) {
  const size_t N = (size_t)a.n, runs = (size_t)ea.rows * (size_t)ea.tiles_x;
  /* at most n / 1024 + rows / 16 + cols / 64 + 1 tiles, at most n / 64 + rows runs: below 2^31 for every n <= INT32_MAX */
  const long long n_tiles = (long long)ea.tiles_x * ea.tiles_y;
  const dim3 bs(EDGE_BLOCK), g_tiles((unsigned)n_tiles), g_runs = grid_for(runs, EDGE_WAVES);
  uint8_t* work = nullptr;
  uint32_t *koff = nullptr, *soff = nullptr;
  ppf_status s = fr.get((size_t)EDGE_N_COUNTERS, &ea.counters);
  if (s == PPF_OK && normals) s = fr.get(N, &work, runs + 1, &ea.run_kept, runs + 1, &koff);
  if (s == PPF_OK && want_cloud) s = fr.get(runs + 1, &ea.run_sel, runs + 1, &soff);
  if (s == PPF_OK && !normals && !d_mask) s = fr.get(N, &d_mask);
  if (s != PPF_OK) return s;
  *counters = ea.counters;
  HIPCHK(hipMemsetAsync(ea.counters, 0, EDGE_N_COUNTERS * sizeof(uint32_t), fr.st));
  uint8_t* first = normals ? work : d_mask;
  depth_typed(format, [&](auto px) { FRAME_LAUNCH(fr, k_depth_edges<decltype(px)>, g_tiles, bs, a, ea, first); });
  HIPCHK(hipGetLastError());
  if (normals) {
    if ((s = frame_scan(fr, ea.run_kept, koff, runs + 1)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_edge_select, g_runs, bs, a, ea, koff, work, d_mask);
    HIPCHK(hipGetLastError());
  }
  if (!want_cloud) return PPF_OK;
  if ((s = frame_scan(fr, ea.run_sel, soff, runs + 1)) != PPF_OK) return s;
  uint32_t total = 0;
  if ((s = fr.sizing({{"counters", ea.counters, EDGE_N_COUNTERS * sizeof(uint32_t), c}, {"row count", soff + runs, sizeof(uint32_t), &total}})) != PPF_OK)
    return s;
  *counters = nullptr; /* read */
  if (normals && (uint32_t)normals->n != c[EDGE_C_KEPT])
    return fail(PPF_ERR_INVALID, "%s: the normals cloud has %d rows, the image keeps %u pixels", who, normals->n, c[EDGE_C_KEPT]);
  if ((s = cloud_alloc(cloud, (int)total)) != PPF_OK) return s;
  depth_typed(format, [&](auto px) {
    FRAME_LAUNCH(fr, k_edge_write<decltype(px)>, g_runs, bs, a, ea, koff, soff, normals ? work : d_mask, total, cloud->rows.p, cloud->curv.p);
  });
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* after the last wait */
ppf_status edge_results(const char* who, const uint32_t* c, const FrameRun& fr, const ppf_cloud* normals, std::unique_ptr<ppf_cloud>& cloud,
                        ppf_cloud** out_cloud, ppf_depth_edge_stats& st) {
  if (normals && (uint32_t)normals->n != c[EDGE_C_KEPT])
    return fail(PPF_ERR_INVALID, "%s: the normals cloud has %d rows, the image keeps %u pixels", who, normals->n, c[EDGE_C_KEPT]);
  st.n_kept = (int32_t)c[EDGE_C_KEPT];
  st.n_occluding = (int32_t)c[EDGE_C_OCCLUDING];
  st.n_occluded = (int32_t)c[EDGE_C_OCCLUDED];
  st.n_boundary = (int32_t)c[EDGE_C_BOUNDARY];
  st.n_curvature = (int32_t)c[EDGE_C_CURVATURE];
  st.n_edge = (int32_t)c[EDGE_C_EDGE];
  st.n_selected = (int32_t)c[EDGE_C_SELECTED];
  st.n_no_normal = (int32_t)c[EDGE_C_NO_NORMAL];
  st.n_rows = cloud ? cloud->n : 0;
  fr.report(st);
  if (out_cloud) *out_cloud = cloud.release();
  return PPF_OK;
}

ppf_status edge_host(const char* who, const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                     const ppf_depth_params* dp, const ppf_cloud* normals, const ppf_depth_edge_params* ep, uint8_t* edges,
                     ppf_cloud** out_cloud, ppf_depth_edge_stats& st) {
  DepthArgs a;
  EdgeArgs ea;
  ppf_status s = edge_check(who, depth, rows, cols, row_pitch_bytes, intr, dp, normals, ep, edges, out_cloud, &a, &ea);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const size_t n = (size_t)rows * (size_t)cols;
  FrameRun fr;
  DevBuf<unsigned char> img;
  uint8_t* d_mask;
  if ((s = depth_bind_host(depth, dp->format, img, &a)) != PPF_OK || (s = fr.get(n, &d_mask)) != PPF_OK) return s;
  std::vector<uint8_t> mask(edges ? n : 0); /* edges stays untouched when a wait brings an error */
  std::unique_ptr<ppf_cloud> cloud;
  uint32_t c[EDGE_N_COUNTERS] = {0};
  uint32_t* d_counters = nullptr;
  s = edge_enqueue(who, fr, a, ea, dp->format, normals, d_mask, out_cloud != nullptr, &d_counters, c, cloud);
  s = fr.finish(who, s, {{"mask", d_mask, n, edges ? mask.data() : nullptr}, {"counters", d_counters, sizeof(c), d_counters ? c : nullptr}});
  if (s != PPF_OK || (s = edge_results(who, c, fr, normals, cloud, out_cloud, st)) != PPF_OK) return s;
  if (edges) std::memcpy(edges, mask.data(), n);
  return PPF_OK;
}

ppf_status edge_device(const char* who, const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                       const ppf_depth_params* dp, const ppf_cloud* normals, const ppf_depth_edge_params* ep, uint8_t* d_edges,
                       hipStream_t stream, ppf_cloud** out_cloud, ppf_depth_edge_stats& st) {
  DepthArgs a;
  EdgeArgs ea;
  StageBuf image;
  ppf_status s = edge_check(who, d_depth, rows, cols, row_pitch_bytes, intr, dp, normals, ep, d_edges, out_cloud, &a, &ea);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = depth_bind_device(who, d_depth, dp->format, &a, &image)) != PPF_OK ||
      (s = depth_outputs_check(who, image, {{"edge mask", d_edges, (size_t)rows * (size_t)cols, nullptr}})) != PPF_OK)
    return s;
  FrameRun fr;
  fr.st = stream;
  std::unique_ptr<ppf_cloud> cloud;
  uint32_t c[EDGE_N_COUNTERS] = {0};
  uint32_t* d_counters = nullptr;
  s = edge_enqueue(who, fr, a, ea, dp->format, normals, d_edges, out_cloud != nullptr, &d_counters, c, cloud);
  s = fr.finish(who, s, {{"counters", d_counters, sizeof(c), d_counters ? c : nullptr}});
  return s != PPF_OK ? s : edge_results(who, c, fr, normals, cloud, out_cloud, st);
}

}  // namespace

extern "C" {

void ppf_default_depth_edge_params(ppf_depth_edge_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->depth_abs = 0.02f;
  p->depth_quad = 0.f;
  p->max_gap = 2;
  p->curvature_threshold = 0.03f;
  p->select = PPF_EDGE_OCCLUDING | PPF_EDGE_BOUNDARY | PPF_EDGE_CURVATURE;
  p->flags = 0;
}

ppf_status ppf_depth_edges(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr, const ppf_depth_params* dp,
                           const ppf_cloud* normals, const ppf_depth_edge_params* ep, uint8_t* edges, ppf_cloud** out_cloud,
                           ppf_depth_edge_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_edge_stats>, [&](ppf_depth_edge_stats& st) {
    return edge_host("ppf_depth_edges", depth, rows, cols, row_pitch_bytes, intr, dp, normals, ep, edges, out_cloud, st);
  });
}

ppf_status ppf_depth_edges_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                  const ppf_depth_params* dp, const ppf_cloud* normals, const ppf_depth_edge_params* ep, uint8_t* d_edges,
                                  void* stream, ppf_cloud** out_cloud, ppf_depth_edge_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_edge_stats>, [&](ppf_depth_edge_stats& st) {
    return edge_device("ppf_depth_edges_device", d_depth, rows, cols, row_pitch_bytes, intr, dp, normals, ep, d_edges,
                       static_cast<hipStream_t>(stream), out_cloud, st);
  });
}

}  // extern "C"

#endif /* PPF_EDGE_HOST_H */
