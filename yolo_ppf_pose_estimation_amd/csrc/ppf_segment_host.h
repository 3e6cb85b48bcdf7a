/*
 * ppf_segment_host.h — host side of ppf_depth_segments / ppf_depth_segments_device: a depth image's surfaces labelled in image
 * space.  Kernels: ppf_segment_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, frame_scan,
 * frame_sort, stage_entry) and ppf_depthimage_host.h (the image check, the bindings, depth_outputs_check, depth_typed).
 *
 * Per call, all on the caller's stream (FrameRun::st): with a normals cloud k_depth_count and a five-launch scan; then k_seg_classify,
 * k_seg_tile, k_seg_merge, k_seg_flatten, k_seg_valid, the ranking's sort (four digit passes of seven launches), k_seg_rank
 * and k_seg_labels: 35 launches, 41 with a normals cloud, whatever the image's size or content.  Nothing the device counts
 * comes to the host before the end: the host waits once, for the counters, the segment heads and the reductions (and, in the
 * host entry, the labels).  The host entry adds one upload of the image.
 */
#ifndef PPF_SEGMENT_HOST_H
#define PPF_SEGMENT_HOST_H

namespace {

/* every argument check of both entries, before any device work; fills the kernel arguments (img and pitch excepted) */
ppf_status segment_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const ppf_depth_params* dp,
                         const ppf_cloud* normals, const ppf_segment_params* sp, const int32_t* labels, const ppf_segment_info* info,
                         const int32_t* counts, DepthArgs* a, SegArgs* sa) {
  if (!labels || !info || !counts) return fail(PPF_ERR_INVALID, "%s: labels, info and counts must not be NULL", who);
  if (!sp) return fail(PPF_ERR_INVALID, "%s: the segment params are NULL", who);
  ppf_status s = depth_image_check(who, depth, rows, cols, pitch, dp, DEPTH_FLAGS_IGNORED, a);
  if (s != PPF_OK) return s;
  if (!(std::isfinite(sp->depth_abs) && sp->depth_abs >= 0.f) || !(std::isfinite(sp->depth_quad) && sp->depth_quad >= 0.f))
    return fail(PPF_ERR_INVALID, "%s: depth_abs and depth_quad must be finite and >= 0", who);
  if (!(std::isfinite(sp->normal_cos) && sp->normal_cos >= -1.f && sp->normal_cos <= 1.f))
    return fail(PPF_ERR_INVALID, "%s: normal_cos must lie in -1..1", who);
  if (!(sp->curvature_threshold >= 0.f)) return fail(PPF_ERR_INVALID, "%s: curvature_threshold must be >= 0 (+inf allowed)", who);
  if (sp->min_size < 1) return fail(PPF_ERR_INVALID, "%s: min_size is %d (>= 1)", who, sp->min_size);
  if (sp->max_size < 0) return fail(PPF_ERR_INVALID, "%s: max_size is %d (>= 0; 0: no bound)", who, sp->max_size);
  if (sp->max_segments < 1 || sp->max_segments > PPF_CLUSTER_MAX_CLUSTERS)
    return fail(PPF_ERR_INVALID, "%s: max_segments is %d (1..%d)", who, sp->max_segments, PPF_CLUSTER_MAX_CLUSTERS);
  if (sp->flags & ~(PPF_SEGMENT_EIGHT | PPF_SEGMENT_UNORIENTED)) return fail(PPF_ERR_INVALID, "%s: unknown segment flags 0x%x", who, (unsigned)sp->flags);
  sa->rows = rows;
  sa->cols = cols;
  sa->tiles_x = (int)(((long long)cols + SEG_TW - 1) / SEG_TW);
  sa->tiles_y = (int)(((long long)rows + SEG_TH - 1) / SEG_TH);
  sa->eight = (sp->flags & PPF_SEGMENT_EIGHT) ? 1 : 0;
  sa->unoriented = (sp->flags & PPF_SEGMENT_UNORIENTED) ? 1 : 0;
  sa->depth_abs = (double)sp->depth_abs;
  sa->depth_quad = (double)sp->depth_quad;
  sa->normal_cos = (double)sp->normal_cos;
  sa->curvature_threshold = sp->curvature_threshold;
  sa->nrm_rows = normals ? normals->rows.p : nullptr;
  sa->nrm_curv = normals ? normals->curv.p : nullptr;
  sa->nrm_n = normals ? (uint32_t)normals->n : 0u;
  return PPF_OK;
}

/* what a call keeps on the device until its one wait */
struct SegWork {
  uint32_t* zero = nullptr; /* [counters | heads | reductions] */
  size_t z_head = 0, z_acc = 0, z_words = 0;
};

/* everything up to the label image, enqueued on fr.st; a.img and a.pitch are set by the caller */
ppf_status segment_enqueue(FrameRun& fr, SegWork& w, const DepthArgs& a, const SegArgs& sa, int format, const ppf_segment_params& sp,
                           int32_t* d_labels) {
  const size_t N = (size_t)a.n;
  const int n = a.n, MC = sp.max_segments;
  const int n_dt = (int)((N + DEPTH_TILE - 1) / DEPTH_TILE), nblk = (n + RS_BLOCK - 1) / RS_BLOCK;
  /* at most n / 1024 + rows / 16 + cols / 64 + 1 tiles: below 2^31 for every n <= INT32_MAX */
  const long long n_tiles = (long long)sa.tiles_x * sa.tiles_y;
  float4* rec;
  uint8_t* cls;
  uint32_t *parent, *size, *nbord, *root, *ka, *va, *kb, *vb, *hist, *offs, *tcnt = nullptr, *toff = nullptr;
  int32_t* rank;
  w.z_head = SEG_N_COUNTERS;
  w.z_acc = w.z_head + (size_t)MC * SEG_HEAD;
  w.z_words = w.z_acc + (size_t)MC * SEG_ACC;
  ppf_status s = fr.get(w.z_words, &w.zero, N, &rec, N, &cls, N, &parent, N, &size, N, &nbord, N, &root, N, &rank, N, &ka, N, &va, N, &kb, N, &vb,
                        (size_t)256 * nblk, &hist, (size_t)256 * nblk, &offs);
  if (s == PPF_OK && sa.nrm_rows) s = fr.get((size_t)n_dt + 1, &tcnt, (size_t)n_dt + 1, &toff);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemsetAsync(w.zero, 0, w.z_words * sizeof(uint32_t), fr.st));
  const dim3 bd(DEPTH_BLOCK), bs(SEG_BLOCK), g_dt((unsigned)n_dt), g_tiles((unsigned)n_tiles), g_px = grid_for(N, SEG_BLOCK);
  if (sa.nrm_rows) {
    depth_typed(format, [&](auto px) { FRAME_LAUNCH(fr, k_depth_count<decltype(px)>, g_dt, bd, a, n_dt, tcnt); });
    HIPCHK(hipGetLastError());
    if ((s = frame_scan(fr, tcnt, toff, (size_t)n_dt + 1)) != PPF_OK) return s;
  }
  depth_typed(format, [&](auto px) { FRAME_LAUNCH(fr, k_seg_classify<decltype(px)>, g_dt, bd, a, sa, toff, rec, cls, size, nbord, rank); });
  FRAME_LAUNCH(fr, k_seg_tile, g_tiles, bs, sa, rec, cls, parent);
  FRAME_LAUNCH(fr, k_seg_merge, g_px, bs, sa, rec, cls, parent);
  FRAME_LAUNCH(fr, k_seg_flatten, g_tiles, bs, sa, rec, cls, parent, root, size, nbord, w.zero);
  FRAME_LAUNCH(fr, k_seg_valid, g_px, bs, (uint32_t)N, root, size, (uint32_t)sp.min_size, (uint32_t)sp.max_size, ka, va, w.zero);
  HIPCHK(hipGetLastError());
  /* all four digits of the key, so the launch count does not depend on the image's size */
  static const int shifts[4] = {0, 8, 16, 24};
  if ((s = frame_sort(fr, ka, va, kb, vb, n, hist, offs, shifts, 4)) != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_seg_rank, dim3(1), dim3(PPF_CLUSTER_MAX_CLUSTERS), (uint32_t)N, va, w.zero, size, nbord, MC, rank,
             reinterpret_cast<int32_t*>(w.zero + w.z_head));
  FRAME_LAUNCH(fr, k_seg_labels, grid_for(N, SEG_TILE), bs, (uint32_t)N, a.cols, root, rank, rec, d_labels, w.zero + w.z_acc);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* after the one wait: z is the zeroed block as the device left it */
ppf_status segment_results(const char* who, const std::vector<uint32_t>& z, const SegWork& w, const FrameRun& fr, const ppf_cloud* normals,
                           const ppf_segment_params& sp, ppf_segment_info* info, int32_t* counts, ppf_segment_stats& st) {
  if (normals && (uint32_t)normals->n != z[SEG_C_KEPT])
    return fail(PPF_ERR_INVALID, "%s: the normals cloud has %d rows, the image keeps %u pixels", who, normals->n, z[SEG_C_KEPT]);
  const uint32_t valid = z[SEG_C_VALID], shown = std::min(valid, (uint32_t)sp.max_segments);
  counts[0] = (int32_t)shown;
  counts[1] = (int32_t)valid;
  counts[2] = (int32_t)z[SEG_C_ALL];
  for (uint32_t r = 0; r < shown; r++) {
    ppf_segment_info& si = info[r];
    const uint32_t* h = &z[w.z_head + (size_t)r * SEG_HEAD];
    const uint32_t* a = &z[w.z_acc + (size_t)r * SEG_ACC];
    si.n_pixels = (int32_t)h[0];
    si.first_pixel = (int32_t)h[1];
    si.n_border = (int32_t)h[2];
    const int32_t u0 = (int32_t)~a[0], u1 = (int32_t)a[1] - 1, v0 = (int32_t)~a[2], v1 = (int32_t)a[3] - 1;
    si.box_xywh[0] = u0; si.box_xywh[1] = v0; si.box_xywh[2] = u1 - u0; si.box_xywh[3] = v1 - v0;
    si.z_lo = ordered_to_float(~a[4]);
    si.z_hi = ordered_to_float(a[5]);
  }
  st.n_kept = (int32_t)z[SEG_C_KEPT];
  st.n_eligible = (int32_t)z[SEG_C_ELIGIBLE];
  st.n_smooth = (int32_t)z[SEG_C_SMOOTH];
  st.n_attached = (int32_t)z[SEG_C_ATTACHED];
  fr.report(st);
  return PPF_OK;
}

ppf_status segment_host(const char* who, const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                        const ppf_cloud* normals, const ppf_segment_params* sp, int32_t* labels, ppf_segment_info* info, int32_t* counts,
                        ppf_segment_stats& st) {
  DepthArgs a;
  SegArgs sa;
  ppf_status s = segment_check(who, depth, rows, cols, row_pitch_bytes, dp, normals, sp, labels, info, counts, &a, &sa);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const size_t n = (size_t)rows * (size_t)cols;
  FrameRun fr;
  SegWork w;
  DevBuf<unsigned char> img;
  int32_t* d_labels;
  if ((s = depth_bind_host(depth, dp->format, img, &a)) != PPF_OK) return s;
  s = fr.get(n, &d_labels);
  if (s != PPF_OK) return s;
  std::vector<int32_t> lab(n); /* labels stay untouched when the wait brings an error */
  std::vector<uint32_t> z;
  if ((s = segment_enqueue(fr, w, a, sa, dp->format, *sp, d_labels)) == PPF_OK) z.resize(w.z_words);
  s = fr.finish(who, s, {{"label buffer", d_labels, n * sizeof(int32_t), lab.data()}, {"counters", w.zero, w.z_words * sizeof(uint32_t), z.data()}});
  if (s != PPF_OK || (s = segment_results(who, z, w, fr, normals, *sp, info, counts, st)) != PPF_OK) return s;
  std::memcpy(labels, lab.data(), n * sizeof(int32_t));
  return PPF_OK;
}

ppf_status segment_device(const char* who, const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                          const ppf_cloud* normals, const ppf_segment_params* sp, int32_t* d_labels, hipStream_t stream, ppf_segment_info* info,
                          int32_t* counts, ppf_segment_stats& st) {
  DepthArgs a;
  SegArgs sa;
  StageBuf image;
  ppf_status s = segment_check(who, d_depth, rows, cols, row_pitch_bytes, dp, normals, sp, d_labels, info, counts, &a, &sa);
  if (s != PPF_OK) return s;
  if ((uintptr_t)d_labels % sizeof(int32_t) != 0) return fail(PPF_ERR_INVALID, "%s: the label buffer is not aligned to 4 bytes", who);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = depth_bind_device(who, d_depth, dp->format, &a, &image)) != PPF_OK ||
      (s = depth_outputs_check(who, image, {{"label buffer", d_labels, (size_t)rows * (size_t)cols * sizeof(int32_t), nullptr}})) != PPF_OK)
    return s;
  FrameRun fr;
  SegWork w;
  fr.st = stream;
  std::vector<uint32_t> z;
  if ((s = segment_enqueue(fr, w, a, sa, dp->format, *sp, d_labels)) == PPF_OK) z.resize(w.z_words);
  s = fr.finish(who, s, {{"counters", w.zero, w.z_words * sizeof(uint32_t), z.data()}});
  return s != PPF_OK ? s : segment_results(who, z, w, fr, normals, *sp, info, counts, st);
}

/* the outputs of a failed call are zero; info is only cleared when the params say how long it is */
void segment_clear(const ppf_segment_params* sp, ppf_segment_info* info, int32_t* counts, ppf_segment_stats& st) {
  std::memset(&st, 0, sizeof(st));
  if (counts) std::memset(counts, 0, 3 * sizeof(int32_t));
  if (info && sp && sp->max_segments >= 1 && sp->max_segments <= PPF_CLUSTER_MAX_CLUSTERS)
    std::memset(info, 0, (size_t)sp->max_segments * sizeof(ppf_segment_info));
}

}  // namespace

extern "C" {

void ppf_default_segment_params(ppf_segment_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->depth_abs = 0.005f;
  p->depth_quad = 0.f;
  p->normal_cos = 0.9659258f;
  p->curvature_threshold = 0.03f;
  p->min_size = 100;
  p->max_size = 0;
  p->max_segments = 64;
  p->flags = 0;
}

ppf_status ppf_depth_segments(const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                              const ppf_cloud* normals, const ppf_segment_params* sp, int32_t* labels, ppf_segment_info* info,
                              int32_t* counts, ppf_segment_stats* stats) {
  return stage_entry(stats, [&](ppf_segment_stats& st, bool) { segment_clear(sp, info, counts, st); }, [&](ppf_segment_stats& st) {
    return segment_host("ppf_depth_segments", depth, rows, cols, row_pitch_bytes, dp, normals, sp, labels, info, counts, st);
  });
}

ppf_status ppf_depth_segments_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                     const ppf_cloud* normals, const ppf_segment_params* sp, int32_t* d_labels, void* stream,
                                     ppf_segment_info* info, int32_t* counts, ppf_segment_stats* stats) {
  return stage_entry(stats, [&](ppf_segment_stats& st, bool) { segment_clear(sp, info, counts, st); }, [&](ppf_segment_stats& st) {
    return segment_device("ppf_depth_segments_device", d_depth, rows, cols, row_pitch_bytes, dp, normals, sp, d_labels,
                          static_cast<hipStream_t>(stream), info, counts, st);
  });
}

}  // extern "C"

#endif /* PPF_SEGMENT_HOST_H */
