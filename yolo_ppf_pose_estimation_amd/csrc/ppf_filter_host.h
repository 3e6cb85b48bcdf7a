/*
 * ppf_filter_host.h — host side of ppf_depth_filter / ppf_depth_filter_device: a depth image without its unsupported pixels,
 * smoothed inside each surface.  Kernel: ppf_filter_kernels.h.  Included by ppf_hip.hip after
 * ppf_depthimage_host.h (the image check, the bindings, depth_outputs_check, stage_finish, stage_entry, depth_typed).
 *
 * Per call: an 8-byte clear of the counters, k_depth_filter -- one launch -- and one blocking wait, whatever the image
 * holds.  The host entry adds one upload of the image and reads the image and the counters back behind that one wait.
 * Scratch (the uploaded image, the host entry's output, the counters) comes from the block cache.
 */
#ifndef PPF_FILTER_HOST_H
#define PPF_FILTER_HOST_H

namespace {

/* every argument check of both entries, before any device work; fills the kernel arguments (img, pitch and counters excepted) */
ppf_status filter_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const ppf_depth_params* dp,
                        const ppf_depth_filter_params* fp, const float* out, DepthArgs* a, DepthFilterArgs* fa) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  if (!fp) return fail(PPF_ERR_INVALID, "%s: the filter params are NULL", who);
  ppf_status s = depth_image_check(who, depth, rows, cols, pitch, dp, DEPTH_FLAGS_IGNORED, a);
  if (s != PPF_OK) return s;
  if (fp->radius < 0 || fp->radius > PPF_DEPTH_FILTER_MAX_RADIUS)
    return fail(PPF_ERR_INVALID, "%s: radius %d is outside 0..%d", who, fp->radius, PPF_DEPTH_FILTER_MAX_RADIUS);
  if (!std::isfinite(fp->range_abs) || !(fp->range_abs > 0.f)) return fail(PPF_ERR_INVALID, "%s: range_abs must be finite and > 0", who);
  if (!(std::isfinite(fp->range_quad) && fp->range_quad >= 0.f) || !(std::isfinite(fp->support_abs) && fp->support_abs >= 0.f) ||
      !(std::isfinite(fp->support_quad) && fp->support_quad >= 0.f))
    return fail(PPF_ERR_INVALID, "%s: range_quad, support_abs and support_quad must be finite and >= 0", who);
  if (fp->min_support < 0 || fp->min_support > 8) return fail(PPF_ERR_INVALID, "%s: min_support %d is outside 0..8", who, fp->min_support);
  if (fp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown filter flags 0x%x", who, (unsigned)fp->flags);
  fa->rows = rows;
  fa->tiles_x = (int)(((long long)cols + DF_TILE_W - 1) / DF_TILE_W);
  fa->radius = fp->radius;
  fa->min_support = fp->min_support;
  fa->range_abs = fp->range_abs;
  fa->range_quad = fp->range_quad;
  fa->support_abs = fp->support_abs;
  fa->support_quad = fp->support_quad;
  fa->counters = nullptr;
  return PPF_OK;
}

/* the counters cleared and the one launch, on `st`; a.img, a.pitch and fa.counters are set by the caller */
ppf_status filter_enqueue(const DepthArgs& a, const DepthFilterArgs& fa, int format, float* d_out, hipStream_t st) {
  /* at most n / 256 + rows / 4 + cols / 64 + 1 workgroups: below 2^31 for every n <= INT32_MAX */
  const long long n_win = (long long)fa.tiles_x * (((long long)fa.rows + DF_TILE_H - 1) / DF_TILE_H);
  HIPCHK(hipMemsetAsync(fa.counters, 0, DF_N_COUNTERS * sizeof(int32_t), st));
  depth_typed(format, [&](auto px) { k_depth_filter<decltype(px)><<<dim3((unsigned)n_win), dim3(DF_BLOCK), 0, st>>>(a, fa, d_out); });
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

void filter_fill_stats(ppf_depth_filter_stats& st, const int32_t* c) {
  st.n_kept = c[DF_C_KEPT];
  st.n_unsupported = c[DF_C_UNSUPPORTED];
  st.n_written = c[DF_C_KEPT] - c[DF_C_UNSUPPORTED];
  st.n_launches = 1;
  st.n_host_syncs = 1;
}

ppf_status filter_host(const char* who, const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                       const ppf_depth_filter_params* fp, float* out, ppf_depth_filter_stats& st) {
  DepthArgs a;
  DepthFilterArgs fa;
  ppf_status s = filter_check(who, depth, rows, cols, row_pitch_bytes, dp, fp, out, &a, &fa);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const size_t n = (size_t)rows * (size_t)cols;
  DevBuf<unsigned char> img;
  DevBuf<float> buf; /* the output, then the counters */
  if ((s = depth_bind_host(depth, dp->format, img, &a)) != PPF_OK) return s;
  HIPCHK(buf.reserve(n + DF_N_COUNTERS));
  fa.counters = reinterpret_cast<int32_t*>(buf.p + n);
  int32_t c[DF_N_COUNTERS];
  s = stage_finish(who, filter_enqueue(a, fa, dp->format, buf.p, nullptr), nullptr,
                   {{"output", buf.p, n * sizeof(float), out}, {"counters", fa.counters, sizeof(c), c}});
  if (s == PPF_OK) filter_fill_stats(st, c);
  return s;
}

ppf_status filter_device(const char* who, const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                         const ppf_depth_filter_params* fp, float* d_out, hipStream_t stream, ppf_depth_filter_stats& st) {
  DepthArgs a;
  DepthFilterArgs fa;
  StageBuf image;
  ppf_status s = filter_check(who, d_depth, rows, cols, row_pitch_bytes, dp, fp, d_out, &a, &fa);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = depth_bind_device(who, d_depth, dp->format, &a, &image)) != PPF_OK ||
      (s = depth_outputs_check(who, image, {{"output", d_out, (size_t)rows * (size_t)cols * sizeof(float), nullptr}})) != PPF_OK)
    return s;
  DevBuf<int32_t> counters;
  HIPCHK(counters.reserve(DF_N_COUNTERS));
  fa.counters = counters.p;
  int32_t c[DF_N_COUNTERS];
  s = stage_finish(who, filter_enqueue(a, fa, dp->format, d_out, stream), stream, {{"counters", counters.p, sizeof(c), c}});
  if (s == PPF_OK) filter_fill_stats(st, c);
  return s;
}

}  // namespace

extern "C" {

void ppf_default_depth_filter_params(ppf_depth_filter_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius = 3;
  p->range_abs = 0.01f;
  p->range_quad = 0.f;
  p->support_abs = 0.01f;
  p->support_quad = 0.f;
  p->min_support = 6;
  p->flags = 0;
}

ppf_status ppf_depth_filter(const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                            const ppf_depth_filter_params* fp, float* out, ppf_depth_filter_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_filter_stats>, [&](ppf_depth_filter_stats& st) {
    return filter_host("ppf_depth_filter", depth, rows, cols, row_pitch_bytes, dp, fp, out, st);
  });
}

ppf_status ppf_depth_filter_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                   const ppf_depth_filter_params* fp, float* d_out, void* stream, ppf_depth_filter_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_filter_stats>, [&](ppf_depth_filter_stats& st) {
    return filter_device("ppf_depth_filter_device", d_depth, rows, cols, row_pitch_bytes, dp, fp, d_out, static_cast<hipStream_t>(stream), st);
  });
}

}  // extern "C"

#endif /* PPF_FILTER_HOST_H */
