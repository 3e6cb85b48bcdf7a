/*
 * ppf_history_host.h — host side of ppf_depth_history: a device-resident ring of a camera's last `window` depth images and
 * the fused image every pushed frame gives.  Kernel: ppf_history_kernels.h.  Included by ppf_hip.hip after
 * ppf_depthimage_host.h (the image check, the bindings, depth_outputs_check, stage_finish, stage_entry, depth_typed).
 *
 * Per push: a 20-byte clear of the counters, k_history_push -- one launch -- and one blocking wait, whatever the image and
 * the history hold.  The host entry adds one upload of the image and reads the images and the counters back behind that one
 * wait.  The ring and the counters belong to the handle; the host entry's scratch comes from the block cache.  A handle's
 * pushes are serialised by its mutex: the ring's slot and t change only after the wait, so a failed push changes neither.
 */
#ifndef PPF_HISTORY_HOST_H
#define PPF_HISTORY_HOST_H

struct ppf_depth_history {
  int rows = 0, cols = 0;
  ppf_depth_params dp;
  ppf_depth_history_params hp;
  long long t = 0; /* pushes since creation or the last reset */
  std::mutex mu;
  DevBuf<float> ring;
  DevBuf<int32_t> counters;
  size_t plane = 0; /* floats per plane */
};

namespace {

/* the instantiation that holds a window: the smallest power of two >= window */
template <class T>
void history_launch(int window, unsigned grid, hipStream_t st, const DepthArgs& a, const HistoryArgs& ha) {
  switch (window <= 1 ? 1 : window <= 2 ? 2 : window <= 4 ? 4 : window <= 8 ? 8 : 16) {
    case 1: k_history_push<T, 1><<<dim3(grid), dim3(DH_BLOCK), 0, st>>>(a, ha); break;
    case 2: k_history_push<T, 2><<<dim3(grid), dim3(DH_BLOCK), 0, st>>>(a, ha); break;
    case 4: k_history_push<T, 4><<<dim3(grid), dim3(DH_BLOCK), 0, st>>>(a, ha); break;
    case 8: k_history_push<T, 8><<<dim3(grid), dim3(DH_BLOCK), 0, st>>>(a, ha); break;
    default: k_history_push<T, 16><<<dim3(grid), dim3(DH_BLOCK), 0, st>>>(a, ha); break;
  }
}

/* the kernel arguments of the push of frame h->t; ring, counters and the three alignment decisions included */
HistoryArgs history_args(const ppf_depth_history* h, const DepthArgs& a, float* d_out, uint8_t* d_state) {
  HistoryArgs ha;
  const int K = h->hp.window;
  ha.rows = h->rows;
  ha.groups = (int)(((long long)h->cols + DH_PX - 1) / DH_PX);
  ha.n_hist = (int)std::min<long long>(h->t + 1, K);
  ha.slot = (int)(h->t % K);
  ha.window = K;
  ha.min_support = h->hp.min_support;
  ha.max_age = h->hp.max_age;
  ha.mean = (h->hp.flags & PPF_HISTORY_MEAN) ? 1 : 0;
  ha.range_abs = h->hp.range_abs;
  ha.range_quad = h->hp.range_quad;
  ha.plane = h->plane;
  ha.ring = h->ring.p;
  ha.out = d_out;
  ha.state = d_state;
  const size_t quad = depth_elem_size(h->dp.format) * DH_PX; /* 16 or 8 bytes */
  ha.in_vec = ((uintptr_t)a.img % quad == 0 && a.pitch % quad == 0) ? 1 : 0;
  ha.out_vec = (h->cols % DH_PX == 0 && (uintptr_t)d_out % 16 == 0) ? 1 : 0;
  ha.state_vec = (h->cols % DH_PX == 0 && (uintptr_t)d_state % 4 == 0) ? 1 : 0;
  ha.counters = h->counters.p;
  return ha;
}

/* the counters cleared and the one launch, on `st` */
ppf_status history_enqueue(const ppf_depth_history* h, const DepthArgs& a, const HistoryArgs& ha, hipStream_t st) {
  /* rows * ceil(cols / 4) lanes: at most rows * cols <= INT32_MAX, so the grid is below 2^23 workgroups */
  const long long lanes = (long long)ha.rows * ha.groups;
  const unsigned grid = (unsigned)((lanes + DH_BLOCK - 1) / DH_BLOCK);
  HIPCHK(hipMemsetAsync(ha.counters, 0, DH_N_COUNTERS * sizeof(int32_t), st));
  depth_typed(h->dp.format, [&](auto px) { history_launch<decltype(px)>(h->hp.window, grid, st, a, ha); });
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

void history_fill_stats(ppf_depth_history_stats& st, const int32_t* c, const ppf_depth_history* h) {
  st.n_kept = c[DH_C_KEPT];
  st.n_measured = c[DH_C_MEASURED];
  st.n_filled = c[DH_C_FILLED];
  st.n_unsupported = c[DH_C_UNSUPPORTED];
  st.n_empty = h->rows * h->cols - c[DH_C_MEASURED] - c[DH_C_FILLED] - c[DH_C_UNSUPPORTED];
  st.n_changed = c[DH_C_CHANGED];
  st.frame = h->t;
  st.n_launches = 1;
  st.n_host_syncs = 1;
}

ppf_status history_push_host(const char* who, ppf_depth_history* h, const void* depth, size_t row_pitch_bytes, float* out, uint8_t* state,
                             ppf_depth_history_stats& st) {
  if (!h) return fail(PPF_ERR_INVALID, "%s: the history is NULL", who);
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  DepthArgs a;
  ppf_status s = depth_image_check(who, depth, h->rows, h->cols, row_pitch_bytes, &h->dp, DEPTH_FLAGS_IGNORED, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  std::lock_guard<std::mutex> lock(h->mu);
  const size_t n = (size_t)h->rows * (size_t)h->cols;
  DevBuf<unsigned char> img;
  DevBuf<float> buf;       /* the output */
  DevBuf<uint8_t> sbuf;    /* the state */
  if ((s = depth_bind_host(depth, h->dp.format, img, &a)) != PPF_OK) return s;
  HIPCHK(buf.reserve(n));
  if (state) HIPCHK(sbuf.reserve(n));
  const HistoryArgs ha = history_args(h, a, buf.p, state ? sbuf.p : nullptr);
  /* into staging first: out and state are only written once everything has succeeded */
  std::vector<float> o(n);
  std::vector<uint8_t> sv(state ? n : 0);
  int32_t c[DH_N_COUNTERS];
  s = stage_finish(who, history_enqueue(h, a, ha, nullptr), nullptr,
                   {{"output", buf.p, n * sizeof(float), o.data()},
                    {"state image", sbuf.p, n, state ? sv.data() : nullptr},
                    {"counters", ha.counters, sizeof(c), c}});
  if (s != PPF_OK) return s;
  std::memcpy(out, o.data(), n * sizeof(float));
  if (state) std::memcpy(state, sv.data(), n);
  history_fill_stats(st, c, h);
  h->t++;
  return PPF_OK;
}

ppf_status history_push_device(const char* who, ppf_depth_history* h, const void* d_depth, size_t row_pitch_bytes, float* d_out,
                               uint8_t* d_state, hipStream_t stream, ppf_depth_history_stats& st) {
  if (!h) return fail(PPF_ERR_INVALID, "%s: the history is NULL", who);
  if (!d_out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  DepthArgs a;
  StageBuf image;
  ppf_status s = depth_image_check(who, d_depth, h->rows, h->cols, row_pitch_bytes, &h->dp, DEPTH_FLAGS_IGNORED, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const size_t n = (size_t)h->rows * (size_t)h->cols;
  if ((s = depth_bind_device(who, d_depth, h->dp.format, &a, &image)) != PPF_OK ||
      (s = depth_outputs_check(who, image, {{"output", d_out, n * sizeof(float), nullptr}, {"state image", d_state, n, nullptr}})) != PPF_OK)
    return s;
  std::lock_guard<std::mutex> lock(h->mu);
  const HistoryArgs ha = history_args(h, a, d_out, d_state);
  int32_t c[DH_N_COUNTERS];
  s = stage_finish(who, history_enqueue(h, a, ha, stream), stream, {{"counters", ha.counters, sizeof(c), c}});
  if (s != PPF_OK) return s;
  history_fill_stats(st, c, h);
  h->t++;
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_depth_history_params(ppf_depth_history_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->window = 8;
  p->range_abs = 0.01f;
  p->range_quad = 0.f;
  p->min_support = 1;
  p->max_age = 7;
  p->flags = 0;
}

ppf_status ppf_depth_history_create(int rows, int cols, const ppf_depth_params* dp, const ppf_depth_history_params* hp,
                                    ppf_depth_history** out) {
  static const char* who = "ppf_depth_history_create";
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!hp) return fail(PPF_ERR_INVALID, "%s: the history params are NULL", who);
  /* rows, cols and dp as every push will have them checked, without an image */
  if (!dp) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  ppf_status s;
  if ((s = depth_size_check(who, rows, cols, dp)) != PPF_OK || (s = depth_scale_check(who, dp)) != PPF_OK ||
      (s = depth_z_check(who, dp)) != PPF_OK)
    return s;
  if (hp->window < 1 || hp->window > PPF_HISTORY_MAX_WINDOW)
    return fail(PPF_ERR_INVALID, "%s: window %d is outside 1..%d", who, hp->window, PPF_HISTORY_MAX_WINDOW);
  if (!std::isfinite(hp->range_abs) || !(hp->range_abs > 0.f)) return fail(PPF_ERR_INVALID, "%s: range_abs must be finite and > 0", who);
  if (!(std::isfinite(hp->range_quad) && hp->range_quad >= 0.f)) return fail(PPF_ERR_INVALID, "%s: range_quad must be finite and >= 0", who);
  if (hp->min_support < 1 || hp->min_support > hp->window)
    return fail(PPF_ERR_INVALID, "%s: min_support %d is outside 1..window (%d)", who, hp->min_support, hp->window);
  if (hp->max_age < 0 || hp->max_age > PPF_HISTORY_MAX_AGE)
    return fail(PPF_ERR_INVALID, "%s: max_age %d is outside 0..%d", who, hp->max_age, PPF_HISTORY_MAX_AGE);
  if (hp->flags & ~PPF_HISTORY_MEAN) return fail(PPF_ERR_INVALID, "%s: unknown history flags 0x%x", who, (unsigned)hp->flags);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  std::unique_ptr<ppf_depth_history> h(new (std::nothrow) ppf_depth_history());
  if (!h) return fail(PPF_ERR_NOMEM, "%s: out of host memory", who);
  h->rows = rows;
  h->cols = cols;
  h->dp = *dp;
  h->hp = *hp;
  h->plane = (size_t)rows * (size_t)((cols + DH_PX - 1) / DH_PX) * DH_PX;
  const hipError_t e = h->ring.reserve(h->plane * (size_t)hp->window);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(PPF_ERR_NOMEM, "%s: a ring of %d planes of %d x %d pixels (%zu bytes) cannot be allocated: %s", who, hp->window, rows, cols,
                h->plane * (size_t)hp->window * sizeof(float), hipGetErrorString(e));
  }
  HIPCHK(h->counters.reserve(DH_N_COUNTERS));
  *out = h.release();
  return PPF_OK;
}

ppf_status ppf_depth_history_push(ppf_depth_history* h, const void* depth, size_t row_pitch_bytes, float* out, uint8_t* state,
                                  ppf_depth_history_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_history_stats>, [&](ppf_depth_history_stats& st) {
    return history_push_host("ppf_depth_history_push", h, depth, row_pitch_bytes, out, state, st);
  });
}

ppf_status ppf_depth_history_push_device(ppf_depth_history* h, const void* d_depth, size_t row_pitch_bytes, float* d_out, uint8_t* d_state,
                                         void* stream, ppf_depth_history_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_history_stats>, [&](ppf_depth_history_stats& st) {
    return history_push_device("ppf_depth_history_push_device", h, d_depth, row_pitch_bytes, d_out, d_state, static_cast<hipStream_t>(stream), st);
  });
}

ppf_status ppf_depth_history_reset(ppf_depth_history* h) {
  if (!h) return fail(PPF_ERR_INVALID, "ppf_depth_history_reset: the history is NULL");
  std::lock_guard<std::mutex> lock(h->mu);
  h->t = 0;
  return PPF_OK;
}

ppf_status ppf_depth_history_info(const ppf_depth_history* h, ppf_depth_history_desc* info) {
  if (info) std::memset(info, 0, sizeof(*info));
  if (!h || !info) return fail(PPF_ERR_INVALID, "ppf_depth_history_info: the history and info must not be NULL");
  std::lock_guard<std::mutex> lock(const_cast<ppf_depth_history*>(h)->mu);
  info->rows = h->rows;
  info->cols = h->cols;
  info->window = h->hp.window;
  info->frames = h->t;
  info->device_bytes = h->ring.bytes() + h->counters.bytes();
  return PPF_OK;
}

ppf_status ppf_depth_history_release(ppf_depth_history* h) {
  delete h; /* every push has waited for its kernel: the ring goes back to the block cache */
  return PPF_OK;
}

}  // extern "C"

#endif /* PPF_HISTORY_HOST_H */
