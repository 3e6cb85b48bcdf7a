/*
 * ppf_register_host.h — host side of the camera entries (ppf_camera_project / _unproject / _map_boxes, host only), of
 * ppf_depth_map and of ppf_depth_register / ppf_depth_register_device: a raw sensor depth image aligned to the colour
 * camera.  Kernels: ppf_register_kernels.h; arithmetic: include/ppf_camera_math.h.  Included by
 * ppf_hip.hip after ppf_depthimage_host.h (the image check, the bindings, depth_outputs_check, stage_finish, stage_entry,
 * depth_typed).
 *
 * Per call: k_reg_clear, k_reg_draw, k_reg_resolve -- three launches -- and one blocking wait, whatever the sizes.  The
 * host entry adds one upload of the image and reads the image and the counters back behind that one wait.  Scratch (the
 * uploaded image, the z-buffer, the counters) comes from the block cache; the device entry draws in d_out itself.
 */
#ifndef PPF_REGISTER_HOST_H
#define PPF_REGISTER_HOST_H

struct ppf_depth_map {
  ppf_camera dcam, ccam;
  int d_rows = 0, d_cols = 0, c_rows = 0, c_cols = 0;
  double R[9], t[3];
  DevBuf<double> rays; /* [d_rows][d_cols][2] */
};

namespace {

ppf_status camera_check(const ppf_camera* c, const char* name, const char* who) {
  if (!c) return fail(PPF_ERR_INVALID, "%s: %s is NULL", who, name);
  if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || c->fx == 0.0 || c->fy == 0.0)
    return fail(PPF_ERR_INVALID, "%s: %s: fx and fy must be finite and non-zero", who, name);
  if (!std::isfinite(c->cx) || !std::isfinite(c->cy)) return fail(PPF_ERR_INVALID, "%s: %s: cx and cy must be finite", who, name);
  const double k[8] = {c->k1, c->k2, c->p1, c->p2, c->k3, c->k4, c->k5, c->k6};
  for (double v : k)
    if (!std::isfinite(v)) return fail(PPF_ERR_INVALID, "%s: %s: a distortion coefficient is not finite", who, name);
  if (!(std::isfinite(c->max_r) && c->max_r >= 0.0)) return fail(PPF_ERR_INVALID, "%s: %s: max_r must be finite and >= 0", who, name);
  for (double v : c->reserved)
    if (!(v == 0.0)) return fail(PPF_ERR_INVALID, "%s: %s: reserved must be 0", who, name);
  return PPF_OK;
}

/* project (unproject == false) or unproject n points; on an argument error the reachable outputs are NaN and 0 */
ppf_status camera_points(const ppf_camera* cam, const double* in, int n, double* out, uint8_t* valid, bool unproject, const char* who) {
  if (n > 0 && out)
    for (size_t i = 0; i < (size_t)n * 2; i++) out[i] = ppf_cam_nan();
  if (n > 0 && valid) std::memset(valid, 0, (size_t)n);
  if (n < 0) return fail(PPF_ERR_INVALID, "%s: n is %d", who, n);
  if (!in || !out) return fail(PPF_ERR_INVALID, "%s: the point arrays must not be NULL", who);
  ppf_status s = camera_check(cam, "cam", who);
  if (s != PPF_OK) return s;
  for (int i = 0; i < n; i++) {
    const double a = in[2 * (size_t)i], b = in[2 * (size_t)i + 1]; /* in and out may be one array */
    const int ok = unproject ? ppf_cam_unproject(cam, a, b, &out[2 * (size_t)i], &out[2 * (size_t)i + 1])
                             : ppf_cam_project(cam, a, b, &out[2 * (size_t)i], &out[2 * (size_t)i + 1]);
    if (valid) valid[i] = (uint8_t)ok;
  }
  return PPF_OK;
}

ppf_status register_check(const char* who, const ppf_depth_map* map, const void* depth, size_t pitch, const ppf_depth_params* dp,
                          const ppf_register_params* rp, const float* out, DepthArgs* a) {
  if (!map) return fail(PPF_ERR_INVALID, "%s: map is NULL", who);
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  if (!rp) return fail(PPF_ERR_INVALID, "%s: the register params are NULL", who);
  /* the image has the map's size */
  ppf_status s = depth_image_check(who, depth, map->d_rows, map->d_cols, pitch, dp, DEPTH_FLAGS_ZERO, a);
  if (s != PPF_OK) return s;
  if (!(std::isfinite(rp->quad_dz_abs) && rp->quad_dz_abs >= 0.f) || !(std::isfinite(rp->quad_dz_rel) && rp->quad_dz_rel >= 0.f))
    return fail(PPF_ERR_INVALID, "%s: quad_dz_abs and quad_dz_rel must be finite and >= 0", who);
  if (rp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)rp->flags);
  return PPF_OK;
}

ppf_status register_device_of(const char* who, const ppf_depth_map* map) {
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (dev != map->rays.device) return fail(PPF_ERR_INVALID, "%s: the map lives on device %d, the current device is %d", who, map->rays.device, dev);
  return PPF_OK;
}

/* clear -> draw -> resolve on `st`, zbuf and out being one buffer or two; a.d.img and a.d.pitch are set by the caller */
ppf_status register_enqueue(const ppf_depth_map* map, RegArgs& a, int format, const ppf_register_params* rp, uint32_t* zbuf, float* d_out,
                            int32_t* counters, hipStream_t st) {
  a.d_rows = map->d_rows;
  a.rays = map->rays.p;
  std::memcpy(a.R, map->R, sizeof(a.R));
  std::memcpy(a.t, map->t, sizeof(a.t));
  a.cc = map->ccam;
  a.c_rows = map->c_rows;
  a.c_cols = map->c_cols;
  a.dz_abs = rp->quad_dz_abs;
  a.dz_rel = rp->quad_dz_rel;
  a.zbuf = zbuf;
  a.counters = counters;
  a.tiles_x = (map->d_cols + REG_TILE - 1) / REG_TILE;
  const size_t n_out = (size_t)map->c_rows * map->c_cols;
  const unsigned out_blocks = (unsigned)((n_out + REG_BLOCK - 1) / REG_BLOCK);
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((map->d_rows + REG_TILE - 1) / REG_TILE);
  k_reg_clear<<<dim3(out_blocks), dim3(REG_BLOCK), 0, st>>>(zbuf, n_out, counters);
  depth_typed(format, [&](auto px) { k_reg_draw<decltype(px)><<<dim3(tiles), dim3(REG_BLOCK), 0, st>>>(a); });
  k_reg_resolve<<<dim3(out_blocks), dim3(REG_BLOCK), 0, st>>>(zbuf, d_out, n_out, counters);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

void register_fill_stats(ppf_register_stats& st, const int32_t* c) {
  st.n_vertices = c[REG_C_VERTICES];
  st.n_quads = c[REG_C_QUADS];
  st.n_quads_cut = c[REG_C_CUT];
  st.n_quads_oversize = c[REG_C_OVERSIZE];
  st.n_filled = c[REG_C_FILLED];
  st.n_launches = 3;
  st.n_host_syncs = 1;
}

ppf_status register_host(const char* who, const ppf_depth_map* map, const void* depth, size_t row_pitch_bytes, const ppf_depth_params* dp,
                         const ppf_register_params* rp, float* out, ppf_register_stats& st) {
  RegArgs a;
  ppf_status s = register_check(who, map, depth, row_pitch_bytes, dp, rp, out, &a.d);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = register_device_of(who, map)) != PPF_OK) return s;
  const size_t n_out = (size_t)map->c_rows * map->c_cols;
  DevBuf<unsigned char> img;
  DevBuf<uint32_t> buf; /* the z-buffer, resolved in place, then the counters */
  if ((s = depth_bind_host(depth, dp->format, img, &a.d)) != PPF_OK) return s;
  HIPCHK(buf.reserve(n_out + REG_N_COUNTERS));
  int32_t* counters = reinterpret_cast<int32_t*>(buf.p + n_out);
  int32_t c[REG_N_COUNTERS];
  s = stage_finish(who, register_enqueue(map, a, dp->format, rp, buf.p, reinterpret_cast<float*>(buf.p), counters, nullptr), nullptr,
                   {{"output", buf.p, n_out * sizeof(float), out}, {"counters", counters, sizeof(c), c}});
  if (s == PPF_OK) register_fill_stats(st, c);
  return s;
}

ppf_status register_device(const char* who, const ppf_depth_map* map, const void* d_depth, size_t row_pitch_bytes,
                           const ppf_depth_params* dp, const ppf_register_params* rp, float* d_out, hipStream_t stream,
                           ppf_register_stats& st) {
  RegArgs a;
  StageBuf image;
  ppf_status s = register_check(who, map, d_depth, row_pitch_bytes, dp, rp, d_out, &a.d);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = register_device_of(who, map)) != PPF_OK || (s = depth_bind_device(who, d_depth, dp->format, &a.d, &image)) != PPF_OK ||
      (s = depth_outputs_check(who, image, {{"output", d_out, (size_t)map->c_rows * map->c_cols * sizeof(float), nullptr}})) != PPF_OK)
    return s;
  DevBuf<int32_t> counters;
  HIPCHK(counters.reserve(REG_N_COUNTERS));
  int32_t c[REG_N_COUNTERS];
  s = stage_finish(who, register_enqueue(map, a, dp->format, rp, reinterpret_cast<uint32_t*>(d_out), d_out, counters.p, stream), stream,
                   {{"counters", counters.p, sizeof(c), c}});
  if (s == PPF_OK) register_fill_stats(st, c);
  return s;
}

}  // namespace

extern "C" {

void ppf_default_camera(ppf_camera* cam, double fx, double fy, double cx, double cy) {
  if (!cam) return;
  std::memset(cam, 0, sizeof(*cam));
  cam->fx = fx;
  cam->fy = fy;
  cam->cx = cx;
  cam->cy = cy;
}

ppf_status ppf_camera_project(const ppf_camera* cam, const double* xy, int n, double* uv, uint8_t* valid) {
  return camera_points(cam, xy, n, uv, valid, false, "ppf_camera_project");
}

ppf_status ppf_camera_unproject(const ppf_camera* cam, const double* uv, int n, double* xy, uint8_t* valid) {
  return camera_points(cam, uv, n, xy, valid, true, "ppf_camera_unproject");
}

ppf_status ppf_camera_map_boxes(const ppf_camera* from, const ppf_camera* to, int to_rows, int to_cols, const int* boxes_xywh, int n,
                                int* out_xywh) {
  static const char* who = "ppf_camera_map_boxes";
  if (n > 0 && out_xywh) std::memset(out_xywh, 0, (size_t)n * 4 * sizeof(int));
  if (n < 0) return fail(PPF_ERR_INVALID, "%s: n is %d", who, n);
  if (!boxes_xywh || !out_xywh) return fail(PPF_ERR_INVALID, "%s: the box arrays must not be NULL", who);
  if (to_rows <= 0 || to_cols <= 0) return fail(PPF_ERR_INVALID, "%s: the image is %d x %d", who, to_rows, to_cols);
  ppf_status s;
  if ((s = camera_check(from, "from", who)) != PPF_OK || (s = camera_check(to, "to", who)) != PPF_OK) return s;
  for (int i = 0; i < n; i++) {
    const int* b = boxes_xywh + 4 * (size_t)i;
    const double xs[3] = {(double)b[0], (double)b[0] + (double)b[2] / 2.0, (double)b[0] + (double)b[2]};
    const double ys[3] = {(double)b[1], (double)b[1] + (double)b[3] / 2.0, (double)b[1] + (double)b[3]};
    double u0 = 0, u1 = 0, v0 = 0, v1 = 0;
    bool any = false;
    for (int iy = 0; iy < 3; iy++)
      for (int ix = 0; ix < 3; ix++) {
        if (ix == 1 && iy == 1) continue; /* corners and side midpoints, not the centre */
        double x, y, u, v;
        if (!ppf_cam_unproject(from, xs[ix], ys[iy], &x, &y) || !ppf_cam_project(to, x, y, &u, &v)) continue;
        if (!any) { u0 = u1 = u; v0 = v1 = v; any = true; }
        u0 = u < u0 ? u : u0;
        u1 = u > u1 ? u : u1;
        v0 = v < v0 ? v : v0;
        v1 = v > v1 ? v : v1;
      }
    if (!any) continue;
    /* outwards, then clamped to the image as doubles: the conversions cannot overflow */
    u0 = std::floor(u0); u1 = std::ceil(u1); v0 = std::floor(v0); v1 = std::ceil(v1);
    const double W = (double)to_cols, H = (double)to_rows;
    u0 = u0 < 0.0 ? 0.0 : (u0 > W ? W : u0);
    u1 = u1 < 0.0 ? 0.0 : (u1 > W ? W : u1);
    v0 = v0 < 0.0 ? 0.0 : (v0 > H ? H : v0);
    v1 = v1 < 0.0 ? 0.0 : (v1 > H ? H : v1);
    if (u1 - u0 <= 0.0 || v1 - v0 <= 0.0) continue;
    int* o = out_xywh + 4 * (size_t)i;
    o[0] = (int)u0;
    o[1] = (int)v0;
    o[2] = (int)(u1 - u0);
    o[3] = (int)(v1 - v0);
  }
  return PPF_OK;
}

ppf_status ppf_depth_map_create(const ppf_camera* depth_cam, int depth_rows, int depth_cols, const ppf_camera* color_cam,
                                int color_rows, int color_cols, const double* R9, const double* t3, ppf_depth_map** out) {
  static const char* who = "ppf_depth_map_create";
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  ppf_status s;
  if ((s = camera_check(depth_cam, "depth_cam", who)) != PPF_OK || (s = camera_check(color_cam, "color_cam", who)) != PPF_OK) return s;
  if (!R9 || !t3) return fail(PPF_ERR_INVALID, "%s: R9 and t3 must not be NULL", who);
  if (depth_rows <= 0 || depth_cols <= 0 || color_rows <= 0 || color_cols <= 0)
    return fail(PPF_ERR_INVALID, "%s: the images are %d x %d and %d x %d", who, depth_rows, depth_cols, color_rows, color_cols);
  if ((long long)depth_rows * depth_cols > 0x7fffffffLL || (long long)color_rows * color_cols > 0x7fffffffLL)
    return fail(PPF_ERR_INVALID, "%s: an image exceeds INT32_MAX pixels", who);
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(R9[i])) return fail(PPF_ERR_INVALID, "%s: R9 is not finite", who);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t3[i])) return fail(PPF_ERR_INVALID, "%s: t3 is not finite", who);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  std::unique_ptr<ppf_depth_map> m(new (std::nothrow) ppf_depth_map());
  if (!m) return fail(PPF_ERR_NOMEM, "%s: out of host memory", who);
  m->dcam = *depth_cam;
  m->ccam = *color_cam;
  m->d_rows = depth_rows; m->d_cols = depth_cols; m->c_rows = color_rows; m->c_cols = color_cols;
  std::memcpy(m->R, R9, sizeof(m->R));
  std::memcpy(m->t, t3, sizeof(m->t));
  const size_t n = (size_t)depth_rows * depth_cols;
  HIPCHK(m->rays.reserve(n * 2));
  k_reg_rays<<<dim3((unsigned)((n + REG_BLOCK - 1) / REG_BLOCK)), dim3(REG_BLOCK), 0, nullptr>>>(m->dcam, depth_cols, (int)n, m->rays.p);
  HIPCHK(hipGetLastError());
  HIPCHK(host_stream_sync(nullptr));
  *out = m.release();
  return PPF_OK;
}

ppf_status ppf_depth_map_release(ppf_depth_map* map) {
  delete map; /* every call that used it has waited for its kernels: the table goes back to the block cache */
  return PPF_OK;
}

ppf_status ppf_depth_map_rays(const ppf_depth_map* map, double* rays) {
  static const char* who = "ppf_depth_map_rays";
  if (!map || !rays) return fail(PPF_ERR_INVALID, "%s: map and rays must not be NULL", who);
  HIPCHK(host_read(rays, map->rays.p, (size_t)map->d_rows * map->d_cols * 2 * sizeof(double)));
  return PPF_OK;
}

void ppf_default_register_params(ppf_register_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->quad_dz_abs = 0.02f;
  p->quad_dz_rel = 0.02f;
  p->flags = 0;
}

ppf_status ppf_depth_register(const ppf_depth_map* map, const void* depth, size_t row_pitch_bytes, const ppf_depth_params* dp,
                              const ppf_register_params* rp, float* out, ppf_register_stats* stats) {
  /* the host entry alone also leaves a failed call's out zero, when the map says how large it is */
  const auto clear = [&](ppf_register_stats& st, bool failed) {
    std::memset(&st, 0, sizeof(st));
    if (failed && map && out) std::memset(out, 0, (size_t)map->c_rows * map->c_cols * sizeof(float));
  };
  return stage_entry(stats, clear, [&](ppf_register_stats& st) {
    return register_host("ppf_depth_register", map, depth, row_pitch_bytes, dp, rp, out, st);
  });
}

ppf_status ppf_depth_register_device(const ppf_depth_map* map, const void* d_depth, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                     const ppf_register_params* rp, float* d_out, void* stream, ppf_register_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_register_stats>, [&](ppf_register_stats& st) {
    return register_device("ppf_depth_register_device", map, d_depth, row_pitch_bytes, dp, rp, d_out, static_cast<hipStream_t>(stream), st);
  });
}

}  // extern "C"

#endif /* PPF_REGISTER_HOST_H */
