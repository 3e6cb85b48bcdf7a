/*
 * ppf_depth_host.h — host side of ppf_cloud_from_depth / ppf_cloud_from_depth_device: the scene cloud from a depth image,
 * resident in HBM (what the reference's CloudProcessor::Deprojection, CloudProcessing.h:262, leaves empty).  Kernels:
 * ppf_depth_kernels.h.  Included by ppf_hip.hip after ppf_prep_host.h (ppf_cloud, cloud_alloc, grid_for) and
 * ppf_depthimage_host.h (the image checks, depth_bind_host / _device, depth_typed).
 *
 * Per call: k_depth_count, one scan launch (up to SCAN_ONE_MAX tiles, about 40 M pixels), k_depth_scatter -- three
 * launches -- one blocking 4-byte read-back of the total and a final wait for the stream.  The host entry adds one
 * host-to-device copy of the image.
 *
 * ppf_cloud_from_depth_normals / _device (kernels: ppf_depth_normals_kernels.h) put k_depth_normals in
 * front and run the same pattern on its flags: four launches, the same read-back and final wait.
 */
#ifndef PPF_DEPTH_HOST_H
#define PPF_DEPTH_HOST_H

namespace {

/* every argument check of the cloud entries, before any device work; fills the kernel arguments (img excepted) */
ppf_status cloud_depth_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const double* intr,
                             const ppf_depth_params* p, ppf_cloud** out, DepthArgs* a) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!intr) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  ppf_status s = depth_pixels_check(who, depth, rows, cols, pitch, p, DEPTH_FLAGS_FP64, a);
  if (s != PPF_OK || (s = depth_intr_check(who, intr, a)) != PPF_OK) return s;
  return depth_z_check(who, p);
}

/* count -> scan -> one read-back -> allocate -> scatter, all on `st`; returns once the cloud is complete */
ppf_status depth_run(const DepthArgs& a, int format, hipStream_t st, ppf_cloud** out) {
  const int n_tiles = (int)(((size_t)a.n + DEPTH_TILE - 1) / DEPTH_TILE);
  DevBuf<uint32_t> counts, offs;
  HIPCHK(counts.reserve((size_t)n_tiles + 1));
  HIPCHK(offs.reserve((size_t)n_tiles + 1));
  depth_typed(format, [&](auto px) { k_depth_count<decltype(px)><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, n_tiles, counts.p); });
  HIPCHK(hipGetLastError());
  ppf_status s = device_exclusive_scan(counts.p, offs.p, (size_t)n_tiles + 1, st);
  if (s != PPF_OK) return s;
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, offs.p + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(host_stream_sync(st));
  std::unique_ptr<ppf_cloud> c;
  if ((s = cloud_alloc(c, (int)total)) != PPF_OK) return s;
  if (total) {
    depth_typed(format, [&](auto px) {
      k_depth_scatter<decltype(px)><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, offs.p, c->rows.p, c->curv.p);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(host_stream_sync(st)); /* the scratch goes back to the block cache at scope exit */
  }
  *out = c.release();
  return PPF_OK;
}

/* the checks ppf_cloud_from_depth_normals adds, before any device work; fills the kernel's arguments */
ppf_status depth_normal_check(const char* who, const ppf_depth_normal_params* np, int rows, int cols, DepthNormalArgs* na) {
  if (!np) return fail(PPF_ERR_INVALID, "%s: the normal params must not be NULL", who);
  if (np->radius < 1 || np->radius > PPF_DEPTH_NORMALS_MAX_RADIUS)
    return fail(PPF_ERR_INVALID, "%s: radius %d is outside 1..%d", who, np->radius, PPF_DEPTH_NORMALS_MAX_RADIUS);
  if (!std::isfinite(np->max_depth_change) || !(np->max_depth_change > 0.f))
    return fail(PPF_ERR_INVALID, "%s: max_depth_change must be finite and > 0", who);
  const int side = 2 * np->radius + 1;
  if (np->min_neighbours < 3 || np->min_neighbours > side * side)
    return fail(PPF_ERR_INVALID, "%s: min_neighbours %d is outside 3..%d", who, np->min_neighbours, side * side);
  if (np->flags & ~PPF_DEPTH_NORMALS_DROP) return fail(PPF_ERR_INVALID, "%s: unknown normal flags 0x%x", who, (unsigned)np->flags);
  na->rows = rows;
  na->tiles_x = (int)(((long long)cols + DN_TILE_W - 1) / DN_TILE_W);
  na->radius = np->radius;
  na->min_neighbours = np->min_neighbours;
  na->max_depth_change = np->max_depth_change;
  na->drop = (np->flags & PPF_DEPTH_NORMALS_DROP) ? 1 : 0;
  return PPF_OK;
}

/* k_depth_normals into pixel-indexed scratch, then depth_run's pattern on its flags: four launches, the same read-back */
ppf_status depth_normals_run(const DepthArgs& a, const DepthNormalArgs& na, int format, hipStream_t st, ppf_cloud** out) {
  const int n_tiles = (int)(((size_t)a.n + DEPTH_TILE - 1) / DEPTH_TILE);
  /* at most n / 256 + rows / 4 + cols / 64 + 1 workgroups: below 2^31 for every n <= INT32_MAX */
  const long long n_win = (long long)na.tiles_x * (((long long)na.rows + DN_TILE_H - 1) / DN_TILE_H);
  DevBuf<float4> nrm;
  DevBuf<uint8_t> flag;
  DevBuf<uint32_t> counts, offs;
  HIPCHK(nrm.reserve((size_t)a.n));
  HIPCHK(flag.reserve((size_t)a.n));
  HIPCHK(counts.reserve((size_t)n_tiles + 1));
  HIPCHK(offs.reserve((size_t)n_tiles + 1));
  depth_typed(format, [&](auto px) { k_depth_normals<decltype(px)><<<dim3((unsigned)n_win), dim3(DN_BLOCK), 0, st>>>(a, na, nrm.p, flag.p); });
  HIPCHK(hipGetLastError());
  k_depthn_count<<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(flag.p, a.n, na.drop, n_tiles, counts.p);
  HIPCHK(hipGetLastError());
  ppf_status s = device_exclusive_scan(counts.p, offs.p, (size_t)n_tiles + 1, st);
  if (s != PPF_OK) return s;
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, offs.p + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(host_stream_sync(st));
  std::unique_ptr<ppf_cloud> c;
  if ((s = cloud_alloc(c, (int)total)) != PPF_OK) return s;
  if (total) {
    depth_typed(format, [&](auto px) {
      k_depthn_scatter<decltype(px)><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, flag.p, na.drop, nrm.p, offs.p, c->rows.p, c->curv.p);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(host_stream_sync(st)); /* the scratch goes back to the block cache at scope exit */
  }
  *out = c.release();
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_depth_params(ppf_depth_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->format = PPF_DEPTH_F32;
  p->flags = 0;
  p->depth_scale = 0.001;
  p->z_min = 0.f;
  p->z_max = 0.f;
}

ppf_status ppf_cloud_from_depth(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                const ppf_depth_params* p, ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth";
  DepthArgs a;
  ppf_status s = cloud_depth_check(who, depth, rows, cols, row_pitch_bytes, intr, p, out, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  DevBuf<unsigned char> img;
  if ((s = depth_bind_host(depth, p->format, img, &a)) != PPF_OK) return s;
  return depth_run(a, p->format, nullptr, out);
}

ppf_status ppf_cloud_from_depth_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                       const ppf_depth_params* p, void* stream, ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth_device";
  DepthArgs a;
  StageBuf image;
  ppf_status s = cloud_depth_check(who, d_depth, rows, cols, row_pitch_bytes, intr, p, out, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = depth_bind_device(who, d_depth, p->format, &a, &image)) != PPF_OK) return s;
  return depth_run(a, p->format, static_cast<hipStream_t>(stream), out);
}

void ppf_default_depth_normal_params(ppf_depth_normal_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius = 3;
  p->max_depth_change = 0.02f;
  p->min_neighbours = 3;
  p->flags = 0;
}

ppf_status ppf_cloud_from_depth_normals(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                        const ppf_depth_params* p, const ppf_depth_normal_params* np, ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth_normals";
  DepthArgs a;
  DepthNormalArgs na;
  ppf_status s = cloud_depth_check(who, depth, rows, cols, row_pitch_bytes, intr, p, out, &a);
  if (s != PPF_OK || (s = depth_normal_check(who, np, rows, cols, &na)) != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  DevBuf<unsigned char> img;
  if ((s = depth_bind_host(depth, p->format, img, &a)) != PPF_OK) return s;
  return depth_normals_run(a, na, p->format, nullptr, out);
}

ppf_status ppf_cloud_from_depth_normals_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                               const ppf_depth_params* p, const ppf_depth_normal_params* np, void* stream,
                                               ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth_normals_device";
  DepthArgs a;
  DepthNormalArgs na;
  StageBuf image;
  ppf_status s = cloud_depth_check(who, d_depth, rows, cols, row_pitch_bytes, intr, p, out, &a);
  if (s != PPF_OK || (s = depth_normal_check(who, np, rows, cols, &na)) != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if ((s = depth_bind_device(who, d_depth, p->format, &a, &image)) != PPF_OK) return s;
  return depth_normals_run(a, na, p->format, static_cast<hipStream_t>(stream), out);
}

}  // extern "C"

#endif /* PPF_DEPTH_HOST_H */
