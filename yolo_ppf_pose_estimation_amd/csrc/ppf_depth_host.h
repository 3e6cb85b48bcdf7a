/*
 * ppf_depth_host.h — host side of ppf_cloud_from_depth / ppf_cloud_from_depth_device: the scene cloud from a depth image,
 * resident in HBM (what the reference's CloudProcessor::Deprojection, CloudProcessing.h:262, leaves empty).  Kernels:
 * ppf_depth_kernels.h.  Included by ppf_hip.hip after ppf_prep_host.h (ppf_cloud, cloud_alloc, grid_for).
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

size_t depth_elem_size(int format) { return format == PPF_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float); }

/* every argument check of both entries, before any device work; fills the kernel arguments (img and pitch excepted) */
ppf_status depth_check(const char* who, const void* depth, int rows, int cols, size_t* pitch, const double* intr,
                       const ppf_depth_params* p, ppf_cloud** out, DepthArgs* a) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!depth || !intr || !p) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  if (rows <= 0 || cols <= 0) return fail(PPF_ERR_INVALID, "%s: the image is %d x %d", who, rows, cols);
  if ((long long)rows * cols > 0x7fffffffLL) return fail(PPF_ERR_INVALID, "%s: %d x %d pixels exceed INT32_MAX", who, rows, cols);
  if (p->format != PPF_DEPTH_F32 && p->format != PPF_DEPTH_U16) return fail(PPF_ERR_INVALID, "%s: unknown depth format %d", who, p->format);
  if (p->flags & ~PPF_DEPTH_FP64) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  const size_t es = depth_elem_size(p->format), width = (size_t)cols * es;
  if (*pitch == 0) *pitch = width;
  if (*pitch < width || *pitch % es != 0)
    return fail(PPF_ERR_INVALID, "%s: row pitch %zu bytes is below %zu or not a multiple of %zu", who, *pitch, width, es);
  if (*pitch > (SIZE_MAX - width) / (size_t)rows) return fail(PPF_ERR_INVALID, "%s: row pitch %zu bytes is too large", who, *pitch);
  if ((uintptr_t)depth % es != 0) return fail(PPF_ERR_INVALID, "%s: the image is not aligned to its %zu-byte elements", who, es);
  if (p->format == PPF_DEPTH_U16 && !(p->depth_scale > 0.0 && std::isfinite(p->depth_scale)))
    return fail(PPF_ERR_INVALID, "%s: depth_scale must be positive and finite for PPF_DEPTH_U16", who);
  const double fx = intr[0], fy = intr[1], ppx = intr[2], ppy = intr[3];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0)
    return fail(PPF_ERR_INVALID, "%s: fx and fy must be finite and non-zero", who);
  if (!std::isfinite(ppx) || !std::isfinite(ppy)) return fail(PPF_ERR_INVALID, "%s: ppx and ppy must be finite", who);
  if (!std::isfinite(p->z_min) || !std::isfinite(p->z_max) || p->z_max < 0.f)
    return fail(PPF_ERR_INVALID, "%s: z_min and z_max must be finite and z_max >= 0", who);
  a->img = nullptr;
  a->pitch = *pitch;
  a->cols = cols;
  a->n = rows * cols;
  a->fx = fx; a->fy = fy; a->ppx = ppx; a->ppy = ppy;
  a->scale = p->depth_scale;
  a->z_min = p->z_min;
  a->z_max = p->z_max;
  a->fp64 = (p->flags & PPF_DEPTH_FP64) ? 1 : 0;
  return PPF_OK;
}

/* `bytes` from d_ptr on must be memory the current device can read directly, inside one allocation; `what` names the buffer */
ppf_status depth_device_range(const char* who, const char* what, const void* d_ptr, size_t bytes) {
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  const hipError_t pe = hipPointerGetAttributes(&attr, d_ptr);
  if (pe != hipSuccess) {
    (void)hipGetLastError(); /* the query's error is the answer, not a sticky state */
    return fail(PPF_ERR_INVALID, "%s: the %s pointer is not device memory (%s)", who, what, hipGetErrorString(pe));
  }
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
    return fail(PPF_ERR_INVALID, "%s: the %s pointer is not device memory (memory type %d)", who, what, (int)attr.type);
  if (attr.device != dev) return fail(PPF_ERR_INVALID, "%s: the %s lives on device %d, the current device is %d", who, what, attr.device, dev);
  hipDeviceptr_t base = nullptr;
  size_t alloc = 0;
  const hipError_t re = hipMemGetAddressRange(&base, &alloc, const_cast<void*>(d_ptr));
  if (re != hipSuccess) {
    (void)hipGetLastError();
    return fail(PPF_ERR_INVALID, "%s: the %s's allocation is unknown (%s)", who, what, hipGetErrorString(re));
  }
  const uintptr_t lo = (uintptr_t)base, at = (uintptr_t)d_ptr;
  if (at < lo || at - lo > alloc || bytes > alloc - (at - lo))
    return fail(PPF_ERR_INVALID, "%s: the %s (%zu bytes) runs past the end of its allocation", who, what, bytes);
  return PPF_OK;
}

/* count -> scan -> one read-back -> allocate -> scatter, all on `st`; returns once the cloud is complete */
ppf_status depth_run(const DepthArgs& a, int format, hipStream_t st, ppf_cloud** out) {
  const int n_tiles = (int)(((size_t)a.n + DEPTH_TILE - 1) / DEPTH_TILE);
  DevBuf<uint32_t> counts, offs;
  HIPCHK(counts.reserve((size_t)n_tiles + 1));
  HIPCHK(offs.reserve((size_t)n_tiles + 1));
  if (format == PPF_DEPTH_U16)
    k_depth_count<uint16_t><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, n_tiles, counts.p);
  else
    k_depth_count<float><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, n_tiles, counts.p);
  HIPCHK(hipGetLastError());
  ppf_status s = device_exclusive_scan(counts.p, offs.p, (size_t)n_tiles + 1, st);
  if (s != PPF_OK) return s;
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, offs.p + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(host_stream_sync(st));
  std::unique_ptr<ppf_cloud> c;
  if ((s = cloud_alloc(c, (int)total)) != PPF_OK) return s;
  if (total) {
    if (format == PPF_DEPTH_U16)
      k_depth_scatter<uint16_t><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, offs.p, c->rows.p, c->curv.p);
    else
      k_depth_scatter<float><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, offs.p, c->rows.p, c->curv.p);
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
  if (format == PPF_DEPTH_U16)
    k_depth_normals<uint16_t><<<dim3((unsigned)n_win), dim3(DN_BLOCK), 0, st>>>(a, na, nrm.p, flag.p);
  else
    k_depth_normals<float><<<dim3((unsigned)n_win), dim3(DN_BLOCK), 0, st>>>(a, na, nrm.p, flag.p);
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
    if (format == PPF_DEPTH_U16)
      k_depthn_scatter<uint16_t><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, flag.p, na.drop, nrm.p, offs.p, c->rows.p, c->curv.p);
    else
      k_depthn_scatter<float><<<dim3((unsigned)n_tiles), dim3(DEPTH_BLOCK), 0, st>>>(a, flag.p, na.drop, nrm.p, offs.p, c->rows.p, c->curv.p);
    HIPCHK(hipGetLastError());
    HIPCHK(host_stream_sync(st)); /* the scratch goes back to the block cache at scope exit */
  }
  *out = c.release();
  return PPF_OK;
}

/* the image of a host entry goes over packed: rows of cols elements */
ppf_status depth_upload(const void* depth, int rows, int cols, size_t pitch, int format, DevBuf<unsigned char>& img, DepthArgs* a) {
  const size_t width = (size_t)cols * depth_elem_size(format);
  HIPCHK(img.reserve(width * (size_t)rows));
  if (pitch == width)
    HIPCHK(hipMemcpy(img.p, depth, width * (size_t)rows, hipMemcpyHostToDevice));
  else
    HIPCHK(hipMemcpy2D(img.p, width, depth, pitch, width, (size_t)rows, hipMemcpyHostToDevice));
  a->img = img.p;
  a->pitch = width;
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
  size_t pitch = row_pitch_bytes;
  ppf_status s = depth_check(who, depth, rows, cols, &pitch, intr, p, out, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  DevBuf<unsigned char> img;
  if ((s = depth_upload(depth, rows, cols, pitch, p->format, img, &a)) != PPF_OK) return s;
  return depth_run(a, p->format, nullptr, out);
}

ppf_status ppf_cloud_from_depth_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                       const ppf_depth_params* p, void* stream, ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth_device";
  DepthArgs a;
  size_t pitch = row_pitch_bytes;
  ppf_status s = depth_check(who, d_depth, rows, cols, &pitch, intr, p, out, &a);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  /* only memory the current device can read directly, and the whole image inside its allocation */
  const size_t bytes = (size_t)(rows - 1) * pitch + (size_t)cols * depth_elem_size(p->format);
  if ((s = depth_device_range(who, "image", d_depth, bytes)) != PPF_OK) return s;
  a.img = static_cast<const unsigned char*>(d_depth);
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
  size_t pitch = row_pitch_bytes;
  ppf_status s = depth_check(who, depth, rows, cols, &pitch, intr, p, out, &a);
  if (s != PPF_OK || (s = depth_normal_check(who, np, rows, cols, &na)) != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  DevBuf<unsigned char> img;
  if ((s = depth_upload(depth, rows, cols, pitch, p->format, img, &a)) != PPF_OK) return s;
  return depth_normals_run(a, na, p->format, nullptr, out);
}

ppf_status ppf_cloud_from_depth_normals_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                               const ppf_depth_params* p, const ppf_depth_normal_params* np, void* stream,
                                               ppf_cloud** out) {
  static const char* who = "ppf_cloud_from_depth_normals_device";
  DepthArgs a;
  DepthNormalArgs na;
  size_t pitch = row_pitch_bytes;
  ppf_status s = depth_check(who, d_depth, rows, cols, &pitch, intr, p, out, &a);
  if (s != PPF_OK || (s = depth_normal_check(who, np, rows, cols, &na)) != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const size_t bytes = (size_t)(rows - 1) * pitch + (size_t)cols * depth_elem_size(p->format);
  if ((s = depth_device_range(who, "image", d_depth, bytes)) != PPF_OK) return s;
  a.img = static_cast<const unsigned char*>(d_depth);
  return depth_normals_run(a, na, p->format, static_cast<hipStream_t>(stream), out);
}

}  // extern "C"

#endif /* PPF_DEPTH_HOST_H */
