/*
 * ppf_depthimage_host.h — the host front end of every stage that takes a depth image: ppf_cloud_from_depth,
 * ppf_cloud_from_depth_normals, ppf_depth_register, ppf_depth_filter, ppf_depth_segments and ppf_depth_history.  No kernel and
 * no entry of its own.  Included by ppf_hip.hip after ppf_stage_host.h (StageBuf, stage_finish, stage_entry) and ppf_prep_host.h,
 * before ppf_depth_host.h, the first of those stages.
 *
 * A stage's host or device function is, in this order: its own NULL checks, depth_image_check, its parameter checks,
 * have_device(), depth_bind_host or depth_bind_device (+ depth_outputs_check), its enqueue, stage_finish (FrameRun::finish where
 * the stage owns a FrameRun), its stats.  Its extern "C" entry is one stage_entry.  What is left in the stage's file is what only that stage knows.
 */
#ifndef PPF_DEPTHIMAGE_HOST_H
#define PPF_DEPTHIMAGE_HOST_H

namespace {

size_t depth_elem_size(int format) { return format == PPF_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float); }

/* the launch fork: f is called with a value of the image's element type, `[&](auto px) { k<decltype(px)><<<...>>>(...); }` */
template <class F>
void depth_typed(int format, F&& f) {
  if (format == PPF_DEPTH_U16)
    f(uint16_t{});
  else
    f(float{});
}

/* what a stage makes of ppf_depth_params::flags */
enum DepthFlags {
  DEPTH_FLAGS_FP64,    /* PPF_DEPTH_FP64 or nothing: the cloud entries */
  DEPTH_FLAGS_IGNORED, /* not looked at: filter, segments, history */
  DEPTH_FLAGS_ZERO     /* must be 0, said before anything about the image: register */
};

/* The three parts of the image check that need no image, which ppf_depth_history_create calls on their own: rows, cols and
 * the format; depth_scale; the z range.  p is not NULL. */
ppf_status depth_size_check(const char* who, int rows, int cols, const ppf_depth_params* p) {
  if (rows <= 0 || cols <= 0) return fail(PPF_ERR_INVALID, "%s: the image is %d x %d", who, rows, cols);
  if ((long long)rows * cols > 0x7fffffffLL) return fail(PPF_ERR_INVALID, "%s: %d x %d pixels exceed INT32_MAX", who, rows, cols);
  if (p->format != PPF_DEPTH_F32 && p->format != PPF_DEPTH_U16) return fail(PPF_ERR_INVALID, "%s: unknown depth format %d", who, p->format);
  return PPF_OK;
}

ppf_status depth_scale_check(const char* who, const ppf_depth_params* p) {
  if (p->format == PPF_DEPTH_U16 && !(p->depth_scale > 0.0 && std::isfinite(p->depth_scale)))
    return fail(PPF_ERR_INVALID, "%s: depth_scale must be positive and finite for PPF_DEPTH_U16", who);
  return PPF_OK;
}

ppf_status depth_z_check(const char* who, const ppf_depth_params* p) {
  if (!std::isfinite(p->z_min) || !std::isfinite(p->z_max) || p->z_max < 0.f)
    return fail(PPF_ERR_INVALID, "%s: z_min and z_max must be finite and z_max >= 0", who);
  return PPF_OK;
}

/* The image check up to depth_scale: pointer, size, p, format, flags, pitch (0: packed), alignment, scale.  Fills a but for
 * img; a has no camera until depth_intr_check gives it one, and its z range is only good once depth_z_check has passed. */
ppf_status depth_pixels_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const ppf_depth_params* p,
                              DepthFlags flags, DepthArgs* a) {
  if (flags == DEPTH_FLAGS_ZERO && p && p->flags != 0)
    return fail(PPF_ERR_INVALID, "%s: the depth params' flags must be 0 here (0x%x)", who, (unsigned)p->flags);
  if (!depth || !p) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  ppf_status s = depth_size_check(who, rows, cols, p);
  if (s != PPF_OK) return s;
  if (flags == DEPTH_FLAGS_FP64 && (p->flags & ~PPF_DEPTH_FP64)) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  const size_t es = depth_elem_size(p->format), width = (size_t)cols * es;
  if (pitch == 0) pitch = width;
  if (pitch < width || pitch % es != 0)
    return fail(PPF_ERR_INVALID, "%s: row pitch %zu bytes is below %zu or not a multiple of %zu", who, pitch, width, es);
  if (pitch > (SIZE_MAX - width) / (size_t)rows) return fail(PPF_ERR_INVALID, "%s: row pitch %zu bytes is too large", who, pitch);
  if ((uintptr_t)depth % es != 0) return fail(PPF_ERR_INVALID, "%s: the image is not aligned to its %zu-byte elements", who, es);
  if ((s = depth_scale_check(who, p)) != PPF_OK) return s;
  a->img = nullptr;
  a->pitch = pitch;
  a->cols = cols;
  a->n = rows * cols;
  a->fx = a->fy = 1.0;
  a->ppx = a->ppy = 0.0;
  a->scale = p->depth_scale;
  a->z_min = p->z_min;
  a->z_max = p->z_max;
  a->fp64 = (flags == DEPTH_FLAGS_FP64 && (p->flags & PPF_DEPTH_FP64)) ? 1 : 0;
  return PPF_OK;
}

/* the intrinsics of the cloud entries: between the scale and the z range, where ppf_cloud_from_depth has always had them */
ppf_status depth_intr_check(const char* who, const double* intr, DepthArgs* a) {
  const double fx = intr[0], fy = intr[1], ppx = intr[2], ppy = intr[3];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0)
    return fail(PPF_ERR_INVALID, "%s: fx and fy must be finite and non-zero", who);
  if (!std::isfinite(ppx) || !std::isfinite(ppy)) return fail(PPF_ERR_INVALID, "%s: ppx and ppy must be finite", who);
  a->fx = fx; a->fy = fy; a->ppx = ppx; a->ppy = ppy;
  return PPF_OK;
}

/* every check of an image without a camera, before any device work */
ppf_status depth_image_check(const char* who, const void* depth, int rows, int cols, size_t pitch, const ppf_depth_params* p,
                             DepthFlags flags, DepthArgs* a) {
  const ppf_status s = depth_pixels_check(who, depth, rows, cols, pitch, p, flags, a);
  return s != PPF_OK ? s : depth_z_check(who, p);
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

bool ranges_overlap(const StageBuf& p, const StageBuf& q) {
  const uintptr_t a = (uintptr_t)p.dev, b = (uintptr_t)q.dev;
  return a < b + q.bytes && b < a + p.bytes;
}

/* the image of a host entry goes over packed, rows of cols elements: a's img and pitch are the upload's */
ppf_status depth_bind_host(const void* depth, int format, DevBuf<unsigned char>& img, DepthArgs* a) {
  const size_t width = (size_t)a->cols * depth_elem_size(format), rows = (size_t)(a->n / a->cols);
  HIPCHK(img.reserve(width * rows));
  if (a->pitch == width)
    HIPCHK(hipMemcpy(img.p, depth, width * rows, hipMemcpyHostToDevice));
  else
    HIPCHK(hipMemcpy2D(img.p, width, depth, a->pitch, width, rows, hipMemcpyHostToDevice));
  a->img = img.p;
  a->pitch = width;
  return PPF_OK;
}

/* the image of a device entry is read where it is: memory the current device reads directly, whole inside its allocation */
ppf_status depth_bind_device(const char* who, const void* d_depth, int format, DepthArgs* a, StageBuf* image) {
  const size_t rows = (size_t)(a->n / a->cols);
  *image = {"image", d_depth, (rows - 1) * a->pitch + (size_t)a->cols * depth_elem_size(format), nullptr};
  a->img = static_cast<const unsigned char*>(d_depth);
  return depth_device_range(who, image->what, image->dev, image->bytes);
}

/* the outputs of a device entry: each inside its allocation, then none of them over the image or over an earlier one */
ppf_status depth_outputs_check(const char* who, const StageBuf& image, std::initializer_list<StageBuf> outs) {
  ppf_status s;
  for (const StageBuf& o : outs)
    if (o.dev && (s = depth_device_range(who, o.what, o.dev, o.bytes)) != PPF_OK) return s;
  for (const StageBuf* o = outs.begin(); o != outs.end(); ++o) {
    if (!o->dev) continue;
    if (ranges_overlap(*o, image)) return fail(PPF_ERR_INVALID, "%s: the %s overlaps the %s", who, o->what, image.what);
    for (const StageBuf* q = outs.begin(); q != o; ++q)
      if (q->dev && ranges_overlap(*o, *q)) return fail(PPF_ERR_INVALID, "%s: the %s overlaps the %s", who, o->what, q->what);
  }
  return PPF_OK;
}

}  // namespace

#endif /* PPF_DEPTHIMAGE_HOST_H */
