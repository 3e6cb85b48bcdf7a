/*
 * ppf_volume_host.h — host side of ppf_depth_volume: posed depth images fused into a truncated signed distance volume that
 * stays on the device, the model depth image it gives from any pose, and its zero surface as a ppf_cloud.
 * Kernels: ppf_volume_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, frame_scan, stage_finish, stage_entry),
 * ppf_prep_host.h (ppf_cloud) and ppf_depthimage_host.h (the image check, the bindings, depth_outputs_check, depth_typed).
 *
 *   integrate  an 8-byte clear of the counter, k_volume_integrate -- one launch -- and one blocking wait.
 *   raycast    an 8-byte clear of the counters, k_volume_raycast -- one launch -- and one blocking wait.
 *   extract    k_volume_cross<0>, the five launches of frame_scan, k_volume_cross<1> -- seven launches -- and two blocking
 *              waits: the read-back that sizes the cloud, and the end.
 *   mesh       a 32-byte clear of the counters, k_vmesh_cells, k_vmesh_edges, two frame_scans, k_vmesh_vertices,
 *              k_vmesh_triangles (ppf_volume_mesh_kernels.h) -- fourteen launches -- and two blocking waits: the read-back
 *              that sizes the mesh, and the end.
 * whatever the images and the volume hold.  The host entries add the upload of the image or the read-back of the outputs
 * behind the same wait.  The volume and its counters belong to the handle, whose mutex serialises every call on it.
 */
#ifndef PPF_VOLUME_HOST_H
#define PPF_VOLUME_HOST_H

struct ppf_depth_volume {
  ppf_depth_volume_params vp;
  size_t n = 0;               /* voxels */
  long long integrations = 0; /* since creation or the last reset */
  std::mutex mu;
  DevBuf<VolVoxel> vox;
  DevBuf<unsigned long long> counters; /* 2: [0] n_updated or the crossings; as int32: n_hits, n_interpolated */
};

/* vertices (rows x y z nx ny nz) and triangles (three vertex indices each), resident on the device */
struct ppf_volume_mesh {
  int64_t nv = 0, nt = 0;
  DevBuf<float> verts;
  DevBuf<int32_t> tris;
};

namespace {

VolArgs volume_args(const ppf_depth_volume* v) {
  VolArgs V;
  V.vox = v->vox.p;
  V.nx = v->vp.dims[0];
  V.ny = v->vp.dims[1];
  V.nz = v->vp.dims[2];
  V.voxel = (double)v->vp.voxel;
  V.trunc = (double)v->vp.trunc;
  for (int a = 0; a < 3; a++) V.o[a] = v->vp.origin[a];
  return V;
}

StageBuf volume_range(const ppf_depth_volume* v) { return {"volume", v->vox.p, v->n * sizeof(VolVoxel), nullptr}; }

ppf_status volume_pose_check(const char* who, const double* pose16) {
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(pose16[i])) return fail(PPF_ERR_INVALID, "%s: pose16 must be finite", who);
  return PPF_OK;
}

/* the device question of every entry on a volume, asked after the argument checks; a handle made without device memory
 * (ppf_debug_depth_volume_shell) gets no further */
ppf_status volume_device(const char* who, const ppf_depth_volume* v) {
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if (!v->vox.p) return fail(PPF_ERR_INVALID, "%s: the volume is a shell without device memory", who);
  return PPF_OK;
}

ppf_status volume_fill(ppf_depth_volume* v) {
  k_volume_fill<<<grid_for((v->n + 1) / 2, 256), dim3(256), 0, nullptr>>>(v->vox.p, v->n);
  HIPCHK(hipGetLastError());
  HIPCHK(host_stream_sync(nullptr));
  v->integrations = 0;
  return PPF_OK;
}

/* ---- integrate ----------------------------------------------------------------------------------------------------- */
/* every argument check of both entries, before any device work; fills the image's kernel arguments (img excepted) */
ppf_status volume_integrate_check(const char* who, const ppf_depth_volume* v, const void* depth, int rows, int cols, size_t pitch,
                                  const double* intr, const ppf_depth_params* dp, const double* pose16, DepthArgs* a) {
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  if (!pose16) return fail(PPF_ERR_INVALID, "%s: pose16 is NULL", who);
  if (!dp || !intr) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  ppf_status s;
  if ((s = depth_image_check(who, depth, rows, cols, pitch, dp, DEPTH_FLAGS_IGNORED, a)) != PPF_OK ||
      (s = depth_intr_check(who, intr, a)) != PPF_OK)
    return s;
  return volume_pose_check(who, pose16);
}

/* the counter cleared and the one launch, on `st`; the caller holds the volume's mutex */
ppf_status volume_integrate_enqueue(ppf_depth_volume* v, const DepthArgs& a, int format, int rows, const double* pose16, hipStream_t st) {
  const VolArgs V = volume_args(v);
  VolPose P;
  std::memcpy(P.T, pose16, sizeof(P.T));
  const int pairs_x = (V.nx + 1) / 2, vec = V.nx % 2 == 0 ? 1 : 0;
  /* ceil(nx / 2) * ny * nz lanes: at most 2^29, so the grid is at most 2^23 workgroups */
  const long long lanes = (long long)pairs_x * V.ny * V.nz;
  HIPCHK(hipMemsetAsync(v->counters.p, 0, sizeof(unsigned long long), st));
  depth_typed(format, [&](auto px) {
    k_volume_integrate<decltype(px)><<<dim3((unsigned)((lanes + DV_BLOCK - 1) / DV_BLOCK)), dim3(DV_BLOCK), 0, st>>>(
        a, V, P, rows, v->vp.max_weight, pairs_x, vec, v->counters.p);
  });
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

ppf_status volume_integrate_done(ppf_depth_volume* v, unsigned long long n, ppf_depth_volume_integrate_stats& st) {
  st.n_updated = (int64_t)n;
  st.n_launches = 1;
  st.n_host_syncs = 1;
  v->integrations++;
  return PPF_OK;
}

ppf_status volume_integrate_host(const char* who, ppf_depth_volume* v, const void* depth, int rows, int cols, size_t pitch, const double* intr,
                                 const ppf_depth_params* dp, const double* pose16, ppf_depth_volume_integrate_stats& st) {
  DepthArgs a;
  ppf_status s = volume_integrate_check(who, v, depth, rows, cols, pitch, intr, dp, pose16, &a);
  if (s != PPF_OK) return s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  DevBuf<unsigned char> img;
  if ((s = depth_bind_host(depth, dp->format, img, &a)) != PPF_OK) return s;
  unsigned long long n = 0;
  s = stage_finish(who, volume_integrate_enqueue(v, a, dp->format, rows, pose16, nullptr), nullptr,
                   {{"counter", v->counters.p, sizeof(n), &n}});
  return s != PPF_OK ? s : volume_integrate_done(v, n, st);
}

ppf_status volume_integrate_device(const char* who, ppf_depth_volume* v, const void* d_depth, int rows, int cols, size_t pitch,
                                   const double* intr, const ppf_depth_params* dp, const double* pose16, hipStream_t stream,
                                   ppf_depth_volume_integrate_stats& st) {
  DepthArgs a;
  StageBuf image;
  ppf_status s = volume_integrate_check(who, v, d_depth, rows, cols, pitch, intr, dp, pose16, &a);
  if (s != PPF_OK) return s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  if ((s = depth_bind_device(who, d_depth, dp->format, &a, &image)) != PPF_OK) return s;
  if (ranges_overlap(image, volume_range(v))) return fail(PPF_ERR_INVALID, "%s: the image overlaps the volume", who);
  std::lock_guard<std::mutex> lock(v->mu);
  unsigned long long n = 0;
  s = stage_finish(who, volume_integrate_enqueue(v, a, dp->format, rows, pose16, stream), stream,
                   {{"counter", v->counters.p, sizeof(n), &n}});
  return s != PPF_OK ? s : volume_integrate_done(v, n, st);
}

/* ---- raycast ------------------------------------------------------------------------------------------------------- */
/* every argument check of both entries, before any device work; fills the kernel's arguments but for the pointers */
ppf_status volume_raycast_check(const char* who, const ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                const ppf_depth_volume_raycast_params* rp, const float* depth_out, VolRay* Q) {
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  if (!depth_out) return fail(PPF_ERR_INVALID, "%s: the depth output is NULL", who);
  if (!pose16) return fail(PPF_ERR_INVALID, "%s: pose16 is NULL", who);
  if (!rp) return fail(PPF_ERR_INVALID, "%s: the raycast params are NULL", who);
  if (!intr) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  if (rows <= 0 || cols <= 0) return fail(PPF_ERR_INVALID, "%s: the image is %d x %d", who, rows, cols);
  if ((long long)rows * cols > 0x7fffffffLL) return fail(PPF_ERR_INVALID, "%s: %d x %d pixels exceed INT32_MAX", who, rows, cols);
  DepthArgs a;
  ppf_status s;
  if ((s = depth_intr_check(who, intr, &a)) != PPF_OK || (s = volume_pose_check(who, pose16)) != PPF_OK) return s;
  if (!(std::isfinite(rp->z_near) && std::isfinite(rp->z_far) && rp->z_near > 0.f && rp->z_near < rp->z_far))
    return fail(PPF_ERR_INVALID, "%s: z_near and z_far must be finite with 0 < z_near < z_far", who);
  if (!(rp->ray_step > 0.f && rp->ray_step <= 1.f)) return fail(PPF_ERR_INVALID, "%s: ray_step must be in (0, 1]", who);
  if (rp->min_weight < 1) return fail(PPF_ERR_INVALID, "%s: min_weight must be >= 1", who);
  if (rp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown raycast flags 0x%x", who, (unsigned)rp->flags);
  const double step = (double)rp->ray_step * (double)v->vp.trunc;
  const double K = std::ceil(((double)rp->z_far - (double)rp->z_near) / step);
  if (!(K <= (double)PPF_VOLUME_MAX_STEPS))
    return fail(PPF_ERR_INVALID, "%s: the walk from z_near to z_far takes more than %d steps", who, PPF_VOLUME_MAX_STEPS);
  /* one workgroup of 256 lanes per 16 x 16 tile: a launch holds fewer than 2^32 lanes */
  const long long tiles = (((long long)cols + DV_TILE - 1) / DV_TILE) * (((long long)rows + DV_TILE - 1) / DV_TILE);
  if (tiles > PPF_VOLUME_MAX_TILES)
    return fail(PPF_ERR_INVALID, "%s: a %d x %d image has %lld tiles of 16 x 16 pixels, more than %d", who, rows, cols, tiles, PPF_VOLUME_MAX_TILES);
  Q->rows = rows;
  Q->cols = cols;
  Q->tiles_x = (cols + DV_TILE - 1) / DV_TILE;
  Q->fx = a.fx; Q->fy = a.fy; Q->ppx = a.ppx; Q->ppy = a.ppy;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Q->R[r * 3 + c] = pose16[r * 4 + c];
  const double t0 = pose16[3], t1 = pose16[7], t2 = pose16[11];
  for (int c = 0; c < 3; c++) Q->c[c] = -((Q->R[c] * t0 + Q->R[3 + c] * t1) + Q->R[6 + c] * t2);
  Q->z_near = (double)rp->z_near;
  Q->step = step;
  Q->K = (int)K;
  Q->min_weight = rp->min_weight;
  Q->depth = nullptr;
  Q->normals = nullptr;
  Q->counters = nullptr;
  return PPF_OK;
}

/* the counters cleared and the one launch, on `st`; the caller holds the volume's mutex */
ppf_status volume_raycast_enqueue(ppf_depth_volume* v, VolRay& Q, float* d_depth, float* d_normals, hipStream_t st) {
  Q.depth = d_depth;
  Q.normals = d_normals;
  Q.counters = reinterpret_cast<int32_t*>(v->counters.p);
  HIPCHK(hipMemsetAsync(v->counters.p, 0, 2 * sizeof(int32_t), st));
  /* the tiles as one grid dimension: at most n / 256 + rows / 16 + cols / 16 + 1 workgroups, below 2^31 */
  const long long tiles = (long long)Q.tiles_x * ((Q.rows + DV_TILE - 1) / DV_TILE);
  k_volume_raycast<<<dim3((unsigned)tiles), dim3(DV_RAY_BLOCK), 0, st>>>(volume_args(v), Q);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

void volume_raycast_done(const int32_t* c, ppf_depth_volume_raycast_stats& st) {
  st.n_hits = c[0];
  st.n_interpolated = c[1];
  st.n_launches = 1;
  st.n_host_syncs = 1;
}

ppf_status volume_raycast_host(const char* who, ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                               const ppf_depth_volume_raycast_params* rp, float* depth_out, float* normals_out,
                               ppf_depth_volume_raycast_stats& st) {
  VolRay Q;
  ppf_status s = volume_raycast_check(who, v, rows, cols, intr, pose16, rp, depth_out, &Q);
  if (s != PPF_OK) return s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  const size_t n = (size_t)rows * (size_t)cols;
  DevBuf<float> dbuf, nbuf;
  HIPCHK(dbuf.reserve(n));
  if (normals_out) HIPCHK(nbuf.reserve(n * 3));
  /* into staging first: the outputs are only written once everything has succeeded */
  std::vector<float> d(n), nr(normals_out ? n * 3 : 0);
  int32_t c[2];
  s = stage_finish(who, volume_raycast_enqueue(v, Q, dbuf.p, normals_out ? nbuf.p : nullptr, nullptr), nullptr,
                   {{"depth output", dbuf.p, n * sizeof(float), d.data()},
                    {"normals output", nbuf.p, n * 3 * sizeof(float), normals_out ? nr.data() : nullptr},
                    {"counters", v->counters.p, sizeof(c), c}});
  if (s != PPF_OK) return s;
  std::memcpy(depth_out, d.data(), n * sizeof(float));
  if (normals_out) std::memcpy(normals_out, nr.data(), n * 3 * sizeof(float));
  volume_raycast_done(c, st);
  return PPF_OK;
}

ppf_status volume_raycast_device(const char* who, ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                 const ppf_depth_volume_raycast_params* rp, float* d_depth, float* d_normals, hipStream_t stream,
                                 ppf_depth_volume_raycast_stats& st) {
  VolRay Q;
  ppf_status s = volume_raycast_check(who, v, rows, cols, intr, pose16, rp, d_depth, &Q);
  if (s != PPF_OK) return s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  const size_t n = (size_t)rows * (size_t)cols;
  if ((s = depth_outputs_check(who, volume_range(v),
                               {{"depth output", d_depth, n * sizeof(float), nullptr}, {"normals output", d_normals, n * 3 * sizeof(float), nullptr}})) !=
      PPF_OK)
    return s;
  std::lock_guard<std::mutex> lock(v->mu);
  int32_t c[2];
  s = stage_finish(who, volume_raycast_enqueue(v, Q, d_depth, d_normals, stream), stream, {{"counters", v->counters.p, sizeof(c), c}});
  if (s != PPF_OK) return s;
  volume_raycast_done(c, st);
  return PPF_OK;
}

/* ---- extract ------------------------------------------------------------------------------------------------------- */
ppf_status volume_extract(const char* who, ppf_depth_volume* v, const ppf_depth_volume_extract_params* ep, ppf_cloud** out,
                          ppf_depth_volume_extract_stats& st) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  if (!ep) return fail(PPF_ERR_INVALID, "%s: the extract params are NULL", who);
  if (ep->min_weight < 1) return fail(PPF_ERR_INVALID, "%s: min_weight must be >= 1", who);
  if (ep->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown extract flags 0x%x", who, (unsigned)ep->flags);
  ppf_status s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  const VolArgs V = volume_args(v);
  const uint32_t n_tiles = (uint32_t)((v->n + DV_X_BLOCK - 1) / DV_X_BLOCK); /* at most 2^22 */
  FrameRun fr;
  uint32_t *counts, *offs;
  s = fr.get((size_t)n_tiles + 1, &counts, (size_t)n_tiles + 1, &offs);
  if (s != PPF_OK) return s;
  std::unique_ptr<ppf_cloud> c;
  uint32_t total = 0;
  unsigned long long n_cross = 0;
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemsetAsync(v->counters.p, 0, sizeof(unsigned long long), fr.st));
    FRAME_LAUNCH(fr, k_volume_cross<0>, dim3(n_tiles), dim3(DV_X_BLOCK), V, ep->min_weight, v->n, n_tiles, counts, v->counters.p, nullptr, nullptr,
                 nullptr);
    HIPCHK(hipGetLastError());
    ppf_status r = frame_scan(fr, counts, offs, (size_t)n_tiles + 1);
    if (r != PPF_OK) return r;
    if ((r = fr.sizing({{"rows", offs + n_tiles, sizeof(total), &total}, {"crossings", v->counters.p, sizeof(n_cross), &n_cross}})) != PPF_OK) return r;
    if (total > 0x7fffffffu) return fail(PPF_ERR_NOMEM, "%s: %u rows exceed INT32_MAX, the most a cloud holds", who, total);
    if ((r = cloud_alloc(c, (int)total)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_volume_cross<1>, dim3(n_tiles), dim3(DV_X_BLOCK), V, ep->min_weight, v->n, n_tiles, nullptr, nullptr, offs, c->rows.p,
                 c->curv.p);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  s = fr.finish(who, run(), {}); /* the end: the scratch goes back to the block cache at scope exit */
  if (s != PPF_OK) return s;
  st.n_crossings = (int64_t)n_cross;
  st.n_rows = (int64_t)total;
  fr.report(st);
  *out = c.release();
  return PPF_OK;
}

/* ---- mesh ---------------------------------------------------------------------------------------------------------- */
ppf_status mesh_alloc(const char* who, std::unique_ptr<ppf_volume_mesh>& m, int64_t nv, int64_t nt) {
  m.reset(new (std::nothrow) ppf_volume_mesh());
  if (!m) return fail(PPF_ERR_NOMEM, "%s: out of host memory", who);
  m->nv = nv;
  m->nt = nt;
  if (m->verts.reserve((size_t)std::max<int64_t>(nv, 1) * 6) != hipSuccess || m->tris.reserve((size_t)std::max<int64_t>(nt, 1) * 3) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PPF_ERR_NOMEM, "%s: a mesh of %lld vertices and %lld triangles cannot be allocated", who, (long long)nv, (long long)nt);
  }
  return PPF_OK;
}

ppf_status volume_mesh(const char* who, ppf_depth_volume* v, const ppf_depth_volume_mesh_params* mp, ppf_volume_mesh** out,
                       ppf_depth_volume_mesh_stats& st) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  if (!mp) return fail(PPF_ERR_INVALID, "%s: the mesh params are NULL", who);
  if (mp->min_weight < 1) return fail(PPF_ERR_INVALID, "%s: min_weight must be >= 1", who);
  if (mp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown mesh flags 0x%x", who, (unsigned)mp->flags);
  ppf_status s;
  if ((s = volume_device(who, v)) != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  const VolArgs V = volume_args(v);
  const uint32_t n_tiles = (uint32_t)((v->n + VM_BLOCK - 1) / VM_BLOCK); /* at most 2^22 */
  FrameRun fr;
  uint32_t *tcnt, *toff, *vcnt, *voff;
  uint8_t *cell, *mask; /* 1 + 1 + 2 = 4 bytes of scratch per voxel */
  uint16_t* rank;
  unsigned long long* ctr;
  s = fr.get((size_t)n_tiles + 1, &tcnt, (size_t)n_tiles + 1, &toff, (size_t)n_tiles + 1, &vcnt, (size_t)n_tiles + 1, &voff, v->n, &cell, v->n, &mask,
             v->n, &rank, (size_t)VM_COUNTERS, &ctr);
  if (s != PPF_OK) return s;
  std::unique_ptr<ppf_volume_mesh> m;
  unsigned long long c[VM_COUNTERS] = {0, 0, 0, 0};
  auto run = [&]() -> ppf_status {
    const dim3 grid(n_tiles), block(VM_BLOCK);
    HIPCHK(hipMemsetAsync(ctr, 0, sizeof(c), fr.st));
    FRAME_LAUNCH(fr, k_vmesh_cells, grid, block, V, mp->min_weight, v->n, n_tiles, cell, tcnt, ctr);
    FRAME_LAUNCH(fr, k_vmesh_edges, grid, block, V, v->n, n_tiles, cell, mask, rank, vcnt, ctr);
    HIPCHK(hipGetLastError());
    ppf_status r;
    if ((r = frame_scan(fr, tcnt, toff, (size_t)n_tiles + 1)) != PPF_OK || (r = frame_scan(fr, vcnt, voff, (size_t)n_tiles + 1)) != PPF_OK) return r;
    if ((r = fr.sizing({{"counters", ctr, sizeof(c), c}})) != PPF_OK) return r;
    /* the 64-bit counts decide: a scan total that wrapped is never looked at */
    if (c[VM_N_VERTICES] > 0x7fffffffull || c[VM_N_TRIANGLES] > 0x7fffffffull)
      return fail(PPF_ERR_NOMEM, "%s: %llu vertices and %llu triangles exceed INT32_MAX, the most a mesh holds", who, c[VM_N_VERTICES],
                  c[VM_N_TRIANGLES]);
    if ((r = mesh_alloc(who, m, (int64_t)c[VM_N_VERTICES], (int64_t)c[VM_N_TRIANGLES])) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_vmesh_vertices, grid, block, V, mp->min_weight, v->n, mask, rank, voff, (uint32_t)m->nv, m->verts.p, ctr);
    FRAME_LAUNCH(fr, k_vmesh_triangles, grid, block, V, v->n, cell, mask, rank, voff, toff, (uint32_t)m->nt, m->tris.p);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  s = fr.finish(who, run(), {{"counters", ctr, sizeof(c), c}}); /* the end: the scratch goes back to the block cache at scope exit */
  if (s != PPF_OK) return s;
  st.n_cells = (int64_t)c[VM_N_CELLS];
  st.n_vertices = m->nv;
  st.n_triangles = m->nt;
  st.n_no_normal = (int64_t)c[VM_N_NO_NORMAL];
  fr.report(st);
  *out = m.release();
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_depth_volume_params(ppf_depth_volume_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->dims[0] = p->dims[1] = p->dims[2] = 256;
  p->voxel = 0.004f;
  p->origin[0] = -0.510;
  p->origin[1] = -0.510;
  p->origin[2] = 0.302;
  p->trunc = 0.016f;
  p->max_weight = 64;
  p->flags = 0;
}

void ppf_default_depth_volume_raycast_params(ppf_depth_volume_raycast_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->z_near = 0.3f;
  p->z_far = 1.5f;
  p->ray_step = 0.5f;
  p->min_weight = 1;
  p->flags = 0;
}

void ppf_default_depth_volume_extract_params(ppf_depth_volume_extract_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_weight = 1;
  p->flags = 0;
}

void ppf_default_depth_volume_mesh_params(ppf_depth_volume_mesh_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_weight = 1;
  p->flags = 0;
}

}  // extern "C"

namespace {

/* out and every field of vp, before any device work; a handle that holds the params and no device memory yet */
ppf_status volume_new(const char* who, const ppf_depth_volume_params* vp, ppf_depth_volume** out, std::unique_ptr<ppf_depth_volume>& v) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (!vp) return fail(PPF_ERR_INVALID, "%s: the volume params are NULL", who);
  for (int a = 0; a < 3; a++)
    if (vp->dims[a] < 1 || vp->dims[a] > PPF_VOLUME_MAX_DIM)
      return fail(PPF_ERR_INVALID, "%s: dims[%d] = %d is outside 1..%d", who, a, vp->dims[a], PPF_VOLUME_MAX_DIM);
  if (!(std::isfinite(vp->voxel) && vp->voxel > 0.f)) return fail(PPF_ERR_INVALID, "%s: voxel must be finite and > 0", who);
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(vp->origin[a])) return fail(PPF_ERR_INVALID, "%s: origin must be finite", who);
  if (!(std::isfinite(vp->trunc) && vp->trunc >= vp->voxel)) return fail(PPF_ERR_INVALID, "%s: trunc must be finite and >= voxel", who);
  if (vp->max_weight < 1 || vp->max_weight > PPF_VOLUME_MAX_WEIGHT)
    return fail(PPF_ERR_INVALID, "%s: max_weight %d is outside 1..%d", who, vp->max_weight, PPF_VOLUME_MAX_WEIGHT);
  if (vp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown volume flags 0x%x", who, (unsigned)vp->flags);
  v.reset(new (std::nothrow) ppf_depth_volume());
  if (!v) return fail(PPF_ERR_NOMEM, "%s: out of host memory", who);
  v->vp = *vp;
  v->n = (size_t)vp->dims[0] * (size_t)vp->dims[1] * (size_t)vp->dims[2];
  return PPF_OK;
}

}  // namespace

extern "C" {

ppf_status ppf_depth_volume_create(const ppf_depth_volume_params* vp, ppf_depth_volume** out) {
  static const char* who = "ppf_depth_volume_create";
  std::unique_ptr<ppf_depth_volume> v;
  ppf_status s = volume_new(who, vp, out, v);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const hipError_t e = v->vox.reserve(v->n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(PPF_ERR_NOMEM, "%s: a volume of %d x %d x %d voxels (%zu bytes) cannot be allocated: %s", who, vp->dims[0], vp->dims[1],
                vp->dims[2], v->n * sizeof(VolVoxel), hipGetErrorString(e));
  }
  HIPCHK(v->counters.reserve(2));
  if ((s = volume_fill(v.get())) != PPF_OK) return s;
  *out = v.release();
  return PPF_OK;
}

ppf_status ppf_debug_depth_volume_shell(const ppf_depth_volume_params* vp, ppf_depth_volume** out) {
  std::unique_ptr<ppf_depth_volume> v;
  const ppf_status s = volume_new("ppf_debug_depth_volume_shell", vp, out, v);
  if (s == PPF_OK) *out = v.release();
  return s;
}

ppf_status ppf_depth_volume_release(ppf_depth_volume* v) {
  delete v; /* every call has waited for its kernels: the volume goes back to the block cache */
  return PPF_OK;
}

ppf_status ppf_depth_volume_reset(ppf_depth_volume* v) {
  static const char* who = "ppf_depth_volume_reset";
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  const ppf_status s = volume_device(who, v);
  if (s != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  return volume_fill(v);
}

ppf_status ppf_depth_volume_info(const ppf_depth_volume* v, ppf_depth_volume_desc* info) {
  if (info) std::memset(info, 0, sizeof(*info));
  if (!v || !info) return fail(PPF_ERR_INVALID, "ppf_depth_volume_info: the volume and info must not be NULL");
  std::lock_guard<std::mutex> lock(const_cast<ppf_depth_volume*>(v)->mu);
  for (int a = 0; a < 3; a++) {
    info->dims[a] = v->vp.dims[a];
    info->origin[a] = v->vp.origin[a];
  }
  info->voxel = v->vp.voxel;
  info->trunc = v->vp.trunc;
  info->max_weight = v->vp.max_weight;
  info->integrations = v->integrations;
  info->device_bytes = v->vox.bytes() + v->counters.bytes();
  return PPF_OK;
}

ppf_status ppf_depth_volume_read(const ppf_depth_volume* v, ppf_depth_volume_voxel* out, size_t n_voxels) {
  static const char* who = "ppf_depth_volume_read";
  if (!v || !out) return fail(PPF_ERR_INVALID, "%s: the volume and out must not be NULL", who);
  if (n_voxels != v->n) return fail(PPF_ERR_INVALID, "%s: out holds %zu records, the volume has %zu voxels", who, n_voxels, v->n);
  const ppf_status s = volume_device(who, v);
  if (s != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(const_cast<ppf_depth_volume*>(v)->mu);
  HIPCHK(hipMemcpy(out, v->vox.p, v->n * sizeof(VolVoxel), hipMemcpyDeviceToHost));
  return PPF_OK;
}

ppf_status ppf_depth_volume_write(ppf_depth_volume* v, const ppf_depth_volume_voxel* in, size_t n_voxels) {
  static const char* who = "ppf_depth_volume_write";
  if (!v) return fail(PPF_ERR_INVALID, "%s: the volume is NULL", who);
  if (!in) return fail(PPF_ERR_INVALID, "%s: in is NULL", who);
  if (n_voxels != v->n) return fail(PPF_ERR_INVALID, "%s: in holds %zu records, the volume has %zu voxels", who, n_voxels, v->n);
  for (size_t q = 0; q < n_voxels; q++) {
    const ppf_depth_volume_voxel& r = in[q];
    if (r.w < 0 || r.w > v->vp.max_weight || !(std::isfinite(r.d) && r.d >= -1.f && r.d <= 1.f))
      return fail(PPF_ERR_INVALID, "%s: record %zu has w = %d and d = %g: w must be in 0..%d and d finite in [-1, 1]", who, q, (int)r.w,
                  (double)r.d, (int)v->vp.max_weight);
  }
  const ppf_status s = volume_device(who, v);
  if (s != PPF_OK) return s;
  std::lock_guard<std::mutex> lock(v->mu);
  HIPCHK(hipMemcpy(v->vox.p, in, v->n * sizeof(VolVoxel), hipMemcpyHostToDevice));
  return PPF_OK;
}

ppf_status ppf_depth_volume_integrate(ppf_depth_volume* v, const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                      const ppf_depth_params* dp, const double* pose16, ppf_depth_volume_integrate_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_volume_integrate_stats>, [&](ppf_depth_volume_integrate_stats& st) {
    return volume_integrate_host("ppf_depth_volume_integrate", v, depth, rows, cols, row_pitch_bytes, intr, dp, pose16, st);
  });
}

ppf_status ppf_depth_volume_integrate_device(ppf_depth_volume* v, const void* d_depth, int rows, int cols, size_t row_pitch_bytes,
                                             const double* intr, const ppf_depth_params* dp, const double* pose16, void* stream,
                                             ppf_depth_volume_integrate_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_volume_integrate_stats>, [&](ppf_depth_volume_integrate_stats& st) {
    return volume_integrate_device("ppf_depth_volume_integrate_device", v, d_depth, rows, cols, row_pitch_bytes, intr, dp, pose16,
                                   static_cast<hipStream_t>(stream), st);
  });
}

ppf_status ppf_depth_volume_raycast(ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                    const ppf_depth_volume_raycast_params* rp, float* depth_out, float* normals_out,
                                    ppf_depth_volume_raycast_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_volume_raycast_stats>, [&](ppf_depth_volume_raycast_stats& st) {
    return volume_raycast_host("ppf_depth_volume_raycast", v, rows, cols, intr, pose16, rp, depth_out, normals_out, st);
  });
}

ppf_status ppf_depth_volume_raycast_device(ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                           const ppf_depth_volume_raycast_params* rp, float* d_depth, float* d_normals, void* stream,
                                           ppf_depth_volume_raycast_stats* stats) {
  return stage_entry(stats, stage_clear_stats<ppf_depth_volume_raycast_stats>, [&](ppf_depth_volume_raycast_stats& st) {
    return volume_raycast_device("ppf_depth_volume_raycast_device", v, rows, cols, intr, pose16, rp, d_depth, d_normals,
                                 static_cast<hipStream_t>(stream), st);
  });
}

ppf_status ppf_depth_volume_extract(ppf_depth_volume* v, const ppf_depth_volume_extract_params* ep, ppf_cloud** out,
                                    ppf_depth_volume_extract_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_depth_volume_extract_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed && out) *out = nullptr;
      },
      [&](ppf_depth_volume_extract_stats& st) { return volume_extract("ppf_depth_volume_extract", v, ep, out, st); });
}

ppf_status ppf_depth_volume_mesh(ppf_depth_volume* v, const ppf_depth_volume_mesh_params* mp, ppf_volume_mesh** out,
                                 ppf_depth_volume_mesh_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_depth_volume_mesh_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed && out) *out = nullptr;
      },
      [&](ppf_depth_volume_mesh_stats& st) { return volume_mesh("ppf_depth_volume_mesh", v, mp, out, st); });
}

ppf_status ppf_volume_mesh_info(const ppf_volume_mesh* m, ppf_volume_mesh_desc* info) {
  if (info) std::memset(info, 0, sizeof(*info));
  if (!m || !info) return fail(PPF_ERR_INVALID, "ppf_volume_mesh_info: the mesh and info must not be NULL");
  info->n_vertices = m->nv;
  info->n_triangles = m->nt;
  info->device_bytes = m->verts.bytes() + m->tris.bytes();
  return PPF_OK;
}

ppf_status ppf_volume_mesh_read(const ppf_volume_mesh* m, float* vertices, size_t n_vertices, int32_t* triangles, size_t n_triangles) {
  static const char* who = "ppf_volume_mesh_read";
  if (!m) return fail(PPF_ERR_INVALID, "%s: the mesh is NULL", who);
  if (n_vertices != (size_t)m->nv || n_triangles != (size_t)m->nt)
    return fail(PPF_ERR_INVALID, "%s: the buffers hold %zu vertices and %zu triangles, the mesh has %lld and %lld", who, n_vertices, n_triangles,
                (long long)m->nv, (long long)m->nt);
  if (n_vertices && !vertices) return fail(PPF_ERR_INVALID, "%s: vertices is NULL", who);
  if (n_triangles && !triangles) return fail(PPF_ERR_INVALID, "%s: triangles is NULL", who);
  if (n_vertices) HIPCHK(hipMemcpy(vertices, m->verts.p, n_vertices * 6 * sizeof(float), hipMemcpyDeviceToHost));
  if (n_triangles) HIPCHK(hipMemcpy(triangles, m->tris.p, n_triangles * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PPF_OK;
}

ppf_status ppf_volume_mesh_release(ppf_volume_mesh* m) {
  delete m; /* the call that made it has waited for its kernels: the buffers go back to the block cache */
  return PPF_OK;
}

}  // extern "C"

#endif /* PPF_VOLUME_HOST_H */
