/*
 * ppf_mesh_host.h — host side of ppf_cloud_from_mesh: a model cloud sampled from a triangle mesh.
 * Kernels: ppf_mesh_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, frame_scan, stage_entry;
 * FrameRun::finish is the one way out of a call once it has enqueued) and ppf_prep_host.h (ppf_cloud).
 *
 *   without visibility   k_mesh_tri, k_mesh_area, frame_scan (5), k_mesh_sample: 8 launches
 *   with visibility      those, then k_mesh_draw_small, k_mesh_draw_large, k_mesh_visible, frame_scan (5), k_mesh_scatter: 17
 * and two blocking waits -- the read-back of the row count, which sizes everything, and the end -- whatever the mesh holds.
 * The large path's workgroups read the length of their list on the device, so it costs no third wait.  The cloud is
 * allocated for the n_sampled rows before the kept ones are counted: that is what the second wait would otherwise be split for.
 */
#ifndef PPF_MESH_HOST_H
#define PPF_MESH_HOST_H

namespace {

/* the 26 views' d, a, b (they do not depend on the mesh) and the box's ctr, r, px; map_size, min_views and depth_tol resolved */
void mesh_views(const ppf_mesh_sample_params& p, const uint32_t* box, MeshViews* W) {
  std::memset(W, 0, sizeof(*W));
  int v = 0;
  for (int x = -1; x <= 1; x++)
    for (int y = -1; y <= 1; y++)
      for (int z = -1; z <= 1; z++) {
        const int nz = (x != 0) + (y != 0) + (z != 0);
        if (!nz) continue;
        const double s = 1.0 / ppf_sqrt((double)nz);
        double* d = W->d[v];
        d[0] = (double)x * s;
        d[1] = (double)y * s;
        d[2] = (double)z * s;
        int ax = 0;
        for (int a = 1; a < 3; a++)
          if (ppf_fabs(d[a]) < ppf_fabs(d[ax])) ax = a;
        const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        const double t[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
        const double tl = ppf_sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        double* a = W->a[v];
        for (int c = 0; c < 3; c++) a[c] = t[c] / tl;
        double* b = W->b[v];
        b[0] = d[1] * a[2] - d[2] * a[1];
        b[1] = d[2] * a[0] - d[0] * a[2];
        b[2] = d[0] * a[1] - d[1] * a[0];
        v++;
      }
  W->R = p.map_size ? p.map_size : 256;
  W->min_views = std::max(1, (int)p.min_views);
  W->orient = p.orient;
  W->half = 0.5 * (double)W->R;
  if (box[3]) { /* some live vertex */
    double g[3];
    for (int a = 0; a < 3; a++) {
      const double lo = (double)mesh_fkey_inv(~box[a]), hi = (double)mesh_fkey_inv(box[3 + a]);
      W->ctr[a] = 0.5 * (lo + hi);
      g[a] = hi - lo;
    }
    W->r = 0.5 * ppf_sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  }
  W->px = 2.0 * W->r / (double)(W->R - 2);
  W->tol = p.depth_tol > 0.f ? (double)p.depth_tol : 2.0 * W->px;
}

/* every argument check, in the header's order, and the host's count of a small mesh */
ppf_status mesh_check(const char* who, const float* vertices, int n_vertices, int vstride, int normal_offset, const int32_t* triangles,
                      int n_triangles, const ppf_mesh_sample_params* p, double* max_rows) {
  if (!p) return fail(PPF_ERR_INVALID, "%s: the params are NULL", who);
  if (!vertices || !triangles) return fail(PPF_ERR_INVALID, "%s: vertices and triangles must not be NULL", who);
  if (n_vertices < 1 || n_triangles < 1)
    return fail(PPF_ERR_INVALID, "%s: a mesh of %d vertices and %d triangles", who, n_vertices, n_triangles);
  if (vstride < 3) return fail(PPF_ERR_INVALID, "%s: vstride %d is below 3", who, vstride);
  if (normal_offset != -1 && (normal_offset < 3 || normal_offset > vstride - 3))
    return fail(PPF_ERR_INVALID, "%s: normal_offset %d is neither -1 nor in 3 .. vstride - 3 = %d", who, normal_offset, vstride - 3);
  if (!(std::isfinite(p->spacing) && p->spacing > 0.f)) return fail(PPF_ERR_INVALID, "%s: spacing must be finite and > 0", who);
  if (p->normals != PPF_MESH_NORMALS_FACE && p->normals != PPF_MESH_NORMALS_VERTEX)
    return fail(PPF_ERR_INVALID, "%s: normals %d is neither PPF_MESH_NORMALS_FACE nor PPF_MESH_NORMALS_VERTEX", who, p->normals);
  if (p->normals == PPF_MESH_NORMALS_VERTEX && normal_offset < 0)
    return fail(PPF_ERR_INVALID, "%s: PPF_MESH_NORMALS_VERTEX needs a normal_offset", who);
  if (p->visibility != 0 && p->visibility != 1) return fail(PPF_ERR_INVALID, "%s: visibility %d is neither 0 nor 1", who, p->visibility);
  if (p->orient != 0 && p->orient != 1) return fail(PPF_ERR_INVALID, "%s: orient %d is neither 0 nor 1", who, p->orient);
  if (p->orient && !p->visibility) return fail(PPF_ERR_INVALID, "%s: orient needs visibility", who);
  if (p->map_size != 0 && (p->map_size < 16 || p->map_size > 1024))
    return fail(PPF_ERR_INVALID, "%s: map_size %d is neither 0 nor in 16 .. 1024", who, p->map_size);
  if (p->min_views < 0 || p->min_views > PPF_MESH_VIEWS)
    return fail(PPF_ERR_INVALID, "%s: min_views %d is outside 0 .. %d", who, p->min_views, PPF_MESH_VIEWS);
  if (!(std::isfinite(p->depth_tol) && p->depth_tol >= 0.f)) return fail(PPF_ERR_INVALID, "%s: depth_tol must be finite and >= 0", who);
  if (p->max_rows < 0) return fail(PPF_ERR_INVALID, "%s: max_rows %d is negative", who, p->max_rows);
  for (int i = 0; i < 4; i++)
    if (p->reserved[i] != 0) return fail(PPF_ERR_INVALID, "%s: reserved must be 0", who);
  if (p->visibility && (unsigned long long)n_triangles * PPF_MESH_VIEWS >= (1ull << 32))
    return fail(PPF_ERR_INVALID, "%s: %d triangles in %d views exceed the 2^32 entries of the draw list", who, n_triangles, PPF_MESH_VIEWS);
  for (int k = 0; k < n_triangles; k++)
    for (int c = 0; c < 3; c++) {
      const int32_t i = triangles[(size_t)k * 3 + c];
      if (i < 0 || i >= n_vertices)
        return fail(PPF_ERR_INVALID, "%s: triangle %d has index %d outside [0, %d)", who, k, (int)i, n_vertices);
    }
  *max_rows = (double)(p->max_rows ? p->max_rows : (1 << 24));
  if (n_triangles <= PPF_MESH_HOST_COUNT) {
    const double s2 = (double)p->spacing * (double)p->spacing;
    unsigned long long total = 0;
    for (int k = 0; k < n_triangles; k++) {
      MeshTri t;
      mesh_tri_geom(vertices, vstride, triangles + (size_t)k * 3, t);
      if (!t.ok) continue;
      uint32_t n = 0;
      if (!mesh_count(t.L, s2, p->seed, (uint32_t)k, *max_rows, &n) || (double)(total += n) > *max_rows)
        return fail(PPF_ERR_CAPACITY, "%s: the mesh gives more than max_rows = %.0f rows at spacing %g", who, *max_rows, (double)p->spacing);
    }
  }
  return PPF_OK;
}

ppf_status mesh_sample(const char* who, const float* vertices, int n_vertices, int vstride, int normal_offset, const int32_t* triangles,
                       int n_triangles, const ppf_mesh_sample_params* p, ppf_cloud** out, ppf_mesh_sample_stats& st) {
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  double max_rows = 0.0;
  ppf_status s = mesh_check(who, vertices, n_vertices, vstride, normal_offset, triangles, n_triangles, p, &max_rows);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);

  const uint32_t nt = (uint32_t)n_triangles;
  const size_t n_vfloats = (size_t)n_vertices * (size_t)vstride;
  const dim3 blk(MESH_BLOCK), tri_grid = grid_for(nt, MESH_BLOCK);
  const int noff = p->normals == PPF_MESH_NORMALS_VERTEX ? normal_offset : -1;
  FrameRun fr;
  float* d_vert;
  int32_t* d_tri;
  uint32_t *nk, *offs;
  uint8_t* live;
  double* area_part;
  MeshCounters* d_C;
  s = fr.get(n_vfloats, &d_vert, (size_t)nt * 3, &d_tri, (size_t)nt + 1, &nk, (size_t)nt + 1, &offs, (size_t)nt, &live, (size_t)tri_grid.x, &area_part,
             (size_t)1, &d_C);
  if (s != PPF_OK) return s;
  std::unique_ptr<ppf_cloud> c;
  MeshCounters C;
  MeshViews W;
  uint32_t n_rows = 0, total = 0;
  uint32_t* pos = nullptr;
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemcpyAsync(d_vert, vertices, n_vfloats * sizeof(float), hipMemcpyHostToDevice, fr.st));
    HIPCHK(hipMemcpyAsync(d_tri, triangles, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, fr.st));
    HIPCHK(hipMemsetAsync(d_C, 0, sizeof(MeshCounters), fr.st));
    FRAME_LAUNCH(fr, k_mesh_tri, tri_grid, blk, d_vert, vstride, d_tri, nt, (double)p->spacing * (double)p->spacing, p->seed, max_rows, nk, live,
                 area_part, d_C);
    FRAME_LAUNCH(fr, k_mesh_area, dim3(1), blk, area_part, tri_grid.x, d_C);
    HIPCHK(hipGetLastError());
    ppf_status r = frame_scan(fr, nk, offs, (size_t)nt + 1);
    if (r != PPF_OK) return r;
    if ((r = fr.sizing({{"counters", d_C, sizeof(C), &C}})) != PPF_OK) return r;
    if (C.over || (double)C.total > max_rows)
      return fail(PPF_ERR_CAPACITY, "%s: the mesh gives more than max_rows = %.0f rows at spacing %g", who, max_rows, (double)p->spacing);
    total = (uint32_t)C.total; /* at most max_rows <= INT32_MAX: the scan of the n_k did not wrap */
    const dim3 row_grid = grid_for(total, MESH_BLOCK);
    if ((r = cloud_alloc(c, (int)total)) != PPF_OK) return r;
    if (!p->visibility) {
      FRAME_LAUNCH(fr, k_mesh_sample, row_grid, blk, d_vert, vstride, noff, d_tri, nt, offs, total, p->seed, c->rows.p, c->curv.p);
      HIPCHK(hipGetLastError());
      n_rows = total;
      return PPF_OK;
    }
    mesh_views(*p, C.box, &W);
    const size_t map_px = (size_t)PPF_MESH_VIEWS * W.R * W.R;
    MeshViews* d_W;
    uint32_t *maps, *list, *keep;
    float* rows;
    r = fr.get((size_t)1, &d_W, map_px, &maps, (size_t)nt * PPF_MESH_VIEWS, &list, (size_t)total * 6, &rows, (size_t)total + 1, &keep, (size_t)total + 1, &pos);
    if (r != PPF_OK) return r;
    HIPCHK(hipMemcpyAsync(d_W, &W, sizeof(W), hipMemcpyHostToDevice, fr.st));
    HIPCHK(hipMemsetAsync(maps, 0xff, map_px * sizeof(uint32_t), fr.st));
    FRAME_LAUNCH(fr, k_mesh_sample, row_grid, blk, d_vert, vstride, noff, d_tri, nt, offs, total, p->seed, rows, (float*)nullptr);
    FRAME_LAUNCH(fr, k_mesh_draw_small, dim3(tri_grid.x, PPF_MESH_VIEWS), blk, d_vert, vstride, d_tri, nt, live, d_W, maps, list, d_C);
    FRAME_LAUNCH(fr, k_mesh_draw_large, dim3(MESH_LARGE_GRID), blk, d_vert, vstride, d_tri, d_W, maps, list, d_C);
    FRAME_LAUNCH(fr, k_mesh_visible, row_grid, blk, rows, total, d_W, maps, keep, d_C);
    HIPCHK(hipGetLastError());
    if ((r = frame_scan(fr, keep, pos, (size_t)total + 1)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_mesh_scatter, row_grid, blk, rows, total, keep, pos, c->rows.p, c->curv.p);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status enq = run();
  const bool vis = enq == PPF_OK && p->visibility;
  s = fr.finish(who, enq, {{"kept rows", vis ? pos + total : nullptr, sizeof(n_rows), vis ? &n_rows : nullptr},
                           {"counters", d_C, sizeof(C), vis ? &C : nullptr}}); /* the end: the scratch goes back at scope exit */
  if (s != PPF_OK) return s;
  c->n = (int)n_rows;
  st.n_triangles = n_triangles;
  st.n_degenerate = (int64_t)C.degenerate;
  st.n_sampled = (int64_t)total;
  st.n_rows = (int64_t)n_rows;
  st.n_hidden = (int64_t)total - (int64_t)n_rows;
  st.n_flipped = (int64_t)C.flipped;
  st.n_large = (int64_t)C.large;
  fr.report(st);
  st.area = C.area;
  *out = c.release();
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_mesh_sample_params(ppf_mesh_sample_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->spacing = 0.004f;
  p->normals = PPF_MESH_NORMALS_FACE;
  p->visibility = 1;
  p->orient = 1;
}

ppf_status ppf_cloud_from_mesh(const float* vertices, int n_vertices, int vstride, int normal_offset, const int32_t* triangles, int n_triangles,
                               const ppf_mesh_sample_params* p, ppf_cloud** out, ppf_mesh_sample_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_mesh_sample_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed && out) *out = nullptr;
      },
      [&](ppf_mesh_sample_stats& st) {
        return mesh_sample("ppf_cloud_from_mesh", vertices, n_vertices, vstride, normal_offset, triangles, n_triangles, p, out, st);
      });
}

}  // extern "C"

#endif /* PPF_MESH_HOST_H */
