/*
 * ppf_mesh_components_host.h — host side of ppf_volume_mesh_upload and ppf_volume_mesh_components: a triangle mesh from host
 * arrays, and a mesh's connected components counted, measured, ranked by area and filtered.  Kernels:
 * ppf_mesh_components_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h (FrameRun, frame_scan, frame_sort, stage_entry)
 * and ppf_volume_host.h (ppf_volume_mesh, mesh_alloc).
 *
 *   components  two clears (the sums and the counters: zeros; the edge table's keys and the lower bounds: all ones), k_mc_init,
 *               k_mc_unite, k_mc_flatten, k_mc_tris, k_mc_edges, a frame_scan, k_mc_comps, eight radix passes over ~area_q
 *               with one gather between the low and the high word, k_mc_rank, k_mc_flags, two frame_scans, and with an
 *               output k_mc_write_vertices and k_mc_write_triangles -- 82 launches, 80 without -- and two blocking waits: the
 *               read-back that sizes the output, and the end, whatever the mesh holds.
 * All scratch comes from FrameRun, so from the block cache; the input mesh is only read.
 */
#ifndef PPF_MESH_COMPONENTS_HOST_H
#define PPF_MESH_COMPONENTS_HOST_H

namespace {

ppf_status mesh_components(const char* who, const ppf_volume_mesh* m, const ppf_mesh_component_params* p, ppf_volume_mesh** out, int32_t* labels,
                           ppf_mesh_component_info* info, int cap_info, ppf_mesh_component_stats& st) {
  if (out) *out = nullptr;
  if (!m) return fail(PPF_ERR_INVALID, "%s: the mesh is NULL", who);
  if (!p) return fail(PPF_ERR_INVALID, "%s: the component params are NULL", who);
  if (p->min_triangles < 1) return fail(PPF_ERR_INVALID, "%s: min_triangles must be >= 1", who);
  if (!(std::isfinite(p->min_area) && p->min_area >= 0.f)) return fail(PPF_ERR_INVALID, "%s: min_area must be finite and >= 0", who);
  if (p->rank_lo < 0) return fail(PPF_ERR_INVALID, "%s: rank_lo must be >= 0", who);
  if (p->rank_hi < p->rank_lo) return fail(PPF_ERR_INVALID, "%s: rank_hi must be >= rank_lo", who);
  if (p->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown component flags 0x%x", who, (unsigned)p->flags);
  if (cap_info < 0) return fail(PPF_ERR_INVALID, "%s: cap_info is %d", who, cap_info);
  if (cap_info > 0 && !info) return fail(PPF_ERR_INVALID, "%s: info is NULL with cap_info %d", who, cap_info);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  if (!m->verts.p) return fail(PPF_ERR_INVALID, "%s: the mesh is a shell without device memory", who);

  const uint32_t nv = (uint32_t)m->nv, nt = (uint32_t)m->nt; /* both at most INT32_MAX */
  const size_t np = std::max<size_t>(nv, 1);                 /* the sort's rows: a component per vertex at the most */
  size_t slots = 64;                                         /* the edge table: a power of two, at least twice the keys */
  while (slots < (size_t)nt * 6) slots <<= 1;
  const uint32_t cap = (uint32_t)std::min<size_t>((size_t)cap_info, np); /* C <= nv: no more records can be filled */
  const int nblk = (int)((np + RS_BLOCK - 1) / RS_BLOCK);
  FrameRun fr;
  ppf_status s;
  /* zeros: the seven sums, hi, the table's counts, the referenced flags, the counters.  All ones: lo, the table's keys */
  unsigned long long *zero64, *ones64;
  const size_t z64 = np + MC_COUNTERS, z32 = np * 10 + slots, o32 = np * 3;
  uint32_t *zero32, *ones32, *parent, *root, *flags, *cid, *comp_root, *klo, *khi, *kb, *va, *vb, *hist, *offs, *rank_of, *keep_of, *vkeep, *vpos,
      *tkeep, *tpos;
  int32_t* dlabels;
  ppf_mesh_component_info* dinfo;
  s = fr.get(z64, &zero64, z32, &zero32, slots, &ones64, o32, &ones32, np, &parent, np, &root, np + 1, &flags, np + 1, &cid, np, &comp_root, np, &klo,
             np, &khi, np, &kb, np, &va, np, &vb, (size_t)256 * nblk, &hist, (size_t)256 * nblk, &offs, np, &rank_of, np, &keep_of, np + 1, &vkeep,
             np + 1, &vpos, (size_t)nt + 1, &tkeep, (size_t)nt + 1, &tpos, np, &dlabels, (size_t)std::max<uint32_t>(cap, 1), &dinfo);
  if (s != PPF_OK) return s;
  McAcc acc;
  acc.area_q = zero64;
  unsigned long long* ctr = zero64 + np;
  acc.n_vert = zero32;
  acc.n_tri = zero32 + np;
  acc.n_deg = zero32 + np * 2;
  acc.n_edge = zero32 + np * 3;
  acc.n_bound = zero32 + np * 4;
  acc.n_nonman = zero32 + np * 5;
  acc.hi = zero32 + np * 6; /* 3 x nv; float_to_ordered is never 0 for a number */
  uint32_t* refd = zero32 + np * 9;
  uint32_t* hcnt = zero32 + np * 10;
  acc.lo = ones32;
  McParams P;
  P.min_triangles = p->min_triangles;
  P.rank_lo = p->rank_lo;
  P.rank_hi = p->rank_hi;
  P.min_area = (double)p->min_area;

  std::unique_ptr<ppf_volume_mesh> o;
  unsigned long long c[MC_COUNTERS] = {0, 0, 0, 0};
  uint32_t nv_out = 0, nt_out = 0;
  auto run = [&]() -> ppf_status {
    const dim3 block(MC_BLOCK);
    HIPCHK(hipMemsetAsync(zero64, 0, z64 * sizeof(*zero64), fr.st));
    HIPCHK(hipMemsetAsync(zero32, 0, z32 * sizeof(*zero32), fr.st));
    HIPCHK(hipMemsetAsync(ones64, 0xff, slots * sizeof(*ones64), fr.st));
    HIPCHK(hipMemsetAsync(ones32, 0xff, o32 * sizeof(*ones32), fr.st));
    HIPCHK(hipMemsetAsync(dinfo, 0, (size_t)std::max<uint32_t>(cap, 1) * sizeof(*dinfo), fr.st));
    FRAME_LAUNCH(fr, k_mc_init, grid_for(nv, MC_BLOCK), block, nv, parent);
    FRAME_LAUNCH(fr, k_mc_unite, grid_for(nt, MC_BLOCK), block, nt, m->tris.p, parent, refd);
    FRAME_LAUNCH(fr, k_mc_flatten, grid_for((size_t)nv + 1, MC_BLOCK), block, nv, m->verts.p, parent, refd, root, flags, acc, ctr);
    FRAME_LAUNCH(fr, k_mc_tris, grid_for(nt, MC_BLOCK), block, nt, m->tris.p, m->verts.p, root, acc, ctr, ones64, hcnt, slots - 1);
    FRAME_LAUNCH(fr, k_mc_edges, grid_for(slots, MC_BLOCK), block, slots, ones64, hcnt, root, acc);
    HIPCHK(hipGetLastError());
    ppf_status r;
    if ((r = frame_scan(fr, flags, cid, (size_t)nv + 1)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_mc_comps, grid_for(np, MC_BLOCK), block, (uint32_t)np, nv, flags, cid, acc.area_q, comp_root, klo, khi, va);
    HIPCHK(hipGetLastError());
    /* stable passes over the low word of ~area_q, then over the high word: (area_q descending, first_vertex ascending) */
    static const int shifts[4] = {0, 8, 16, 24};
    uint32_t* ka = klo;
    if ((r = frame_sort(fr, ka, va, kb, vb, (int)np, hist, offs, shifts, 4)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_frame_gather_u32, grid_for(np, 256), dim3(256), khi, va, (int)np, ka);
    if ((r = frame_sort(fr, ka, va, kb, vb, (int)np, hist, offs, shifts, 4)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_mc_rank, grid_for(np, MC_BLOCK), block, (uint32_t)np, nv, cid, va, comp_root, acc, P, rank_of, keep_of, dinfo, cap, ctr);
    FRAME_LAUNCH(fr, k_mc_flags, grid_for((size_t)std::max(nv, nt) + 1, MC_BLOCK), block, nv, nt, m->tris.p, root, rank_of, keep_of, vkeep, tkeep,
                 dlabels);
    HIPCHK(hipGetLastError());
    if ((r = frame_scan(fr, vkeep, vpos, (size_t)nv + 1)) != PPF_OK || (r = frame_scan(fr, tkeep, tpos, (size_t)nt + 1)) != PPF_OK) return r;
    r = fr.sizing({{"vertices kept", vpos + nv, sizeof(nv_out), &nv_out}, {"triangles kept", tpos + nt, sizeof(nt_out), &nt_out}, {"counters", ctr, sizeof(c), c}});
    if (r != PPF_OK) return r;
    if (!out) return PPF_OK;
    if ((r = mesh_alloc(who, o, nv_out, nt_out)) != PPF_OK) return r;
    FRAME_LAUNCH(fr, k_mc_write_vertices, grid_for((size_t)nv * 6, MC_BLOCK), block, (size_t)nv * 6, reinterpret_cast<const uint32_t*>(m->verts.p),
                 vkeep, vpos, reinterpret_cast<uint32_t*>(o->verts.p));
    FRAME_LAUNCH(fr, k_mc_write_triangles, grid_for((size_t)nt * 3, MC_BLOCK), block, (size_t)nt * 3, m->tris.p, tkeep, tpos, vpos, o->tris.p);
    HIPCHK(hipGetLastError());
    return PPF_OK;
  };
  const ppf_status ran = run();
  const size_t n_info = ran == PPF_OK ? (size_t)std::min<unsigned long long>(c[MC_N_COMPONENTS], cap) : 0;
  /* the end: the scratch goes back to the block cache at scope exit */
  s = fr.finish(who, ran, {{"labels", dlabels, (size_t)nv * sizeof(int32_t), nv ? labels : nullptr},
                           {"info", dinfo, n_info * sizeof(*dinfo), n_info ? info : nullptr}});
  if (s != PPF_OK) return s;
  st.n_components = (int64_t)c[MC_N_COMPONENTS];
  st.n_kept = (int64_t)c[MC_N_KEPT];
  st.n_unreferenced = (int64_t)c[MC_N_UNREFERENCED];
  st.n_bad_area = (int64_t)c[MC_N_BAD_AREA];
  st.n_vertices_out = nv_out;
  st.n_triangles_out = nt_out;
  fr.report(st);
  if (out) *out = o.release();
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_mesh_component_params(ppf_mesh_component_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_triangles = 1;
  p->min_area = 0.f;
  p->rank_lo = 0;
  p->rank_hi = INT32_MAX;
  p->flags = 0;
}

ppf_status ppf_volume_mesh_upload(const float* vertices, int64_t n_vertices, int32_t vstride, int32_t normal_offset, const int32_t* triangles,
                                  int64_t n_triangles, ppf_volume_mesh** out) {
  static const char* who = "ppf_volume_mesh_upload";
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (n_vertices < 0 || n_vertices > INT32_MAX) return fail(PPF_ERR_INVALID, "%s: n_vertices is %lld", who, (long long)n_vertices);
  if (n_triangles < 0 || n_triangles > INT32_MAX) return fail(PPF_ERR_INVALID, "%s: n_triangles is %lld", who, (long long)n_triangles);
  if (n_vertices > 0 && !vertices) return fail(PPF_ERR_INVALID, "%s: vertices is NULL", who);
  if (n_triangles > 0 && !triangles) return fail(PPF_ERR_INVALID, "%s: triangles is NULL", who);
  if (vstride < 3) return fail(PPF_ERR_INVALID, "%s: vstride is %d, a row holds at least x y z", who, vstride);
  if (normal_offset < -1 || (int64_t)normal_offset + 3 > (int64_t)vstride)
    return fail(PPF_ERR_INVALID, "%s: normal_offset %d does not fit a row of %d floats", who, normal_offset, vstride);
  for (int64_t v = 0; v < n_vertices; v++) {
    const float* r = vertices + (size_t)v * vstride;
    if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2])))
      return fail(PPF_ERR_INVALID, "%s: vertex %lld has a position that is not finite", who, (long long)v);
  }
  for (int64_t t = 0; t < n_triangles; t++)
    for (int k = 0; k < 3; k++) {
      const int32_t i = triangles[(size_t)t * 3 + k];
      if (i < 0 || i >= n_vertices)
        return fail(PPF_ERR_INVALID, "%s: triangle %lld names vertex %d of %lld", who, (long long)t, i, (long long)n_vertices);
    }
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  std::unique_ptr<ppf_volume_mesh> m;
  ppf_status s = mesh_alloc(who, m, n_vertices, n_triangles);
  if (s != PPF_OK) return s;
  std::vector<float> rows((size_t)n_vertices * 6, 0.f);
  for (int64_t v = 0; v < n_vertices; v++) {
    const float* r = vertices + (size_t)v * vstride;
    std::memcpy(&rows[(size_t)v * 6], r, 3 * sizeof(float));
    if (normal_offset >= 0) std::memcpy(&rows[(size_t)v * 6 + 3], r + normal_offset, 3 * sizeof(float));
  }
  if (n_vertices) HIPCHK(hipMemcpy(m->verts.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
  if (n_triangles) HIPCHK(hipMemcpy(m->tris.p, triangles, (size_t)n_triangles * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
  *out = m.release();
  return PPF_OK;
}

ppf_status ppf_debug_volume_mesh_shell(int64_t n_vertices, int64_t n_triangles, ppf_volume_mesh** out) {
  static const char* who = "ppf_debug_volume_mesh_shell";
  if (!out) return fail(PPF_ERR_INVALID, "%s: out is NULL", who);
  *out = nullptr;
  if (n_vertices < 0 || n_vertices > INT32_MAX || n_triangles < 0 || n_triangles > INT32_MAX)
    return fail(PPF_ERR_INVALID, "%s: the counts are %lld and %lld", who, (long long)n_vertices, (long long)n_triangles);
  ppf_volume_mesh* m = new (std::nothrow) ppf_volume_mesh();
  if (!m) return fail(PPF_ERR_NOMEM, "%s: out of host memory", who);
  m->nv = n_vertices;
  m->nt = n_triangles;
  *out = m;
  return PPF_OK;
}

ppf_status ppf_volume_mesh_components(const ppf_volume_mesh* m, const ppf_mesh_component_params* p, ppf_volume_mesh** out, int32_t* labels,
                                      ppf_mesh_component_info* info, int cap_info, ppf_mesh_component_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_mesh_component_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed && out) *out = nullptr;
      },
      [&](ppf_mesh_component_stats& st) { return mesh_components("ppf_volume_mesh_components", m, p, out, labels, info, cap_info, st); });
}

}  // extern "C"

#endif /* PPF_MESH_COMPONENTS_HOST_H */
