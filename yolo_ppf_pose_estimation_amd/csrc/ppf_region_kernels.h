/*
 * ppf_region_kernels.h — the kernels ppf_prep_regions adds to ppf_prep_clusters': smooth surface regions, the connected
 * components of "two smooth rows are near and their normals agree", with the border rows attached afterwards (DESIGN.md §22;
 * host side: ppf_region_host.h).  Included by ppf_hip.hip after ppf_cluster_kernels.h: the grid, the sorts, the table of cells,
 * the neighbour-cell lookup (clu_neighbour) and the whole tail from k_clu_valid on are that file's; the union-find (uf_find /
 * uf_unite, uf_root) and cells_lower_bound are ppf_label_kernels.h's.
 *
 *   k_reg_runs     the sorted rows as two float4: {x, y, z, index} and {nx, ny, nz, kind}
 *   k_reg_link     the hot pass, one wave per occupied cell.  §20's guarantee (2) holds (linked rows are at most two cells
 *                  apart on an axis); guarantee (1) does not: two rows of one cell may disagree in normal, so a cell's rows are
 *                  tested against each other and a pair of cells cannot stop at its first hit.  What is cut instead is the
 *                  union of two rows the lane knows to be in one set already (RgnTile::r, below).
 *   k_reg_flatten  after the launch boundary, plain loads: every smooth row its root, the sizes counted
 *   k_reg_attach   every border row to the nearest smooth row it can attach to
 * (ppf_register_kernels.h has k_reg_ kernels and REG_ constants of its own, the depth registration's; the helpers here are
 * rgn_ / RGN_.)  The memory rules inside k_reg_link are k_clu_link's: parent[] is read and written by uf_find / uf_unite only.
 */
#ifndef PPF_REGION_KERNELS_H
#define PPF_REGION_KERNELS_H

constexpr uint32_t RGN_NONE = 0u, RGN_SMOOTH = 1u, RGN_BORDER = 2u; /* a sorted row's kind */

/* agree(): the normals' fp64 dot product against normal_cos, |dot| with PPF_REGION_UNORIENTED */
__device__ __forceinline__ bool rgn_agree(double ax, double ay, double az, double bx, double by, double bz, double cosv, bool unoriented) {
  const double dot = (ax * bx + ay * by) + az * bz;
  return (unoriented ? fabs(dot) : dot) >= cosv;
}

/* k_clu_runs with the normal and the kind beside the point: a row of a cell (k_clu_keys<true> gave it a key: x, y, z and the
 * normal are finite) is smooth iff curvature <= threshold, a float comparison that a NaN fails.  grid: rows + 1 */
__global__ __launch_bounds__(CLU_BLOCK) void k_reg_runs(const CluSeg* __restrict__ tab, uint32_t N, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ lkey, const uint32_t* __restrict__ skey, float curv_thr,
                                                        float4* __restrict__ pts, float4* __restrict__ nrm, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i > N) return;
  if (i == N) { flags[N] = 0u; return; }
  const uint32_t g = order[i];
  const CluSeg sg = tab[skey[g]];
  const float* p = clu_row(sg, g);
  uint32_t kind = RGN_NONE;
  if (lkey[g] != CLU_NO_KEY) kind = sg.curv[g - sg.off] <= curv_thr ? RGN_SMOOTH : RGN_BORDER;
  pts[i] = make_float4(p[0], p[1], p[2], __uint_as_float(g));
  nrm[i] = make_float4(p[3], p[4], p[5], __uint_as_float(kind));
  flags[i] = clu_starts_run(order, lkey, skey, i, g);
}

/* The staged tile of the wave's cell: xyz as fp64 (what near() takes), the normal (widened where agree() is reached, for the
 * few pairs that are near), g[] the row's index (CLU_NO_KEY: not smooth, no partner of a link), r[] a row that was in the
 * staged row's set when it was read (uf_find's answer).  Sets only ever merge, so two staged rows of equal r[] are in one set
 * for good. */
struct RgnTile {
  double p[CLU_TILE * 3];
  float n[CLU_TILE * 3];
  uint32_t g[CLU_TILE], r[CLU_TILE];
};

/* Lanes own the sorted rows b0 .. b1 and test them against the staged rows 0 .. nt (TRI: against the staged rows before their
 * own place only, b0 being the tile's first row: every pair of the tile once).  A hit is united unless the lane knows the two
 * rows to be in one set: `known` is r[] of the staged row its own row was last united with, so its row, that staged row and
 * every staged row of the same r[] are one set already.  A skipped union is one that would have found two equal roots. */
template <bool TRI>
__device__ __forceinline__ void rgn_pass(const RgnTile& t, int nt, const float4* __restrict__ pts, const float4* __restrict__ nrm, uint32_t b0,
                                         uint32_t b1, double tol2, double cosv, bool unoriented, uint32_t* parent, int lane) {
  for (uint32_t jb = b0; jb < b1; jb += 64) {
    const uint32_t j = jb + (uint32_t)lane;
    if (j >= b1) continue;
    const float4 m = nrm[j];
    if (__float_as_uint(m.w) != RGN_SMOOTH) continue;
    const float4 q = pts[j];
    const double bx = (double)q.x, by = (double)q.y, bz = (double)q.z, mx = (double)m.x, my = (double)m.y, mz = (double)m.z;
    const uint32_t gj = __float_as_uint(q.w);
    const int lim = TRI ? min(nt, (int)(j - b0)) : nt;
    uint32_t known = CLU_NO_KEY;
    for (int i = 0; i < lim; i++) {
      const uint32_t gi = t.g[i];
      if (gi == CLU_NO_KEY) continue;
      if (!clu_linked(t.p[i * 3], t.p[i * 3 + 1], t.p[i * 3 + 2], bx, by, bz, tol2)) continue;
      if (!rgn_agree((double)t.n[i * 3], (double)t.n[i * 3 + 1], (double)t.n[i * 3 + 2], mx, my, mz, cosv, unoriented)) continue;
      const uint32_t ri = t.r[i];
      if (ri == known) continue;
      uf_unite(parent, gi, gj);
      known = ri;
    }
  }
}

/* one wave per occupied cell.  Per tile of 256 of its rows: the tile against itself, r[] read again (most of a surface
 * patch's rows now share a root), then the cell's later rows and the 62 neighbour cells of a larger key against the tile.
 * grid: rows (an upper bound of the cells; workgroups past n_cells[0] leave) */
__global__ __launch_bounds__(64) void k_reg_link(const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                 const unsigned long long* __restrict__ ckey, const uint32_t* __restrict__ cstart,
                                                 const uint32_t* __restrict__ n_cells, double tol2, double cosv, int unoriented,
                                                 uint32_t* parent) {
  __shared__ RgnTile t;
  const uint32_t c = blockIdx.x, nc = n_cells[0];
  if (c >= nc) return;
  const unsigned long long self = ckey[c];
  if ((uint32_t)self == CLU_NO_KEY) return; /* the rows of no cell */
  const int lane = threadIdx.x;
  const uint32_t a0 = cstart[c], a1 = cstart[c + 1];

  uint32_t nbs, nbe;
  clu_neighbour(ckey, cstart, c, nc, self, lane, &nbs, &nbe);
  const unsigned long long todo = __ballot(nbe > nbs);

  for (uint32_t ta = a0; ta < a1; ta += CLU_TILE) {
    const int nt = (int)min((uint32_t)CLU_TILE, a1 - ta);
    __syncthreads(); /* the last tile's readers are done */
    bool any = false;
    for (int i = lane; i < nt; i += 64) {
      const float4 q = pts[ta + i], m = nrm[ta + i];
      const bool smooth = __float_as_uint(m.w) == RGN_SMOOTH;
      const uint32_t g = __float_as_uint(q.w);
      t.p[i * 3] = (double)q.x; t.p[i * 3 + 1] = (double)q.y; t.p[i * 3 + 2] = (double)q.z;
      t.n[i * 3] = m.x; t.n[i * 3 + 1] = m.y; t.n[i * 3 + 2] = m.z;
      t.g[i] = smooth ? g : CLU_NO_KEY;
      t.r[i] = smooth ? uf_find(parent, g) : CLU_NO_KEY;
      any |= smooth;
    }
    __syncthreads();
    if (!__any(any)) continue; /* no smooth row staged: nothing can link to this tile */
    rgn_pass<true>(t, nt, pts, nrm, ta, ta + (uint32_t)nt, tol2, cosv, unoriented != 0, parent, lane);
    __syncthreads();
    for (int i = lane; i < nt; i += 64)
      if (t.g[i] != CLU_NO_KEY) t.r[i] = uf_find(parent, t.g[i]);
    __syncthreads();
    rgn_pass<false>(t, nt, pts, nrm, ta + (uint32_t)nt, a1, tol2, cosv, unoriented != 0, parent, lane);
    unsigned long long m = todo;
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint32_t bs = (uint32_t)__shfl((int)nbs, l), be = (uint32_t)__shfl((int)nbe, l);
      rgn_pass<false>(t, nt, pts, nrm, bs, be, tol2, cosv, unoriented != 0, parent, lane);
    }
  }
}

/* after the launch boundary plain loads do.  Per sorted row: root[g] = the root of a smooth row, size[root]++; CLU_NO_KEY for
 * every other row (a border row gets its root in k_reg_attach).  grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_reg_flatten(uint32_t N, const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                           const uint32_t* __restrict__ parent, uint32_t* __restrict__ root,
                                                           uint32_t* __restrict__ size) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i >= N) return;
  const uint32_t g = __float_as_uint(pts[i].w);
  uint32_t r = CLU_NO_KEY;
  if (__float_as_uint(nrm[i].w) == RGN_SMOOTH) {
    r = uf_root(parent, g);
    atomicAdd(&size[r], 1u);
  }
  root[g] = r;
}

/* One thread per sorted row; a border row looks at the 125 cells around its own, in both directions: the five cells along z
 * of one (x, y) have consecutive keys, so they are one run of the sorted rows, found by one binary search in the table of
 * cells.  It takes the smallest (bits of the squared distance, row index) over the smooth rows that are near and agree (the
 * distance is >= 0: its bits order it), and joins that row's component: root[] of smooth rows is final since k_reg_flatten
 * and only read here, the border row's own root[] is written by this thread alone.  att[segment] counts the attached rows.
 * grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_reg_attach(uint32_t N, const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                          const uint32_t* __restrict__ lkey, const uint32_t* __restrict__ skey,
                                                          const unsigned long long* __restrict__ ckey, const uint32_t* __restrict__ cstart,
                                                          const uint32_t* __restrict__ n_cells, double tol2, double cosv, int unoriented,
                                                          uint32_t* root, uint32_t* __restrict__ size, uint32_t* __restrict__ att) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i >= N) return;
  const float4 m = nrm[i];
  if (__float_as_uint(m.w) != RGN_BORDER) return;
  const float4 q = pts[i];
  const uint32_t g = __float_as_uint(q.w), key = lkey[g], seg = skey[g], nc = n_cells[0];
  const double bx = (double)q.x, by = (double)q.y, bz = (double)q.z, mx = (double)m.x, my = (double)m.y, mz = (double)m.z;
  const int cx = (int)((key >> 20) & 1023u), cy = (int)((key >> 10) & 1023u), cz = (int)(key & 1023u);
  const uint32_t z0 = (uint32_t)max(cz - 2, 0), z1 = (uint32_t)min(cz + 2, CLU_AXIS - 1);
  unsigned long long best_d = ~0ull;
  uint32_t best_g = CLU_NO_KEY;
  for (int o = 0; o < 25; o++) {
    const int x = cx + o / 5 - 2, y = cy + o % 5 - 2;
    if (x < 0 || x >= CLU_AXIS || y < 0 || y >= CLU_AXIS) continue;
    const unsigned long long base = ((unsigned long long)seg << 32) | (unsigned long long)(((uint32_t)x << 20) | ((uint32_t)y << 10));
    const uint32_t lo = cells_lower_bound(ckey, 0, nc, base | z0);
    uint32_t ce = lo; /* at most five cells on */
    while (ce < nc && ckey[ce] <= (base | z1)) ce++;
    if (ce == lo) continue;
    for (uint32_t j = cstart[lo], je = cstart[ce]; j < je; j++) {
      const float4 a = nrm[j];
      if (__float_as_uint(a.w) != RGN_SMOOTH) continue;
      const float4 p = pts[j];
      const double dx = (double)p.x - bx, dy = (double)p.y - by, dz = (double)p.z - bz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (!(d2 <= tol2) || !rgn_agree((double)a.x, (double)a.y, (double)a.z, mx, my, mz, cosv, unoriented != 0)) continue;
      const unsigned long long d = (unsigned long long)__double_as_longlong(d2);
      const uint32_t ga = __float_as_uint(p.w);
      if (d < best_d || (d == best_d && ga < best_g)) { best_d = d; best_g = ga; }
    }
  }
  if (best_g == CLU_NO_KEY) return;
  const uint32_t r = root[best_g];
  root[g] = r;
  atomicAdd(&size[r], 1u);
  atomicAdd(&att[seg], 1u);
}

#endif /* PPF_REGION_KERNELS_H */
