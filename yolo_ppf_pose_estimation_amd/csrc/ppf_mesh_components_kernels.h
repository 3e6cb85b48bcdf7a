/*
 * ppf_mesh_components_kernels.h — a triangle mesh's connected components on gfx950: counted, measured, ranked by area and
 * filtered (ppf_volume_mesh_components).  Included by ppf_hip.hip after ppf_label_kernels.h (uf_unite,
 * uf_root) and ppf_sample_kernels.h (float_to_ordered, the radix sort); host side: ppf_mesh_components_host.h.
 *
 *   k_mc_init     parent[v] = v.
 *   k_mc_unite    one lane per triangle: its three vertices are marked referenced and united.  A lane skips a pair when the
 *                 lane before it in the wave holds a triangle with both vertices: that lane unites them itself in this
 *                 launch (triangles arrive in cube order, neighbours share an edge more often than not).
 *   k_mc_flatten  after the launch boundary: root[v] by plain loads (MC_NONE when unreferenced), the root flags for the scan,
 *                 and the per-vertex sums (count, bounds) at the root's index.
 *   k_mc_tris     one lane per triangle: the area in fp64 as COMPONENTS writes it, its integer form, the triangle sums at the
 *                 root's index, and the three edges of a non-degenerate triangle into the edge table.
 *   k_mc_edges    one lane per slot of the edge table: the edge's three counts at its component's root.
 *   k_mc_comps    after the scan of the root flags: the components in first_vertex order, and the sort's keys ~area_q.
 *   k_mc_rank     after the sort: rank -> component; kept or not; the info records; rank and keep flag at the root's index.
 *   k_mc_flags    keep flags per vertex and per triangle for the two scans, and the labels.
 *   k_mc_write_vertices / k_mc_write_triangles   the gather passes: a place is a scan's value, never an atomic's.
 *
 * Sums by component.  Every sum is an integer (counts, area_q, ordered-uint bounds), so the result does not depend on the
 * order.  A wave whose live lanes lie in one component -- almost every wave of a scan, which is one huge component and some
 * scraps -- combines by shuffles and adds once (mc_wave_sum, as wave_max_by_key does for maxima); a mixed wave adds lane by
 * lane.  k_mc_edges is the exception: the hash scatters a component's edges, so it takes one round of ballots per component
 * present in the wave.
 *
 * The edge table.  Open addressing with linear probing over `slots` 64-bit keys (min << 32 | max), slots a power of two of
 * at least twice the keys inserted, all bits set meaning empty (no key has them: an index is below 2^31).  A slot is claimed
 * by a 64-bit compare-and-swap and never given up; the count is an integer add on the slot's word.  Why the loop ends: at most
 * slots / 2 keys are ever inserted, so an empty slot always exists; a probe that fails steps to the next slot, and after at
 * most `slots` steps it has met the key's own slot or an empty one, which it then claims or finds claimed by the same key.
 * No lane waits for another.
 *
 * No float atomic, no inline assembly, no grid-wide synchronisation, no private memory.
 */
#ifndef PPF_MESH_COMPONENTS_KERNELS_H
#define PPF_MESH_COMPONENTS_KERNELS_H

constexpr int MC_BLOCK = 256;
constexpr uint32_t MC_NONE = 0xFFFFFFFFu;            /* root[] of an unreferenced vertex */
constexpr unsigned long long MC_EMPTY = ~0ull;       /* an unclaimed slot of the edge table */
/* counters of a call */
constexpr int MC_N_COMPONENTS = 0, MC_N_KEPT = 1, MC_N_UNREFERENCED = 2, MC_N_BAD_AREA = 3, MC_COUNTERS = 4;

/* the sums of a call, all indexed by a component's root vertex */
struct McAcc {
  uint32_t *n_vert, *n_tri, *n_deg, *n_edge, *n_bound, *n_nonman; /* nv each */
  unsigned long long* area_q;                                     /* nv */
  uint32_t *lo, *hi;                                              /* 3 x nv each, ordered uints; lo starts at all ones */
};

struct McParams {
  int32_t min_triangles, rank_lo, rank_hi;
  double min_area;
};

/* Every lane of the wave calls it: `in` says the lane holds v[] (zero otherwise) for the component `key`.  When the live lanes
 * lie in one component, lane 0 ends up with the sums and that key and is the only lane that adds; otherwise every live lane
 * adds its own.  Returns whether this lane adds */
template <class T, int W>
__device__ __forceinline__ bool mc_wave_sum(bool in, uint32_t& key, T (&v)[W]) {
  const unsigned long long live = __ballot(in);
  if (!live) return false;
  const uint32_t key0 = (uint32_t)__shfl((int)key, __ffsll((long long)live) - 1);
  if (__all(!in || key == key0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < W; k++) v[k] += __shfl_down(v[k], o);
    }
    if ((threadIdx.x & 63) != 0) return false;
    key = key0;
    return true;
  }
  return in;
}

/* lanes with `flag` in the wave, added to *ctr by one of them */
__device__ __forceinline__ void mc_count(bool flag, unsigned long long* ctr) {
  const unsigned long long b = __ballot(flag);
  if (b && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)b) - 1)) atomicAdd(ctr, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_init(uint32_t nv, uint32_t* __restrict__ parent) {
  const size_t v = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (v < nv) parent[v] = (uint32_t)v;
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_unite(uint32_t nt, const int32_t* __restrict__ tris, uint32_t* parent,
                                                       uint32_t* __restrict__ refd) {
  const size_t t = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const bool in = t < nt;
  uint32_t i0 = 0, i1 = 0, i2 = 0;
  if (in) {
    i0 = (uint32_t)tris[t * 3];
    i1 = (uint32_t)tris[t * 3 + 1];
    i2 = (uint32_t)tris[t * 3 + 2];
  }
  /* the triangle of the lane before (lane 0, and the lane after a dead one, see their own: nothing is skipped there) */
  const uint32_t p0 = (uint32_t)__shfl_up((int)i0, 1), p1 = (uint32_t)__shfl_up((int)i1, 1), p2 = (uint32_t)__shfl_up((int)i2, 1);
  if (!in) return;
  refd[i0] = 1u; /* every writer writes 1 */
  refd[i1] = 1u;
  refd[i2] = 1u;
  const bool prev = (threadIdx.x & 63) != 0; /* the lane before is live: t - 1 < t < nt */
  const bool h0 = prev && (i0 == p0 || i0 == p1 || i0 == p2), h1 = prev && (i1 == p0 || i1 == p1 || i1 == p2),
             h2 = prev && (i2 == p0 || i2 == p1 || i2 == p2);
  if (i0 != i1 && !(h0 && h1)) uf_unite(parent, i0, i1);
  if (i0 != i2 && i1 != i2 && !(h0 && h2)) uf_unite(parent, i0, i2); /* i1 == i2: the first pair was this one */
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_flatten(uint32_t nv, const float* __restrict__ verts, const uint32_t* __restrict__ parent,
                                                         const uint32_t* __restrict__ refd, uint32_t* __restrict__ root,
                                                         uint32_t* __restrict__ flags /* nv + 1 */, McAcc acc,
                                                         unsigned long long* __restrict__ ctr) {
  const size_t v = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const bool in = v < nv && refd[v] != 0u;
  uint32_t r = in ? uf_root(parent, (uint32_t)v) : MC_NONE;
  if (v < nv) root[v] = r;
  if (v <= nv) flags[v] = in && r == (uint32_t)v ? 1u : 0u;
  mc_count(v < nv && !in, ctr + MC_N_UNREFERENCED);
  uint32_t lo[3] = {MC_NONE, MC_NONE, MC_NONE}, hi[3] = {0u, 0u, 0u};
  uint32_t cnt[1] = {in ? 1u : 0u};
  if (in) {
#pragma unroll
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = float_to_ordered(verts[v * 6 + k]);
  }
  const unsigned long long live = __ballot(in);
  if (!live) return;
  const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll((long long)live) - 1);
  bool add = in;
  if (__all(!in || r == r0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt[0] += (uint32_t)__shfl_down((int)cnt[0], o);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        lo[k] = min(lo[k], (uint32_t)__shfl_down((int)lo[k], o));
        hi[k] = max(hi[k], (uint32_t)__shfl_down((int)hi[k], o));
      }
    }
    add = (threadIdx.x & 63) == 0;
    r = r0;
  }
  if (!add) return;
  atomicAdd(acc.n_vert + r, cnt[0]);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    atomicMin(acc.lo + (size_t)k * nv + r, lo[k]);
    atomicMax(acc.hi + (size_t)k * nv + r, hi[k]);
  }
}

__device__ __forceinline__ void mc_edge_insert(unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hcnt, size_t mask, uint32_t a,
                                               uint32_t b) {
  const unsigned long long key = (unsigned long long)min(a, b) << 32 | (unsigned long long)max(a, b);
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  size_t slot = (size_t)h & mask;
  for (;;) {
    const unsigned long long was = atomicCAS(hkeys + slot, MC_EMPTY, key);
    if (was == MC_EMPTY || was == key) break;
    slot = (slot + 1) & mask;
  }
  atomicAdd(hcnt + slot, 1u);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_tris(uint32_t nt, const int32_t* __restrict__ tris, const float* __restrict__ verts,
                                                      const uint32_t* __restrict__ root, McAcc acc, unsigned long long* __restrict__ ctr,
                                                      unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hcnt, size_t mask) {
  const size_t t = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const bool in = t < nt;
  uint32_t i0 = 0, i1 = 0, i2 = 0, r = MC_NONE;
  bool deg = false, bad = false;
  unsigned long long q[1] = {0ull};
  if (in) {
    i0 = (uint32_t)tris[t * 3];
    i1 = (uint32_t)tris[t * 3 + 1];
    i2 = (uint32_t)tris[t * 3 + 2];
    r = root[i0];
    deg = i0 == i1 || i1 == i2 || i0 == i2;
    const float *p0 = verts + (size_t)i0 * 6, *p1 = verts + (size_t)i1 * 6, *p2 = verts + (size_t)i2 * 6;
    const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
    const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    const double s = A * 1099511627776.0; /* 2^40 */
    bad = !(s < 9223372036854775808.0);   /* not finite, or >= 2^63 */
    if (!bad) q[0] = (unsigned long long)s;
  }
  mc_count(bad, ctr + MC_N_BAD_AREA);
  uint32_t c[2] = {in ? 1u : 0u, deg ? 1u : 0u};
  uint32_t rq = r;
  if (mc_wave_sum(in, rq, q) && q[0]) atomicAdd(acc.area_q + rq, q[0]);
  if (mc_wave_sum(in, r, c)) {
    atomicAdd(acc.n_tri + r, c[0]);
    if (c[1]) atomicAdd(acc.n_deg + r, c[1]);
  }
  if (in && !deg) {
    mc_edge_insert(hkeys, hcnt, mask, i0, i1);
    mc_edge_insert(hkeys, hcnt, mask, i1, i2);
    mc_edge_insert(hkeys, hcnt, mask, i2, i0);
  }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_edges(size_t slots, const unsigned long long* __restrict__ hkeys,
                                                       const uint32_t* __restrict__ hcnt, const uint32_t* __restrict__ root, McAcc acc) {
  const size_t s = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const unsigned long long key = s < slots ? hkeys[s] : MC_EMPTY;
  const bool in = key != MC_EMPTY;
  uint32_t r = MC_NONE, c[3] = {0u, 0u, 0u};
  if (in) {
    const uint32_t m = hcnt[s];
    r = root[(uint32_t)(key >> 32)];
    c[0] = 1u;
    c[1] = m == 1u ? 1u : 0u;
    c[2] = m > 2u ? 1u : 0u;
  }
  /* the hash scatters a component's edges over the table, so a wave holds the edges of several components: one round per
   * component present, its three counts by ballots, added by its first lane (the loop's condition is the same in every lane) */
  const uint32_t lane = threadIdx.x & 63;
  for (unsigned long long todo = __ballot(in); todo;) {
    const int first = __ffsll((long long)todo) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)r, first);
    const bool mine = in && r == r0;
    const unsigned long long same = __ballot(mine), b1 = __ballot(mine && c[1]), b2 = __ballot(mine && c[2]);
    if (lane == (uint32_t)first) {
      atomicAdd(acc.n_edge + r0, (uint32_t)__popcll(same));
      if (b1) atomicAdd(acc.n_bound + r0, (uint32_t)__popcll(b1));
      if (b2) atomicAdd(acc.n_nonman + r0, (uint32_t)__popcll(b2));
    }
    todo &= ~same;
  }
}

/* n = max(nv, 1) lanes.  cid = the exclusive scan of the root flags: cid[root] is the component's place in first_vertex order
 * and cid[nv] = C.  A root writes slot cid[root] < C, lane i >= C pads slot i: no slot has two writers.  The padding's keys are
 * all ones, like those of a component of area 0, and stay behind every component because the sort is stable */
__global__ __launch_bounds__(MC_BLOCK) void k_mc_comps(uint32_t n, uint32_t nv, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ cid,
                                                       const unsigned long long* __restrict__ area_q, uint32_t* __restrict__ comp_root,
                                                       uint32_t* __restrict__ klo, uint32_t* __restrict__ khi, uint32_t* __restrict__ val) {
  const size_t i = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t C = cid[nv];
  if (i < nv && flags[i]) {
    const uint32_t c = cid[i];
    const unsigned long long k = ~area_q[i];
    comp_root[c] = (uint32_t)i;
    klo[c] = (uint32_t)k;
    khi[c] = (uint32_t)(k >> 32);
  }
  if (i >= C) klo[i] = khi[i] = MC_NONE;
  val[i] = (uint32_t)i;
}

/* n = max(nv, 1) lanes, one per rank.  order[r]: the component (in first_vertex order) of rank r */
__global__ __launch_bounds__(MC_BLOCK) void k_mc_rank(uint32_t n, uint32_t nv, const uint32_t* __restrict__ cid, const uint32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ comp_root, McAcc acc, McParams P,
                                                      uint32_t* __restrict__ rank_of, uint32_t* __restrict__ keep_of,
                                                      ppf_mesh_component_info* __restrict__ info, uint32_t cap_info,
                                                      unsigned long long* __restrict__ ctr) {
  const size_t i = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t C = cid[nv];
  const bool in = i < n && i < C;
  bool kept = false;
  if (in) {
    const uint32_t r = (uint32_t)i, root = comp_root[order[r]];
    const double area = (double)acc.area_q[root] * (1.0 / 1099511627776.0);
    const uint32_t n_tri = acc.n_tri[root];
    kept = (long long)r >= (long long)P.rank_lo && (long long)r < (long long)P.rank_hi && n_tri >= (uint32_t)P.min_triangles && area >= P.min_area;
    rank_of[root] = r;
    keep_of[root] = kept ? 1u : 0u;
    if (r < cap_info) {
      ppf_mesh_component_info& o = info[r]; /* the array was cleared: reserved stays 0 */
      o.n_vertices = (int32_t)acc.n_vert[root];
      o.n_triangles = (int32_t)n_tri;
      o.n_degenerate = (int32_t)acc.n_deg[root];
      o.n_edges = (int32_t)acc.n_edge[root];
      o.n_boundary_edges = (int32_t)acc.n_bound[root];
      o.n_nonmanifold_edges = (int32_t)acc.n_nonman[root];
      o.first_vertex = (int32_t)root;
      o.kept = kept ? 1 : 0;
      o.area = area;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        o.lo[k] = ordered_to_float(acc.lo[(size_t)k * nv + root]);
        o.hi[k] = ordered_to_float(acc.hi[(size_t)k * nv + root]);
      }
    }
  }
  mc_count(kept, ctr + MC_N_KEPT);
  if (i == 0) ctr[MC_N_COMPONENTS] = C;
}

/* max(nv, nt) + 1 lanes: lane i has vertex i and triangle i; vkeep and tkeep hold one word more than the mesh, 0, for the
 * scans' totals */
__global__ __launch_bounds__(MC_BLOCK) void k_mc_flags(uint32_t nv, uint32_t nt, const int32_t* __restrict__ tris, const uint32_t* __restrict__ root,
                                                       const uint32_t* __restrict__ rank_of, const uint32_t* __restrict__ keep_of,
                                                       uint32_t* __restrict__ vkeep, uint32_t* __restrict__ tkeep, int32_t* __restrict__ labels) {
  const size_t i = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i <= nv) {
    const uint32_t r = i < nv ? root[i] : MC_NONE;
    vkeep[i] = r != MC_NONE ? keep_of[r] : 0u;
    if (i < nv) labels[i] = r != MC_NONE ? (int32_t)rank_of[r] : -1;
  }
  if (i <= nt) tkeep[i] = i < nt ? keep_of[root[(uint32_t)tris[i * 3]]] : 0u;
}

/* one lane per word of the input's vertex rows: the kept rows, every byte as it is */
__global__ __launch_bounds__(MC_BLOCK) void k_mc_write_vertices(size_t n_words, const uint32_t* __restrict__ in, const uint32_t* __restrict__ vkeep,
                                                                const uint32_t* __restrict__ vpos, uint32_t* __restrict__ out) {
  const size_t w = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (w >= n_words) return;
  const size_t v = w / 6;
  if (vkeep[v]) out[(size_t)vpos[v] * 6 + (w - v * 6)] = in[w];
}

/* one lane per index of the input's triangles: a kept triangle's vertices are all kept, vpos is their new number */
__global__ __launch_bounds__(MC_BLOCK) void k_mc_write_triangles(size_t n_words, const int32_t* __restrict__ in, const uint32_t* __restrict__ tkeep,
                                                                 const uint32_t* __restrict__ tpos, const uint32_t* __restrict__ vpos,
                                                                 int32_t* __restrict__ out) {
  const size_t w = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (w >= n_words) return;
  const size_t t = w / 3;
  if (tkeep[t]) out[(size_t)tpos[t] * 3 + (w - t * 3)] = (int32_t)vpos[(uint32_t)in[w]];
}

#endif /* PPF_MESH_COMPONENTS_KERNELS_H */
