/*
 * ppf_cluster_kernels.h — the kernels of ppf_prep_clusters: Euclidean cluster extraction, the connected components of
 * "two rows are no farther apart than the tolerance", of K <= 256 clouds at once (host side:
 * ppf_cluster_host.h).  Included by ppf_hip.hip after ppf_prep_kernels.h (frame_find, prep_finite3),
 * ppf_sample_kernels.h (float_to_ordered, the radix-sort passes) and ppf_label_kernels.h (the union-find uf_find / uf_unite,
 * uf_root, cells_lower_bound, wave_max_by_key).
 *
 * The specification is closed -- the link predicate is fp64, evaluated as written, a component is a set, its rank is by
 * integers -- so every output byte equals tests/cluster_oracle.py whatever the order the unions happen in.  The clouds are
 * K segments of one concatenation (CluSeg); a row is named by its index g in it, so a segment's rows are off .. off + n.
 *
 *   grid          cells of edge h = CLU_CELL * tolerance, CLU_CELL a little below 1 / sqrt(3): two rows of one cell are
 *                 always linked, two linked rows are at most two cells apart on an axis (DESIGN.md §20 has the margins).
 *                 Rows are sorted by (segment, cell), stable, so a cell is a run whose first row has its smallest index.
 *   k_clu_link    the hot pass, one wave per occupied cell.  The union-find runs over row indices, so a root is its
 *                 component's smallest row.  The cell's rows are united with its first row; then, for each of the 62
 *                 neighbour cells with a larger key (clu_neighbour: found by binary search in the table of occupied cells),
 *                 lanes own rows of the neighbour and test them against the cell's rows, staged in LDS as fp64 and read by
 *                 broadcast.  A cell pair stops at its first hit: both cells are one set each, so one union per pair of
 *                 cells suffices.  Inside that launch parent[] is read and written by uf_find / uf_unite only
 *                 (ppf_label_kernels.h has the memory rules and why no loop waits).
 */
#ifndef PPF_CLUSTER_KERNELS_H
#define PPF_CLUSTER_KERNELS_H

constexpr int CLU_BLOCK = 256;
constexpr int CLU_TILE = 256;       /* rows of a cell staged in LDS at a time (6 KiB as fp64 x y z) */
constexpr int CLU_AXIS = 1024;      /* cells per axis: 10 bits of the key */
constexpr int CLU_BOUNDS_WGS = 16;  /* workgroups that share a segment's bounds */
constexpr int CLU_ACC = 10;         /* words of a cluster's reduction: ~lo[3], hi[3], ~umin, umax + 1, ~vmin, vmax + 1 */
constexpr double CLU_CELL = 0.5773; /* h / tolerance; 1 / sqrt(3) = 0.57735027 */
constexpr uint32_t CLU_NO_KEY = 0xFFFFFFFFu;
constexpr uint32_t CLU_LOOSE = 0x10000u; /* the gather key of a row in no cluster: past every (segment << 8 | rank) */

struct CluSeg {
  const float* rows; /* the cloud's n x 6 rows */
  const float* curv;
  uint32_t off, n;   /* its rows' place in the concatenation */
};
static_assert(sizeof(CluSeg) == 24, "frame_find walks CluSeg::off with a stride of 6 words");

struct CluGrid {
  double lo[3]; /* the finite rows' minimum */
  double h;
  uint32_t cells[3]; /* cells the extent needs per axis (saturated at 2^31) */
  uint32_t ok;       /* every axis fits CLU_AXIS cells */
};

__device__ __forceinline__ int clu_seg_of(const CluSeg* __restrict__ tab, int K, uint32_t g) { return frame_find(&tab[0].off, 6, K, g); }
__device__ __forceinline__ const float* clu_row(const CluSeg& sg, uint32_t g) { return sg.rows + (size_t)(g - sg.off) * 6; }
/* the rows that take part: those of finite x, y, z; NORMALS (ppf_prep_regions): of finite normals too */
template <bool NORMALS>
__device__ __forceinline__ bool clu_takes(const float* p) { return prep_finite3(p) && (!NORMALS || prep_finite3(p + 3)); }

/* per-segment bounds of the finite rows, as k_frame_bounds keeps them: mm[s][0..2] = ~min, [3..5] = max (ordered words,
 * identity 0), fin[s] = their number; integer atomicMax / atomicAdd on zeroed words.  grid: (K, CLU_BOUNDS_WGS) */
template <bool NORMALS = false>
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_bounds(const CluSeg* __restrict__ tab, uint32_t* __restrict__ mm, uint32_t* __restrict__ fin) {
  const int s = blockIdx.x;
  const CluSeg sg = tab[s];
  uint32_t v[7] = {0, 0, 0, 0, 0, 0, 0};
  for (uint32_t i = blockIdx.y * CLU_BLOCK + threadIdx.x; i < sg.n; i += CLU_BLOCK * gridDim.y) {
    const float* p = sg.rows + (size_t)i * 6;
    if (!clu_takes<NORMALS>(p)) continue;
    v[6]++;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t o = float_to_ordered(p[k]);
      v[k] = max(v[k], ~o);
      v[3 + k] = max(v[3 + k], o);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = max(v[k], (uint32_t)__shfl_down(v[k], o));
    v[6] += (uint32_t)__shfl_down(v[6], o);
  }
  if ((threadIdx.x & 63) == 0 && v[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) atomicMax(&mm[(size_t)s * 6 + k], v[k]);
    atomicAdd(&fin[s], v[6]);
  }
}

/* the cells an extent needs on one axis: floor((hi - lo) / h) + 1, in fp64 as the keys are */
__host__ __device__ __forceinline__ uint32_t clu_axis_cells(double lo, double hi, double h) {
  const double q = (hi - lo) / h;
  return q < 2147483647.0 ? (uint32_t)q + 1u : 0x80000000u;
}

/* a segment's grid.  One thread per segment */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_clu_grid(const uint32_t* __restrict__ mm, const uint32_t* __restrict__ fin, int K, double h,
                                                              CluGrid* __restrict__ grid) {
  const int s = threadIdx.x;
  if (s >= K) return;
  CluGrid g;
  g.h = h;
  g.ok = 1u;
  for (int k = 0; k < 3; k++) {
    g.lo[k] = 0.0;
    g.cells[k] = 0u;
    if (fin[s]) {
      g.lo[k] = (double)ordered_to_float(~mm[(size_t)s * 6 + k]);
      g.cells[k] = clu_axis_cells(g.lo[k], (double)ordered_to_float(mm[(size_t)s * 6 + 3 + k]), h);
      if (g.cells[k] > (uint32_t)CLU_AXIS) g.ok = 0u;
    }
  }
  grid[s] = g;
}

/* per row g: its cell key (10 bits per axis; CLU_NO_KEY: not finite, or its segment's grid does not fit), its segment,
 * and the union-find's start: every row its own parent, every size 0.  grid: rows */
template <bool NORMALS = false>
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_keys(const CluSeg* __restrict__ tab, int K, uint32_t N, const CluGrid* __restrict__ grid,
                                                        uint32_t* __restrict__ lkey, uint32_t* __restrict__ sort_key, uint32_t* __restrict__ skey,
                                                        uint32_t* __restrict__ vals, uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
  const uint32_t g = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (g >= N) return;
  const int s = clu_seg_of(tab, K, g);
  const CluSeg sg = tab[s];
  const float* p = clu_row(sg, g);
  uint32_t key = CLU_NO_KEY;
  if (clu_takes<NORMALS>(p) && grid[s].ok) {
    key = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double q = ((double)p[k] - grid[s].lo[k]) / grid[s].h; /* >= 0 and < CLU_AXIS: lo is the minimum, ok says the maximum fits */
      key = (key << 10) | min((uint32_t)q, (uint32_t)(CLU_AXIS - 1));
    }
  }
  lkey[g] = key;
  sort_key[g] = key;
  skey[g] = (uint32_t)s;
  vals[g] = g;
  parent[g] = g;
  size[g] = 0u;
}

/* does sorted row i (row g = order[i]) start a run of equal (segment, cell)? */
__device__ __forceinline__ uint32_t clu_starts_run(const uint32_t* __restrict__ order, const uint32_t* __restrict__ lkey,
                                                   const uint32_t* __restrict__ skey, uint32_t i, uint32_t g) {
  if (i == 0) return 1u;
  const uint32_t q = order[i - 1];
  return (lkey[q] != lkey[g] || skey[q] != skey[g]) ? 1u : 0u;
}

/* after the sort by (segment, cell): pts[i] = {x, y, z, bits of g} of the i-th row, flags[i] = it starts a run;
 * flags[N] = 0 closes the scan.  grid: rows + 1 */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_runs(const CluSeg* __restrict__ tab, int K, uint32_t N, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ lkey, const uint32_t* __restrict__ skey,
                                                        float4* __restrict__ pts, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i > N) return;
  if (i == N) { flags[N] = 0u; return; }
  const uint32_t g = order[i];
  const float* p = clu_row(tab[skey[g]], g);
  pts[i] = make_float4(p[0], p[1], p[2], __uint_as_float(g));
  flags[i] = clu_starts_run(order, lkey, skey, i, g);
}

/* the table of occupied cells, ascending: ckey[c] = segment << 32 | cell key, cstart[c] = its first sorted row;
 * cstart[cells] = N.  runid = the exclusive scan of flags, runid[N] = the number of cells.  grid: rows + 1 */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_cells(uint32_t N, const uint32_t* __restrict__ order, const uint32_t* __restrict__ lkey,
                                                         const uint32_t* __restrict__ skey, const uint32_t* __restrict__ flags,
                                                         const uint32_t* __restrict__ runid, unsigned long long* __restrict__ ckey,
                                                         uint32_t* __restrict__ cstart) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i > N) return;
  if (i == N) { cstart[runid[N]] = N; return; }
  if (!flags[i]) return;
  const uint32_t g = order[i], c = runid[i];
  ckey[c] = ((unsigned long long)skey[g] << 32) | lkey[g];
  cstart[c] = i;
}

__device__ __forceinline__ bool clu_linked(double ax, double ay, double az, double bx, double by, double bz, double tol2) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return ((dx * dx + dy * dy) + dz * dz) <= tol2;
}

/* Of the 62 cells within two cells per axis of cell c (key `self`) whose key is larger, lane t < 62 looks for the t-th: its
 * sorted rows are *nbs .. *nbe, none (0, 0) where the table of cells does not hold it */
__device__ __forceinline__ void clu_neighbour(const unsigned long long* __restrict__ ckey, const uint32_t* __restrict__ cstart, uint32_t c,
                                              uint32_t nc, unsigned long long self, int lane, uint32_t* nbs, uint32_t* nbe) {
  *nbs = 0;
  *nbe = 0;
  if (lane < 62) {
    const int o = 63 + lane; /* 62 is the cell itself */
    const int cx = (int)((self >> 20) & 1023u) + o / 25 - 2, cy = (int)((self >> 10) & 1023u) + (o / 5) % 5 - 2, cz = (int)(self & 1023u) + o % 5 - 2;
    if (cx >= 0 && cx < CLU_AXIS && cy >= 0 && cy < CLU_AXIS && cz >= 0 && cz < CLU_AXIS) {
      const unsigned long long want = (self & 0xFFFFFFFF00000000ull) | (unsigned long long)(((uint32_t)cx << 20) | ((uint32_t)cy << 10) | (uint32_t)cz);
      const uint32_t lo = cells_lower_bound(ckey, c + 1, nc, want); /* a larger key lies past c */
      if (lo < nc && ckey[lo] == want) { *nbs = cstart[lo]; *nbe = cstart[lo + 1]; }
    }
  }
}

/* one wave per occupied cell.  grid: rows (an upper bound of the cells; workgroups past n_cells[0] leave) */
__global__ __launch_bounds__(64) void k_clu_link(const float4* __restrict__ pts, const unsigned long long* __restrict__ ckey,
                                                 const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ n_cells, double tol2,
                                                 uint32_t* parent) {
  __shared__ double sa[CLU_TILE * 3];
  const uint32_t c = blockIdx.x, nc = n_cells[0];
  if (c >= nc) return;
  const unsigned long long self = ckey[c];
  if ((uint32_t)self == CLU_NO_KEY) return; /* the rows of no cell */
  const int lane = threadIdx.x;
  const uint32_t a0 = cstart[c], a1 = cstart[c + 1];

  uint32_t nbs, nbe;
  clu_neighbour(ckey, cstart, c, nc, self, lane, &nbs, &nbe);
  unsigned long long todo = __ballot(nbe > nbs);

  /* the cell is one set: its first row has its smallest index */
  const uint32_t first = __float_as_uint(pts[a0].w);
  for (uint32_t i = a0 + 1 + (uint32_t)lane; i < a1; i += 64) uf_unite(parent, first, __float_as_uint(pts[i].w));

  for (uint32_t ta = a0; ta < a1 && todo; ta += CLU_TILE) { /* todo is the same in every lane */
    const int nt = (int)min((uint32_t)CLU_TILE, a1 - ta);
    __syncthreads(); /* the last tile's readers are done */
    for (int i = lane; i < nt; i += 64) {
      const float4 q = pts[ta + i];
      sa[i * 3] = (double)q.x; sa[i * 3 + 1] = (double)q.y; sa[i * 3 + 2] = (double)q.z;
    }
    __syncthreads();
    unsigned long long m = todo;
    while (m) {
      const int t = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint32_t bs = (uint32_t)__shfl((int)nbs, t), be = (uint32_t)__shfl((int)nbe, t);
      bool found = false;
      for (uint32_t jb = bs; jb < be && !found; jb += 64) {
        const uint32_t j = jb + (uint32_t)lane;
        bool hit = false;
        if (j < be) {
          const float4 q = pts[j];
          const double bx = (double)q.x, by = (double)q.y, bz = (double)q.z;
#pragma unroll 4
          for (int i = 0; i < nt; i++) hit |= clu_linked(sa[i * 3], sa[i * 3 + 1], sa[i * 3 + 2], bx, by, bz, tol2);
        }
        found = __any(hit);
      }
      if (found) {
        todo &= ~(1ull << t);
        if (lane == 0) uf_unite(parent, first, __float_as_uint(pts[bs].w));
      }
    }
  }
}

/* after the launch boundary plain loads do: root[g] = the root of g (CLU_NO_KEY for a row of no cell), size[root]++.
 * grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_flatten(uint32_t N, const uint32_t* __restrict__ lkey, const uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ root, uint32_t* __restrict__ size) {
  const uint32_t g = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (g >= N) return;
  uint32_t r = CLU_NO_KEY;
  if (lkey[g] != CLU_NO_KEY) {
    r = uf_root(parent, g);
    atomicAdd(&size[r], 1u);
  }
  root[g] = r;
}

/* the ranking's sort key of row g: n - n_rows for the root of a valid component, CLU_NO_KEY for every other row; a stable
 * sort of the rows by it puts a segment's clusters first, largest first and the earlier first_row first among equals.
 * cnt[s] = {valid components, all components}.  grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_valid(const CluSeg* __restrict__ tab, int K, uint32_t N, const uint32_t* __restrict__ root,
                                                         const uint32_t* __restrict__ size, uint32_t min_size, uint32_t max_size,
                                                         uint32_t* __restrict__ sort_key, uint32_t* __restrict__ vals, uint32_t* __restrict__ cnt) {
  const uint32_t g = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (g >= N) return;
  uint32_t key = CLU_NO_KEY;
  if (root[g] == g) {
    const int s = clu_seg_of(tab, K, g);
    const uint32_t n = size[g];
    atomicAdd(&cnt[s * 2 + 1], 1u);
    if (min_size <= n && (max_size == 0u || n <= max_size)) {
      atomicAdd(&cnt[s * 2], 1u);
      key = tab[s].n - n;
    }
  }
  sort_key[g] = key;
  vals[g] = g;
}

/* position i of the ranking's order lies in the segment of row i, at rank i - off: rank[g] = it, for the root of one of the
 * segment's clusters, else -1; the cluster's size and first row.  grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_rank(const CluSeg* __restrict__ tab, int K, uint32_t N, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ size, int max_clusters,
                                                        int32_t* __restrict__ rank, int32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int s = clu_seg_of(tab, K, i);
  const uint32_t g = order[i], r = i - tab[s].off;
  const bool in = r < cnt[s * 2] && r < (uint32_t)max_clusters;
  rank[g] = in ? (int32_t)r : -1;
  if (in) {
    head[((size_t)s * max_clusters + r) * 2] = (int32_t)size[g];
    head[((size_t)s * max_clusters + r) * 2 + 1] = (int32_t)(g - tab[s].off);
  }
}

/* labels[g] = the rank of g's cluster or -1, and the gather's sort key: segment << 8 | rank, CLU_LOOSE for a row of no
 * cluster.  grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_labels(uint32_t N, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ root,
                                                          const int32_t* __restrict__ rank, int32_t* __restrict__ labels,
                                                          uint32_t* __restrict__ sort_key, uint32_t* __restrict__ vals) {
  const uint32_t g = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (g >= N) return;
  const int32_t l = root[g] != CLU_NO_KEY ? rank[root[g]] : -1;
  labels[g] = l;
  sort_key[g] = l >= 0 ? (skey[g] << 8) | (uint32_t)l : CLU_LOOSE;
  vals[g] = g;
}

/* the clusters' rows, cluster after cluster in (segment, rank) order and in row order inside one: position i of that order
 * is row i of the output block.  grid: rows */
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_gather(const CluSeg* __restrict__ tab, uint32_t N, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ order, float* __restrict__ out_rows,
                                                          float* __restrict__ out_curv) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  if (i >= N || keys[i] == CLU_LOOSE) return;
  const uint32_t g = order[i];
  const CluSeg sg = tab[keys[i] >> 8];
  const float* p = clu_row(sg, g);
  float* o = out_rows + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; k++) o[k] = p[k];
  out_curv[i] = sg.curv[g - sg.off];
}

/* acc[segment][rank] = the maxima of {~lo, hi, ~umin, umax + 1, ~vmin, vmax + 1} over a cluster's rows, zero the identity of
 * all ten: ordered words and integers only.  The image words come from the rows with z > 0 (intr == NULL: none).  A wave
 * that lies in one cluster, as most do, combines by shuffles and adds once (wave_max_by_key).  grid: rows */
struct CluIntr {
  double fx, fy, ppx, ppy;
  int rows, cols, on;
};
__device__ __forceinline__ uint32_t clu_pixel(double a, double z, double f, double pp, int size) {
  const double v = floor(((a / z) * f + pp) + 0.5);
  return (uint32_t)(v >= 0.0 ? (v <= (double)(size - 1) ? (int)v : size - 1) : 0); /* NaN cannot occur: a, z finite, z > 0 */
}
__global__ __launch_bounds__(CLU_BLOCK) void k_clu_reduce(const CluSeg* __restrict__ tab, uint32_t N, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ order, CluIntr cam, int max_clusters,
                                                          uint32_t* __restrict__ acc) {
  const uint32_t i = blockIdx.x * CLU_BLOCK + threadIdx.x;
  const uint32_t key = i < N ? keys[i] : CLU_LOOSE;
  const bool in = key != CLU_LOOSE;
  uint32_t v[CLU_ACC];
#pragma unroll
  for (int k = 0; k < CLU_ACC; k++) v[k] = 0u;
  if (in) {
    const uint32_t g = order[i];
    const float* p = clu_row(tab[key >> 8], g);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t o = float_to_ordered(p[k]);
      v[k] = ~o;
      v[3 + k] = o;
    }
    if (cam.on && p[2] > 0.f) {
      const uint32_t pu = clu_pixel((double)p[0], (double)p[2], cam.fx, cam.ppx, cam.cols), pv = clu_pixel((double)p[1], (double)p[2], cam.fy, cam.ppy, cam.rows);
      v[6] = ~pu; v[7] = pu + 1u; v[8] = ~pv; v[9] = pv + 1u;
    }
  }
  uint32_t k1 = key;
  if (!wave_max_by_key(in, k1, v)) return;
  uint32_t* dst = acc + ((size_t)(k1 >> 8) * max_clusters + (k1 & 255u)) * CLU_ACC;
#pragma unroll
  for (int k = 0; k < CLU_ACC; k++)
    if (v[k]) atomicMax(&dst[k], v[k]);
}

#endif /* PPF_CLUSTER_KERNELS_H */
