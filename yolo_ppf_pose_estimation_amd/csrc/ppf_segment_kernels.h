/*
 * ppf_segment_kernels.h — the kernels of ppf_depth_segments: the connected surfaces of a depth image, labelled in image space
 * (host side: ppf_segment_host.h).  Included by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_pixel),
 * ppf_sample_kernels.h (float_to_ordered, the radix-sort passes) and ppf_label_kernels.h (uf_find, uf_unite, uf_root, agent_ld,
 * wave_max_by_key).
 *
 * The specification is closed -- step and agree are fp64 expressions evaluated as written, a component is a set, its rank is by
 * integers -- so every output byte equals tests/depth_segments_oracle.py whatever the order the unions happen in.  A pixel is
 * named by p = v * cols + u.  The image is cut into tiles of SEG_TW x SEG_TH pixels; inside a tile local index
 * i = ly * SEG_TW + lx grows with p, so "the smaller index" means the same thing in a tile and in the image.
 *
 *   k_seg_classify  per pixel its class (SEG_OUT / SEG_KEPT / SEG_SMOOTH / SEG_BORDER) and a record {z, nx, ny, nz}.  With a
 *                   normals cloud the pixel's row is its rank among the kept pixels: k_depth_count's tile counts, scanned,
 *                   plus the ballot rank inside the tile, exactly as k_depth_scatter places rows.  A rank at or past the
 *                   cloud's row count reads nothing (the pixel gets SEG_KEPT; the host refuses the call after its one wait).
 *                   Also the start of everything per pixel: size, border count 0, rank -1.
 *   k_seg_tile      one 256-thread workgroup per tile, four pixels a thread.  Records and classes are staged in LDS; a
 *                   union-find over the tile's 1,024 pixels runs entirely in LDS with uf_find / uf_unite on a shared array
 *                   (each smooth pixel unites with its right, lower and, for 8-connectivity, two lower diagonal neighbours
 *                   inside the tile).  After a barrier every pixel walks to its local root and writes the global
 *                   parent[p] = that root's pixel index; a pixel that is not smooth is its own parent.
 *   k_seg_merge     the links that cross a tile edge: one thread per pixel, only those of a tile's last column, last row or
 *                   (diagonals) first column do anything; uf_unite on the global parent[].
 *   k_seg_flatten   one workgroup per tile.  A smooth pixel walks to its root; a border pixel picks its smooth neighbour by
 *                   the border rule from the global records and takes that pixel's root.  The tile then counts its pixels per
 *                   root in an LDS hash table (a wave that lies in one set inserts once with its popcount) and issues one
 *                   global atomicAdd per distinct root it holds -- not one per pixel, which is what made k_reg_flatten
 *                   2.4 ms on a frame whose largest region holds most rows.
 *   k_seg_valid     the ranking's sort key per pixel (N - n_pixels for the root of a valid component, N for every other),
 *                   the counts of valid and all components by ballots.
 *   k_seg_rank      after the stable sort: the first min(valid, max_segments) positions are the segments.
 *   k_seg_labels    the label image and the per-segment maxima of {~umin, umax + 1, ~vmin, vmax + 1, ~z_lo, z_hi}: integers
 *                   and ordered words only.  A workgroup gathers the maxima of 1,024 pixels per segment in LDS (a wave that
 *                   lies in one segment combines by shuffles and adds once) and issues a global atomicMax only for a word
 *                   that still raises the total: one add per wave on the words of the frame's largest segment cost 1.05 ms.
 *
 * Why every loop ends.  The union-find's loops end by ppf_label_kernels.h's argument; uf_root is used by k_seg_tile after its
 * barrier and by k_seg_flatten after a launch boundary.  The hash insert of k_seg_flatten probes a table of 2 * SEG_TILE slots
 * that receives at most SEG_TILE distinct keys, so a free or equal slot is always met.  No workgroup waits for another.
 * Inside k_seg_merge parent[] is touched by uf_unite only.
 */
#ifndef PPF_SEGMENT_KERNELS_H
#define PPF_SEGMENT_KERNELS_H

constexpr int SEG_TW = 64, SEG_TH = 16; /* a tile: one wave spans a tile row, 16 rows keep the edge pixels at 1/6 of all */
constexpr int SEG_TILE = SEG_TW * SEG_TH;
constexpr int SEG_BLOCK = 256;
constexpr int SEG_PER = SEG_TILE / SEG_BLOCK; /* pixels a thread owns: local index threadIdx.x + k * SEG_BLOCK */
constexpr int SEG_HASH = 2 * SEG_TILE;
constexpr int SEG_ACC = 6; /* ~umin, umax + 1, ~vmin, vmax + 1, ~z_lo, z_hi */
constexpr uint32_t SEG_NONE = 0xFFFFFFFFu;
constexpr uint8_t SEG_OUT = 0, SEG_KEPT = 1, SEG_SMOOTH = 2, SEG_BORDER = 3;
/* the zeroed block of a call, in words */
constexpr int SEG_C_KEPT = 0, SEG_C_ELIGIBLE = 1, SEG_C_SMOOTH = 2, SEG_C_ATTACHED = 3, SEG_C_VALID = 4, SEG_C_ALL = 5, SEG_N_COUNTERS = 8;
constexpr int SEG_HEAD = 3; /* n_pixels, first_pixel, n_border per segment */
static_assert(SEG_TW == 64 && SEG_BLOCK == 256 && SEG_PER == 4, "a wave spans a tile row");

struct SegArgs {
  int rows, cols, tiles_x, tiles_y;
  int eight, unoriented;
  double depth_abs, depth_quad, normal_cos;
  float curvature_threshold;
  const float* nrm_rows; /* the normals cloud's n x 6 rows, or NULL */
  const float* nrm_curv;
  uint32_t nrm_n;
};

__device__ __forceinline__ bool seg_step(double zp, double zq, const SegArgs& sa) {
  return ppf_fabs(zq - zp) <= sa.depth_abs + sa.depth_quad * (zp * zq);
}
__device__ __forceinline__ bool seg_agree(const float4& a, const float4& b, const SegArgs& sa) {
  if (!sa.nrm_rows) return true;
  double dot = ((double)a.y * (double)b.y + (double)a.z * (double)b.z) + (double)a.w * (double)b.w;
  if (sa.unoriented) dot = ppf_fabs(dot);
  return dot >= sa.normal_cos;
}
__device__ __forceinline__ bool seg_link(const float4& a, const float4& b, const SegArgs& sa) {
  return seg_step((double)a.x, (double)b.x, sa) && seg_agree(a, b, sa);
}

/* grid: the DEPTH_TILE tiles of k_depth_count.  tile_off: the scanned counts (NULL without a normals cloud) */
template <class T>
__global__ __launch_bounds__(DEPTH_BLOCK) void k_seg_classify(DepthArgs a, SegArgs sa, const uint32_t* __restrict__ tile_off,
                                                              float4* __restrict__ rec, uint8_t* __restrict__ cls, uint32_t* __restrict__ size,
                                                              uint32_t* __restrict__ nbord, int32_t* __restrict__ rank) {
  __shared__ uint32_t cnt[DEPTH_ROUNDS][DEPTH_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * DEPTH_TILE;
  bool keep[DEPTH_ROUNDS];
  float z[DEPTH_ROUNDS];
  uint32_t below[DEPTH_ROUNDS];
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    const int p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    int u, v;
    z[r] = 0.f;
    keep[r] = p < a.n && depth_pixel<T>(a, p, &u, &v, &z[r]);
    const unsigned long long m = __ballot(keep[r]);
    below[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) cnt[r][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t off = tile_off ? tile_off[blockIdx.x] : 0u;
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    uint32_t o = off;
#pragma unroll
    for (int w = 0; w < DEPTH_BLOCK / 64; w++) {
      if (w < wv) o += cnt[r][w];
      off += cnt[r][w];
    }
    const int p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    if (p >= a.n) continue;
    float4 q = make_float4(z[r], 0.f, 0.f, 0.f);
    uint8_t c = SEG_OUT;
    if (keep[r]) {
      c = SEG_SMOOTH;
      if (sa.nrm_rows) {
        const uint32_t row = o + below[r];
        c = SEG_KEPT;
        if (row < sa.nrm_n) {
          const float* nr = sa.nrm_rows + (size_t)row * 6;
          q.y = nr[3]; q.z = nr[4]; q.w = nr[5];
          if (isfinite(q.y) && isfinite(q.z) && isfinite(q.w)) c = sa.nrm_curv[row] <= sa.curvature_threshold ? SEG_SMOOTH : SEG_BORDER;
        }
      }
    }
    rec[p] = q;
    cls[p] = c;
    size[p] = 0u;
    nbord[p] = 0u;
    rank[p] = -1;
  }
}

/* grid: tiles_x * tiles_y */
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_tile(SegArgs sa, const float4* __restrict__ rec, const uint8_t* __restrict__ cls,
                                                        uint32_t* __restrict__ parent) {
  __shared__ float4 s_rec[SEG_TILE];
  __shared__ uint8_t s_cls[SEG_TILE];
  __shared__ uint32_t s_par[SEG_TILE];
  const int tile_y = (int)blockIdx.x / sa.tiles_x, tile_x = (int)blockIdx.x - tile_y * sa.tiles_x;
  const int u0 = tile_x * SEG_TW, v0 = tile_y * SEG_TH;
#pragma unroll
  for (int k = 0; k < SEG_PER; k++) {
    const int i = (int)threadIdx.x + k * SEG_BLOCK, lx = i & (SEG_TW - 1), ly = i >> 6;
    const int u = u0 + lx, v = v0 + ly;
    uint8_t c = SEG_OUT;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u < sa.cols && v < sa.rows) {
      const size_t p = (size_t)v * (size_t)sa.cols + (size_t)u;
      c = cls[p];
      q = rec[p];
    }
    s_cls[i] = c;
    s_rec[i] = q;
    s_par[i] = (uint32_t)i;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_PER; k++) {
    const int i = (int)threadIdx.x + k * SEG_BLOCK, lx = i & (SEG_TW - 1), ly = i >> 6;
    if (s_cls[i] != SEG_SMOOTH) continue;
    const float4 me = s_rec[i];
    if (lx + 1 < SEG_TW && s_cls[i + 1] == SEG_SMOOTH && seg_link(me, s_rec[i + 1], sa)) uf_unite(s_par, (uint32_t)i, (uint32_t)(i + 1));
    if (ly + 1 < SEG_TH) {
      const int d = i + SEG_TW;
      if (s_cls[d] == SEG_SMOOTH && seg_link(me, s_rec[d], sa)) uf_unite(s_par, (uint32_t)i, (uint32_t)d);
      if (sa.eight) {
        if (lx > 0 && s_cls[d - 1] == SEG_SMOOTH && seg_link(me, s_rec[d - 1], sa)) uf_unite(s_par, (uint32_t)i, (uint32_t)(d - 1));
        if (lx + 1 < SEG_TW && s_cls[d + 1] == SEG_SMOOTH && seg_link(me, s_rec[d + 1], sa)) uf_unite(s_par, (uint32_t)i, (uint32_t)(d + 1));
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_PER; k++) {
    const int i = (int)threadIdx.x + k * SEG_BLOCK, lx = i & (SEG_TW - 1), ly = i >> 6;
    const int u = u0 + lx, v = v0 + ly;
    if (u >= sa.cols || v >= sa.rows) continue;
    const uint32_t r = uf_root(s_par, (uint32_t)i); /* nobody writes s_par after the barrier */
    const int rx = (int)r & (SEG_TW - 1), ry = (int)r >> 6;
    parent[(size_t)v * (size_t)sa.cols + (size_t)u] = (uint32_t)(v0 + ry) * (uint32_t)sa.cols + (uint32_t)(u0 + rx);
  }
}

/* grid: pixels */
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_merge(SegArgs sa, const float4* __restrict__ rec, const uint8_t* __restrict__ cls,
                                                         uint32_t* parent) {
  const uint32_t p = blockIdx.x * SEG_BLOCK + threadIdx.x;
  if (p >= (uint32_t)sa.rows * (uint32_t)sa.cols) return;
  const int v = (int)(p / (uint32_t)sa.cols), u = (int)(p - (uint32_t)v * (uint32_t)sa.cols);
  const int lx = u & (SEG_TW - 1), ly = v & (SEG_TH - 1);
  const bool last_x = lx == SEG_TW - 1, last_y = ly == SEG_TH - 1, first_x = lx == 0;
  if (!last_x && !last_y && !(sa.eight && first_x)) return;
  if (cls[p] != SEG_SMOOTH) return;
  const float4 me = rec[p];
  const bool right = u + 1 < sa.cols, down = v + 1 < sa.rows;
  if (last_x && right) {
    const uint32_t q = p + 1u;
    if (cls[q] == SEG_SMOOTH && seg_link(me, rec[q], sa)) uf_unite(parent, p, q);
  }
  if (down) {
    const uint32_t d = p + (uint32_t)sa.cols;
    if (last_y && cls[d] == SEG_SMOOTH && seg_link(me, rec[d], sa)) uf_unite(parent, p, d);
    if (sa.eight) {
      if (u > 0 && (last_y || first_x) && cls[d - 1u] == SEG_SMOOTH && seg_link(me, rec[d - 1u], sa)) uf_unite(parent, p, d - 1u);
      if (right && (last_y || last_x) && cls[d + 1u] == SEG_SMOOTH && seg_link(me, rec[d + 1u], sa)) uf_unite(parent, p, d + 1u);
    }
  }
}

/* grid: tiles_x * tiles_y.  counters: SEG_C_KEPT .. SEG_C_ATTACHED */
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_flatten(SegArgs sa, const float4* __restrict__ rec, const uint8_t* __restrict__ cls,
                                                           const uint32_t* __restrict__ parent, uint32_t* __restrict__ root,
                                                           uint32_t* __restrict__ size, uint32_t* __restrict__ nbord, uint32_t* __restrict__ counters) {
  __shared__ uint32_t h_key[SEG_HASH], h_cnt[SEG_HASH], h_bor[SEG_HASH];
  __shared__ uint32_t s_n[4];
  for (int i = threadIdx.x; i < SEG_HASH; i += SEG_BLOCK) {
    h_key[i] = SEG_NONE;
    h_cnt[i] = 0u;
    h_bor[i] = 0u;
  }
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const int tile_y = (int)blockIdx.x / sa.tiles_x, tile_x = (int)blockIdx.x - tile_y * sa.tiles_x;
  const int u0 = tile_x * SEG_TW, v0 = tile_y * SEG_TH;
  const int lane = threadIdx.x & 63;
  uint32_t n_kept = 0, n_elig = 0, n_smooth = 0, n_att = 0;
#pragma unroll 1
  for (int k = 0; k < SEG_PER; k++) {
    const int i = (int)threadIdx.x + k * SEG_BLOCK, lx = i & (SEG_TW - 1), ly = i >> 6;
    const int u = u0 + lx, v = v0 + ly;
    const bool inside = u < sa.cols && v < sa.rows;
    const uint32_t p = inside ? (uint32_t)v * (uint32_t)sa.cols + (uint32_t)u : 0u;
    const uint8_t c = inside ? cls[p] : SEG_OUT;
    uint32_t r = SEG_NONE;
    if (c == SEG_SMOOTH) {
      r = uf_root(parent, p);
    } else if (c == SEG_BORDER) {
      const float4 me = rec[p];
      double best = 0.0;
      uint32_t bq = SEG_NONE;
      /* the neighbours in ascending pixel index: the first of equal distances wins */
      for (int dv = -1; dv <= 1; dv++)
        for (int du = -1; du <= 1; du++) {
          if ((du == 0 && dv == 0) || (!sa.eight && du != 0 && dv != 0)) continue;
          const int qu = u + du, qv = v + dv;
          if (qu < 0 || qu >= sa.cols || qv < 0 || qv >= sa.rows) continue;
          const uint32_t q = (uint32_t)qv * (uint32_t)sa.cols + (uint32_t)qu;
          if (cls[q] != SEG_SMOOTH) continue;
          const float4 o = rec[q];
          if (!seg_link(me, o, sa)) continue;
          const double d = ppf_fabs((double)o.x - (double)me.x);
          if (bq == SEG_NONE || d < best) {
            best = d;
            bq = q;
          }
        }
      if (bq != SEG_NONE) r = uf_root(parent, bq);
    }
    if (inside) root[p] = r;
    const bool in = r != SEG_NONE, bor = in && c == SEG_BORDER;
    const unsigned long long live = __ballot(in), mb = __ballot(bor);
    n_kept += (uint32_t)__popcll(__ballot(c != SEG_OUT));
    n_elig += (uint32_t)__popcll(__ballot(c == SEG_SMOOTH || c == SEG_BORDER));
    n_smooth += (uint32_t)__popcll(__ballot(c == SEG_SMOOTH));
    n_att += (uint32_t)__popcll(mb);
    if (!live) continue;
    const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll((long long)live) - 1);
    const bool one = __all(!in || r == r0);
    uint32_t add = 1u, addb = bor ? 1u : 0u;
    bool ins = in;
    if (one) {
      ins = lane == __ffsll((long long)live) - 1;
      add = (uint32_t)__popcll(live);
      addb = (uint32_t)__popcll(mb);
    }
    if (ins) {
      uint32_t h = (r * 2654435761u) >> 21; /* 11 bits: SEG_HASH slots */
      for (;;) {
        const uint32_t prev = atomicCAS(&h_key[h], SEG_NONE, r);
        if (prev == SEG_NONE || prev == r) break;
        h = (h + 1u) & (uint32_t)(SEG_HASH - 1);
      }
      atomicAdd(&h_cnt[h], add);
      if (addb) atomicAdd(&h_bor[h], addb);
    }
  }
  if (lane == 0) {
    if (n_kept) atomicAdd(&s_n[0], n_kept);
    if (n_elig) atomicAdd(&s_n[1], n_elig);
    if (n_smooth) atomicAdd(&s_n[2], n_smooth);
    if (n_att) atomicAdd(&s_n[3], n_att);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SEG_HASH; i += SEG_BLOCK) {
    const uint32_t r = h_key[i];
    if (r == SEG_NONE) continue;
    atomicAdd(&size[r], h_cnt[i]);
    if (h_bor[i]) atomicAdd(&nbord[r], h_bor[i]);
  }
  if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&counters[SEG_C_KEPT + threadIdx.x], s_n[threadIdx.x]);
}
static_assert(SEG_HASH == 2048, "the hash keeps 11 bits");

/* grid: pixels */
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_valid(uint32_t N, const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                                                         uint32_t min_size, uint32_t max_size, uint32_t* __restrict__ sort_key,
                                                         uint32_t* __restrict__ vals, uint32_t* __restrict__ counters) {
  const uint32_t p = blockIdx.x * SEG_BLOCK + threadIdx.x;
  bool is_root = false, valid = false;
  if (p < N) {
    uint32_t key = N;
    if (root[p] == p) {
      const uint32_t n = size[p];
      is_root = true;
      valid = min_size <= n && (max_size == 0u || n <= max_size);
      if (valid) key = N - n;
    }
    sort_key[p] = key;
    vals[p] = p;
  }
  const unsigned long long mr = __ballot(is_root), mv = __ballot(valid);
  if ((threadIdx.x & 63) == 0) {
    if (mr) atomicAdd(&counters[SEG_C_ALL], (uint32_t)__popcll(mr));
    if (mv) atomicAdd(&counters[SEG_C_VALID], (uint32_t)__popcll(mv));
  }
}

/* one workgroup of PPF_CLUSTER_MAX_CLUSTERS threads: position i of the ranking's order is segment i */
__global__ __launch_bounds__(PPF_CLUSTER_MAX_CLUSTERS) void k_seg_rank(uint32_t N, const uint32_t* __restrict__ order, const uint32_t* __restrict__ counters,
                                                                       const uint32_t* __restrict__ size, const uint32_t* __restrict__ nbord,
                                                                       int max_segments, int32_t* __restrict__ rank, int32_t* __restrict__ head) {
  const uint32_t i = threadIdx.x;
  if (i >= N || i >= counters[SEG_C_VALID] || i >= (uint32_t)max_segments) return;
  const uint32_t g = order[i];
  rank[g] = (int32_t)i;
  head[i * SEG_HEAD] = (int32_t)size[g];
  head[i * SEG_HEAD + 1] = (int32_t)g;
  head[i * SEG_HEAD + 2] = (int32_t)nbord[g];
}

/* grid: spans of SEG_TILE consecutive pixels.  The span's maxima per segment are gathered in LDS first (a wave that lies in
 * one segment combines by shuffles and adds once: wave_max_by_key), then one global atomicMax per word that still raises the
 * total: a stale read of the total (agent_ld) is never above it, so a skipped add is one that could not have changed it */
__global__ __launch_bounds__(SEG_BLOCK) void k_seg_labels(uint32_t N, int cols, const uint32_t* __restrict__ root, const int32_t* __restrict__ rank,
                                                          const float4* __restrict__ rec, int32_t* __restrict__ labels, uint32_t* acc) {
  __shared__ uint32_t s_acc[PPF_CLUSTER_MAX_CLUSTERS * SEG_ACC];
  for (int i = threadIdx.x; i < PPF_CLUSTER_MAX_CLUSTERS * SEG_ACC; i += SEG_BLOCK) s_acc[i] = 0u;
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < SEG_PER; k++) {
    const uint32_t p = blockIdx.x * (uint32_t)SEG_TILE + (uint32_t)k * SEG_BLOCK + threadIdx.x; /* N <= INT32_MAX: no wrap */
    int32_t l = -1;
    uint32_t v[SEG_ACC];
#pragma unroll
    for (int j = 0; j < SEG_ACC; j++) v[j] = 0u;
    if (p < N) {
      const uint32_t r = root[p];
      if (r != SEG_NONE) l = rank[r];
      labels[p] = l;
      if (l >= 0) {
        const uint32_t pv = p / (uint32_t)cols, pu = p - pv * (uint32_t)cols, o = float_to_ordered(rec[p].x);
        v[0] = ~pu; v[1] = pu + 1u; v[2] = ~pv; v[3] = pv + 1u; v[4] = ~o; v[5] = o;
      }
    }
    uint32_t l1 = (uint32_t)l;
    if (wave_max_by_key(l >= 0, l1, v)) {
#pragma unroll
      for (int j = 0; j < SEG_ACC; j++)
        if (v[j]) atomicMax(&s_acc[l1 * SEG_ACC + j], v[j]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PPF_CLUSTER_MAX_CLUSTERS * SEG_ACC; i += SEG_BLOCK) {
    const uint32_t m = s_acc[i];
    if (m && agent_ld(acc + i) < m) atomicMax(acc + i, m);
  }
}

#endif /* PPF_SEGMENT_KERNELS_H */
