/*
 * ppf_plane_kernels.h — the kernels of ppf_prep_planes / ppf_prep_planes_apply: a frame's support planes (the table, a
 * wall) found by a seeded hypothesis search and taken out of K <= 256 clouds at once (host side:
 * ppf_plane_host.h).  Included by ppf_hip.hip after ppf_prep_kernels.h (frame_find, prep_smallest_eigvec) and
 * ppf_refine_kernels.h (rfn_wave_sum).
 *
 * The specification is closed -- u32 hashing, fp64 + - * / sqrt evaluated as written, exact integer counts, sums by one
 * fixed tree -- so every output byte equals tests/plane_oracle.py.  The clouds are K segments of one concatenation
 * (PlnSeg: where a cloud's rows lie and its offset in it); a segment's live rows L sit, in order, in the first m slots of
 * its span as float4 {x, y, z, bits of the row's index in the cloud}.  m lives on the device (PlnWork): grids are sized
 * for the rows the host knows and workgroups past m leave, so no round waits for the host.  Rows are dealt out in tiles
 * of PLN_TILE rows from a segment's start (a tile is two levels of the sum tree, and eight spans of the counting pass).
 *
 *   k_pln_count   the hot pass.  Lanes own hypotheses: the four fp64 coefficients of one plane live in a lane's
 *                 registers and so does its count.  A workgroup stages PLN_SPAN rows in LDS, widened to fp64 once; then
 *                 every lane reads the same row (a same-address LDS read broadcasts: one ds_read serves 64 tests), with
 *                 no cross-lane step, and one integer atomicAdd per hypothesis per workgroup at the end.
 *   k_pln_sum     the refit's sums: one wave per 64 rows by the fixed tree (rfn_wave_sum), 64 of those per workgroup by
 *                 the same tree; k_pln_finish carries the tree on over a segment's tiles and fits the plane.
 */
#ifndef PPF_PLANE_KERNELS_H
#define PPF_PLANE_KERNELS_H

constexpr int PLN_BLOCK = 256;
constexpr int PLN_SPAN = 512;                   /* rows a counting workgroup stages in LDS (16 KiB as fp64 x y z pad) */
constexpr int PLN_TILE = 4096;                  /* rows of a tile: 64 x 64, two levels of the sum tree */
constexpr int PLN_SPANS = PLN_TILE / PLN_SPAN;  /* counting workgroups per tile */

struct PlnSeg {
  const float* rows; /* the cloud's n x 6 rows */
  const float* curv;
  uint32_t off, n;   /* its rows' place in the concatenation */
  uint32_t tile0;    /* its first tile; a cloud has ceil(n / PLN_TILE) of them */
  uint32_t pad;
};
static_assert(sizeof(PlnSeg) == 32, "frame_find walks PlnSeg::tile0 with a stride of 8 words");

/* a plane is {n0, n1, n2, d}; an invalid one is {0, 0, 0, NaN}: its s is NaN for every row, so it counts nothing */
struct PlnWork {
  uint32_t m;           /* |L| */
  int32_t done;         /* an earlier round ended the search */
  int32_t act;          /* this round removes a plane */
  int32_t best_h, k0;   /* the best hypothesis and its count */
  uint32_t k1;          /* the refitted plane's count */
  int32_t pad[2];
  double P0[4], c[3], P1[4], P[4]; /* hypothesis, centroid, refit, the plane that is removed */
};

__device__ __forceinline__ uint32_t pln_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ double pln_s(const double* P, double x, double y, double z) { return ((P[0] * x + P[1] * y) + P[2] * z) + P[3]; }
__device__ __forceinline__ bool pln_inlier(double s, double thr) { return __builtin_fabs(s) <= thr; }
__device__ __forceinline__ bool pln_finite4(const double* P) { return isfinite(P[0]) && isfinite(P[1]) && isfinite(P[2]) && isfinite(P[3]); }
__device__ __forceinline__ void pln_invalid(double* P) { P[0] = 0.0; P[1] = 0.0; P[2] = 0.0; P[3] = __builtin_nan(""); }
/* the segment of tile t */
__device__ __forceinline__ int pln_seg_of(const PlnSeg* __restrict__ tab, int K, uint32_t t) { return frame_find(&tab[0].tile0, 8, K, t); }
/* the rows of a workgroup this wave's lanes flag: one atomicAdd per wave */
__device__ __forceinline__ void pln_wave_count(bool flag, uint32_t* dst) {
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(dst, (uint32_t)__popcll(b));
}

/* L = every row, labels = 0, m = n.  grid: tiles */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_load(const PlnSeg* __restrict__ tab, int K, float4* __restrict__ lp, uint8_t* __restrict__ labels,
                                                        PlnWork* __restrict__ work) {
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const uint32_t base = (t - sg.tile0) * PLN_TILE;
  if (base == 0 && threadIdx.x == 0) work[s].m = sg.n;
  for (uint32_t j = base + threadIdx.x; j < min(sg.n, base + PLN_TILE); j += PLN_BLOCK) {
    const float* p = sg.rows + (size_t)j * 6;
    lp[sg.off + j] = make_float4(p[0], p[1], p[2], __uint_as_float(j));
    labels[sg.off + j] = 0;
  }
}

/* round r's hypotheses of every segment, and their counts zeroed.  grid: (ceil(H / PLN_BLOCK), K) */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_hyp(const PlnSeg* __restrict__ tab, const PlnWork* __restrict__ work, const float4* __restrict__ lp,
                                                       int r, uint32_t seed, int H, double* __restrict__ hyp, uint32_t* __restrict__ cnt) {
  const int s = blockIdx.y, h = blockIdx.x * PLN_BLOCK + threadIdx.x;
  if (h >= H) return;
  cnt[(size_t)s * H + h] = 0u;
  double* P = hyp + ((size_t)s * H + h) * 4;
  pln_invalid(P);
  const uint32_t m = work[s].m;
  if (work[s].done || m < 3u) return;
  const uint32_t base = pln_mix(seed + 0x9e3779b9u * (uint32_t)(r + 1));
  double a[3], e1[3], e2[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t idx = (uint32_t)(((unsigned long long)pln_mix(pln_mix(base ^ (uint32_t)h) ^ k) * (unsigned long long)m) >> 32);
    const float4 q = lp[tab[s].off + idx];
    const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
    if (k == 0) { a[0] = x; a[1] = y; a[2] = z; }
    else if (k == 1) { e1[0] = x - a[0]; e1[1] = y - a[1]; e1[2] = z - a[2]; }
    else { e2[0] = x - a[0]; e2[1] = y - a[1]; e2[2] = z - a[2]; }
  }
  double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (!(isfinite(l2) && l2 > 0.0)) return;
  const double len = ppf_sqrt(l2);
  n[0] /= len; n[1] /= len; n[2] /= len;
  double d = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]);
  if (d < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; d = -d; }
  P[0] = n[0]; P[1] = n[1]; P[2] = n[2]; P[3] = d;
}

/* cnt[s][h] += the inliers of hypothesis h among one span of L.  grid: (tiles * PLN_SPANS, ceil(H / PLN_BLOCK)) */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_count(const PlnSeg* __restrict__ tab, int K, const PlnWork* __restrict__ work,
                                                         const float4* __restrict__ lp, const double* __restrict__ hyp, int H, double thr,
                                                         uint32_t* __restrict__ cnt) {
  __shared__ double sp[PLN_SPAN * 4];
  const uint32_t t = blockIdx.x / PLN_SPANS;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const uint32_t m = work[s].m, start = (t - sg.tile0) * PLN_TILE + (blockIdx.x % PLN_SPANS) * PLN_SPAN;
  if (work[s].done || m < 3u || start >= m) return; /* uniform over the workgroup */
  const int rows = (int)min((uint32_t)PLN_SPAN, m - start);
  for (int i = threadIdx.x; i < rows; i += PLN_BLOCK) {
    const float4 q = lp[sg.off + start + i];
    sp[i * 4] = (double)q.x; sp[i * 4 + 1] = (double)q.y; sp[i * 4 + 2] = (double)q.z;
  }
  __syncthreads();
  const int h = blockIdx.y * PLN_BLOCK + threadIdx.x;
  if (blockIdx.y * PLN_BLOCK + (threadIdx.x & ~63) >= H) return; /* a wave without a hypothesis */
  double P[4];
  if (h < H) {
    const double* src = hyp + ((size_t)s * H + h) * 4;
    P[0] = src[0]; P[1] = src[1]; P[2] = src[2]; P[3] = src[3];
  } else {
    pln_invalid(P);
  }
  uint32_t c = 0;
#pragma unroll 4
  for (int i = 0; i < rows; i++) c += pln_inlier(pln_s(P, sp[i * 4], sp[i * 4 + 1], sp[i * 4 + 2]), thr) ? 1u : 0u;
  if (c) atomicAdd(&cnt[(size_t)s * H + h], c); /* c != 0 only where h < H */
}

/* the round's verdict per segment: the best hypothesis (largest count, lowest h), NONE / REJECTED / on to the removal.
 * grid: K */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_best(PlnWork* __restrict__ work, const double* __restrict__ hyp, const uint32_t* __restrict__ cnt,
                                                        int H, int min_inliers, double min_share, int r, int max_planes,
                                                        ppf_plane_info* __restrict__ info) {
  __shared__ unsigned long long sh[PLN_BLOCK];
  const int s = blockIdx.x, tid = threadIdx.x;
  PlnWork* w = &work[s];
  const uint32_t m = w->m;
  const bool idle = w->done || m < 3u;
  unsigned long long key = 0; /* count << 32 | ~h: the maximum is the largest count, then the lowest h */
  if (!idle)
    for (int h = tid; h < H; h += PLN_BLOCK) key = max(key, ((unsigned long long)cnt[(size_t)s * H + h] << 32) | (uint32_t)~(uint32_t)h);
  sh[tid] = key;
  __syncthreads();
  for (int o = PLN_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = max(sh[tid], sh[tid + o]);
    __syncthreads();
  }
  if (tid != 0) return;
  w->act = 0;
  if (idle) { w->done = 1; return; }
  const uint32_t count = (uint32_t)(sh[0] >> 32);
  const int h = (int)~(uint32_t)sh[0];
  const double* P = hyp + ((size_t)s * H + h) * 4;
  ppf_plane_info* ir = &info[(size_t)s * max_planes + r];
  const bool valid = P[3] == P[3];
  for (int k = 0; k < 3; k++) ir->n[k] = valid ? P[k] : 0.0;
  ir->d = valid ? P[3] : 0.0;
  ir->hypothesis = h;
  ir->n_rows = (int32_t)m;
  ir->n_hyp_inliers = (int32_t)count;
  if ((int64_t)count < (int64_t)min_inliers || (double)count < min_share * (double)m) {
    ir->status = PPF_PLANE_REJECTED;
    w->done = 1;
    return;
  }
  ir->status = PPF_PLANE_REMOVED;
  ir->n_inliers = (int32_t)count;
  w->act = 1;
  w->best_h = h;
  w->k0 = (int32_t)count;
  w->k1 = 0u;
  for (int k = 0; k < 4; k++) { w->P0[k] = P[k]; w->P[k] = P[k]; }
}

/* the refit's sums over the inliers of P0, each value at its row's place in L and +0.0 elsewhere: part[t][e] = tile t's
 * two levels of the tree.  NV = 3: x, y, z;  NV = 6: the products of the rows' offsets from the centroid.  grid: tiles */
template <int NV>
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_sum(const PlnSeg* __restrict__ tab, int K, const PlnWork* __restrict__ work,
                                                       const float4* __restrict__ lp, double thr, double* __restrict__ part) {
  __shared__ double sh[NV][64];
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const PlnWork* w = &work[s];
  const uint32_t m = w->m, base = (t - sg.tile0) * PLN_TILE;
  if (!w->act || base >= m) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double P[4] = {w->P0[0], w->P0[1], w->P0[2], w->P0[3]}, c[3] = {w->c[0], w->c[1], w->c[2]};
  for (int ch = wave; ch < 64; ch += PLN_BLOCK / 64) {
    const uint32_t j = base + (uint32_t)ch * 64u + (uint32_t)lane;
    double v[NV];
#pragma unroll
    for (int e = 0; e < NV; e++) v[e] = 0.0;
    if (j < m) {
      const float4 q = lp[sg.off + j];
      const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
      if (pln_inlier(pln_s(P, x, y, z), thr)) {
        if constexpr (NV == 3) {
          v[0] = x; v[1] = y; v[2] = z;
        } else {
          const double d0 = x - c[0], d1 = y - c[1], d2 = z - c[2];
          v[0] = d0 * d0; v[1] = d0 * d1; v[2] = d0 * d2; v[3] = d1 * d1; v[4] = d1 * d2; v[5] = d2 * d2;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < NV; e++) {
      const double r = rfn_wave_sum(v[e]);
      if (lane == 0) sh[e][ch] = r;
    }
  }
  __syncthreads();
  const bool one = m <= 64u; /* one value is left after the first level: the tree ends there */
  for (int e = wave; e < NV; e += PLN_BLOCK / 64) {
    const double r = rfn_wave_sum(sh[e][lane]);
    if (lane == 0) part[(size_t)t * NV + e] = one ? sh[e][0] : r;
  }
}

/* the rest of the tree over a segment's `count` tile sums src[i * NV + e], by one workgroup: 64 at a time, level by level
 * through the segment's slots of A and B, until one value is left.  Every thread returns it. */
template <int NV>
__device__ __forceinline__ double pln_tree_rest(const double* src, uint32_t count, int e, double* A, double* B) {
  __shared__ double res;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* in = src;
  double* out = A;
  __syncthreads(); /* an earlier call's readers are done with res */
  while (count > 1u) {
    const uint32_t groups = (count + 63u) / 64u;
    for (uint32_t g = wave; g < groups; g += PLN_BLOCK / 64) {
      const uint32_t i = g * 64u + (uint32_t)lane;
      const double r = rfn_wave_sum(i < count ? in[(size_t)i * NV + e] : 0.0);
      if (lane == 0) out[(size_t)g * NV + e] = r;
    }
    __syncthreads();
    in = out;
    out = out == A ? B : A;
    count = groups;
  }
  if (threadIdx.x == 0) res = in[e];
  __syncthreads();
  return res;
}

/* NV = 3: the centroid of the inliers.  NV = 6: the covariance, its smallest eigenvector by the Jacobi sweeps of the
 * normals, the refitted plane P1 (invalid unless its four numbers are finite).  grid: K */
template <int NV>
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_finish(const PlnSeg* __restrict__ tab, PlnWork* __restrict__ work, const double* __restrict__ part,
                                                          double* __restrict__ A, double* __restrict__ B) {
  const int s = blockIdx.x;
  PlnWork* w = &work[s];
  if (!w->act) return;
  const PlnSeg sg = tab[s];
  const uint32_t tiles = (w->m + PLN_TILE - 1) / PLN_TILE;
  const size_t slot = ((size_t)(sg.tile0 / 64u) + (size_t)s) * NV; /* disjoint for disjoint runs of tiles */
  const double k = (double)w->k0;
  double v[NV];
  for (int e = 0; e < NV; e++) v[e] = pln_tree_rest<NV>(part + (size_t)sg.tile0 * NV, tiles, e, A + slot, B + slot) / k;
  if (threadIdx.x != 0) return;
  if constexpr (NV == 3) {
    for (int e = 0; e < 3; e++) w->c[e] = v[e];
  } else {
    double P[4], nv[3];
    (void)prep_smallest_eigvec(v, nv);
    double d = -((nv[0] * w->c[0] + nv[1] * w->c[1]) + nv[2] * w->c[2]);
    if (d < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; d = -d; }
    P[0] = nv[0]; P[1] = nv[1]; P[2] = nv[2]; P[3] = d;
    if (!pln_finite4(P)) pln_invalid(P);
    for (int e = 0; e < 4; e++) w->P1[e] = P[e];
  }
}

/* k1 = the refitted plane's inliers in L.  grid: tiles */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_recount(const PlnSeg* __restrict__ tab, int K, PlnWork* __restrict__ work,
                                                           const float4* __restrict__ lp, double thr) {
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  PlnWork* w = &work[s];
  const uint32_t m = w->m, base = (t - sg.tile0) * PLN_TILE;
  if (!w->act || base >= m) return;
  const double P[4] = {w->P1[0], w->P1[1], w->P1[2], w->P1[3]};
  for (uint32_t j0 = base; j0 < min(m, base + PLN_TILE); j0 += PLN_BLOCK) { /* uniform trip count: the ballot sees whole waves */
    const uint32_t j = j0 + threadIdx.x;
    bool in = false;
    if (j < m) {
      const float4 q = lp[sg.off + j];
      in = pln_inlier(pln_s(P, (double)q.x, (double)q.y, (double)q.z), thr);
    }
    pln_wave_count(in, &w->k1);
  }
}

/* the refitted plane is used iff it is finite and counts at least what the hypothesis did.  One thread per segment */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_pln_choose(PlnWork* __restrict__ work, int K, int r, int max_planes,
                                                                ppf_plane_info* __restrict__ info) {
  const int s = threadIdx.x;
  if (s >= K || !work[s].act) return;
  PlnWork* w = &work[s];
  if (!(pln_finite4(w->P1) && w->k1 >= (uint32_t)w->k0)) return;
  ppf_plane_info* ir = &info[(size_t)s * max_planes + r];
  for (int k = 0; k < 4; k++) w->P[k] = w->P1[k];
  for (int k = 0; k < 3; k++) ir->n[k] = w->P1[k];
  ir->d = w->P1[3];
  ir->refit = 1;
  ir->n_inliers = (int32_t)w->k1;
}

/* flags[i] = row i of L stays (0 past m; flags[total] = 0 closes the scan); the rows that leave get their label.
 * grid: tiles */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_flags(const PlnSeg* __restrict__ tab, int K, const PlnWork* __restrict__ work,
                                                         const float4* __restrict__ lp, double thr, int behind, int r, int max_planes,
                                                         uint32_t total, uint32_t* __restrict__ flags, uint8_t* __restrict__ labels,
                                                         ppf_plane_info* __restrict__ info) {
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const PlnWork* w = &work[s];
  const uint32_t m = w->m, base = (t - sg.tile0) * PLN_TILE;
  const bool act = w->act != 0;
  const double P[4] = {w->P[0], w->P[1], w->P[2], w->P[3]};
  if (t == 0 && threadIdx.x == 0) flags[total] = 0u;
  for (uint32_t j0 = base; j0 < min(sg.n, base + PLN_TILE); j0 += PLN_BLOCK) {
    const uint32_t j = j0 + threadIdx.x;
    bool beh = false;
    if (j < sg.n) {
      uint32_t keep = j < m ? 1u : 0u;
      if (act && j < m) {
        const float4 q = lp[sg.off + j];
        const double sv = pln_s(P, (double)q.x, (double)q.y, (double)q.z);
        const bool in = pln_inlier(sv, thr);
        beh = behind && isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && sv < -thr;
        if (in || beh) {
          keep = 0u;
          labels[sg.off + __float_as_uint(q.w)] = (uint8_t)(in ? 1 + r : 0x80 | (1 + r));
        }
      }
      flags[sg.off + j] = keep;
    }
    if (behind && act) pln_wave_count(beh, reinterpret_cast<uint32_t*>(&info[(size_t)s * max_planes + r].n_behind));
  }
}

/* the rows that stay move up, in order; m = their number.  pos = the exclusive scan of flags.  grid: tiles */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_compact(const PlnSeg* __restrict__ tab, int K, PlnWork* __restrict__ work,
                                                           const float4* __restrict__ lp, const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ pos, float4* __restrict__ lp_out) {
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const uint32_t base = (t - sg.tile0) * PLN_TILE, p0 = pos[sg.off];
  if (base == 0 && threadIdx.x == 0) work[s].m = pos[sg.off + sg.n] - p0;
  for (uint32_t j = base + threadIdx.x; j < min(sg.n, base + PLN_TILE); j += PLN_BLOCK)
    if (flags[sg.off + j]) lp_out[sg.off + (pos[sg.off + j] - p0)] = lp[sg.off + j];
}

/* out = the rows of L, whole: six floats and the curvature of each, at the cloud's place in the output block.
 * grid: tiles */
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_gather(const PlnSeg* __restrict__ tab, int K, const PlnWork* __restrict__ work,
                                                          const float4* __restrict__ lp, float* __restrict__ out_rows, float* __restrict__ out_curv) {
  const uint32_t t = blockIdx.x;
  const int s = pln_seg_of(tab, K, t);
  const PlnSeg sg = tab[s];
  const uint32_t base = (t - sg.tile0) * PLN_TILE;
  for (uint32_t j = base + threadIdx.x; j < min(work[s].m, base + PLN_TILE); j += PLN_BLOCK) {
    const uint32_t i = __float_as_uint(lp[sg.off + j].w);
    const float* p = sg.rows + (size_t)i * 6;
    float* o = out_rows + (size_t)(sg.off + j) * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = p[k];
    out_curv[sg.off + j] = sg.curv[i];
  }
}

/* ppf_prep_planes_apply: flags[i] = row i is neither an inlier of one of the planes nor (behind != 0) behind one;
 * flags[n] = 0 */
struct PlnPlanes {
  double P[PPF_PLANE_MAX_PLANES][4];
  int n;
};
__global__ __launch_bounds__(PLN_BLOCK) void k_pln_apply_flags(const float* __restrict__ rows, int n, PlnPlanes pl, double thr, int behind,
                                                               uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { flags[n] = 0u; return; }
  const float* p = rows + (size_t)i * 6;
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  bool keep = true;
  for (int k = 0; k < pl.n; k++) {
    const double sv = pln_s(pl.P[k], x, y, z);
    if (pln_inlier(sv, thr) || (behind && prep_finite3(p) && sv < -thr)) keep = false;
  }
  flags[i] = keep ? 1u : 0u;
}

#endif /* PPF_PLANE_KERNELS_H */
