/*
 * ppf_prep_kernels.h — the stages that produce the matcher's N x 6 input, on gfx950 (SURVEY.md §8f row N4;
 * /root/reference/include/CloudProcessing.h: SceneCropping :263-339, Subsampling :361-380, OutlierProcessing :341-360,
 * NormalEstimation :381-405, EdgeExtraction :406-427, PointCloudXYZNormalToMat :163-190).  Included by ppf_hip.hip.
 *
 * The arithmetic and every order-dependent choice is the one oracle/ppf_prep_oracle.cpp freezes; results are
 * bit-identical to it.  Clouds are device rows `x y z nx ny nz` (pitch 6) plus a curvature array.  There is one kernel
 * family: every stage works on K <= 256 segments of one concatenated cloud (ppf_prep_frame), and a single cloud
 * (ppf_prep_crop ... ppf_prep_to_mat) is the case K = 1.  The device bodies come first, the kernels after them.
 *   crop / outlier / edge : per-point predicate -> flags -> exclusive scan -> ordered gather (HBM streaming, 28 B/pt)
 *   voxel grid            : finite min/max -> PCL's cell index -> stable LSD radix sort (passes shared with the
 *                           sampler) -> one thread per cell, float sums in point order
 *   k nearest neighbours  : uniform grid (counting sort into cell order), ONE WAVE per query, cube of cells
 *                           grown until the k-th distance is provably final; the k <= 64 best (distance bits, index)
 *                           keys live one per lane and 64 candidates at a time are merged in by a register bitonic
 *                           network.  Exact: equals the oracle's exhaustive search bit for bit.
 *   normals               : one thread per point, fp64 two-pass covariance over its neighbour list, cyclic Jacobi in
 *                           registers (12 sweeps, + - * / sqrt only), smallest eigenvector, flip towards the origin.
 */
#ifndef PPF_PREP_KERNELS_H
#define PPF_PREP_KERNELS_H

constexpr int KNN_WAVES = 4;  /* queries (waves) per workgroup */
constexpr int KNN_MAX_K = 64; /* the k best keys live one per lane */

struct CropPlanes {
  double n[4][3]; /* inward normals of the four side planes through the origin */
  float z_base;
};

__device__ __forceinline__ bool prep_finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* point inside the pyramid {origin, 4 corners} */
__device__ __forceinline__ bool prep_crop_inside(const float* p, const CropPlanes& pl) {
  bool in = prep_finite3(p) && p[2] <= pl.z_base;
#pragma unroll
  for (int f = 0; f < 4; f++) in = in && (pl.n[f][0] * (double)p[0] + pl.n[f][1] * (double)p[1] + pl.n[f][2] * (double)p[2]) >= 0.0;
  return in;
}

/* rows of `cols` floats at `stride` -> packed rows of 6 (+ zero curvature) */
__global__ __launch_bounds__(256) void k_prep_pack(const float* __restrict__ src, int n, int stride, int noff, int cols, float* __restrict__ rows,
                                                   float* __restrict__ curv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    rows[(size_t)i * 6 + k] = src[(size_t)i * stride + k];
    rows[(size_t)i * 6 + 3 + k] = cols == 6 ? src[(size_t)i * stride + noff + k] : 0.f;
  }
  curv[i] = 0.f;
}

/* ---- voxel grid ------------------------------------------------------------------------------------------- */
struct VoxelGridDims {
  float inv_leaf;
  int min_b[3], div_b[3];
};
/* PCL: ijk = (int)(floor(p * inv_leaf) - (float)min_b); idx = i + j*div0 + k*div0*div1 */
__device__ __forceinline__ uint32_t prep_voxel_key(const float* p, const VoxelGridDims& g) {
  const int i0 = ppf_f2i(floorf(p[0] * g.inv_leaf) - (float)g.min_b[0]);
  const int i1 = ppf_f2i(floorf(p[1] * g.inv_leaf) - (float)g.min_b[1]);
  const int i2 = ppf_f2i(floorf(p[2] * g.inv_leaf) - (float)g.min_b[2]);
  return (uint32_t)(i0 + i1 * g.div_b[0] + i2 * g.div_b[0] * g.div_b[1]);
}
/* one thread per occupied cell: float sums in ascending point order, divided by the float count */
__global__ __launch_bounds__(64) void k_prep_voxel_sum(const float* __restrict__ rows, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ starts, int n_cells, int n, float* __restrict__ out_rows,
                                                       float* __restrict__ out_curv) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_cells) return;
  const uint32_t s = starts[r], e = (r + 1 < n_cells) ? starts[r + 1] : (uint32_t)n;
  float acc[3] = {0.f, 0.f, 0.f};
  for (uint32_t k = s; k < e; k++) {
    const float* p = rows + (size_t)vals[k] * 6;
    acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
  }
  const float cnt = (float)(e - s);
  out_rows[(size_t)r * 6] = acc[0] / cnt; out_rows[(size_t)r * 6 + 1] = acc[1] / cnt; out_rows[(size_t)r * 6 + 2] = acc[2] / cnt;
  out_rows[(size_t)r * 6 + 3] = 0.f; out_rows[(size_t)r * 6 + 4] = 0.f; out_rows[(size_t)r * 6 + 5] = 0.f;
  out_curv[r] = 0.f;
}

/* ---- exact k nearest neighbours ----------------------------------------------------------------------------- */
/* Uniform grid over the cloud's bounding box; points sorted by cell (x fastest).  A query scans the cube of cells of
 * radius r around its own cell and keeps its k best keys (float d2 bits << 32 | original index: d2 >= +0, so the
 * u64 order IS (distance, index) order, independent of the scan order).  Every point
 * outside that cube is farther than r*h, so the list is final once its k-th distance is within (0.9999 r h)^2 (the
 * margin covers the float rounding of the cell assignment); otherwise the cube grows.  When the cube covers the whole
 * grid the search has been exhaustive.  Results equal the oracle's brute force bit for bit. */
struct KnnGrid {
  float lo[3];
  float inv_h, h;
  int dim[3];
};
__device__ __forceinline__ void knn_cell(const KnnGrid& g, float x, float y, float z, int* c) {
  c[0] = min(max(ppf_f2i(floorf((x - g.lo[0]) * g.inv_h)), 0), g.dim[0] - 1);
  c[1] = min(max(ppf_f2i(floorf((y - g.lo[1]) * g.inv_h)), 0), g.dim[1] - 1);
  c[2] = min(max(ppf_f2i(floorf((z - g.lo[2]) * g.inv_h)), 0), g.dim[2] - 1);
}
/* bitonic compare-exchange across lanes */
__device__ __forceinline__ unsigned long long knn_cex(unsigned long long key, int stride, bool take_min) {
  const unsigned long long other = __shfl_xor(key, stride);
  return take_min ? (key < other ? key : other) : (key < other ? other : key);
}
/* ONE WAVE PER QUERY: its k <= 64 nearest points, ascending (d2, index).
 * The wave reads 64 candidates per step (coalesced within a row of cells); its current k best keys live one per
 * lane, ascending by lane (lanes >= k hold the sentinel).  A step whose candidates all fail the k-th key costs one
 * ballot; otherwise the 64 new keys are bitonic-sorted across the lanes (21 exchanges) and merged with the list
 * (reverse + min = the 64 smallest of both as a bitonic sequence, 6 more exchanges).  No LDS. */
__device__ __forceinline__ unsigned long long prep_knn_search(const float4* __restrict__ pts, const uint32_t* __restrict__ cell_begin,
                                                                const KnnGrid& g, const float4 p, const int k, const int lane) {
  int c[3];
  knn_cell(g, p.x, p.y, p.z, c);
  const unsigned long long none = ~0ull;
  unsigned long long best;
  for (int r = 1;; r++) {
    best = none;
    unsigned long long worst = none; /* the k-th key, wave-uniform */
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.dim[0] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.dim[1] - 1);
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.dim[2] - 1);
    for (int cz = z0; cz <= z1; cz++)
      for (int cy = y0; cy <= y1; cy++) {
        const int base = (cz * g.dim[1] + cy) * g.dim[0];
        const uint32_t jb = cell_begin[base + x0], je = cell_begin[base + x1 + 1];
        for (uint32_t j0 = jb; j0 < je; j0 += 64) {
          const uint32_t j = j0 + (uint32_t)lane;
          unsigned long long key = none;
          if (j < je) {
            const float4 q = pts[j];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d >= 0.f) key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(q.w); /* drops NaN */
          }
          if (!__any(key < worst)) continue;
          /* sort the 64 new keys ascending by lane */
#pragma unroll
          for (int size = 2; size <= 64; size <<= 1) {
            const bool up = (lane & size) == 0 || size == 64;
#pragma unroll
            for (int stride = size >> 1; stride > 0; stride >>= 1) key = knn_cex(key, stride, ((lane & stride) == 0) == up);
          }
          /* the 64 smallest of (best, key): best ascending, key reversed -> elementwise min is bitonic */
          const unsigned long long rev = __shfl(key, 63 - lane);
          best = best < rev ? best : rev;
#pragma unroll
          for (int stride = 32; stride > 0; stride >>= 1) best = knn_cex(best, stride, (lane & stride) == 0);
          if (lane >= k) best = none;
          worst = __shfl(best, k - 1);
        }
      }
    const bool whole = x0 == 0 && y0 == 0 && z0 == 0 && x1 == g.dim[0] - 1 && y1 == g.dim[1] - 1 && z1 == g.dim[2] - 1;
    const float lim = (float)r * g.h * 0.9999f;
    if (whole || (worst != none && __uint_as_float((uint32_t)(worst >> 32)) <= lim * lim)) break;
  }
  return best; /* lane m holds the m-th best key (m < k), or ~0 */
}

/* ---- statistical outlier removal ---------------------------------------------------------------------------- */
/* dist[i] = (float)(sum_{m=1..mean_k} sqrtf(d2[i][m]) / mean_k), fp64 sum in neighbour order; 0 when n <= mean_k */
__device__ __forceinline__ float prep_sor_mean_dist(const float* __restrict__ d2_row, int mean_k) {
  double s = 0;
  for (int m = 1; m <= mean_k; m++) s += (double)sqrtf(d2_row[m]);
  return (float)(s / (double)mean_k);
}
/* per-chunk (64 points) sums of d and d*d in fp64 */
__device__ __forceinline__ void prep_sor_chunk(const float* __restrict__ dist, int b, int e, double* __restrict__ part) {
  double ps = 0, pq = 0;
  for (int i = b; i < e; i++) { const double v = (double)dist[i]; ps += v; pq += v * v; }
  part[0] = ps; part[1] = pq;
}
/* out[0] = mean + mul * stddev */
__device__ __forceinline__ double prep_sor_thr(double sum, double sq, int n, double std_mul) {
  const double mean = sum / (double)n;
  const double variance = (sq - sum * sum / (double)n) / ((double)n - 1);
  return mean + std_mul * ppf_sqrt(variance);
}

/* ---- normals + curvature ------------------------------------------------------------------------------------ */
__device__ __forceinline__ void prep_jacobi_rotate(double (&A)[3][3], double (&V)[3][3], const int p, const int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double at = theta < 0 ? -theta : theta;
  double t = 1.0 / (at + ppf_sqrt(theta * theta + 1.0));
  if (theta < 0) t = -t;
  const double c = 1.0 / ppf_sqrt(t * t + 1.0), s = t * c;
  const double app = A[p][p], aqq = A[q][q];
  A[p][p] = app - t * apq;
  A[q][q] = aqq + t * apq;
  A[p][q] = 0.0; A[q][p] = 0.0;
  const int r = 3 - p - q;
  const double arp = A[r][p], arq = A[r][q];
  A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
  A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

/* 12 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) of the symmetric matrix {xx, xy, xz, yy, yz, zz}: nv = the column of the
 * smallest diagonal entry (strict <, in the order 0, 1, 2) divided by its length; returns that entry.  Shared by the
 * normals (prep_normal_point) and the plane refit (ppf_plane_kernels.h) */
__device__ __forceinline__ double prep_smallest_eigvec(const double (&cov)[6], double (&nv)[3]) {
  double A[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; sweep++) {
    prep_jacobi_rotate(A, V, 0, 1);
    prep_jacobi_rotate(A, V, 0, 2);
    prep_jacobi_rotate(A, V, 1, 2);
  }
  double lam = A[0][0];
  nv[0] = V[0][0]; nv[1] = V[1][0]; nv[2] = V[2][0];
  if (A[1][1] < lam) { lam = A[1][1]; nv[0] = V[0][1]; nv[1] = V[1][1]; nv[2] = V[2][1]; }
  if (A[2][2] < lam) { lam = A[2][2]; nv[0] = V[0][2]; nv[1] = V[1][2]; nv[2] = V[2][2]; }
  const double len = ppf_sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
  nv[0] /= len; nv[1] /= len; nv[2] /= len;
  return lam;
}

/* in place: o[3..5] = normal, *curv = curvature of the point o from its k neighbours nb (indices into q4) */
__device__ __forceinline__ void prep_normal_point(float* __restrict__ o, float* __restrict__ curv_out, const int* __restrict__ nb, int k,
                                                  const float4* __restrict__ q4) {
  if (k < 3) {
    const float qn = __builtin_nanf("");
    o[3] = o[4] = o[5] = qn; *curv_out = qn;
    return;
  }
  double c[3] = {0, 0, 0};
  for (int m = 0; m < k; m++) { const float4 q = q4[nb[m]]; c[0] += (double)q.x; c[1] += (double)q.y; c[2] += (double)q.z; }
  c[0] /= (double)k; c[1] /= (double)k; c[2] /= (double)k;
  double cov[6] = {0, 0, 0, 0, 0, 0};
  for (int m = 0; m < k; m++) {
    const float4 q = q4[nb[m]];
    const double d0 = (double)q.x - c[0], d1 = (double)q.y - c[1], d2 = (double)q.z - c[2];
    cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2;
    cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
  }
#pragma unroll
  for (int a = 0; a < 6; a++) cov[a] /= (double)k;
  const double trace = cov[0] + cov[3] + cov[5];
  double nv[3];
  double lam = prep_smallest_eigvec(cov, nv);
  const double cos_theta = -((double)o[0] * nv[0] + (double)o[1] * nv[1] + (double)o[2] * nv[2]);
  if (cos_theta < 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  o[3] = (float)nv[0]; o[4] = (float)nv[1]; o[5] = (float)nv[2];
  if (lam < 0) lam = -lam;
  const double at = trace < 0 ? -trace : trace;
  *curv_out = trace != 0.0 ? (float)(lam / at) : 0.f;
}
/* PointCloudXYZNormalToMat: n /= (float)sqrtf(n.n) when that length exceeds 1e-5 */
__device__ __forceinline__ void prep_to_mat_row(const float* __restrict__ row, float* __restrict__ out) {
  float d[6];
#pragma unroll
  for (int k = 0; k < 6; k++) d[k] = row[k];
  const float s = d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
  const double A = (double)sqrtf(s);
  if (A > 0.00001) { d[3] /= (float)A; d[4] /= (float)A; d[5] /= (float)A; }
#pragma unroll
  for (int k = 0; k < 6; k++) out[k] = d[k];
}

/* ============================================================================================================ */
/* The stage kernels: K segments at once (host side: ppf_prep_host.h; ppf_prep_frame: ppf_frame_host.h)           */
/* ============================================================================================================ */
/* A stage's input is the concatenation of K <= FRAME_MAX_BOXES segments, one per box, described by a device table
 * {off, n} (segments are contiguous and in box order).  Counts never leave the device: grids are sized for a worst
 * case the host knows and threads past the segment table's total exit.  Every floating-point reduction runs over a
 * segment's own rows in their order, counted from the segment's start, so a segment's result depends neither on K
 * nor on its neighbours: it is what the stage gives for that segment alone (K = 1, the per-cloud entries).  The
 * small per-segment kernels run one workgroup of FRAME_MAX_BOXES threads. */
constexpr int FRAME_MAX_BOXES = 256;
struct FrameSeg {
  uint32_t off, n;
};

/* the largest s < K with a[s * stride] <= v (a nondecreasing, a[0] = 0): the segment holding element v */
__device__ __forceinline__ int frame_find(const uint32_t* __restrict__ a, int stride, int K, uint32_t v) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a[(size_t)mid * stride] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int frame_seg_of(const FrameSeg* __restrict__ seg, int K, uint32_t i) {
  return frame_find(&seg[0].off, 2, K, i);
}
__device__ __forceinline__ uint32_t frame_total(const FrameSeg* __restrict__ seg, int K) { return seg[K - 1].off + seg[K - 1].n; }
/* exclusive scan of one value per thread over a FRAME_MAX_BOXES-thread workgroup; *total = the sum */
__device__ __forceinline__ uint32_t frame_block_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t sh[FRAME_MAX_BOXES];
  const int t = threadIdx.x;
  __syncthreads(); /* an earlier call's readers are done with sh */
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < FRAME_MAX_BOXES; o <<= 1) {
    const uint32_t y = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += y;
    __syncthreads();
  }
  *total = sh[FRAME_MAX_BOXES - 1];
  return sh[t] - v;
}

__global__ __launch_bounds__(256) void k_frame_fill_u32(uint32_t* __restrict__ p, size_t n, uint32_t v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ __launch_bounds__(256) void k_frame_gather_u32(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx, int n,
                                                          uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}

/* ---- crop: flags[b][i] = point i inside box b's pyramid (grid.y = box); flags[K*n] = 0 closes the scan ---- */
__global__ __launch_bounds__(256) void k_frame_crop_flags(const float* __restrict__ rows, int n, int K, const CropPlanes* __restrict__ pl,
                                                          uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (b == 0 && i == 0) flags[(size_t)K * n] = 0u;
  if (i >= n) return;
  flags[(size_t)b * n + i] = prep_crop_inside(rows + (size_t)i * 6, pl[b]) ? 1u : 0u;
}
/* box-major ordered gather; the first workgroup of each box writes its segment */
__global__ __launch_bounds__(256) void k_frame_crop_gather(const float* __restrict__ rows, const float* __restrict__ curv, int n,
                                                           const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                           float* __restrict__ out_rows, float* __restrict__ out_curv, FrameSeg* __restrict__ seg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  const size_t fb = (size_t)b * n;
  if (i == 0) seg[b] = FrameSeg{pos[fb], pos[fb + n] - pos[fb]};
  if (i >= n || !flags[fb + i]) return;
  const uint32_t o = pos[fb + i];
#pragma unroll
  for (int k = 0; k < 6; k++) out_rows[(size_t)o * 6 + k] = rows[(size_t)i * 6 + k];
  out_curv[o] = curv[i];
}

/* ---- per-segment bounds of the finite points: mm[s][0..2] = ~min, [3..5] = max (order-preserving words; the minimum
 * is stored complemented, so that 0 is the identity of all seven words), fin[s] = count.  gridDim.y workgroups share a
 * segment: one stores its result, several combine theirs with integer atomicMax / atomicAdd on words the host has
 * zeroed (order-independent, so the result does not depend on gridDim.y) ---- */
__global__ __launch_bounds__(256) void k_frame_bounds(const float* __restrict__ rows, const FrameSeg* __restrict__ seg,
                                                      uint32_t* __restrict__ mm, uint32_t* __restrict__ fin) {
  const int s = blockIdx.x;
  const FrameSeg sg = seg[s];
  uint32_t nlo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, cnt = 0;
  for (uint32_t i = sg.off + blockIdx.y * blockDim.x + threadIdx.x; i < sg.off + sg.n; i += blockDim.x * gridDim.y) {
    const float* p = rows + (size_t)i * 6;
    if (!prep_finite3(p)) continue;
    cnt++;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t o = float_to_ordered(p[k]);
      nlo[k] = max(nlo[k], ~o);
      hi[k] = max(hi[k], o);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      nlo[k] = max(nlo[k], (uint32_t)__shfl_down(nlo[k], o));
      hi[k] = max(hi[k], (uint32_t)__shfl_down(hi[k], o));
    }
    cnt += (uint32_t)__shfl_down(cnt, o);
  }
  __shared__ uint32_t s_mm[4][7];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) { s_mm[wave][k] = nlo[k]; s_mm[wave][3 + k] = hi[k]; }
    s_mm[wave][6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    uint32_t v = s_mm[0][k];
    for (int w = 1; w < 4; w++) v = k < 6 ? max(v, s_mm[w][k]) : v + s_mm[w][k];
    uint32_t* dst = k < 6 ? &mm[(size_t)s * 6 + k] : &fin[s];
    if (gridDim.y == 1) *dst = v;
    else if (k < 6) atomicMax(dst, v);
    else atomicAdd(dst, v);
  }
}

/* ---- voxel grid ---- */
/* per segment: PCL's min_b / div_b from the bounds of its finite points; *err = the first box whose cell index would
 * overflow (~0 = none) */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_frame_voxel_dims(const uint32_t* __restrict__ mm, const uint32_t* __restrict__ fin, int K,
                                                                      float inv_leaf, VoxelGridDims* __restrict__ dims, uint32_t* __restrict__ err) {
  __shared__ uint32_t e;
  const int s = threadIdx.x;
  if (s == 0) e = 0xFFFFFFFFu;
  __syncthreads();
  if (s < K) {
    VoxelGridDims g;
    g.inv_leaf = inv_leaf;
    for (int k = 0; k < 3; k++) { g.min_b[k] = 0; g.div_b[k] = 0; }
    if (fin[s]) {
      long long cells = 1;
      for (int k = 0; k < 3; k++) {
        const float lo = ordered_to_float(~mm[(size_t)s * 6 + k]), hi = ordered_to_float(mm[(size_t)s * 6 + 3 + k]);
        g.min_b[k] = ppf_f2i(floorf(lo * inv_leaf));
        const int max_b = ppf_f2i(floorf(hi * inv_leaf));
        g.div_b[k] = max_b - g.min_b[k] + 1;
        cells *= g.div_b[k];
        if (cells > 0x7fffffffLL) { atomicMin(&e, (uint32_t)s); break; }
      }
    }
    dims[s] = g;
  }
  __syncthreads();
  if (s == 0) *err = e;
}
/* local PCL cell index per point (non-finite points: key ~0 and segment 255, so the two sorts put them last) */
__global__ __launch_bounds__(256) void k_frame_voxel_keys(const float* __restrict__ rows, int n, const FrameSeg* __restrict__ seg, int K,
                                                          const VoxelGridDims* __restrict__ dims, uint32_t* __restrict__ lkey,
                                                          uint32_t* __restrict__ lkey_keep, uint32_t* __restrict__ skey, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = rows + (size_t)i * 6;
  const int s = frame_seg_of(seg, K, (uint32_t)i);
  const bool ok = prep_finite3(p);
  const uint32_t k = ok ? prep_voxel_key(p, dims[s]) : 0xFFFFFFFFu;
  lkey[i] = k;
  lkey_keep[i] = k;
  skey[i] = ok ? (uint32_t)s : 255u;
  vals[i] = (uint32_t)i;
}
/* a run of equal (segment, cell) starts at sorted position j; flags[n] = 0 */
__global__ __launch_bounds__(256) void k_frame_voxel_runs(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ lkey,
                                                          const uint32_t* __restrict__ skey, int n, uint32_t* __restrict__ flags) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  if (j == n) { flags[n] = 0u; return; }
  const uint32_t v = vals[j], key = lkey[v];
  bool start = key != 0xFFFFFFFFu;
  if (start && j > 0) {
    const uint32_t u = vals[j - 1];
    start = key != lkey[u] || skey[v] != skey[u];
  }
  flags[j] = start ? 1u : 0u;
}
/* seg_v[s] = segment s's cells (runs); out = {cells in all, finite points in all, overflow box, cells per box[K]} */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_frame_voxel_table(const uint32_t* __restrict__ fin, int K, const uint32_t* __restrict__ runid,
                                                                       const uint32_t* __restrict__ err, FrameSeg* __restrict__ seg_v,
                                                                       uint32_t* __restrict__ out) {
  const int s = threadIdx.x;
  const uint32_t f = s < K ? fin[s] : 0u;
  uint32_t total;
  const uint32_t first = frame_block_scan(f, &total); /* the sorted finite points are segment-major */
  if (s < K) {
    const uint32_t a = runid[first], b = runid[first + f];
    seg_v[s] = FrameSeg{a, b - a};
    out[3 + s] = b - a;
  }
  if (s == 0) { out[0] = runid[total]; out[1] = total; out[2] = *err; }
}

/* ---- neighbour search: one uniform grid per segment, cells of all grids in one array ---- */
/* per segment: its grid, about sqrt(n) / gdiv cells along the longest side of the bounding box (a 3x3x3 cube of a
 * surface-like cloud then holds a few hundred points), at most 128; k_eff (mode 0: SOR, n > k ? k + 1 : 0; mode 1:
 * normals, min(k, n); 0 = not searched, also for a segment that holds a non-finite row: fin[s] != n); the base of its
 * cells and of its 64-point SOR chunks */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_frame_knn_grids(const uint32_t* __restrict__ mm, const uint32_t* __restrict__ fin,
                                                                     const FrameSeg* __restrict__ seg, int K, int mode, int k, double gdiv,
                                                                     KnnGrid* __restrict__ grids, uint32_t* __restrict__ cell_base,
                                                                     int* __restrict__ keff, uint32_t* __restrict__ chunk_base) {
  const int s = threadIdx.x;
  uint32_t cells = 0, chunks = 0;
  if (s < K) {
    const int n = (int)seg[s].n;
    const int ke = fin[s] != (uint32_t)n ? 0 : mode == 0 ? (n > k ? k + 1 : 0) : min(k, n);
    KnnGrid g;
    float ext_max = 0.f;
    for (int a = 0; a < 3; a++) {
      g.lo[a] = ordered_to_float(~mm[(size_t)s * 6 + a]);
      ext_max = fmaxf(ext_max, ordered_to_float(mm[(size_t)s * 6 + 3 + a]) - g.lo[a]);
    }
    const int G = max(1, min(128, (int)(sqrt((double)n) / gdiv)));
    g.h = ext_max > 0.f ? ext_max / (float)G : 1.0f;
    g.inv_h = 1.0f / g.h;
    cells = 1;
    for (int a = 0; a < 3; a++) {
      const float hi = ordered_to_float(mm[(size_t)s * 6 + 3 + a]);
      g.dim[a] = max(1, min(G + 1, (int)floorf((hi - g.lo[a]) * g.inv_h) + 1));
      cells *= (uint32_t)g.dim[a];
    }
    if (ke == 0) cells = 0;
    chunks = ((uint32_t)n + 63) / 64;
    grids[s] = g;
    keff[s] = ke;
  }
  uint32_t tc, tk;
  const uint32_t cb = frame_block_scan(cells, &tc);
  const uint32_t kb = frame_block_scan(chunks, &tk);
  if (s < K) { cell_base[s] = cb; chunk_base[s] = kb; }
  if (s == 0) { cell_base[K] = tc; chunk_base[K] = tk; }
}
__global__ __launch_bounds__(256) void k_frame_knn_keys(const float* __restrict__ rows, int cap, const FrameSeg* __restrict__ seg, int K,
                                                        const KnnGrid* __restrict__ grids, const uint32_t* __restrict__ cell_base,
                                                        const int* __restrict__ keff, uint32_t* __restrict__ keys, uint32_t* __restrict__ cell_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || (uint32_t)i >= frame_total(seg, K)) return;
  const int s = frame_seg_of(seg, K, (uint32_t)i);
  if (keff[s] == 0) { keys[i] = 0xFFFFFFFFu; return; }
  const KnnGrid g = grids[s];
  int c[3];
  knn_cell(g, rows[(size_t)i * 6], rows[(size_t)i * 6 + 1], rows[(size_t)i * 6 + 2], c);
  const uint32_t key = cell_base[s] + (uint32_t)((c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0]);
  keys[i] = key;
  atomicAdd(&cell_count[key], 1u);
}
/* counting-sort scatter into cell order (the order inside a cell is free: the search's result does not depend on it);
 * pts.w = the point's index in the concatenation.  q4 = xyz by row. */
__global__ __launch_bounds__(256) void k_frame_knn_scatter(const float* __restrict__ rows, int cap, const FrameSeg* __restrict__ seg, int K,
                                                           const uint32_t* __restrict__ keys, const uint32_t* __restrict__ cell_begin,
                                                           uint32_t* __restrict__ cell_count, float4* __restrict__ pts, float4* __restrict__ q4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || (uint32_t)i >= frame_total(seg, K)) return;
  const float x = rows[(size_t)i * 6], y = rows[(size_t)i * 6 + 1], z = rows[(size_t)i * 6 + 2];
  q4[i] = make_float4(x, y, z, 0.f);
  const uint32_t key = keys[i];
  if (key == 0xFFFFFFFFu) return;
  const uint32_t slot = cell_begin[key] + atomicSub(&cell_count[key], 1u) - 1u;
  pts[slot] = make_float4(x, y, z, __uint_as_float((uint32_t)i));
}
/* ONE WAVE PER POINT in cell order, prep_knn_search on the point's own segment grid; idx (segment-local indices) /
 * d2 are [row][kstride] at the point's row, with the segment's k_eff entries */
__global__ __launch_bounds__(256) void k_frame_knn(const float4* __restrict__ pts, const uint32_t* __restrict__ cell_begin,
                                                   const KnnGrid* __restrict__ grids, const uint32_t* __restrict__ cell_base,
                                                   const FrameSeg* __restrict__ seg, int K, const int* __restrict__ keff, int cap, int kstride,
                                                   int* __restrict__ idx_out, float* __restrict__ d2_out) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); /* wave-uniform */
  if (w >= cap || (uint32_t)w >= cell_begin[cell_base[K]]) return;
  const float4 p = pts[w];
  const uint32_t gi = __float_as_uint(p.w);
  const int s = frame_seg_of(seg, K, gi);
  const int k = keff[s];
  const KnnGrid g = grids[s];
  const unsigned long long best = prep_knn_search(pts, cell_begin + cell_base[s], g, p, k, lane), none = ~0ull;
  if (lane < k) {
    const size_t row = (size_t)gi * kstride;
    idx_out[row + lane] = best == none ? -1 : (int)((uint32_t)best - seg[s].off);
    d2_out[row + lane] = best == none ? 0.f : __uint_as_float((uint32_t)(best >> 32));
  }
}

/* ---- statistical outlier removal: per-segment mean distance, 64-point chunks from each segment's start, one
 * threshold per segment ---- */
__global__ __launch_bounds__(256) void k_frame_sor_dist(const float* __restrict__ d2, int cap, const FrameSeg* __restrict__ seg, int K,
                                                        const int* __restrict__ keff, int mean_k, float* __restrict__ dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || (uint32_t)i >= frame_total(seg, K)) return;
  const int s = frame_seg_of(seg, K, (uint32_t)i);
  dist[i] = keff[s] ? prep_sor_mean_dist(d2 + (size_t)i * (mean_k + 1), mean_k) : 0.f; /* a segment that was not searched has no lists */
}
__global__ __launch_bounds__(64) void k_frame_sor_chunks(const float* __restrict__ dist, int cap_chunks, const FrameSeg* __restrict__ seg, int K,
                                                         const uint32_t* __restrict__ chunk_base, double* __restrict__ parts) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cap_chunks || (uint32_t)c >= chunk_base[K]) return;
  const int s = frame_find(chunk_base, 1, K, (uint32_t)c);
  const FrameSeg sg = seg[s];
  const uint32_t c0 = sg.off + ((uint32_t)c - chunk_base[s]) * 64u;
  prep_sor_chunk(dist, (int)c0, (int)min(sg.off + sg.n, c0 + 64u), parts + (size_t)c * 2);
}
/* one workgroup per segment */
__global__ __launch_bounds__(64) void k_frame_sor_threshold(const double* __restrict__ parts, const FrameSeg* __restrict__ seg,
                                                            const uint32_t* __restrict__ chunk_base, double std_mul, double* __restrict__ thr) {
  __shared__ double tot[2];
  const int s = blockIdx.x;
  const int n = (int)seg[s].n;
  if (n == 0) return;
  if (threadIdx.x < 2) tot[threadIdx.x] = icp_sum_parts(parts + (size_t)chunk_base[s] * 2 + threadIdx.x, (n + 63) / 64, 2);
  __syncthreads();
  if (threadIdx.x == 0) thr[s] = prep_sor_thr(tot[0], tot[1], n, std_mul);
}
/* flags[i] for i <= cap (0 past the total: the scan over cap + 1 entries then counts the kept rows) */
__global__ __launch_bounds__(256) void k_frame_sor_flags(const float* __restrict__ dist, int cap, const FrameSeg* __restrict__ seg, int K,
                                                         const double* __restrict__ thr, uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > cap) return;
  if ((uint32_t)i >= frame_total(seg, K)) { flags[i] = 0u; return; }
  flags[i] = !((double)dist[i] > thr[frame_seg_of(seg, K, (uint32_t)i)]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_frame_curv_flags(const float* __restrict__ curv, int cap, const FrameSeg* __restrict__ seg, int K,
                                                          float thr, uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > cap) return;
  flags[i] = (uint32_t)i < frame_total(seg, K) && curv[i] > thr ? 1u : 0u;
}
/* segmented compaction: ordered gather of the flagged rows (pos = exclusive scan of flags[0..cap]) and the segment
 * table of the result */
__global__ __launch_bounds__(256) void k_frame_gather(const float* __restrict__ rows, const float* __restrict__ curv, int cap,
                                                      const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                      const FrameSeg* __restrict__ seg_in, int K, float* __restrict__ out_rows,
                                                      float* __restrict__ out_curv, FrameSeg* __restrict__ seg_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && (int)threadIdx.x < K) {
    const FrameSeg sg = seg_in[threadIdx.x];
    seg_out[threadIdx.x] = FrameSeg{pos[sg.off], pos[sg.off + sg.n] - pos[sg.off]};
  }
  if (i >= cap || !flags[i]) return;
  const uint32_t o = pos[i];
#pragma unroll
  for (int k = 0; k < 6; k++) out_rows[(size_t)o * 6 + k] = rows[(size_t)i * 6 + k];
  out_curv[o] = curv[i];
}

/* ---- normals, to-Mat, the report ---- */
__global__ __launch_bounds__(64) void k_frame_normals(const float* __restrict__ rows, int cap, const FrameSeg* __restrict__ seg, int K,
                                                      const int* __restrict__ idx, int kstride, const int* __restrict__ keff,
                                                      const float4* __restrict__ q4, float* __restrict__ out_rows, float* __restrict__ out_curv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || (uint32_t)i >= frame_total(seg, K)) return;
  const int s = frame_seg_of(seg, K, (uint32_t)i);
  float* o = out_rows + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; k++) o[k] = rows[(size_t)i * 6 + k];
  prep_normal_point(o, out_curv + i, idx + (size_t)i * kstride, keff[s], q4 + seg[s].off);
}
__global__ __launch_bounds__(256) void k_frame_to_mat(const float* __restrict__ rows, const float* __restrict__ curv, int cap,
                                                      const FrameSeg* __restrict__ seg, int K, float* __restrict__ out_rows,
                                                      float* __restrict__ out_curv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap || (uint32_t)i >= frame_total(seg, K)) return;
  prep_to_mat_row(rows + (size_t)i * 6, out_rows + (size_t)i * 6);
  out_curv[i] = curv[i];
}
/* rep[s] = {rows after crop, voxel grid, outlier removal, edge extraction, object offset, edge offset} */
__global__ __launch_bounds__(FRAME_MAX_BOXES) void k_frame_report(const FrameSeg* __restrict__ seg_c, const FrameSeg* __restrict__ seg_v,
                                                                  const FrameSeg* __restrict__ seg_o, const FrameSeg* __restrict__ seg_e, int K,
                                                                  uint32_t* __restrict__ rep) {
  const int s = threadIdx.x;
  if (s >= K) return;
  uint32_t* r = rep + (size_t)s * 6;
  r[0] = seg_c[s].n; r[1] = seg_v[s].n; r[2] = seg_o[s].n; r[3] = seg_e[s].n; r[4] = seg_o[s].off; r[5] = seg_e[s].off;
}

#endif /* PPF_PREP_KERNELS_H */
