/*
 * ppf_verify_kernels.h — pose verification on gfx950 (ppf_verify_frame): how well every refined pose of
 * every detection of a frame is supported by its object cloud and by the depth image.  Included by ppf_hip.hip; the host
 * side is ppf_verify_host.h.
 *
 * Neighbour structure: one hashed uniform grid per live detection over its finite scene rows, cell edge
 * inlier_dist * VFY_CELL_MARGIN, cell = floor of the absolute coordinate / edge in fp64 (no bounding-box pass), the cell
 * index clamped to +-2^30 before the conversion to int.  A scene row within inlier_dist of a query lies in one of the 3 x 3 x 3
 * cells around the query's (the margin covers the fp32 rounding of the distance test); a hash collision only adds candidates,
 * every candidate's distance is tested.  Detection i owns next_pow2(max(64, 2 n_scene_i)) slots of the concatenated table:
 *   k_vfy_grid_count    per scene row its slot and its rank among the slot's rows (u32 atomics on the slot counters)
 *   (exclusive scan of the concatenated counters, one trailing element: frame_scan)
 *   k_vfy_grid_scatter  float4 (x, y, z, row) at slot start + rank; the order inside a slot is arbitrary and does not matter
 * Scoring: one thread per (job, model row scored), 256 per block, grid (blocks of the largest job) x jobs:
 *   k_vfy_score   moves its row (icp_transform_row: the bits of ppf_transform_pc_pose), the facing / inlier / depth tests,
 *                 per-block counts through wave ballots, the block's fp64 sum of the inliers' least d2 through a fixed
 *                 shuffle tree and the waves in order; one partial per (job, block) in block order
 *   k_vfy_finish  one wave per job: lane l adds the partials of a contiguous range of blocks in block order, the lanes meet in
 *                 a fixed shuffle tree; writes the job's ppf_pose_score
 * No float atomics: a pose's score row depends only on its own job, never on the other jobs or detections of the call.
 */
#ifndef PPF_VERIFY_KERNELS_H
#define PPF_VERIFY_KERNELS_H

constexpr int VFY_BLOCK = 256;
constexpr double VFY_CELL_MARGIN = 1.001;
constexpr double VFY_CELL_CLAMP = 1073741824.0; /* 2^30 */

struct VfyDet {
  const float* rows; /* n x 6 */
  int n;
  uint32_t slot_off, slot_mask; /* the detection's slots: slot_off .. slot_off + slot_mask */
  uint32_t row_off;             /* the detection's first row in the concatenated rank array */
};

struct VfyJob {
  double T[16];
  const float* model; /* n_model x 6 */
  const float* scene; /* the detection's scene rows (normals under PPF_VERIFY_NORMALS) */
  int n_rows;         /* ceil(n_model / step) */
  int nb;             /* blocks of k_vfy_score that carry rows */
  int det;            /* index into the VfyDet table */
  int pad;
};

struct VfyArgs {
  const VfyDet* dets;
  const VfyJob* jobs;
  const uint32_t* slot_start; /* exclusive scan of the slot counters, + total */
  const float4* pts;          /* scene rows in slot order: x y z, row index as int bits */
  const float* depth;         /* NULL: no depth test */
  int rows, cols;
  double fx, fy, ppx, ppy;
  double inv_h; /* 1 / (inlier_dist * VFY_CELL_MARGIN) */
  float r2, normal_cos, depth_tol;
  int step, all_rows, normals, max_nb;
};

struct VfyPartial {
  uint32_t c[6]; /* considered, inliers, visible, supported, occluded, violations */
  double s;      /* sum of the inliers' least d2 */
};

__device__ __forceinline__ int vfy_cell(float v, double inv_h) {
  double c = floor((double)v * inv_h);
  c = c < -VFY_CELL_CLAMP ? -VFY_CELL_CLAMP : (c > VFY_CELL_CLAMP ? VFY_CELL_CLAMP : c); /* NaN never gets here */
  return (int)c;
}

__device__ __forceinline__ uint32_t vfy_hash(int cx, int cy, int cz, uint32_t mask) {
  return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u)) & mask;
}

__device__ __forceinline__ bool vfy_finite6(const float* p) {
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]) && isfinite(p[4]) && isfinite(p[5]);
}

/* grid (blocks of the largest scene) x live detections; rank[row_off + r] = the row's rank in its slot, ~0u when left out */
__global__ __launch_bounds__(256) void k_vfy_grid_count(const VfyDet* __restrict__ dets, double inv_h, uint32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ rank) {
  const VfyDet D = dets[blockIdx.y];
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.n) return;
  const float* p = D.rows + (size_t)r * 6;
  uint32_t k = ~0u;
  if (vfy_finite6(p)) {
    const uint32_t slot = D.slot_off + vfy_hash(vfy_cell(p[0], inv_h), vfy_cell(p[1], inv_h), vfy_cell(p[2], inv_h), D.slot_mask);
    k = atomicAdd(&counts[slot], 1u);
  }
  rank[D.row_off + r] = k;
}

__global__ __launch_bounds__(256) void k_vfy_grid_scatter(const VfyDet* __restrict__ dets, double inv_h, const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ rank, float4* __restrict__ pts) {
  const VfyDet D = dets[blockIdx.y];
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.n) return;
  const uint32_t k = rank[D.row_off + r];
  if (k == ~0u) return;
  const float* p = D.rows + (size_t)r * 6;
  const uint32_t slot = D.slot_off + vfy_hash(vfy_cell(p[0], inv_h), vfy_cell(p[1], inv_h), vfy_cell(p[2], inv_h), D.slot_mask);
  pts[start[slot] + k] = make_float4(p[0], p[1], p[2], __int_as_float(r));
}

/* the least d2 over the scene rows that support (x, y, z, n): false when there is none */
__device__ __forceinline__ bool vfy_nearest(const VfyArgs& a, const VfyDet& D, const float* scene, const float* o, float* best) {
  const int cx = vfy_cell(o[0], a.inv_h), cy = vfy_cell(o[1], a.inv_h), cz = vfy_cell(o[2], a.inv_h);
  bool found = false;
  float m = 0.f;
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const uint32_t slot = D.slot_off + vfy_hash(cx + dx, cy + dy, cz + dz, D.slot_mask);
        const uint32_t e = a.slot_start[slot + 1];
        for (uint32_t q = a.slot_start[slot]; q < e; q++) {
          const float4 s = a.pts[q];
          const float ex = s.x - o[0], ey = s.y - o[1], ez = s.z - o[2];
          const float d2 = ex * ex + ey * ey + ez * ez;
          if (!(d2 <= a.r2)) continue;
          if (a.normals) {
            const float* sn = scene + (size_t)__float_as_int(s.w) * 6 + 3;
            if (!(o[3] * sn[0] + o[4] * sn[1] + o[5] * sn[2] >= a.normal_cos)) continue;
          }
          if (!found || d2 < m) m = d2;
          found = true;
        }
      }
  *best = m;
  return found;
}

/* the body of k_vfy_score; with VIS a considered row must also be visible in its own pose's render (rnd_visible, *rv:
 * ppf_render_kernels.h, ppf_verify_frame_rendered) -- every other bit is shared */
template <bool VIS, class View>
__device__ __forceinline__ void vfy_score_rows(const VfyArgs& a, const View* rv, VfyPartial* __restrict__ part) {
  __shared__ uint32_t wc[VFY_BLOCK / 64][6];
  __shared__ double ws[VFY_BLOCK / 64];
  const VfyJob& J = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= J.nb) return; /* the grid is sized for the largest job: uniform per block */
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * VFY_BLOCK + threadIdx.x;
  bool cons = false, inl = false, vis = false, sup = false, occ = false, vio = false;
  double d2 = 0.0;
  if (r < J.n_rows) {
    double M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = J.T[k];
    const float* p = J.model + (size_t)r * a.step * 6;
    float o[6];
    icp_transform_row(p, p + 3, M, o);
    if (vfy_finite6(o)) {
      const double facing = (double)o[3] * (double)o[0] + (double)o[4] * (double)o[1] + (double)o[5] * (double)o[2];
      cons = a.all_rows || facing < 0.0;
      if constexpr (VIS) cons = cons && rnd_visible(o, *rv, (int)blockIdx.y);
    }
    if (cons) {
      float m;
      inl = vfy_nearest(a, a.dets[J.det], J.scene, o, &m);
      if (inl) d2 = (double)m;
      if (a.depth && o[2] > 0.f) {
        const double uf = (double)o[0] * a.fx / (double)o[2] + a.ppx;
        const double vf = (double)o[1] * a.fy / (double)o[2] + a.ppy;
        const double ui = floor(uf + 0.5), vi = floor(vf + 0.5);
        if (ui >= 0.0 && ui < (double)a.cols && vi >= 0.0 && vi < (double)a.rows) {
          const float d = a.depth[(size_t)(int)vi * a.cols + (int)ui];
          if (isfinite(d) && d > 0.f) {
            vis = true;
            const float e = d - o[2];
            sup = fabsf(e) <= a.depth_tol;
            occ = e < -a.depth_tol;
            vio = e > a.depth_tol;
          }
        }
      }
    }
  }
  const bool f[6] = {cons, inl, vis, sup, occ, vio};
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const uint32_t c = (uint32_t)__popcll(__ballot(f[k]));
    if (lane == 0) wc[wv][k] = c;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d2 += __shfl_down(d2, off);
  if (lane == 0) ws[wv] = d2;
  __syncthreads();
  if (threadIdx.x == 0) {
    VfyPartial P;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      uint32_t t = 0;
      for (int w = 0; w < VFY_BLOCK / 64; w++) t += wc[w][k];
      P.c[k] = t;
    }
    double s = ws[0];
    for (int w = 1; w < VFY_BLOCK / 64; w++) s += ws[w];
    P.s = s;
    part[(size_t)blockIdx.y * a.max_nb + blockIdx.x] = P;
  }
}

__global__ __launch_bounds__(VFY_BLOCK) void k_vfy_score(VfyArgs a, VfyPartial* __restrict__ part) {
  vfy_score_rows<false>(a, (const int*)nullptr, part);
}

/* one 64-thread block per job */
__global__ __launch_bounds__(64) void k_vfy_finish(const VfyJob* __restrict__ jobs, const VfyPartial* __restrict__ part, int max_nb,
                                                   int has_depth, ppf_pose_score* __restrict__ out) {
  const int job = blockIdx.x, lane = threadIdx.x;
  const VfyJob& J = jobs[job];
  const int per = (J.nb + 63) / 64;
  const int b0 = min(J.nb, lane * per), b1 = min(J.nb, b0 + per);
  uint32_t c[6] = {0, 0, 0, 0, 0, 0};
  double s = 0.0;
  for (int b = b0; b < b1; b++) {
    const VfyPartial& P = part[(size_t)job * max_nb + b];
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] += P.c[k];
    s += P.s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] += (uint32_t)__shfl_down((int)c[k], off);
  }
  if (lane != 0) return;
  ppf_pose_score r;
  r.n_rows = J.n_rows;
  r.n_considered = (int32_t)c[0];
  r.n_inliers = (int32_t)c[1];
  r.n_visible = (int32_t)c[2];
  r.n_supported = (int32_t)c[3];
  r.n_occluded = (int32_t)c[4];
  r.n_violations = (int32_t)c[5];
  r.inlier_rmse = c[1] ? (float)ppf_sqrt(s / (double)c[1]) : 0.f;
  r.fitness = c[0] ? (float)((double)c[1] / (double)c[0]) : 0.f;
  const uint32_t den = c[2] - c[4];
  r.support = den ? (float)((double)c[3] / (double)den) : 0.f;
  r.score = has_depth ? r.support : r.fitness;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
  out[job] = r;
}

#endif /* PPF_VERIFY_KERNELS_H */
