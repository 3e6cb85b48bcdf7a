/*
 * ppf_edge_kernels.h — a depth image's occluding, occluded and boundary edges on gfx950 (ppf_depth_edges).
 * Included by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_z, depth_keep, depth_back_project); host side:
 * ppf_edge_host.h.
 *
 * The image is cut into tiles of EDGE_TW x EDGE_TH pixels and, finer, into runs: run (v, t) is the pixels u = 64 t .. 64 t + 63
 * of image row v, and run index v * tiles_x + t grows with the pixel index, so a scan over per-run counts ranks pixels in
 * row-major order.  One wave always owns one run, so a ballot is a run's count and no atomic decides a place.
 *
 *   k_depth_edges   one 256-thread workgroup per tile.  (1) The tile plus a halo of max_gap + 1 pixels is staged in LDS as one
 *                   float plane: z of a kept pixel (> 0), EDGE_NOT_KEPT or EDGE_OUTSIDE.  Loads go through the row pitch and
 *                   never leave the image; z is converted once per staged pixel.  (2) Wave w owns the tile rows w, w + 4, ...;
 *                   one lane per pixel walks its 8 directions out of LDS (the 64 lanes of a wave read 64 consecutive words of
 *                   a row, or of rows one word apart: no bank conflict) and writes the pixel's mask byte.  The ballots of
 *                   kept and selected are the run's counts (run_kept, run_sel); the class counts are popcounts of ballots,
 *                   summed per wave in registers, per block in LDS, one integer atomicAdd per counter and block.  With
 *                   `mark` the byte also carries EDGE_W_KEPT for the passes below.
 *   k_edge_select   with a normals cloud, after the scan of run_kept: one wave per run.  A kept pixel's normals row is the
 *                   run's offset plus its rank in the ballot; a row at or past the cloud's count reads nothing (the host
 *                   refuses the call at its first wait).  Sets PPF_EDGE_CURVATURE, writes the final mask, marks the pixels
 *                   that go to the cloud (EDGE_W_CLOUD) and counts them per run.
 *   k_edge_write    after the scan of run_sel: one wave per run; the cloud's row is the run's offset plus the ballot rank.
 *                   With normals the row is copied word for word, without it is ppf_cloud_from_depth's.
 * Nothing is fused (-ffp-contract=off), no float atomic, no private memory; no launch depends on the image's content.
 */
#ifndef PPF_EDGE_KERNELS_H
#define PPF_EDGE_KERNELS_H

constexpr int EDGE_TW = 64, EDGE_TH = 16; /* a tile: a wave spans a tile row; 16 rows keep the halo of 3 at half the tile */
constexpr int EDGE_BLOCK = 256;
constexpr int EDGE_WAVES = EDGE_BLOCK / 64;
constexpr int EDGE_MAX_H = PPF_DEPTH_EDGE_MAX_GAP + 1;
constexpr int EDGE_LDS = (EDGE_TW + 2 * EDGE_MAX_H) * (EDGE_TH + 2 * EDGE_MAX_H);
constexpr float EDGE_NOT_KEPT = 0.f, EDGE_OUTSIDE = -1.f; /* a kept z is > 0 */
constexpr uint8_t EDGE_CLASSES = 15, EDGE_W_CLOUD = 64, EDGE_W_KEPT = 128; /* the work byte: the mask and two marks */
constexpr int EDGE_C_KEPT = 0, EDGE_C_OCCLUDING = 1, EDGE_C_OCCLUDED = 2, EDGE_C_BOUNDARY = 3, EDGE_C_CURVATURE = 4, EDGE_C_EDGE = 5,
              EDGE_C_SELECTED = 6, EDGE_C_NO_NORMAL = 7, EDGE_N_COUNTERS = 8;
static_assert(EDGE_TW == 64 && EDGE_BLOCK == 256 && EDGE_TH % EDGE_WAVES == 0, "a wave spans a tile row");

struct EdgeArgs {
  int rows, tiles_x, tiles_y; /* tiles per image row and column; runs: rows * tiles_x */
  int max_gap, select;
  int mark;   /* 1: a later pass follows, the work byte carries EDGE_W_KEPT */
  int final_; /* 1: the geometric mask is the result: k_depth_edges counts edge and selected pixels too */
  double depth_abs, depth_quad;
  float curvature_threshold;
  const float* nrm_rows; /* the normals cloud's n x 6 rows, or NULL */
  const float* nrm_curv;
  uint32_t nrm_n;
  uint32_t* counters; /* EDGE_N_COUNTERS, preset to 0 */
  uint32_t* run_kept; /* [runs + 1] or NULL */
  uint32_t* run_sel;  /* [runs + 1] or NULL */
};

/* one direction of the walk; c is the pixel's word in the staged plane, d the direction's step in words */
__device__ __forceinline__ int edge_walk(const float* sz, int c, int d, double zp, const EdgeArgs& ea) {
  if (sz[c + d] == EDGE_OUTSIDE) return 0;
  for (int j = 1; j <= ea.max_gap + 1; j++) {
    const float q = sz[c + j * d];
    if (q == EDGE_OUTSIDE) break;
    if (q > 0.f) {
      const double zq = (double)q;
      if (!(ppf_fabs(zq - zp) > ea.depth_abs + ea.depth_quad * (zp * zq))) return 0;
      return zq > zp ? PPF_EDGE_OCCLUDING : (zq < zp ? PPF_EDGE_OCCLUDED : 0);
    }
  }
  return PPF_EDGE_BOUNDARY;
}

/* grid: tiles_x * tiles_y */
template <class T>
__global__ __launch_bounds__(EDGE_BLOCK) void k_depth_edges(DepthArgs a, EdgeArgs ea, uint8_t* __restrict__ out) {
  __shared__ float sz[EDGE_LDS];
  __shared__ uint32_t s_n[EDGE_WAVES][EDGE_N_COUNTERS];
  const int h = ea.max_gap + 1;
  const int zw = EDGE_TW + 2 * h, zh = EDGE_TH + 2 * h; /* the staged plane: origin (u0 - h, v0 - h) */
  const int tile_y = (int)blockIdx.x / ea.tiles_x, tile_x = (int)blockIdx.x - tile_y * ea.tiles_x;
  const long long u0 = (long long)tile_x * EDGE_TW, v0 = (long long)tile_y * EDGE_TH;
  for (int i = threadIdx.x; i < zw * zh; i += EDGE_BLOCK) {
    const int wy = i / zw, wx = i - wy * zw;
    const long long u = u0 - h + wx, v = v0 - h + wy;
    float z = EDGE_OUTSIDE;
    if (u >= 0 && u < a.cols && v >= 0 && v < ea.rows) {
      const float zq = depth_z(reinterpret_cast<const T*>(a.img + (size_t)v * a.pitch) + u, a);
      z = depth_keep(zq, a) ? zq : EDGE_NOT_KEPT;
    }
    sz[i] = z;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long u = u0 + lx;
  uint32_t n_kept = 0, n_ing = 0, n_ed = 0, n_bnd = 0, n_edge = 0, n_sel = 0;
#pragma unroll 1
  for (int ly = wv; ly < EDGE_TH; ly += EDGE_WAVES) {
    const long long v = v0 + ly;
    if (v >= ea.rows) break; /* uniform in the wave */
    const bool inside = u < a.cols;
    const int c = (ly + h) * zw + lx + h;
    const float pz = sz[c];
    const bool kept = inside && pz > 0.f;
    int m = 0;
    if (kept) {
      const double zp = (double)pz;
      m |= edge_walk(sz, c, -zw - 1, zp, ea);
      m |= edge_walk(sz, c, -zw, zp, ea);
      m |= edge_walk(sz, c, -zw + 1, zp, ea);
      m |= edge_walk(sz, c, -1, zp, ea);
      m |= edge_walk(sz, c, 1, zp, ea);
      m |= edge_walk(sz, c, zw - 1, zp, ea);
      m |= edge_walk(sz, c, zw, zp, ea);
      m |= edge_walk(sz, c, zw + 1, zp, ea);
    }
    if (inside) out[(size_t)v * (size_t)a.cols + (size_t)u] = (uint8_t)(m | ((ea.mark && kept) ? EDGE_W_KEPT : 0));
    const uint32_t c_kept = (uint32_t)__popcll(__ballot(kept)), c_sel = (uint32_t)__popcll(__ballot((m & ea.select) != 0));
    n_kept += c_kept;
    n_sel += c_sel;
    n_ing += (uint32_t)__popcll(__ballot((m & PPF_EDGE_OCCLUDING) != 0));
    n_ed += (uint32_t)__popcll(__ballot((m & PPF_EDGE_OCCLUDED) != 0));
    n_bnd += (uint32_t)__popcll(__ballot((m & PPF_EDGE_BOUNDARY) != 0));
    n_edge += (uint32_t)__popcll(__ballot(m != 0));
    if (lx == 0) {
      const size_t run = (size_t)v * (size_t)ea.tiles_x + (size_t)tile_x;
      if (ea.run_kept) ea.run_kept[run] = c_kept;
      if (ea.run_sel && ea.final_) ea.run_sel[run] = c_sel;
    }
  }
  if (lx == 0) {
    s_n[wv][EDGE_C_KEPT] = n_kept;
    s_n[wv][EDGE_C_OCCLUDING] = n_ing;
    s_n[wv][EDGE_C_OCCLUDED] = n_ed;
    s_n[wv][EDGE_C_BOUNDARY] = n_bnd;
    s_n[wv][EDGE_C_CURVATURE] = 0u;
    s_n[wv][EDGE_C_EDGE] = ea.final_ ? n_edge : 0u;
    s_n[wv][EDGE_C_SELECTED] = ea.final_ ? n_sel : 0u;
    s_n[wv][EDGE_C_NO_NORMAL] = 0u;
  }
  __syncthreads();
  if (threadIdx.x < EDGE_N_COUNTERS) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < EDGE_WAVES; w++) n += s_n[w][threadIdx.x];
    if (n) atomicAdd(&ea.counters[threadIdx.x], n);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { /* the trailing elements the scans turn into the totals */
    const size_t runs = (size_t)ea.rows * (size_t)ea.tiles_x;
    if (ea.run_kept) ea.run_kept[runs] = 0u;
    if (ea.run_sel) ea.run_sel[runs] = 0u;
  }
}

/* the pixel of this lane in run `run`: false past the image's last column */
__device__ __forceinline__ bool edge_run_pixel(const DepthArgs& a, const EdgeArgs& ea, size_t run, int lane, int* u, int* v) {
  *v = (int)(run / (size_t)ea.tiles_x);
  const long long uu = (long long)(run - (size_t)*v * (size_t)ea.tiles_x) * 64 + lane;
  *u = (int)uu;
  return uu < a.cols;
}

/* grid: ceil(runs / EDGE_WAVES); work: k_depth_edges' bytes with EDGE_W_KEPT; out: the final mask or NULL */
__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_select(DepthArgs a, EdgeArgs ea, const uint32_t* __restrict__ run_koff,
                                                            uint8_t* __restrict__ work, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_n[EDGE_WAVES][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t runs = (size_t)ea.rows * (size_t)ea.tiles_x, run = (size_t)blockIdx.x * EDGE_WAVES + wv;
  uint32_t n_curv = 0, n_edge = 0, n_sel = 0, n_non = 0;
  if (run < runs) { /* uniform in the wave */
    int u, v;
    const bool inside = edge_run_pixel(a, ea, run, lane, &u, &v);
    const size_t p = (size_t)v * (size_t)a.cols + (size_t)u;
    const uint8_t w = inside ? work[p] : (uint8_t)0;
    const bool kept = (w & EDGE_W_KEPT) != 0;
    const unsigned long long bk = __ballot(kept);
    const uint32_t row = run_koff[run] + __builtin_amdgcn_mbcnt_hi((uint32_t)(bk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bk, 0u));
    int m = w & EDGE_CLASSES;
    bool finite = false;
    if (kept && row < ea.nrm_n) {
      const float* nr = ea.nrm_rows + (size_t)row * 6;
      finite = isfinite(nr[3]) && isfinite(nr[4]) && isfinite(nr[5]);
      if (ea.nrm_curv[row] > ea.curvature_threshold) m |= PPF_EDGE_CURVATURE;
    }
    const bool sel = (m & ea.select) != 0, cloud = sel && finite;
    if (inside) {
      work[p] = (uint8_t)(m | (kept ? EDGE_W_KEPT : 0) | (cloud ? EDGE_W_CLOUD : 0));
      if (out) out[p] = (uint8_t)m;
    }
    n_curv = (uint32_t)__popcll(__ballot((m & PPF_EDGE_CURVATURE) != 0));
    n_edge = (uint32_t)__popcll(__ballot(m != 0));
    n_sel = (uint32_t)__popcll(__ballot(sel));
    n_non = (uint32_t)__popcll(__ballot(sel && !finite));
    if (lane == 0 && ea.run_sel) ea.run_sel[run] = n_sel - n_non;
  }
  if (lane == 0) {
    s_n[wv][0] = n_curv;
    s_n[wv][1] = n_edge;
    s_n[wv][2] = n_sel;
    s_n[wv][3] = n_non;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < EDGE_WAVES; w++) n += s_n[w][threadIdx.x];
    if (n) atomicAdd(&ea.counters[EDGE_C_CURVATURE + threadIdx.x], n);
  }
}

/* grid: ceil(runs / EDGE_WAVES); work: the mask (no normals) or k_edge_select's bytes; rows / curv: the cloud of n_rows rows */
template <class T>
__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_write(DepthArgs a, EdgeArgs ea, const uint32_t* __restrict__ run_koff,
                                                           const uint32_t* __restrict__ run_soff, const uint8_t* __restrict__ work,
                                                           uint32_t n_rows, float* __restrict__ rows, float* __restrict__ curv) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t runs = (size_t)ea.rows * (size_t)ea.tiles_x, run = (size_t)blockIdx.x * EDGE_WAVES + wv;
  if (run >= runs) return; /* uniform in the wave */
  int u, v;
  const bool inside = edge_run_pixel(a, ea, run, lane, &u, &v);
  const uint8_t w = inside ? work[(size_t)v * (size_t)a.cols + (size_t)u] : (uint8_t)0;
  const bool cloud = ea.nrm_rows ? (w & EDGE_W_CLOUD) != 0 : (w & ea.select) != 0;
  const unsigned long long bc = __ballot(cloud);
  const uint32_t dst = run_soff[run] + __builtin_amdgcn_mbcnt_hi((uint32_t)(bc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bc, 0u));
  if (ea.nrm_rows) {
    const unsigned long long bk = __ballot((w & EDGE_W_KEPT) != 0);
    const uint32_t src = run_koff[run] + __builtin_amdgcn_mbcnt_hi((uint32_t)(bk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bk, 0u));
    if (cloud && dst < n_rows && src < ea.nrm_n) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(ea.nrm_rows) + (size_t)src * 6;
      uint32_t* d = reinterpret_cast<uint32_t*>(rows) + (size_t)dst * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) d[k] = s[k];
      reinterpret_cast<uint32_t*>(curv)[dst] = reinterpret_cast<const uint32_t*>(ea.nrm_curv)[src];
    }
  } else if (cloud && dst < n_rows) {
    const float z = depth_z(reinterpret_cast<const T*>(a.img + (size_t)v * a.pitch) + u, a);
    float* d = rows + (size_t)dst * 6;
    d[0] = depth_back_project(u, a.ppx, a.fx, z, a.fp64);
    d[1] = depth_back_project(v, a.ppy, a.fy, z, a.fp64);
    d[2] = z;
    d[3] = 0.f;
    d[4] = 0.f;
    d[5] = 0.f;
    curv[dst] = 0.f;
  }
}

#endif /* PPF_EDGE_KERNELS_H */
