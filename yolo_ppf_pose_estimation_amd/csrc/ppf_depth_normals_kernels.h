/*
 * ppf_depth_normals_kernels.h — normals and curvature of the organised scene cloud from the depth image's own
 * neighbourhoods on gfx950 (ppf_cloud_from_depth_normals).  Included by ppf_hip.hip after ppf_prep_kernels.h
 * (prep_smallest_eigvec) and ppf_depth_kernels.h (DepthArgs, depth_pixel, depth_back_project); host side: ppf_depth_host.h.
 *
 *   k_depth_normals   one 256-thread workgroup per tile of DN_TILE_W x DN_TILE_H pixels.  The tile plus a halo of `radius`
 *                     pixels is staged in LDS as three float planes x, y, z (the values the cloud's rows hold); a pixel
 *                     that is not kept or lies outside the image has z = NaN, which no depth test passes.  Loads are
 *                     clamped to the image and go through the row pitch.  Then one lane owns one pixel (wave w = tile row
 *                     w, lane = column): it walks its window twice, row by row -- the 64 lanes of a wave read 64
 *                     consecutive words of a plane, no bank conflict, and a lane's order is the specified one (dv, then du)
 *                     -- for the centroid and then the covariance, each a sequential fp64 sum of that lane alone, runs
 *                     prep_smallest_eigvec in registers and writes {nx, ny, nz, curvature} and a flag (DN_NOT_KEPT /
 *                     DN_NORMAL / DN_NO_NORMAL) at the pixel's index.
 *   k_depthn_count    k_depth_count on the flags (PPF_DEPTH_NORMALS_DROP: only DN_NORMAL counts)
 *   k_depthn_scatter  k_depth_scatter on the flags: x y z recomputed from the image by the same functions, the normal and
 *                     curvature copied from the pixel's slot
 * No atomics; nothing is fused (-ffp-contract=off), no sum is a tree; the launches do not depend on the image's content.
 */
#ifndef PPF_DEPTH_NORMALS_KERNELS_H
#define PPF_DEPTH_NORMALS_KERNELS_H

constexpr int DN_TILE_W = 64, DN_TILE_H = 4; /* one wave per tile row */
constexpr int DN_BLOCK = DN_TILE_W * DN_TILE_H;
constexpr int DN_LDS_PIXELS = (DN_TILE_W + 2 * PPF_DEPTH_NORMALS_MAX_RADIUS) * (DN_TILE_H + 2 * PPF_DEPTH_NORMALS_MAX_RADIUS);
static_assert(DN_BLOCK == DEPTH_BLOCK && DN_TILE_W == 64, "one wave per tile row; the count and scatter kernels share DEPTH_BLOCK");
constexpr uint8_t DN_NOT_KEPT = 0, DN_NORMAL = 1, DN_NO_NORMAL = 2;

struct DepthNormalArgs {
  int rows, tiles_x; /* tiles per image row; the grid is tiles_x * ceil(rows / DN_TILE_H) */
  int radius, min_neighbours;
  float max_depth_change;
  int drop;
};

template <class T>
__global__ __launch_bounds__(DN_BLOCK) void k_depth_normals(DepthArgs a, DepthNormalArgs na, float4* __restrict__ nrm,
                                                            uint8_t* __restrict__ flag) {
  __shared__ float sx[DN_LDS_PIXELS], sy[DN_LDS_PIXELS], sz[DN_LDS_PIXELS];
  const int r = na.radius, tw = DN_TILE_W + 2 * r, th = DN_TILE_H + 2 * r;
  const int tile_y = (int)blockIdx.x / na.tiles_x, tile_x = (int)blockIdx.x - tile_y * na.tiles_x;
  const long long u0 = (long long)tile_x * DN_TILE_W, v0 = (long long)tile_y * DN_TILE_H;
  for (int i = threadIdx.x; i < tw * th; i += DN_BLOCK) {
    const int wy = i / tw, wx = i - wy * tw;
    const long long u = u0 - r + wx, v = v0 - r + wy;
    float x = 0.f, y = 0.f, z = __builtin_nanf("");
    if (u >= 0 && u < a.cols && v >= 0 && v < na.rows) {
      const float zq = depth_z(reinterpret_cast<const T*>(a.img + (size_t)v * a.pitch) + u, a);
      if (depth_keep(zq, a)) {
        x = depth_back_project((int)u, a.ppx, a.fx, zq, a.fp64);
        y = depth_back_project((int)v, a.ppy, a.fy, zq, a.fp64);
        z = zq;
      }
    }
    sx[i] = x; sy[i] = y; sz[i] = z;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const long long u = u0 + lx, v = v0 + ly;
  if (u >= a.cols || v >= na.rows) return;
  const size_t p = (size_t)v * (size_t)a.cols + (size_t)u;
  const int ci = (ly + r) * tw + lx + r;
  const float pz = sz[ci];
  if (pz != pz) { flag[p] = DN_NOT_KEPT; return; }
  const double zp = (double)pz, lim = (double)na.max_depth_change * zp;
  /* the window of this lane starts at LDS pixel (ly, lx); a NaN z fails the test */
  const int side = 2 * r + 1;
  int k = 0;
  double c[3] = {0, 0, 0};
  for (int dv = 0; dv < side; dv++) {
    const int rb = (ly + dv) * tw + lx;
    for (int du = 0; du < side; du++) {
      const double zq = (double)sz[rb + du];
      if (ppf_fabs(zq - zp) <= lim) {
        k++;
        c[0] += (double)sx[rb + du]; c[1] += (double)sy[rb + du]; c[2] += zq;
      }
    }
  }
  if (k < na.min_neighbours) {
    const float qn = __builtin_nanf("");
    nrm[p] = make_float4(qn, qn, qn, qn);
    flag[p] = DN_NO_NORMAL;
    return;
  }
  c[0] /= (double)k; c[1] /= (double)k; c[2] /= (double)k;
  double cov[6] = {0, 0, 0, 0, 0, 0};
  for (int dv = 0; dv < side; dv++) {
    const int rb = (ly + dv) * tw + lx;
    for (int du = 0; du < side; du++) {
      const double zq = (double)sz[rb + du];
      if (ppf_fabs(zq - zp) <= lim) {
        const double d0 = (double)sx[rb + du] - c[0], d1 = (double)sy[rb + du] - c[1], d2 = zq - c[2];
        cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2;
        cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 6; m++) cov[m] /= (double)k;
  const double trace = cov[0] + cov[3] + cov[5];
  double nv[3];
  double lam = prep_smallest_eigvec(cov, nv);
  const double cos_theta = -((double)sx[ci] * nv[0] + (double)sy[ci] * nv[1] + zp * nv[2]);
  if (cos_theta < 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  if (lam < 0) lam = -lam;
  const double at = trace < 0 ? -trace : trace;
  nrm[p] = make_float4((float)nv[0], (float)nv[1], (float)nv[2], trace != 0.0 ? (float)(lam / at) : 0.f);
  flag[p] = DN_NORMAL;
}

__device__ __forceinline__ bool depthn_keep(const uint8_t* __restrict__ flag, int p, int n, int drop) {
  if (p >= n) return false;
  const uint8_t f = flag[p];
  return drop ? f == DN_NORMAL : f != DN_NOT_KEPT;
}

/* as k_depth_count, the validity read from the flags */
__global__ __launch_bounds__(DEPTH_BLOCK) void k_depthn_count(const uint8_t* __restrict__ flag, int n, int drop, int n_tiles,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[DEPTH_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * DEPTH_TILE;
  uint32_t cnt = 0;
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    const long long p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    const bool keep = p < n && depthn_keep(flag, (int)p, n, drop);
    cnt += (uint32_t)__popcll(__ballot(keep));
  }
  if (lane == 0) wave_cnt[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < DEPTH_BLOCK / 64; w++) t += wave_cnt[w];
    counts[blockIdx.x] = t;
    if (blockIdx.x == 0) counts[n_tiles] = 0; /* the trailing element the scan turns into the total */
  }
}

/* as k_depth_scatter, with the pixel's normal and curvature */
template <class T>
__global__ __launch_bounds__(DEPTH_BLOCK) void k_depthn_scatter(DepthArgs a, const uint8_t* __restrict__ flag, int drop,
                                                                const float4* __restrict__ nrm, const uint32_t* __restrict__ tile_off,
                                                                float* __restrict__ rows, float* __restrict__ curv) {
  __shared__ uint32_t cnt[DEPTH_ROUNDS][DEPTH_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * DEPTH_TILE;
  bool keep[DEPTH_ROUNDS];
  uint32_t below[DEPTH_ROUNDS]; /* kept lanes of this wave below this one, per round */
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    const long long p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    keep[r] = p < a.n && depthn_keep(flag, (int)p, a.n, drop);
    const unsigned long long m = __ballot(keep[r]);
    below[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) cnt[r][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t off = tile_off[blockIdx.x];
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    uint32_t o = off;
#pragma unroll
    for (int w = 0; w < DEPTH_BLOCK / 64; w++) {
      if (w < wv) o += cnt[r][w];
      off += cnt[r][w];
    }
    if (keep[r]) {
      const int p = (int)(base + r * DEPTH_BLOCK + (int)threadIdx.x);
      int u, v;
      float z;
      (void)depth_pixel<T>(a, p, &u, &v, &z);
      const float4 nc = nrm[p];
      float* row = rows + (size_t)(o + below[r]) * 6;
      row[0] = depth_back_project(u, a.ppx, a.fx, z, a.fp64);
      row[1] = depth_back_project(v, a.ppy, a.fy, z, a.fp64);
      row[2] = z;
      row[3] = nc.x;
      row[4] = nc.y;
      row[5] = nc.z;
      curv[o + below[r]] = nc.w;
    }
  }
}

#endif /* PPF_DEPTH_NORMALS_KERNELS_H */
