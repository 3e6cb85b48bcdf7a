/*
 * ppf_depth_kernels.h — the organised scene cloud from a depth image on gfx950 (ppf_cloud_from_depth).
 * Included by ppf_hip.hip; the host side is ppf_depth_host.h.
 *
 * The image is cut into tiles of DEPTH_TILE pixels in row-major pixel order (p = v * cols + u).  One 256-thread
 * workgroup per tile takes its pixels in DEPTH_ROUNDS rounds of 256 (pixel base + r * 256 + threadIdx.x), so within a tile
 * the order is (round, wave, lane) == pixel order.  Two passes over the image:
 *   k_depth_count    per wave and round a ballot of the validity flags and its popcount; the tile's total -> counts[tile]
 *   (exclusive scan of the tile counts, one trailing element for the total: device_exclusive_scan)
 *   k_depth_scatter  the same flags again; a pixel's row = tile offset + the (round, wave)s before it + its lane's rank in
 *                    the ballot mask (mbcnt); writes x y z 0 0 0 and curvature 0
 * No atomic decides an order, so the result is deterministic and identical to np.nonzero order.  The arithmetic is
 * evaluated exactly as written (the library is built with -ffp-contract=off): no FMA, IEEE fp32 multiply, fp64 multiply
 * and divide, round-to-nearest conversions -- the bits equal the host's.
 */
#ifndef PPF_DEPTH_KERNELS_H
#define PPF_DEPTH_KERNELS_H

constexpr int DEPTH_BLOCK = 256;
constexpr int DEPTH_ROUNDS = 4;
constexpr int DEPTH_TILE = DEPTH_BLOCK * DEPTH_ROUNDS; /* 1,024 pixels: the C1 frame is 900 tiles, one scan launch */

struct DepthArgs {
  const unsigned char* img; /* first pixel of row 0 */
  size_t pitch;             /* bytes between rows */
  int cols, n;              /* n = rows * cols (<= INT32_MAX) */
  double fx, fy, ppx, ppy;
  double scale;             /* U16: metres per unit */
  float z_min, z_max;
  int fp64;
};

/* metric depth of pixel (u, v): F32 as stored, U16 through the scale in fp64 */
__device__ __forceinline__ float depth_z(const float* px, const DepthArgs&) { return *px; }
__device__ __forceinline__ float depth_z(const uint16_t* px, const DepthArgs& a) { return (float)((double)*px * a.scale); }

__device__ __forceinline__ bool depth_keep(float z, const DepthArgs& a) {
  return isfinite(z) && z > 0.f && z >= a.z_min && (a.z_max == 0.f || z <= a.z_max);
}

/* pixel p (< a.n): its depth and whether it is kept */
template <class T>
__device__ __forceinline__ bool depth_pixel(const DepthArgs& a, int p, int* u, int* v, float* z) {
  *v = p / a.cols;
  *u = p - *v * a.cols;
  *z = depth_z(reinterpret_cast<const T*>(a.img + (size_t)*v * a.pitch) + *u, a);
  return depth_keep(*z, a);
}

/* Camera::back_projection (Camera.h:44-46), or the fp64 formula of the C1 fixtures */
__device__ __forceinline__ float depth_back_project(int u, double pp, double f, float z, int fp64) {
  if (fp64) return (float)(((double)u - pp) * (double)z / f);
  const float d = (float)((double)u - pp);
  return (float)((double)(d * z) / f);
}

template <class T>
__global__ __launch_bounds__(DEPTH_BLOCK) void k_depth_count(DepthArgs a, int n_tiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[DEPTH_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * DEPTH_TILE;
  uint32_t cnt = 0;
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    const int p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    int u, v;
    float z;
    const bool keep = p < a.n && depth_pixel<T>(a, p, &u, &v, &z);
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

template <class T>
__global__ __launch_bounds__(DEPTH_BLOCK) void k_depth_scatter(DepthArgs a, const uint32_t* __restrict__ tile_off, float* __restrict__ rows,
                                                               float* __restrict__ curv) {
  __shared__ uint32_t cnt[DEPTH_ROUNDS][DEPTH_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * DEPTH_TILE;
  bool keep[DEPTH_ROUNDS];
  int u[DEPTH_ROUNDS], v[DEPTH_ROUNDS];
  float z[DEPTH_ROUNDS];
  uint32_t below[DEPTH_ROUNDS]; /* kept lanes of this wave below this one, per round */
#pragma unroll
  for (int r = 0; r < DEPTH_ROUNDS; r++) {
    const int p = base + r * DEPTH_BLOCK + (int)threadIdx.x;
    keep[r] = p < a.n && depth_pixel<T>(a, p, &u[r], &v[r], &z[r]);
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
      float* row = rows + (size_t)(o + below[r]) * 6;
      row[0] = depth_back_project(u[r], a.ppx, a.fx, z[r], a.fp64);
      row[1] = depth_back_project(v[r], a.ppy, a.fy, z[r], a.fp64);
      row[2] = z[r];
      row[3] = 0.f;
      row[4] = 0.f;
      row[5] = 0.f;
      curv[o + below[r]] = 0.f;
    }
  }
}

#endif /* PPF_DEPTH_KERNELS_H */
