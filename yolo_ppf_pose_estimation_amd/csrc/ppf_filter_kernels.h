/*
 * ppf_filter_kernels.h — edge-preserving smoothing of a depth image on gfx950 (ppf_depth_filter).  Included
 * by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_z, depth_keep); host side: ppf_filter_host.h.
 *
 *   k_depth_filter   one 256-thread workgroup per tile of DF_TILE_W x DF_TILE_H pixels, in three steps with a barrier between
 *                    them.  (1) The tile plus a halo of radius + 1 pixels is staged in LDS as one float plane: z of a kept
 *                    pixel (> 0), DF_NOT_KEPT or DF_OUTSIDE.  Loads go through the row pitch and never leave the image.
 *                    The first (2 radius + 1)^2 threads also fill a table of the spatial weights s * s (-1: a tap with
 *                    s <= 0), so the window walk has no division by D.  (2) The support test runs over the tile plus a halo
 *                    of `radius` -- the extra ring of (1) is what lets the halo pixels' own support be decided -- and writes
 *                    a second plane: z of a supported pixel, NaN (no test passes) for every other.  (3) One lane owns one
 *                    pixel (wave w = tile row w, lane = column) and walks its window row by row: the 64 lanes of a wave read
 *                    64 consecutive words of the second plane, no bank conflict, in the specified order (dv, then du); num
 *                    and den are sequential fp64 sums of that lane alone.  Every pixel of the image is written (0 where
 *                    nothing is).  n_kept and n_unsupported come from ballots: one integer atomicAdd each per block.
 * Nothing is fused (-ffp-contract=off), no sum is a tree, no float atomic; the launch does not depend on the image's content.
 */
#ifndef PPF_FILTER_KERNELS_H
#define PPF_FILTER_KERNELS_H

constexpr int DF_TILE_W = 64, DF_TILE_H = 4; /* one wave per tile row */
constexpr int DF_BLOCK = DF_TILE_W * DF_TILE_H;
constexpr int DF_MAX_R = PPF_DEPTH_FILTER_MAX_RADIUS;
constexpr int DF_LDS_Z = (DF_TILE_W + 2 * (DF_MAX_R + 1)) * (DF_TILE_H + 2 * (DF_MAX_R + 1)); /* the staged plane */
constexpr int DF_LDS_S = (DF_TILE_W + 2 * DF_MAX_R) * (DF_TILE_H + 2 * DF_MAX_R);             /* the supported plane */
constexpr int DF_TAPS = (2 * DF_MAX_R + 1) * (2 * DF_MAX_R + 1);
constexpr float DF_NOT_KEPT = 0.f, DF_OUTSIDE = -1.f; /* a kept z is > 0 */
constexpr int DF_C_KEPT = 0, DF_C_UNSUPPORTED = 1, DF_N_COUNTERS = 2;
static_assert(DF_BLOCK == 256 && DF_TILE_W == 64, "one wave per tile row");

struct DepthFilterArgs {
  int rows, tiles_x; /* tiles per image row; the grid is tiles_x * ceil(rows / DF_TILE_H) */
  int radius, min_support;
  float range_abs, range_quad, support_abs, support_quad;
  int32_t* counters; /* DF_N_COUNTERS, preset to 0 */
};

template <class T>
__global__ __launch_bounds__(DF_BLOCK) void k_depth_filter(DepthArgs a, DepthFilterArgs fa, float* __restrict__ out) {
  __shared__ float sz[DF_LDS_Z], ss[DF_LDS_S];
  __shared__ double tap[DF_TAPS];
  __shared__ int s_n[DF_TILE_H][DF_N_COUNTERS];
  const int r = fa.radius, h = r + 1, side = 2 * r + 1;
  const int zw = DF_TILE_W + 2 * h, zh = DF_TILE_H + 2 * h; /* the staged plane: origin (u0 - h, v0 - h) */
  const int pw = DF_TILE_W + 2 * r, ph = DF_TILE_H + 2 * r; /* the supported plane: origin (u0 - r, v0 - r) */
  const int tile_y = (int)blockIdx.x / fa.tiles_x, tile_x = (int)blockIdx.x - tile_y * fa.tiles_x;
  const long long u0 = (long long)tile_x * DF_TILE_W, v0 = (long long)tile_y * DF_TILE_H;
  for (int i = threadIdx.x; i < zw * zh; i += DF_BLOCK) {
    const int wy = i / zw, wx = i - wy * zw;
    const long long u = u0 - h + wx, v = v0 - h + wy;
    float z = DF_OUTSIDE;
    if (u >= 0 && u < a.cols && v >= 0 && v < fa.rows) {
      const float zq = depth_z(reinterpret_cast<const T*>(a.img + (size_t)v * a.pitch) + u, a);
      z = depth_keep(zq, a) ? zq : DF_NOT_KEPT;
    }
    sz[i] = z;
  }
  const double D = (double)((r + 1) * (r + 1));
  for (int i = threadIdx.x; i < side * side; i += DF_BLOCK) {
    const int dv = i / side - r, du = i - (dv + r) * side - r;
    const double s = 1.0 - (double)(du * du + dv * dv) / D;
    tap[i] = s > 0 ? s * s : -1.0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < pw * ph; i += DF_BLOCK) {
    const int wy = i / pw, wx = i - wy * pw;
    const int ci = (wy + 1) * zw + wx + 1;
    const float pz = sz[ci];
    float keep = __builtin_nanf("");
    if (pz > 0.f) {
      const double zp = (double)pz;
      const double S = (double)fa.support_abs + (double)fa.support_quad * (zp * zp);
      int count = 0;
#pragma unroll
      for (int dv = -1; dv <= 1; dv++)
#pragma unroll
        for (int du = -1; du <= 1; du++) {
          if (du == 0 && dv == 0) continue;
          const float qz = sz[ci + dv * zw + du];
          count += (qz == DF_OUTSIDE || (qz > 0.f && ppf_fabs((double)qz - zp) <= S)) ? 1 : 0;
        }
      if (fa.min_support == 0 || count >= fa.min_support) keep = pz;
    }
    ss[i] = keep;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const long long u = u0 + lx, v = v0 + ly;
  const bool inside = u < a.cols && v < fa.rows;
  const bool kept = inside && sz[(ly + h) * zw + lx + h] > 0.f;
  const float pz = ss[(ly + r) * pw + lx + r];
  const bool supported = inside && pz == pz;
  float res = 0.f;
  if (supported) {
    const double zp = (double)pz;
    const double R = (double)fa.range_abs + (double)fa.range_quad * (zp * zp);
    double num = 0.0, den = 0.0;
    /* the window of this lane starts at pixel (ly, lx) of the supported plane; a NaN z gives a NaN k, which fails k > 0 */
    for (int dv = 0; dv < side; dv++) {
      const int rb = (ly + dv) * pw + lx;
      for (int du = 0; du < side; du++) {
        const double s2 = tap[dv * side + du];
        if (s2 < 0) continue; /* uniform */
        const double zq = (double)ss[rb + du];
        const double t = (zq - zp) / R;
        const double k = 1.0 - t * t;
        if (k > 0) {
          const double w = s2 * (k * k);
          num = num + w * zq;
          den = den + w;
        }
      }
    }
    res = (float)(num / den);
  }
  if (inside) out[(size_t)v * (size_t)a.cols + (size_t)u] = res;
  const unsigned long long bk = __ballot(kept), bu = __ballot(kept && !supported);
  if (lx == 0) {
    s_n[ly][DF_C_KEPT] = __popcll(bk);
    s_n[ly][DF_C_UNSUPPORTED] = __popcll(bu);
  }
  __syncthreads();
  if (threadIdx.x < DF_N_COUNTERS) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < DF_TILE_H; w++) n += s_n[w][threadIdx.x];
    if (n) atomicAdd(&fa.counters[threadIdx.x], n);
  }
}

#endif /* PPF_FILTER_KERNELS_H */
