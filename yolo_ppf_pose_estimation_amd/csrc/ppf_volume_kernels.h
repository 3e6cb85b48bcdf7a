/*
 * ppf_volume_kernels.h — posed depth images fused into a truncated signed distance volume on gfx950 (ppf_depth_volume,
 * DESIGN.md §30).  Included by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_z, depth_keep); host side:
 * ppf_volume_host.h.  The volume is nx * ny * nz records {float d; int32_t w}, x fastest: (k * ny + j) * nx + i.
 *
 *   k_volume_fill       every record to {1.0f, 0}: one lane per pair of records.
 *   k_volume_integrate  one lane per pair of x-neighbours (i = 2 * ip, 2 * ip + 1), 64 lanes per workgroup.  Where nx is even
 *                       a lane's pair is one aligned 16-byte load and, when either voxel was updated, one 16-byte store (a
 *                       skipped voxel of an updated pair is stored with the bytes it was loaded with); where nx is odd every
 *                       record is an 8-byte access and the last column's lane has one voxel.  The pixel a voxel falls on is
 *                       read through the row pitch.  No LDS, no scratch; no workgroup returns early: there is no brick
 *                       test.  n_updated is two ballots per wave and one 64-bit integer atomicAdd per workgroup.
 *   k_volume_raycast    one lane per pixel in 16 x 16 tiles (a wave is 16 x 4 pixels, so its rays stay close in the volume).
 *                       The walk reads one record per step (near); the 16 records of the two tri samples are read only at
 *                       the hit, the 48 of the normal only with a normals image.  n_hits and n_interpolated are ballots,
 *                       summed over the workgroup's four waves in LDS: one integer atomicAdd each per workgroup.
 *   k_volume_cross<0>   flag and count: one lane per voxel in tiles of 256 consecutive voxels; a lane finds which of its three
 *                       crossings (x, y, z) give a row; the tile's row count -> counts[tile], the crossings -> one counter.
 *   k_volume_cross<1>   after the exclusive scan of the tile counts: the same flags again; a row's place is the tile's
 *                       offset + the waves before + the rows of the lanes below (mbcnt of the three ballots) + the lane's
 *                       earlier axes: (linear voxel index, axis) order, no atomic decides a place.
 * Everything is fp64 as written, left to right, nothing fused (-ffp-contract=off); no float atomic, no inline assembly, no
 * grid-wide synchronisation.
 */
#ifndef PPF_VOLUME_KERNELS_H
#define PPF_VOLUME_KERNELS_H

constexpr int DV_BLOCK = 64;    /* k_volume_integrate: one wave, so the count needs no LDS */
constexpr int DV_TILE = 16;     /* k_volume_raycast: pixels per tile edge */
constexpr int DV_RAY_BLOCK = DV_TILE * DV_TILE;
constexpr int DV_X_BLOCK = 256; /* k_volume_cross: voxels per tile */

struct VolVoxel {
  float d;
  int32_t w;
};
static_assert(sizeof(VolVoxel) == 8 && sizeof(VolVoxel) == sizeof(ppf_depth_volume_voxel), "the record is 8 bytes");

struct VolArgs {
  VolVoxel* vox;
  int nx, ny, nz;
  double voxel, trunc; /* (double) of the floats */
  double o[3];
};

struct VolPose {
  double T[16];
};

struct VolRay {
  int rows, cols, tiles_x;
  double fx, fy, ppx, ppy;
  double R[9], c[3]; /* the pose's rotation; the camera centre in world coordinates */
  double z_near, step;
  int K, min_weight;
  float* depth;   /* packed rows x cols */
  float* normals; /* packed rows x cols x 3, or nullptr */
  int32_t* counters; /* n_hits, n_interpolated: preset to 0 */
};

__global__ __launch_bounds__(256) void k_volume_fill(VolVoxel* __restrict__ vox, size_t n) {
  const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2; /* the buffer starts on a 16-byte boundary */
  if (p + 1 < n)
    *reinterpret_cast<float4*>(vox + p) = make_float4(1.0f, 0.f, 1.0f, 0.f); /* w = 0 has the bits of 0.0f */
  else if (p < n)
    vox[p] = VolVoxel{1.0f, 0};
}

/* steps 1 to 6 of the integration for voxel (i, j, k) holding r; true: r was updated */
template <class T>
__device__ __forceinline__ bool volume_update(const DepthArgs& a, const VolArgs& V, const VolPose& P, int rows, int max_weight, int i,
                                              double P1, double P2, VolVoxel* r) {
  const double P0 = V.o[0] + (double)i * V.voxel;
  const double p0 = ((P.T[0] * P0 + P.T[1] * P1) + P.T[2] * P2) + P.T[3];
  const double p1 = ((P.T[4] * P0 + P.T[5] * P1) + P.T[6] * P2) + P.T[7];
  const double p2 = ((P.T[8] * P0 + P.T[9] * P1) + P.T[10] * P2) + P.T[11];
  if (!(p2 > 0.0)) return false;
  const double uf = __builtin_floor((p0 * a.fx / p2 + a.ppx) + 0.5), vf = __builtin_floor((p1 * a.fy / p2 + a.ppy) + 0.5);
  if (!(uf >= 0.0 && uf < (double)a.cols && vf >= 0.0 && vf < (double)rows)) return false; /* NaN fails here */
  const int ui = (int)uf, vi = (int)vf;
  const float z = depth_z(reinterpret_cast<const T*>(a.img + (size_t)vi * a.pitch) + ui, a);
  if (!depth_keep(z, a)) return false;
  const double sdf = (double)z - p2;
  if (sdf < -V.trunc) return false;
  double dn = sdf / V.trunc;
  if (dn > 1.0) dn = 1.0;
  r->d = (float)(((double)r->d * (double)r->w + dn) / (double)(r->w + 1));
  r->w = r->w + 1 < max_weight ? r->w + 1 : max_weight;
  return true;
}

template <class T>
__global__ __launch_bounds__(DV_BLOCK) void k_volume_integrate(DepthArgs a, VolArgs V, VolPose P, int rows, int max_weight, int pairs_x,
                                                               int vec, unsigned long long* __restrict__ n_updated) {
  const long long g = (long long)blockIdx.x * DV_BLOCK + threadIdx.x;
  const long long per_slice = (long long)pairs_x * V.ny;
  bool up0 = false, up1 = false;
  if (g < per_slice * V.nz) {
    const int k = (int)(g / per_slice);
    const int rem = (int)(g - (long long)k * per_slice);
    const int j = rem / pairs_x, i = (rem - j * pairs_x) * 2;
    const bool two = i + 1 < V.nx;
    const double P1 = V.o[1] + (double)j * V.voxel, P2 = V.o[2] + (double)k * V.voxel;
    VolVoxel* at = V.vox + ((size_t)k * V.ny + j) * V.nx + i;
    VolVoxel r0, r1 = VolVoxel{1.0f, 0};
    if (vec) { /* nx is even: two is true and `at` is 16-byte aligned */
      const float4 q = *reinterpret_cast<const float4*>(at);
      r0 = VolVoxel{q.x, (int32_t)__float_as_uint(q.y)};
      r1 = VolVoxel{q.z, (int32_t)__float_as_uint(q.w)};
    } else {
      r0 = at[0];
      if (two) r1 = at[1];
    }
    up0 = volume_update<T>(a, V, P, rows, max_weight, i, P1, P2, &r0);
    if (two) up1 = volume_update<T>(a, V, P, rows, max_weight, i + 1, P1, P2, &r1);
    if (vec) {
      if (up0 || up1)
        *reinterpret_cast<float4*>(at) = make_float4(r0.d, __uint_as_float((uint32_t)r0.w), r1.d, __uint_as_float((uint32_t)r1.w));
    } else {
      if (up0) at[0] = r0;
      if (up1) at[1] = r1;
    }
  }
  const int n = __popcll(__ballot(up0)) + __popcll(__ballot(up1));
  if (threadIdx.x == 0 && n) atomicAdd(n_updated, (unsigned long long)n);
}

/* near(P): false is "none" */
__device__ __forceinline__ bool volume_near(const VolArgs& V, int min_weight, double P0, double P1, double P2, double* d) {
  const double x = __builtin_floor((P0 - V.o[0]) / V.voxel + 0.5), y = __builtin_floor((P1 - V.o[1]) / V.voxel + 0.5),
               z = __builtin_floor((P2 - V.o[2]) / V.voxel + 0.5);
  if (!(x >= 0.0 && x < (double)V.nx && y >= 0.0 && y < (double)V.ny && z >= 0.0 && z < (double)V.nz)) return false;
  const VolVoxel r = V.vox[((size_t)(int)z * V.ny + (int)y) * V.nx + (int)x];
  if (r.w < min_weight) return false;
  *d = (double)r.d;
  return true;
}

/* tri(P): false is "none" */
__device__ __forceinline__ bool volume_tri(const VolArgs& V, int min_weight, double P0, double P1, double P2, double* d) {
  const double g0 = (P0 - V.o[0]) / V.voxel, g1 = (P1 - V.o[1]) / V.voxel, g2 = (P2 - V.o[2]) / V.voxel;
  const double b0 = __builtin_floor(g0), b1 = __builtin_floor(g1), b2 = __builtin_floor(g2);
  if (!(b0 >= 0.0 && b0 + 1.0 < (double)V.nx && b1 >= 0.0 && b1 + 1.0 < (double)V.ny && b2 >= 0.0 && b2 + 1.0 < (double)V.nz)) return false;
  const double f0 = g0 - b0, f1 = g1 - b1, f2 = g2 - b2;
  const VolVoxel* at = V.vox + ((size_t)(int)b2 * V.ny + (int)b1) * V.nx + (int)b0;
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * V.ny;
  const VolVoxel c000 = at[0], c100 = at[1], c010 = at[sy], c110 = at[sy + 1];
  const VolVoxel c001 = at[sz], c101 = at[sz + 1], c011 = at[sz + sy], c111 = at[sz + sy + 1];
  if (c000.w < min_weight || c100.w < min_weight || c010.w < min_weight || c110.w < min_weight || c001.w < min_weight ||
      c101.w < min_weight || c011.w < min_weight || c111.w < min_weight)
    return false;
  const double x00 = (double)c000.d + f0 * ((double)c100.d - (double)c000.d);
  const double x10 = (double)c010.d + f0 * ((double)c110.d - (double)c010.d);
  const double x01 = (double)c001.d + f0 * ((double)c101.d - (double)c001.d);
  const double x11 = (double)c011.d + f0 * ((double)c111.d - (double)c011.d);
  const double y0 = x00 + f1 * (x10 - x00);
  const double y1 = x01 + f1 * (x11 - x01);
  *d = y0 + f2 * (y1 - y0);
  return true;
}

__global__ __launch_bounds__(DV_RAY_BLOCK) void k_volume_raycast(VolArgs V, VolRay Q) {
  __shared__ int s_n[DV_RAY_BLOCK / 64][2];
  const int ty = (int)blockIdx.x / Q.tiles_x, tx = (int)blockIdx.x - ty * Q.tiles_x;
  const int u = tx * DV_TILE + ((int)threadIdx.x & (DV_TILE - 1)), v = ty * DV_TILE + ((int)threadIdx.x >> 4);
  const bool active = u < Q.cols && v < Q.rows;
  bool hit = false, interp = false;
  if (active) {
    const double dc0 = ((double)u - Q.ppx) / Q.fx, dc1 = ((double)v - Q.ppy) / Q.fy;
    const double dw0 = (Q.R[0] * dc0 + Q.R[3] * dc1) + Q.R[6] * 1.0;
    const double dw1 = (Q.R[1] * dc0 + Q.R[4] * dc1) + Q.R[7] * 1.0;
    const double dw2 = (Q.R[2] * dc0 + Q.R[5] * dc1) + Q.R[8] * 1.0;
    bool prev_front = false;
    double fp = 0.0, fk = 0.0;
    int kb = -1;
    for (int k = 0; k < Q.K; k++) {
      const double s = Q.z_near + (double)k * Q.step;
      double d = 0.0;
      const bool some = volume_near(V, Q.min_weight, Q.c[0] + s * dw0, Q.c[1] + s * dw1, Q.c[2] + s * dw2, &d);
      if (some && !(d > 0.0)) { /* the first back sample ends the walk */
        kb = k;
        fk = d;
        break;
      }
      prev_front = some;
      fp = d;
    }
    float depth = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (kb >= 1 && prev_front) {
      hit = true;
      const double s0 = Q.z_near + (double)(kb - 1) * Q.step, s1 = Q.z_near + (double)kb * Q.step;
      double a0, a1;
      const bool h0 = volume_tri(V, Q.min_weight, Q.c[0] + s0 * dw0, Q.c[1] + s0 * dw1, Q.c[2] + s0 * dw2, &a0);
      const bool h1 = volume_tri(V, Q.min_weight, Q.c[0] + s1 * dw0, Q.c[1] + s1 * dw1, Q.c[2] + s1 * dw2, &a1);
      double f0 = fp, f1 = fk;
      if (h0 && h1 && a0 > 0.0 && 0.0 >= a1) {
        f0 = a0;
        f1 = a1;
        interp = true;
      }
      const double ss = s0 + Q.step * f0 / (f0 - f1);
      depth = (float)ss;
      if (Q.normals) {
        const double X0 = Q.c[0] + ss * dw0, X1 = Q.c[1] + ss * dw1, X2 = Q.c[2] + ss * dw2;
        double hi, lo, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        bool ok = volume_tri(V, Q.min_weight, X0 + V.voxel, X1, X2, &hi) && volume_tri(V, Q.min_weight, X0 - V.voxel, X1, X2, &lo);
        if (ok) g0 = hi - lo;
        ok = ok && volume_tri(V, Q.min_weight, X0, X1 + V.voxel, X2, &hi) && volume_tri(V, Q.min_weight, X0, X1 - V.voxel, X2, &lo);
        if (ok) g1 = hi - lo;
        ok = ok && volume_tri(V, Q.min_weight, X0, X1, X2 + V.voxel, &hi) && volume_tri(V, Q.min_weight, X0, X1, X2 - V.voxel, &lo);
        if (ok) g2 = hi - lo;
        const double len = ppf_sqrt((g0 * g0 + g1 * g1) + g2 * g2);
        if (ok && len > 0.0) {
          const double w0 = g0 / len, w1 = g1 / len, w2 = g2 / len;
          n0 = (float)((Q.R[0] * w0 + Q.R[1] * w1) + Q.R[2] * w2);
          n1 = (float)((Q.R[3] * w0 + Q.R[4] * w1) + Q.R[5] * w2);
          n2 = (float)((Q.R[6] * w0 + Q.R[7] * w1) + Q.R[8] * w2);
        }
      }
    }
    const size_t p = (size_t)v * Q.cols + u;
    Q.depth[p] = depth;
    if (Q.normals) {
      Q.normals[p * 3] = n0;
      Q.normals[p * 3 + 1] = n1;
      Q.normals[p * 3 + 2] = n2;
    }
  }
  const int nh = __popcll(__ballot(hit)), ni = __popcll(__ballot(interp));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    s_n[wv][0] = nh;
    s_n[wv][1] = ni;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < DV_RAY_BLOCK / 64; w++) t += s_n[w][threadIdx.x];
    if (t) atomicAdd(&Q.counters[threadIdx.x], t);
  }
}

/* the gradient at lattice voxel (i, j, k), which is inside the volume: false when a neighbour is outside or below min_weight */
__device__ __forceinline__ bool volume_gradient(const VolArgs& V, int min_weight, int i, int j, int k, double* g) {
  if (i < 1 || i + 1 >= V.nx || j < 1 || j + 1 >= V.ny || k < 1 || k + 1 >= V.nz) return false;
  const VolVoxel* at = V.vox + ((size_t)k * V.ny + j) * V.nx + i;
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * V.ny;
  const VolVoxel xh = at[1], xl = *(at - 1), yh = at[sy], yl = *(at - sy), zh = at[sz], zl = *(at - sz);
  if (xh.w < min_weight || xl.w < min_weight || yh.w < min_weight || yl.w < min_weight || zh.w < min_weight || zl.w < min_weight) return false;
  g[0] = (double)xh.d - (double)xl.d;
  g[1] = (double)yh.d - (double)yl.d;
  g[2] = (double)zh.d - (double)zl.d;
  return true;
}

/* the crossing between voxel (i, j, k) holding r0 and its neighbour one step along `axis`: 0 none, 1 a crossing without a
 * row, 3 a crossing with the row written to row[0..5] */
__device__ __forceinline__ int volume_crossing(const VolArgs& V, int min_weight, int i, int j, int k, const VolVoxel& r0, int axis,
                                               float* row) {
  const int mi = i + (axis == 0), mj = j + (axis == 1), mk = k + (axis == 2);
  if (mi >= V.nx || mj >= V.ny || mk >= V.nz) return 0;
  const VolVoxel r1 = V.vox[((size_t)mk * V.ny + mj) * V.nx + mi];
  if (r0.w < min_weight || r1.w < min_weight) return 0;
  const double d0 = (double)r0.d, d1 = (double)r1.d;
  if (!(ppf_fabs(d0) < 1.0 && ppf_fabs(d1) < 1.0)) return 0;
  if ((d0 > 0.0) == (d1 > 0.0)) return 0;
  double ga[3], gb[3];
  if (!volume_gradient(V, min_weight, i, j, k, ga) || !volume_gradient(V, min_weight, mi, mj, mk, gb)) return 1;
  const double t = d0 / (d0 - d1);
  const double g0 = ga[0] + t * (gb[0] - ga[0]), g1 = ga[1] + t * (gb[1] - ga[1]), g2 = ga[2] + t * (gb[2] - ga[2]);
  const double len = ppf_sqrt((g0 * g0 + g1 * g1) + g2 * g2);
  if (!(len > 0.0)) return 1;
  const double c0 = V.o[0] + (double)i * V.voxel, c1 = V.o[1] + (double)j * V.voxel, c2 = V.o[2] + (double)k * V.voxel;
  const double m = t * V.voxel;
  row[0] = (float)(axis == 0 ? c0 + m : c0);
  row[1] = (float)(axis == 1 ? c1 + m : c1);
  row[2] = (float)(axis == 2 ? c2 + m : c2);
  row[3] = (float)(g0 / len);
  row[4] = (float)(g1 / len);
  row[5] = (float)(g2 / len);
  return 3;
}

/* WRITE 0: counts[tile] = the tile's rows (and counts[n_tiles] = 0 for the scan's total), crossings added to *n_cross;
 * WRITE 1: the rows written at tile_off[tile] + their rank inside the tile */
template <int WRITE>
__global__ __launch_bounds__(DV_X_BLOCK) void k_volume_cross(VolArgs V, int min_weight, size_t n_vox, uint32_t n_tiles,
                                                             uint32_t* __restrict__ counts, unsigned long long* __restrict__ n_cross,
                                                             const uint32_t* __restrict__ tile_off, float* __restrict__ rows,
                                                             float* __restrict__ curv) {
  __shared__ uint32_t s_rows[DV_X_BLOCK / 64], s_cross[DV_X_BLOCK / 64];
  const size_t p = (size_t)blockIdx.x * DV_X_BLOCK + threadIdx.x;
  int res[3] = {0, 0, 0};
  float row[3][6];
  if (p < n_vox) {
    const size_t slice = (size_t)V.nx * V.ny;
    const int k = (int)(p / slice);
    const int rem = (int)(p - (size_t)k * slice);
    const int j = rem / V.nx, i = rem - j * V.nx;
    const VolVoxel r0 = V.vox[p];
#pragma unroll
    for (int axis = 0; axis < 3; axis++) res[axis] = volume_crossing(V, min_weight, i, j, k, r0, axis, row[axis]);
  }
  const unsigned long long m0 = __ballot(res[0] == 3), m1 = __ballot(res[1] == 3), m2 = __ballot(res[2] == 3);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_rows[wv] = (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2));
  if (WRITE == 0) {
    const int nc = __popcll(__ballot(res[0] != 0)) + __popcll(__ballot(res[1] != 0)) + __popcll(__ballot(res[2] != 0));
    if (lane == 0) s_cross[wv] = (uint32_t)nc;
  }
  __syncthreads();
  if (WRITE == 0) {
    if (threadIdx.x == 0) {
      uint32_t t = 0, c = 0;
#pragma unroll
      for (int w = 0; w < DV_X_BLOCK / 64; w++) {
        t += s_rows[w];
        c += s_cross[w];
      }
      counts[blockIdx.x] = t;
      if (blockIdx.x == 0) counts[n_tiles] = 0; /* the trailing element the scan turns into the total */
      if (c) atomicAdd(n_cross, (unsigned long long)c);
    }
  } else {
    uint32_t o = tile_off[blockIdx.x];
#pragma unroll
    for (int w = 0; w < DV_X_BLOCK / 64; w++)
      if (w < wv) o += s_rows[w];
    o += __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
    o += __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
    o += __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
#pragma unroll
    for (int axis = 0; axis < 3; axis++)
      if (res[axis] == 3) {
        float* dst = rows + (size_t)o * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) dst[c] = row[axis][c];
        curv[o] = 0.f;
        o++;
      }
  }
}

#endif /* PPF_VOLUME_KERNELS_H */
