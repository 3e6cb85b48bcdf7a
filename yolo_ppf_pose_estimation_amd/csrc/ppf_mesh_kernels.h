/*
 * ppf_mesh_kernels.h — ppf_cloud_from_mesh: a model cloud sampled from a triangle mesh, without the rows no
 * view can see and with the normals turned outward.  The specification is the comment above the entry in include/ppf_hip.h;
 * the arithmetic that the host shares with the kernels (the hash, a triangle's cross product, its row count) is PPF_HD.
 *
 *   k_mesh_tri         one lane per triangle: L, the degenerate flag, n_k, the box of the live vertices; a wave reduction, then
 *                      one integer atomic per workgroup and bound, and the workgroup's share of the area into its own slot
 *   k_mesh_area        one workgroup: the slots summed in a fixed order
 *   k_mesh_sample      one lane per row: (k, j) by a binary search over the offsets, the point and the normal
 *   k_mesh_draw_small  grid.y the view, one lane per triangle: its clamped box when that is at most 16 x 16 pixels, else the
 *                      (triangle, view) pair appended to a list
 *   k_mesh_draw_large  a fixed grid of workgroups striding over the list, whose length they read on the device: the lanes
 *                      over the box's pixels
 *   k_mesh_visible     one lane per row over the 26 views: the keep flag, the normal negated in place
 *   k_mesh_scatter     the kept rows to their place behind the scan of the flags
 * Integer atomics only (the minimum of a positive float's bit pattern is order-free), no grid-wide wait.
 */
#ifndef PPF_MESH_KERNELS_H
#define PPF_MESH_KERNELS_H

#define MESH_BLOCK 256
#define MESH_SMALL_PX 16      /* a clamped box of at most this many pixels a side is looped by one lane */
#define MESH_LARGE_GRID 1024  /* workgroups of k_mesh_draw_large */
#define MESH_EMPTY 0xffffffffu

/* zeroed before a call; the box as maxima only: [0..2] of the complement of lo's key, [3..5] of hi's key (0: no vertex) */
struct MeshCounters {
  unsigned long long total;      /* sum n_k */
  unsigned long long degenerate;
  double area;
  uint32_t box[6];
  uint32_t over;                 /* a triangle with q >= max_rows */
  uint32_t large;                /* entries of the list */
  uint32_t flipped;
  uint32_t pad;
};

struct MeshViews {
  double d[PPF_MESH_VIEWS][3], a[PPF_MESH_VIEWS][3], b[PPF_MESH_VIEWS][3];
  double ctr[3], r, px, half, tol;
  int R, min_views, orient, pad;
};

struct MeshTri {
  double v0[3], e1[3], e2[3], c[3], L;
  bool ok;
};

PPF_HD uint32_t mesh_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}
PPF_HD uint32_t mesh_hash(uint32_t seed, uint32_t k, uint32_t c) { return mesh_mix(mesh_mix(mesh_mix(seed + 0x9e3779b9u) ^ k) ^ c); }

/* the order-preserving key of a float (-0 below +0) and back */
PPF_HD uint32_t mesh_fkey(float f) {
  uint32_t b;
  __builtin_memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
PPF_HD float mesh_fkey_inv(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

PPF_HD void mesh_tri_geom(const float* __restrict__ vertices, int vstride, const int32_t* __restrict__ tri, MeshTri& t) {
  const float* p0 = vertices + (size_t)tri[0] * vstride;
  const float* p1 = vertices + (size_t)tri[1] * vstride;
  const float* p2 = vertices + (size_t)tri[2] * vstride;
  for (int a = 0; a < 3; a++) {
    t.v0[a] = (double)p0[a];
    t.e1[a] = (double)p1[a] - t.v0[a];
    t.e2[a] = (double)p2[a] - t.v0[a];
  }
  t.c[0] = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
  t.c[1] = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
  t.c[2] = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
  t.L = ppf_sqrt((t.c[0] * t.c[0] + t.c[1] * t.c[1]) + t.c[2] * t.c[2]);
  t.ok = t.L > 0.0 && t.L < __builtin_inf();
}

/* n_k of a live triangle; false: q >= max_rows */
PPF_HD bool mesh_count(double L, double s2, uint32_t seed, uint32_t k, double max_rows, uint32_t* n) {
  const double q = (0.5 * L) / s2;
  if (!(q < max_rows)) return false;
  const double f = __builtin_floor(q);
  const uint32_t thr = (uint32_t)__builtin_floor((q - f) * 16777216.0);
  *n = (uint32_t)f + ((mesh_hash(seed, k, 0u) >> 8) < thr ? 1u : 0u);
  return true;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_tri(const float* __restrict__ vertices, int vstride, const int32_t* __restrict__ tris,
                                                         uint32_t nt, double s2, uint32_t seed, double max_rows, uint32_t* __restrict__ nk,
                                                         uint8_t* __restrict__ live, double* __restrict__ area_part,
                                                         MeshCounters* __restrict__ C) {
  __shared__ unsigned long long s_sum[MESH_BLOCK / 64];
  __shared__ uint32_t s_deg[MESH_BLOCK / 64], s_over[MESH_BLOCK / 64], s_box[MESH_BLOCK / 64][6];
  __shared__ double s_area[MESH_BLOCK / 64];
  const uint32_t k = blockIdx.x * MESH_BLOCK + threadIdx.x;
  uint32_t n = 0, box[6] = {0, 0, 0, 0, 0, 0};
  bool deg = false, over = false;
  double area = 0.0;
  if (k < nt) {
    const int32_t* tri = tris + (size_t)k * 3;
    MeshTri t;
    mesh_tri_geom(vertices, vstride, tri, t);
    deg = !t.ok;
    if (t.ok) {
      area = 0.5 * t.L;
      over = !mesh_count(t.L, s2, seed, k, max_rows, &n);
      for (int c = 0; c < 3; c++) {
        const float* p = vertices + (size_t)tri[c] * vstride;
        for (int a = 0; a < 3; a++) {
          const uint32_t key = mesh_fkey(p[a]);
          box[a] = max(box[a], ~key);
          box[3 + a] = max(box[3 + a], key);
        }
      }
    }
    nk[k] = n;
    live[k] = t.ok ? 1 : 0;
  }
  if (k == 0) nk[nt] = 0; /* the trailing element the scan turns into the total */
  unsigned long long sum = n;
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    area += __shfl_xor(area, o); /* a butterfly: every lane holds the same sum, in an order fixed by the lanes */
#pragma unroll
    for (int a = 0; a < 6; a++) box[a] = max(box[a], (uint32_t)__shfl_xor((int)box[a], o));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t ndeg = (uint32_t)__popcll(__ballot(deg)), nover = (uint32_t)__popcll(__ballot(over));
  if (lane == 0) {
    s_sum[wv] = sum;
    s_deg[wv] = ndeg;
    s_over[wv] = nover;
    s_area[wv] = area;
#pragma unroll
    for (int a = 0; a < 6; a++) s_box[wv][a] = box[a];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    uint32_t d = 0, ov = 0;
    double ar = 0.0;
    for (int w = 0; w < MESH_BLOCK / 64; w++) {
      t += s_sum[w];
      d += s_deg[w];
      ov += s_over[w];
      ar += s_area[w];
    }
    area_part[blockIdx.x] = ar;
    if (t) atomicAdd(&C->total, t);
    if (d) atomicAdd(&C->degenerate, (unsigned long long)d);
    if (ov) atomicOr(&C->over, 1u);
  }
  if (threadIdx.x < 6) {
    uint32_t b = 0;
    for (int w = 0; w < MESH_BLOCK / 64; w++) b = max(b, s_box[w][threadIdx.x]);
    if (b) atomicMax(&C->box[threadIdx.x], b);
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_area(const double* __restrict__ area_part, uint32_t n, MeshCounters* __restrict__ C) {
  __shared__ double s[MESH_BLOCK];
  double a = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += MESH_BLOCK) a += area_part[i];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int o = MESH_BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) C->area = s[0];
}

/* normal_offset < 0: face normals.  curv: NULL when the rows go to the scratch that k_mesh_visible tests */
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_sample(const float* __restrict__ vertices, int vstride, int normal_offset,
                                                            const int32_t* __restrict__ tris, uint32_t nt, const uint32_t* __restrict__ offs,
                                                            uint32_t total, uint32_t seed, float* __restrict__ rows, float* __restrict__ curv) {
  const uint32_t row = blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (row >= total) return;
  uint32_t lo = 0, hi = nt; /* the smallest k with offs[k + 1] > row; offs[nt] = total > row */
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (offs[mid + 1] <= row) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t k = lo, j = row - offs[k];
  const int32_t* tri = tris + (size_t)k * 3;
  MeshTri t;
  mesh_tri_geom(vertices, vstride, tri, t);
  double u = ((double)(mesh_hash(seed, k, 2u * j + 1u) >> 8) + 0.5) / 16777216.0;
  double v = ((double)(mesh_hash(seed, k, 2u * j + 2u) >> 8) + 0.5) / 16777216.0;
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
  float out[6];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    out[a] = (float)((t.v0[a] + u * t.e1[a]) + v * t.e2[a]);
    out[3 + a] = (float)(t.c[a] / t.L);
  }
  if (normal_offset >= 0) {
    const float* n0 = vertices + (size_t)tri[0] * vstride + normal_offset;
    const float* n1 = vertices + (size_t)tri[1] * vstride + normal_offset;
    const float* n2 = vertices + (size_t)tri[2] * vstride + normal_offset;
    const double w = (1.0 - u) - v;
    double m[3];
#pragma unroll
    for (int a = 0; a < 3; a++) m[a] = (w * (double)n0[a] + u * (double)n1[a]) + v * (double)n2[a];
    const double l = ppf_sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (l > 0.0 && l < __builtin_inf()) {
#pragma unroll
      for (int a = 0; a < 3; a++) out[3 + a] = (float)(m[a] / l);
    }
  }
  float2* dst = reinterpret_cast<float2*>(rows + (size_t)row * 6);
  dst[0] = make_float2(out[0], out[1]);
  dst[1] = make_float2(out[2], out[3]);
  dst[2] = make_float2(out[4], out[5]);
  if (curv) curv[row] = 0.f;
}

__device__ __forceinline__ void mesh_project(const MeshViews* __restrict__ W, int v, double x, double y, double z, double* X, double* Y,
                                             double* D) {
  const double sx = x - W->ctr[0], sy = y - W->ctr[1], sz = z - W->ctr[2];
  *X = ((sx * W->a[v][0] + sy * W->a[v][1]) + sz * W->a[v][2]) / W->px + W->half;
  *Y = ((sx * W->b[v][0] + sy * W->b[v][1]) + sz * W->b[v][2]) / W->px + W->half;
  *D = ((sx * W->d[v][0] + sy * W->d[v][1]) + sz * W->d[v][2]) + W->r;
}

/* a triangle in a view: its vertices' map coordinates and float depths, its clamped box (empty: i1 < i0) and area2 */
struct MeshProj {
  double ax, ay, bx, by, cx, cy, area;
  float az, bz, cz;
  int i0, i1, j0, j1;
};

__device__ __forceinline__ void mesh_tri_project(const float* __restrict__ vertices, int vstride, const int32_t* __restrict__ tri,
                                                 const MeshViews* __restrict__ W, int v, MeshProj& P) {
  const float* p0 = vertices + (size_t)tri[0] * vstride;
  const float* p1 = vertices + (size_t)tri[1] * vstride;
  const float* p2 = vertices + (size_t)tri[2] * vstride;
  double D;
  mesh_project(W, v, (double)p0[0], (double)p0[1], (double)p0[2], &P.ax, &P.ay, &D);
  P.az = (float)D;
  mesh_project(W, v, (double)p1[0], (double)p1[1], (double)p1[2], &P.bx, &P.by, &D);
  P.bz = (float)D;
  mesh_project(W, v, (double)p2[0], (double)p2[1], (double)p2[2], &P.cx, &P.cy, &D);
  P.cz = (float)D;
  double x0 = P.ax < P.bx ? P.ax : P.bx, x1 = P.ax > P.bx ? P.ax : P.bx, y0 = P.ay < P.by ? P.ay : P.by, y1 = P.ay > P.by ? P.ay : P.by;
  x0 = ceil(x0 < P.cx ? x0 : P.cx);
  x1 = floor(x1 > P.cx ? x1 : P.cx);
  y0 = ceil(y0 < P.cy ? y0 : P.cy);
  y1 = floor(y1 > P.cy ? y1 : P.cy);
  /* clamped to the map as doubles: the conversions to int cannot overflow */
  const double last = (double)(W->R - 1);
  x0 = x0 < 0.0 ? 0.0 : x0;
  y0 = y0 < 0.0 ? 0.0 : y0;
  x1 = x1 > last ? last : x1;
  y1 = y1 > last ? last : y1;
  P.area = (P.bx - P.ax) * (P.cy - P.ay) - (P.by - P.ay) * (P.cx - P.ax);
  if (!(x1 >= x0 && y1 >= y0) || !(P.area != 0.0)) { /* also a NaN coordinate */
    P.i0 = P.j0 = 0;
    P.i1 = P.j1 = -1;
    return;
  }
  P.i0 = (int)x0;
  P.i1 = (int)x1;
  P.j0 = (int)y0;
  P.j1 = (int)y1;
}

/* pixel (i, j) of the map, inside it by the clamped box */
__device__ __forceinline__ void mesh_pixel(const MeshProj& P, int i, int j, uint32_t* __restrict__ map, int R) {
  const double px = (double)i, py = (double)j;
  const double w0 = (P.cx - P.bx) * (py - P.by) - (P.cy - P.by) * (px - P.bx);
  const double w1 = (P.ax - P.cx) * (py - P.cy) - (P.ay - P.cy) * (px - P.cx);
  const double w2 = (P.bx - P.ax) * (py - P.ay) - (P.by - P.ay) * (px - P.ax);
  if ((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0)) {
    const float z = (float)(((w0 * (double)P.az + w1 * (double)P.bz) + w2 * (double)P.cz) / P.area);
    atomicMin(&map[(size_t)j * R + i], __float_as_uint(z > 0.f ? z : 0.f));
  }
}

/* grid: (triangles / MESH_BLOCK, views); list holds 26 nt entries, k * 26 + v each */
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_draw_small(const float* __restrict__ vertices, int vstride, const int32_t* __restrict__ tris,
                                                                uint32_t nt, const uint8_t* __restrict__ live,
                                                                const MeshViews* __restrict__ W, uint32_t* __restrict__ maps,
                                                                uint32_t* __restrict__ list, MeshCounters* __restrict__ C) {
  const uint32_t k = blockIdx.x * MESH_BLOCK + threadIdx.x;
  const int v = (int)blockIdx.y;
  if (k >= nt || !live[k]) return;
  MeshProj P;
  mesh_tri_project(vertices, vstride, tris + (size_t)k * 3, W, v, P);
  if (P.i1 < P.i0) return;
  if (P.i1 - P.i0 >= MESH_SMALL_PX || P.j1 - P.j0 >= MESH_SMALL_PX) {
    list[atomicAdd(&C->large, 1u)] = k * (uint32_t)PPF_MESH_VIEWS + (uint32_t)v;
    return;
  }
  const int R = W->R;
  uint32_t* map = maps + (size_t)v * R * R;
  for (int j = P.j0; j <= P.j1; j++)
    for (int i = P.i0; i <= P.i1; i++) mesh_pixel(P, i, j, map, R);
}

/* grid: MESH_LARGE_GRID workgroups over the C->large entries the launch before appended */
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_draw_large(const float* __restrict__ vertices, int vstride, const int32_t* __restrict__ tris,
                                                                const MeshViews* __restrict__ W, uint32_t* __restrict__ maps,
                                                                const uint32_t* __restrict__ list, const MeshCounters* __restrict__ C) {
  const uint32_t n = C->large;
  const int R = W->R;
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint32_t ent = list[e], k = ent / (uint32_t)PPF_MESH_VIEWS;
    const int v = (int)(ent - k * (uint32_t)PPF_MESH_VIEWS);
    MeshProj P;
    mesh_tri_project(vertices, vstride, tris + (size_t)k * 3, W, v, P);
    if (P.i1 < P.i0) continue;
    uint32_t* map = maps + (size_t)v * R * R;
    const int w = P.i1 - P.i0 + 1, npx = w * (P.j1 - P.j0 + 1); /* at most 1024 x 1024 */
    for (int p = threadIdx.x; p < npx; p += MESH_BLOCK) {
      const int dj = p / w;
      mesh_pixel(P, P.i0 + (p - dj * w), P.j0 + dj, map, R);
    }
  }
}

/* keep: total + 1 flags (the last 0, for the scan's total); a flipped row's normal is negated in rows */
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_visible(float* __restrict__ rows, uint32_t total, const MeshViews* __restrict__ W,
                                                             const uint32_t* __restrict__ maps, uint32_t* __restrict__ keep,
                                                             MeshCounters* __restrict__ C) {
  const uint32_t row = blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (row == 0) keep[total] = 0;
  bool flip = false;
  if (row < total) {
    float2* src = reinterpret_cast<float2*>(rows + (size_t)row * 6);
    const float2 r0 = src[0], r1 = src[1], r2 = src[2];
    const double x = (double)r0.x, y = (double)r0.y, z = (double)r1.x, nx = (double)r1.y, ny = (double)r2.x, nz = (double)r2.y;
    const int R = W->R;
    const double last = (double)(R - 1);
    int seen = 0, front = 0, back = 0;
    for (int v = 0; v < PPF_MESH_VIEWS; v++) {
      double X, Y, D;
      mesh_project(W, v, x, y, z, &X, &Y, &D);
      const double fi = floor(X + 0.5), fj = floor(Y + 0.5);
      bool vis = true;
      if (fi >= 0.0 && fi <= last && fj >= 0.0 && fj <= last) {
        const uint32_t zb = maps[((size_t)v * R + (size_t)(int)fj) * R + (size_t)(int)fi];
        vis = zb == MESH_EMPTY || (double)(float)D <= (double)__uint_as_float(zb) + W->tol;
      }
      if (vis) {
        const double s = (nx * W->d[v][0] + ny * W->d[v][1]) + nz * W->d[v][2];
        seen++;
        front += s < 0.0;
        back += s > 0.0;
      }
    }
    const bool kept = seen >= W->min_views;
    flip = kept && W->orient && back > front;
    if (flip) {
      src[1] = make_float2(r1.x, -r1.y);
      src[2] = make_float2(-r2.x, -r2.y);
    }
    keep[row] = kept ? 1u : 0u;
  }
  const unsigned long long m = __ballot(flip);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&C->flipped, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_scatter(const float* __restrict__ rows, uint32_t total, const uint32_t* __restrict__ keep,
                                                             const uint32_t* __restrict__ pos, float* __restrict__ out,
                                                             float* __restrict__ curv) {
  const uint32_t row = blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (row >= total || !keep[row]) return;
  const uint32_t o = pos[row];
  const float2* src = reinterpret_cast<const float2*>(rows + (size_t)row * 6);
  float2* dst = reinterpret_cast<float2*>(out + (size_t)o * 6);
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
  curv[o] = 0.f;
}

#endif /* PPF_MESH_KERNELS_H */
