/*
 * ppf_render_kernels.h — surfel z-buffers of posed model clouds on gfx950: the visibility test of
 * ppf_verify_frame_rendered and the depth / instance-label images of ppf_render_frame.  Included by ppf_hip.hip after
 * ppf_verify_kernels.h; the host side is ppf_render_host.h.
 *
 * A rendered row (finite, z > 0) is a disk of radius r in its tangent plane.  Its candidate pixels are the
 * (2 rx + 1) x (2 ry + 1) pixels around its centre pixel, clipped to the image; a candidate is covered when its ray meets
 * the disk, at the depth of that intersection (rnd_cover, all in fp64).  A pixel keeps the least depth of its covers:
 * positive floats order like their u32 bits, so an integer atomicMin gives the same bits whatever the schedule.
 *   k_rnd_window     per job the rectangle of its rows' candidate pixels (block reduction, four int atomicMax per block)
 *   k_rnd_splat      one thread per (job, model row): u32 atomicMin of the depth bits into the job's own window
 *   k_rnd_vfy_score  k_vfy_score with the visibility test (vfy_score_rows<true>): a considered row must also be visible
 *                    in its own pose's render
 *   k_rnd_splat_frame  one thread per (chosen pose, model row): u64 atomicMin of (depth bits << 32 | detection) into
 *                    one frame-wide buffer
 *   k_rnd_resolve    the frame buffer -> depth (0 where empty) and label (-1 where empty)
 * No float atomics anywhere.
 */
#ifndef PPF_RENDER_KERNELS_H
#define PPF_RENDER_KERNELS_H

constexpr int RND_BLOCK = 256;
constexpr uint32_t RND_EMPTY = 0xffffffffu;         /* an empty pixel of a job's window */
constexpr unsigned long long RND_EMPTY64 = ~0ull;  /* an empty pixel of the frame buffer */

struct RndCam {
  int rows, cols;
  double fx, fy, ppx, ppy;
  double r;  /* splat_radius */
  float tol; /* visible_tol */
};

struct RndJob {
  double T[16];
  const float* model; /* n x 6: every row is rendered */
  int n;
  int label; /* ppf_render_frame: the detection index */
};

/* a job's window: pixels u0 .. u0 + w - 1, v0 .. v0 + h - 1, stored row-major from off */
struct RndWin {
  int u0, v0, w, h;
  unsigned long long off;
};

/* the clipped candidate rectangle of a moved row: false when it is not rendered or none of its pixels is in the image */
__device__ __forceinline__ bool rnd_rect(const float* o, const RndCam& c, int* ulo, int* uhi, int* vlo, int* vhi) {
  if (!(vfy_finite6(o) && o[2] > 0.f)) return false;
  const double ui = floor((double)o[0] * c.fx / (double)o[2] + c.ppx + 0.5);
  const double vi = floor((double)o[1] * c.fy / (double)o[2] + c.ppy + 0.5);
  double rx = ceil(c.r * c.fx / (double)o[2]), ry = ceil(c.r * c.fy / (double)o[2]);
  rx = rx < (double)PPF_RENDER_MAX_SPLAT ? rx : (double)PPF_RENDER_MAX_SPLAT;
  ry = ry < (double)PPF_RENDER_MAX_SPLAT ? ry : (double)PPF_RENDER_MAX_SPLAT;
  double a = ui - rx, b = ui + rx, e = vi - ry, f = vi + ry;
  a = a > 0.0 ? a : 0.0;
  e = e > 0.0 ? e : 0.0;
  b = b < (double)(c.cols - 1) ? b : (double)(c.cols - 1);
  f = f < (double)(c.rows - 1) ? f : (double)(c.rows - 1);
  if (!(a <= b && e <= f)) return false; /* every bound is now in [0, cols) / [0, rows): safe to convert */
  *ulo = (int)a;
  *uhi = (int)b;
  *vlo = (int)e;
  *vhi = (int)f;
  return true;
}

/* whether pixel (u, v) is covered by the disk of the moved row o (npd = n.p in fp64), and at which depth */
__device__ __forceinline__ bool rnd_cover(const float* o, double npd, int u, int v, const RndCam& c, float* depth) {
  const double dx = ((double)u - c.ppx) / c.fx, dy = ((double)v - c.ppy) / c.fy;
  const double den = (double)o[3] * dx + (double)o[4] * dy + (double)o[5];
  if (den == 0.0) return false;
  const double t = npd / den;
  if (!(isfinite(t) && t > 0.0)) return false;
  const double ex = t * dx - (double)o[0], ey = t * dy - (double)o[1], ez = t - (double)o[2];
  if (!(ex * ex + ey * ey + ez * ez <= c.r * c.r)) return false;
  *depth = (float)t;
  return true;
}

__device__ __forceinline__ double rnd_npd(const float* o) {
  return (double)o[3] * (double)o[0] + (double)o[4] * (double)o[1] + (double)o[5] * (double)o[2];
}

__device__ __forceinline__ void rnd_move(const RndJob& J, int r, float* o) {
  double M[16];
#pragma unroll
  for (int k = 0; k < 16; k++) M[k] = J.T[k];
  const float* p = J.model + (size_t)r * 6;
  icp_transform_row(p, p + 3, M, o);
}

/* grid (blocks of the largest model) x jobs; box[4 job + k] = {-u0, -v0, u1, v1}, preset to 0x80808080 (below any) */
__global__ __launch_bounds__(RND_BLOCK) void k_rnd_window(const RndJob* __restrict__ jobs, RndCam c, int* __restrict__ box) {
  __shared__ int ws[RND_BLOCK / 64][4];
  const RndJob& J = jobs[blockIdx.y];
  if ((int)blockIdx.x * RND_BLOCK >= J.n) return; /* uniform per block */
  const int r = blockIdx.x * RND_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int m[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN};
  if (r < J.n) {
    float o[6];
    rnd_move(J, r, o);
    int ulo, uhi, vlo, vhi;
    if (rnd_rect(o, c, &ulo, &uhi, &vlo, &vhi)) {
      m[0] = -ulo;
      m[1] = -vlo;
      m[2] = uhi;
      m[3] = vhi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = max(m[k], __shfl_xor(m[k], off));
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 4; k++) ws[wv][k] = m[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    int v = ws[0][threadIdx.x];
    for (int w = 1; w < RND_BLOCK / 64; w++) v = max(v, ws[w][threadIdx.x]);
    if (v != INT_MIN) atomicMax(&box[(size_t)blockIdx.y * 4 + threadIdx.x], v);
  }
}

/* grid (blocks of the largest model) x jobs: every rendered row's covers into its job's window */
__global__ __launch_bounds__(RND_BLOCK) void k_rnd_splat(const RndJob* __restrict__ jobs, const RndWin* __restrict__ wins, RndCam c,
                                                         uint32_t* __restrict__ zbuf) {
  const RndJob& J = jobs[blockIdx.y];
  const int r = blockIdx.x * RND_BLOCK + threadIdx.x;
  if (r >= J.n) return;
  float o[6];
  rnd_move(J, r, o);
  int ulo, uhi, vlo, vhi;
  if (!rnd_rect(o, c, &ulo, &uhi, &vlo, &vhi)) return;
  const RndWin W = wins[blockIdx.y];
  if (ulo < W.u0 || vlo < W.v0 || uhi >= W.u0 + W.w || vhi >= W.v0 + W.h) return; /* never: the window holds every rectangle */
  const double npd = rnd_npd(o);
  for (int v = vlo; v <= vhi; v++)
    for (int u = ulo; u <= uhi; u++) {
      float d;
      if (rnd_cover(o, npd, u, v, c, &d))
        atomicMin(&zbuf[W.off + (size_t)(v - W.v0) * W.w + (u - W.u0)], __float_as_uint(d));
    }
}

/* the visibility test of a considered moved row o against its job's render */
struct RndView {
  const RndWin* wins;
  const uint32_t* zbuf;
  RndCam c;
};

__device__ __forceinline__ bool rnd_visible(const float* o, const RndView& rv, int job) {
  if (!(o[2] > 0.f)) return false;
  const double ui = floor((double)o[0] * rv.c.fx / (double)o[2] + rv.c.ppx + 0.5);
  const double vi = floor((double)o[1] * rv.c.fy / (double)o[2] + rv.c.ppy + 0.5);
  if (!(ui >= 0.0 && ui < (double)rv.c.cols && vi >= 0.0 && vi < (double)rv.c.rows)) return false;
  const RndWin W = rv.wins[job];
  const int u = (int)ui - W.u0, v = (int)vi - W.v0;
  if (u < 0 || v < 0 || u >= W.w || v >= W.h) return true; /* never: the window holds the centre of every rendered row */
  const uint32_t zb = rv.zbuf[W.off + (size_t)v * W.w + u];
  return zb == RND_EMPTY || o[2] <= __uint_as_float(zb) + rv.c.tol;
}

__global__ __launch_bounds__(VFY_BLOCK) void k_rnd_vfy_score(VfyArgs a, RndView rv, VfyPartial* __restrict__ part) {
  vfy_score_rows<true>(a, &rv, part);
}

/* grid (blocks of the largest model) x chosen poses: one frame-wide buffer of (depth bits << 32 | label) */
__global__ __launch_bounds__(RND_BLOCK) void k_rnd_splat_frame(const RndJob* __restrict__ jobs, RndCam c, unsigned long long* __restrict__ zbuf) {
  const RndJob& J = jobs[blockIdx.y];
  const int r = blockIdx.x * RND_BLOCK + threadIdx.x;
  if (r >= J.n) return;
  float o[6];
  rnd_move(J, r, o);
  int ulo, uhi, vlo, vhi;
  if (!rnd_rect(o, c, &ulo, &uhi, &vlo, &vhi)) return;
  const double npd = rnd_npd(o);
  const unsigned long long lab = (unsigned long long)(uint32_t)J.label;
  for (int v = vlo; v <= vhi; v++)
    for (int u = ulo; u <= uhi; u++) {
      float d;
      if (rnd_cover(o, npd, u, v, c, &d)) atomicMin(&zbuf[(size_t)v * c.cols + u], ((unsigned long long)__float_as_uint(d) << 32) | lab);
    }
}

__global__ __launch_bounds__(256) void k_rnd_resolve(const unsigned long long* __restrict__ zbuf, size_t n, float* __restrict__ depth,
                                                     int32_t* __restrict__ label) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = zbuf[i];
  depth[i] = k == RND_EMPTY64 ? 0.f : __uint_as_float((uint32_t)(k >> 32));
  label[i] = k == RND_EMPTY64 ? -1 : (int32_t)(uint32_t)k;
}

#endif /* PPF_RENDER_KERNELS_H */
