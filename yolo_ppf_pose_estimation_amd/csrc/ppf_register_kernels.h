/*
 * ppf_register_kernels.h — a raw sensor depth image drawn into the colour camera's pixel grid on gfx950
 * (ppf_depth_register).  Included by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_z, depth_keep);
 * the host side is ppf_register_host.h; the camera arithmetic is include/ppf_camera_math.h, shared with the host entries.
 *
 *   k_reg_rays     once per calibration: one thread per depth pixel unprojects it, 16 bytes a pixel
 *   k_reg_clear    the u32 z-buffer to all ones, the counters to 0
 *   k_reg_draw     a workgroup per 16 x 16 tile of depth pixels: its 17 x 17 vertices (uc, vc as doubles, zc) once into
 *                  LDS, then a thread per quad draws the quad's two triangles with atomicMin of the depth's bit pattern
 *                  (positive floats order as unsigned integers); the counters through wave ballots, one integer atomicAdd
 *                  per counter and block
 *   k_reg_resolve  z-buffer -> float image (in place when they are one buffer), all ones -> 0; counts the filled pixels
 * Integer atomics only; a triangle's pixel loop is bounded by PPF_REGISTER_MAX_QUAD_PX in the kernel itself, so a runaway
 * vertex cannot turn into a long loop.  Every value is a fixed fp64 / fp32 expression evaluated as written (the library is
 * built with -ffp-contract=off), and the minimum does not depend on the order of the atomics.
 */
#ifndef PPF_REGISTER_KERNELS_H
#define PPF_REGISTER_KERNELS_H

#include "../../include/ppf_camera_math.h"

constexpr int REG_BLOCK = 256;
constexpr int REG_TILE = 16;               /* depth pixels (and quads) per tile side */
constexpr int REG_VSIDE = REG_TILE + 1;    /* vertices per tile side */
constexpr int REG_VERTS = REG_VSIDE * REG_VSIDE;
constexpr uint32_t REG_EMPTY = 0xffffffffu;
enum { REG_C_VERTICES = 0, REG_C_QUADS, REG_C_CUT, REG_C_OVERSIZE, REG_C_FILLED, REG_N_COUNTERS = 8 };

struct RegArgs {
  DepthArgs d;         /* the depth image: img, pitch, cols, n, scale, z_min, z_max (the intrinsics are not used) */
  int d_rows;
  const double* rays;  /* [d_rows][d.cols][2] */
  double R[9], t[3];
  ppf_camera cc;       /* the colour camera */
  int c_rows, c_cols;
  float dz_abs, dz_rel;
  uint32_t* zbuf;      /* c_rows x c_cols */
  int32_t* counters;   /* REG_N_COUNTERS */
  int tiles_x;
};

__global__ __launch_bounds__(REG_BLOCK) void k_reg_rays(ppf_camera cam, int cols, int n, double* __restrict__ rays) {
  const size_t p = (size_t)blockIdx.x * REG_BLOCK + threadIdx.x;
  if (p >= (size_t)n) return;
  const int v = (int)(p / (size_t)cols), u = (int)(p - (size_t)v * cols);
  double x, y;
  (void)ppf_cam_unproject(&cam, (double)u, (double)v, &x, &y);
  reinterpret_cast<double2*>(rays)[p] = make_double2(x, y);
}

__global__ __launch_bounds__(REG_BLOCK) void k_reg_clear(uint32_t* __restrict__ zbuf, size_t n, int32_t* __restrict__ counters) {
  const size_t p = (size_t)blockIdx.x * REG_BLOCK + threadIdx.x;
  if (p < n) zbuf[p] = REG_EMPTY;
  if (p < (size_t)REG_N_COUNTERS) counters[p] = 0;
}

/* One triangle (a, b, c), z the vertices' depths: every pixel of its clamped bounding box that it covers takes the
 * minimum of the interpolated depth.  Returns true when the box is over PPF_REGISTER_MAX_QUAD_PX and nothing was drawn. */
__device__ __forceinline__ bool reg_draw_triangle(double ax, double ay, float az, double bx, double by, float bz, double cx, double cy,
                                                  float cz, uint32_t* __restrict__ zbuf, int rows, int cols) {
  double x0 = ax < bx ? ax : bx, x1 = ax > bx ? ax : bx, y0 = ay < by ? ay : by, y1 = ay > by ? ay : by;
  x0 = ceil(x0 < cx ? x0 : cx);
  x1 = floor(x1 > cx ? x1 : cx);
  y0 = ceil(y0 < cy ? y0 : cy);
  y1 = floor(y1 > cy ? y1 : cy);
  /* clamped to the image as doubles: the conversions to int below cannot overflow */
  x0 = x0 < 0.0 ? 0.0 : x0;
  y0 = y0 < 0.0 ? 0.0 : y0;
  x1 = x1 > (double)(cols - 1) ? (double)(cols - 1) : x1;
  y1 = y1 > (double)(rows - 1) ? (double)(rows - 1) : y1;
  if (x1 < x0 || y1 < y0) return false;
  if (x1 - x0 >= (double)PPF_REGISTER_MAX_QUAD_PX || y1 - y0 >= (double)PPF_REGISTER_MAX_QUAD_PX) return true;
  const int i0 = (int)x0, i1 = (int)x1, j0 = (int)y0, j1 = (int)y1; /* at most 16 x 16 pixels */
  const double area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  if (!(area != 0.0)) return false;
  for (int j = j0; j <= j1; j++) {
    const double py = (double)j;
    for (int i = i0; i <= i1; i++) {
      const double px = (double)i;
      const double w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
      const double w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
      const double w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
      if ((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0)) {
        const float zz = (float)((w0 * (double)az + w1 * (double)bz + w2 * (double)cz) / area);
        if (isfinite(zz) && zz > 0.f) atomicMin(&zbuf[(size_t)j * cols + i], __float_as_uint(zz));
      }
    }
  }
  return false;
}

/* grid: tiles_x * tiles_y tiles of REG_TILE x REG_TILE depth pixels (1-D: a one-column image has more tile rows than a grid's
 * y extent); thread (tx, ty) = (threadIdx.x & 15, threadIdx.x >> 4) owns vertex and quad (u0 + tx, v0 + ty) */
template <class T>
__global__ __launch_bounds__(REG_BLOCK) void k_reg_draw(RegArgs a) {
  __shared__ double s_u[REG_VERTS], s_v[REG_VERTS]; /* uc NaN: not a valid vertex */
  __shared__ float s_z[REG_VERTS];
  __shared__ int s_cnt[REG_BLOCK / 64][4];
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int u0 = tile_x * REG_TILE, v0 = tile_y * REG_TILE;
  const int cols = a.d.cols, rows = a.d_rows;
  for (int i = threadIdx.x; i < REG_VERTS; i += REG_BLOCK) {
    const int ly = i / REG_VSIDE, lx = i - ly * REG_VSIDE;
    const int u = u0 + lx, v = v0 + ly;
    double uc = ppf_cam_nan(), vc = ppf_cam_nan();
    float zc = 0.f;
    if (u < cols && v < rows) {
      const float z = depth_z(reinterpret_cast<const T*>(a.d.img + (size_t)v * a.d.pitch) + u, a.d);
      if (depth_keep(z, a.d)) {
        const double2 ray = reinterpret_cast<const double2*>(a.rays)[(size_t)v * cols + u];
        if (ray.x == ray.x) { /* an invalid ray is NaN NaN */
          const double P0 = ray.x * (double)z, P1 = ray.y * (double)z, P2 = (double)z;
          const double Q0 = a.R[0] * P0 + a.R[1] * P1 + a.R[2] * P2 + a.t[0];
          const double Q1 = a.R[3] * P0 + a.R[4] * P1 + a.R[5] * P2 + a.t[1];
          const double Q2 = a.R[6] * P0 + a.R[7] * P1 + a.R[8] * P2 + a.t[2];
          if (Q2 > 0.0) {
            (void)ppf_cam_project(&a.cc, Q0 / Q2, Q1 / Q2, &uc, &vc); /* NaN NaN when invalid */
            zc = (float)Q2;
          }
        }
      }
    }
    s_u[i] = uc;
    s_v[i] = vc;
    s_z[i] = zc;
  }
  __syncthreads();
  const int tx = threadIdx.x & (REG_TILE - 1), ty = threadIdx.x >> 4, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i00 = ty * REG_VSIDE + tx, i10 = i00 + 1, i01 = i00 + REG_VSIDE, i11 = i01 + 1;
  const double u00 = s_u[i00];
  const bool vertex = u00 == u00; /* pixels past the image were stored as NaN */
  bool quad = false, cut = false, oversize = false;
  if (u0 + tx < cols - 1 && v0 + ty < rows - 1) {
    const double u10 = s_u[i10], u01 = s_u[i01], u11 = s_u[i11];
    quad = vertex && u10 == u10 && u01 == u01 && u11 == u11;
    if (quad) {
      const float z00 = s_z[i00], z10 = s_z[i10], z01 = s_z[i01], z11 = s_z[i11];
      float lo = z00 < z10 ? z00 : z10, hi = z00 > z10 ? z00 : z10;
      lo = lo < z01 ? lo : z01;
      hi = hi > z01 ? hi : z01;
      lo = lo < z11 ? lo : z11;
      hi = hi > z11 ? hi : z11;
      cut = hi - lo > a.dz_abs + a.dz_rel * lo;
      if (!cut) {
        const double v00 = s_v[i00], v10 = s_v[i10], v01 = s_v[i01], v11 = s_v[i11];
        const bool o1 = reg_draw_triangle(u00, v00, z00, u10, v10, z10, u01, v01, z01, a.zbuf, a.c_rows, a.c_cols);
        const bool o2 = reg_draw_triangle(u11, v11, z11, u01, v01, z01, u10, v10, z10, a.zbuf, a.c_rows, a.c_cols);
        oversize = o1 || o2;
      }
    }
  }
  const int nv = __popcll(__ballot(vertex)), nq = __popcll(__ballot(quad)), nc = __popcll(__ballot(cut)), no = __popcll(__ballot(oversize));
  if (lane == 0) {
    s_cnt[wv][0] = nv;
    s_cnt[wv][1] = nq;
    s_cnt[wv][2] = nc;
    s_cnt[wv][3] = no;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < REG_BLOCK / 64; w++) n += s_cnt[w][threadIdx.x];
    if (n) atomicAdd(&a.counters[threadIdx.x], n);
  }
}

/* zbuf and out may be one buffer: every thread reads its own word before it writes it */
__global__ __launch_bounds__(REG_BLOCK) void k_reg_resolve(const uint32_t* zbuf, float* out, size_t n, int32_t* __restrict__ counters) {
  __shared__ int s_n[REG_BLOCK / 64];
  const size_t p = (size_t)blockIdx.x * REG_BLOCK + threadIdx.x;
  bool filled = false;
  if (p < n) {
    const uint32_t z = zbuf[p];
    filled = z != REG_EMPTY;
    out[p] = filled ? __uint_as_float(z) : 0.f;
  }
  const int nf = __popcll(__ballot(filled));
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = nf;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < REG_BLOCK / 64; w++) t += s_n[w];
    if (t) atomicAdd(&counters[REG_C_FILLED], t);
  }
}

#endif /* PPF_REGISTER_KERNELS_H */
