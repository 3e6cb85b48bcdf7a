/*
 * ppf_motion_kernels.h — the camera's motion between two depth images on gfx950: whole-image projective point-to-plane ICP
 * over a small pyramid (ppf_depth_motion; the arithmetic is the comment above ppf_depth_motion in
 * include/ppf_hip.h).  Included by ppf_hip.hip after ppf_history_kernels.h (history_load) and ppf_refine_kernels.h
 * (rfn_wave_sum; icp_solve6_wave, icp_transform_from_euler through ppf_icp_kernels.h); host side: ppf_motion_host.h.
 *
 *   k_motion_level0<T>  both images (blockIdx.y) through their pitches into packed float z, 0 where a pixel is not kept: one
 *                    lane owns four pixels of a row and loads them as k_history_push does (history_load); block 0 also
 *                    writes the call's state: T = the start, everything else 0
 *   k_motion_down    level l -> l + 1 of both images, one lane per output pixel
 *   k_motion_maps    one 16-byte record (z, nx, ny, nz) per pixel of a level of both images; a 16 x 16 tile with a one-pixel
 *                    halo of z staged in LDS; a pixel without a normal keeps its z and gets a zero normal (a normal is a
 *                    unit vector cast to float, never all zero); the source count of `prev` from ballots, one integer
 *                    atomicAdd per workgroup
 *   k_motion_eval    one lane per source pixel, one wave per chunk of 64: one 16-byte load of the source record, one
 *                    dependent 16-byte load of the target record, the 28 products in registers, rfn_wave_sum's tree (the
 *                    function ppf_refine_frame uses), lane 0 writes the chunk's 28 partials and its pair count (a ballot's
 *                    popcount).  A chunk without a pair writes +0.0 without running the tree: the tree of 64 times +0.0
 *   k_motion_group   the same tree over 64 partials: one wave per (group, component), the pair counts as integers
 *   k_motion_tail    one workgroup: the last one or two tree levels (at most DM_TAIL_MAX partials come in), the guards,
 *                    icp_solve6_wave, the step check, T <- M T, the level's row and the state
 * Partials are stored component-major, [component][chunk], so the next stage's lanes read neighbouring doubles.
 *
 * Every kernel of an evaluation reads the state first and returns when the call has ended (LOST, STEP) or its level has
 * (CONVERGED, SKIPPED): the host enqueues every evaluation of every level ahead and waits once.  No float atomics, no
 * inline assembly, no grid-wide synchronisation; nothing is fused (-ffp-contract=off).
 */
#ifndef PPF_MOTION_KERNELS_H
#define PPF_MOTION_KERNELS_H

constexpr int DM_BLOCK = 256;
constexpr int DM_WAVES = DM_BLOCK / 64;
constexpr int DM_TILE = 16;                 /* k_motion_maps: DM_TILE x DM_TILE pixels per workgroup */
constexpr int DM_HALO = DM_TILE + 2;
constexpr int DM_TAIL_BLOCK = 512;          /* 8 waves, as k_rfn_refine: icp_solve6_wave keeps a 6 x 7 system in registers */
constexpr int DM_TAIL_WAVES = DM_TAIL_BLOCK / 64;
constexpr int DM_TAIL_MAX = 1024;           /* partial rows k_motion_tail takes: 16 groups, then one */
constexpr int DM_TAIL_GROUPS = DM_TAIL_MAX / 64;
constexpr int DM_COMPONENTS = ICP_ENTRIES + 1; /* k_motion_group: the 28 sums and the pair count */

struct MotionState {
  double T[16];
  ppf_depth_motion_level rows[PPF_MOTION_MAX_LEVELS];
  int32_t ended;                              /* 0, or the status (LOST, STEP) that ended the call */
  int32_t last_status;                        /* the status of the last level that got one */
  int32_t n_evaluations;
  int32_t pad;
  int32_t level_done[PPF_MOTION_MAX_LEVELS];  /* a level's status once it has one */
  int32_t n_source[PPF_MOTION_MAX_LEVELS];
};

struct MotionInit {
  double T[16];
};

/* one level of both images: 0 = prev, 1 = cur */
struct MotionLvl {
  int level, rows, cols, n; /* n = rows * cols */
  double fx, fy, ppx, ppy;
  double ngate;             /* (double)normal_gate * 2^level */
  const float* z0;
  const float* z1;
  float4* rec0;
  float4* rec1;
};

struct MotionRun {
  double dist2, normal_cos, min_pair_share;
  double max_rot2, max_trans2, eps_rot2, eps_trans2;
  int min_pairs, pad;
  MotionState* state;
};

/* an evaluation of level l has nothing to do: the call or the level has ended, or the level will be skipped */
__device__ __forceinline__ bool motion_idle(const MotionState* S, int l, int min_pairs) {
  return S->ended != 0 || S->level_done[l] != 0 || S->n_source[l] < min_pairs;
}

/* grid: (ceil(rows * groups / DM_BLOCK), 2) */
template <class T>
__global__ __launch_bounds__(DM_BLOCK) void k_motion_level0(DepthArgs a0, DepthArgs a1, int in_vec0, int in_vec1, int rows, int groups,
                                                            float* __restrict__ z0, float* __restrict__ z1, int out_vec, MotionState* S,
                                                            MotionInit init) {
  const bool second = blockIdx.y != 0;
  if (blockIdx.x == 0 && !second) {
    /* the state: T = the start, the rest zero */
    int32_t* w = reinterpret_cast<int32_t*>(S);
    for (int i = threadIdx.x; i < (int)(sizeof(MotionState) / sizeof(int32_t)); i += DM_BLOCK) {
      const int e = i >> 1;
      w[i] = e < 16 ? ((i & 1) ? __double2hiint(init.T[e]) : __double2loint(init.T[e])) : 0;
    }
  }
  const long long g = (long long)blockIdx.x * DM_BLOCK + threadIdx.x;
  if (g >= (long long)rows * groups) return;
  const int v = (int)(g / groups), u0 = (int)(g - (long long)v * groups) * DH_PX;
  float z[DH_PX];
  int cols;
  if (second) {
    history_load<T>(a1, in_vec1, v, u0, z);
    cols = a1.cols;
  } else {
    history_load<T>(a0, in_vec0, v, u0, z);
    cols = a0.cols;
  }
  float* out = (second ? z1 : z0) + (size_t)v * (size_t)cols + (size_t)u0;
  if (out_vec) {
    *reinterpret_cast<float4*>(out) = make_float4(z[0], z[1], z[2], z[3]);
  } else {
#pragma unroll
    for (int j = 0; j < DH_PX; j++)
      if (u0 + j < cols) out[j] = z[j];
  }
}

/* grid: (ceil(rows_out * cols_out / DM_BLOCK), 2); rows_out = rows_in / 2, cols_out = cols_in / 2 */
__global__ __launch_bounds__(DM_BLOCK) void k_motion_down(const float* __restrict__ in0, const float* __restrict__ in1, float* __restrict__ out0,
                                                          float* __restrict__ out1, int cols_in, int rows_out, int cols_out, double pyr_gate) {
  const long long p = (long long)blockIdx.x * DM_BLOCK + threadIdx.x;
  if (p >= (long long)rows_out * cols_out) return;
  const int v = (int)(p / cols_out), u = (int)(p - (long long)v * cols_out);
  const float* in = (blockIdx.y ? in1 : in0) + (size_t)(2 * v) * (size_t)cols_in + (size_t)(2 * u);
  const float s[4] = {in[0], in[1], in[cols_in], in[cols_in + 1]};
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (s[i] > 0.f && (m == 0.f || s[i] < m)) m = s[i];
  double sum = 0.0;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (s[i] > 0.f && (double)s[i] - (double)m <= pyr_gate) {
      sum = sum + (double)s[i];
      cnt++;
    }
  (blockIdx.y ? out1 : out0)[p] = cnt ? (float)(sum / (double)cnt) : 0.f;
}

/* grid: (tiles_x * ceil(rows / DM_TILE), 2), tiles_x = ceil(cols / DM_TILE); DM_BLOCK threads */
__global__ __launch_bounds__(DM_BLOCK) void k_motion_maps(MotionLvl L, int tiles_x, MotionState* S) {
  __shared__ float s_z[DM_HALO][DM_HALO];
  __shared__ int s_n[DM_WAVES];
  const bool second = blockIdx.y != 0;
  const float* __restrict__ zimg = second ? L.z1 : L.z0;
  const int bu = (int)(blockIdx.x % (unsigned)tiles_x) * DM_TILE, bv = (int)(blockIdx.x / (unsigned)tiles_x) * DM_TILE;
  for (int i = threadIdx.x; i < DM_HALO * DM_HALO; i += DM_BLOCK) {
    const int ty = i / DM_HALO, tx = i - ty * DM_HALO;
    const int gu = bu + tx - 1, gv = bv + ty - 1;
    s_z[ty][tx] = (gu >= 0 && gu < L.cols && gv >= 0 && gv < L.rows) ? zimg[(size_t)gv * (size_t)L.cols + (size_t)gu] : 0.f;
  }
  __syncthreads();
  const int tx = threadIdx.x % DM_TILE, ty = threadIdx.x / DM_TILE;
  const int u = bu + tx, v = bv + ty;
  const bool inside = u < L.cols && v < L.rows;
  bool has = false;
  float nrm[3] = {0.f, 0.f, 0.f};
  const float zc = s_z[ty + 1][tx + 1];
  if (inside && zc > 0.f) {
    /* a neighbour outside the image was staged as 0: not kept */
    const float zl = s_z[ty + 1][tx], zr = s_z[ty + 1][tx + 2], zu = s_z[ty][tx + 1], zd = s_z[ty + 2][tx + 1];
    const double Z = (double)zc, Zl = (double)zl, Zr = (double)zr, Zu = (double)zu, Zd = (double)zd;
    if (zl > 0.f && zr > 0.f && zu > 0.f && zd > 0.f && ppf_fabs(Zl - Z) <= L.ngate && ppf_fabs(Zr - Z) <= L.ngate &&
        ppf_fabs(Zu - Z) <= L.ngate && ppf_fabs(Zd - Z) <= L.ngate) {
      const double xm = (double)(u - 1) - L.ppx, x0 = (double)u - L.ppx, xp = (double)(u + 1) - L.ppx;
      const double ym = (double)(v - 1) - L.ppy, y0 = (double)v - L.ppy, yp = (double)(v + 1) - L.ppy;
      const double dx[3] = {xp * Zr / L.fx - xm * Zl / L.fx, y0 * Zr / L.fy - y0 * Zl / L.fy, Zr - Zl};
      const double dy[3] = {x0 * Zd / L.fx - x0 * Zu / L.fx, yp * Zd / L.fy - ym * Zu / L.fy, Zd - Zu};
      const double c[3] = {dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]};
      const double len = ppf_sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
      if (len > 0.0) {
        const float n0 = (float)(c[0] / len), n1 = (float)(c[1] / len), n2 = (float)(c[2] / len);
        const double V[3] = {x0 * Z / L.fx, y0 * Z / L.fy, Z};
        const double facing = ((double)n0 * V[0] + (double)n1 * V[1]) + (double)n2 * V[2];
        if (facing < 0.0 && (n0 != 0.f || n1 != 0.f || n2 != 0.f)) {
          has = true;
          nrm[0] = n0; nrm[1] = n1; nrm[2] = n2;
        }
      }
    }
  }
  if (inside) (second ? L.rec1 : L.rec0)[(size_t)v * (size_t)L.cols + (size_t)u] = make_float4(zc, nrm[0], nrm[1], nrm[2]);
  if (second) return; /* uniform over the workgroup: only prev's normals are counted */
  const int cnt = __popcll(__ballot(has));
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < DM_WAVES; w++) t += s_n[w];
    if (t) atomicAdd(&S->n_source[L.level], t);
  }
}

/* grid: ceil(n_chunks / DM_WAVES), n_chunks = ceil(L.n / 64); parts: [ICP_ENTRIES][n_chunks], counts: [n_chunks] */
__global__ __launch_bounds__(DM_BLOCK) void k_motion_eval(MotionLvl L, MotionRun R, double* __restrict__ parts, uint32_t* __restrict__ counts) {
  const MotionState* S = R.state;
  if (motion_idle(S, L.level, R.min_pairs)) return;
  const int lane = threadIdx.x & 63;
  const int n_chunks = (int)(((long long)L.n + 63) / 64);
  const int chunk = blockIdx.x * DM_WAVES + (threadIdx.x >> 6);
  if (chunk >= n_chunks) return; /* uniform over the wave */
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; e++) T[e] = S->T[e];
  const long long j = (long long)chunk * 64 + lane;
  bool pair = false;
  double Jv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  if (j < L.n) {
    const float4 s = L.rec0[j];
    if (s.y != 0.f || s.z != 0.f || s.w != 0.f) {
      const int v = (int)(j / L.cols), u = (int)(j - (long long)v * L.cols);
      const double Z = (double)s.x;
      const double V[3] = {((double)u - L.ppx) * Z / L.fx, ((double)v - L.ppy) * Z / L.fy, Z};
      const double n[3] = {(double)s.y, (double)s.z, (double)s.w};
      double p[3], nn[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        p[a] = ((T[a * 4] * V[0] + T[a * 4 + 1] * V[1]) + T[a * 4 + 2] * V[2]) + T[a * 4 + 3];
        nn[a] = (T[a * 4] * n[0] + T[a * 4 + 1] * n[1]) + T[a * 4 + 2] * n[2];
      }
      if (p[2] > 0.0) {
        const double ui = floor((p[0] * L.fx / p[2] + L.ppx) + 0.5), vi = floor((p[1] * L.fy / p[2] + L.ppy) + 0.5);
        if (ui >= 0.0 && ui < (double)L.cols && vi >= 0.0 && vi < (double)L.rows) {
          const float4 t = L.rec1[(size_t)(int)vi * (size_t)L.cols + (size_t)(int)ui];
          if (t.y != 0.f || t.z != 0.f || t.w != 0.f) {
            const double Zt = (double)t.x;
            const double nt[3] = {(double)t.y, (double)t.z, (double)t.w};
            const double dq[3] = {(ui - L.ppx) * Zt / L.fx - p[0], (vi - L.ppy) * Zt / L.fy - p[1], Zt - p[2]};
            const double d2 = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
            const double cs = (nn[0] * nt[0] + nn[1] * nt[1]) + nn[2] * nt[2];
            if (d2 <= R.dist2 && cs >= R.normal_cos) {
              pair = true;
              r = (nt[0] * dq[0] + nt[1] * dq[1]) + nt[2] * dq[2];
              Jv[0] = p[1] * nt[2] - p[2] * nt[1];
              Jv[1] = p[2] * nt[0] - p[0] * nt[2];
              Jv[2] = p[0] * nt[1] - p[1] * nt[0];
              Jv[3] = nt[0]; Jv[4] = nt[1]; Jv[5] = nt[2];
            }
          }
        }
      }
    }
  }
  const unsigned long long mask = __ballot(pair);
  if (lane == 0) counts[chunk] = (uint32_t)__popcll(mask);
  if (mask == 0ull) { /* uniform: 64 lanes of +0.0 sum to +0.0 */
    if (lane < ICP_ENTRIES) parts[(size_t)lane * n_chunks + chunk] = 0.0;
    return;
  }
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int jj = i; jj < 6; jj++) {
      const double s = rfn_wave_sum(Jv[i] * Jv[jj]);
      if (lane == 0) parts[(size_t)e * n_chunks + chunk] = s;
      e++;
    }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const double s = rfn_wave_sum(Jv[i] * r);
    if (lane == 0) parts[(size_t)(21 + i) * n_chunks + chunk] = s;
  }
  {
    const double s = rfn_wave_sum(r * r);
    if (lane == 0) parts[(size_t)27 * n_chunks + chunk] = s;
  }
}

/* n_in partial rows -> n_out = ceil(n_in / 64); grid: ceil(n_out * DM_COMPONENTS / DM_WAVES): one wave per (group, component) */
__global__ __launch_bounds__(DM_BLOCK) void k_motion_group(const MotionState* S, int level, int min_pairs, const double* __restrict__ in,
                                                           const uint32_t* __restrict__ cin, int n_in, double* __restrict__ out,
                                                           uint32_t* __restrict__ cout, int n_out) {
  if (motion_idle(S, level, min_pairs)) return;
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * DM_WAVES + (threadIdx.x >> 6);
  if (w >= (long long)n_out * DM_COMPONENTS) return; /* uniform over the wave */
  const int g = (int)(w / DM_COMPONENTS), e = (int)(w - (long long)g * DM_COMPONENTS);
  const int c = g * 64 + lane;
  if (e < ICP_ENTRIES) {
    const double s = rfn_wave_sum(c < n_in ? in[(size_t)e * n_in + c] : 0.0);
    if (lane == 0) out[(size_t)e * n_out + g] = s;
  } else {
    uint32_t t = c < n_in ? cin[c] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
    if (lane == 0) cout[g] = t;
  }
}

/* one workgroup of DM_TAIL_BLOCK threads; n_in <= DM_TAIL_MAX partial rows; evaluation k of level L.level, which has iters
 * evaluations enqueued (0: the launch only marks the level SKIPPED) */
__global__ __launch_bounds__(DM_TAIL_BLOCK) void k_motion_tail(MotionLvl L, MotionRun R, const double* __restrict__ in,
                                                               const uint32_t* __restrict__ cin, int n_in, int k, int iters) {
  __shared__ double s_grp[ICP_ENTRIES][DM_TAIL_GROUPS];
  __shared__ double s_tot[ICP_ENTRIES];
  __shared__ uint32_t s_np;
  __shared__ int s_go;
  MotionState* S = R.state;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = L.level;
  if (tid == 0) {
    s_np = 0;
    s_go = 0;
    if (S->ended == 0 && S->level_done[l] == 0) {
      if (iters == 0 || S->n_source[l] < R.min_pairs) {
        ppf_depth_motion_level& row = S->rows[l];
        row.status = PPF_MOTION_SKIPPED;
        row.rows = L.rows;
        row.cols = L.cols;
        row.n_source = S->n_source[l];
        S->level_done[l] = PPF_MOTION_SKIPPED;
        S->last_status = PPF_MOTION_SKIPPED;
      } else {
        s_go = 1;
      }
    }
  }
  __syncthreads();
  if (!s_go) return;
  /* ---- the pair count ---- */
  {
    uint32_t t = 0;
    for (int i = tid; i < n_in; i += DM_TAIL_BLOCK) t += cin[i];
    if (t) atomicAdd(&s_np, t);
  }
  /* ---- the last tree levels ---- */
  if (n_in > 64) {
    const int groups = (n_in + 63) / 64;
    for (int t = wave; t < groups * ICP_ENTRIES; t += DM_TAIL_WAVES) {
      const int g = t / ICP_ENTRIES, e = t - g * ICP_ENTRIES, c = g * 64 + lane;
      const double s = rfn_wave_sum(c < n_in ? in[(size_t)e * n_in + c] : 0.0);
      if (lane == 0) s_grp[e][g] = s;
    }
    __syncthreads();
    for (int e = wave; e < ICP_ENTRIES; e += DM_TAIL_WAVES) {
      const double s = groups > 1 ? rfn_wave_sum(lane < groups ? s_grp[e][lane] : 0.0) : s_grp[e][0];
      if (lane == 0) s_tot[e] = s;
    }
  } else {
    for (int e = wave; e < ICP_ENTRIES; e += DM_TAIL_WAVES) {
      /* one value left: it is the sum */
      const double s = n_in > 1 ? rfn_wave_sum(lane < n_in ? in[(size_t)e * n_in + lane] : 0.0) : in[e];
      if (lane == 0) s_tot[e] = s;
    }
  }
  __syncthreads();
  /* ---- the step (wave 0), as k_rfn_refine's with the rotation about the camera origin ---- */
  if (wave != 0) return;
  const uint32_t np = s_np;
  const int32_t n_source = S->n_source[l];
  int status = 0;
  if ((int)np < R.min_pairs || (double)np < R.min_pair_share * (double)n_source) status = PPF_MOTION_LOST;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = false;
  if (!status) ok = icp_solve6_wave(s_tot, lane, x); /* uniform over the wave */
  if (lane != 0) return;
  ppf_depth_motion_level& row = S->rows[l];
  int32_t iterations = k == 0 ? 0 : row.iterations;
  if (!status) {
    const double ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], tt = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
    bool fin = ok;
#pragma unroll
    for (int i = 0; i < 6; i++) fin = fin && isfinite(x[i]);
    if (!fin || ww > R.max_rot2 || tt > R.max_trans2) {
      status = PPF_MOTION_STEP;
    } else {
      double T[16], M[16], Tn[16];
#pragma unroll
      for (int e = 0; e < 16; e++) T[e] = S->T[e];
      icp_transform_from_euler(x, x + 3, M);
      ppf_mat44_mul(M, T, Tn);
#pragma unroll
      for (int e = 0; e < 16; e++) S->T[e] = Tn[e];
      iterations = k + 1;
      if (ww <= R.eps_rot2 && tt <= R.eps_trans2) status = PPF_MOTION_CONVERGED;
      else if (k + 1 == iters) status = PPF_MOTION_MAX_ITERS_REACHED;
    }
  }
  const float rmse = np ? (float)ppf_sqrt(s_tot[27] / (double)np) : 0.f;
  row.status = status;
  row.iterations = iterations;
  row.rows = L.rows;
  row.cols = L.cols;
  row.n_source = n_source;
  if (k == 0) {
    row.n_pairs_first = (int32_t)np;
    row.rmse_first = rmse;
  }
  row.n_pairs_last = (int32_t)np;
  row.rmse_last = rmse;
  S->n_evaluations = S->n_evaluations + 1;
  if (status) {
    S->level_done[l] = status;
    S->last_status = status;
    if (status == PPF_MOTION_LOST || status == PPF_MOTION_STEP) S->ended = status;
  }
}

#endif /* PPF_MOTION_KERNELS_H */
