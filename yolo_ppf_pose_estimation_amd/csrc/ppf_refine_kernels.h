/*
 * ppf_refine_kernels.h — projective point-to-plane refinement of posed model clouds on the depth image itself, on gfx950
 * (ppf_refine_frame).  Included by ppf_hip.hip after ppf_icp_kernels.h (icp_transform_row, icp_sum_staged,
 * icp_solve6_wave, icp_transform_from_euler) and ppf_verify_kernels.h (vfy_finite6); the host side is ppf_refine_host.h.
 *
 * One kernel, one persistent workgroup per job (a pose of a detection), every iteration inside the one launch:
 *   prologue    c0 = the mean of the finite scored model rows (chunk sums as below)
 *   evaluation  a wave takes a chunk of ICP_CHUNK scored rows, one row per lane: the row is moved (icp_transform_row), tested
 *               (finite, facing), projected, and paired with the depth pixel under it when that pixel is within depth_gate;
 *               the lane's 28 products (21 of J^T J's upper triangle, 6 of J^T r, r^2; +0.0 without a pair) are reduced over
 *               the wave by a fixed tree (lane l adds lane l + 32, 16, 8, 4, 2, 1) through v_permlane32_swap,
 *               v_permlane16_swap and DPP row shifts -- no LDS -- and lane 0 writes the chunk's partial row to job scratch
 *   sums        the partial rows in chunk order, staged through LDS (icp_sum_staged)
 *   step        wave 0: the pair-share guard, the 6x6 solve (icp_solve6_wave), the step limits, T <- M T
 * No float atomics, and nothing a job reads or adds depends on the other jobs of the call.
 */
#ifndef PPF_REFINE_KERNELS_H
#define PPF_REFINE_KERNELS_H

constexpr int RFN_BLOCK = 512; /* 8 waves: two per SIMD, so a lane may hold the 28 fp64 products and a pose in registers */
constexpr int RFN_WAVES = RFN_BLOCK / 64;
constexpr int RFN_TILE = 64;    /* chunks per LDS tile of the 28-component sums */
constexpr int RFN_TILE_C0 = RFN_TILE * ICP_ENTRIES / 3; /* ... of the 3-component sums, in the same LDS */

struct RfnJob {
  double T[16];
  const float* model; /* n_model x 6 */
  int n_rows;         /* ceil(n_model / step) */
  int pad;
  size_t o_parts;     /* the job's first double in the partials */
};

struct RfnOut {
  double T[16];
  ppf_refine_info info;
};

struct RfnArgs {
  const RfnJob* jobs;
  const float* depth;
  int rows, cols;
  double fx, fy, ppx, ppy;
  double max_rot2, max_trans2, eps_rot2, eps_trans2; /* the squares of the limits, in fp64 */
  float gate, min_pair_share;
  int min_pairs, max_iters, step;
  double* parts; /* per job chunks x ICP_ENTRIES */
  RfnOut* out;
};

template <int CTRL>
__device__ __forceinline__ double rfn_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

/* lane 0 gets the sum of the wave's values by the fixed tree: lane l adds lane l + 32, then + 16, 8, 4, 2, 1.  The upper
 * half comes down through v_permlane32_swap, row 1 onto row 0 through v_permlane16_swap, the rest are DPP shifts inside
 * the row of 16.  The lanes that are not part of the tree end with values nobody reads. */
__device__ __forceinline__ double rfn_wave_sum(double v) {
  {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    v = v + __hiloint2double((int)b[1], (int)a[1]);
  }
  {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = v + __hiloint2double((int)b[1], (int)a[1]);
  }
  v = v + rfn_dpp<0x108>(v); /* row_shl:8 */
  v = v + rfn_dpp<0x104>(v);
  v = v + rfn_dpp<0x102>(v);
  v = v + rfn_dpp<0x101>(v);
  return v;
}

/* grid: jobs; RFN_BLOCK threads */
__global__ __launch_bounds__(RFN_BLOCK) void k_rfn_refine(RfnArgs a) {
  __shared__ double s_tile[RFN_TILE * ICP_ENTRIES];
  __shared__ double s_tot[ICP_ENTRIES];
  __shared__ double s_T[16], s_c0[3];
  __shared__ uint32_t s_cnt[RFN_WAVES][3]; /* finite model rows; considered; pairs */
  __shared__ int s_status;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RfnJob& J = a.jobs[blockIdx.x];
  const float* __restrict__ model = J.model;
  const int n_rows = J.n_rows, n_chunks = (n_rows + ICP_CHUNK - 1) / ICP_CHUNK;
  double* __restrict__ parts = a.parts + J.o_parts;

  /* ---- c0: the mean of the finite scored rows, in model coordinates ---- */
  {
    uint32_t n_fin = 0;
    for (int c = wave; c < n_chunks; c += RFN_WAVES) {
      const int j = c * ICP_CHUNK + lane;
      double v[3] = {0.0, 0.0, 0.0};
      bool fin = false;
      if (j < n_rows) {
        const float* p = model + (size_t)j * a.step * 6;
        fin = vfy_finite6(p);
        if (fin) { v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2]; }
      }
      n_fin += (uint32_t)__popcll(__ballot(fin));
#pragma unroll
      for (int e = 0; e < 3; e++) {
        const double s = rfn_wave_sum(v[e]);
        if (lane == 0) parts[(size_t)c * 3 + e] = s;
      }
    }
    if (lane == 0) s_cnt[wave][0] = n_fin;
  }
  __syncthreads();
  {
    const double acc = icp_sum_staged<3, RFN_TILE_C0>(parts, n_chunks, s_tile, tid, RFN_BLOCK);
    uint32_t n_fin = 0;
    for (int w = 0; w < RFN_WAVES; w++) n_fin += s_cnt[w][0];
    if (tid < 3) s_c0[tid] = n_fin ? acc / (double)n_fin : 0.0;
    if (tid < 16) s_T[tid] = J.T[tid];
  }
  __syncthreads(); /* also: nobody reads the c0 partials any more */

  int32_t iterations = 0, n_cons_last = 0, n_pairs_first = 0, n_pairs_last = 0; /* thread 0's */
  float rmse_first = 0.f, rmse_last = 0.f;
  for (int k = 0;; k++) {
    double T[16], ck[3];
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = s_T[e];
#pragma unroll
    for (int r = 0; r < 3; r++) ck[r] = T[r * 4] * s_c0[0] + T[r * 4 + 1] * s_c0[1] + T[r * 4 + 2] * s_c0[2] + T[r * 4 + 3];
    /* ---- evaluation k: the chunks' partial rows ---- */
    uint32_t n_cons = 0, n_pairs = 0;
    for (int c = wave; c < n_chunks; c += RFN_WAVES) {
      const int j = c * ICP_CHUNK + lane;
      bool cons = false, pair = false;
      double Jv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
      if (j < n_rows) {
        const float* p = model + (size_t)j * a.step * 6;
        float o[6];
        icp_transform_row(p, p + 3, T, o);
        if (vfy_finite6(o)) {
          const double facing = (double)o[3] * (double)o[0] + (double)o[4] * (double)o[1] + (double)o[5] * (double)o[2];
          cons = facing < 0.0;
        }
        if (cons && o[2] > 0.f) {
          const double uf = (double)o[0] * a.fx / (double)o[2] + a.ppx;
          const double vf = (double)o[1] * a.fy / (double)o[2] + a.ppy;
          const double ui = floor(uf + 0.5), vi = floor(vf + 0.5);
          if (ui >= 0.0 && ui < (double)a.cols && vi >= 0.0 && vi < (double)a.rows) {
            const float d = a.depth[(size_t)(int)vi * a.cols + (int)ui];
            if (isfinite(d) && d > 0.f && fabsf(d - o[2]) <= a.gate) {
              pair = true;
              const double dd = (double)d;
              const double q[3] = {(ui - a.ppx) * dd / a.fx, (vi - a.ppy) * dd / a.fy, dd};
              const double pp[3] = {(double)o[0], (double)o[1], (double)o[2]}, n[3] = {(double)o[3], (double)o[4], (double)o[5]};
              const double av[3] = {pp[0] - ck[0], pp[1] - ck[1], pp[2] - ck[2]};
              r = n[0] * (q[0] - pp[0]) + n[1] * (q[1] - pp[1]) + n[2] * (q[2] - pp[2]);
              Jv[0] = av[1] * n[2] - av[2] * n[1];
              Jv[1] = av[2] * n[0] - av[0] * n[2];
              Jv[2] = av[0] * n[1] - av[1] * n[0];
              Jv[3] = n[0]; Jv[4] = n[1]; Jv[5] = n[2];
            }
          }
        }
      }
      n_cons += (uint32_t)__popcll(__ballot(cons));
      n_pairs += (uint32_t)__popcll(__ballot(pair));
      double* row = parts + (size_t)c * ICP_ENTRIES;
      int e = 0;
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int jj = i; jj < 6; jj++) {
          const double s = rfn_wave_sum(Jv[i] * Jv[jj]);
          if (lane == 0) row[e] = s;
          e++;
        }
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const double s = rfn_wave_sum(Jv[i] * r);
        if (lane == 0) row[21 + i] = s;
      }
      {
        const double s = rfn_wave_sum(r * r);
        if (lane == 0) row[27] = s;
      }
    }
    if (lane == 0) { s_cnt[wave][1] = n_cons; s_cnt[wave][2] = n_pairs; }
    __syncthreads();
    /* ---- the 28 sums in chunk order ---- */
    const double acc = icp_sum_staged<ICP_ENTRIES, RFN_TILE>(parts, n_chunks, s_tile, tid, RFN_BLOCK);
    if (tid < ICP_ENTRIES) s_tot[tid] = acc;
    __syncthreads();
    /* ---- the step (wave 0) ---- */
    if (wave == 0) {
      uint32_t nc = 0, np = 0;
      for (int w = 0; w < RFN_WAVES; w++) { nc += s_cnt[w][1]; np += s_cnt[w][2]; }
      int status = 0;
      if ((int)np < a.min_pairs || (double)np < (double)a.min_pair_share * (double)nc) status = PPF_REFINE_LOST;
      double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      bool ok = false;
      if (!status) ok = icp_solve6_wave(s_tot, lane, x); /* uniform over the wave */
      if (lane == 0) {
        n_cons_last = (int32_t)nc;
        n_pairs_last = (int32_t)np;
        rmse_last = np ? (float)ppf_sqrt(s_tot[27] / (double)np) : 0.f;
        if (k == 0) { n_pairs_first = n_pairs_last; rmse_first = rmse_last; }
        if (!status) {
          const double ww = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], tt = x[3] * x[3] + x[4] * x[4] + x[5] * x[5];
          bool fin = ok;
#pragma unroll
          for (int i = 0; i < 6; i++) fin = fin && isfinite(x[i]);
          if (!fin || ww > a.max_rot2 || tt > a.max_trans2) {
            status = PPF_REFINE_STEP;
          } else {
            const double zero[3] = {0.0, 0.0, 0.0};
            double M[16], Tn[16];
            icp_transform_from_euler(x, zero, M);
#pragma unroll
            for (int i = 0; i < 3; i++)
              M[i * 4 + 3] = (ck[i] + x[3 + i]) - (M[i * 4] * ck[0] + M[i * 4 + 1] * ck[1] + M[i * 4 + 2] * ck[2]);
            ppf_mat44_mul(M, T, Tn);
#pragma unroll
            for (int e = 0; e < 16; e++) s_T[e] = Tn[e];
            iterations = k + 1;
            if (ww <= a.eps_rot2 && tt <= a.eps_trans2) status = PPF_REFINE_CONVERGED;
            else if (k + 1 == a.max_iters) status = PPF_REFINE_MAX_ITERS;
          }
        }
        s_status = status;
      }
    }
    __syncthreads();
    if (s_status) break;
  }
  if (tid != 0) return;
  RfnOut& O = a.out[blockIdx.x];
#pragma unroll
  for (int e = 0; e < 16; e++) O.T[e] = s_T[e];
  O.info.status = s_status;
  O.info.iterations = iterations;
  O.info.n_rows = n_rows;
  O.info.n_considered = n_cons_last;
  O.info.n_pairs_first = n_pairs_first;
  O.info.n_pairs_last = n_pairs_last;
  O.info.rmse_first = rmse_first;
  O.info.rmse_last = rmse_last;
  O.info.reserved[0] = O.info.reserved[1] = O.info.reserved[2] = O.info.reserved[3] = 0;
}

#endif /* PPF_REFINE_KERNELS_H */
