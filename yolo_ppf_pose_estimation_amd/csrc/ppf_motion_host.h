/*
 * ppf_motion_host.h — host side of ppf_depth_motion / ppf_depth_motion_device: the camera's motion between two depth images
 * (DESIGN.md §28).  Kernels: ppf_motion_kernels.h.  Included by ppf_hip.hip after ppf_depthimage_host.h (the image check, the
 * bindings, stage_finish, stage_entry, depth_typed).
 *
 * Per call: k_motion_level0, levels - 1 k_motion_down, levels k_motion_maps, then per level from the coarsest and per
 * evaluation k < iters[l]: k_motion_eval, k_motion_group while more than DM_TAIL_MAX partial rows are left (and once when
 * more than 64 are), k_motion_tail -- all enqueued ahead, whatever the images hold -- and one blocking wait that also brings
 * the state back.  A level with iters[l] == 0 gets one k_motion_tail that marks it.  The host entry adds the two uploads.
 * Scratch (the pyramids, the records, the partials, the state) is one block from the block cache.
 */
#ifndef PPF_MOTION_HOST_H
#define PPF_MOTION_HOST_H

namespace {

struct MotionPlan {
  int levels;
  int rows[PPF_MOTION_MAX_LEVELS], cols[PPF_MOTION_MAX_LEVELS];
  size_t o_z[2][PPF_MOTION_MAX_LEVELS], o_rec[2][PPF_MOTION_MAX_LEVELS], o_parts[2], o_counts[2], o_state, bytes;
  int n_launches, n_enqueued;
};

/* partial rows left after the group stages of an evaluation over n_chunks chunks, and how many stages that takes */
int motion_group_stages(int n_chunks, int* left) {
  int n = n_chunks, stages = 0;
  if (n > 64) do {
      n = (n + 63) / 64;
      stages++;
    } while (n > DM_TAIL_MAX);
  *left = n;
  return stages;
}

/* the level sizes, the scratch layout and the launch count: a function of the size and mp alone */
void motion_plan(int rows, int cols, const ppf_depth_motion_params* mp, MotionPlan* P) {
  P->levels = mp->levels;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  for (int l = 0; l < PPF_MOTION_MAX_LEVELS; l++) {
    P->rows[l] = l ? P->rows[l - 1] / 2 : rows;
    P->cols[l] = l ? P->cols[l - 1] / 2 : cols;
  }
  for (int i = 0; i < 2; i++)
    for (int l = 0; l < mp->levels; l++) {
      const size_t n = (size_t)P->rows[l] * (size_t)P->cols[l];
      P->o_z[i][l] = take(n * sizeof(float));
      P->o_rec[i][l] = take(n * sizeof(float4));
    }
  const size_t chunks0 = ((size_t)rows * (size_t)cols + 63) / 64, chunks1 = (chunks0 + 63) / 64;
  P->o_parts[0] = take(chunks0 * ICP_ENTRIES * sizeof(double));
  P->o_parts[1] = take(chunks1 * ICP_ENTRIES * sizeof(double));
  P->o_counts[0] = take(chunks0 * sizeof(uint32_t));
  P->o_counts[1] = take(chunks1 * sizeof(uint32_t));
  P->o_state = take(sizeof(MotionState));
  P->bytes = at;
  P->n_launches = 1 + (mp->levels - 1) + mp->levels;
  P->n_enqueued = 0;
  for (int l = 0; l < mp->levels; l++) {
    int left;
    const int stages = motion_group_stages((int)(((long long)P->rows[l] * P->cols[l] + 63) / 64), &left);
    P->n_launches += mp->iters[l] == 0 ? 1 : mp->iters[l] * (2 + stages);
    P->n_enqueued += mp->iters[l];
  }
}

void motion_start(const double* init16, double* T) {
  static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(T, init16 ? init16 : eye, sizeof(eye));
}

/* every argument check of both entries, before any device work; fills both images' kernel arguments (img excepted) */
ppf_status motion_check(const char* who, const void* prev, size_t prev_pitch, const void* cur, size_t cur_pitch, int rows, int cols,
                        const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp, const double* init16,
                        const double* pose16, DepthArgs* a0, DepthArgs* a1) {
  if (!pose16) return fail(PPF_ERR_INVALID, "%s: pose16 is NULL", who);
  if (!mp) return fail(PPF_ERR_INVALID, "%s: the motion params are NULL", who);
  if (!dp || !intr) return fail(PPF_ERR_INVALID, "%s: depth, intr and params must not be NULL", who);
  const std::string w0 = std::string(who) + " (prev)", w1 = std::string(who) + " (cur)";
  ppf_status s;
  if ((s = depth_image_check(w0.c_str(), prev, rows, cols, prev_pitch, dp, DEPTH_FLAGS_IGNORED, a0)) != PPF_OK ||
      (s = depth_image_check(w1.c_str(), cur, rows, cols, cur_pitch, dp, DEPTH_FLAGS_IGNORED, a1)) != PPF_OK ||
      (s = depth_intr_check(who, intr, a0)) != PPF_OK || (s = depth_intr_check(who, intr, a1)) != PPF_OK)
    return s;
  for (int i = 0; init16 && i < 16; i++)
    if (!std::isfinite(init16[i])) return fail(PPF_ERR_INVALID, "%s: init16 must be finite", who);
  if (mp->levels < 1 || mp->levels > PPF_MOTION_MAX_LEVELS)
    return fail(PPF_ERR_INVALID, "%s: levels %d is outside 1..%d", who, mp->levels, PPF_MOTION_MAX_LEVELS);
  for (int l = 0; l < PPF_MOTION_MAX_LEVELS; l++)
    if (mp->iters[l] < 0 || mp->iters[l] > PPF_MOTION_MAX_ITERS)
      return fail(PPF_ERR_INVALID, "%s: iters[%d] = %d is outside 0..%d", who, l, mp->iters[l], PPF_MOTION_MAX_ITERS);
  if (!(std::isfinite(mp->pyr_gate) && mp->pyr_gate > 0.f)) return fail(PPF_ERR_INVALID, "%s: pyr_gate must be finite and > 0", who);
  if (!(std::isfinite(mp->normal_gate) && mp->normal_gate > 0.f)) return fail(PPF_ERR_INVALID, "%s: normal_gate must be finite and > 0", who);
  if (!(std::isfinite(mp->dist_gate) && mp->dist_gate > 0.f)) return fail(PPF_ERR_INVALID, "%s: dist_gate must be finite and > 0", who);
  if (!(mp->normal_cos >= -1.f && mp->normal_cos <= 1.f)) return fail(PPF_ERR_INVALID, "%s: normal_cos must be in [-1, 1]", who);
  if (!(std::isfinite(mp->max_step_rot) && mp->max_step_rot > 0.f)) return fail(PPF_ERR_INVALID, "%s: max_step_rot must be finite and > 0", who);
  if (!(std::isfinite(mp->max_step_trans) && mp->max_step_trans > 0.f))
    return fail(PPF_ERR_INVALID, "%s: max_step_trans must be finite and > 0", who);
  if (!(std::isfinite(mp->eps_rot) && mp->eps_rot >= 0.f)) return fail(PPF_ERR_INVALID, "%s: eps_rot must be finite and >= 0", who);
  if (!(std::isfinite(mp->eps_trans) && mp->eps_trans >= 0.f)) return fail(PPF_ERR_INVALID, "%s: eps_trans must be finite and >= 0", who);
  if (!(mp->min_pair_share >= 0.f && mp->min_pair_share <= 1.f)) return fail(PPF_ERR_INVALID, "%s: min_pair_share must be in [0, 1]", who);
  if (mp->min_pairs < 6) return fail(PPF_ERR_INVALID, "%s: min_pairs must be >= 6", who);
  if (mp->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown motion flags 0x%x", who, (unsigned)mp->flags);
  if ((rows >> (mp->levels - 1)) < 1 || (cols >> (mp->levels - 1)) < 1)
    return fail(PPF_ERR_INVALID, "%s: a %d x %d image has no level %d", who, rows, cols, mp->levels - 1);
  return PPF_OK;
}

/* every launch of a call, on `st`; a0.img / a1.img and the pitches are bound, `base` is the call's scratch */
ppf_status motion_enqueue(const DepthArgs& a0, const DepthArgs& a1, int format, const ppf_depth_motion_params* mp, const double* T0,
                          const MotionPlan& P, unsigned char* base, hipStream_t st) {
  MotionState* S = reinterpret_cast<MotionState*>(base + P.o_state);
  MotionLvl L[PPF_MOTION_MAX_LEVELS];
  for (int l = 0; l < P.levels; l++) {
    L[l].level = l;
    L[l].rows = P.rows[l];
    L[l].cols = P.cols[l];
    L[l].n = P.rows[l] * P.cols[l];
    L[l].fx = l ? L[l - 1].fx / 2.0 : a0.fx;
    L[l].fy = l ? L[l - 1].fy / 2.0 : a0.fy;
    L[l].ppx = l ? (L[l - 1].ppx - 0.5) / 2.0 : a0.ppx;
    L[l].ppy = l ? (L[l - 1].ppy - 0.5) / 2.0 : a0.ppy;
    L[l].ngate = (double)mp->normal_gate * (double)(1 << l);
    L[l].z0 = reinterpret_cast<const float*>(base + P.o_z[0][l]);
    L[l].z1 = reinterpret_cast<const float*>(base + P.o_z[1][l]);
    L[l].rec0 = reinterpret_cast<float4*>(base + P.o_rec[0][l]);
    L[l].rec1 = reinterpret_cast<float4*>(base + P.o_rec[1][l]);
  }
  MotionRun R;
  R.dist2 = (double)mp->dist_gate * (double)mp->dist_gate;
  R.normal_cos = (double)mp->normal_cos;
  R.min_pair_share = (double)mp->min_pair_share;
  R.max_rot2 = (double)mp->max_step_rot * (double)mp->max_step_rot;
  R.max_trans2 = (double)mp->max_step_trans * (double)mp->max_step_trans;
  R.eps_rot2 = (double)mp->eps_rot * (double)mp->eps_rot;
  R.eps_trans2 = (double)mp->eps_trans * (double)mp->eps_trans;
  R.min_pairs = mp->min_pairs;
  R.pad = 0;
  R.state = S;
  double* parts[2] = {reinterpret_cast<double*>(base + P.o_parts[0]), reinterpret_cast<double*>(base + P.o_parts[1])};
  uint32_t* counts[2] = {reinterpret_cast<uint32_t*>(base + P.o_counts[0]), reinterpret_cast<uint32_t*>(base + P.o_counts[1])};
  {
    MotionInit init;
    std::memcpy(init.T, T0, sizeof(init.T));
    const int groups = (int)(((long long)a0.cols + DH_PX - 1) / DH_PX);
    const size_t quad = depth_elem_size(format) * DH_PX; /* 16 or 8 bytes */
    const int in_vec0 = ((uintptr_t)a0.img % quad == 0 && a0.pitch % quad == 0) ? 1 : 0;
    const int in_vec1 = ((uintptr_t)a1.img % quad == 0 && a1.pitch % quad == 0) ? 1 : 0;
    const int out_vec = a0.cols % DH_PX == 0 ? 1 : 0; /* the scratch planes start on 256-byte boundaries */
    /* rows * ceil(cols / 4) lanes: at most rows * cols <= INT32_MAX, so the grid is below 2^23 workgroups */
    const long long lanes = (long long)P.rows[0] * groups;
    const dim3 grid((unsigned)((lanes + DM_BLOCK - 1) / DM_BLOCK), 2);
    depth_typed(format, [&](auto px) {
      k_motion_level0<decltype(px)><<<grid, dim3(DM_BLOCK), 0, st>>>(a0, a1, in_vec0, in_vec1, P.rows[0], groups, const_cast<float*>(L[0].z0),
                                                                      const_cast<float*>(L[0].z1), out_vec, S, init);
    });
    HIPCHK(hipGetLastError());
  }
  for (int l = 1; l < P.levels; l++) {
    const dim3 grid((unsigned)(((long long)L[l].n + DM_BLOCK - 1) / DM_BLOCK), 2);
    k_motion_down<<<grid, dim3(DM_BLOCK), 0, st>>>(L[l - 1].z0, L[l - 1].z1, const_cast<float*>(L[l].z0), const_cast<float*>(L[l].z1),
                                                   L[l - 1].cols, L[l].rows, L[l].cols, (double)mp->pyr_gate);
    HIPCHK(hipGetLastError());
  }
  for (int l = 0; l < P.levels; l++) {
    /* the tiles as one grid dimension: at most n / 256 + rows / 16 + cols / 16 + 1 workgroups, below 2^31 */
    const int tx = (L[l].cols + DM_TILE - 1) / DM_TILE, ty = (L[l].rows + DM_TILE - 1) / DM_TILE;
    k_motion_maps<<<dim3((unsigned)((long long)tx * ty), 2), dim3(DM_BLOCK), 0, st>>>(L[l], tx, S);
    HIPCHK(hipGetLastError());
  }
  for (int l = P.levels - 1; l >= 0; l--) {
    const int n_chunks = (int)(((long long)L[l].n + 63) / 64);
    if (mp->iters[l] == 0) {
      k_motion_tail<<<dim3(1), dim3(DM_TAIL_BLOCK), 0, st>>>(L[l], R, parts[0], counts[0], 0, 0, 0);
      HIPCHK(hipGetLastError());
      continue;
    }
    for (int k = 0; k < mp->iters[l]; k++) {
      k_motion_eval<<<dim3((unsigned)((n_chunks + DM_WAVES - 1) / DM_WAVES)), dim3(DM_BLOCK), 0, st>>>(L[l], R, parts[0], counts[0]);
      int n = n_chunks, at = 0;
      if (n > 64) do {
          const int n_out = (n + 63) / 64;
          const long long waves = (long long)n_out * DM_COMPONENTS;
          k_motion_group<<<dim3((unsigned)((waves + DM_WAVES - 1) / DM_WAVES)), dim3(DM_BLOCK), 0, st>>>(S, l, mp->min_pairs, parts[at], counts[at], n,
                                                                                                        parts[at ^ 1], counts[at ^ 1], n_out);
          n = n_out;
          at ^= 1;
        } while (n > DM_TAIL_MAX);
      k_motion_tail<<<dim3(1), dim3(DM_TAIL_BLOCK), 0, st>>>(L[l], R, parts[at], counts[at], n, k, mp->iters[l]);
      HIPCHK(hipGetLastError());
    }
  }
  return PPF_OK;
}

void motion_report(const MotionState& S, const MotionPlan& P, double* pose16, ppf_depth_motion_level* level_rows, ppf_depth_motion_stats& st) {
  std::memcpy(pose16, S.T, sizeof(S.T));
  if (level_rows) std::memcpy(level_rows, S.rows, sizeof(S.rows));
  st.status = S.last_status;
  st.n_evaluations = S.n_evaluations;
  st.n_enqueued = P.n_enqueued;
  st.n_launches = P.n_launches;
  st.n_host_syncs = 1;
}

ppf_status motion_host(const char* who, const void* prev, size_t prev_pitch, const void* cur, size_t cur_pitch, int rows, int cols,
                       const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp, const double* init16, double* pose16,
                       ppf_depth_motion_level* level_rows, ppf_depth_motion_stats& st) {
  DepthArgs a0, a1;
  ppf_status s = motion_check(who, prev, prev_pitch, cur, cur_pitch, rows, cols, intr, dp, mp, init16, pose16, &a0, &a1);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  MotionPlan P;
  motion_plan(rows, cols, mp, &P);
  DevBuf<unsigned char> img0, img1, scratch;
  if ((s = depth_bind_host(prev, dp->format, img0, &a0)) != PPF_OK || (s = depth_bind_host(cur, dp->format, img1, &a1)) != PPF_OK) return s;
  HIPCHK(scratch.reserve(P.bytes));
  double T0[16];
  motion_start(init16, T0);
  MotionState S;
  s = stage_finish(who, motion_enqueue(a0, a1, dp->format, mp, T0, P, scratch.p, nullptr), nullptr,
                   {{"state", scratch.p + P.o_state, sizeof(S), &S}});
  if (s == PPF_OK) motion_report(S, P, pose16, level_rows, st);
  return s;
}

ppf_status motion_device(const char* who, const void* d_prev, size_t prev_pitch, const void* d_cur, size_t cur_pitch, int rows, int cols,
                         const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp, const double* init16,
                         hipStream_t stream, double* pose16, ppf_depth_motion_level* level_rows, ppf_depth_motion_stats& st) {
  DepthArgs a0, a1;
  StageBuf image0, image1;
  ppf_status s = motion_check(who, d_prev, prev_pitch, d_cur, cur_pitch, rows, cols, intr, dp, mp, init16, pose16, &a0, &a1);
  if (s != PPF_OK) return s;
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  const std::string w0 = std::string(who) + " (prev)", w1 = std::string(who) + " (cur)";
  if ((s = depth_bind_device(w0.c_str(), d_prev, dp->format, &a0, &image0)) != PPF_OK ||
      (s = depth_bind_device(w1.c_str(), d_cur, dp->format, &a1, &image1)) != PPF_OK)
    return s;
  if (ranges_overlap(image0, image1)) return fail(PPF_ERR_INVALID, "%s: the two images overlap", who);
  MotionPlan P;
  motion_plan(rows, cols, mp, &P);
  DevBuf<unsigned char> scratch;
  HIPCHK(scratch.reserve(P.bytes));
  double T0[16];
  motion_start(init16, T0);
  MotionState S;
  s = stage_finish(who, motion_enqueue(a0, a1, dp->format, mp, T0, P, scratch.p, stream), stream,
                   {{"state", scratch.p + P.o_state, sizeof(S), &S}});
  if (s == PPF_OK) motion_report(S, P, pose16, level_rows, st);
  return s;
}

/* what a failed call leaves: pose16 = the start as given (pose16 may be init16 itself), the rows zero */
void motion_clear(const double* init16, double* pose16, ppf_depth_motion_level* level_rows) {
  if (pose16) {
    double T[16];
    motion_start(init16, T);
    std::memcpy(pose16, T, sizeof(T));
  }
  if (level_rows) std::memset(level_rows, 0, sizeof(ppf_depth_motion_level) * PPF_MOTION_MAX_LEVELS);
}

}  // namespace

extern "C" {

void ppf_default_depth_motion_params(ppf_depth_motion_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->levels = 3;
  p->iters[0] = 10;
  p->iters[1] = 5;
  p->iters[2] = 4;
  p->iters[3] = 4;
  p->pyr_gate = 0.03f;
  p->normal_gate = 0.01f;
  p->dist_gate = 0.05f;
  p->normal_cos = 0.8f;
  p->max_step_rot = 0.3f;
  p->max_step_trans = 0.15f;
  p->eps_rot = 1e-5f;
  p->eps_trans = 1e-5f;
  p->min_pair_share = 0.25f;
  p->min_pairs = 16;
  p->flags = 0;
}

ppf_status ppf_depth_motion(const void* prev, size_t prev_pitch_bytes, const void* cur, size_t cur_pitch_bytes, int rows, int cols,
                            const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp, const double* init16,
                            double* pose16, ppf_depth_motion_level* level_rows, ppf_depth_motion_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_depth_motion_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed) motion_clear(init16, pose16, level_rows);
      },
      [&](ppf_depth_motion_stats& st) {
        return motion_host("ppf_depth_motion", prev, prev_pitch_bytes, cur, cur_pitch_bytes, rows, cols, intr, dp, mp, init16, pose16, level_rows, st);
      });
}

ppf_status ppf_depth_motion_device(const void* d_prev, size_t prev_pitch_bytes, const void* d_cur, size_t cur_pitch_bytes, int rows,
                                   int cols, const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp,
                                   const double* init16, void* stream, double* pose16, ppf_depth_motion_level* level_rows,
                                   ppf_depth_motion_stats* stats) {
  return stage_entry(
      stats,
      [&](ppf_depth_motion_stats& st, bool failed) {
        std::memset(&st, 0, sizeof(st));
        if (failed) motion_clear(init16, pose16, level_rows);
      },
      [&](ppf_depth_motion_stats& st) {
        return motion_device("ppf_depth_motion_device", d_prev, prev_pitch_bytes, d_cur, cur_pitch_bytes, rows, cols, intr, dp, mp, init16,
                             static_cast<hipStream_t>(stream), pose16, level_rows, st);
      });
}

}  // extern "C"

#endif /* PPF_MOTION_HOST_H */
