/*
 * ppf_icp_host.h — host side of the ICP refinement (row N2): the batched runner (every pose of a call is a job; all jobs
 * advance level by level through the same launches, kernels k_icp2_*) and the C-ABI entry points ppf_icp_refine /
 * ppf_icp_refine_device / ppf_icp_register (+ the edge helpers ppf_sample_cloud / ppf_transform_pc_pose, which run on the
 * device too).  Kernels: ppf_icp_kernels.h.
 * Included by ppf_hip.hip (one translation unit: shares DevBuf, fail(), HIPCHK and the kernels above).
 */
/* ============================================================================================ */
/* ICP refinement (row N2; kernels in ppf_icp_kernels.h)                                          */
/* ============================================================================================ */
namespace {

#ifndef PPF_ICP_NN_WAVES
#define PPF_ICP_NN_WAVES 65536   /* waves of the neighbour search beyond which a wave takes several rows */
#endif
#ifndef PPF_ICP_BATCH2
#define PPF_ICP_BATCH2 2         /* passes (two launches each) kept in the stream ahead of the device (1: 3.30 ms, 2: 3.16 - 3.20, 3: 3.25 ms of ICP on C1) */
#endif

inline long icp_round(double v) { return std::lrint(v); } /* cvRound */

struct IcpBatchScratch {
  DevBuf<float> src0, dst0, src_pct;
  DevBuf<unsigned long long> best, owner;
  DevBuf<int2> sel;
  DevBuf<double> parts, sum_src, sum_dst;
  DevBuf<float4> g_pts, g_box2;
  DevBuf<uint32_t> g_start, g_cur, g_box1u, own_a;
  DevBuf<float> bb_parts;
  DevBuf<IcpState2> state;
  DevBuf<unsigned char> tables;  /* the call's IcpJobDesc table, then its IcpLevelDesc table */
  int host_jobs = 0, host_table_bytes = 0; /* capacity of the pinned buffers below */
  int* h_done = nullptr;        /* pinned: one flag per job, written by the kernels */
  IcpState2* h_state = nullptr; /* pinned: the jobs' loop states, written by the kernels when a level ends */
  unsigned long long* h_ticks = nullptr; /* pinned: finished k_icp2_tail workgroups of the running call */
  unsigned char* h_tables = nullptr;     /* pinned staging of `tables` */
  ~IcpBatchScratch() {
    if (h_done) (void)hipHostFree(h_done);
    if (h_state) (void)hipHostFree(h_state);
    if (h_ticks) (void)hipHostFree(h_ticks);
    if (h_tables) (void)hipHostFree(h_tables);
  }
};

/* one registration of a batched call: its clouds (rows of stride floats, normal at noff) and its initial pose (NULL: the
 * identity) */
struct IcpJobSpec {
  const float* src;
  int n, sstride, snoff;
  const float* dst;
  int nd_all, dstride, dnoff;
  const double* init;
};

/* what a batched call enqueued (ppf_match_frame_stats) */
struct IcpRunCount {
  int launches = 0, passes = 0, syncs = 0;
};

/* ICP::registerModelToScene's level schedule for a source of n rows and a destination of nd_all rows */
IcpLevelDesc icp_level_desc(int n, int nd_all, int level) {
  const double div = std::pow(2.0, (double)level);
  const int num_samples = (int)icp_round((double)n / div);
  const int step = std::max(1, (int)icp_round((double)n / (double)std::max(num_samples, 1)));
  IcpLevelDesc L;
  memset(&L, 0, sizeof(L));
  L.step = step;
  L.ns = (n + step - 1) / step;
  L.nd = (nd_all + step - 1) / step;
  L.step_shift = -1;
  if ((step & (step - 1)) == 0) { L.step_shift = 0; while ((1 << L.step_shift) < step) L.step_shift++; }
  L.staged = L.ns <= 32768 ? 1 : 0; /* the level's distances fit LDS (4 bytes each): the selection passes read them there */
  return L;
}

/* registerModelToScene for `jobs` (<= ICP_GROUP_JOBS) registrations at once, each with its own clouds and initial pose:
 * every launch covers all jobs (sized for the largest), an iteration is two launches (k_icp2_nn, k_icp2_tail), the host
 * keeps PPF_ICP_BATCH2 of them in the stream ahead of the device and reads the jobs' done flags whenever one reports.  The
 * level loop is lock-step over the jobs: a level ends when every job is done with it.  Everything runs on `st`. */
ppf_status icp_register_group(const IcpJobSpec* specs, int jobs, const ppf_icp_params& prm, IcpBatchScratch& sc, hipStream_t st,
                              double* poses_out /* jobs x 16 */, double* residuals, int* iters_total, IcpRunCount& cnt) {
  const int nl_levels = std::max(prm.num_levels, 0);
  const size_t J = (size_t)jobs;
  const size_t levels_off = J * sizeof(IcpJobDesc);
  const size_t table_bytes = levels_off + J * (size_t)std::max(nl_levels, 1) * sizeof(IcpLevelDesc);
  static_assert(sizeof(IcpJobDesc) % 16 == 0, "the level table follows the job table 16-byte aligned");
  if (sc.host_jobs < jobs) {
    if (sc.h_done) { (void)hipHostFree(sc.h_done); sc.h_done = nullptr; }
    if (sc.h_state) { (void)hipHostFree(sc.h_state); sc.h_state = nullptr; }
    sc.host_jobs = 0;
    HIPCHK(hipHostMalloc((void**)&sc.h_done, std::max(jobs, ICP_MAX_JOBS) * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void**)&sc.h_state, std::max(jobs, ICP_MAX_JOBS) * sizeof(IcpState2), hipHostMallocDefault));
    sc.host_jobs = std::max(jobs, ICP_MAX_JOBS);
  }
  if ((size_t)sc.host_table_bytes < table_bytes) {
    if (sc.h_tables) { (void)hipHostFree(sc.h_tables); sc.h_tables = nullptr; }
    sc.host_table_bytes = 0;
    HIPCHK(hipHostMalloc((void**)&sc.h_tables, table_bytes, hipHostMallocDefault));
    sc.host_table_bytes = (int)table_bytes;
  }
  if (!sc.h_ticks) HIPCHK(hipHostMalloc((void**)&sc.h_ticks, 64, hipHostMallocDefault));
  /* the tables: every job's place in the shared scratch arrays, its initial pose, its level schedule */
  IcpJobDesc* jd = reinterpret_cast<IcpJobDesc*>(sc.h_tables);
  IcpLevelDesc* ld = reinterpret_cast<IcpLevelDesc*>(sc.h_tables + levels_off);
  size_t t_src = 0, t_dst = 0, t_sel = 0, t_parts = 0, t_sums = 0, t_sumd = 0;
  int max_n = 0, max_nd = 0, max_chunks = 0, max_rows_blocks = 0, max_dst_blocks = 0;
  for (int j = 0; j < jobs; j++) {
    const IcpJobSpec& S = specs[j];
    IcpJobDesc& D = jd[j];
    memset(&D, 0, sizeof(D));
    D.src = S.src; D.dst = S.dst;
    D.n = S.n; D.sstride = S.sstride; D.snoff = S.snoff; D.nd_all = S.nd_all; D.dstride = S.dstride; D.dnoff = S.dnoff;
    D.has_init = S.init ? 1 : 0;
    for (int k = 0; k < 16; k++) D.T0[k] = S.init ? S.init[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    const size_t chunks_src = ((size_t)S.n + ICP_CHUNK - 1) / ICP_CHUNK, chunks_dst = ((size_t)S.nd_all + ICP_CHUNK - 1) / ICP_CHUNK;
    const size_t m = (size_t)std::min(S.n, S.nd_all);
    D.o_src0 = t_src * 6; D.o_best = t_src; D.o_dst0 = t_dst * 6; D.o_owner = t_dst;
    D.o_sel = t_sel; D.o_parts = t_parts; D.o_sums = t_sums; D.o_sumd = t_sumd;
    t_src += (size_t)S.n; t_dst += (size_t)S.nd_all; t_sel += m; t_parts += (m + ICP_CHUNK - 1) / ICP_CHUNK * ICP_ENTRIES;
    t_sums += chunks_src * 3; t_sumd += chunks_dst * 3;
    max_n = std::max(max_n, S.n); max_nd = std::max(max_nd, S.nd_all);
    max_chunks = std::max(max_chunks, (int)(chunks_src + chunks_dst));
    const int nb_dst = (S.nd_all + ICP_ROWS_BLOCK - 1) / ICP_ROWS_BLOCK, nb_src = (S.n + ICP_ROWS_BLOCK - 1) / ICP_ROWS_BLOCK;
    max_rows_blocks = std::max(max_rows_blocks, nb_dst + nb_src);
    max_dst_blocks = std::max(max_dst_blocks, nb_dst);
    for (int level = 0; level < nl_levels; level++) ld[(size_t)j * nl_levels + level] = icp_level_desc(S.n, S.nd_all, level);
  }
  HIPCHK(sc.src0.reserve(t_src * 6));
  HIPCHK(sc.src_pct.reserve(t_src * 6));
  HIPCHK(sc.dst0.reserve(t_dst * 6));
  HIPCHK(sc.best.reserve(t_src));
  HIPCHK(sc.owner.reserve(t_dst));
  HIPCHK(sc.sel.reserve(t_sel));
  HIPCHK(sc.parts.reserve(t_parts));
  HIPCHK(sc.sum_src.reserve(t_sums));
  HIPCHK(sc.sum_dst.reserve(t_sumd));
  HIPCHK(sc.g_pts.reserve(t_dst));
  HIPCHK(sc.g_start.reserve(J * (ICP_LEAVES + 64)));
  HIPCHK(sc.g_cur.reserve(J * ICP_LEAVES));
  HIPCHK(sc.g_box2.reserve(J * ICP_LEAVES * 2));
  HIPCHK(sc.g_box1u.reserve(J * 64 * 8));
  HIPCHK(sc.own_a.reserve(t_dst));
  HIPCHK(sc.bb_parts.reserve(t_sumd * 2));
  HIPCHK(sc.state.reserve(std::max<size_t>(J, ICP_MAX_JOBS)));
  HIPCHK(sc.tables.reserve(table_bytes));
  *sc.h_ticks = 0ull; /* no kernel of an earlier call is running: every call ends with all of its launches accounted for, and an
                         error return drains the stream first (icp_batch_run) */
  IcpBatch B;
  memset(&B, 0, sizeof(B));
  B.jobs = reinterpret_cast<const IcpJobDesc*>(sc.tables.p);
  B.levels = reinterpret_cast<const IcpLevelDesc*>(sc.tables.p + levels_off);
  B.num_levels = nl_levels;
  B.src0 = sc.src0.p; B.dst0 = sc.dst0.p; B.src_pct = sc.src_pct.p;
  B.best = sc.best.p; B.owner = sc.owner.p; B.sel = sc.sel.p;
  B.parts = sc.parts.p; B.sum_src = sc.sum_src.p; B.sum_dst = sc.sum_dst.p;
  B.g_pts = sc.g_pts.p; B.g_start = sc.g_start.p; B.g_cur = sc.g_cur.p; B.g_box2 = sc.g_box2.p; B.g_box1u = sc.g_box1u.p; B.own_a = sc.own_a.p; B.bb_parts = sc.bb_parts.p;
  B.state = sc.state.p;
  B.h_done = sc.h_done;
  B.h_ticks = sc.h_ticks;
  B.h_state = sc.h_state;
  static std::once_flag once_tail;
  static hipError_t attr_tail = hipSuccess;
  std::call_once(once_tail, [] {
    attr_tail = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_icp2_tail<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
    if (attr_tail == hipSuccess)
      attr_tail = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_icp2_tail<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
  });
  HIPCHK(attr_tail);
  /* one pair of clouds for every job: the per-pass kernels take the geometry from their arguments (IcpUniform) */
  bool uniform = true;
  for (int j = 1; j < jobs; j++)
    uniform &= specs[j].src == specs[0].src && specs[j].n == specs[0].n && specs[j].sstride == specs[0].sstride &&
               specs[j].snoff == specs[0].snoff && specs[j].dst == specs[0].dst && specs[j].nd_all == specs[0].nd_all &&
               specs[j].dstride == specs[0].dstride && specs[j].dnoff == specs[0].dnoff;
  /* the tables go up once, through k_icp2_reset; the pinned staging is not touched again before the call has finished */
  static_assert(sizeof(IcpLevelDesc) % 16 == 0, "the tables are copied in 16-byte words");
  B.table_words = (uint32_t)(table_bytes / 16);
  B.h_tables = reinterpret_cast<const uint4*>(sc.h_tables);
  B.d_tables = reinterpret_cast<uint4*>(sc.tables.p);
  const unsigned uj = (unsigned)jobs;
  /* the two clouds packed (the source moved by its job's initial pose), centred on the average of the two means, scaled to
   * unit average distance from the origin; the search grid over each job's scene */
  k_icp2_reset<<<dim3(uj, 32), dim3(256), 0, st>>>(B);
  k_icp2_pack_sums<<<dim3((unsigned)max_chunks, uj), dim3(64), 0, st>>>(B);
  k_icp2_mean<<<dim3(uj), dim3(256), 0, st>>>(B);
  k_icp2_dist_sums<<<dim3((unsigned)max_chunks, uj), dim3(64), 0, st>>>(B);
  k_icp2_scale<<<dim3(uj), dim3(256), 0, st>>>(B);
  k_icp2_rows_count<<<dim3((unsigned)max_rows_blocks, uj), dim3(1024), 0, st>>>(B);
  k_icp2_grid_scan<<<dim3(uj), dim3(1024), 0, st>>>(B);
  k_icp2_grid_scatter<<<dim3((unsigned)max_dst_blocks, uj), dim3(1024), 0, st>>>(B);
  k_icp2_grid_boxes<<<dim3(ICP_LEAVES / 4, uj), dim3(256), 0, st>>>(B);
  cnt.launches += 9;
  HIPCHK(hipGetLastError());
  const int robust = prm.rejection_scale > 0 ? 1 : 0;
  unsigned long long tails_launched = 0;
  bool last_level_waited = false;
  auto wait_ticks = [&](const unsigned long long want) -> ppf_status {
    volatile unsigned long long* ticks = sc.h_ticks;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (*ticks < want) {
      __builtin_ia32_pause();
      if ((++spins & 0xFFFFu) == 0) {
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > 0.05 && hipStreamQuery(st) != hipErrorNotReady) { /* the stream is idle (or broken): nothing more will come */
          cnt.syncs++;
          HIPCHK(hipStreamSynchronize(st));
          if (*ticks < want) return fail(PPF_ERR_HIP, "ICP: %llu of %llu workgroups reported", (unsigned long long)*ticks, want);
        }
        if (waited > 30.0) return fail(PPF_ERR_HIP, "ICP: timed out waiting for the device");
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return PPF_OK;
  };
  for (int level = prm.num_levels - 1; level >= 0; level--) {
    const double tol_p = (double)prm.tolerance * (double)(level + 1) * (level + 1);
    const int max_iter = (int)icp_round((double)prm.iterations / (level + 1));
    /* launch shapes for the largest job of the level; the dynamic LDS of the tail is the most any job needs */
    int max_ns = 0;
    long long sum_ns = 0;
    size_t tail_lds = (size_t)ICP_TAIL_VAL_BYTES;
    for (int j = 0; j < jobs; j++) {
      const IcpLevelDesc& L = ld[(size_t)j * nl_levels + level];
      max_ns = std::max(max_ns, L.ns);
      sum_ns += L.ns;
      tail_lds = std::max(tail_lds, L.staged ? (size_t)L.ns * 4 : (size_t)0);
    }
    IcpUniform U;
    memset(&U, 0, sizeof(U));
    if (uniform) {
      const IcpLevelDesc& L = ld[level];
      U.ns = L.ns; U.nd = L.nd; U.step = L.step; U.step_shift = L.step_shift; U.staged = L.staged;
      U.n = specs[0].n; U.nd_all = specs[0].nd_all;
      U.p_sel = (size_t)std::min(specs[0].n, specs[0].nd_all);
      U.p_parts = (U.p_sel + ICP_CHUNK - 1) / ICP_CHUNK * ICP_ENTRIES;
    }
    k_icp2_level_begin<<<dim3((unsigned)((max_ns + 255) / 256), uj), dim3(256), 0, st>>>(B, level, tol_p, max_iter, robust, level == 0 ? 1 : 0);
    cnt.launches++;
    /* rows per wave of the neighbour search: one, unless that makes more waves than the chip holds several times over */
    const int nn_rows = (int)std::min<long long>(ICP_NN_ROWS, std::max<long long>(1, sum_ns / PPF_ICP_NN_WAVES));
    const unsigned nn_blocks = (unsigned)((max_ns + 4 * nn_rows - 1) / (4 * nn_rows));
    /* The passes of a level are launched ahead of the device: PPF_ICP_BATCH2 (neighbour search, tail) pairs are in the stream,
     * and every time the oldest of them reports, the next one is launched -- the device never waits for the host between
     * passes (with whole batches it idled ~11 us after every second pass).  Every k_icp2_tail workgroup, whatever it did,
     * adds one to a counter in pinned memory as its last act (after its done flag and, at the end of a level, its state);
     * polling that is a few microseconds quicker than going through the stream (which is only asked when the counter has
     * not moved for a long while).  A pass launched after the level's last one finds every job done and returns at once. */
    int launched = 0, reported = 0;
    unsigned long long due[PPF_ICP_BATCH2 + 1]; /* the counter's value when pass k has reported, k modulo the passes in the stream */
    bool first_of_level = true;
    while (true) {
      while (launched < max_iter && launched - reported < (int)PPF_ICP_BATCH2) {
        /* a pass is launched for the jobs that had not finished the level when the host last looked (all of them at its start);
         * the list travels as a kernel argument, copied at the launch */
        IcpLive live;
        unsigned nl = 0;
        for (int j = 0; j < jobs; j++)
          if (first_of_level || reinterpret_cast<volatile int*>(sc.h_done)[j] == 0) live.job[nl++] = (uint16_t)j;
        if (nl == 0) live.job[nl++] = 0; /* cannot happen: the loop ends when every job is done */
        const int brute_nd = (prm.flags & PPF_ICP_GRID_ALWAYS) ? 0 : ICP_BRUTE_ND;
        if (uniform) {
          k_icp2_nn<false><<<dim3(nn_blocks, nl), dim3(256), 0, st>>>(B, live, level, U, nn_rows, brute_nd);
          k_icp2_tail<false><<<dim3(nl), dim3(1024), tail_lds, st>>>(B, live, level, U, prm.rejection_scale, level == 0 ? 1 : 0);
        } else {
          k_icp2_nn<true><<<dim3(nn_blocks, nl), dim3(256), 0, st>>>(B, live, level, U, nn_rows, brute_nd);
          k_icp2_tail<true><<<dim3(nl), dim3(1024), tail_lds, st>>>(B, live, level, U, prm.rejection_scale, level == 0 ? 1 : 0);
        }
        cnt.launches += 2;
        cnt.passes++;
        tails_launched += (unsigned long long)nl;
        due[launched % (PPF_ICP_BATCH2 + 1)] = tails_launched;
        launched++;
      }
      first_of_level = false;
      HIPCHK(hipGetLastError());
      if (reported >= launched) break; /* max_iter == 0, or every launched pass has reported */
      if (ppf_status rc = wait_ticks(due[reported % (PPF_ICP_BATCH2 + 1)])) return rc;
      reported++;
      bool all = true;
      for (int j = 0; j < jobs; j++) all &= reinterpret_cast<volatile int*>(sc.h_done)[j] != 0;
      if (all) break; /* the passes still in the stream return at once; the next level's launches queue up behind them */
    }
    last_level_waited = launched > 0;
  }
  /* the passes launched ahead of the last level's end are still in the stream and will report too: the scratch (and its
   * counter) goes back to the pool only when they have */
  if (ppf_status rc = wait_ticks(tails_launched)) return rc;
  if (!last_level_waited) { /* nothing was polled after the last state went out */
    cnt.syncs++;
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int j = 0; j < jobs; j++) {
    /* undo centring and scaling: t = t/scale + meanAvg - R*meanAvg */
    const IcpState2& h = sc.h_state[j];
    double pose[16];
    memcpy(pose, h.pose, sizeof(pose));
    double Rm[3];
    for (int r = 0; r < 3; r++) Rm[r] = pose[r * 4] * h.mean_avg[0] + pose[r * 4 + 1] * h.mean_avg[1] + pose[r * 4 + 2] * h.mean_avg[2];
    for (int r = 0; r < 3; r++) pose[r * 4 + 3] = pose[r * 4 + 3] / h.scale + h.mean_avg[r] - Rm[r];
    memcpy(poses_out + (size_t)j * 16, pose, sizeof(pose));
    if (residuals) residuals[j] = h.fval_min;
    if (iters_total) iters_total[j] = h.total;
#ifdef PPF_ICP_CLOCKS
    fprintf(stderr, "icp job %d: start + staging %.1f  median %.1f  MAD %.1f  ownership %.1f  compaction %.1f  chunks %.1f  sums %.1f  solve %.1f us (iterations %d)\n", j,
            h.ph[6] * 0.01, h.ph[7] * 0.01, h.ph[0] * 0.01, h.ph[1] * 0.01, h.ph[2] * 0.01, h.ph[3] * 0.01, h.ph[4] * 0.01, h.ph[5] * 0.01, h.total);
#endif
  }
  return PPF_OK;
}

/* all `count` jobs, ICP_GROUP_JOBS at a time (one launch sequence per group, one group after the other).  On an error the
 * stream is drained before returning: passes launched ahead would otherwise still count into the scratch's pinned
 * counter and write its flags and states after the scratch has gone back to its pool. */
ppf_status icp_register_batch(const IcpJobSpec* specs, int count, const ppf_icp_params& prm, IcpBatchScratch& sc, hipStream_t st,
                              double* poses_out, double* residuals, int* iters_total, IcpRunCount& cnt) {
  for (int g0 = 0; g0 < count; g0 += ICP_GROUP_JOBS) {
    const int g = std::min(ICP_GROUP_JOBS, count - g0);
    const ppf_status s = icp_register_group(specs + g0, g, prm, sc, st, poses_out + (size_t)g0 * 16, residuals ? residuals + g0 : nullptr,
                                            iters_total ? iters_total + g0 : nullptr, cnt);
    if (s != PPF_OK) {
      (void)hipStreamSynchronize(st);
      return s;
    }
  }
  return PPF_OK;
}

/* one process-wide scratch for the batched path (buffers only grow); a second concurrent caller works on a private one */
struct IcpBatchPool {
  std::mutex mu;
  IcpBatchScratch sc;
  int device = -1;
};
IcpBatchPool& g_icp_batch_pool = *new IcpBatchPool(); /* never destroyed: nothing is freed after the HIP runtime has shut down */

ppf_status icp_batch_run_jobs(const IcpJobSpec* specs, int count, const ppf_icp_params& prm, hipStream_t st, double* poses_out,
                              double* residuals, int* iters_total, IcpRunCount& cnt) {
  std::unique_lock<std::mutex> lock(g_icp_batch_pool.mu, std::try_to_lock);
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (lock.owns_lock() && (g_icp_batch_pool.device == dev || g_icp_batch_pool.device < 0)) {
    g_icp_batch_pool.device = dev;
    return icp_register_batch(specs, count, prm, g_icp_batch_pool.sc, st, poses_out, residuals, iters_total, cnt);
  }
  IcpBatchScratch priv;
  const ppf_status s = icp_register_batch(specs, count, prm, priv, st, poses_out, residuals, iters_total, cnt);
  (void)hipStreamSynchronize(st); /* the private scratch goes back to the block cache */
  return s;
}

/* `jobs` initial poses against one pair of clouds (init_poses NULL: one registration from the identity) */
ppf_status icp_batch_run(const float* d_src, int n, int sstride, int snoff, const float* d_dst, int nd_all, int dstride, int dnoff,
                         const ppf_icp_params& prm, const double* const* init_poses, int jobs, hipStream_t st, double* poses_out,
                         double* residuals, int* iters_total) {
  IcpJobSpec specs[ICP_MAX_JOBS];
  for (int j = 0; j < jobs; j++) specs[j] = IcpJobSpec{d_src, n, sstride, snoff, d_dst, nd_all, dstride, dnoff, init_poses ? init_poses[j] : nullptr};
  IcpRunCount cnt;
  return icp_batch_run_jobs(specs, jobs, prm, st, poses_out, residuals, iters_total, cnt);
}

ppf_status icp_check(const char* who, const void* src, int n, int sstride, int snoff, const void* dst, int nd, int dstride, int dnoff,
                     const ppf_icp_params* prm) {
  if (!src || !dst || !prm || n <= 0 || nd <= 0 || bad_layout(sstride, snoff) || bad_layout(dstride, dnoff))
    return fail(PPF_ERR_INVALID, "%s: bad argument", who);
  if (prm->iterations < 0 || prm->num_levels < 0 || prm->num_levels > 30 || !(prm->tolerance >= 0))
    return fail(PPF_ERR_INVALID, "%s: bad ICP parameters", who);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);
  return PPF_OK;
}

/* a pose record's matrix replaced by M: q / t / angle from the new matrix */
void icp_set_pose(ppf_pose* p, const double* M, double residual) {
  memcpy(p->pose, M, 16 * sizeof(double));
  const double R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
  p->t[0] = M[3]; p->t[1] = M[7]; p->t[2] = M[11];
  ppf_dcm_to_quat(R, p->q);
  p->angle = ppf_angle_from_trace(R[0] + R[4] + R[8]);
  p->residual = residual;
}

/* Pose3D::appendPose: pose = incremental * pose, then q / t / angle from the new matrix */
void icp_append_pose(ppf_pose* p, const double* inc, double residual) {
  double out[16];
  ppf_mat44_mul(inc, p->pose, out);
  icp_set_pose(p, out, residual);
}

ppf_status icp_refine_device(const float* d_model, int n, int mstride, int mnoff, const float* d_scene, int nd, int sstride, int snoff,
                             const ppf_icp_params* prm, ppf_pose* poses, int n_poses, int* iters, hipStream_t st) {
  for (int k0 = 0; k0 < n_poses; k0 += ICP_MAX_JOBS) {
    const int cnt = std::min(ICP_MAX_JOBS, n_poses - k0);
    const double* init[ICP_MAX_JOBS];
    double inc[ICP_MAX_JOBS * 16], res[ICP_MAX_JOBS];
    int it[ICP_MAX_JOBS];
    for (int j = 0; j < cnt; j++) init[j] = poses[k0 + j].pose;
    const ppf_status s = icp_batch_run(d_model, n, mstride, mnoff, d_scene, nd, sstride, snoff, *prm, init, cnt, st, inc, res, it);
    if (s != PPF_OK) return s;
    for (int j = 0; j < cnt; j++) {
      icp_append_pose(&poses[k0 + j], inc + j * 16, res[j]);
      if (iters) iters[k0 + j] = it[j];
    }
  }
  return PPF_OK;
}

/* host rows (x y z at 0, normal at noff) -> packed device rows of 6 */
ppf_status icp_upload(const float* h, int n, int stride, int noff, DevBuf<float>& d) {
  HIPCHK(d.reserve((size_t)n * 6));
  if (noff == 3) {
    HIPCHK(hipMemcpy2D(d.p, 6 * sizeof(float), h, (size_t)stride * sizeof(float), 6 * sizeof(float), (size_t)n, hipMemcpyHostToDevice));
  } else {
    HIPCHK(hipMemcpy2D(d.p, 6 * sizeof(float), h, (size_t)stride * sizeof(float), 3 * sizeof(float), (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy2D(d.p + 3, 6 * sizeof(float), h + noff, (size_t)stride * sizeof(float), 3 * sizeof(float), (size_t)n, hipMemcpyHostToDevice));
  }
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_icp_params(ppf_icp_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->iterations = 100; /* ICP icp(100, 0.005f, 2.5f, 8), CloudProcessing.h:465,518 */
  p->tolerance = 0.005f;
  p->rejection_scale = 2.5f;
  p->num_levels = 8;
}

ppf_status ppf_icp_refine(const float* model, int n_model, int mstride, int mnoff, const float* scene, int n_scene, int sstride,
                          int snoff, const ppf_icp_params* params, ppf_pose* poses_io, int n_poses, int* iterations_out) {
  ppf_status s = icp_check("ppf_icp_refine", model, n_model, mstride, mnoff, scene, n_scene, sstride, snoff, params);
  if (s != PPF_OK) return s;
  if (n_poses < 0 || (n_poses > 0 && !poses_io)) return fail(PPF_ERR_INVALID, "ppf_icp_refine: bad pose list");
  DevBuf<float> dm, ds;
  if ((s = icp_upload(model, n_model, mstride, mnoff, dm)) != PPF_OK) return s;
  if ((s = icp_upload(scene, n_scene, sstride, snoff, ds)) != PPF_OK) return s;
  return icp_refine_device(dm.p, n_model, 6, 3, ds.p, n_scene, 6, 3, params, poses_io, n_poses, iterations_out, nullptr);
}

ppf_status ppf_icp_refine_device(const float* d_model, int n_model, int mstride, int mnoff, const float* d_scene, int n_scene,
                                 int sstride, int snoff, const ppf_icp_params* params, ppf_pose* poses_io, int n_poses,
                                 int* iterations_out, void* stream) {
  ppf_status s = icp_check("ppf_icp_refine_device", d_model, n_model, mstride, mnoff, d_scene, n_scene, sstride, snoff, params);
  if (s != PPF_OK) return s;
  if (n_poses < 0 || (n_poses > 0 && !poses_io)) return fail(PPF_ERR_INVALID, "ppf_icp_refine_device: bad pose list");
  return icp_refine_device(d_model, n_model, mstride, mnoff, d_scene, n_scene, sstride, snoff, params, poses_io, n_poses,
                           iterations_out, (hipStream_t)stream);
}

ppf_status ppf_icp_register(const float* src, int n_src, int sstride, int snoff, const float* dst, int n_dst, int dstride, int dnoff,
                            const ppf_icp_params* params, double* pose16_out, double* residual_out, int* iterations_out) {
  ppf_status s = icp_check("ppf_icp_register", src, n_src, sstride, snoff, dst, n_dst, dstride, dnoff, params);
  if (s != PPF_OK) return s;
  if (!pose16_out) return fail(PPF_ERR_INVALID, "ppf_icp_register: pose16_out is NULL");
  DevBuf<float> dsrc, ddst;
  if ((s = icp_upload(src, n_src, sstride, snoff, dsrc)) != PPF_OK) return s;
  if ((s = icp_upload(dst, n_dst, dstride, dnoff, ddst)) != PPF_OK) return s;
  return icp_batch_run(dsrc.p, n_src, 6, 3, ddst.p, n_dst, 6, 3, *params, nullptr, 1, nullptr, pose16_out, residual_out, iterations_out);
}

/* ---- helpers on the path's edges, on the device like everything else ---------------------------------------- */
ppf_status ppf_sample_cloud(const float* xyzn, int n, int stride, int noff, double relative_step, float* out, int cap_rows,
                            int* n_out) {
  if (!xyzn || n <= 0 || bad_layout(stride, noff) || !(relative_step > 0)) return fail(PPF_ERR_INVALID, "ppf_sample_cloud: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_sample_cloud: no HIP device (this engine has no CPU fallback)");
  DevBuf<float> d_raw;
  HIPCHK(d_raw.reserve((size_t)n * stride));
  HIPCHK(hipMemcpy(d_raw.p, xyzn, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  CloudDev sampled;
  std::vector<float> rows_host;
  ppf_status s = device_sample_cloud(d_raw.p, n, stride, noff, (float)relative_step, sampled, &rows_host, nullptr);
  if (s != PPF_OK) return s;
  const int rows = (int)(rows_host.size() / 6);
  if (n_out) *n_out = rows;
  if (out) {
    if (cap_rows < rows) return fail(PPF_ERR_CAPACITY, "ppf_sample_cloud: need %d rows, have %d", rows, cap_rows);
    memcpy(out, rows_host.data(), rows_host.size() * sizeof(float));
  }
  return PPF_OK;
}

ppf_status ppf_transform_pc_pose(const float* xyzn, int n, int stride, int noff, const double* T, float* out) {
  if (!xyzn || !T || !out || n < 0 || bad_layout(stride, noff)) return fail(PPF_ERR_INVALID, "ppf_transform_pc_pose: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_transform_pc_pose: no HIP device (this engine has no CPU fallback)");
  if (n == 0) return PPF_OK;
  DevBuf<float> d_in, d_out;
  DevBuf<double> d_T;
  ppf_status s = icp_upload(xyzn, n, stride, noff, d_in);
  if (s != PPF_OK) return s;
  HIPCHK(d_out.reserve((size_t)n * 6));
  HIPCHK(d_T.reserve(16));
  HIPCHK(hipMemcpy(d_T.p, T, 16 * sizeof(double), hipMemcpyHostToDevice));
  k_icp_transform<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d_in.p, 6, 3, 1, n, d_T.p, d_out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d_out.p, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost));
  return PPF_OK;
}

}  // extern "C"
