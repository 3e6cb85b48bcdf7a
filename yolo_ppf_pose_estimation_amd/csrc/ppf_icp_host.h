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
  /* one pinned block, carved by each call's plan: the count of finished k_icp2_tail workgroups in 64 bytes of its own, one
   * done flag per job and the jobs' loop states (both written by the kernels), the staging of `tables` */
  unsigned char* pinned = nullptr;
  size_t pinned_bytes = 0;
  ~IcpBatchScratch() {
    if (pinned) (void)hipHostFree(pinned);
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

/* every launch of the runner: on the call's stream, with `lds` bytes of dynamic LDS, counted */
#define ICP_LAUNCH(cnt, st, kern, grid, block, lds, ...)  \
  do {                                                    \
    kern<<<(grid), (block), (lds), (st)>>>(__VA_ARGS__);  \
    (cnt).launches++;                                     \
  } while (0)

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

/* ---- the plan of a launch sequence: where every job lives, its level schedule, every launch shape ------------------------ */
/* a level's launches, sized for its largest job; the dynamic LDS of the tail is the most any job needs */
struct IcpLevelPlan {
  double tol_p;
  int max_iter, max_ns, nn_rows;
  long long sum_ns;
  size_t tail_lds;
  unsigned begin_blocks, nn_blocks;
  IcpUniform U; /* uniform: what the per-pass kernels take from their arguments instead of the tables; else zero */
};
struct IcpPlan {
  bool uniform;
  int robust, num_levels;              /* num_levels: the level table's pitch, >= 0 */
  std::vector<IcpJobDesc> job;         /* n, nd_all and the o_* offsets of every job; the clouds, their layout and T0 are the caller's */
  std::vector<IcpLevelDesc> level_of;  /* job-major, as the device table */
  std::vector<IcpLevelPlan> level;
  size_t t_src, t_dst, t_sel, t_parts, t_sums, t_sumd;        /* the jobs' arrays end to end, in elements (IcpJobDesc) */
  size_t g_start, g_cur, g_box2, g_box1u, state, bb_parts;    /* the arrays of a fixed pitch per job, the states, the extents */
  size_t table_bytes, levels_off;
  size_t h_done_off, h_state_off, h_tables_off, pinned_bytes; /* the pinned block; the tick counter is at 0 */
  int max_chunks, max_rows_blocks, max_dst_blocks;            /* grid extents of the set-up launches */
};

/* A pure function of the jobs' row counts (specs[].n and .nd_all: nothing else of a spec is read), of whether all jobs
 * share one pair of clouds and one layout, and of the parameters (no HIP call, no scratch): ppf_debug_icp_plan exposes it
 * to the tests.  When `uniform`, job j's offsets are j times job 0's pitches: icp_pass_geom<false> computes them so. */
IcpPlan icp_plan(const IcpJobSpec* specs, int jobs, bool uniform, const ppf_icp_params& prm) {
  IcpPlan p{};
  const int nl = std::max(prm.num_levels, 0);
  const size_t J = (size_t)jobs;
  p.uniform = uniform;
  p.robust = prm.rejection_scale > 0 ? 1 : 0;
  p.num_levels = nl;
  p.levels_off = J * sizeof(IcpJobDesc);
  p.table_bytes = p.levels_off + J * (size_t)std::max(nl, 1) * sizeof(IcpLevelDesc);
  static_assert(sizeof(IcpJobDesc) % 16 == 0, "the level table follows the job table 16-byte aligned");
  static_assert(sizeof(IcpLevelDesc) % 16 == 0, "the tables are copied in 16-byte words");
  p.job.resize(J);
  p.level_of.resize(J * nl);
  for (int j = 0; j < jobs; j++) {
    const IcpJobSpec& S = specs[j];
    IcpJobDesc& D = p.job[j];
    D.n = S.n; D.nd_all = S.nd_all;
    const size_t chunks_src = ((size_t)S.n + ICP_CHUNK - 1) / ICP_CHUNK, chunks_dst = ((size_t)S.nd_all + ICP_CHUNK - 1) / ICP_CHUNK;
    const size_t m = (size_t)std::min(S.n, S.nd_all);
    D.o_src0 = p.t_src * 6; D.o_best = p.t_src; D.o_dst0 = p.t_dst * 6; D.o_owner = p.t_dst;
    D.o_sel = p.t_sel; D.o_parts = p.t_parts; D.o_sums = p.t_sums; D.o_sumd = p.t_sumd;
    p.t_src += (size_t)S.n; p.t_dst += (size_t)S.nd_all; p.t_sel += m; p.t_parts += (m + ICP_CHUNK - 1) / ICP_CHUNK * ICP_ENTRIES;
    p.t_sums += chunks_src * 3; p.t_sumd += chunks_dst * 3;
    p.max_chunks = std::max(p.max_chunks, (int)(chunks_src + chunks_dst));
    const int nb_dst = (S.nd_all + ICP_ROWS_BLOCK - 1) / ICP_ROWS_BLOCK, nb_src = (S.n + ICP_ROWS_BLOCK - 1) / ICP_ROWS_BLOCK;
    p.max_rows_blocks = std::max(p.max_rows_blocks, nb_dst + nb_src);
    p.max_dst_blocks = std::max(p.max_dst_blocks, nb_dst);
    for (int level = 0; level < nl; level++) p.level_of[(size_t)j * nl + level] = icp_level_desc(S.n, S.nd_all, level);
  }
  p.g_start = J * (ICP_LEAVES + 64);
  p.g_cur = J * ICP_LEAVES;
  p.g_box2 = J * ICP_LEAVES * 2;
  p.g_box1u = J * 64 * 8;
  p.state = std::max<size_t>(J, ICP_MAX_JOBS);
  p.bb_parts = p.t_sumd * 2;
  /* every part of the pinned block is 16-byte aligned (the tables are read as uint4); room for ICP_MAX_JOBS jobs at least */
  const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
  p.h_done_off = 64;
  p.h_state_off = p.h_done_off + up16(p.state * sizeof(int));
  p.h_tables_off = p.h_state_off + up16(p.state * sizeof(IcpState2));
  p.pinned_bytes = p.h_tables_off + p.table_bytes;
  p.level.resize((size_t)nl);
  for (int level = 0; level < nl; level++) {
    IcpLevelPlan& P = p.level[level];
    P.tol_p = (double)prm.tolerance * (double)(level + 1) * (level + 1);
    P.max_iter = (int)icp_round((double)prm.iterations / (level + 1));
    P.tail_lds = (size_t)ICP_TAIL_VAL_BYTES;
    for (int j = 0; j < jobs; j++) {
      const IcpLevelDesc& L = p.level_of[(size_t)j * nl + level];
      P.max_ns = std::max(P.max_ns, L.ns);
      P.sum_ns += L.ns;
      P.tail_lds = std::max(P.tail_lds, L.staged ? (size_t)L.ns * 4 : (size_t)0);
    }
    P.begin_blocks = (unsigned)((P.max_ns + 255) / 256);
    /* rows per wave of the neighbour search: one, unless that makes more waves than the chip holds several times over */
    P.nn_rows = (int)std::min<long long>(ICP_NN_ROWS, std::max<long long>(1, P.sum_ns / PPF_ICP_NN_WAVES));
    P.nn_blocks = (unsigned)((P.max_ns + 4 * P.nn_rows - 1) / (4 * P.nn_rows));
    if (uniform) {
      const IcpLevelDesc& L = p.level_of[level];
      IcpUniform& U = P.U;
      U.ns = L.ns; U.nd = L.nd; U.step = L.step; U.step_shift = L.step_shift; U.staged = L.staged;
      U.n = specs[0].n; U.nd_all = specs[0].nd_all;
      U.p_sel = (size_t)std::min(specs[0].n, specs[0].nd_all);
      U.p_parts = (U.p_sel + ICP_CHUNK - 1) / ICP_CHUNK * ICP_ENTRIES;
    }
  }
  return p;
}

/* The device arrays of a launch sequence, each stated once: the buffer and the IcpBatch pointer of one name, its elements
 * by the plan.  Reserving and addressing are this one walk. */
ppf_status icp_reserve(IcpBatchScratch& sc, const IcpPlan& p, IcpBatch& B) {
#define ICP_ARRAY(name, count)       \
  HIPCHK(sc.name.reserve((count))); \
  B.name = sc.name.p
  ICP_ARRAY(src0, p.t_src * 6);
  ICP_ARRAY(src_pct, p.t_src * 6);
  ICP_ARRAY(dst0, p.t_dst * 6);
  ICP_ARRAY(best, p.t_src);
  ICP_ARRAY(owner, p.t_dst);
  ICP_ARRAY(sel, p.t_sel);
  ICP_ARRAY(parts, p.t_parts);
  ICP_ARRAY(sum_src, p.t_sums);
  ICP_ARRAY(sum_dst, p.t_sumd);
  ICP_ARRAY(g_pts, p.t_dst);
  ICP_ARRAY(g_start, p.g_start);
  ICP_ARRAY(g_cur, p.g_cur);
  ICP_ARRAY(g_box2, p.g_box2);
  ICP_ARRAY(g_box1u, p.g_box1u);
  ICP_ARRAY(own_a, p.t_dst);
  ICP_ARRAY(bb_parts, p.bb_parts);
  ICP_ARRAY(state, p.state);
#undef ICP_ARRAY
  HIPCHK(sc.tables.reserve(p.table_bytes)); /* both tables; they go up once, through k_icp2_reset */
  B.d_tables = reinterpret_cast<uint4*>(sc.tables.p);
  B.jobs = reinterpret_cast<const IcpJobDesc*>(sc.tables.p);
  B.levels = reinterpret_cast<const IcpLevelDesc*>(sc.tables.p + p.levels_off);
  B.num_levels = p.num_levels;
  B.table_words = (uint32_t)(p.table_bytes / 16);
  /* the pinned block grows here only: before the call's first launch, when nothing of an earlier call is in flight */
  if (sc.pinned_bytes < p.pinned_bytes) {
    if (sc.pinned) { (void)hipHostFree(sc.pinned); sc.pinned = nullptr; }
    sc.pinned_bytes = 0;
    HIPCHK(hipHostMalloc((void**)&sc.pinned, p.pinned_bytes, hipHostMallocDefault));
    sc.pinned_bytes = p.pinned_bytes;
  }
  B.h_ticks = reinterpret_cast<unsigned long long*>(sc.pinned);
  B.h_done = reinterpret_cast<int*>(sc.pinned + p.h_done_off);
  B.h_state = reinterpret_cast<IcpState2*>(sc.pinned + p.h_state_off);
  B.h_tables = reinterpret_cast<const uint4*>(sc.pinned + p.h_tables_off);
  return PPF_OK;
}

/* until `want` k_icp2_tail workgroups of the call have reported.  The stream is only asked when the counter has not
 * moved for a long while */
ppf_status icp_wait_ticks(volatile unsigned long long* ticks, const unsigned long long want, hipStream_t st, IcpRunCount& cnt) {
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
}

/* a pass for the live jobs: neighbour search, then the tail; SEG as the kernels' (!SEG: the geometry travels in U) */
template <bool SEG>
void icp_launch_pass(const IcpBatch& B, const IcpLive& live, unsigned nl, int level, const IcpLevelPlan& P, const ppf_icp_params& prm,
                     hipStream_t st, IcpRunCount& cnt) {
  const int brute_nd = (prm.flags & PPF_ICP_GRID_ALWAYS) ? 0 : ICP_BRUTE_ND;
  ICP_LAUNCH(cnt, st, k_icp2_nn<SEG>, dim3(P.nn_blocks, nl), dim3(256), 0, B, live, level, P.U, P.nn_rows, brute_nd);
  ICP_LAUNCH(cnt, st, k_icp2_tail<SEG>, dim3(nl), dim3(1024), P.tail_lds, B, live, level, P.U, prm.rejection_scale, level == 0 ? 1 : 0);
  cnt.passes++;
}

/* a job's final state as the caller's pose: centring and scaling undone, t = t/scale + meanAvg - R*meanAvg */
void icp_job_result(const IcpState2& h, int j, double* pose_out, double* residual, int* iters) {
  double pose[16];
  memcpy(pose, h.pose, sizeof(pose));
  double Rm[3];
  for (int r = 0; r < 3; r++) Rm[r] = pose[r * 4] * h.mean_avg[0] + pose[r * 4 + 1] * h.mean_avg[1] + pose[r * 4 + 2] * h.mean_avg[2];
  for (int r = 0; r < 3; r++) pose[r * 4 + 3] = pose[r * 4 + 3] / h.scale + h.mean_avg[r] - Rm[r];
  memcpy(pose_out, pose, sizeof(pose));
  if (residual) *residual = h.fval_min;
  if (iters) *iters = h.total;
#ifdef PPF_ICP_CLOCKS
  fprintf(stderr, "icp job %d: start + staging %.1f  median %.1f  MAD %.1f  ownership %.1f  compaction %.1f  chunks %.1f  sums %.1f  solve %.1f us (iterations %d)\n", j,
          h.ph[6] * 0.01, h.ph[7] * 0.01, h.ph[0] * 0.01, h.ph[1] * 0.01, h.ph[2] * 0.01, h.ph[3] * 0.01, h.ph[4] * 0.01, h.ph[5] * 0.01, h.total);
#endif
  (void)j;
}

/* registerModelToScene for `jobs` (<= ICP_GROUP_JOBS) registrations at once, each with its own clouds and initial pose:
 * every launch covers all jobs (sized for the largest), an iteration is two launches (k_icp2_nn, k_icp2_tail), the host
 * keeps PPF_ICP_BATCH2 of them in the stream ahead of the device and reads the jobs' done flags whenever one reports.  The
 * level loop is lock-step over the jobs: a level ends when every job is done with it.  Everything runs on `st`.
 * Plan, reserve, the set-up launches, the level loop, the last wait, the results. */
ppf_status icp_register_group(const IcpJobSpec* specs, int jobs, const ppf_icp_params& prm, IcpBatchScratch& sc, hipStream_t st,
                              double* poses_out /* jobs x 16 */, double* residuals, int* iters_total, IcpRunCount& cnt) {
  /* one pair of clouds for every job: the per-pass kernels take the geometry from their arguments (IcpUniform) */
  bool uniform = true;
  for (int j = 1; j < jobs; j++)
    uniform &= specs[j].src == specs[0].src && specs[j].n == specs[0].n && specs[j].sstride == specs[0].sstride &&
               specs[j].snoff == specs[0].snoff && specs[j].dst == specs[0].dst && specs[j].nd_all == specs[0].nd_all &&
               specs[j].dstride == specs[0].dstride && specs[j].dnoff == specs[0].dnoff;
  const IcpPlan plan = icp_plan(specs, jobs, uniform, prm);
  IcpBatch B;
  memset(&B, 0, sizeof(B));
  if (ppf_status rc = icp_reserve(sc, plan, B)) return rc;
  /* the tables, in their pinned staging (not touched again before the call has finished): every job's place in the shared
   * scratch arrays, its clouds and initial pose, its level schedule */
  IcpJobDesc* jd = reinterpret_cast<IcpJobDesc*>(sc.pinned + plan.h_tables_off);
  for (int j = 0; j < jobs; j++) {
    const IcpJobSpec& S = specs[j];
    IcpJobDesc& D = jd[j];
    D = plan.job[j];
    D.src = S.src; D.dst = S.dst;
    D.sstride = S.sstride; D.snoff = S.snoff; D.dstride = S.dstride; D.dnoff = S.dnoff;
    D.has_init = S.init ? 1 : 0;
    for (int k = 0; k < 16; k++) D.T0[k] = S.init ? S.init[k] : ((k % 5 == 0) ? 1.0 : 0.0);
  }
  if (!plan.level_of.empty()) memcpy(sc.pinned + plan.h_tables_off + plan.levels_off, plan.level_of.data(), plan.level_of.size() * sizeof(IcpLevelDesc));
  *B.h_ticks = 0ull; /* no kernel of an earlier call is running: every call ends with all of its launches accounted for, and an
                        error return drains the stream first (icp_register_batch) */
  static std::once_flag once_tail;
  static hipError_t attr_tail = hipSuccess;
  std::call_once(once_tail, [] {
    attr_tail = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_icp2_tail<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
    if (attr_tail == hipSuccess)
      attr_tail = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_icp2_tail<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
  });
  HIPCHK(attr_tail);
  const unsigned uj = (unsigned)jobs;
  const dim3 per_job(uj), chunks((unsigned)plan.max_chunks, uj);
  /* the two clouds packed (the source moved by its job's initial pose), centred on the average of the two means, scaled to
   * unit average distance from the origin; the search grid over each job's scene */
  ICP_LAUNCH(cnt, st, k_icp2_reset, dim3(uj, 32), dim3(256), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_pack_sums, chunks, dim3(64), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_mean, per_job, dim3(256), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_dist_sums, chunks, dim3(64), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_scale, per_job, dim3(256), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_rows_count, dim3((unsigned)plan.max_rows_blocks, uj), dim3(1024), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_grid_scan, per_job, dim3(1024), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_grid_scatter, dim3((unsigned)plan.max_dst_blocks, uj), dim3(1024), 0, B);
  ICP_LAUNCH(cnt, st, k_icp2_grid_boxes, dim3(ICP_LEAVES / 4, uj), dim3(256), 0, B);
  HIPCHK(hipGetLastError());
  const auto launch_pass = plan.uniform ? icp_launch_pass<false> : icp_launch_pass<true>;
  volatile int* h_done = B.h_done;
  unsigned long long tails_launched = 0;
  bool last_level_waited = false;
  for (int level = plan.num_levels - 1; level >= 0; level--) {
    const IcpLevelPlan& P = plan.level[level];
    ICP_LAUNCH(cnt, st, k_icp2_level_begin, dim3(P.begin_blocks, uj), dim3(256), 0, B, level, P.tol_p, P.max_iter, plan.robust, level == 0 ? 1 : 0);
    /* The passes of a level are launched ahead of the device: PPF_ICP_BATCH2 (neighbour search, tail) pairs are in the stream,
     * and every time the oldest of them reports, the next one is launched -- the device never waits for the host between
     * passes (with whole batches it idled ~11 us after every second pass).  Every k_icp2_tail workgroup, whatever it did,
     * adds one to a counter in pinned memory as its last act (after its done flag and, at the end of a level, its state);
     * polling that is a few microseconds quicker than going through the stream.  A pass launched after the level's last one
     * finds every job done and returns at once. */
    int launched = 0, reported = 0;
    unsigned long long due[PPF_ICP_BATCH2 + 1]; /* the counter's value when pass k has reported, k modulo the passes in the stream */
    bool first_of_level = true;
    while (true) {
      while (launched < P.max_iter && launched - reported < (int)PPF_ICP_BATCH2) {
        /* a pass is launched for the jobs that had not finished the level when the host last looked (all of them at its start);
         * the list travels as a kernel argument, copied at the launch */
        IcpLive live;
        unsigned nl = 0;
        for (int j = 0; j < jobs; j++)
          if (first_of_level || h_done[j] == 0) live.job[nl++] = (uint16_t)j;
        if (nl == 0) live.job[nl++] = 0; /* cannot happen: the loop ends when every job is done */
        launch_pass(B, live, nl, level, P, prm, st, cnt);
        tails_launched += (unsigned long long)nl;
        due[launched % (PPF_ICP_BATCH2 + 1)] = tails_launched;
        launched++;
      }
      first_of_level = false;
      HIPCHK(hipGetLastError());
      if (reported >= launched) break; /* max_iter == 0, or every launched pass has reported */
      if (ppf_status rc = icp_wait_ticks(B.h_ticks, due[reported % (PPF_ICP_BATCH2 + 1)], st, cnt)) return rc;
      reported++;
      bool all = true;
      for (int j = 0; j < jobs; j++) all &= h_done[j] != 0;
      if (all) break; /* the passes still in the stream return at once; the next level's launches queue up behind them */
    }
    last_level_waited = launched > 0;
  }
  /* the passes launched ahead of the last level's end are still in the stream and will report too: the scratch (and its
   * counter) goes back to the pool only when they have */
  if (ppf_status rc = icp_wait_ticks(B.h_ticks, tails_launched, st, cnt)) return rc;
  if (!last_level_waited) { /* nothing was polled after the last state went out */
    cnt.syncs++;
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int j = 0; j < jobs; j++)
    icp_job_result(B.h_state[j], j, poses_out + (size_t)j * 16, residuals ? residuals + j : nullptr, iters_total ? iters_total + j : nullptr);
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

ppf_status ppf_debug_icp_plan(const ppf_debug_icp_plan_in* in, ppf_debug_icp_plan_out* out) {
  if (!in || !out) return fail(PPF_ERR_INVALID, "ppf_debug_icp_plan: NULL");
  memset(out, 0, sizeof(*out));
  bool ok = in->jobs >= 1 && in->jobs <= 8 && in->iterations >= 0 && in->num_levels >= 0 && in->num_levels <= 8 && in->tolerance >= 0;
  for (int j = 0; ok && j < in->jobs; j++)
    ok = in->n[j] >= 1 && in->nd_all[j] >= 1 && (!in->uniform || (in->n[j] == in->n[0] && in->nd_all[j] == in->nd_all[0]));
  if (!ok) return fail(PPF_ERR_INVALID, "ppf_debug_icp_plan: bad argument");
  IcpJobSpec specs[8];
  for (int j = 0; j < in->jobs; j++) specs[j] = IcpJobSpec{nullptr, in->n[j], 6, 3, nullptr, in->nd_all[j], 6, 3, nullptr};
  ppf_icp_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.iterations = in->iterations; prm.tolerance = in->tolerance; prm.rejection_scale = in->rejection_scale; prm.num_levels = in->num_levels;
  const IcpPlan p = icp_plan(specs, in->jobs, in->uniform != 0, prm);
  out->t_src = p.t_src; out->t_dst = p.t_dst; out->t_sel = p.t_sel; out->t_parts = p.t_parts; out->t_sums = p.t_sums; out->t_sumd = p.t_sumd;
  out->g_start = p.g_start; out->g_cur = p.g_cur; out->g_box2 = p.g_box2; out->g_box1u = p.g_box1u; out->state = p.state; out->bb_parts = p.bb_parts;
  out->table_bytes = p.table_bytes; out->levels_off = p.levels_off;
  out->h_done_off = p.h_done_off; out->h_state_off = p.h_state_off; out->h_tables_off = p.h_tables_off; out->pinned_bytes = p.pinned_bytes;
  const int last = in->jobs - 1;
  const auto offsets = [](const IcpJobDesc& D, uint64_t* o) {
    const size_t v[8] = {D.o_src0, D.o_dst0, D.o_best, D.o_owner, D.o_sel, D.o_parts, D.o_sums, D.o_sumd};
    for (int k = 0; k < 8; k++) o[k] = v[k];
  };
  offsets(p.job[0], out->first_off);
  offsets(p.job[last], out->last_off);
  out->max_chunks = p.max_chunks; out->max_rows_blocks = p.max_rows_blocks; out->max_dst_blocks = p.max_dst_blocks;
  out->robust = p.robust;
  out->n_levels = p.num_levels;
  for (int l = 0; l < p.num_levels; l++) {
    const IcpLevelPlan& P = p.level[l];
    out->tol_p[l] = P.tol_p; out->sum_ns[l] = P.sum_ns; out->tail_lds[l] = P.tail_lds;
    out->max_iter[l] = P.max_iter; out->max_ns[l] = P.max_ns; out->nn_rows[l] = P.nn_rows;
    out->nn_blocks[l] = P.nn_blocks; out->begin_blocks[l] = P.begin_blocks;
    const auto level = [](const IcpLevelDesc& L, int32_t* o) { o[0] = L.step; o[1] = L.ns; o[2] = L.nd; o[3] = L.step_shift; o[4] = L.staged; };
    level(p.level_of[l], out->first_level[l]);
    level(p.level_of[(size_t)last * p.num_levels + l], out->last_level[l]);
    const IcpUniform& U = P.U;
    const int32_t u[7] = {U.ns, U.nd, U.step, U.step_shift, U.staged, U.n, U.nd_all};
    memcpy(out->uni[l], u, sizeof(u));
    out->uni_p_sel[l] = U.p_sel; out->uni_p_parts[l] = U.p_parts;
  }
  return PPF_OK;
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
