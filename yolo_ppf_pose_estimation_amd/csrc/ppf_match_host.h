/*
 * ppf_match_host.h — C-ABI, matching side: workspaces, ppf_match_device and its result accessors, the host-buffer entries
 * ppf_match / ppf_raw_votes, pose-list clustering.  Reference call sites: /root/reference/include/CloudProcessing.h:442 (match), :495 (match_S2B).
 */
#ifndef PPF_MATCH_HOST_H
#define PPF_MATCH_HOST_H

extern "C" {

/* ---- workspace / matching --------------------------------------------------------------------- */
ppf_status ppf_workspace_create(ppf_workspace** out) {
  if (!out) return fail(PPF_ERR_INVALID, "ppf_workspace_create: NULL");
  *out = new (std::nothrow) ppf_workspace();
  if (!*out) return fail(PPF_ERR_NOMEM, "ppf_workspace_create: out of memory");
  return PPF_OK;
}
ppf_status ppf_workspace_destroy(ppf_workspace* ws) {
  if (!ws) return PPF_OK;
  delete ws; /* the destructor drains the device its buffers live on before they return to the block cache */
  return PPF_OK;
}
ppf_status ppf_workspace_set_option(ppf_workspace* ws, int option, double value) {
  if (!ws) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: NULL");
  switch (option) {
    case PPF_OPT_HIT_FRACTION:
      if (!(value > 0 && value <= 1)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: hit fraction must be in (0, 1]");
      ws->frac.hit = value;
      ws->frac_known = true;
      return PPF_OK;
    case PPF_OPT_GROUP_ROUND_BUCKETS:
      if (!(value >= 0 && value <= 1e9)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: bad bucket count");
      ws->round_buckets_cap = (int)value;
      return PPF_OK;
    case PPF_OPT_CLUSTER_SERIAL:
      ws->cluster_serial = value != 0;
      return PPF_OK;
    case PPF_OPT_ACC32:
      if (!(value == 0 || value == 1 || value == 2 || value == 3)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: PPF_OPT_ACC32 takes 0 .. 3");
      ws->force_acc32 = value == 1;
      ws->acc32_policy = value == 1 ? 0 : (int)value;
      ws->heavy_votes = ~0ull;
      if (value != 0) ws->acc32 = false;
      return PPF_OK;
    case PPF_OPT_BATCH_REFS:
      if (!(value >= 0 && value <= 1e9)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: bad batch size");
      ws->batch_refs_cap = (int)value;
      return PPF_OK;
    case PPF_OPT_RUN_STAGING:
      if (!(value >= 0 && value <= 1e9)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: bad run staging size");
      ws->run_seg_cap = (int)value;
      return PPF_OK;
    case PPF_OPT_TABLE_FRACTION:
      if (!(value > 0 && value <= 1)) return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: table fraction must be in (0, 1]");
      ws->frac.tbl = std::min(TBL_FRAC_MAX, value);
      return PPF_OK;
    default:
      return fail(PPF_ERR_INVALID, "ppf_workspace_set_option: unknown option %d", option);
  }
}
ppf_status ppf_workspace_enable_timing(ppf_workspace* ws, int on) {
  if (!ws) return fail(PPF_ERR_INVALID, "ppf_workspace_enable_timing: NULL");
  if (on && !ws->ev[0])
    for (auto& e : ws->ev) HIPCHK(hipEventCreate(&e));
  ws->timing = on != 0;
  return PPF_OK;
}

static ppf_status check_match_args(const ppf_model* m, const void* scene, int ns, int sstride, int snoff, const void* edge, int ne,
                                   int estride, int enoff, const ppf_match_params* p) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  if (!scene || ns <= 0 || bad_layout(sstride, snoff) || !p) return fail(PPF_ERR_INVALID, "match: bad scene argument");
  if (edge && (ne <= 0 || bad_layout(estride, enoff))) return fail(PPF_ERR_INVALID, "match: bad edge argument");
  if (!(p->relative_scene_sample_step <= 1 && p->relative_scene_sample_step > 0))
    return fail(PPF_ERR_INVALID, "match: relativeSceneSampleStep must be in (0, 1]");
  if (!p->presampled && !(p->relative_scene_distance > 0)) return fail(PPF_ERR_INVALID, "match: relativeSceneDistance must be > 0");
  if (p->ref_stride < 1 || p->ref_offset < 0) return fail(PPF_ERR_INVALID, "match: bad ref_offset/ref_stride");
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev != m->device)
    return fail(PPF_ERR_INVALID, "match: the model lives on device %d, the calling thread's current device is %d", m->device, dev);
  return PPF_OK;
}

/* A2: sample the scene (and edge) cloud into the workspace, or take the rows as they are */
static ppf_status prepare_scene(ppf_workspace* ws, const float* d_scene, int ns, int sstride, int snoff, const float* d_edge, int ne,
                                int estride, int enoff, const ppf_match_params* params, hipStream_t st) {
  auto load = [&](CloudDev& dst, const float* d_src, int rows, int stride, int noff) -> ppf_status {
    if (params->presampled) return dst.load_device(d_src, rows, stride, noff, st);
    return device_sample_cloud(d_src, rows, stride, noff, (float)params->relative_scene_distance, dst, nullptr, st);
  };
  ppf_status s = load(ws->surf, d_scene, ns, sstride, snoff);
  if (s != PPF_OK) return s;
  if (d_edge) s = load(ws->edge, d_edge, ne, estride, enoff);
  ws->has_edge = d_edge != nullptr;
  return s;
}

static ppf_status match_prepared(const ppf_model* m, ppf_workspace* ws, const ppf_match_params* params, hipStream_t st, bool retry = false);

ppf_status ppf_match_device(const ppf_model* m, ppf_workspace* ws, const float* d_scene, int ns, int sstride, int snoff,
                            const float* d_edge, int ne, int estride, int enoff, const ppf_match_params* params, void* stream) {
  if (!ws) return fail(PPF_ERR_INVALID, "ppf_match_device: workspace is NULL");
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_match_device: no HIP device (this engine has no CPU fallback)");
  ppf_status s = check_match_args(m, d_scene, ns, sstride, snoff, d_edge, ne, estride, enoff, params);
  if (s != PPF_OK) return s;
  hipStream_t st = (hipStream_t)stream;
  s = prepare_scene(ws, d_scene, ns, sstride, snoff, d_edge, ne, estride, enoff, params, st);
  if (s != PPF_OK) return s;
  return match_prepared(m, ws, params, st);
}

/* The fractions a workspace has learned for a model (hits per scene pair, runs per hit), keyed by the model's serial
 * number; create = true makes room for a model it has not met (at most 16 are remembered, the oldest goes). */
static ppf_workspace::Learned* workspace_learned(ppf_workspace* ws, const ppf_model* m, bool create) {
  for (auto& fm : ws->frac_by_model)
    if (fm.model_serial == m->serial) return &fm;
  if (!create) return nullptr;
  if (ws->frac_by_model.size() >= 16) ws->frac_by_model.erase(ws->frac_by_model.begin());
  ws->frac_by_model.push_back({m->serial, PoolFractions()});
  return &ws->frac_by_model.back();
}

/* store the current model's learned fractions */
static void workspace_remember_frac(ppf_workspace* ws) {
  if (!ws->model || !ws->frac_known) return;
  workspace_learned(ws, ws->model, true)->frac = ws->frac;
}

/* the workspace keeps the model alive until its next call (or its destruction): results are fetched later.  A context
 * workspace (model_owns_me) lives inside its model and takes no reference. */
static void workspace_hold_model(ppf_workspace* ws, const ppf_model* m) {
  if (ws->model == m) return;
  ppf_model* old = ws->model;
  ws->model = const_cast<ppf_model*>(m);
  if (ws->model_owns_me) return;
  if (ws->model) ws->model->refcount.fetch_add(1);
  if (old) (void)ppf_model_release(old);
}

ppf_workspace::~ppf_workspace() {
  sync_device(device); /* buffers return to the block cache: nothing may still be using them */
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : batch_ev)
    if (e) (void)hipEventDestroy(e);
  if (model && !model_owns_me) (void)ppf_model_release(model);
  if (h_sum) (void)hipHostFree(h_sum);
}

/* bytes of hit scratch one hit costs: raw {bucket, j} + sorted payload alpha_s + its share of the run table (+ 2 bytes for the
 * cell the payload no longer carries: kept, so that the batches of reference points stay the size they were tuned at) */
constexpr double HIT_SCRATCH_BYTES = 8.0 + 8.0 + 2.0 + 16.0 / 6.0;
/* match_plan lets a batch of more than one reference point expect at most HIT_BYTES_BUDGET / HIT_SCRATCH_BYTES hits (a batch
 * of one has at most its paired points, an int), so every offset into the hit pools fits 32 bits */
static_assert((double)HIT_BYTES_BUDGET / HIT_SCRATCH_BYTES < 2.0e9, "a batch's expected hits must leave 32-bit pool offsets room");

/* two run-time switches as compile-time ones: calls f(std::bool_constant<a>, std::bool_constant<b>) */
extern "C++" template <typename F>
void bools_typed(bool a, bool b, F&& f) {
  if (a && b) f(std::true_type{}, std::true_type{});
  else if (a) f(std::true_type{}, std::false_type{});
  else if (b) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

/* k_pairs<pair feature, surface-to-boundary>: same_cloud == 0 is match_S2B (the paired points come from the edge cloud) */
static void launch_pairs(const MatchArgs& va, bool darboux, hipStream_t st) {
  const dim3 grid(va.pair_chunks, va.n_ref), block(PAIR_BLOCK);
  const dim3 ogrid((unsigned)std::min(va.n_ref, 1024)), oblock(256); /* k_pairs_odd: adds up hit_count, then returns at once unless k_frames raised its flag */
  bools_typed(darboux, !va.same_cloud, [&](auto D, auto S) {
    constexpr bool DARBOUX = decltype(D)::value, S2B = decltype(S)::value;
    k_pairs<DARBOUX, S2B><<<grid, block, 0, st>>>(va);
    if (!va.count_only) k_pairs_odd<DARBOUX, S2B><<<ogrid, oblock, 0, st>>>(va);
  });
}

/* k_vote<alpha over 2 pi, 32-bit cells> */
static void launch_vote(const MatchArgs& va, bool wrap, bool acc32, dim3 grid, size_t lds, hipStream_t st) {
  bools_typed(wrap, acc32, [&](auto W, auto A) { k_vote<decltype(W)::value, decltype(A)::value><<<grid, dim3(VOTE_BLOCK), lds, st>>>(va); });
}

/* k_vote (every instantiation) and k_group may take the whole LDS: said once per process */
static hipError_t match_kernel_attributes() {
  static std::once_flag once;
  static hipError_t attr_err = hipSuccess;
  std::call_once(once, [] {
    auto set = [](const void* f, int bytes) {
      if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    };
    for (bool acc32 : {false, true})
      for (bool wrap : {false, true})
        bools_typed(wrap, acc32, [&](auto W, auto A) { set(reinterpret_cast<const void*>(&k_vote<decltype(W)::value, decltype(A)::value>), LDS_BYTES); });
    set(reinterpret_cast<const void*>(&k_group), LDS_BYTES - 1024);
  });
  return attr_err;
}

/* ---- the plan of a call: how many reference points per batch, how big each hit pool, how much LDS ---------------------- */
/* inputs and outputs are the two plain records of include/ppf_hip.h, which ppf_debug_match_plan hands through as they are */
typedef ppf_debug_match_plan_in MatchPlanIn;
typedef ppf_debug_match_plan_out MatchPlan;

/* k_pairs workgroups that cover the paired points of one reference point */
static int pair_chunks_of(int n_paired) { return (n_paired + PAIR_BLOCK * PAIRS_PER_THREAD - 1) / (PAIR_BLOCK * PAIRS_PER_THREAD); }

/* A pure function of a handful of numbers (no HIP call, no workspace): ppf_debug_match_plan exposes it to the tests. */
static ppf_status match_plan(const MatchPlanIn& in, MatchPlan* plan) {
  MatchPlan p{};
  p.pair_chunks = pair_chunks_of(in.n_paired);
  const uint32_t round_cap = in.round_buckets_cap > 0 ? (uint32_t)std::min(in.round_buckets_cap, GROUP_MAX_BUCKETS) : (uint32_t)GROUP_MAX_BUCKETS;
  p.n_rounds = std::max(1, (int)((in.n_buckets + round_cap - 1) / round_cap));
  p.round_buckets = (int)std::min<uint32_t>(std::max<uint32_t>(in.n_buckets, 1u), round_cap);
  /* batch of reference points: its expected hits fit the scratch budget */
  const double frac = std::min(1.0, std::max(in.hit_frac, 1e-3));
  const double hits_per_ref = std::max(64.0, frac * (double)in.n_paired);
  const double tbl_frac = !in.count_tables ? 0.0 : frac >= 1.0 ? TBL_FRAC_MAX : std::min(TBL_FRAC_MAX, in.tbl_frac);
  int batch = (int)std::min<double>((double)in.n_ref, std::max(1.0, (double)HIT_BYTES_BUDGET / (hits_per_ref * (HIT_SCRATCH_BYTES + tbl_frac * TBL_BYTES))));
  batch = std::min(batch, 32768); /* grid.y of k_pairs */
  if (in.batch_refs_cap > 0) batch = std::min(batch, in.batch_refs_cap);
  p.batch = batch;
  p.n_batches = (in.n_ref + batch - 1) / batch;
  const bool worst_case = frac >= 1.0;
  const double est = hits_per_ref * (double)batch;
  /* a stripe receives whole workgroups of up to PAIR_BLOCK*PAIRS_PER_THREAD hits; at worst-case size every workgroup of
   * the batch could be full and land anywhere, otherwise 4 % + two workgroups of slack over an even share */
  const uint32_t wg_hits = PAIR_BLOCK * PAIRS_PER_THREAD;
  p.stripe_bits = 6; /* 64 stripes, fewer while a stripe would average over less than 512 workgroups */
  while (p.stripe_bits > 0 && ((size_t)batch * p.pair_chunks >> p.stripe_bits) < 512) p.stripe_bits--;
  if (worst_case) p.stripe_bits = 0; /* one stripe that holds every pair of the batch: nothing can overflow */
  const uint32_t n_stripes = 1u << p.stripe_bits;
  p.stripe_cap = worst_case ? (uint32_t)std::min<double>(4.0e9 / n_stripes, (double)batch * p.pair_chunks * wg_hits)
                            : (uint32_t)(est / n_stripes * 1.04) + 2 * wg_hits;
  p.sorted_cap = (uint32_t)std::min(4.0e9, est + 4096.0);
  p.run_cap = worst_case ? p.sorted_cap : (uint32_t)std::min<double>((double)p.sorted_cap, std::max(est * std::min(1.0, in.run_frac), 64.0 * batch) + 1024.0);
  /* count tables: a run of c >= agg_min_hits hits takes ceil(c / AGG_SUB), so TBL_FRAC_MAX per hit is the ceiling */
  p.table_cap = !in.count_tables ? 1u : (uint32_t)std::min(1.0e9, std::max(est * (worst_case ? TBL_FRAC_MAX : tbl_frac), 4.0 * batch) + 256.0);
  /* the item staging gets the LDS this model's accumulator tile leaves (its least size is what the tile was sized against) */
  const size_t acc_words = (size_t)vote_lds_words(in.tile_refs, in.num_angles);
  p.run_seg = vote_run_seg(acc_words, (size_t)LDS_BYTES);
  if (in.run_seg_cap > 0) p.run_seg = std::max(64, std::min(p.run_seg, in.run_seg_cap / 64 * 64)); /* test knob: PPF_OPT_RUN_STAGING */
  p.vote_lds = vote_lds_fixed(p.run_seg) + acc_words * 4;
  if (p.vote_lds > (size_t)LDS_BYTES) return fail(PPF_ERR_INVALID, "match: model tile of %d reference points does not fit the LDS accumulator", in.tile_refs);
  /* k_group's dynamic LDS: one counter per bucket of a round, the prefix of the pool pieces */
  p.group_lds = (size_t)((p.round_buckets + 1) & ~1) * sizeof(uint32_t) + (size_t)((p.pair_chunks + 2) & ~1) * sizeof(uint32_t) * 2;
  if (p.group_lds + 2048 > (size_t)LDS_BYTES) return fail(PPF_ERR_INVALID, "match: %d paired points are more than one call can group", in.n_paired);
  *plan = p;
  return PPF_OK;
}

ppf_status ppf_debug_match_plan(const ppf_debug_match_plan_in* in, ppf_debug_match_plan_out* out) {
  if (!in || !out) return fail(PPF_ERR_INVALID, "ppf_debug_match_plan: NULL");
  memset(out, 0, sizeof(*out));
  if (in->n_ref < 1 || in->n_paired < 1 || in->tile_refs < 1 || in->num_angles < 1 || in->batch_refs_cap < 0 || in->round_buckets_cap < 0 ||
      in->run_seg_cap < 0)
    return fail(PPF_ERR_INVALID, "ppf_debug_match_plan: bad argument");
  return match_plan(*in, out);
}

/* ---- the steps of match_prepared ------------------------------------------------------------------------------------ */

/* 16-bit cells first, 32-bit cells for the (reference point, tile)s whose cells overflow -- until a call casts more than
 * PPF_ACC32_SWITCH of its votes twice that way: from then on 32-bit cells for everything (what they cost extra is less than
 * what the repeats cost: profiles/r04_c4_acc32_policies.md).  PPF_OPT_ACC32 = 3 instead sends the items that will cast at
 * least ws->heavy_votes votes straight to the 32-bit launch, decided on the device, per item, for THIS scene, before a vote
 * is cast (measured on C4: slower than either, the vote count of an item says little about its fullest cell). */
static bool acc32_for_all(const ppf_workspace* ws) { return ws->force_acc32 || (ws->acc32 && ws->acc32_policy == 0); }

/* the state of the call: model and its learned fractions, parameters, stream, the reference points it votes, zeroed stats */
static ppf_status match_reset(const ppf_model* m, ppf_workspace* ws, const ppf_match_params* params, hipStream_t st, bool retry) {
  if (ws->model != m) { /* another model: its own hit density (remembered if it has been here before) */
    workspace_remember_frac(ws);
    ws->acc32 = false;
    ws->heavy_votes = ~0ull; /* another table: its own limit, learned from its first call on */
    if (const ppf_workspace::Learned* fm = workspace_learned(ws, m, false)) {
      ws->frac = fm->frac;
      ws->frac_known = true;
    } else if (!ws->frac_by_model.empty()) {
      ws->frac_known = false; /* a model this workspace has not met: count first */
    }
  }
  workspace_hold_model(ws, m);
  HIPCHK(hipGetDevice(&ws->device));
  ws->params = *params;
  ws->stream = st;
  ws->clustered = false;
  ws->checked = false;
  ws->sum_valid = false;
  ws->final_poses.clear();
  const int retries = retry ? ws->stats.n_retries : 0;
  memset(&ws->stats, 0, sizeof(ws->stats));
  ws->stats.n_retries = retries;
  const int rows = ws->surf.n;
  const int scene_step = (int)(1.0 / params->relative_scene_sample_step);
  const int n_ref_total = (rows + scene_step - 1) / scene_step;
  const int n_ref = n_ref_total > params->ref_offset ? (n_ref_total - params->ref_offset + params->ref_stride - 1) / params->ref_stride : 0;
  ws->rows = rows;
  ws->n_ref_total = n_ref_total;
  ws->n_ref = n_ref;
  ws->n_batches = 0;
  ws->stats.n_scene_sampled = rows;
  ws->stats.n_paired = ws->has_edge ? ws->edge.n : rows;
  ws->stats.n_ref = n_ref;
  ws->pending = true;
  return PPF_OK;
}

/* what the call keeps per reference point (and tile): reserved, cleared where a kernel accumulates, and named in va */
static ppf_status match_call_buffers(ppf_workspace* ws, MatchArgs& va) {
  const ppf_model* m = ws->model;
  const int n_ref = ws->n_ref, T = m->info.n_tiles;
  hipStream_t st = ws->stream;
  HIPCHK(ws->partial.reserve((size_t)n_ref * T * 2));
  HIPCHK(ws->half_edge.reserve((size_t)n_ref * T * 2));
  HIPCHK(ws->ovf_items.reserve((size_t)n_ref * T));
  if (ws->acc32_policy == 3) {
    HIPCHK(ws->item_votes.reserve((size_t)n_ref * T));
    HIPCHK(ws->need_hist.reserve(2 * ACC_HIST));
  }
  const size_t n_cnt = (size_t)n_ref * T + n_ref + 16; /* cellsum | pairs | totals[2] | tally[14]: LDS operations, hits, runs, 32-bit items, votes cast twice, count tables, 8 phase clocks (diagnostic build) */
  HIPCHK(ws->counters.reserve(n_cnt));
  HIPCHK(ws->votes.reserve(n_ref));
  HIPCHK(ws->raw_poses.reserve(n_ref));
  if (ws->timing) HIPCHK(hipEventRecord(ws->ev[0], st));
  /* counters, ovf_items, the cursors and table_desc are cleared by k_frames (of the first batch / of every batch) */
  if (ws->acc_dump) /* debug dump of the full accumulators: a repeat of the call starts from zeros again (one of its cells is accumulated, not assigned) */
    HIPCHK(hipMemsetAsync(ws->acc_dump, 0, (size_t)n_ref * (size_t)m->info.n_ref * (size_t)m->info.num_angles * sizeof(uint32_t), st));
  if (ws->acc32_policy == 3) {
    HIPCHK(hipMemsetAsync(ws->need_hist.p, 0, 2 * ACC_HIST * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(ws->item_votes.p, 0, (size_t)n_ref * T * sizeof(unsigned long long), st));
  }
  va.partial = ws->partial.p;
  va.edge = ws->half_edge.p;
  va.ovf_items = ws->ovf_items.p;
  va.cellsum = ws->counters.p;
  va.pairs = ws->counters.p + (size_t)n_ref * T;
  va.tally = ws->counters.p + (size_t)n_ref * T + n_ref + 2;
  va.acc_dump = ws->acc_dump;
  va.item_votes = (!acc32_for_all(ws) && ws->acc32_policy == 3) ? ws->item_votes.p : nullptr;
  va.heavy_votes = ws->heavy_votes;
  va.n_counters = n_cnt;
  va.n_ovf_items = (unsigned long long)n_ref * T;
  return PPF_OK;
}

/* the clouds, the model's tables and the call's parameters; the cursors */
static ppf_status match_args(ppf_workspace* ws, MatchArgs& va) {
  const ppf_model* m = ws->model;
  const ppf_match_params* params = &ws->params;
  va.surf = ws->surf.view();
  va.paired = ws->has_edge ? ws->edge.view() : ws->surf.view();
  va.same_cloud = ws->has_edge ? 0 : 1;
  va.scene_step = (int)(1.0 / params->relative_scene_sample_step); va.ref_offset = params->ref_offset; va.ref_stride = params->ref_stride;
  va.slotmap = m->slotmap.p; va.slot_mask = m->info.slots - 1;
  va.key_lut = m->key_lut.p; va.kd = m->kd;
  va.bucket_off = m->bucket_off.p; va.n_buckets = (int)m->info.n_buckets;
  va.records = m->records.p;
  va.n_tiles = m->info.n_tiles; va.tile_refs = m->info.tile_refs; va.num_angles = m->info.num_angles; va.n_model = m->info.n_ref;
  va.angle_step = m->info.angle_step; va.dist_step = m->info.distance_step;
  va.bucket_total = m->bucket_total.p;
  va.bucket_mid = m->bucket_mid.p;
  va.grp_records = m->n_grp_records ? m->grp_records.p : nullptr;
  va.grp_hdr = m->n_grp_records ? m->grp_hdr.p : nullptr;
  va.key_exact = m->params.key_equality == PPF_KEY_EXACT;
  va.pair_radius = params->pair_radius;
  va.pair_chunks = pair_chunks_of(va.paired.n);
  va.agg_min_hits = (params->vote_mode == PPF_VOTE_DIRECT || params->alpha_range_2pi || m->info.num_angles > AGG_MAX_ANGLES) ? 0 : PPF_AGG_MIN_HITS;
  const bool cursors_new = !ws->cursors.p;
  HIPCHK(ws->cursors.reserve(CUR_WORDS));
  va.cursors = ws->cursors.p;
  if (cursors_new) HIPCHK(hipMemsetAsync(ws->cursors.p, 0, CUR_WORDS * sizeof(uint32_t), ws->stream)); /* k_frames never clears cursors[CUR_ODDVALUES]: a fresh block must not hold a launch's number by chance (see odd_epoch; 0, which the cold pass and the wrap below write, is no launch's number) */
  return PPF_OK;
}

/* Cold workspace: nothing is known about this scene's hit density, so the pair kernel first only counts its hits
 * (same arithmetic, nothing stored) and the pools are sized from the exact number.  Costs one extra pair pass and
 * one wait for the device, once: later calls size their pools from what the previous call saw. */
static ppf_status match_cold_count(ppf_workspace* ws, MatchArgs& va, bool darboux) {
  hipStream_t st = ws->stream;
  const int n_ref = ws->n_ref;
  HIPCHK(hipMemsetAsync(ws->cursors.p, 0, CUR_WORDS * sizeof(uint32_t), st));
  va.count_only = 1;
  va.stripe_bits = 6;
  for (int base = 0; base < n_ref; base += 32768) {
    va.ref_base = base;
    va.n_ref = std::min(32768, n_ref - base);
    launch_pairs(va, darboux, st);
    HIPCHK(hipGetLastError());
  }
  va.count_only = 0;
  std::vector<uint32_t> cw(CUR_SORTED);
  HIPCHK(hipMemcpyAsync(cw.data(), ws->cursors.p, cw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(host_stream_sync(st));
  unsigned long long hits = 0;
  for (int sidx = 0; sidx < POOL_STRIPES; sidx++)
    hits += (unsigned long long)cw[sidx * CUR_STRIDE] | ((unsigned long long)cw[sidx * CUR_STRIDE + 1] << 32);
  ws->frac.learn_hits(hits, (double)n_ref * (double)va.paired.n);
  ws->frac_known = true;
  return PPF_OK;
}

/* the hit scratch of one batch, sized by the plan, and the plan's numbers into va */
static ppf_status match_reserve(ppf_workspace* ws, const MatchPlan& p, MatchArgs& va) {
  HIPCHK(ws->frames.reserve((size_t)p.batch * 12));
  HIPCHK(ws->raw.fit((size_t)p.stripe_cap << p.stripe_bits));
  HIPCHK(ws->chunk_desc.reserve((size_t)p.batch * p.pair_chunks));
  HIPCHK(ws->hit_count.reserve(p.batch));
  HIPCHK(ws->s_a64.fit(p.sorted_cap));
  HIPCHK(ws->runs.fit(p.run_cap));
  HIPCHK(ws->tables.fit((size_t)p.table_cap * TBL_BYTES));
  HIPCHK(ws->table_desc.fit(p.table_cap));
  HIPCHK(ws->run_blocks.reserve((size_t)p.batch * p.n_rounds));
  HIPCHK(ws->work.reserve(p.batch));
  HIPCHK(ws->perm.reserve(p.batch));
  HIPCHK(ws->perm_group.reserve(p.batch));
  HIPCHK(ws->ovf_list.reserve((size_t)p.batch * va.n_tiles));
  ws->stats.scratch_bytes = ws->frames.bytes() + ws->raw.bytes() + ws->cursors.bytes() + ws->chunk_desc.bytes() + ws->hit_count.bytes() +
                            ws->s_a64.bytes() + ws->runs.bytes() + ws->run_blocks.bytes() + ws->tables.bytes() + ws->table_desc.bytes() +
                            ws->work.bytes() + ws->perm.bytes() + ws->perm_group.bytes();
  va.n_rounds = p.n_rounds; va.round_buckets = p.round_buckets; va.run_seg = p.run_seg;
  va.ovf_list = ws->ovf_list.p;
  va.frames = ws->frames.p;
  va.raw = ws->raw.p; va.stripe_cap = p.stripe_cap; va.stripe_bits = p.stripe_bits;
  va.chunk_desc = ws->chunk_desc.p; va.hit_count = ws->hit_count.p;
  va.s_a64 = ws->s_a64.p; va.sorted_cap = p.sorted_cap;
  va.runs = ws->runs.p; va.run_cap = p.run_cap; va.run_blocks = ws->run_blocks.p;
  va.tables = ws->tables.p; va.table_desc = ws->table_desc.p; va.table_cap = p.table_cap;
  va.work = ws->work.p; va.perm = ws->perm.p; va.perm_group = ws->perm_group.p;
  ws->n_batches = p.n_batches;
  ws->stats.n_batches = p.n_batches;
  if (ws->timing)
    while (ws->batch_ev.size() < ws->ev_base + (size_t)p.n_batches * 4) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreate(&e));
      ws->batch_ev.push_back(e);
    }
  return PPF_OK;
}

/* One batch of reference points, va.ref_base .. + va.n_ref: frames, pairs, rank, group, tables, rank, vote16, vote32.
 * `ev` is the batch's four events (timing on) or NULL. */
static ppf_status match_enqueue_batch(ppf_workspace* ws, MatchArgs& va, const MatchPlan& p, bool darboux, const hipEvent_t* ev) {
  hipStream_t st = ws->stream;
#if PPF_ABL_GROUP != 1 /* attribution builds of k_group store no payload: the later kernels read zeros, never stale values */
  HIPCHK(hipMemsetAsync(ws->s_a64.p, 0, ws->s_a64.cap * sizeof(*ws->s_a64.p), st));
#endif
  /* k_frames clears the batch's cursors and table_desc on the side, for the first batch also the call's counters, ovf_items and
   * the overflow word (which lives on through the later batches); it raises "odd values" by writing this launch's own number.
   * A thread per reference point, and enough threads for its look at the paired points (40 waves walking 50,000 points: 10 us) */
  k_frames<<<dim3(std::max((va.n_ref + 63) / 64, std::min((va.paired.n + 63) / 64, 1024))), dim3(64), 0, st>>>(va);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev[0], st));
  launch_pairs(va, darboux, st);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev[1], st));
  /* k_group takes the reference points with the most hits first */
  k_rank<<<dim3((va.n_ref + RANK_KEYS - 1) / RANK_KEYS), dim3(256), 0, st>>>(va.hit_count, va.n_ref, nullptr, ws->perm_group.p, nullptr);
  k_group<<<dim3(va.n_ref), dim3(GROUP_BLOCK), p.group_lds, st>>>(va);
  HIPCHK(hipGetLastError());
  if (va.agg_min_hits) { /* the count tables of the batch's many-hit runs, once per run */
    k_tables<<<dim3((p.table_cap + TABLE_BLOCK / 64 - 1) / (TABLE_BLOCK / 64)), dim3(TABLE_BLOCK), 0, st>>>(va);
    HIPCHK(hipGetLastError());
  }
  /* k_vote takes the reference points that will cast the most votes first */
  k_rank<<<dim3((va.n_ref + RANK_KEYS - 1) / RANK_KEYS), dim3(256), 0, st>>>(va.work, va.n_ref, nullptr, va.perm, nullptr);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev[2], st));
  const bool acc32_all = acc32_for_all(ws), wrap = ws->params.alpha_range_2pi != 0;
  const dim3 grid16((unsigned)((size_t)va.n_ref * va.n_tiles)), grid32((unsigned)((size_t)va.n_ref * va.n_tiles * 2));
  if (!acc32_all) {
    va.acc32 = 0;
    launch_vote(va, wrap, false, grid16, p.vote_lds, st);
    HIPCHK(hipGetLastError());
  }
  va.acc32 = acc32_all ? 1 : 2; /* 2: the (reference point, tile)s the 16-bit launch listed, over a grid that does not depend on their number */
  /* one workgroup per CU walks the list (a launch of 1,024 with nothing to do: 10 us) */
  launch_vote(va, wrap, true, acc32_all ? grid32 : dim3(std::min(grid32.x, 256u)), p.vote_lds, st);
  va.acc32 = 0;
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev[3], st));
  return PPF_OK;
}

/* after the last batch: the poses of the reference points, their clusters, and the summary the host reads first */
static ppf_status match_enqueue_tail(ppf_workspace* ws, const MatchArgs& va) {
  const ppf_model* m = ws->model;
  const ppf_match_params* params = &ws->params;
  hipStream_t st = ws->stream;
  const int n_ref = ws->n_ref, T = m->info.n_tiles;
  FinalArgs fa;
  fa.surf = ws->surf.view(); fa.model = m->cloud.view();
  fa.scene_step = va.scene_step; fa.ref_offset = params->ref_offset; fa.ref_stride = params->ref_stride; fa.n_ref = n_ref;
  fa.n_tiles = T; fa.tile_refs = m->info.tile_refs; fa.num_angles = m->info.num_angles;
  fa.alpha_2pi = params->alpha_range_2pi != 0;
  fa.acc32 = acc32_for_all(ws) ? 1 : 0; fa.ovf_items = ws->ovf_items.p; fa.edge = ws->half_edge.p;
  fa.partial = ws->partial.p; fa.cellsum = va.cellsum; fa.pairs = va.pairs;
  fa.votes = ws->votes.p; fa.poses = ws->raw_poses.p;
  fa.totals = ws->counters.p + (size_t)n_ref * T + n_ref;
  fa.item_votes = va.item_votes; fa.need_hist = va.item_votes ? ws->need_hist.p : nullptr;
  fa.vkeys = nullptr;
  if (!params->skip_clustering) { /* the clustering ranks the poses by their votes: k_finalize leaves the keys where enqueue_cluster looks for them */
    HIPCHK(ws->cl_votes.reserve(2 * (size_t)n_ref));
    fa.vkeys = ws->cl_votes.p + n_ref;
  }
  k_finalize<<<dim3((n_ref + 63) / 64), dim3(64), 0, st>>>(fa);
  HIPCHK(hipGetLastError());
  if (!params->skip_clustering) {
    double pos, rot;
    resolve_thresholds(m, params, &pos, &rot);
    /* the reference clusters sampled.rows / sceneSamplingStep poses (integer division: the lowest-voted
     * pose is dropped when the stride does not divide the row count); a shard clusters its own share */
    const int num = (params->ref_stride == 1 && params->ref_offset == 0) ? ws->rows / va.scene_step : n_ref;
    const ppf_status s = enqueue_cluster(ws, ws->raw_poses.p, n_ref, num, pos, rot, params->use_weighted_avg != 0, st, params->rot_metric_relative != 0, true);
    if (s != PPF_OK) return s;
    ws->clustered = true;
  }
  if (ws->timing) HIPCHK(hipEventRecord(ws->ev[1], st));
  if (!ws->h_sum) HIPCHK(hipHostMalloc((void**)&ws->h_sum, 32 * sizeof(unsigned long long), hipHostMallocDefault));
  k_summary<<<dim3(1), dim3(64), 0, st>>>(fa.totals, ws->cursors.p + CUR_OVERFLOW, ws->clustered ? ws->cl_u32.p : nullptr, ws->h_sum);
  HIPCHK(hipGetLastError());
  ws->sum_valid = true;
  return PPF_OK;
}

/* everything after A2: frames -> pairs -> group -> rank -> vote -> finalize -> cluster, on the clouds held by ws.
 * Nothing here waits for the device: the hit pools are sized by match_plan from ws->frac (learned from the previous
 * calls); a pool that turns out too small raises a device flag, which the first accessor of the results reads
 * (workspace_finish) and answers by repeating the call with bigger pools. */
static ppf_status match_prepared(const ppf_model* m, ppf_workspace* ws, const ppf_match_params* params, hipStream_t st, bool retry) {
  ppf_status s = match_reset(m, ws, params, st, retry);
  if (s != PPF_OK || ws->n_ref == 0) return s;
  const bool darboux = m->params.feature == PPF_FEATURE_DARBOUX;
  MatchArgs va;
  memset(&va, 0, sizeof(va));
  if ((s = match_call_buffers(ws, va)) != PPF_OK) return s;
  if ((s = match_args(ws, va)) != PPF_OK) return s;
  if (!ws->frac_known && (s = match_cold_count(ws, va, darboux)) != PPF_OK) return s;
  MatchPlan plan;
  const MatchPlanIn in = {ws->n_ref, va.paired.n, ws->frac.hit, ws->frac.run, ws->frac.tbl, va.agg_min_hits != 0, ws->batch_refs_cap,
                          ws->round_buckets_cap, ws->run_seg_cap, m->info.n_buckets, m->info.tile_refs, m->info.num_angles};
  if ((s = match_plan(in, &plan)) != PPF_OK) return s;
  if ((s = match_reserve(ws, plan, va)) != PPF_OK) return s;
  HIPCHK(match_kernel_attributes());
  for (int bi = 0; bi < plan.n_batches; bi++) {
    va.ref_base = bi * plan.batch;
    va.n_ref = std::min(plan.batch, ws->n_ref - va.ref_base);
    va.first_batch = bi == 0;
    if (++ws->odd_epoch == 0u) { /* wrapped: a word left by the launch 2^32 before this one must not match */
      HIPCHK(hipMemsetAsync(ws->cursors.p + CUR_ODDVALUES, 0, sizeof(uint32_t), st));
      ws->odd_epoch = 1u;
    }
    va.odd_epoch = ws->odd_epoch;
    if ((s = match_enqueue_batch(ws, va, plan, darboux, ws->timing ? &ws->batch_ev[ws->ev_base + (size_t)bi * 4] : nullptr)) != PPF_OK) return s;
  }
  return match_enqueue_tail(ws, va);
}

/* the batch events of a call (four per batch from `base`: pairs start / end, vote start / end) as milliseconds, added to the three sums */
static ppf_status add_batch_ms(const ppf_workspace* ws, size_t base, int n_batches, float* pair, float* group, float* vote) {
  for (int b = 0; b < n_batches; b++) {
    const hipEvent_t* e = &ws->batch_ev[base + (size_t)b * 4];
    float t0 = 0, t1 = 0, t2 = 0;
    HIPCHK(hipEventElapsedTime(&t0, e[0], e[1]));
    HIPCHK(hipEventElapsedTime(&t1, e[1], e[2]));
    HIPCHK(hipEventElapsedTime(&t2, e[2], e[3]));
    *pair += t0; *group += t1; *vote += t2;
  }
  return PPF_OK;
}

/* PPF_OPT_ACC32 = 3, the limit of the next call: k_finalize filed the votes of every (reference point, tile) under its size
 * class, as "needed 32-bit cells" (a cell beyond 65,535; hist[class]) or "did not" (hist[ACC_HIST + class]).  An item sent to
 * 32-bit cells costs about PPF_ACC32_COST of what 16-bit cells cost it; one that overflows 16-bit cells costs
 * 1 + PPF_ACC32_COST.  The class boundary that makes the sum smallest becomes the limit (none above every class: the scene
 * needs no 32-bit cells). */
static unsigned long long acc32_heavy_votes(const unsigned long long* hist) {
  double best = -1;
  int best_k = ACC_HIST;
  double above = 0, below = 0; /* cost of the classes >= k (sent to 32-bit cells) / < k (tried with 16-bit cells) */
  for (int b = 0; b < ACC_HIST; b++) below += (double)hist[ACC_HIST + b] + (1.0 + PPF_ACC32_COST) * (double)hist[b];
  for (int k = ACC_HIST; k >= 0; k--) {
    if (k < ACC_HIST) {
      const double need = (double)hist[k], rest = (double)hist[ACC_HIST + k];
      above += PPF_ACC32_COST * (need + rest);
      below -= rest + (1.0 + PPF_ACC32_COST) * need;
    }
    const double cost = above + below;
    if (best < 0 || cost < best) { best = cost; best_k = k; }
  }
  const unsigned long long heavy_votes = best_k >= ACC_HIST ? ~0ull : acc_hist_lower(best_k);
  if (getenv("PPF_DEBUG_ACC32")) {
    for (int b = 0; b < ACC_HIST; b++)
      if (hist[b] || hist[ACC_HIST + b])
        fprintf(stderr, "acc32 class %3d (>= %llu votes): needed %llu  not needed %llu\n", b, acc_hist_lower(b), hist[b], hist[ACC_HIST + b]);
    fprintf(stderr, "acc32 limit -> class %d (%llu votes)\n", best_k, heavy_votes);
  }
  return heavy_votes;
}

/* Wait for the workspace's pending call and make sure it ran with big enough hit pools: when a pool overflowed (device
 * flag), the call is repeated on the same stream with grown fractions, until it fits (at frac.hit == 1 the pools
 * hold every scene pair).  Then reads the counters and learns the fractions for the next call. */
static ppf_status workspace_finish(ppf_workspace* ws) {
  if (!ws->pending) return fail(PPF_ERR_INVALID, "no call in this workspace");
  HIPCHK(host_stream_sync(ws->stream));
  if (ws->checked || ws->n_ref == 0) { ws->checked = true; return PPF_OK; }
  unsigned long long tot[16];
  for (;;) {
    uint32_t ovf = 0;
    if (ws->sum_valid) { /* k_summary wrote them into pinned memory as the call's last act */
      memcpy(tot, ws->h_sum, sizeof(tot));
      ovf = (uint32_t)ws->h_sum[16];
    } else {
      HIPCHK(host_read(tot, ws->counters.p + (size_t)ws->n_ref * ws->model->info.n_tiles + ws->n_ref, sizeof(tot)));
      HIPCHK(host_read(&ovf, ws->cursors.p + CUR_OVERFLOW, sizeof(ovf)));
    }
    if (!ovf) break;
    if (ws->frac.hit >= 1.0) {
      ws->pools_failed = true; /* not the caller's output buffer: a context in this state is not kept (HostLoan) */
      return fail(PPF_ERR_CAPACITY, "match: hit pools overflowed at worst-case size (flags %u)", ovf);
    }
    ws->frac.grow(ovf);
    ws->stats.n_retries++;
    const ppf_match_params p = ws->params;
    ppf_status s = match_prepared(ws->model, ws, &p, ws->stream, true);
    if (s != PPF_OK) return s;
    HIPCHK(host_stream_sync(ws->stream));
  }
  ws->stats.n_votes = tot[0];
  ws->stats.n_pairs = tot[1];
  ws->stats.n_lds_atomics = tot[2];
  ws->stats.n_hits = tot[3];
  ws->stats.n_acc32_items = tot[5];
  ws->stats.n_tables = tot[7];
  for (int k = 0; k < 8; k++) ws->stats.phase_clocks[k] = tot[8 + k];
  if (ws->clustered) {
    uint32_t nf = 0;
    if (ws->sum_valid) nf = (uint32_t)ws->h_sum[17];
    else HIPCHK(host_read(&nf, ws->cl_u32.p, sizeof(uint32_t)));
    ws->stats.n_poses = (int)nf;
  }
  ws->frac.learn(tot);
  ws->frac_known = true;
  if (!ws->acc32 && ws->acc32_policy == 0 && (double)tot[6] > PPF_ACC32_SWITCH * (double)tot[0]) ws->acc32 = true;
  if (!ws->force_acc32 && ws->acc32_policy == 3) {
    unsigned long long hist[2 * ACC_HIST];
    HIPCHK(host_read(hist, ws->need_hist.p, sizeof(hist)));
    ws->heavy_votes = acc32_heavy_votes(hist);
  }
  if (ws->timing) {
    const ppf_status s = add_batch_ms(ws, ws->ev_base, ws->n_batches, &ws->stats.ms_pair_kernel, &ws->stats.ms_group_kernel, &ws->stats.ms_vote_kernel);
    if (s != PPF_OK) return s;
    HIPCHK(hipEventElapsedTime(&ws->stats.ms_total_device, ws->ev[0], ws->ev[1]));
  }
  ws->checked = true;
  return PPF_OK;
}

ppf_status ppf_workspace_results(ppf_workspace* ws, ppf_vote* votes, ppf_pose* raw_poses, int cap_ref, int* n_ref,
                                 ppf_pose* poses, int cap_poses, int* n_poses, ppf_match_stats* stats) {
  if (!ws || !ws->pending) return fail(PPF_ERR_INVALID, "ppf_workspace_results: no call in this workspace");
  ppf_status sf = workspace_finish(ws);
  if (sf != PPF_OK) return sf;
  const int nr = ws->n_ref;
  if (n_ref) *n_ref = nr;
  if ((votes || raw_poses) && cap_ref < nr) return fail(PPF_ERR_CAPACITY, "ppf_workspace_results: need room for %d reference points", nr);
  if (nr > 0) {
    if (votes) HIPCHK(host_read(votes, ws->votes.p, (size_t)nr * sizeof(ppf_vote)));
    if (raw_poses) HIPCHK(host_read(raw_poses, ws->raw_poses.p, (size_t)nr * sizeof(ppf_pose)));
  }
  if ((poses || n_poses) && ws->clustered) {
    if (ws->final_poses.empty() && nr > 0) {
      uint32_t nf = 0;
      if (ws->sum_valid) nf = (uint32_t)ws->h_sum[17];
      else HIPCHK(host_read(&nf, ws->cl_u32.p, sizeof(uint32_t)));
      ws->final_poses.resize(nf);
      if (nf) HIPCHK(host_read(ws->final_poses.data(), ws->d_final.p, (size_t)nf * sizeof(ppf_pose)));
    }
    ws->stats.n_poses = (int)ws->final_poses.size();
    if (n_poses) *n_poses = (int)ws->final_poses.size();
    if (poses) {
      if (cap_poses < (int)ws->final_poses.size())
        return fail(PPF_ERR_CAPACITY, "ppf_workspace_results: need room for %d poses", (int)ws->final_poses.size());
      memcpy(poses, ws->final_poses.data(), ws->final_poses.size() * sizeof(ppf_pose));
    }
  } else if (n_poses) {
    *n_poses = 0;
  }
  if (stats) *stats = ws->stats;
  return PPF_OK;
}

static ppf_status run_host(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                           int estride, int enoff, const ppf_match_params* params, ppf_workspace* ws);

ppf_status ppf_workspace_ref_counters(ppf_workspace* ws, uint64_t* votes_per_ref, uint64_t* pairs_per_ref, int cap) {
  if (!ws || !ws->pending) return fail(PPF_ERR_INVALID, "ppf_workspace_ref_counters: no call in this workspace");
  ppf_status sf = workspace_finish(ws);
  if (sf != PPF_OK) return sf;
  const int nr = ws->n_ref;
  if (cap < nr) return fail(PPF_ERR_CAPACITY, "ppf_workspace_ref_counters: need room for %d reference points", nr);
  if (nr == 0) return PPF_OK;
  const int T = ws->model->info.n_tiles;
  std::vector<unsigned long long> h((size_t)nr * T + nr);
  HIPCHK(hipMemcpy(h.data(), ws->counters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int r = 0; r < nr; r++) {
    unsigned long long v = 0;
    for (int t = 0; t < T; t++) v += h[(size_t)r * T + t];
    if (votes_per_ref) votes_per_ref[r] = v;
    if (pairs_per_ref) pairs_per_ref[r] = h[(size_t)nr * T + r];
  }
  return PPF_OK;
}

/* the dump runs on the caller's workspace: its options (32-bit cells, staging segments, group rounds, batches, pool fractions),
 * its learned pool estimates and its 16/32-bit decision all apply, and the call's results stay readable through
 * ppf_workspace_results / ppf_workspace_ref_counters.  ws->acc_dump is set for this one call and cleared on every way out. */
ppf_status ppf_debug_accumulators_ws(const ppf_model* m, ppf_workspace* ws, const float* scene, int ns, int sstride, int snoff,
                                     const float* edge, int ne, int estride, int enoff, const ppf_match_params* params, uint32_t* acc,
                                     size_t cap_words, int* n_ref) {
  if (!m || !ws || !acc || !params) return fail(PPF_ERR_INVALID, "ppf_debug_accumulators: bad argument");
  ppf_match_params p = *params;
  const size_t per_ref = (size_t)m->info.n_ref * m->info.num_angles;
  if (!(p.relative_scene_sample_step <= 1 && p.relative_scene_sample_step > 0) || p.ref_stride < 1 || p.ref_offset < 0 || ns <= 0)
    return fail(PPF_ERR_INVALID, "ppf_debug_accumulators: bad argument");
  const int scene_step = (int)(1.0 / p.relative_scene_sample_step);
  if (!p.presampled) return fail(PPF_ERR_INVALID, "ppf_debug_accumulators: presampled clouds only");
  const int n_ref_total = (ns + scene_step - 1) / scene_step;
  const int nr = n_ref_total > p.ref_offset ? (n_ref_total - p.ref_offset + p.ref_stride - 1) / p.ref_stride : 0;
  if (cap_words < per_ref * nr) return fail(PPF_ERR_CAPACITY, "ppf_debug_accumulators: need %zu words", per_ref * nr);
  DevBuf<uint32_t> dump;
  struct Reset { /* also after an error: a later call of the workspace must not write into a block that went back to the cache */
    ppf_workspace* w;
    ~Reset() { w->acc_dump = nullptr; }
  } reset{ws};
  HIPCHK(dump.reserve(std::max<size_t>(per_ref * nr, 1)));
  HIPCHK(hipMemset(dump.p, 0, per_ref * nr * sizeof(uint32_t)));
  ws->acc_dump = dump.p;
  p.skip_clustering = 1;
  ppf_status s = run_host(m, scene, ns, sstride, snoff, edge, ne, estride, enoff, &p, ws);
  /* a workspace sizes its pools from estimates: when one ran out, runs were left out of the vote and the dump is incomplete.
   * workspace_finish reads the flag and repeats the call with bigger pools (match_prepared clears the dump first) -- without it
   * this entry returned a partial accumulator whenever the table pool's first guess was too small, depending on which
   * reference points reached the pool first */
  if (s == PPF_OK) s = workspace_finish(ws);
  if (s != PPF_OK) {
    if (have_device()) (void)hipDeviceSynchronize(); /* nothing may still write the dump when it goes back to the block cache */
    return s;
  }
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(hipMemcpy(acc, dump.p, per_ref * nr * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_ref) *n_ref = nr;
  return PPF_OK;
}

/* the same on a fresh workspace: cold, default options */
ppf_status ppf_debug_accumulators(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                                  int estride, int enoff, const ppf_match_params* params, uint32_t* acc, size_t cap_words,
                                  int* n_ref) {
  if (!m || !acc || !params) return fail(PPF_ERR_INVALID, "ppf_debug_accumulators: bad argument");
  ppf_workspace ws;
  return ppf_debug_accumulators_ws(m, &ws, scene, ns, sstride, snoff, edge, ne, estride, enoff, params, acc, cap_words, n_ref);
}

/* the block cache's size class for a request (host only): what DevBuf is granted for `bytes` */
size_t ppf_debug_block_size(size_t bytes) {
  return DevPool::class_size(DevPool::class_of(std::max<size_t>(bytes, 256)));
}

/* the block cache's guard mode (ppf_device_mem.h) */
ppf_status ppf_debug_pool_guard(int mode) {
  if (mode < 0 || mode > 2) return fail(PPF_ERR_INVALID, "ppf_debug_pool_guard: mode is 0 (off), 1 or 2");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_debug_pool_guard: no HIP device");
  DevPool::get().set_guard(mode);
  return PPF_OK;
}

ppf_status ppf_debug_pool_check(ppf_debug_pool_report* r) {
  if (!r) return fail(PPF_ERR_INVALID, "ppf_debug_pool_check: NULL");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_debug_pool_check: no HIP device");
  HIPCHK(DevPool::get().check(r));
  return PPF_OK;
}

ppf_status ppf_debug_device_math(int fn, const double* x, const double* y, double* out, int n) {
  if (!x || !out || n <= 0 || fn < 0 || fn > 5) return fail(PPF_ERR_INVALID, "ppf_debug_device_math: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_debug_device_math: no HIP device");
  DevBuf<double> dx, dy, dout;
  HIPCHK(dx.reserve(n));
  HIPCHK(dy.reserve(n));
  HIPCHK(dout.reserve(n));
  HIPCHK(hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy.p, y ? y : x, (size_t)n * 8, hipMemcpyHostToDevice));
  k_debug_math<<<dim3((n + 255) / 256), dim3(256)>>>(fn, dx.p, dy.p, dout.p, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return PPF_OK;
}

ppf_status ppf_workspace_device_poses(ppf_workspace* ws, void** d_raw_poses, int* n_ref) {
  if (!ws || !ws->pending || !d_raw_poses) return fail(PPF_ERR_INVALID, "ppf_workspace_device_poses: bad argument");
  *d_raw_poses = ws->raw_poses.p;
  if (n_ref) *n_ref = ws->n_ref;
  return PPF_OK;
}

/* copy `cap` pose records to dst: the first min(n, cap) from src, zeros after them (num_votes == 0 marks an empty row);
 * n comes from the device (n_dev) when given.  Optionally also saves the count, the overflow flag of the call and its
 * four 64-bit totals (votes, pairs, LDS operations, hits) next to the block: what a batch needs per (crop, model). */
__global__ __launch_bounds__(256) void k_pose_block(const ppf_pose* __restrict__ src, const uint32_t* __restrict__ n_dev, int n_host,
                                                    ppf_pose* __restrict__ dst, int cap, uint32_t* __restrict__ meta_out,
                                                    const uint32_t* __restrict__ flag_in, unsigned long long* __restrict__ tot_out,
                                                    const unsigned long long* __restrict__ tot_in) {
  constexpr int W = (int)(sizeof(ppf_pose) / 8);
  const int n = n_dev ? (int)*n_dev : n_host;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap * W) {
    const int row = i / W;
    const unsigned long long* s64 = reinterpret_cast<const unsigned long long*>(src);
    reinterpret_cast<unsigned long long*>(dst)[i] = row < n ? s64[i] : 0ull;
  }
  if (i == 0 && meta_out) { meta_out[0] = (uint32_t)n; meta_out[1] = flag_in ? *flag_in : 0u; }
  if (i < 8 && tot_out && tot_in) tot_out[i] = tot_in[i]; /* votes, pairs, LDS operations, hits, runs, (two of k_vote's own), count tables */
}

ppf_status ppf_workspace_copy_top_poses(ppf_workspace* ws, void* d_dst, int k, void* stream) {
  if (!ws || !ws->pending || !d_dst || k <= 0) return fail(PPF_ERR_INVALID, "ppf_workspace_copy_top_poses: bad argument");
  if (!ws->clustered || ws->n_ref == 0) {
    HIPCHK(hipMemsetAsync(d_dst, 0, (size_t)k * sizeof(ppf_pose), (hipStream_t)stream));
    return PPF_OK;
  }
  const int words = k * (int)(sizeof(ppf_pose) / 8);
  k_pose_block<<<dim3((words + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(ws->d_final.p, ws->cl_u32.p, 0, (ppf_pose*)d_dst, k, nullptr,
                                                                                 nullptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

ppf_status ppf_workspace_copy_raw_poses(ppf_workspace* ws, void* d_dst, int cap, void* stream) {
  if (!ws || !ws->pending || !d_dst || cap <= 0) return fail(PPF_ERR_INVALID, "ppf_workspace_copy_raw_poses: bad argument");
  if (cap < ws->n_ref) return fail(PPF_ERR_CAPACITY, "ppf_workspace_copy_raw_poses: need room for %d reference points", ws->n_ref);
  if (ws->n_ref == 0) {
    HIPCHK(hipMemsetAsync(d_dst, 0, (size_t)cap * sizeof(ppf_pose), (hipStream_t)stream));
    return PPF_OK;
  }
  const int words = cap * (int)(sizeof(ppf_pose) / 8);
  k_pose_block<<<dim3((words + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(ws->raw_poses.p, nullptr, ws->n_ref, (ppf_pose*)d_dst, cap,
                                                                                 nullptr, nullptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

ppf_status ppf_cluster_poses_device(const ppf_model* m, ppf_workspace* ws, const void* d_in, int n, int num_poses,
                                    const ppf_match_params* params, void* stream) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "ppf_cluster_poses_device: model is NULL");
  if (!ws || (!d_in && n > 0) || n < 0 || !params) return fail(PPF_ERR_INVALID, "ppf_cluster_poses_device: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_cluster_poses_device: no HIP device (this engine has no CPU fallback)");
  workspace_hold_model(ws, m);
  HIPCHK(hipGetDevice(&ws->device));
  ws->params = *params;
  ws->stream = (hipStream_t)stream;
  ws->final_poses.clear();
  memset(&ws->stats, 0, sizeof(ws->stats));
  ws->n_ref = 0; ws->n_ref_total = 0; ws->n_batches = 0;
  ws->pending = true; ws->checked = true; /* no hit pools involved */
  ws->sum_valid = false;
  ws->clustered = false;
  if (n == 0) return PPF_OK;
  double pos, rot;
  resolve_thresholds(m, params, &pos, &rot);
  ppf_status s = enqueue_cluster(ws, (const ppf_pose*)d_in, n, num_poses, pos, rot, params->use_weighted_avg != 0, (hipStream_t)stream,
                                 params->rot_metric_relative != 0);
  if (s != PPF_OK) return s;
  ws->clustered = true;
  ws->n_ref = n; /* d_final / cl_u32 hold the clusters; results come back through ppf_workspace_results(poses) / _copy_top_poses */
  ws->stats.n_ref = n;
  return PPF_OK;
}

ppf_status ppf_cluster_poses(const ppf_model* m, const ppf_pose* in, int n, int num_poses,
                             const ppf_match_params* params, ppf_pose* out, int cap, int* n_out) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "ppf_cluster_poses: model is NULL");
  if ((!in && n > 0) || n < 0 || !params || !n_out) return fail(PPF_ERR_INVALID, "ppf_cluster_poses: bad argument");
  *n_out = 0;
  if (n == 0) return PPF_OK;
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_cluster_poses: no HIP device (this engine has no CPU fallback)");
  ppf_workspace ws;
  DevBuf<ppf_pose> d_in;
  HIPCHK(d_in.reserve(n));
  HIPCHK(hipMemcpy(d_in.p, in, (size_t)n * sizeof(ppf_pose), hipMemcpyHostToDevice));
  double pos, rot;
  resolve_thresholds(m, params, &pos, &rot);
  ppf_status s = enqueue_cluster(&ws, d_in.p, n, num_poses, pos, rot, params->use_weighted_avg != 0, nullptr, params->rot_metric_relative != 0);
  if (s != PPF_OK) return s;
  HIPCHK(hipStreamSynchronize(nullptr));
  uint32_t nf = 0;
  HIPCHK(hipMemcpy(&nf, ws.cl_u32.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  *n_out = (int)nf;
  if (out) {
    if (cap < (int)nf) return fail(PPF_ERR_CAPACITY, "ppf_cluster_poses: need room for %d poses", (int)nf);
    if (nf) HIPCHK(hipMemcpy(out, ws.d_final.p, (size_t)nf * sizeof(ppf_pose), hipMemcpyDeviceToHost));
  }
  return PPF_OK;
}

/* ---- host-buffer entries (what detector.match / match_S2B bind to) --------------------------------------------------
 * The reference calls match() once per detected object, again and again on the same detector
 * (/root/reference/include/CloudProcessing.h:441-446, :494-499 -- its own "PPF Elapsed Time" bracket).  A call therefore
 * borrows a WARM context from its model: a workspace that has already sized its hit pools and learned this scene
 * family's hit density (no counting pass, no scratch allocation), a non-blocking stream, pinned staging for the upload.
 * Contexts are handed out under the model's mutex, one per call in flight, so concurrent calls on one model from several
 * host threads stay independent.  A model keeps as many idle ones as it has had calls in flight at once (at least
 * HOST_CTX_KEEP, at most HOST_CTX_MAX): N threads matching on one detector all stay warm; ppf_model_trim_contexts releases
 * them (each holds the scratch of its last call: 0.45 GB for a C2-sized crop). */
constexpr size_t HOST_CTX_KEEP = 2;
constexpr size_t HOST_CTX_MAX = 16;

struct HostCtx {
  ppf_workspace ws;
  hipStream_t stream = nullptr;
  float* pinned[2] = {nullptr, nullptr}; /* scene, edge */
  size_t pinned_cap[2] = {0, 0};
  DevBuf<float> d_rows[2];
  int device = -1;
  ~HostCtx() {
    /* everything this context ever enqueued went to its own stream: wait for that, not for the whole device (other threads'
     * calls on other contexts keep running) */
    if (stream) (void)hipStreamSynchronize(stream); else sync_device(device);
    for (float* p : pinned)
      if (p) (void)hipHostFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

ppf_model::~ppf_model() {
  for (HostCtx* c : ctx_idle) delete c;
}

extern "C" ppf_status ppf_model_trim_contexts(const ppf_model* m, int keep, int* released) {
  if (!m || keep < 0) return fail(PPF_ERR_INVALID, "ppf_model_trim_contexts: bad argument");
  std::vector<HostCtx*> drop;
  {
    std::lock_guard<std::mutex> g(m->ctx_mu);
    while (m->ctx_idle.size() > (size_t)keep) { drop.push_back(m->ctx_idle.back()); m->ctx_idle.pop_back(); }
    m->ctx_peak = m->ctx_out; /* the high-water mark starts again: later calls keep what THEY need */
  }
  for (HostCtx* c : drop) delete c; /* waits for the context's stream, returns its scratch to the block cache */
  if (released) *released = (int)drop.size();
  return PPF_OK;
}

namespace {

/* RAII loan of a context: returned to the model's idle list when the call succeeded, destroyed otherwise (a failed call
 * leaves pools and flags in an unknown state; fail() has already drained the device) */
struct HostLoan {
  const ppf_model* m;
  HostCtx* c = nullptr;
  bool ok = false;
  bool counted = false;
  explicit HostLoan(const ppf_model* model) : m(model) {}
  ppf_status open() {
    {
      std::lock_guard<std::mutex> g(m->ctx_mu);
      if (!m->ctx_idle.empty()) { c = m->ctx_idle.back(); m->ctx_idle.pop_back(); }
      m->ctx_out++;
      m->ctx_peak = std::max(m->ctx_peak, m->ctx_out);
      counted = true;
    }
    if (c) return PPF_OK;
    std::unique_ptr<HostCtx> n(new (std::nothrow) HostCtx());
    if (!n) return fail(PPF_ERR_NOMEM, "match: out of memory");
    n->ws.model_owns_me = true;
    HIPCHK(hipGetDevice(&n->device));
    HIPCHK(hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking));
    c = n.release();
    return PPF_OK;
  }
  ~HostLoan() {
    {
      std::lock_guard<std::mutex> g(m->ctx_mu);
      if (counted) m->ctx_out--;
      if (c && ok && !c->ws.pools_failed && m->ctx_idle.size() < std::min(HOST_CTX_MAX, std::max(HOST_CTX_KEEP, m->ctx_peak))) {
        m->ctx_idle.push_back(c);
        c = nullptr;
      }
    }
    delete c; /* outside the lock: it waits for its stream */
  }
  /* host rows -> pinned staging -> device, all on the context's stream */
  ppf_status upload(int which, const float* rows, int n, int stride, const float** d_out) {
    const size_t floats = (size_t)n * stride;
    if (c->pinned_cap[which] < floats) {
      if (c->pinned[which]) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipHostFree(c->pinned[which])); }
      c->pinned[which] = nullptr; c->pinned_cap[which] = 0;
      const size_t want = floats + floats / 4; /* some slack: crops of one camera differ by a few percent */
      HIPCHK(hipHostMalloc((void**)&c->pinned[which], want * sizeof(float), hipHostMallocDefault));
      c->pinned_cap[which] = want;
    }
    memcpy(c->pinned[which], rows, floats * sizeof(float));
    HIPCHK(c->d_rows[which].reserve(floats));
    HIPCHK(hipMemcpyAsync(c->d_rows[which].p, c->pinned[which], floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *d_out = c->d_rows[which].p;
    return PPF_OK;
  }
};

/* upload + enqueue on a borrowed context; the caller fetches through ppf_workspace_results(&loan.c->ws, ...) */
ppf_status run_host_warm(HostLoan& loan, const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                         int estride, int enoff, const ppf_match_params* params, bool timing) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  if (!have_device()) return fail(PPF_ERR_HIP, "match: no HIP device (this engine has no CPU fallback)");
  ppf_status s = check_match_args(m, scene, ns, sstride, snoff, edge, ne, estride, enoff, params);
  if (s != PPF_OK) return s;
  if ((s = loan.open()) != PPF_OK) return s;
  if ((s = ppf_workspace_enable_timing(&loan.c->ws, timing ? 1 : 0)) != PPF_OK) return s;
  const float *d_scene = nullptr, *d_edge = nullptr;
  if ((s = loan.upload(0, scene, ns, sstride, &d_scene)) != PPF_OK) return s;
  if (edge && (s = loan.upload(1, edge, ne, estride, &d_edge)) != PPF_OK) return s;
  return ppf_match_device(m, &loan.c->ws, d_scene, ns, sstride, snoff, d_edge, ne, estride, enoff, params, loan.c->stream);
}

}  // namespace

/* cold variant on the caller's own workspace and the default stream (debug entry only) */
static ppf_status run_host(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                           int estride, int enoff, const ppf_match_params* params, ppf_workspace* ws) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  if (!have_device()) return fail(PPF_ERR_HIP, "match: no HIP device (this engine has no CPU fallback)");
  ppf_status s = check_match_args(m, scene, ns, sstride, snoff, edge, ne, estride, enoff, params);
  if (s != PPF_OK) return s;
  DevBuf<float> d_scene, d_edge;
  HIPCHK(d_scene.reserve((size_t)ns * sstride));
  HIPCHK(hipMemcpy(d_scene.p, scene, (size_t)ns * sstride * sizeof(float), hipMemcpyHostToDevice));
  if (edge) {
    HIPCHK(d_edge.reserve((size_t)ne * estride));
    HIPCHK(hipMemcpy(d_edge.p, edge, (size_t)ne * estride * sizeof(float), hipMemcpyHostToDevice));
  }
  s = ppf_match_device(m, ws, d_scene.p, ns, sstride, snoff, edge ? d_edge.p : nullptr, ne, estride, enoff, params, nullptr);
  if (s != PPF_OK) return s;
  HIPCHK(hipStreamSynchronize(nullptr));
  return PPF_OK;
}

ppf_status ppf_match(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                     int estride, int enoff, const ppf_match_params* params, ppf_pose* out, int cap, int* n_out) {
  if (!n_out) return fail(PPF_ERR_INVALID, "ppf_match: n_out is NULL");
  *n_out = 0;
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  HostLoan loan(m);
  ppf_status s = run_host_warm(loan, m, scene, ns, sstride, snoff, edge, ne, estride, enoff, params, false);
  if (s == PPF_OK) s = ppf_workspace_results(&loan.c->ws, nullptr, nullptr, 0, nullptr, out, cap, n_out, nullptr);
  loan.ok = s == PPF_OK || s == PPF_ERR_CAPACITY; /* a too small output buffer leaves the context in order */
  return s;
}

ppf_status ppf_raw_votes(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                         int estride, int enoff, const ppf_match_params* params, ppf_vote* votes, ppf_pose* raw_poses, int cap,
                         int* n_ref, ppf_match_stats* stats) {
  if (!m) return fail(PPF_ERR_NOT_TRAINED, "The model is not trained. Cannot match without training");
  HostLoan loan(m);
  ppf_status s = run_host_warm(loan, m, scene, ns, sstride, snoff, edge, ne, estride, enoff, params, true);
  if (s == PPF_OK) s = ppf_workspace_results(&loan.c->ws, votes, raw_poses, cap, n_ref, nullptr, 0, nullptr, stats);
  loan.ok = s == PPF_OK || s == PPF_ERR_CAPACITY;
  return s;
}

}  // extern "C"

#endif /* PPF_MATCH_HOST_H */
