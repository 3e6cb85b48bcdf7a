/*
 * ppf_recognize_host.h — host side of ppf_recognizer_* and ppf_recognize_frame: per proposal cloud a shortlist of the trained
 * models it can be a view of.  Kernels: ppf_recognize_kernels.h.  Included by ppf_hip.hip after ppf_stage_host.h
 * (FrameRun, FRAME_LAUNCH, stage_entry), ppf_prep_host.h (ppf_cloud) and ppf_model_host.h.
 *
 * Create, per model: k_rec_dmax, one read-back (the bitmap's size), k_rec_build, k_rec_popcount, one read-back (the bitmap and
 * n_keys).  A frame call: one work list built from the row counts (a cloud handle knows its size), one upload, one memset of the
 * counters and hit bitmaps, k_rec_score and k_rec_finish, one wait; the scores and the ranking are host arithmetic on the
 * integers that come back.
 */
#ifndef PPF_RECOGNIZE_HOST_H
#define PPF_RECOGNIZE_HOST_H

struct ppf_recognizer {
  std::atomic<int> refcount{1};
  int device = 0;
  struct Set {
    DevBuf<uint32_t> bits;
    std::vector<uint32_t> host; /* the same words: ppf_recognizer_keys needs no device */
    uint32_t words = 0;
    int n_a = 0, n_d = 0, lds = 0;
    uint64_t n_keys = 0;
  };
  std::vector<ppf_model*> models; /* retained */
  std::vector<std::unique_ptr<Set>> sets;
  DevBuf<RecModel> d_models;
  uint32_t lds_words = 0; /* the largest set that is staged in LDS */
  ~ppf_recognizer() {
    for (ppf_model* m : models) (void)ppf_model_release(m);
  }
};

namespace {

constexpr size_t REC_HIT_BYTES_MAX = (size_t)2 << 30; /* hit bitmaps of one call */
constexpr uint64_t REC_SET_BITS_MAX = (uint64_t)1 << 30;

ppf_status recognizer_build_set(const ppf_model* m, ppf_recognizer::Set& s) {
  const double angle_step = m->info.angle_step, dist_step = m->info.distance_step;
  const CloudSoA c = m->cloud.view();
  DevBuf<uint32_t> word;
  HIPCHK(word.reserve(2));
  HIPCHK(hipMemsetAsync(word.p, 0, 2 * sizeof(uint32_t), nullptr));
  k_rec_dmax<<<dim3((unsigned)c.n), dim3(REC_BLOCK), 0, nullptr>>>(c, dist_step, word.p);
  HIPCHK(hipGetLastError());
  uint32_t dmax = 0;
  HIPCHK(hipMemcpy(&dmax, word.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  s.n_a = (int)std::floor(PPF_PI / angle_step) + 2;
  s.n_d = (int)dmax + 1;
  const uint64_t n_bits = (uint64_t)s.n_a * s.n_a * s.n_a * (uint64_t)s.n_d;
  if (s.n_a < 2 || n_bits > REC_SET_BITS_MAX)
    return fail(PPF_ERR_INVALID, "ppf_recognizer_create: a key set of %d^3 x %d bins is too large (at most 2^30)", s.n_a, s.n_d);
  s.words = (uint32_t)((n_bits + 31) / 32);
  s.lds = (size_t)s.words * 4 <= REC_LDS_SET_BYTES ? 1 : 0;
  HIPCHK(s.bits.reserve(s.words));
  HIPCHK(hipMemsetAsync(s.bits.p, 0, (size_t)s.words * sizeof(uint32_t), nullptr));
  k_rec_build<<<dim3((unsigned)c.n), dim3(REC_BLOCK), 0, nullptr>>>(c, angle_step, dist_step, s.n_a, s.n_d, s.bits.p);
  k_rec_popcount<<<dim3(std::min<unsigned>((s.words + REC_BLOCK - 1) / REC_BLOCK, 256u)), dim3(REC_BLOCK), 0, nullptr>>>(s.bits.p, s.words, word.p + 1);
  HIPCHK(hipGetLastError());
  s.host.resize(s.words);
  uint32_t n_keys = 0;
  HIPCHK(hipMemcpy(s.host.data(), s.bits.p, (size_t)s.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&n_keys, word.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
  s.n_keys = n_keys;
  return PPF_OK;
}

ppf_status recognizer_create(const ppf_model* const* models, int n_models, ppf_recognizer** out) {
  if (!models) return fail(PPF_ERR_INVALID, "ppf_recognizer_create: models is NULL");
  if (n_models < 1 || n_models > PPF_RECOGNIZE_MAX_MODELS)
    return fail(PPF_ERR_INVALID, "ppf_recognizer_create: n_models is %d (1..%d)", n_models, PPF_RECOGNIZE_MAX_MODELS);
  for (int i = 0; i < n_models; i++)
    if (!models[i]) return fail(PPF_ERR_INVALID, "ppf_recognizer_create: model %d is NULL", i);
  /* a model only exists where there is a device: without one nothing below has a handle to look into */
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_recognizer_create: no HIP device (this engine has no CPU fallback)");
  for (int i = 0; i < n_models; i++) {
    if (models[i]->params.feature != PPF_FEATURE_PPF)
      return fail(PPF_ERR_INVALID, "ppf_recognizer_create: model %d was trained with PPF_FEATURE_DARBOUX; only PPF_FEATURE_PPF models have key sets", i);
    if (models[i]->info.n_ref < 2) return fail(PPF_ERR_INVALID, "ppf_recognizer_create: model %d has %d sampled rows (at least 2)", i, models[i]->info.n_ref);
  }
  std::unique_ptr<ppf_recognizer> rec(new ppf_recognizer());
  HIPCHK(hipGetDevice(&rec->device));
  for (int i = 0; i < n_models; i++)
    if (models[i]->device != rec->device)
      return fail(PPF_ERR_INVALID, "ppf_recognizer_create: model %d lives on device %d, the current device is %d", i, models[i]->device, rec->device);
  std::vector<RecModel> table((size_t)n_models);
  for (int i = 0; i < n_models; i++) {
    ppf_model* m = const_cast<ppf_model*>(models[i]);
    (void)ppf_model_retain(m);
    rec->models.push_back(m);
    rec->sets.emplace_back(new ppf_recognizer::Set());
    ppf_recognizer::Set& s = *rec->sets.back();
    const ppf_status st = recognizer_build_set(m, s);
    /* kernels of the failed build may still run on blocks that now return to the cache: stage_finish drains the device */
    if (st != PPF_OK) return stage_finish("ppf_recognizer_create", st, nullptr, {});
    RecModel& t = table[(size_t)i];
    t.bits = s.bits.p; t.words = s.words; t.n_a = s.n_a; t.n_d = s.n_d; t.lds = s.lds; t.pad = 0;
    t.angle_step = m->info.angle_step; t.dist_step = m->info.distance_step;
    if (s.lds) rec->lds_words = std::max(rec->lds_words, s.words);
  }
  HIPCHK(rec->d_models.reserve((size_t)n_models));
  HIPCHK(hipMemcpy(rec->d_models.p, table.data(), table.size() * sizeof(RecModel), hipMemcpyHostToDevice));
  *out = rec.release();
  return PPF_OK;
}

/* the outputs of a failed call are zero, where the arguments say how long they are */
void recognize_clear(const ppf_recognizer* rec, int n_clouds, const ppf_recognize_params* p, int32_t* n_used, uint64_t* counts,
                     ppf_recognize_score* ranked, int32_t* n_ranked, ppf_recognize_stats& st) {
  std::memset(&st, 0, sizeof(st));
  if (n_clouds < 1 || n_clouds > PPF_RECOGNIZE_MAX_CLOUDS) return;
  if (n_used) std::memset(n_used, 0, (size_t)n_clouds * sizeof(int32_t));
  if (n_ranked) std::memset(n_ranked, 0, (size_t)n_clouds * sizeof(int32_t));
  if (counts && rec) std::memset(counts, 0, (size_t)n_clouds * rec->models.size() * 2 * sizeof(uint64_t));
  if (ranked && p && p->top >= 1 && p->top <= PPF_RECOGNIZE_MAX_TOP) std::memset(ranked, 0, (size_t)n_clouds * p->top * sizeof(ppf_recognize_score));
}

ppf_status recognize_frame(const ppf_recognizer* rec, const ppf_cloud* const* clouds, int n_clouds, const ppf_recognize_params* p,
                           int32_t* n_used, uint64_t* counts, ppf_recognize_score* ranked, int32_t* n_ranked, ppf_recognize_stats& st) {
  const char* who = "ppf_recognize_frame";
  if (!rec) return fail(PPF_ERR_INVALID, "%s: the recogniser is NULL", who);
  if (!p) return fail(PPF_ERR_INVALID, "%s: the params are NULL", who);
  if (n_clouds < 0 || n_clouds > PPF_RECOGNIZE_MAX_CLOUDS) return fail(PPF_ERR_INVALID, "%s: n_clouds is %d (0..%d)", who, n_clouds, PPF_RECOGNIZE_MAX_CLOUDS);
  if (!ranked || !n_ranked) return fail(PPF_ERR_INVALID, "%s: ranked and n_ranked must not be NULL", who);
  if (n_clouds > 0 && !clouds) return fail(PPF_ERR_INVALID, "%s: clouds is NULL", who);
  if (p->max_rows < 2 || p->max_rows > PPF_RECOGNIZE_MAX_ROWS) return fail(PPF_ERR_INVALID, "%s: max_rows is %d (2..%d)", who, p->max_rows, PPF_RECOGNIZE_MAX_ROWS);
  if (p->top < 1 || p->top > PPF_RECOGNIZE_MAX_TOP) return fail(PPF_ERR_INVALID, "%s: top is %d (1..%d)", who, p->top, PPF_RECOGNIZE_MAX_TOP);
  if (!(std::isfinite(p->min_score) && p->min_score >= 0.0) || !(std::isfinite(p->min_precision) && p->min_precision >= 0.0))
    return fail(PPF_ERR_INVALID, "%s: min_score and min_precision must be finite and >= 0", who);
  if (p->flags != 0) return fail(PPF_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
  if (!have_device()) return fail(PPF_ERR_HIP, "%s: no HIP device (this engine has no CPU fallback)", who);

  const int M = (int)rec->models.size();
  const size_t n_pairs = (size_t)n_clouds * M;
  /* the work list: per proposal with a candidate row, per model, one item per REC_SLICE reference candidates */
  std::vector<RecCloud> h_clouds((size_t)std::max(n_clouds, 1));
  std::vector<unsigned long long> h_off(std::max<size_t>(n_pairs, 1), REC_NO_HITS);
  std::vector<RecItem> h_items;
  int row_cap = REC_SLICE;
  size_t hit_words = 0;
  for (int c = 0; c < n_clouds; c++) {
    RecCloud& rc = h_clouds[(size_t)c];
    rc = RecCloud{nullptr, 0, 1, 0, 0};
    const ppf_cloud* cl = clouds[c];
    if (!cl || cl->n <= 0) continue;
    rc.rows = cl->rows.p;
    rc.n = cl->n;
    rc.step = (int)(((long long)cl->n + p->max_rows - 1) / p->max_rows);
    rc.cand = (int)(((long long)cl->n + rc.step - 1) / rc.step);
    row_cap = std::max(row_cap, (rc.cand + REC_SLICE - 1) / REC_SLICE * REC_SLICE);
    for (int m = 0; m < M; m++) {
      const size_t pair = (size_t)c * M + m;
      h_off[pair] = hit_words;
      hit_words += rec->sets[(size_t)m]->words;
      for (int b = 0; b < rc.cand; b += REC_SLICE) h_items.push_back(RecItem{(uint32_t)c, (uint32_t)m, (uint32_t)b, (uint32_t)pair});
    }
  }
  if (hit_words * sizeof(uint32_t) > REC_HIT_BYTES_MAX)
    return fail(PPF_ERR_NOMEM, "%s: the hit bitmaps of this call take %zu bytes (at most %zu): pass fewer clouds per call", who,
                hit_words * sizeof(uint32_t), REC_HIT_BYTES_MAX);
  const size_t lds_bytes = ((size_t)6 * row_cap + (size_t)2 * rec->lds_words) * sizeof(uint32_t);
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rec_score), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(((size_t)6 * REC_MAX_ROWS) * sizeof(uint32_t) + 2 * REC_LDS_SET_BYTES));
  });
  HIPCHK(attr);

  /* one upload: [clouds | hit offsets | items], and one zeroed block: [counts (2 u64 a pair) | n_used | hit bitmaps] */
  const size_t b_clouds = h_clouds.size() * sizeof(RecCloud), b_off = h_off.size() * sizeof(unsigned long long),
               b_items = std::max<size_t>(h_items.size(), 1) * sizeof(RecItem);
  std::vector<unsigned char> blob(b_clouds + b_off + b_items, 0);
  std::memcpy(blob.data(), h_clouds.data(), b_clouds);
  std::memcpy(blob.data() + b_clouds, h_off.data(), b_off);
  if (!h_items.empty()) std::memcpy(blob.data() + b_clouds + b_off, h_items.data(), h_items.size() * sizeof(RecItem));
  const size_t z_counts = std::max<size_t>(n_pairs, 1) * 2 * sizeof(unsigned long long), z_used = (size_t)std::max(n_clouds, 1) * sizeof(int32_t);
  const size_t z_head = (z_counts + z_used + 7) / 8 * 8, z_bytes = z_head + std::max<size_t>(hit_words, 1) * sizeof(uint32_t);
  FrameRun fr;
  unsigned char *d_blob, *d_zero;
  ppf_status s = fr.get(blob.size(), &d_blob, z_bytes, &d_zero);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  const RecCloud* d_clouds = reinterpret_cast<const RecCloud*>(d_blob);
  const unsigned long long* d_off = reinterpret_cast<const unsigned long long*>(d_blob + b_clouds);
  const RecItem* d_items = reinterpret_cast<const RecItem*>(d_blob + b_clouds + b_off);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(d_zero);
  int32_t* d_used = reinterpret_cast<int32_t*>(d_zero + z_counts);
  uint32_t* d_hits = reinterpret_cast<uint32_t*>(d_zero + z_head);
  const int n_items = (int)h_items.size();
  auto run = [&]() -> ppf_status {
    HIPCHK(hipMemsetAsync(d_zero, 0, z_bytes, fr.st));
    /* dynamic LDS, which FRAME_LAUNCH does not pass: counted by hand */
    k_rec_score<<<dim3((unsigned)std::max(n_items, 1)), dim3(REC_BLOCK), lds_bytes, fr.st>>>(d_items, n_items, d_clouds, rec->d_models.p, row_cap,
                                                                                            rec->lds_words, d_hits, d_off, d_counts, d_used);
    fr.launches++;
    FRAME_LAUNCH(fr, k_rec_finish, dim3((unsigned)std::max<size_t>(n_pairs, 1)), dim3(REC_BLOCK), (int)n_pairs, M, rec->d_models.p, d_hits, d_off, d_counts);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PPF_OK : fail(PPF_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  };
  const ppf_status ran = run();
  std::vector<unsigned char> back(z_head); /* filled while the kernels run */
  if ((s = fr.finish(who, ran, {{"counters", d_zero, z_head, back.data()}})) != PPF_OK) return s;
  const unsigned long long* r_counts = reinterpret_cast<const unsigned long long*>(back.data());
  const int32_t* r_used = reinterpret_cast<const int32_t*>(back.data() + z_counts);
  std::vector<ppf_recognize_score> all((size_t)M);
  for (int c = 0; c < n_clouds; c++) {
    const int32_t used = r_used[c];
    if (n_used) n_used[c] = used;
    const uint64_t pairs = (uint64_t)used * (uint64_t)(used > 0 ? used - 1 : 0);
    int n_pass = 0;
    for (int m = 0; m < M; m++) {
      const uint64_t known = r_counts[((size_t)c * M + m) * 2], hit = r_counts[((size_t)c * M + m) * 2 + 1];
      if (counts) {
        counts[((size_t)c * M + m) * 2] = known;
        counts[((size_t)c * M + m) * 2 + 1] = hit;
      }
      ppf_recognize_score sc;
      std::memset(&sc, 0, sizeof(sc));
      sc.model = m;
      sc.n_known = known;
      sc.n_keys_hit = hit;
      if (pairs > 0) {
        sc.precision = (double)known / (double)pairs;
        sc.recall = (double)hit / (double)rec->sets[(size_t)m]->n_keys;
        sc.score = sc.precision * sc.recall;
      }
      if (sc.score >= p->min_score && sc.precision >= p->min_precision) all[(size_t)n_pass++] = sc;
    }
    if (!clouds[c] || clouds[c]->n <= 0) n_pass = 0; /* no cloud, or one without rows, is nobody's view */
    std::stable_sort(all.begin(), all.begin() + n_pass, [](const ppf_recognize_score& a, const ppf_recognize_score& b) { return a.score > b.score; });
    const int k = std::min(n_pass, (int)p->top);
    n_ranked[c] = k;
    for (int r = 0; r < k; r++) ranked[(size_t)c * p->top + r] = all[(size_t)r];
  }
  st.n_clouds = n_clouds;
  st.n_models = M;
  fr.report(st);
  return PPF_OK;
}

}  // namespace

extern "C" {

void ppf_default_recognize_params(ppf_recognize_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_rows = 512;
  p->top = 2;
  p->min_score = 0.0;
  p->min_precision = 0.0;
  p->flags = 0;
}

ppf_status ppf_recognizer_create(const ppf_model* const* models, int n_models, ppf_recognizer** out) {
  if (!out) return fail(PPF_ERR_INVALID, "ppf_recognizer_create: out is NULL");
  *out = nullptr;
  return recognizer_create(models, n_models, out);
}

ppf_status ppf_recognizer_retain(ppf_recognizer* rec) {
  if (!rec) return fail(PPF_ERR_INVALID, "ppf_recognizer_retain: NULL");
  rec->refcount.fetch_add(1);
  return PPF_OK;
}

ppf_status ppf_recognizer_release(ppf_recognizer* rec) {
  if (!rec) return PPF_OK;
  if (rec->refcount.fetch_sub(1) == 1) {
    sync_device(rec->device); /* the key sets return to the block cache: no call may still be reading them */
    delete rec;
  }
  return PPF_OK;
}

ppf_status ppf_recognizer_model_info(const ppf_recognizer* rec, int i, ppf_recognizer_info* info) {
  if (!rec || !info) return fail(PPF_ERR_INVALID, "ppf_recognizer_model_info: NULL");
  std::memset(info, 0, sizeof(*info));
  if (i < 0 || i >= (int)rec->models.size()) return fail(PPF_ERR_INVALID, "ppf_recognizer_model_info: model %d of %d", i, (int)rec->models.size());
  const ppf_recognizer::Set& s = *rec->sets[(size_t)i];
  info->n_rows = rec->models[(size_t)i]->info.n_ref;
  info->n_bins[0] = info->n_bins[1] = info->n_bins[2] = s.n_a;
  info->n_bins[3] = s.n_d;
  info->in_lds = s.lds;
  info->n_keys = s.n_keys;
  info->bytes = s.bits.bytes();
  return PPF_OK;
}

ppf_status ppf_recognizer_keys(const ppf_recognizer* rec, int i, int32_t* keys4, int cap, int* n) {
  if (!rec || !n) return fail(PPF_ERR_INVALID, "ppf_recognizer_keys: NULL");
  *n = 0;
  if (i < 0 || i >= (int)rec->models.size()) return fail(PPF_ERR_INVALID, "ppf_recognizer_keys: model %d of %d", i, (int)rec->models.size());
  const ppf_recognizer::Set& s = *rec->sets[(size_t)i];
  *n = (int)s.n_keys;
  if (!keys4 || cap < (int)s.n_keys) return fail(PPF_ERR_CAPACITY, "ppf_recognizer_keys: need room for %d keys", (int)s.n_keys);
  /* Bit order is tuple order but for the NaN bin, which sits last in its dimension and is INT32_MIN: walking every angle
   * dimension from its last bin round to the others gives the lexicographic order without a sort. */
  const int A = s.n_a, D = s.n_d;
  int32_t* o = keys4;
  for (int a0 = 0; a0 < A; a0++)
    for (int a1 = 0; a1 < A; a1++)
      for (int a2 = 0; a2 < A; a2++) {
        const int k0 = (a0 + A - 1) % A, k1 = (a1 + A - 1) % A, k2 = (a2 + A - 1) % A;
        const uint32_t base = (((uint32_t)k0 * (uint32_t)A + (uint32_t)k1) * (uint32_t)A + (uint32_t)k2) * (uint32_t)D;
        for (int k3 = 0; k3 < D; k3++) {
          const uint32_t bit = base + (uint32_t)k3;
          if (!(s.host[bit >> 5] >> (bit & 31u) & 1u)) continue;
          o[0] = k0 == A - 1 ? INT32_MIN : k0;
          o[1] = k1 == A - 1 ? INT32_MIN : k1;
          o[2] = k2 == A - 1 ? INT32_MIN : k2;
          o[3] = k3;
          o += 4;
        }
      }
  return PPF_OK;
}

ppf_status ppf_recognize_frame(const ppf_recognizer* rec, const ppf_cloud* const* clouds, int n_clouds, const ppf_recognize_params* p,
                               int32_t* n_used, uint64_t* counts, ppf_recognize_score* ranked, int32_t* n_ranked, ppf_recognize_stats* stats) {
  return stage_entry(stats, [&](ppf_recognize_stats& st, bool) { recognize_clear(rec, n_clouds, p, n_used, counts, ranked, n_ranked, st); },
                     [&](ppf_recognize_stats& st) { return recognize_frame(rec, clouds, n_clouds, p, n_used, counts, ranked, n_ranked, st); });
}

}  // extern "C"

#endif /* PPF_RECOGNIZE_HOST_H */
