/*
 * ppf_stage_host.h — what every stage call shares on the host: the one wait of a call (stage_finish), the body
 * of an extern "C" entry (stage_entry), and FrameRun, one call's counted launches on one stream with scratch from the block
 * cache, with the scan and the radix sort that run on it.  No kernel and no entry of its own.  Included by ppf_hip.hip after
 * ppf_icp_host.h and before ppf_prep_host.h, the first stage.
 *
 * A stage that owns a FrameRun is, in this order: its argument checks; `FrameRun fr; fr.get(...)`; a `run` that enqueues, with
 * fr.sizing where the device says how large the output is; `fr.finish(who, run(), {...})`; its results and fr.report(st).  Its
 * extern "C" entry is one stage_entry.
 */
#ifndef PPF_STAGE_HOST_H
#define PPF_STAGE_HOST_H

namespace {

inline dim3 grid_for(size_t items, int block) { return dim3((unsigned)std::max<size_t>((items + block - 1) / block, 1)); }

/* a device buffer of a call: its name in messages, its extent, and where stage_finish copies it (NULL: nowhere).  A NULL dev
 * is an optional buffer the caller left out. */
struct StageBuf {
  const char* what;
  const void* dev;
  size_t bytes;
  void* host;
};

/* The one wait of a call.  `enqueued` is what the stage's enqueue returned; when it is PPF_OK the buffers of `back` that have
 * a host address are read back behind the kernels on `st` and the host waits once, for all of it.
 *
 * The rule, for every stage: from its first enqueue on, a call returns only through here.  Its scratch (DevBuf, FrameRun)
 * goes back to the block cache when the caller's scope ends, and the next call may be handed it at once; so when the enqueue,
 * a read-back or the wait has failed, kernels of this call may still be queued on that scratch, and the call waits for the
 * whole device before it returns. */
ppf_status stage_finish(const char* who, ppf_status enqueued, hipStream_t st, std::initializer_list<StageBuf> back) {
  ppf_status s = enqueued;
  if (s == PPF_OK) {
    hipError_t e = hipSuccess;
    for (const StageBuf& b : back)
      if (e == hipSuccess && b.host) e = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = host_stream_sync(st);
    if (e != hipSuccess) s = fail(PPF_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (s != PPF_OK) (void)hipDeviceSynchronize();
  return s;
}

template <class Stats>
void stage_clear_stats(Stats& st, bool) {
  std::memset(&st, 0, sizeof(st));
}

/* ms_wall of the stats that have one */
template <class Stats>
auto stage_wall(Stats& st, float ms, int) -> decltype((void)st.ms_wall) { st.ms_wall = ms; }
template <class Stats>
void stage_wall(Stats&, float, long) {}

/* The body of an extern "C" entry: the caller's stats or a local, cleared; the call; cleared again when it failed, ms_wall
 * when it did not.  clear(st, failed) is the stage's: it zeroes the stats and whatever else a failed call must leave zero. */
template <class Stats, class Clear, class Call>
ppf_status stage_entry(Stats* stats, Clear clear, Call call) {
  const auto t0 = std::chrono::steady_clock::now();
  Stats local;
  Stats& st = stats ? *stats : local;
  clear(st, false);
  const ppf_status s = call(st);
  if (s != PPF_OK) {
    clear(st, true);
    return s;
  }
  stage_wall(st, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(), 0);
  return PPF_OK;
}

/* one call's launches, counted, on one stream (the null stream unless the entry has a stream argument), and its scratch,
 * from the block cache; it lives until the call returns (after the last read-back) */
struct FrameRun {
  hipStream_t st = nullptr;
  int launches = 0, syncs = 0;
  struct Holder {
    virtual ~Holder() {}
  };
  template <class T>
  struct Buf : Holder {
    DevBuf<T> b;
  };
  std::vector<std::unique_ptr<Holder>> keep;
  template <class T>
  ppf_status get(size_t n, T** out) {
    std::unique_ptr<Buf<T>> h(new Buf<T>());
    HIPCHK(h->b.reserve(std::max<size_t>(n, 1)));
    *out = h->b.p;
    keep.push_back(std::move(h));
    return PPF_OK;
  }
  /* get(n1, &p1, n2, &p2, ...): every buffer in turn, the first failure */
  template <class T, class... More>
  ppf_status get(size_t n, T** out, More... more) {
    const ppf_status s = get(n, out);
    return s != PPF_OK ? s : get(more...);
  }
  /* a blocking read-back (counted), on the null stream: the stages that run on a caller's stream never call it */
  ppf_status read(void* dst, const void* src, size_t bytes) {
    syncs++;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PPF_OK;
  }
  /* the counted wait in the middle of a call, for what sizes its output: the read-backs behind the kernels on st, one wait */
  ppf_status sizing(std::initializer_list<StageBuf> back) {
    for (const StageBuf& b : back)
      if (b.host) HIPCHK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(host_stream_sync(st));
    syncs++;
    return PPF_OK;
  }
  /* the one end of a call (stage_finish on st): counted when it succeeded, the device drained when it did not.  A single
   * read-back on the null stream is the blocking copy the pose-table stages always ended in, which is the wait: sent through
   * stage_finish it cost them 0.02 ms a call (profiles/r35_stage_host_refactor.json, rejected_variant) */
  ppf_status finish(const char* who, ppf_status enqueued, std::initializer_list<StageBuf> back) {
    const StageBuf* one = nullptr;
    int n = 0;
    for (const StageBuf& b : back)
      if (b.host) { one = &b; n++; }
    if (enqueued == PPF_OK && !st && n == 1) {
      const hipError_t e = hipMemcpy(one->host, one->dev, one->bytes, hipMemcpyDeviceToHost);
      if (e == hipSuccess) { syncs++; return PPF_OK; }
      return stage_finish(who, fail(PPF_ERR_HIP, "%s: %s", who, hipGetErrorString(e)), st, {});
    }
    const ppf_status s = stage_finish(who, enqueued, st, back);
    if (s == PPF_OK) syncs++;
    return s;
  }
  template <class Stats>
  void report(Stats& stats) const {
    stats.n_launches = launches;
    stats.n_host_syncs = syncs;
  }
};

#define FRAME_LAUNCH(fr, kern, grid, block, ...)        \
  do {                                                  \
    kern<<<(grid), (block), 0, (fr).st>>>(__VA_ARGS__); \
    (fr).launches++;                                    \
  } while (0)

/* exclusive scan of n u32 in five launches whatever n is (device_exclusive_scan picks its launches by n and waits for
 * its scratch; here the scratch lives in `fr`) */
ppf_status frame_scan(FrameRun& fr, const uint32_t* in, uint32_t* out, size_t n) {
  const size_t nb1 = std::max<size_t>((n + 1023) / 1024, 1), nb2 = (nb1 + 1023) / 1024;
  uint32_t *s1, *s1x, *s2, *s2x;
  const ppf_status s = fr.get(nb1, &s1, nb1, &s1x, nb2, &s2, nb2, &s2x);
  if (s != PPF_OK) return s;
  FRAME_LAUNCH(fr, k_scan_block, dim3((unsigned)nb1), dim3(256), in, out, s1, n);
  FRAME_LAUNCH(fr, k_scan_block, dim3((unsigned)nb2), dim3(256), s1, s1x, s2, nb1);
  FRAME_LAUNCH(fr, k_scan_one, dim3(1), dim3(1024), s2, s2x, nb2);
  FRAME_LAUNCH(fr, k_scan_add, grid_for(nb1, 256), dim3(256), s1x, s2x, nb1);
  FRAME_LAUNCH(fr, k_scan_add, grid_for(n, 256), dim3(256), out, s1x, n);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* the frame-level radix sort: stable LSD passes over the digits at `shifts` of keys ka (values va), seven launches a pass
 * whatever n is (hist and offs: 256 words per RS_BLOCK rows each); the sorted arrays end in ka / va */
ppf_status frame_sort(FrameRun& fr, uint32_t*& ka, uint32_t*& va, uint32_t*& kb, uint32_t*& vb, int n, uint32_t* hist, uint32_t* offs,
                      const int* shifts, int passes) {
  const int nblk = (n + RS_BLOCK - 1) / RS_BLOCK;
  ppf_status s;
  for (int pass = 0; pass < passes; pass++) {
    FRAME_LAUNCH(fr, k_rs_hist, dim3(nblk), dim3(RS_BLOCK), ka, n, shifts[pass], nblk, hist);
    HIPCHK(hipGetLastError());
    if ((s = frame_scan(fr, hist, offs, (size_t)256 * nblk)) != PPF_OK) return s;
    FRAME_LAUNCH(fr, k_rs_scatter, dim3(nblk), dim3(RS_BLOCK), ka, va, n, shifts[pass], nblk, offs, kb, vb);
    HIPCHK(hipGetLastError());
    std::swap(ka, kb);
    std::swap(va, vb);
  }
  return PPF_OK;
}

}  // namespace

#endif /* PPF_STAGE_HOST_H */
