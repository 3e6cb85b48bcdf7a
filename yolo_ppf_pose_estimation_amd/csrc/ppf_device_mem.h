/*
 * ppf_device_mem.h — errors (fail / HIPCHK), the process-wide device block cache (DevPool) and the buffers drawn from it (DevBuf).
 * Part of the one translation unit ppf_hip.hip.
 */
#ifndef PPF_DEVICE_MEM_H
#define PPF_DEVICE_MEM_H

/* ============================================================================================ */
/* errors                                                                                         */
/* ============================================================================================ */
namespace {

thread_local std::string g_last_error;

ppf_status fail(ppf_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  /* error paths return while kernels of the failed call may still run; their scratch goes back to the block cache
   * (DevPool) as the locals unwind, so drain the device first.  Errors are rare: the cost does not matter. */
  if (st == PPF_ERR_HIP || st == PPF_ERR_NOMEM || st == PPF_ERR_CAPACITY) (void)hipDeviceSynchronize();
  return st;
}

/* blocking waits of the calling thread on the match path (ppf_match_frame reports the ones its call made) */
thread_local int g_host_syncs = 0;
inline hipError_t host_stream_sync(hipStream_t st) {
  g_host_syncs++;
  return hipStreamSynchronize(st);
}
inline hipError_t host_read(void* dst, const void* src, size_t bytes) {
  g_host_syncs++;
  return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}

#define HIPCHK(expr)                                                                                       \
  do {                                                                                                     \
    hipError_t e__ = (expr);                                                                               \
    if (e__ != hipSuccess)                                                                                 \
      return fail(PPF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

/* Device memory for scratch and results comes from a process-wide cache of freed blocks (power-of-two size classes
 * per device): hipMalloc costs tens of microseconds and hipFree synchronises the whole device, which is most of the
 * time of the small stages (cloud stages, ICP set-up).  A block is only released by a DevBuf whose last user has been
 * synchronised with (every entry point waits for its kernels before its scratch goes out of scope), so a reused block
 * is never still in flight.  PPF_NO_POOL=1 turns the cache off; PPF_POOL_GUARD=1|2 turns its guard mode on (below). */
class DevPool {
 public:
  static DevPool& get() {
    static DevPool* p = new DevPool(); /* never destroyed: no hipFree after the runtime is gone */
    return *p;
  }
  /* size classes: 8 per octave (1, 1.125, ... 1.875 x 2^k), so a block wastes at most 12.5 % of what was asked for */
  static size_t class_size(int cls) { return ((size_t)8 + (size_t)(cls & 7)) << (cls >> 3); }
  static int class_of(size_t bytes) {
    int cls = 5 * 8; /* 256 B */
    while (class_size(cls) < bytes) cls++;
    return cls;
  }
  hipError_t acquire(size_t bytes, void** out, size_t* granted, int* device) {
    *out = nullptr;
    const size_t want = std::max<size_t>(bytes, 256);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    *device = dev; /* a block goes back to the list of the device it was allocated on, whatever is current then */
    if (const int mode = guard_.load(std::memory_order_relaxed)) return acquire_guarded(bytes, mode, dev, out, granted);
    if (off_) { *granted = want; return hipMalloc(out, want); }
    const int cls = class_of(want);
    if ((*out = take(dev, cls)) != nullptr) { *granted = class_size(cls); return hipSuccess; }
    *granted = class_size(cls);
    return alloc(out, *granted);
  }
  void release(void* p, size_t granted, int dev) {
    if (!p) return;
    if (guard_seen_.load(std::memory_order_relaxed) && release_guarded(p, dev)) return;
    if (off_) { (void)hipFree(p); return; }
    const int cls = class_of(granted);
    std::lock_guard<std::mutex> g(mu_);
    free_[key(dev, cls)].push_back(p);
  }
  void trim() {
    std::lock_guard<std::mutex> g(mu_);
    for (auto& kv : free_) {
      for (void* p : kv.second) (void)hipFree(p);
      kv.second.clear();
    }
  }

  /* ---- guard mode (ppf_debug_pool_guard, PPF_POOL_GUARD): a test surface, off by default -------------------------
   * A guarded block is acquired for requested + 256 + 4,096 bytes, rounded up to its size class:
   *   [base, base + 256)                    front zone, 0xA5
   *   [base + 256, base + 256 + requested)  what the caller gets, filled with the mode's word (1: 0, 2: 1)
   *   [base + 256 + requested, end)         back zone (>= 4 KiB: the block's whole slack), 0xA5 in its first 4 KiB
   * so a store a few bytes past what a reserve() asked for, which the size classes' slack hides, damages a zone, and
   * a read of scratch that was never written sees the fill word, not the previous call's bytes.  The zones are read
   * back when the block is released (its users have been waited for: the cache's rule) and by check().  The fills and
   * read-backs are plain HIP calls of the cache's own: no stage counts them among its launches or host waits. */
  static constexpr size_t GUARD_ZONE = 256, GUARD_CHECKED = 4096;
  void set_guard(int mode) {
    trim(); /* the free lists never hold blocks of two modes */
    if (mode) guard_seen_.store(true, std::memory_order_relaxed);
    guard_.store(mode, std::memory_order_relaxed);
  }
  /* waits for the device, checks every live guarded block, adds what releases found since the last check */
  hipError_t check(ppf_debug_pool_report* r) {
    memset(r, 0, sizeof(*r));
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu_);
    r->n_blocks_live = live_.size();
    r->n_blocks_checked = n_release_checked_;
    std::vector<ppf_debug_pool_violation> found;
    found.swap(violations_);
    n_release_checked_ = 0;
    for (const auto& kv : live_) {
      ppf_debug_pool_violation v;
      bool damaged = false;
      if ((e = read_zones(kv.second, &v, &damaged)) != hipSuccess) return e;
      r->n_blocks_checked++;
      if (damaged) { found.push_back(v); report(v, "live"); }
    }
    r->n_violations = found.size();
    for (size_t i = 0; i < found.size() && i < 8; i++) r->first[i] = found[i];
    return hipSuccess;
  }

 private:
  struct GuardBlock { char* base; size_t requested, granted; };
  DevPool() : off_(getenv("PPF_NO_POOL") != nullptr) {
    const char* g = getenv("PPF_POOL_GUARD");
    const int mode = g && (!strcmp(g, "1") || !strcmp(g, "2")) ? g[0] - '0' : 0;
    guard_.store(mode, std::memory_order_relaxed);
    guard_seen_.store(mode != 0, std::memory_order_relaxed);
    guard_env_ = mode != 0;
  }
  static int key(int dev, int cls) { return dev * 1024 + cls; }
  void* take(int dev, int cls) {
    std::lock_guard<std::mutex> g(mu_);
    auto& lst = free_[key(dev, cls)];
    if (lst.empty()) return nullptr;
    void* p = lst.back();
    lst.pop_back();
    return p;
  }
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) { /* out of memory: drop the cache and retry once */
      trim();
      e = hipMalloc(out, bytes);
    }
    return e;
  }
  hipError_t acquire_guarded(size_t requested, int mode, int dev, void** out, size_t* granted) {
    const size_t total = requested + GUARD_ZONE + GUARD_CHECKED;
    const int cls = class_of(total);
    const size_t blk = off_ ? total : class_size(cls);
    void* b = off_ ? nullptr : take(dev, cls);
    hipError_t e = b ? hipSuccess : alloc(&b, blk);
    if (e != hipSuccess) return e;
    char* base = static_cast<char*>(b);
    char* p = base + GUARD_ZONE;
    const size_t back = blk - GUARD_ZONE - requested;
    /* the word fill may run up to 3 bytes into the back zone, which is filled after it */
    e = mode == 2 ? hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), 1, (requested + 3) / 4) : hipMemset(p, 0, requested);
    if (e == hipSuccess) e = hipMemset(base, 0xA5, GUARD_ZONE);
    if (e == hipSuccess) e = hipMemset(p + requested, 0xA5, std::min(back, GUARD_CHECKED));
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* whatever stream the caller uses next sees the fills */
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    std::lock_guard<std::mutex> g(mu_);
    live_[p] = GuardBlock{base, requested, blk};
    *out = p;
    *granted = blk;
    return hipSuccess;
  }
  /* false: p is no guarded block (it was acquired before the guard was switched on) */
  bool release_guarded(void* p, int dev) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = live_.find(p);
    if (it == live_.end()) return false;
    const GuardBlock b = it->second;
    live_.erase(it);
    ppf_debug_pool_violation v;
    bool damaged = false;
    if (read_zones(b, &v, &damaged) == hipSuccess) {
      n_release_checked_++;
      if (damaged) { violations_.push_back(v); report(v, "released"); }
    }
    if (off_) (void)hipFree(b.base);
    else free_[key(dev, class_of(b.granted))].push_back(b.base);
    return true;
  }
  hipError_t read_zones(const GuardBlock& b, ppf_debug_pool_violation* v, bool* damaged) const {
    const size_t back = std::min(b.granted - GUARD_ZONE - b.requested, GUARD_CHECKED);
    unsigned char host[GUARD_ZONE + GUARD_CHECKED];
    hipError_t e = hipMemcpy(host, b.base, GUARD_ZONE, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(host + GUARD_ZONE, b.base + GUARD_ZONE + b.requested, back, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    v->requested_bytes = b.requested;
    v->first_offset = 0;
    v->n_bytes_damaged = 0;
    for (size_t i = 0; i < GUARD_ZONE + back; i++)
      if (host[i] != 0xA5) {
        if (!v->n_bytes_damaged++) v->first_offset = i < GUARD_ZONE ? (int64_t)i - (int64_t)GUARD_ZONE : (int64_t)(b.requested + i - GUARD_ZONE);
      }
    *damaged = v->n_bytes_damaged != 0;
    return hipSuccess;
  }
  void report(const ppf_debug_pool_violation& v, const char* when) const {
    if (guard_env_)
      fprintf(stderr, "ppf pool guard: %s block of %llu bytes: %llu bytes damaged, the first at offset %lld\n", when,
              (unsigned long long)v.requested_bytes, (unsigned long long)v.n_bytes_damaged, (long long)v.first_offset);
  }
  std::mutex mu_;
  std::map<int, std::vector<void*>> free_;
  bool off_;
  std::atomic<int> guard_{0};        /* 0 off, 1 fill word 0, 2 fill word 1: the mode new blocks are acquired in */
  std::atomic<bool> guard_seen_{false}; /* the guard has been on: a released pointer may be a guarded block */
  bool guard_env_ = false;           /* switched on by PPF_POOL_GUARD: violations are also printed */
  std::map<void*, GuardBlock> live_; /* handed-out pointer -> its block */
  std::vector<ppf_debug_pool_violation> violations_; /* found at releases since the last check */
  uint64_t n_release_checked_ = 0;
};

void sync_device_of_block(int dev); /* = sync_device, defined below */

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;      /* elements usable */
  size_t granted = 0;  /* bytes of the block behind p */
  int device = 0;      /* device the block lives on */
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { DevPool::get().release(p, granted, device); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) { /* growing a live buffer (rare): earlier asynchronous work may still use the old block */
      sync_device_of_block(device);
      DevPool::get().release(p, granted, device); p = nullptr; cap = 0; granted = 0;
    }
    void* q = nullptr;
    hipError_t e = DevPool::get().acquire(std::max<size_t>(n, 1) * sizeof(T), &q, &granted, &device);
    if (e == hipSuccess) { p = static_cast<T*>(q); cap = n; }
    return e;
  }
  /* like reserve, but a block more than twice as big as needed (and above 16 MiB) is traded for a fitting one: the hit
   * pools of a workspace shrink again after an unusually dense scene */
  hipError_t fit(size_t n) {
    if (p && granted > ((size_t)16 << 20) && granted > 2 * std::max<size_t>(n, 1) * sizeof(T)) {
      sync_device_of_block(device);
      DevPool::get().release(p, granted, device); p = nullptr; cap = 0; granted = 0;
    }
    return reserve(n);
  }
  size_t bytes() const { return granted; }
};

void sync_device(int dev);
void sync_device_of_block(int dev) { sync_device(dev); }

/* wait for everything enqueued on device `dev` (the device a buffer lives on, which need not be the current one) */
void sync_device(int dev) {
  int cur = -1;
  if (dev < 0 || hipGetDevice(&cur) != hipSuccess || cur == dev) { (void)hipDeviceSynchronize(); return; }
  if (hipSetDevice(dev) == hipSuccess) {
    (void)hipDeviceSynchronize();
    (void)hipSetDevice(cur);
  }
}

constexpr int LDS_BYTES = 160 * 1024;              /* LDS per CU == per k_vote workgroup */
constexpr size_t HIT_BYTES_BUDGET = 4ull << 30;    /* hit scratch per batch of reference points */
constexpr float SPILL_ALPHA_MIN = 3.1415f;         /* entries with alpha_m >= this can reach alpha bin == numAngles */

}  // namespace

#endif /* PPF_DEVICE_MEM_H */
