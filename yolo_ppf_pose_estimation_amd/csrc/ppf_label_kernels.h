/*
 * ppf_label_kernels.h — what the stages that label connected components on the device share: ppf_prep_clusters
 * (ppf_cluster_kernels.h), ppf_prep_regions (ppf_region_kernels.h) and ppf_depth_segments (ppf_segment_kernels.h).  Device
 * functions only, no kernel.  Included by ppf_hip.hip before ppf_cluster_kernels.h.
 *
 *   uf_find / uf_unite  a lock-free union-find over indices, in HBM or in LDS: a parent is always a smaller index, so a root
 *                       is its set's smallest member.  While a kernel unites, every read of parent[] is an agent-scope relaxed
 *                       atomic load (uf_ld; L1 is per CU: a plain load may return a stale line for ever), every write a
 *                       compare-and-swap on a root, or the atomic store (uf_st) of a grandparent (path halving): parent[] is
 *                       touched by uf_ld / uf_st / uf_unite's compare-and-swap only.
 *   uf_root             the walk to the root by plain loads, for use once nobody writes parent[] any more: after a barrier
 *                       (LDS) or a launch boundary (HBM).
 *   cells_lower_bound   a binary search in an ascending table of 64-bit keys (the table of occupied cells).
 *   wave_max_by_key     per-set maxima of W words: a wave that lies in one set combines by shuffles and adds once.
 *
 * Why every loop ends.  uf_find and uf_root step to a strictly smaller index.  uf_unite retries only after a failed
 * compare-and-swap, which means another thread's succeeded, and the number of roots only falls.  No workgroup waits for
 * another.
 */
#ifndef PPF_LABEL_KERNELS_H
#define PPF_LABEL_KERNELS_H

/* a word that other workgroups of the running kernel write: read from L2, never from this CU's L1 */
__device__ __forceinline__ uint32_t agent_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t uf_ld(const uint32_t* p) { return agent_ld(p); }
__device__ __forceinline__ void uf_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
/* the root of x as far as this thread can see.  A member that is not a root never becomes one again and its parent only ever
 * moves to another member of its set: storing a grandparent is safe whatever other threads do */
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_ld(parent + x);
    if (p == x) return x;
    const uint32_t gp = uf_ld(parent + p);
    if (gp == p) return p;
    uf_st(parent + x, gp);
    x = gp;
  }
}
/* the larger root is hung under the smaller.  A failed compare-and-swap: another thread hung that root first */
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    if (atomicCAS(parent + a, a, b) == a) return;
  }
}
__device__ __forceinline__ uint32_t uf_root(const uint32_t* __restrict__ parent, uint32_t r) {
  for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
  return r;
}

/* the first index in lo .. hi whose key is >= want (hi: none) */
__device__ __forceinline__ uint32_t cells_lower_bound(const unsigned long long* __restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long want) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

/* Every lane of the wave calls it: `in` says the lane holds words v[] (zero: the identity) for the set `key`.  When the live
 * lanes lie in one set, lane 0 ends up with the wave's maxima and that set's key (lane 0 may itself be in none) and is the
 * only lane that adds; otherwise every live lane adds its own.  Returns whether this lane adds */
template <int W>
__device__ __forceinline__ bool wave_max_by_key(bool in, uint32_t& key, uint32_t (&v)[W]) {
  const unsigned long long live = __ballot(in);
  if (!live) return false;
  const uint32_t key0 = (uint32_t)__shfl((int)key, __ffsll((long long)live) - 1);
  if (__all(!in || key == key0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < W; k++) v[k] = max(v[k], (uint32_t)__shfl_down((int)v[k], o));
    }
    if ((threadIdx.x & 63) != 0) return false;
  } else if (!in) {
    return false;
  }
  if ((threadIdx.x & 63) == 0) key = key0;
  return true;
}

#endif /* PPF_LABEL_KERNELS_H */
