/*
 * ppf_recognize_kernels.h — kernels of ppf_recognizer_create / ppf_recognize_frame: which trained models a proposal cloud can be
 * a view of, from the quantised pair features the models were trained on (the specification is the comment of
 * ppf_recognize_frame in include/ppf_hip.h).  Host side: ppf_recognize_host.h.  Included by ppf_hip.hip after ppf_train_kernels.h
 * (CloudSoA, ld3) and ppf_core.h (ppf_pair_feature, ppf_d2i).
 *
 * A model's key set is a dense bitmap over n_a x n_a x n_a x n_d bins (the last bin of an angle dimension takes INT32_MIN, as
 * key_index_nan does), bit ((k0 * n_a + k1) * n_a + k2) * n_d + k3.
 *   create   k_rec_dmax (the largest distance bin of the model's own pairs, one wait) -> k_rec_build (bits set with vector
 *            atomics on global memory) -> k_rec_popcount (n_keys)
 *   frame    k_rec_score: one workgroup per (proposal, model, 64 reference rows); k_rec_finish: one per (proposal, model)
 * Every sum is an integer and every bitmap is OR-ed, so nothing depends on scheduling.
 */
#ifndef PPF_RECOGNIZE_KERNELS_H
#define PPF_RECOGNIZE_KERNELS_H

constexpr int REC_BLOCK = 256;                     /* threads of a workgroup: four waves */
constexpr int REC_WAVES = REC_BLOCK / 64;
constexpr int REC_SLICE = 64;                      /* reference rows of a scoring workgroup: one per lane */
constexpr int REC_MAX_ROWS = 2048;                 /* ppf_recognize_params.max_rows at most */
constexpr uint32_t REC_LDS_SET_BYTES = 48 * 1024;  /* a key set up to this size is staged in LDS next to its hit bitmap:
                                                      6 x 2,048 floats of rows + 2 x 48 KB = 144 KB of the CU's 160 KB */
constexpr uint64_t REC_NO_HITS = ~0ull;            /* RecPair::hit_off of a proposal without a pair */

struct RecModel {
  const uint32_t* bits; /* the key set */
  uint32_t words;       /* ceil(n_a^3 * n_d / 32) */
  int32_t n_a, n_d;
  int32_t lds;          /* 1: staged in LDS by k_rec_score */
  int32_t pad;
  double angle_step, dist_step;
};
struct RecCloud {
  const float* rows; /* n x 6 */
  int32_t n, step;   /* the candidates are rows 0, step, 2 step, ... */
  int32_t cand, pad; /* ceil(n / step) <= max_rows */
};
struct RecItem {
  uint32_t cloud, model, begin; /* reference candidates begin .. begin + REC_SLICE - 1 */
  uint32_t pair;                /* cloud * n_models + model */
};

/* bit index of the key of the ordered pair (1, 2) in model m's bitmap; false: the key cannot be in the set (its distance bin
 * lies past the model's largest) */
__device__ __forceinline__ bool rec_key_bit(const ppf_vec3& p1, const ppf_vec3& n1, const ppf_vec3& p2, const ppf_vec3& n2,
                                            double angle_step, double dist_step, int32_t n_a, int32_t n_d, uint32_t* bit) {
  double f[4] = {0.0, 0.0, 0.0, 0.0};
  ppf_pair_feature(p1, n1, p2, n2, f);
  const int32_t nan_bin = (int32_t)0x80000000;
  int32_t k0 = ppf_d2i(f[0] / angle_step), k1 = ppf_d2i(f[1] / angle_step), k2 = ppf_d2i(f[2] / angle_step);
  const int32_t k3 = ppf_d2i(f[3] / dist_step);
  if (k0 == nan_bin) k0 = n_a - 1;
  if (k1 == nan_bin) k1 = n_a - 1;
  if (k2 == nan_bin) k2 = n_a - 1;
  /* an angle is in 0..pi or NaN, so its bin is below n_a; the test keeps a wrong step from ever indexing past the bitmap */
  if (!(((uint32_t)k0 < (uint32_t)n_a) & ((uint32_t)k1 < (uint32_t)n_a) & ((uint32_t)k2 < (uint32_t)n_a) & ((uint32_t)k3 < (uint32_t)n_d)))
    return false;
  *bit = (((uint32_t)k0 * (uint32_t)n_a + (uint32_t)k1) * (uint32_t)n_a + (uint32_t)k2) * (uint32_t)n_d + (uint32_t)k3;
  return true;
}

__device__ __forceinline__ uint32_t rec_wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}

/* ---- create: the largest distance bin among the model's ordered pairs (i != j); *dmax comes in zero -------------------- */
__global__ __launch_bounds__(REC_BLOCK) void k_rec_dmax(CloudSoA m, double dist_step, uint32_t* __restrict__ dmax) {
  const int i = blockIdx.x;
  const ppf_vec3 p1 = ld3(m.x, m.y, m.z, i);
  uint32_t best = 0;
  for (int j = threadIdx.x; j < m.n; j += REC_BLOCK) {
    if (j == i) continue;
    const ppf_vec3 p2 = ld3(m.x, m.y, m.z, j);
    /* f[3] of ppf_pair_feature, the same operations in the same order */
    const ppf_vec3 d = ppf_mk3(p2.x - p1.x, p2.y - p1.y, p2.z - p1.z);
    const int32_t k3 = ppf_d2i(ppf_sqrt(d.x * d.x + d.y * d.y + d.z * d.z) / dist_step);
    if (k3 >= 0) best = max(best, (uint32_t)k3);
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o));
  if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(dmax, best);
}

/* ---- create: the key set; bits comes in zero ----------------------------------------------------------------------- */
__global__ __launch_bounds__(REC_BLOCK) void k_rec_build(CloudSoA m, double angle_step, double dist_step, int32_t n_a, int32_t n_d,
                                                         uint32_t* __restrict__ bits) {
  const int i = blockIdx.x;
  const ppf_vec3 p1 = ld3(m.x, m.y, m.z, i), n1 = ld3(m.nx, m.ny, m.nz, i);
  for (int j = threadIdx.x; j < m.n; j += REC_BLOCK) {
    if (j == i) continue;
    const ppf_vec3 p2 = ld3(m.x, m.y, m.z, j), n2 = ld3(m.nx, m.ny, m.nz, j);
    uint32_t bit;
    if (!rec_key_bit(p1, n1, p2, n2, angle_step, dist_step, n_a, n_d, &bit)) continue;
    uint32_t* w = bits + (bit >> 5);
    const uint32_t b = 1u << (bit & 31u);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b)) atomicOr(w, b);
  }
}

/* ---- create: *total (zero on entry) += the set bits of bits[0 .. words) ---------------------------------------------- */
__global__ __launch_bounds__(REC_BLOCK) void k_rec_popcount(const uint32_t* __restrict__ bits, uint32_t words, uint32_t* __restrict__ total) {
  uint32_t s = 0;
  for (uint32_t w = blockIdx.x * REC_BLOCK + threadIdx.x; w < words; w += gridDim.x * REC_BLOCK) s += (uint32_t)__popc(bits[w]);
  s = rec_wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

/* ---- frame: the pairs of 64 reference rows of one proposal against one model ------------------------------------------
 * LDS: six planes of row_cap floats (every candidate row of the proposal; a row with a non-finite value has x = NaN and is no
 * row at all), then, for a model staged in LDS, its key set and a hit bitmap of the same size (lds_words each).  Lane l of
 * every wave owns reference row begin + l; wave w walks the partner rows w, w + 4, ...: a partner is one LDS address for
 * the whole wave (a broadcast).  n_known is counted in a register, summed over the wave and the workgroup and added to
 * global memory once; a hit bit is OR-ed only where it is not set yet, and the workgroup's hit words go to the pair's
 * global hit bitmap (hits + pair_hit_off[pair], zero on entry) at the end -- directly, bit by bit, for a key set that is read
 * from global memory.  counts: [pairs][2], word 0 = n_known (zero on entry); k_rec_finish writes word 1. */
__global__ __launch_bounds__(REC_BLOCK) void k_rec_score(const RecItem* __restrict__ items, int n_items, const RecCloud* __restrict__ clouds,
                                                         const RecModel* __restrict__ models, int row_cap, uint32_t lds_words,
                                                         uint32_t* __restrict__ hits, const unsigned long long* __restrict__ pair_hit_off,
                                                         unsigned long long* __restrict__ counts, int32_t* __restrict__ n_used) {
  extern __shared__ uint32_t rec_lds[];
  __shared__ uint32_t s_used, s_known;
  if ((int)blockIdx.x >= n_items) return;
  const RecItem it = items[blockIdx.x];
  const RecCloud cl = clouds[it.cloud];
  const RecModel md = models[it.model];
  float* rows = reinterpret_cast<float*>(rec_lds);
  uint32_t* set = rec_lds + (size_t)6 * row_cap;
  uint32_t* hit = set + lds_words;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { s_used = 0; s_known = 0; }
  uint32_t used = 0;
  for (int c = tid; c < cl.cand; c += REC_BLOCK) {
    const float* r = cl.rows + (size_t)c * (size_t)cl.step * 6;
    float v[6];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      v[k] = r[k];
      ok = ok && (fabsf(v[k]) <= 3.402823466e+38f); /* finite: false for NaN and the infinities */
    }
    rows[c] = ok ? v[0] : __int_as_float(0x7fc00000);
#pragma unroll
    for (int k = 1; k < 6; k++) rows[k * row_cap + c] = v[k];
    used += ok ? 1u : 0u;
  }
  if (md.lds)
    for (uint32_t w = tid; w < md.words; w += REC_BLOCK) {
      set[w] = md.bits[w];
      hit[w] = 0u;
    }
  __syncthreads();
  used = rec_wave_sum(used);
  if (lane == 0 && used) atomicAdd(&s_used, used);

  uint32_t* ghit = hits + pair_hit_off[it.pair];
  const int i = (int)it.begin + lane;
  const float xi = rows[i < cl.cand ? i : 0]; /* an item's proposal has a candidate */
  const bool live = i < cl.cand && xi == xi;
  uint32_t known = 0;
  if (live) {
    const ppf_vec3 p1 = ppf_mk3((double)rows[i], (double)rows[row_cap + i], (double)rows[2 * row_cap + i]);
    const ppf_vec3 n1 = ppf_mk3((double)rows[3 * row_cap + i], (double)rows[4 * row_cap + i], (double)rows[5 * row_cap + i]);
    for (int j = wave; j < cl.cand; j += REC_WAVES) {
      const float xj = rows[j];
      if (!(xj == xj) || j == i) continue;
      const ppf_vec3 p2 = ppf_mk3((double)xj, (double)rows[row_cap + j], (double)rows[2 * row_cap + j]);
      const ppf_vec3 n2 = ppf_mk3((double)rows[3 * row_cap + j], (double)rows[4 * row_cap + j], (double)rows[5 * row_cap + j]);
      uint32_t bit;
      if (!rec_key_bit(p1, n1, p2, n2, md.angle_step, md.dist_step, md.n_a, md.n_d, &bit)) continue;
      const uint32_t w = bit >> 5, b = 1u << (bit & 31u);
      if (md.lds) {
        if (set[w] & b) {
          known++;
          if (!(__hip_atomic_load(hit + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & b)) atomicOr(hit + w, b);
        }
      } else if (md.bits[w] & b) {
        known++;
        if (!(__hip_atomic_load(ghit + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b)) atomicOr(ghit + w, b);
      }
    }
  }
  known = rec_wave_sum(known);
  if (lane == 0 && known) atomicAdd(&s_known, known);
  __syncthreads();
  if (md.lds)
    for (uint32_t w = tid; w < md.words; w += REC_BLOCK) {
      const uint32_t h = hit[w];
      if (h && (__hip_atomic_load(ghit + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & h) != h) atomicOr(ghit + w, h);
    }
  if (tid == 0) {
    if (s_known) atomicAdd(counts + (size_t)2 * it.pair, (unsigned long long)s_known);
    if (it.model == 0 && it.begin == 0) n_used[it.cloud] = (int32_t)s_used;
  }
}

/* ---- frame: n_keys_hit of every (proposal, model) = the set bits of its merged hit bitmap ----------------------------- */
__global__ __launch_bounds__(REC_BLOCK) void k_rec_finish(int n_pairs, int n_models, const RecModel* __restrict__ models,
                                                          const uint32_t* __restrict__ hits, const unsigned long long* __restrict__ pair_hit_off,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_sum;
  const int pair = blockIdx.x;
  if (pair >= n_pairs) return;
  const unsigned long long off = pair_hit_off[pair];
  if (off == REC_NO_HITS) return; /* counts stay zero */
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const uint32_t words = models[pair % n_models].words;
  const uint32_t* h = hits + off;
  uint32_t s = 0;
  for (uint32_t w = threadIdx.x; w < words; w += REC_BLOCK) s += (uint32_t)__popc(h[w]);
  s = rec_wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(&s_sum, s);
  __syncthreads();
  if (threadIdx.x == 0) counts[(size_t)2 * pair + 1] = s_sum;
}

#endif /* PPF_RECOGNIZE_KERNELS_H */
