/*
 * ppf_history_kernels.h — the last K depth images of a fixed camera fused into one on gfx950 (ppf_depth_history, DESIGN.md
 * §26).  Included by ppf_hip.hip after ppf_depth_kernels.h (DepthArgs, depth_z, depth_keep); host side: ppf_history_host.h.
 *
 *   k_history_push<T, K>   one lane owns four consecutive pixels of one image row, so the ring and the output move 16 bytes per
 *                    lane and access.  The ring is `window` float planes (z of a kept pixel, 0 elsewhere) whose rows are
 *                    padded to a multiple of four pixels: a lane's float4 is aligned in every plane whatever cols is, and the
 *                    pad columns are written as 0 and never used.  A lane converts its four input pixels through the row
 *                    pitch (one 16- or 8-byte load where pitch and pointer allow it, element loads otherwise and in a row's
 *                    tail), stores them into plane t mod window, loads the other n_hist - 1 planes (ages past n_hist are 0:
 *                    not kept) and decides each pixel from its K samples in registers: every loop over the ages is unrolled,
 *                    no array is indexed by a run-time value.  The median is a bitonic network over the consensus' values as
 *                    their bit patterns -- a kept float is positive, so unsigned integer order is its order -- with the others
 *                    set to all ones; the rank is picked by a chain of selects.  The mean is one sequential fp64 sum, oldest
 *                    first.  out takes one float4 store where cols and the pointer allow it, element stores otherwise; state
 *                    likewise four bytes in one store.  The five counts come from ballots: one integer atomicAdd each per
 *                    workgroup.
 * K is the instantiation (1, 2, 4, 8, 16: the smallest that holds `window`); the ages window .. K - 1 are masked with the
 * same test as the ages the history has not seen yet.  Nothing is fused (-ffp-contract=off), no float atomic; the launch
 * depends on the image size alone.
 */
#ifndef PPF_HISTORY_KERNELS_H
#define PPF_HISTORY_KERNELS_H

constexpr int DH_BLOCK = 256;
constexpr int DH_PX = 4; /* pixels per lane */
constexpr int DH_C_KEPT = 0, DH_C_MEASURED = 1, DH_C_FILLED = 2, DH_C_UNSUPPORTED = 3, DH_C_CHANGED = 4, DH_N_COUNTERS = 5;
constexpr uint32_t DH_ABSENT = 0xffffffffu; /* above every kept float's bits */

struct HistoryArgs {
  int rows, groups;     /* groups of DH_PX pixels per row: ceil(cols / 4); the ring's row pitch is groups * 4 floats */
  int n_hist, slot;     /* min(t + 1, window); the plane frame t goes to: t mod window */
  int window;
  int min_support, max_age, mean;
  float range_abs, range_quad;
  size_t plane;         /* floats per ring plane: rows * groups * 4 */
  float* ring;          /* window planes */
  float* out;           /* packed rows x cols */
  uint8_t* state;       /* packed rows x cols, or nullptr */
  int in_vec, out_vec, state_vec; /* the whole-lane accesses are aligned: decided on the host from pointers, pitch and cols */
  int32_t* counters;    /* DH_N_COUNTERS, preset to 0 */
};

/* a lane's four input pixels as z, 0 where the pixel is not kept or lies past the row's end; in_vec: the whole-lane load is
 * aligned (decided on the host from pointer and pitch).  Shared with ppf_motion_kernels.h. */
template <class T>
__device__ __forceinline__ void history_load(const DepthArgs& a, int in_vec, int v, int u0, float (&z)[DH_PX]) {
  const T* row = reinterpret_cast<const T*>(a.img + (size_t)v * a.pitch) + u0;
  T px[DH_PX];
  if (in_vec && u0 + DH_PX <= a.cols) {
    struct alignas(sizeof(T) * DH_PX) Quad { T e[DH_PX]; };
    const Quad q = *reinterpret_cast<const Quad*>(row);
#pragma unroll
    for (int j = 0; j < DH_PX; j++) px[j] = q.e[j];
  } else {
#pragma unroll
    for (int j = 0; j < DH_PX; j++) px[j] = u0 + j < a.cols ? row[j] : T(0);
  }
#pragma unroll
  for (int j = 0; j < DH_PX; j++) {
    const float zq = depth_z(&px[j], a);
    z[j] = (u0 + j < a.cols && depth_keep(zq, a)) ? zq : 0.f;
  }
}

__device__ __forceinline__ void history_cswap(uint32_t& lo, uint32_t& hi) {
  const uint32_t a = lo, b = hi;
  lo = a < b ? a : b;
  hi = a < b ? b : a;
}

/* one pixel from its K samples by age (0: not kept); returns the state, *res = the value */
template <int K>
__device__ __forceinline__ int history_pixel(const float (&s)[K], const HistoryArgs& ha, float* res) {
  *res = 0.f;
  int astar = -1;
  float za = 0.f;
  bool older = false;
#pragma unroll
  for (int a = K - 1; a >= 0; a--) { /* descending, so the smallest age is the one that stays */
    const bool kept = s[a] > 0.f;
    if (kept && a <= ha.max_age) {
      astar = a;
      za = s[a];
    }
    if (a > 0) older = older || kept;
  }
  if (astar < 0) return 0;
  const double Za = (double)za;
  const double R = (double)ha.range_abs + (double)ha.range_quad * (Za * Za);
  bool in[K];
  int n = 0;
#pragma unroll
  for (int a = 0; a < K; a++) {
    in[a] = s[a] > 0.f && ppf_fabs((double)s[a] - Za) <= R;
    n += in[a] ? 1 : 0;
  }
  if (n < ha.min_support) return PPF_HISTORY_UNSUPPORTED;
  if (ha.mean) {
    double sum = 0.0;
#pragma unroll
    for (int a = K - 1; a >= 0; a--)
      if (in[a]) sum = sum + (double)s[a];
    *res = (float)(sum / (double)n);
  } else {
    uint32_t w[K];
#pragma unroll
    for (int a = 0; a < K; a++) w[a] = in[a] ? __float_as_uint(s[a]) : DH_ABSENT;
    /* bitonic network, ascending; K is a power of two */
#pragma unroll
    for (int k = 2; k <= K; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
        for (int i = 0; i < K; i++) {
          const int l = i ^ j;
          if (l > i) {
            if ((i & k) == 0) history_cswap(w[i], w[l]);
            else history_cswap(w[l], w[i]);
          }
        }
    const int rank = (n - 1) >> 1;
    uint32_t m = w[0];
#pragma unroll
    for (int i = 1; i < K; i++) m = rank == i ? w[i] : m;
    *res = __uint_as_float(m);
  }
  if (astar > 0) return PPF_HISTORY_FILLED;
  return PPF_HISTORY_MEASURED | ((n == 1 && older) ? PPF_HISTORY_CHANGED : 0);
}

template <class T, int K>
__global__ __launch_bounds__(DH_BLOCK) void k_history_push(DepthArgs a, HistoryArgs ha) {
  static_assert(K >= 1 && K <= PPF_HISTORY_MAX_WINDOW && (K & (K - 1)) == 0, "the network needs a power of two");
  __shared__ int s_n[DH_BLOCK / 64][DH_N_COUNTERS];
  const long long g = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
  const bool active = g < (long long)ha.rows * ha.groups;
  const int v = active ? (int)(g / ha.groups) : 0;
  const int u0 = active ? (int)(g - (long long)v * ha.groups) * DH_PX : 0;
  int st[DH_PX] = {0, 0, 0, 0};
  bool kept[DH_PX] = {false, false, false, false};
  if (active) {
    float s[DH_PX][K];
    {
      float z[DH_PX];
      history_load<T>(a, ha.in_vec, v, u0, z);
#pragma unroll
      for (int j = 0; j < DH_PX; j++) {
        s[j][0] = z[j];
        kept[j] = z[j] > 0.f;
      }
    }
    const size_t cell = ((size_t)v * (size_t)ha.groups) * DH_PX + (size_t)u0; /* inside a plane; a multiple of 4 */
    *reinterpret_cast<float4*>(ha.ring + (size_t)ha.slot * ha.plane + cell) = make_float4(s[0][0], s[1][0], s[2][0], s[3][0]);
#pragma unroll
    for (int age = 1; age < K; age++) {
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (age < ha.n_hist) { /* uniform; n_hist <= window, so the plane exists */
        int p = ha.slot - age;
        p += p < 0 ? ha.window : 0;
        q = *reinterpret_cast<const float4*>(ha.ring + (size_t)p * ha.plane + cell);
      }
      s[0][age] = q.x;
      s[1][age] = q.y;
      s[2][age] = q.z;
      s[3][age] = q.w;
    }
    float res[DH_PX];
#pragma unroll
    for (int j = 0; j < DH_PX; j++) st[j] = history_pixel<K>(s[j], ha, &res[j]);
    const size_t o = (size_t)v * (size_t)a.cols + (size_t)u0;
    if (ha.out_vec) {
      *reinterpret_cast<float4*>(ha.out + o) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
#pragma unroll
      for (int j = 0; j < DH_PX; j++)
        if (u0 + j < a.cols) ha.out[o + j] = res[j];
    }
    if (ha.state) {
      if (ha.state_vec) {
        *reinterpret_cast<uint32_t*>(ha.state + o) = (uint32_t)st[0] | (uint32_t)st[1] << 8 | (uint32_t)st[2] << 16 | (uint32_t)st[3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < DH_PX; j++)
          if (u0 + j < a.cols) ha.state[o + j] = (uint8_t)st[j];
      }
    }
  }
  /* a pixel past the row's end, or of an inactive lane, has kept false and state 0: it counts nowhere */
  int n[DH_N_COUNTERS] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < DH_PX; j++) {
    n[DH_C_KEPT] += __popcll(__ballot(kept[j]));
    n[DH_C_MEASURED] += __popcll(__ballot((st[j] & 15) == PPF_HISTORY_MEASURED));
    n[DH_C_FILLED] += __popcll(__ballot(st[j] == PPF_HISTORY_FILLED));
    n[DH_C_UNSUPPORTED] += __popcll(__ballot(st[j] == PPF_HISTORY_UNSUPPORTED));
    n[DH_C_CHANGED] += __popcll(__ballot((st[j] & PPF_HISTORY_CHANGED) != 0));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < DH_N_COUNTERS; c++) s_n[wv][c] = n[c];
  }
  __syncthreads();
  if (threadIdx.x < DH_N_COUNTERS) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < DH_BLOCK / 64; w++) t += s_n[w][threadIdx.x];
    if (t) atomicAdd(&ha.counters[threadIdx.x], t);
  }
}

#endif /* PPF_HISTORY_KERNELS_H */
