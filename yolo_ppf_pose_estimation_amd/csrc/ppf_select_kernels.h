/*
 * ppf_select_kernels.h — one consistent set of poses per frame on gfx950: the bit-packed supported-pixel
 * masks of every hypothesis, their pairwise intersections, the greedy selection and the images of the selected poses.
 * Included by ppf_hip.hip after ppf_render_kernels.h (RndWin, RND_EMPTY, the per-job windows of k_rnd_splat); the host side
 * is ppf_select_host.h.
 *
 * A hypothesis is a job q (dense, in flat order j = i * top + k).  Its mask S holds one bit per pixel of its window, in u64
 * words aligned to image column u & ~63, so the words of two hypotheses on one image row line up and an intersection is a
 * popcount of A & B over the words the two windows share.
 *   k_sel_mask     a wave per mask word, eight words in turn: 64 consecutive pixels of the window against the depth image,
 *                  the wave's ballot is the word; n_drawn and n_supported from popcounts, one integer atomic each per block
 *   k_sel_key      one thread per hypothesis: explained, key, the gate, the info row and the 64-bit sort key
 *   k_sel_overlap  one wave per pair of eligible hypotheses (a < b): the intersection, the conflict test, two bits of the
 *                  conflict matrix (integer atomicOr); pairs with disjoint windows leave at once
 *   k_sel_greedy   one workgroup: a bitonic sort of the (key, q) words in LDS, then the greedy pass, serial over the
 *                  candidates in order and parallel over the later candidates each selected one suppresses
 *   k_sel_report   one wave per suppressed hypothesis: its intersection with its suppressor
 *   k_sel_paint    one thread per window pixel of a selected hypothesis: u64 atomicMin of (depth bits << 32 | j) into the
 *                  frame buffer that k_rnd_resolve turns into the two images
 * Integer atomics only; every output is an integer or a fixed fp32 / fp64 expression of integers.
 */
#ifndef PPF_SELECT_KERNELS_H
#define PPF_SELECT_KERNELS_H

constexpr int SEL_BLOCK = 256;
constexpr int SEL_WAVES = SEL_BLOCK / 64;
constexpr int SEL_MASK_WORDS = 32; /* mask words per block of k_sel_mask: eight per wave */
constexpr int SEL_MAX_JOBS = 4096; /* n_dets 256 x top 16: what k_sel_greedy sorts in LDS */
constexpr int SEL_GREEDY_BLOCK = 1024;
constexpr unsigned long long SEL_NO_KEY = ~0ull; /* the sort key of a gated hypothesis: after every eligible one */

/* the mask of a job: words per window row, the word column (u >> 6) of the first, stored row-major from off (in words) */
struct SelMask {
  int wc0, ww;
  unsigned long long off;
};

struct SelGate {
  float min_score;
  int min_pixels;
};

/* grid (blocks of the largest mask) x jobs, SEL_MASK_WORDS words per block; counts[2 q] = n_drawn, counts[2 q + 1] =
 * n_supported, preset to 0 */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_mask(const RndWin* __restrict__ wins, const SelMask* __restrict__ masks,
                                                        const uint32_t* __restrict__ zbuf, const float* __restrict__ depth, int cols,
                                                        float tol, unsigned long long* __restrict__ bits, int* __restrict__ counts) {
  __shared__ int s_n[SEL_WAVES][2];
  const int q = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RndWin W = wins[q];
  const SelMask M = masks[q];
  const long long n_words = (long long)M.ww * W.h;
  if ((long long)blockIdx.x * SEL_MASK_WORDS >= n_words) return; /* uniform per block */
  int nd = 0, ns = 0; /* the same in every lane of the wave */
  for (int k = 0; k < SEL_MASK_WORDS / SEL_WAVES; k++) {
    const long long wi = (long long)blockIdx.x * SEL_MASK_WORDS + wv * (SEL_MASK_WORDS / SEL_WAVES) + k;
    if (wi >= n_words) break; /* uniform per wave */
    const int row = (int)(wi / M.ww), u = (M.wc0 + (int)(wi % M.ww)) * 64 + lane;
    bool drawn = false, supported = false;
    if (u >= W.u0 && u < W.u0 + W.w) { /* inside the window, so inside the image */
      const uint32_t zb = zbuf[W.off + (size_t)row * W.w + (u - W.u0)];
      if (zb != RND_EMPTY) {
        drawn = true;
        const float d = depth[(size_t)(W.v0 + row) * cols + u];
        supported = isfinite(d) && d > 0.f && fabsf(d - __uint_as_float(zb)) <= tol;
      }
    }
    const unsigned long long bd = __ballot(drawn), bs = __ballot(supported);
    if (lane == 0) bits[M.off + wi] = bs;
    nd += __popcll(bd);
    ns += __popcll(bs);
  }
  if (lane == 0) {
    s_n[wv][0] = nd;
    s_n[wv][1] = ns;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int n = 0;
    for (int w = 0; w < SEL_WAVES; w++) n += s_n[w][threadIdx.x];
    if (n) atomicAdd(&counts[2 * q + threadIdx.x], n);
  }
}

/* descending key, then ascending q, as one ascending u64; -0 ranks as +0 */
__device__ __forceinline__ unsigned long long sel_sort_key(float key, int q) {
  uint32_t b = __float_as_uint(key == 0.f ? 0.f : key);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u); /* ascending with the float */
  return ((unsigned long long)(~b) << 32) | (uint32_t)q;
}

/* one thread per job: score == nullptr ranks by explained */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_key(const int* __restrict__ counts, const float* __restrict__ score, int nj, SelGate g,
                                                       ppf_select_info* __restrict__ info, unsigned long long* __restrict__ skey) {
  const int q = blockIdx.x * SEL_BLOCK + threadIdx.x;
  if (q >= nj) return;
  const int nd = counts[2 * q], ns = counts[2 * q + 1];
  const float explained = nd > 0 ? (float)((double)ns / (double)nd) : 0.f;
  const float key = score ? score[q] : explained;
  const bool eligible = key >= g.min_score && ns >= g.min_pixels; /* false for a NaN key */
  ppf_select_info r;
  r.status = eligible ? PPF_SELECT_SELECTED : PPF_SELECT_GATED; /* k_sel_greedy settles the eligible ones */
  r.rank = -1;
  r.suppressed_by = -1;
  r.n_drawn = nd;
  r.n_supported = ns;
  r.n_overlap = 0;
  r.explained = explained;
  r.key = key;
#pragma unroll
  for (int k = 0; k < 4; k++) r.reserved[k] = 0;
  info[q] = r;
  skey[q] = eligible ? sel_sort_key(key, q) : SEL_NO_KEY;
}

/* |S_a ∩ S_b| by one wave: the words of the rows and word columns both windows hold; every lane returns the sum */
__device__ __forceinline__ int sel_intersection(const RndWin& A, const SelMask& MA, const RndWin& B, const SelMask& MB,
                                                const unsigned long long* __restrict__ bits, int lane) {
  const int v_lo = max(A.v0, B.v0), v_hi = min(A.v0 + A.h, B.v0 + B.h);
  const int c_lo = max(MA.wc0, MB.wc0), c_hi = min(MA.wc0 + MA.ww, MB.wc0 + MB.ww);
  if (v_lo >= v_hi || c_lo >= c_hi) return 0; /* disjoint (or an empty window) */
  const int nc = c_hi - c_lo;
  const long long n = (long long)nc * (v_hi - v_lo);
  int sum = 0;
  for (long long t = lane; t < n; t += 64) {
    const int v = v_lo + (int)(t / nc), c = c_lo + (int)(t % nc);
    const unsigned long long a = bits[MA.off + (size_t)(v - A.v0) * MA.ww + (c - MA.wc0)];
    const unsigned long long b = bits[MB.off + (size_t)(v - B.v0) * MB.ww + (c - MB.wc0)];
    sum += __popcll(a & b);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  return sum;
}

/* grid (blocks of nj waves) x nj: the wave of pair (a = blockIdx.y, b); conf is nj rows of cw u32, preset to 0 */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_overlap(const RndWin* __restrict__ wins, const SelMask* __restrict__ masks,
                                                           const unsigned long long* __restrict__ bits,
                                                           const unsigned long long* __restrict__ skey,
                                                           const ppf_select_info* __restrict__ info, int nj, double max_overlap,
                                                           uint32_t* __restrict__ conf, int cw) {
  const int a = blockIdx.y, b = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b <= a || b >= nj) return; /* uniform per wave */
  if (skey[a] == SEL_NO_KEY || skey[b] == SEL_NO_KEY) return;
  const RndWin A = wins[a], B = wins[b];
  const int ov = sel_intersection(A, masks[a], B, masks[b], bits, lane);
  if (lane != 0 || ov == 0) return; /* no shared pixel is never a conflict: max_overlap >= 0 */
  const int m = min(info[a].n_supported, info[b].n_supported);
  if ((double)ov > max_overlap * (double)m) {
    atomicOr(&conf[(size_t)a * cw + (b >> 5)], 1u << (b & 31));
    atomicOr(&conf[(size_t)b * cw + (a >> 5)], 1u << (a & 31));
  }
}

/* one workgroup.  flat[q] = j; selected (preset to -1) takes the selected j in order, count = {n_selected, n_eligible},
 * sup_of[q] (preset to -1) the job that suppressed q */
__global__ __launch_bounds__(SEL_GREEDY_BLOCK) void k_sel_greedy(const unsigned long long* __restrict__ skey, int nj,
                                                                 const uint32_t* __restrict__ conf, int cw, const int* __restrict__ flat,
                                                                 ppf_select_info* __restrict__ info, int* __restrict__ selected,
                                                                 int* __restrict__ count, int* __restrict__ sup_of) {
  __shared__ unsigned long long s_key[SEL_MAX_JOBS];
  __shared__ int s_sup[SEL_MAX_JOBS];
  __shared__ int s_ne;
  const int tid = threadIdx.x;
  int n2 = 2;
  while (n2 < nj) n2 <<= 1; /* nj <= SEL_MAX_JOBS */
  for (int i = tid; i < n2; i += SEL_GREEDY_BLOCK) {
    s_key[i] = i < nj ? skey[i] : SEL_NO_KEY;
    s_sup[i] = -1;
  }
  if (tid == 0) s_ne = 0;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += SEL_GREEDY_BLOCK) {
        const int i = ((t & ~(s - 1)) << 1) | (t & (s - 1)), p = i | s; /* the pair (i, i + s) of this step */
        const unsigned long long x = s_key[i], y = s_key[p];
        if ((x > y) == ((i & k) == 0)) {
          s_key[i] = y;
          s_key[p] = x;
        }
      }
      __syncthreads();
    }
  /* the keys are distinct, so the eligible ones are the first s_ne */
  for (int i = tid; i < n2; i += SEL_GREEDY_BLOCK)
    if (s_key[i] != SEL_NO_KEY && (i + 1 == n2 || s_key[i + 1] == SEL_NO_KEY)) s_ne = i + 1;
  __syncthreads();
  const int ne = s_ne;
  int n_sel = 0;
  for (int t = 0; t < ne; t++) {
    if (s_sup[t] >= 0) continue; /* uniform: every write to s_sup is followed by a barrier */
    const int a = (int)(uint32_t)s_key[t];
    if (tid == 0) {
      info[a].rank = n_sel;
      selected[n_sel] = flat[a];
    }
    n_sel++;
    const uint32_t* row = conf + (size_t)a * cw;
    for (int r = t + 1 + tid; r < ne; r += SEL_GREEDY_BLOCK)
      if (s_sup[r] < 0) {
        const int b = (int)(uint32_t)s_key[r];
        if ((row[b >> 5] >> (b & 31)) & 1u) s_sup[r] = a; /* a is the earliest selected one b conflicts with */
      }
    __syncthreads();
  }
  for (int r = tid; r < ne; r += SEL_GREEDY_BLOCK)
    if (s_sup[r] >= 0) {
      const int b = (int)(uint32_t)s_key[r];
      info[b].status = PPF_SELECT_SUPPRESSED;
      info[b].suppressed_by = flat[s_sup[r]];
      sup_of[b] = s_sup[r];
    }
  if (tid == 0) {
    count[0] = n_sel;
    count[1] = ne;
  }
}

/* one wave per job: n_overlap of a suppressed hypothesis */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_report(const RndWin* __restrict__ wins, const SelMask* __restrict__ masks,
                                                          const unsigned long long* __restrict__ bits, const int* __restrict__ sup_of, int nj,
                                                          ppf_select_info* __restrict__ info) {
  const int q = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= nj) return;
  const int a = sup_of[q];
  if (a < 0) return;
  const RndWin A = wins[a], B = wins[q];
  const int ov = sel_intersection(A, masks[a], B, masks[q], bits, lane);
  if (lane == 0) info[q].n_overlap = ov;
}

/* grid (blocks of the largest window) x jobs: the drawn pixels of the selected hypotheses into the frame buffer */
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_paint(const RndWin* __restrict__ wins, const uint32_t* __restrict__ zbuf,
                                                         const ppf_select_info* __restrict__ info, const int* __restrict__ flat, int cols,
                                                         unsigned long long* __restrict__ frame) {
  const int q = blockIdx.y;
  if (info[q].rank < 0) return; /* uniform per block: not selected */
  const RndWin W = wins[q];
  const long long p = (long long)blockIdx.x * SEL_BLOCK + threadIdx.x;
  if (p >= (long long)W.w * W.h) return;
  const uint32_t zb = zbuf[W.off + p];
  if (zb == RND_EMPTY) return;
  const int v = W.v0 + (int)(p / W.w), u = W.u0 + (int)(p % W.w);
  atomicMin(&frame[(size_t)v * cols + u], ((unsigned long long)zb << 32) | (uint32_t)flat[q]);
}

#endif /* PPF_SELECT_KERNELS_H */
