/*
 * ppf_volume_mesh_kernels.h — the zero surface of a ppf_depth_volume as a triangle mesh by marching tetrahedra on gfx950
 * (ppf_depth_volume_mesh).  Included by ppf_hip.hip after ppf_volume_kernels.h (VolArgs, VolVoxel,
 * volume_gradient); host side: ppf_volume_host.h.  One lane per voxel in tiles of VM_BLOCK = 256 consecutive voxels, as
 * k_volume_cross has them; a voxel is the corner 0 of a cube and the owner of up to seven edges.
 *
 *   k_vmesh_cells      a byte per voxel as a cube's corner 0: 0x80 | triangles (0..12) when all eight corners are valid, else
 *                      0; the tile's triangles -> tri_counts[tile]; active cubes and triangles -> two 64-bit counters.
 *   k_vmesh_edges      a 7-bit mask per voxel as an edge owner: bit e when the edge's ends differ in sign and one of the cubes
 *                      that contain it (the cell bytes of this voxel and of the at most seven behind it) is active; the
 *                      voxel's rank among the tile's vertices (seven ballots + mbcnt, at most 1,792 a tile) as 16 bits; the
 *                      tile's vertices -> vert_counts[tile]; vertices -> a 64-bit counter.
 *   k_vmesh_vertices   after the exclusive scan of vert_counts: a voxel's vertices in type order at the tile's offset + its rank.
 *   k_vmesh_triangles  after the exclusive scan of tri_counts: a cube's place is the tile's offset + the waves before + the
 *                      triangles of the lanes below (four ballots over the bits of the count + mbcnt); the six cases again
 *                      from the eight signs; a vertex index is the owner's tile offset + the owner's rank +
 *                      popcount(mask & ((1 << e) - 1)).
 * The rule's table is the same for every tetrahedron but for a swap that the parity of its axis permutation decides, so it is
 * 16 cases of at most two triangles of local edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3): seven integer constants, one per
 * field, shifted by the case.  There is no table in memory and no array that a lane indexes at run time.
 * Everything is fp64 as written, left to right, nothing fused (-ffp-contract=off); no float atomic, no inline assembly, no
 * grid-wide synchronisation; scratch memory per voxel: 1 + 1 + 2 = 4 bytes.
 */
#ifndef PPF_VOLUME_MESH_KERNELS_H
#define PPF_VOLUME_MESH_KERNELS_H

constexpr int VM_BLOCK = DV_X_BLOCK; /* voxels per tile */
constexpr int VM_WAVES = VM_BLOCK / 64;
/* counters of a call */
constexpr int VM_N_CELLS = 0, VM_N_TRIANGLES = 1, VM_N_VERTICES = 2, VM_N_NO_NORMAL = 3, VM_COUNTERS = 4;

/* tetrahedron ti = (0, t1, t2, 7): the axis permutations in lexicographic order; bit ti of VM_PARITY: odd permutation */
constexpr uint32_t VM_T1 = 1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15;
constexpr uint32_t VM_T2 = 3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15;
constexpr uint32_t VM_PARITY = 0x26u;
/* per case (bit n: corner t_n positive): the triangles, two bits a case; and the local edge of each of the six triangle
 * corners, three bits a case, oriented for an even tetrahedron (an odd one swaps the second and third corner) */
constexpr uint32_t VM_COUNT = 0x16696994u;
constexpr unsigned long long VM_V0 = 0x001202401200ull, VM_V1 = 0x062764a6d6d0ull, VM_V2 = 0x09caad95b908ull,
                             VM_V3 = 0x001000000200ull, VM_V4 = 0x0040e8150800ull, VM_V5 = 0x003148128400ull;

__device__ __forceinline__ constexpr int vm_t1(int ti) { return (int)((VM_T1 >> (3 * ti)) & 7u); }
__device__ __forceinline__ constexpr int vm_t2(int ti) { return (int)((VM_T2 >> (3 * ti)) & 7u); }

__device__ __forceinline__ uint32_t vm_case(uint32_t pos, int ti) {
  return (pos & 1u) | ((pos >> vm_t1(ti)) & 1u) << 1 | ((pos >> vm_t2(ti)) & 1u) << 2 | ((pos >> 7) & 1u) << 3;
}

__device__ __forceinline__ size_t vm_corner(const VolArgs& V, int c) {
  return (size_t)(c & 1) + (size_t)((c >> 1) & 1) * (size_t)V.nx + (size_t)((c >> 2) & 1) * ((size_t)V.nx * V.ny);
}

__device__ __forceinline__ void vm_coords(const VolArgs& V, size_t p, int* i, int* j, int* k) {
  const size_t slice = (size_t)V.nx * V.ny;
  *k = (int)(p / slice);
  const int rem = (int)(p - (size_t)*k * slice);
  *j = rem / V.nx;
  *i = rem - *j * V.nx;
}

/* lanes below this one that have the bit set in `b` */
__device__ __forceinline__ uint32_t vm_below(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

/* the sum over the wave of a per-lane value of `bits` bits, and the sum over the lanes below */
template <int BITS>
__device__ __forceinline__ uint32_t vm_wave_sum(uint32_t v, uint32_t* below) {
  uint32_t total = 0, lo = 0;
#pragma unroll
  for (int b = 0; b < BITS; b++) {
    const unsigned long long m = __ballot((v >> b) & 1u);
    total += (uint32_t)__popcll(m) << b;
    lo += vm_below(m) << b;
  }
  *below = lo;
  return total;
}

__global__ __launch_bounds__(VM_BLOCK) void k_vmesh_cells(VolArgs V, int min_weight, size_t n_vox, uint32_t n_tiles,
                                                          uint8_t* __restrict__ cell, uint32_t* __restrict__ tri_counts,
                                                          unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_tri[VM_WAVES], s_act[VM_WAVES];
  const size_t p = (size_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  uint32_t nt = 0;
  bool act = false;
  if (p < n_vox) {
    int i, j, k;
    vm_coords(V, p, &i, &j, &k);
    if (i + 1 < V.nx && j + 1 < V.ny && k + 1 < V.nz) {
      uint32_t pos = 0;
      act = true;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const VolVoxel r = V.vox[p + vm_corner(V, c)];
        const double d = (double)r.d;
        act = act && r.w >= min_weight && ppf_fabs(d) < 1.0;
        pos |= (d > 0.0 ? 1u : 0u) << c;
      }
      if (act) {
#pragma unroll
        for (int ti = 0; ti < 6; ti++) nt += (VM_COUNT >> (2 * vm_case(pos, ti))) & 3u;
      }
    }
    cell[p] = act ? (uint8_t)(0x80u | nt) : (uint8_t)0;
  }
  uint32_t below;
  const uint32_t wt = vm_wave_sum<4>(nt, &below);
  const uint32_t wa = (uint32_t)__popcll(__ballot(act));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    s_tri[wv] = wt;
    s_act[wv] = wa;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0, a = 0;
#pragma unroll
    for (int w = 0; w < VM_WAVES; w++) {
      t += s_tri[w];
      a += s_act[w];
    }
    tri_counts[blockIdx.x] = t;
    if (blockIdx.x == 0) tri_counts[n_tiles] = 0; /* the trailing element the scan turns into the total */
    if (a) atomicAdd(&counters[VM_N_CELLS], (unsigned long long)a);
    if (t) atomicAdd(&counters[VM_N_TRIANGLES], (unsigned long long)t);
  }
}

/* the cubes that contain the edge of direction D from a voxel, as bits over the voxel's corner number in the cube */
__device__ __forceinline__ constexpr uint32_t vm_cubes_of(int D) {
  uint32_t m = 0;
  for (int off = 0; off < 8; off++)
    if (!(off & D)) m |= 1u << off;
  return m;
}

__global__ __launch_bounds__(VM_BLOCK) void k_vmesh_edges(VolArgs V, size_t n_vox, uint32_t n_tiles, const uint8_t* __restrict__ cell,
                                                          uint8_t* __restrict__ mask, uint16_t* __restrict__ rank,
                                                          uint32_t* __restrict__ vert_counts, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_n[VM_WAVES];
  const size_t p = (size_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  uint32_t m = 0;
  if (p < n_vox) {
    int i, j, k;
    vm_coords(V, p, &i, &j, &k);
    uint32_t act = 0; /* bit off: the cube in which this voxel is corner `off` is active */
#pragma unroll
    for (int off = 0; off < 8; off++)
      if (i >= (off & 1) && j >= ((off >> 1) & 1) && k >= ((off >> 2) & 1)) act |= (uint32_t)(cell[p - vm_corner(V, off)] >> 7) << off;
    if (act) {
      const bool p0 = (double)V.vox[p].d > 0.0;
#pragma unroll
      for (int e = 0; e < 7; e++)
        if (act & vm_cubes_of(e + 1)) { /* an active cube holds both ends: the other end is inside the volume */
          const bool p1 = (double)V.vox[p + vm_corner(V, e + 1)].d > 0.0;
          if (p0 != p1) m |= 1u << e;
        }
    }
    mask[p] = (uint8_t)m;
  }
  uint32_t r = 0, total = 0;
#pragma unroll
  for (int e = 0; e < 7; e++) {
    const unsigned long long b = __ballot((m >> e) & 1u);
    total += (uint32_t)__popcll(b);
    r += vm_below(b);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_n[wv] = total;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < VM_WAVES; w++)
    if (w < wv) r += s_n[w];
  if (p < n_vox) rank[p] = (uint16_t)r; /* at most 7 * 255 */
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < VM_WAVES; w++) t += s_n[w];
    vert_counts[blockIdx.x] = t;
    if (blockIdx.x == 0) vert_counts[n_tiles] = 0;
    if (t) atomicAdd(&counters[VM_N_VERTICES], (unsigned long long)t);
  }
}

__global__ __launch_bounds__(VM_BLOCK) void k_vmesh_vertices(VolArgs V, int min_weight, size_t n_vox, const uint8_t* __restrict__ mask,
                                                             const uint16_t* __restrict__ rank, const uint32_t* __restrict__ vert_off,
                                                             uint32_t n_vertices, float* __restrict__ rows,
                                                             unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_n[VM_WAVES];
  const size_t p = (size_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  uint32_t bad = 0;
  const uint32_t m = p < n_vox ? mask[p] : 0u;
  if (m) {
    int i, j, k;
    vm_coords(V, p, &i, &j, &k);
    uint32_t o = vert_off[blockIdx.x] + rank[p];
    const double d0 = (double)V.vox[p].d;
    const double c0 = V.o[0] + (double)i * V.voxel, c1 = V.o[1] + (double)j * V.voxel, c2 = V.o[2] + (double)k * V.voxel;
    double ga[3] = {0.0, 0.0, 0.0};
    const bool oka = volume_gradient(V, min_weight, i, j, k, ga);
    for (int e = 0; e < 7; e++) {
      if (!((m >> e) & 1u)) continue;
      const int D = e + 1, dx = D & 1, dy = (D >> 1) & 1, dz = (D >> 2) & 1;
      const double d1 = (double)V.vox[p + vm_corner(V, D)].d;
      const double t = d0 / (d0 - d1);
      const double mv = t * V.voxel;
      double gb[3] = {0.0, 0.0, 0.0};
      const bool okb = volume_gradient(V, min_weight, i + dx, j + dy, k + dz, gb);
      const double g0 = ga[0] + t * (gb[0] - ga[0]), g1 = ga[1] + t * (gb[1] - ga[1]), g2 = ga[2] + t * (gb[2] - ga[2]);
      const double len = ppf_sqrt((g0 * g0 + g1 * g1) + g2 * g2);
      const bool ok = oka && okb && len > 0.0;
      if (!ok) bad++;
      if (o < n_vertices) { /* always true while the volume is what k_vmesh_edges saw: a store never leaves the buffer */
        float* dst = rows + (size_t)o * 6;
        dst[0] = (float)(dx ? c0 + mv : c0);
        dst[1] = (float)(dy ? c1 + mv : c1);
        dst[2] = (float)(dz ? c2 + mv : c2);
        dst[3] = ok ? (float)(g0 / len) : 0.f;
        dst[4] = ok ? (float)(g1 / len) : 0.f;
        dst[5] = ok ? (float)(g2 / len) : 0.f;
      }
      o++;
    }
  }
  uint32_t below;
  const uint32_t wb = vm_wave_sum<3>(bad, &below);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_n[wv] = wb;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < VM_WAVES; w++) t += s_n[w];
    if (t) atomicAdd(&counters[VM_N_NO_NORMAL], (unsigned long long)t);
  }
}

/* one of six values by a number 0..5 that differs from lane to lane: selects, not an indexed array */
__device__ __forceinline__ uint32_t vm_pick(uint32_t q, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, uint32_t a5) {
  const uint32_t lo = q == 0 ? a0 : (q == 1 ? a1 : a2), hi = q == 3 ? a3 : (q == 4 ? a4 : a5);
  return q < 3 ? lo : hi;
}

__global__ __launch_bounds__(VM_BLOCK) void k_vmesh_triangles(VolArgs V, size_t n_vox, const uint8_t* __restrict__ cell,
                                                              const uint8_t* __restrict__ mask, const uint16_t* __restrict__ rank,
                                                              const uint32_t* __restrict__ vert_off, const uint32_t* __restrict__ tri_off,
                                                              uint32_t n_triangles, int32_t* __restrict__ tris) {
  __shared__ uint32_t s_n[VM_WAVES];
  const size_t p = (size_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  const uint32_t nt = p < n_vox ? (uint32_t)(cell[p] & 15u) : 0u;
  uint32_t below;
  const uint32_t wt = vm_wave_sum<4>(nt, &below);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_n[wv] = wt;
  __syncthreads();
  if (!nt) return; /* no barrier below */
  uint32_t o = tri_off[blockIdx.x] + below;
#pragma unroll
  for (int w = 0; w < VM_WAVES; w++)
    if (w < wv) o += s_n[w];
  /* the cube is active: its eight corners are inside the volume */
  uint32_t pos = 0, vb[7], mk[7];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const size_t q = p + vm_corner(V, c);
    pos |= ((double)V.vox[q].d > 0.0 ? 1u : 0u) << c;
    if (c < 7) { /* corner 7 owns no edge of this cube */
      vb[c] = vert_off[q / VM_BLOCK] + rank[q];
      mk[c] = mask[q];
    }
  }
#pragma unroll
  for (int ti = 0; ti < 6; ti++) {
    const int t1 = vm_t1(ti), t2 = vm_t2(ti);
    const uint32_t cs = vm_case(pos, ti);
    const uint32_t n = (VM_COUNT >> (2 * cs)) & 3u;
    if (!n) continue;
    /* the vertex on each local edge (0,1) (0,2) (0,3) (1,2) (1,3) (2,3): owner and type are constants here */
    const uint32_t e0 = vb[0] + __popc(mk[0] & ((1u << (t1 - 1)) - 1u));
    const uint32_t e1 = vb[0] + __popc(mk[0] & ((1u << (t2 - 1)) - 1u));
    const uint32_t e2 = vb[0] + __popc(mk[0] & ((1u << 6) - 1u));
    const uint32_t e3 = vb[t1] + __popc(mk[t1] & ((1u << ((t1 ^ t2) - 1)) - 1u));
    const uint32_t e4 = vb[t1] + __popc(mk[t1] & ((1u << ((t1 ^ 7) - 1)) - 1u));
    const uint32_t e5 = vb[t2] + __popc(mk[t2] & ((1u << ((t2 ^ 7) - 1)) - 1u));
    const bool odd = (VM_PARITY >> ti) & 1u;
    const uint32_t sh = 3 * cs;
    {
      const uint32_t a = (uint32_t)(VM_V0 >> sh) & 7u, b = (uint32_t)(VM_V1 >> sh) & 7u, c = (uint32_t)(VM_V2 >> sh) & 7u;
      if (o < n_triangles) { /* always true while the volume is what k_vmesh_cells saw: a store never leaves the buffer */
        int32_t* dst = tris + (size_t)o * 3;
        dst[0] = (int32_t)vm_pick(a, e0, e1, e2, e3, e4, e5);
        dst[1] = (int32_t)vm_pick(odd ? c : b, e0, e1, e2, e3, e4, e5);
        dst[2] = (int32_t)vm_pick(odd ? b : c, e0, e1, e2, e3, e4, e5);
      }
      o++;
    }
    if (n == 2) {
      const uint32_t a = (uint32_t)(VM_V3 >> sh) & 7u, b = (uint32_t)(VM_V4 >> sh) & 7u, c = (uint32_t)(VM_V5 >> sh) & 7u;
      if (o < n_triangles) {
        int32_t* dst = tris + (size_t)o * 3;
        dst[0] = (int32_t)vm_pick(a, e0, e1, e2, e3, e4, e5);
        dst[1] = (int32_t)vm_pick(odd ? c : b, e0, e1, e2, e3, e4, e5);
        dst[2] = (int32_t)vm_pick(odd ? b : c, e0, e1, e2, e3, e4, e5);
      }
      o++;
    }
  }
}

#endif /* PPF_VOLUME_MESH_KERNELS_H */
