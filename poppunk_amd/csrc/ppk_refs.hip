// Reference genomes of a cluster network ([EXT]): PopPUNK/network.py:283-487 (extractReferences) as a
// deterministic rule -- greedy lowest-index clique pruning per component (or fastPrune's rank test), then a repair
// that joins the references of a component along breadth-first parent paths from its lowest reference.
//
// Integer arithmetic only; the same edges in any order give the same bits.  Stages (ppk_prof_stages names):
//   validate     ids in range, no self-loop: the first offender.  The components and the layout are enqueued behind it
//                (the union-find skips an offending edge), so that the call's ONE synchronisation reads the first
//                offender, the bit-matrix words, the largest component and the component count together.
//   layout       lock-free union-find (ppk_device.h); a root is its component's smallest vertex.  Vertices sorted by
//                (root, index): the position within the component is the LOCAL index, which keeps the index order.
//                Every component of 3 or more vertices gets a |V| x ceil(|V| / 64) bit matrix in SLOT_REFS_BITS,
//                filled with atomicOr (both directions of every edge; a repeated edge sets the same bits).
//   prune_small  3 <= |V| <= 64: one wave per component, lane l holds row l; R, C, min and the reference test are
//                ballot / ctz / readlane work on wave-uniform 64-bit masks.  No LDS, no barrier.
//   prune_large  |V| > 64: one workgroup per component.  R, C and the reference flags are bitsets in LDS up to option
//                refs_lds_bits vertices, in global scratch beyond.  Within one clique v only increases, every lower
//                bit of C is already clear and N(v) never holds v: a pass for v touches the words from v's on, ANDs,
//                and reports the lowest vertex left in C with one LDS atomicMin -- one barrier per vertex taken.
//                (Also: |V| <= 2, the lowest vertex unconditionally; fast mode, a rank test on the layout.)
//   repair       union-find over the reference-reference edges; a reference outside the set of its component's
//                lowest reference r0 is a stray.  One workgroup per component with a stray: pull-style BFS from r0 on
//                the bit rows (an unvisited vertex takes the lowest set bit of row & frontier as its parent: |V|^2 / 64
//                words a level, as many levels as r0's eccentricity), then one lane per stray walks the parents.
//   compact      flags to ranks and reference-reference edges to positions (rocPRIM scans); the ordered write.
// A row-compressed adjacency for components whose bit matrix passes option refs_scratch_mb is NOT built: the call
// fails with PPK_ERR_CAPACITY and names the component's size.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <string>

#include "ppk_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsWords = 1024;            // 65 536 vertices: the most a component's bitsets take of LDS (8 KiB each)
constexpr unsigned kInf = 0xffffffffu;

// control words (u64): the first four are read back
enum { C_BAD = 0, C_WORDS, C_MAXSIZE, C_NCOMP, C_CLIQUES, C_PICK_A, C_PICK_B, C_EXISTING, C_REPAIRED, C_WORDS_N = 16 };

__device__ __forceinline__ bool edge_ok(long long i, long long j, long long n) {
  return i >= 0 && i < n && j >= 0 && j < n && i != j;
}
__device__ __forceinline__ size_t words_of(int sz) { return ((size_t)sz + 63) >> 6; }
__device__ __forceinline__ u64 bit_of(int l) { return 1ull << (l & 63); }

#define REFS_GRID_LOOP(var, count) \
  for (size_t var = (size_t)blockIdx.x * blockDim.x + threadIdx.x; var < (count); var += (size_t)gridDim.x * blockDim.x)

// ---- validate, components --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) refs_validate_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                 size_t m, long long n, u64 *bad) {
  REFS_GRID_LOOP(k, m)
    if (!edge_ok(ei[k * stride], ej[k * stride], n)) atomicMin(bad, (u64)k);
}
__global__ void __launch_bounds__(kThreads) refs_iota_kernel(int *parent, size_t n) {
  REFS_GRID_LOOP(v, n) parent[v] = (int)v;
}
// links the ends of every valid edge; with `flag`, only where both ends are references
__global__ void __launch_bounds__(kThreads) refs_union_kernel(const long long *ei, const long long *ej, size_t stride,
                                                              size_t m, long long n, const uint8_t *flag, int *parent) {
  REFS_GRID_LOOP(k, m) {
    const long long i = ei[k * stride], j = ej[k * stride];
    if (!edge_ok(i, j, n)) continue;
    if (flag && !(flag[i] && flag[j])) continue;
    uf_union(parent, (int)i, (int)j);
  }
}
__global__ void __launch_bounds__(kThreads) refs_roots_kernel(const int *parent, size_t n, int *root, int *size) {
  REFS_GRID_LOOP(v, n) {
    const int r = uf_find_ro(parent, (int)v);
    root[v] = r;
    atomicAdd(&size[r], 1);
  }
}
// the sort key of every vertex, the root flags, the matrix words of every component (at its root) and the totals
__global__ void __launch_bounds__(kThreads) refs_keys_kernel(const int *root, const int *size, size_t n, u64 *keys,
                                                             int *is_root, u64 *wneed, u64 *ctl) {
  REFS_GRID_LOOP(v, n) {
    const int r = root[v];
    keys[v] = (u64)(unsigned)r << 32 | (u64)v;
    const bool mine = r == (int)v;
    is_root[v] = mine;
    u64 w = 0;
    if (mine) {
      const int sz = size[v];
      if (sz >= 3) w = (u64)sz * words_of(sz);
      atomicAdd(&ctl[C_WORDS], w);
      atomicMax(&ctl[C_MAXSIZE], (u64)sz);
      atomicAdd(&ctl[C_NCOMP], 1ull);
    }
    wneed[v] = w;
  }
}
__global__ void __launch_bounds__(kThreads) refs_starts_kernel(const u64 *sorted, size_t n, const int *crank, int *order,
                                                               int *cstart, int *comp_root) {
  REFS_GRID_LOOP(p, n) {
    const int v = (int)(sorted[p] & 0xffffffffu), r = (int)(sorted[p] >> 32);
    order[p] = v;
    if (v == r) {
      cstart[r] = (int)p;
      comp_root[crank[r]] = r;
    }
  }
}
__global__ void __launch_bounds__(kThreads) refs_local_kernel(const int *order, const int *root, const int *cstart,
                                                              size_t n, int *local) {
  REFS_GRID_LOOP(p, n) {
    const int v = order[p];
    local[v] = (int)p - cstart[root[v]];
  }
}
__global__ void __launch_bounds__(kThreads) refs_bits_kernel(const long long *ei, const long long *ej, size_t stride,
                                                             size_t m, const int *root, const int *size, const int *local,
                                                             const u64 *woff, u64 *bits) {
  REFS_GRID_LOOP(k, m) {
    const int i = (int)ei[k * stride], j = (int)ej[k * stride];
    const int r = root[i], sz = size[r];
    if (sz < 3) continue;
    const size_t W = words_of(sz);
    u64 *rows = bits + woff[r];
    const int li = local[i], lj = local[j];
    atomicOr(&rows[(size_t)li * W + (lj >> 6)], bit_of(lj));
    atomicOr(&rows[(size_t)lj * W + (li >> 6)], bit_of(li));
  }
}

// ---- flags -------------------------------------------------------------------------------------------------------
// is_ref = existing (as 0 / 1); their count; fast mode: which components hold one
__global__ void __launch_bounds__(kThreads) refs_flags_kernel(const uint8_t *existing, size_t n, const int *root,
                                                              uint8_t *is_ref, int *has_ref, u64 *ctl) {
  u64 mine = 0;
  REFS_GRID_LOOP(v, n) {
    const bool f = existing && existing[v];
    is_ref[v] = f;
    if (f) {
      ++mine;
      if (has_ref) has_ref[root[v]] = 1;
    }
  }
  mine = wave_sum_all(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&ctl[C_EXISTING], mine);
}
// |V| <= 2: the lowest vertex, whatever else the component holds (network.py:215-216)
__global__ void __launch_bounds__(kThreads) refs_tiny_kernel(const int *root, const int *size, size_t n, uint8_t *is_ref,
                                                             u64 *ctl) {
  u64 mine = 0;
  REFS_GRID_LOOP(v, n)
    if (root[v] == (int)v && size[v] <= 2 && !is_ref[v]) {
      is_ref[v] = 1;
      ++mine;
    }
  mine = wave_sum_all(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&ctl[C_PICK_B], mine);
}

// ---- clique pruning, 3 <= |V| <= 64 ------------------------------------------------------------------------------
__device__ __forceinline__ u64 row_of_lane(u64 row, int l) {
  const int s = __builtin_amdgcn_readfirstlane(l);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)row, s);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(row >> 32), s);
  return (u64)hi << 32 | lo;
}
__global__ void __launch_bounds__(kThreads) refs_prune_small_kernel(const int *comp_root, unsigned n_comp, const int *size,
                                                                    const int *cstart, const u64 *woff, const int *order,
                                                                    const u64 *bits, uint8_t *is_ref, u64 *ctl) {
  const int lane = threadIdx.x & 63;
  const unsigned wave = blockIdx.x * kWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kWaves;
  u64 cliques = 0, picks = 0;
  for (unsigned c = wave; c < n_comp; c += n_waves) {
    const int r = comp_root[c], sz = size[r];
    if (sz < 3 || sz > 64) continue;                 // (wave-uniform)
    const int v = lane < sz ? order[cstart[r] + lane] : -1;
    const u64 row = lane < sz ? bits[woff[r] + lane] : 0ull;      // one word a row
    const u64 had = __ballot(v >= 0 && is_ref[v]);
    u64 ref = had, R = sz == 64 ? ~0ull : (1ull << sz) - 1;
    while (R) {
      const int s = __builtin_ctzll(R);
      u64 K = 1ull << s, C = row_of_lane(row, s) & R;
      while (C) {
        const int x = __builtin_ctzll(C);
        K |= 1ull << x;
        C &= row_of_lane(row, x);
      }
      if (!(K & ref)) {
        ref |= 1ull << s;
        ++picks;
      }
      R &= ~K;
      ++cliques;
    }
    if (v >= 0 && (((ref & ~had) >> lane) & 1)) is_ref[v] = 1;
  }
  if (lane == 0) {
    if (cliques) atomicAdd(&ctl[C_CLIQUES], cliques);
    if (picks) atomicAdd(&ctl[C_PICK_A], picks);
  }
}

// ---- clique pruning, |V| > 64 ------------------------------------------------------------------------------------
// R, C, REF: W words each, LDS or global.  slot: three LDS words, all kInf on entry; step k reports through slot k % 3
// and clears slot (k + 1) % 3, whose last reader passed barrier k - 1 to get here.  A step publishes the VERTEX it
// found (64 w + ctz), not the word: after the barrier every thread takes s or v from the slot alone and none reads a
// word of R or C that the next pass's owner may already be rewriting.  The thread that owns v's word in the pass for v
// takes v out of R; within a pass a word of R or C is read and written by its owner only.
__device__ void refs_prune_large(int sz, const u64 *rows, const int *ord, uint8_t *is_ref, u64 *R, u64 *C, u64 *REF,
                                 unsigned *slot, u64 &cliques, u64 &picks) {
  const int tid = threadIdx.x;
  const size_t W = words_of(sz);
  for (size_t w = tid; w < W; w += kThreads) {
    const long long left = (long long)sz - (long long)(w * 64);
    const int nb = left >= 64 ? 64 : (int)left;
    R[w] = nb == 64 ? ~0ull : (1ull << nb) - 1;
    u64 f = 0;
    for (int b = 0; b < nb; ++b) f |= (u64)(is_ref[ord[w * 64 + b]] != 0) << b;
    REF[w] = f;
  }
  if (tid < 3) slot[tid] = kInf;
  __syncthreads();
  unsigned step = 0;
  size_t rcur = 0;
  while (true) {
    unsigned *mine = slot + step % 3;
    if (tid == 0) slot[(step + 1) % 3] = kInf;
    for (size_t w = rcur + tid; w < W; w += kThreads)
      if (const u64 r = R[w]) {
        atomicMin(mine, (unsigned)(w * 64) + (unsigned)__builtin_ctzll(r));
        break;
      }
    __syncthreads();
    ++step;
    unsigned found = *mine;
    if (found == kInf) break;                        // R is empty (uniform)
    const int s = (int)found;
    rcur = found >> 6;
    bool has_ref = (REF[s >> 6] >> (s & 63)) & 1;
    int v = s;
    bool first = true;
    while (true) {
      mine = slot + step % 3;
      if (tid == 0) slot[(step + 1) % 3] = kInf;
      const u64 *row = rows + (size_t)v * W;
      const size_t cw = (size_t)v >> 6;
      bool sent = false;
      for (size_t w = cw + tid; w < W; w += kThreads) {
        u64 c;
        if (first) {
          u64 r = R[w];
          if (w == cw) {
            r &= ~bit_of(v);
            R[w] = r;
          }
          c = row[w] & r;
        } else {
          if (w == cw) R[w] &= ~bit_of(v);
          c = C[w] & row[w];
        }
        C[w] = c;
        if (c && !sent) {
          atomicMin(mine, (unsigned)(w * 64) + (unsigned)__builtin_ctzll(c));
          sent = true;
        }
      }
      __syncthreads();
      ++step;
      found = *mine;
      if (found == kInf) break;                      // C is empty: the clique is maximal in G[R] (uniform)
      v = (int)found;
      has_ref = has_ref || ((REF[v >> 6] >> (v & 63)) & 1);
      first = false;
    }
    ++cliques;
    if (!has_ref) {
      ++picks;
      if (tid == 0) {
        REF[s >> 6] |= bit_of(s);
        is_ref[ord[s]] = 1;
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) refs_prune_large_kernel(const int *comp_root, unsigned n_comp, const int *size,
                                                                    const int *cstart, const u64 *woff, const int *order,
                                                                    const u64 *bits, u64 *aux, int lds_bits,
                                                                    uint8_t *is_ref, u64 *ctl) {
  __shared__ u64 sR[kLdsWords], sC[kLdsWords], sF[kLdsWords];
  __shared__ unsigned slot[3];
  u64 cliques = 0, picks = 0;
  for (unsigned c = blockIdx.x; c < n_comp; c += gridDim.x) {
    const int r = comp_root[c], sz = size[r];
    if (sz <= 64) continue;                          // (uniform)
    const int p0 = cstart[r];
    if (sz <= lds_bits) {
      refs_prune_large(sz, bits + woff[r], order + p0, is_ref, sR, sC, sF, slot, cliques, picks);
    } else {
      const size_t W = words_of(sz);
      u64 *a = aux + 4 * ((size_t)(p0 >> 6) + c);    // disjoint: the next component's offset is at least W further on, times 4
      refs_prune_large(sz, bits + woff[r], order + p0, is_ref, a, a + W, a + 2 * W, slot, cliques, picks);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (cliques) atomicAdd(&ctl[C_CLIQUES], cliques);
    if (picks) atomicAdd(&ctl[C_PICK_A], picks);
  }
}

// ---- fast mode (network.py:222-261) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) refs_merged_flags_kernel(const int *order, const uint8_t *merged, size_t n,
                                                                     int *mflag) {
  REFS_GRID_LOOP(p, n + 1) mflag[p] = p < n && merged && merged[order[p]];
}
// position p of the layout: |V| / 10 + 1 lowest vertices where the component holds no reference, and the m / 3 + 1
// lowest of its m merged queries (mscan: the exclusive prefix of the merged flags, n + 1 entries)
__global__ void __launch_bounds__(kThreads) refs_fast_kernel(const int *order, const int *root, const int *size,
                                                             const int *cstart, const int *has_ref, const int *mscan,
                                                             const uint8_t *merged, size_t n, uint8_t *is_ref, u64 *ctl) {
  u64 a = 0, b = 0;
  REFS_GRID_LOOP(p, n) {
    const int v = order[p], r = root[v], sz = size[r], p0 = cstart[r];
    const int li = (int)p - p0;
    bool pick = false;
    if (!has_ref[r] && li < sz / 10 + 1) {
      pick = true;
      ++a;
    }
    if (!pick && merged && merged[v]) {
      const int mm = mscan[p0 + sz] - mscan[p0], mr = mscan[p] - mscan[p0];
      if (mr < mm / 3 + 1 && !is_ref[v]) {
        pick = true;
        ++b;
      }
    }
    if (pick) is_ref[v] = 1;
  }
  a = wave_sum_all(a);
  b = wave_sum_all(b);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&ctl[C_PICK_A], a);
    if (b) atomicAdd(&ctl[C_PICK_B], b);
  }
}

// ---- repair --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) refs_lowest_kernel(const uint8_t *is_ref, const int *root, size_t n,
                                                               unsigned *r0) {
  REFS_GRID_LOOP(v, n)
    if (is_ref[v]) atomicMin(&r0[root[v]], (unsigned)v);
}
// a reference outside its component's r0 set (a set's root is its smallest vertex, so r0 is its own root)
__global__ void __launch_bounds__(kThreads) refs_stray_kernel(const uint8_t *is_ref, const int *root, const int *parent2,
                                                              const unsigned *r0, size_t n, int *needs, u64 *ctl) {
  REFS_GRID_LOOP(v, n)
    if (is_ref[v]) {
      const int r = root[v];
      if (uf_find_ro(parent2, (int)v) != (int)r0[r] && atomicCAS(&needs[r], 0, 1) == 0) atomicAdd(&ctl[C_REPAIRED], 1ull);
    }
}
// VIS, FR, NX, ST: W words each
__device__ void refs_repair_bfs(int sz, const u64 *rows, const int *ord, const int *local, uint8_t *is_ref,
                                const int *parent2, int r0v, int *bpar, u64 *VIS, u64 *FR, u64 *NX, u64 *ST,
                                unsigned *any) {
  const int tid = threadIdx.x;
  const size_t W = words_of(sz);
  const int r0l = local[r0v];
  for (size_t w = tid; w < W; w += kThreads) {
    const u64 x = w == (size_t)(r0l >> 6) ? bit_of(r0l) : 0ull;
    VIS[w] = x;
    FR[w] = x;
    NX[w] = 0;
    ST[w] = 0;
  }
  if (tid == 0) *any = 0;
  __syncthreads();
  for (int l = tid; l < sz; l += kThreads) {
    const int v = ord[l];
    if (is_ref[v] && uf_find_ro(parent2, v) != r0v) atomicOr(&ST[l >> 6], bit_of(l));
  }
  while (true) {
    bool found = false;
    for (int l = tid; l < sz; l += kThreads) {
      if ((VIS[l >> 6] >> (l & 63)) & 1) continue;
      const u64 *row = rows + (size_t)l * W;
      for (size_t w = 0; w < W; ++w) {
        const u64 x = row[w] & FR[w];
        if (x) {
          bpar[l] = (int)(w * 64) + __builtin_ctzll(x);      // the lowest neighbour of the level before
          atomicOr(&NX[l >> 6], bit_of(l));
          found = true;
          break;
        }
      }
    }
    if (found) *any = 1;
    __syncthreads();
    const bool go = *any != 0;
    __syncthreads();
    if (!go) break;                                  // (uniform)
    if (tid == 0) *any = 0;
    for (size_t w = tid; w < W; w += kThreads) {
      const u64 x = NX[w];
      FR[w] = x;
      VIS[w] |= x;
      NX[w] = 0;
    }
    __syncthreads();
  }
  // (the barriers above also stand between the strays' atomicOr and these reads)
  for (int l = tid; l < sz; l += kThreads)
    if ((ST[l >> 6] >> (l & 63)) & 1)
      for (int p = l; p != r0l;) {
        p = bpar[p];
        is_ref[ord[p]] = 1;
      }
}
__global__ void __launch_bounds__(kThreads) refs_repair_kernel(const int *comp_root, unsigned n_comp, const int *size,
                                                               const int *cstart, const u64 *woff, const int *order,
                                                               const int *local, const u64 *bits, u64 *aux, int lds_bits,
                                                               const int *needs, const unsigned *r0, const int *parent2,
                                                               int *bpar, uint8_t *is_ref) {
  __shared__ u64 sV[kLdsWords], sF[kLdsWords], sN[kLdsWords], sS[kLdsWords];
  __shared__ unsigned any;
  for (unsigned c = blockIdx.x; c < n_comp; c += gridDim.x) {
    const int r = comp_root[c];
    if (!needs[r]) continue;                         // (uniform; a component that needs repair has 3 or more vertices)
    const int sz = size[r], p0 = cstart[r];
    if (sz <= lds_bits) {
      refs_repair_bfs(sz, bits + woff[r], order + p0, local, is_ref, parent2, (int)r0[r], bpar + p0, sV, sF, sN, sS, &any);
    } else {
      const size_t W = words_of(sz);
      u64 *a = aux + 4 * ((size_t)(p0 >> 6) + c);
      refs_repair_bfs(sz, bits + woff[r], order + p0, local, is_ref, parent2, (int)r0[r], bpar + p0, a, a + W, a + 2 * W,
                      a + 3 * W, &any);
    }
    __syncthreads();
  }
}

// ---- compact -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) refs_rank_flags_kernel(const uint8_t *is_ref, size_t n, int *flag) {
  REFS_GRID_LOOP(v, n) flag[v] = is_ref[v] != 0;
}
__global__ void __launch_bounds__(kThreads) refs_edge_flags_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                   size_t m, const uint8_t *is_ref, int *flag) {
  REFS_GRID_LOOP(k, m) flag[k] = is_ref[ei[k * stride]] && is_ref[ej[k * stride]];
}
__global__ void __launch_bounds__(kThreads) refs_edge_write_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                   size_t m, const int *flag, const int *pos,
                                                                   const int *rank, long long *out) {
  REFS_GRID_LOOP(k, m)
    if (flag[k]) {
      out[2 * (size_t)pos[k]] = rank[ei[k * stride]];
      out[2 * (size_t)pos[k] + 1] = rank[ej[k * stride]];
    }
}
// counts: references, reference edges, components, cliques removed, picks A, picks B, added by repair, components repaired
__global__ void refs_counts_kernel(const u64 *ctl, const int *vflag, const int *rank, size_t n, const int *eflag,
                                   const int *epos, size_t m, long long *counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long refs = n ? rank[n - 1] + vflag[n - 1] : 0;
  counts[0] = refs;
  counts[1] = m ? epos[m - 1] + eflag[m - 1] : 0;
  counts[2] = (long long)ctl[C_NCOMP];
  counts[3] = (long long)ctl[C_CLIQUES];
  counts[4] = (long long)ctl[C_PICK_A];
  counts[5] = (long long)ctl[C_PICK_B];
  counts[6] = refs - (long long)(ctl[C_EXISTING] + ctl[C_PICK_A] + ctl[C_PICK_B]);
  counts[7] = (long long)ctl[C_REPAIRED];
}

const char *kWho = "ppk_pick_refs";

int check_sizes(const std::string &who, size_t n_edges, size_t n_vertices) {
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_vertices must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_pick_refs_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges,
                                 size_t n_vertices, const uint8_t *d_existing, const uint8_t *d_merged, int fast,
                                 uint8_t *d_is_ref, long long *d_ref_edges, long long *d_counts, void *stream) {
  const std::string who = kWho;
  int rc = check_sizes(who, n_edges, n_vertices);
  if (rc != PPK_OK) return rc;
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, who + ": stride must be 1 or 2");
  if (fast != 0 && fast != 1) return ppk_fail(PPK_ERR_ARG, who + ": fast must be 0 or 1");
  if (!d_counts || (!d_is_ref && n_vertices) || (n_edges && (!d_i || !d_j))) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const long long cap_mb = ppk_config().refs_scratch_mb.load();
  long long lds_bits = ppk_config().refs_lds_bits.load();
  if (cap_mb < 1) return ppk_fail(PPK_ERR_ARG, who + ": option refs_scratch_mb must be at least 1");
  if (lds_bits < 64 || lds_bits > kLdsWords * 64)
    return ppk_fail(PPK_ERR_ARG, who + ": option refs_lds_bits must be 64 .. " + std::to_string(kLdsWords * 64));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n_edges, n = n_vertices;
  if (n == 0) {                          // (and so m == 0, or the first edge is the offender)
    if (m) return ppk_fail(PPK_ERR_ARG, who + ": edge 0: vertex id out of range [0, 0)");
    PPK_HIP(hipMemsetAsync(d_counts, 0, 64, s));
    return PPK_OK;
  }

  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < n) ++bits;
  const unsigned end_bit = 32 + bits;
  size_t sort_tmp = 0, scan_i = 0, scan_w = 0, scan_m = 0;
  PPK_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp, (u64 *)nullptr, (u64 *)nullptr, n, 0u, end_bit, s));
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_i, (int *)nullptr, (int *)nullptr, 0, n + 1, rocprim::plus<int>(), s));
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_w, (u64 *)nullptr, (u64 *)nullptr, 0ull, n, rocprim::plus<u64>(), s));
  if (m) PPK_HIP(rocprim::exclusive_scan(nullptr, scan_m, (int *)nullptr, (int *)nullptr, 0, m, rocprim::plus<int>(), s));
  size_t tmp = sort_tmp;
  for (size_t t : {scan_i, scan_w, scan_m}) tmp = t > tmp ? t : tmp;

  u64 *ctl, *ka, *kb, *wneed, *woff;
  int *parent, *root, *size, *is_root, *crank, *order, *cstart, *comp_root, *local, *has_ref, *mflag, *mscan, *parent2,
      *needs, *bpar, *vflag, *rank, *eflag, *epos;
  unsigned *r0;
  char *d_tmp;
  rc = ppk_scratch_carve(dev, SLOT_REFS, [&](Carve &c) {
    c.take(ctl, C_WORDS_N).take(ka, n).take(kb, n).take(wneed, n).take(woff, n);
    c.take(parent, n).take(root, n).take(size, n).take(is_root, n).take(crank, n).take(order, n).take(cstart, n);
    c.take(comp_root, n).take(local, n).take(has_ref, n).take(mflag, n + 1).take(mscan, n + 1).take(parent2, n);
    c.take(needs, n).take(bpar, n).take(vflag, n).take(rank, n).take(eflag, m).take(epos, m).take(r0, n);
    c.take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;
  const dim3 blk(kThreads), gn(grid_for(n, kThreads * 4, 2048)), gm(grid_for(m, kThreads * 4, 2048));

  // -- validate; the components and the layout behind it; the one synchronisation
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(ctl, 0, C_WORDS_N * 8, s));
  PPK_HIP(hipMemsetAsync(ctl, 0xff, 8, s));
  if (m) hipLaunchKernelGGL(refs_validate_kernel, gm, blk, 0, s, d_i, d_j, stride, m, (long long)n, ctl + C_BAD);
  ppk_prof_stage("layout", s);
  hipLaunchKernelGGL(refs_iota_kernel, gn, blk, 0, s, parent, n);
  if (m)
    hipLaunchKernelGGL(refs_union_kernel, gm, blk, 0, s, d_i, d_j, stride, m, (long long)n, (const uint8_t *)nullptr,
                       parent);
  PPK_HIP(hipMemsetAsync(size, 0, n * 4, s));
  hipLaunchKernelGGL(refs_roots_kernel, gn, blk, 0, s, parent, n, root, size);
  hipLaunchKernelGGL(refs_keys_kernel, gn, blk, 0, s, root, size, n, ka, is_root, wneed, ctl);
  PPK_HIP(hipGetLastError());
  size_t tb = tmp;
  PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, ka, kb, n, 0u, end_bit, s));
  tb = tmp;
  PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, is_root, crank, 0, n, rocprim::plus<int>(), s));
  tb = tmp;
  PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, wneed, woff, 0ull, n, rocprim::plus<u64>(), s));
  hipLaunchKernelGGL(refs_starts_kernel, gn, blk, 0, s, kb, n, crank, order, cstart, comp_root);
  hipLaunchKernelGGL(refs_local_kernel, gn, blk, 0, s, order, root, cstart, n, local);
  PPK_HIP(hipGetLastError());
  const u64 *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{ctl, 32}}, &h)) != PPK_OK) return rc;
  if (h[C_BAD] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    const size_t k = (size_t)h[C_BAD];
    long long i = 0, j = 0, o = 0;
    if (!ppk_read_edge(d_i, d_j, stride, nullptr, k, &i, &j, &o))
      return ppk_fail(PPK_ERR_HIP, who + ": cannot read back the bad edge");
    const bool range = i < 0 || (size_t)i >= n || j < 0 || (size_t)j >= n;
    return ppk_fail(PPK_ERR_ARG, who + ": edge " + std::to_string(k) + " (i=" + std::to_string(i) + ", j=" +
                                     std::to_string(j) + "): " +
                                     (range ? "vertex id out of range [0, " + std::to_string(n) + ")" : std::string("self-loop")));
  }
  const size_t total_words = (size_t)h[C_WORDS], max_size = (size_t)h[C_MAXSIZE];
  const unsigned n_comp = (unsigned)h[C_NCOMP];
  if (total_words * 8 > (size_t)cap_mb << 20) {
    ppk_prof_stage(nullptr, s);
    return ppk_fail(PPK_ERR_CAPACITY, who + ": the largest component has " + std::to_string(max_size) +
                                          " vertices; the components' bit matrices take " +
                                          std::to_string((total_words * 8 + ((size_t)1 << 20) - 1) >> 20) +
                                          " MiB, over option refs_scratch_mb (" + std::to_string(cap_mb) +
                                          "); a row-compressed adjacency is not built");
  }
  u64 *bitsm, *aux;
  const size_t aux_words = 4 * (n / 64 + n_comp + 2);
  rc = ppk_scratch_carve(dev, SLOT_REFS_BITS, [&](Carve &c) { c.take(bitsm, total_words + 1).take(aux, aux_words); });
  if (rc != PPK_OK) return rc;
  if (total_words) PPK_HIP(hipMemsetAsync(bitsm, 0, total_words * 8, s));
  if (m && total_words)
    hipLaunchKernelGGL(refs_bits_kernel, gm, blk, 0, s, d_i, d_j, stride, m, root, size, local, woff, bitsm);
  if (fast) PPK_HIP(hipMemsetAsync(has_ref, 0, n * 4, s));
  hipLaunchKernelGGL(refs_flags_kernel, gn, blk, 0, s, d_existing, n, root, d_is_ref, fast ? has_ref : (int *)nullptr, ctl);
  PPK_HIP(hipGetLastError());

  const dim3 g_wave(grid_for(n_comp, kWaves, 4096)), g_block(grid_for(n_comp, 1, 2048));
  if (fast) {
    ppk_prof_stage("fast", s);
    hipLaunchKernelGGL(refs_merged_flags_kernel, gn, blk, 0, s, order, d_merged, n, mflag);
    tb = tmp;
    PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, mflag, mscan, 0, n + 1, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(refs_fast_kernel, gn, blk, 0, s, order, root, size, cstart, has_ref, mscan, d_merged, n, d_is_ref,
                       ctl);
  } else {
    ppk_prof_stage("prune_small", s);
    hipLaunchKernelGGL(refs_tiny_kernel, gn, blk, 0, s, root, size, n, d_is_ref, ctl);
    if (total_words)
      hipLaunchKernelGGL(refs_prune_small_kernel, g_wave, blk, 0, s, comp_root, n_comp, size, cstart, woff, order, bitsm,
                         d_is_ref, ctl);
    ppk_prof_stage("prune_large", s);
    if (max_size > 64)
      hipLaunchKernelGGL(refs_prune_large_kernel, g_block, blk, 0, s, comp_root, n_comp, size, cstart, woff, order, bitsm,
                         aux, (int)lds_bits, d_is_ref, ctl);
  }
  PPK_HIP(hipGetLastError());

  ppk_prof_stage("repair", s);
  if (m && max_size >= 3) {
    hipLaunchKernelGGL(refs_iota_kernel, gn, blk, 0, s, parent2, n);
    hipLaunchKernelGGL(refs_union_kernel, gm, blk, 0, s, d_i, d_j, stride, m, (long long)n, (const uint8_t *)d_is_ref,
                       parent2);
    PPK_HIP(hipMemsetAsync(r0, 0xff, n * 4, s));
    PPK_HIP(hipMemsetAsync(needs, 0, n * 4, s));
    hipLaunchKernelGGL(refs_lowest_kernel, gn, blk, 0, s, d_is_ref, root, n, r0);
    hipLaunchKernelGGL(refs_stray_kernel, gn, blk, 0, s, d_is_ref, root, parent2, r0, n, needs, ctl);
    hipLaunchKernelGGL(refs_repair_kernel, g_block, blk, 0, s, comp_root, n_comp, size, cstart, woff, order, local, bitsm,
                       aux, (int)lds_bits, needs, r0, parent2, bpar, d_is_ref);
    PPK_HIP(hipGetLastError());
  }

  ppk_prof_stage("compact", s);
  hipLaunchKernelGGL(refs_rank_flags_kernel, gn, blk, 0, s, d_is_ref, n, vflag);
  tb = tmp;
  PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, vflag, rank, 0, n, rocprim::plus<int>(), s));
  if (m) {
    hipLaunchKernelGGL(refs_edge_flags_kernel, gm, blk, 0, s, d_i, d_j, stride, m, d_is_ref, eflag);
    tb = tmp;
    PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, eflag, epos, 0, m, rocprim::plus<int>(), s));
    if (d_ref_edges)
      hipLaunchKernelGGL(refs_edge_write_kernel, gm, blk, 0, s, d_i, d_j, stride, m, eflag, epos, rank, d_ref_edges);
  }
  hipLaunchKernelGGL(refs_counts_kernel, dim3(1), dim3(64), 0, s, ctl, vflag, rank, n, eflag, epos, m, d_counts);
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_pick_refs(const long long *i, const long long *j, size_t n_edges, size_t n_vertices,
                             const uint8_t *existing, const uint8_t *merged, int fast, int device_id, uint8_t *is_ref,
                             long long *ref_edges, long long *counts) {
  const std::string who = kWho;
  if (!counts || (!is_ref && n_vertices) || (n_edges && (!i || !j))) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const int rc0 = check_sizes(who, n_edges, n_vertices);
  if (rc0 != PPK_OK) return rc0;
  long long *d_i, *d_j, *d_edges, *d_counts;
  uint8_t *d_existing, *d_merged, *d_is_ref;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_existing, n_vertices).take(d_merged, n_vertices);
    c.take(d_is_ref, n_vertices).take(d_edges, 2 * n_edges).take(d_counts, 8);
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
    }
    if (existing && n_vertices) PPK_HIP(hipMemcpy(d_existing, existing, n_vertices, hipMemcpyHostToDevice));
    if (merged && n_vertices) PPK_HIP(hipMemcpy(d_merged, merged, n_vertices, hipMemcpyHostToDevice));
    const int rc = ppk_pick_refs_dev(d_i, d_j, 1, n_edges, n_vertices, existing ? d_existing : nullptr,
                                     merged ? d_merged : nullptr, fast, d_is_ref, ref_edges ? d_edges : nullptr, d_counts,
                                     nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(counts, d_counts, 64, hipMemcpyDeviceToHost));
    if (n_vertices) PPK_HIP(hipMemcpy(is_ref, d_is_ref, n_vertices, hipMemcpyDeviceToHost));
    if (ref_edges && counts[1]) PPK_HIP(hipMemcpy(ref_edges, d_edges, (size_t)counts[1] * 16, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}
