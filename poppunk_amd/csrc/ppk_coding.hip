// The coded copies of a resident bbits = 14 database (PpkCoding in ppk_internal.h): the kernels that build them, the
// choice among them as pure functions of the count pass's figures (pinned on the CPU through ppk_choose_coding and
// ppk_choose_holder: tests/test_rank_fold2_host.py, tests/test_rank_foldh_host.py), the execution of that choice for
// ppk_db_create, and the accessors of what it built.  Nothing here computes a distance: a self job reads the copies
// through coded_planes / launch_rank in ppk_dist.hip.
#include <algorithm>

#include "ppk_internal.h"

// Rank codes of a bbits = 14 database (PpkCoding: the injective copy, the folded pair).  One workgroup per (k, 64-bin block, byte g of
// the block's words) = 8 bin positions.  Per position a 16 384-bit presence bitmap of the values samples [0, n) hold
// there goes into LDS, and next to it (count pass, folded codes) the bitmap of the values seen at least twice: the
// presence atomicOr returns the old word, and a bit that was already set is a second holder.  A prefix popcount turns a
// value into its rank among the position's distinct (or shared) values.
//   WRITE = false: D, the largest number of distinct values of any position, into max_distinct[0], and of any position
//                  of each (k, 64-bin block) into max_distinct[1 + k * s64 + block].  Behind them, at
//                  max_distinct[1 + nk * s64 ...], the same two for E = S + 2, the codes a folded position spans (S: its
//                  shared values, those with at least two holders).
//   WRITE = true:  byte g of the PL code planes of every sample, out = [k][block * PL + plane][npad] (padding samples
//                  get code 0).  The caller has checked that every code is below 2^PL.
//     FOLD = false: code = rank among the position's distinct values (injective).
//     FOLD = true:  two copies.  A shared value gets 2 + its rank among the position's shared values in both; a value
//                   with a single holder gets 0 in `out` (the ref side) and 1 in `out_q` (the query side): it can match
//                   nothing in a job that compares two different samples, and 0 != 1 != every shared code says so.
constexpr int RANK_BMW = (1 << RANK_BB) / 32;      // bitmap dwords per position
//     FOLD2 (with FOLD): the two-holder pair.  A third bitmap, fed by what the atomicOr into "seen twice" returns, holds
//                   the values with at least three holders; they alone keep codes 2 + rank (among themselves), and a
//                   value with one or two holders is 0 in `out` and 1 in `out_q`.  Every two-holder value is an event:
//                   its rank among the position's two-holder values names a pair of LDS slots, the samples that hold it
//                   atomicMin / atomicMax themselves into them, and the workgroup appends (hi, lo, k) to ev.raw and
//                   counts the event's bucket (PpkCoding::d_list).
//   The count pass leaves E2 = S3 + 2 behind E in the same form, behind that the most two-holder values of any
//   position and their number over all positions (PPK_RANK_EXTRA words), and behind those E2 of every position,
//   [k][64 * s64]: what ppk_db_create sorts the positions of the two-holder pair by.
//     FOLD2 with `bytes`: no planes are written; the ref-side code of stored position i of k goes to
//                   bytes[(k * 64 * s64 + i) * npad + sample] (padding samples 0), for fold2_slice_kernel.
struct Fold2Emit {
  unsigned long long *raw;      // hi | lo << 28 | k << 56
  unsigned *count;              // events appended so far
  unsigned *bucket;             // events per bucket (lo / 32) * rt + hi / 256
  unsigned cap, rt;
};
template <bool WRITE, bool FOLD = false, bool FOLD2 = false>
__global__ void __launch_bounds__(256)
rank_code_kernel(const uint64_t *__restrict__ skT, uint8_t *__restrict__ out, uint8_t *__restrict__ out_q,
                 unsigned *__restrict__ max_distinct, size_t n, size_t npad, int s64, int pl, const Fold2Emit ev,
                 uint8_t *__restrict__ bytes = nullptr) {
  static_assert(!FOLD2 || (WRITE && FOLD), "the two-holder pair is a folded pair");
  constexpr bool TWICE = !WRITE || FOLD;
  constexpr bool THRICE = !WRITE || FOLD2;
  constexpr int SLOTS = PPK_FOLD2_SLOTS;
  __shared__ uint32_t bitmap[8][RANK_BMW];                 // (FOLD2, after the feed: the values with exactly two holders)
  __shared__ uint32_t twice[TWICE ? 8 : 1][RANK_BMW];      // values with at least two holders
  __shared__ uint32_t thrice[THRICE ? 8 : 1][RANK_BMW];    // values with at least three holders
  __shared__ uint16_t before[WRITE ? 8 : 1][RANK_BMW];     // coded values (distinct; FOLD: shared; FOLD2: thrice held) below the dword's first one
  __shared__ uint16_t before2[FOLD2 ? 8 : 1][RANK_BMW];    // two-holder values below the dword's first one
  __shared__ uint32_t ev_lo[FOLD2 ? 8 : 1][FOLD2 ? SLOTS : 1], ev_hi[FOLD2 ? 8 : 1][FOLD2 ? SLOTS : 1];
  __shared__ uint32_t ev_n[8], ev_base[8];
  const int g = blockIdx.x & 7;
  const size_t kb = blockIdx.x >> 3;            // k * s64 + block
  const uint64_t *src = skT + kb * RANK_BB * npad;
  for (int i = threadIdx.x; i < 8 * RANK_BMW; i += 256) {
    (&bitmap[0][0])[i] = 0;
    if (TWICE) (&twice[0][0])[i] = 0;
    if (THRICE) (&thrice[0][0])[i] = 0;
  }
  if constexpr (FOLD2) {
    for (int i = threadIdx.x; i < 8 * SLOTS; i += 256) {
      (&ev_lo[0][0])[i] = 0xffffffffu;
      (&ev_hi[0][0])[i] = 0;
    }
  }
  __syncthreads();
  auto values = [&](size_t smp, uint32_t (&v)[8]) {
    uint32_t byte[RANK_BB];
#pragma unroll
    for (int b = 0; b < RANK_BB; ++b) byte[b] = (uint32_t)(src[(size_t)b * npad + smp] >> (8 * g)) & 0xffu;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = 0;
#pragma unroll
      for (int b = 0; b < RANK_BB; ++b) v[j] |= ((byte[b] >> j) & 1u) << b;
    }
  };
  for (size_t smp = threadIdx.x; smp < n; smp += 256) {
    uint32_t v[8];
    values(smp, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t bit = 1u << (v[j] & 31u);
      const uint32_t old = atomicOr(&bitmap[j][v[j] >> 5], bit);
      if (TWICE && (old & bit)) {
        const uint32_t old2 = atomicOr(&twice[j][v[j] >> 5], bit);
        if (THRICE && (old2 & bit)) atomicOr(&thrice[j][v[j] >> 5], bit);
      }
    }
  }
  __syncthreads();
  // 32 threads per position, 16 consecutive dwords each: an exclusive prefix sum of their popcounts
  {
    const int j = threadIdx.x >> 5, t = threadIdx.x & 31;
    auto prefix = [&](const uint32_t *bm, uint32_t &sum) {
      sum = 0;
      for (int w = 0; w < RANK_BMW / 32; ++w) sum += __popc(bm[t * (RANK_BMW / 32) + w]);
      uint32_t incl = sum;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 32);
        if (t >= d) incl += up;
      }
      return incl;
    };
    if constexpr (!WRITE) {
      uint32_t sum;
      const uint32_t d_incl = prefix(bitmap[j], sum), s_incl = prefix(twice[j], sum), s3_incl = prefix(thrice[j], sum);
      if (t == 31) {
        const unsigned seg = 1 + gridDim.x / 8;
        unsigned *max_fold = max_distinct + seg, *max_fold2 = max_distinct + 2 * seg, *extra = max_distinct + 3 * seg;
        atomicMax(max_distinct, d_incl);
        atomicMax(max_distinct + 1 + kb, d_incl);
        atomicMax(max_fold, s_incl + 2u);
        atomicMax(max_fold + 1 + kb, s_incl + 2u);
        atomicMax(max_fold2, s3_incl + 2u);
        atomicMax(max_fold2 + 1 + kb, s3_incl + 2u);
        atomicMax(extra, s_incl - s3_incl);
        atomicAdd(extra + 1, s_incl - s3_incl);
        extra[PPK_RANK_EXTRA + kb * 64 + (size_t)(g * 8 + j)] = s3_incl + 2u;
      }
      return;
    } else {
      if constexpr (FOLD2) {
        for (int w = 0; w < RANK_BMW / 32; ++w) {
          const int i = t * (RANK_BMW / 32) + w;
          bitmap[j][i] = twice[j][i] & ~thrice[j][i];      // (this thread's own 16 dwords, read back below)
        }
      }
      auto ranks = [&](const uint32_t *bm, uint16_t *bef) {
        uint32_t sum;
        const uint32_t incl = prefix(bm, sum);
        uint32_t run = incl - sum;
        for (int w = 0; w < RANK_BMW / 32; ++w) {
          bef[t * (RANK_BMW / 32) + w] = (uint16_t)run;
          run += __popc(bm[t * (RANK_BMW / 32) + w]);
        }
        return incl;
      };
      ranks(FOLD2 ? thrice[j] : FOLD ? twice[j] : bitmap[j], before[j]);
      if constexpr (FOLD2) {
        const uint32_t two_incl = ranks(bitmap[j], before2[j]);
        if (t == 31) ev_n[j] = two_incl < (uint32_t)SLOTS ? two_incl : (uint32_t)SLOTS;      // (the caller has checked: never above)
      }
    }
  }
  __syncthreads();
  uint8_t *dst = out + kb * (size_t)pl * npad * 8 + g;
  uint8_t *dst_q = FOLD ? out_q + kb * (size_t)pl * npad * 8 + g : nullptr;
  for (size_t smp = threadIdx.x; smp < npad; smp += 256) {
    uint32_t code[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t single = 0;      // FOLD: bit j set where the sample's value at position j has no other holder (FOLD2: at most one)
    if (smp < n) {
      uint32_t v[8];
      values(smp, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w = v[j] >> 5, bit = 1u << (v[j] & 31u);
        if constexpr (FOLD2) {
          if (thrice[j][w] & bit) {
            code[j] = 2u + before[j][w] + __popc(thrice[j][w] & (bit - 1u));
          } else {
            single |= 1u << j;
            if (bitmap[j][w] & bit) {
              const uint32_t slot = before2[j][w] + __popc(bitmap[j][w] & (bit - 1u));
              if (slot < (uint32_t)SLOTS) {
                atomicMin(&ev_lo[j][slot], (uint32_t)smp);
                atomicMax(&ev_hi[j][slot], (uint32_t)smp);
              }
            }
          }
        } else if constexpr (FOLD) {
          if (twice[j][w] & bit) code[j] = 2u + before[j][w] + __popc(twice[j][w] & (bit - 1u));
          else single |= 1u << j;
        } else {
          code[j] = before[j][w] + __popc(bitmap[j][w] & (bit - 1u));
        }
      }
    }
    if constexpr (FOLD2) {
      if (bytes) {      // (workgroup-uniform)
#pragma unroll
        for (int j = 0; j < 8; ++j) bytes[(kb * 64 + (size_t)(g * 8 + j)) * npad + smp] = (uint8_t)code[j];
        continue;
      }
    }
    for (int b = 0; b < pl; ++b) {
      uint32_t byte = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) byte |= ((code[j] >> b) & 1u) << j;
      dst[((size_t)b * npad + smp) * 8] = (uint8_t)byte;
      // (a shared code is the same on both sides; a single holder's differs in bit 0 alone)
      if constexpr (FOLD) dst_q[((size_t)b * npad + smp) * 8] = (uint8_t)(b == 0 ? byte | single : byte);
    }
  }
  if constexpr (FOLD2) {
    // one event per two-holder value: one reservation per workgroup, then 32 threads per position
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
      for (int j = 0; j < 8; ++j) {
        ev_base[j] = total;
        total += ev_n[j];
      }
      const uint32_t at = total ? atomicAdd(ev.count, total) : 0u;
      for (int j = 0; j < 8; ++j) ev_base[j] += at;
    }
    __syncthreads();
    const int j = threadIdx.x >> 5;
    const unsigned long long k = kb / (size_t)s64;
    for (uint32_t slot = threadIdx.x & 31; slot < ev_n[j]; slot += 32) {
      const uint32_t hi = ev_hi[j][slot], lo = ev_lo[j][slot], at = ev_base[j] + slot;
      if (at >= ev.cap) continue;
      if (hi < n && lo < hi) {
        ev.raw[at] = (unsigned long long)hi | ((unsigned long long)lo << 28) | (k << 56);
        atomicAdd(ev.bucket + (size_t)(lo >> 5) * ev.rt + (hi >> 8), 1u);
      } else {
        ev.raw[at] = ~0ull;      // (not two holders after all: never -- the scatter reports it, the pair is dropped)
      }
    }
  }
}

// The planes of the two-holder pair with its positions in sorted order (PpkCoding::order): slot i of k holds stored
// position order[k * 64 * s64 + i].  One workgroup per (k, destination block, byte g of its words) and 256 samples; a
// thread gathers its sample's 8 byte codes (rank_code_kernel with `bytes`) and writes byte g of the `pl` planes of both
// copies, laid out as rank_code_kernel writes them.  A code is 0 or at least 2: 0 is 1 on the query side (samples below n).
__global__ void __launch_bounds__(256)
fold2_slice_kernel(const uint8_t *__restrict__ bytes, const unsigned *__restrict__ order, uint8_t *__restrict__ out,
                   uint8_t *__restrict__ out_q, size_t n, size_t npad, int s64, int pl) {
  const int g = blockIdx.x & 7;
  const size_t kb = blockIdx.x >> 3, k = kb / (size_t)s64, nbins = 64 * (size_t)s64;
  const size_t smp = (size_t)blockIdx.y * 256 + threadIdx.x;
  if (smp >= npad) return;
  const unsigned *ord = order + k * nbins + (kb % (size_t)s64) * 64 + (size_t)g * 8;
  uint32_t code[8], single = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const size_t pos = ord[j] < nbins ? ord[j] : 0;      // (a permutation of [0, nbins): always below)
    code[j] = bytes[(k * nbins + pos) * npad + smp];
    if (smp < n && code[j] == 0) single |= 1u << j;
  }
  uint8_t *dst = out + kb * (size_t)pl * npad * 8 + g, *dst_q = out_q + kb * (size_t)pl * npad * 8 + g;
  for (int b = 0; b < pl; ++b) {
    uint32_t byte = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) byte |= ((code[j] >> b) & 1u) << j;
    dst[((size_t)b * npad + smp) * 8] = (uint8_t)byte;
    dst_q[((size_t)b * npad + smp) * 8] = (uint8_t)(b == 0 ? byte | single : byte);
  }
}

constexpr int FOLD2_TILE_PAIRS = 256 * 32;      // pairs of one (256 refs x 32 queries) tile: 13 bits of an event
// The counting sort of the events into their buckets (PpkCoding::d_list) and the check of the per-pair cap.
// fold2_scan_kernel: one workgroup; off = exclusive prefix sum of cnt (nb entries, off[nb] = the total), cnt back to
// zero for the scatter's cursors.
__global__ void __launch_bounds__(1024)
fold2_scan_kernel(unsigned *__restrict__ cnt, unsigned *__restrict__ off, size_t nb) {
  __shared__ unsigned part[1024];
  const size_t per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
  unsigned sum = 0;
  for (size_t b = b0; b < b1; ++b) sum += cnt[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const unsigned up = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += up;
    __syncthreads();
  }
  unsigned run = part[threadIdx.x] - sum;
  for (size_t b = b0; b < b1; ++b) {
    off[b] = run;
    run += cnt[b];
    cnt[b] = 0;
  }
  if (threadIdx.x == 1023) off[nb] = part[1023];
}
__global__ void __launch_bounds__(256)
fold2_scatter_kernel(const unsigned long long *__restrict__ raw, unsigned *n_raw, unsigned cap,
                     const unsigned *__restrict__ off, unsigned *__restrict__ cursor, uint16_t *__restrict__ ev, unsigned rt) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x, total = *n_raw < cap ? *n_raw : cap;
  if (i >= total) return;
  const unsigned long long e = raw[i];
  if (e == ~0ull) {
    n_raw[1] = 1u;      // the overflow flag sits behind the counter
    return;
  }
  const uint32_t hi = (uint32_t)e & 0xfffffffu, lo = (uint32_t)(e >> 28) & 0xfffffffu, k = (uint32_t)(e >> 56);
  const size_t b = (size_t)(lo >> 5) * rt + (hi >> 8);
  const unsigned at = off[b] + atomicAdd(cursor + b, 1u);
  if (at < off[b + 1]) ev[at] = (uint16_t)((hi & 255u) | ((lo & 31u) << 8) | (k << 13));
}
// one workgroup per bucket, the tile kernel's own correction words: a field that is asked to count past 63 sets *overflow
__global__ void __launch_bounds__(256)
fold2_check_kernel(const uint16_t *__restrict__ ev, const unsigned *__restrict__ off, unsigned *__restrict__ overflow) {
  __shared__ uint32_t corr[FOLD2_TILE_PAIRS];
  const unsigned e0 = off[blockIdx.x], e1 = off[blockIdx.x + 1];
  if (e0 == e1) return;      // (workgroup-uniform)
  for (int i = threadIdx.x; i < FOLD2_TILE_PAIRS; i += 256) corr[i] = 0;
  __syncthreads();
  for (unsigned e = e0 + threadIdx.x; e < e1; e += 256) {
    const uint32_t v = ev[e], k = v >> 13;
    const uint32_t old = atomicAdd(&corr[v & 0x1fffu], 1u << (6u * k));
    if (((old >> (6u * k)) & 63u) == (uint32_t)PPK_FOLD2_MAX_PER_PAIR) *overflow = 1u;
  }
}

// ---- the holder pair (PPK_CODING_FOLDH) --------------------------------------------------------------------------------
// Holder counts.  One workgroup per (k, 64-bin block, byte g) = 8 positions, as rank_code_kernel: a first pass over the
// samples leaves the bitmap of the values at least two samples hold (the position's SHARED values), a prefix popcount
// ranks them, and a second pass counts every shared value's holders in an LDS counter named by its rank (the caller
// has checked that no position has more than PPK_FOLDH_SLOTS shared values).  Out: the bitmap, twice[position][512];
// the counts in rank order, saturated at 65 535, holders[position][PPK_FOLDH_SLOTS]; and per position and bound H of
// `ladder` E_H = (values with more than H holders) + 2, pos_e[position][PPK_FOLDH_LADDER].
struct FoldhLadder {
  unsigned h[PPK_FOLDH_LADDER];
};
__device__ __forceinline__ void foldh_values(const uint64_t *src, size_t npad, size_t smp, int g, uint32_t (&v)[8]) {
  uint32_t byte[RANK_BB];
#pragma unroll
  for (int b = 0; b < RANK_BB; ++b) byte[b] = (uint32_t)(src[(size_t)b * npad + smp] >> (8 * g)) & 0xffu;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = 0;
#pragma unroll
    for (int b = 0; b < RANK_BB; ++b) v[j] |= ((byte[b] >> j) & 1u) << b;
  }
}
// 32 threads per position (t = their index), 16 consecutive dwords each: before[i] = set bits below dword i
__device__ __forceinline__ void foldh_rank_bitmap(const uint32_t *bm, uint16_t *bef, int t) {
  uint32_t sum = 0;
  for (int w = 0; w < RANK_BMW / 32; ++w) sum += __popc(bm[t * (RANK_BMW / 32) + w]);
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 32);
    if (t >= d) incl += up;
  }
  uint32_t run = incl - sum;
  for (int w = 0; w < RANK_BMW / 32; ++w) {
    bef[t * (RANK_BMW / 32) + w] = (uint16_t)run;
    run += __popc(bm[t * (RANK_BMW / 32) + w]);
  }
}
__global__ void __launch_bounds__(256)
foldh_count_kernel(const uint64_t *__restrict__ skT, unsigned *__restrict__ twice_out, uint16_t *__restrict__ holders,
                   unsigned *__restrict__ pos_e, size_t n, size_t npad, const FoldhLadder ladder) {
  constexpr int SLOTS = PPK_FOLDH_SLOTS;
  __shared__ uint32_t bitmap[8][RANK_BMW];
  __shared__ uint32_t twice[8][RANK_BMW];
  __shared__ uint16_t before[8][RANK_BMW];
  __shared__ uint32_t cnt[8][SLOTS];
  const int g = blockIdx.x & 7;
  const size_t kb = blockIdx.x >> 3;            // k * s64 + block
  const uint64_t *src = skT + kb * RANK_BB * npad;
  for (int i = threadIdx.x; i < 8 * RANK_BMW; i += 256) {
    (&bitmap[0][0])[i] = 0;
    (&twice[0][0])[i] = 0;
  }
  for (int i = threadIdx.x; i < 8 * SLOTS; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  for (size_t smp = threadIdx.x; smp < n; smp += 256) {
    uint32_t v[8];
    foldh_values(src, npad, smp, g, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t bit = 1u << (v[j] & 31u);
      const uint32_t old = atomicOr(&bitmap[j][v[j] >> 5], bit);
      if (old & bit) atomicOr(&twice[j][v[j] >> 5], bit);
    }
  }
  __syncthreads();
  const int pj = threadIdx.x >> 5, t = threadIdx.x & 31;
  foldh_rank_bitmap(twice[pj], before[pj], t);
  __syncthreads();
  for (size_t smp = threadIdx.x; smp < n; smp += 256) {
    uint32_t v[8];
    foldh_values(src, npad, smp, g, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w = v[j] >> 5, bit = 1u << (v[j] & 31u);
      if (twice[j][w] & bit) {
        const uint32_t slot = before[j][w] + __popc(twice[j][w] & (bit - 1u));
        if (slot < (uint32_t)SLOTS) atomicAdd(&cnt[j][slot], 1u);
      }
    }
  }
  __syncthreads();
  const size_t pos = kb * 64 + (size_t)(g * 8 + pj);
  unsigned above[PPK_FOLDH_LADDER];
#pragma unroll
  for (int i = 0; i < PPK_FOLDH_LADDER; ++i) above[i] = 0;
  for (int sl = t; sl < SLOTS; sl += 32) {
    const uint32_t c = cnt[pj][sl];
    holders[pos * SLOTS + sl] = (uint16_t)(c < 65535u ? c : 65535u);
#pragma unroll
    for (int i = 0; i < PPK_FOLDH_LADDER; ++i) above[i] += c > ladder.h[i] ? 1u : 0u;
  }
  for (int w = t; w < RANK_BMW; w += 32) twice_out[pos * RANK_BMW + w] = twice[pj][w];
#pragma unroll
  for (int i = 0; i < PPK_FOLDH_LADDER; ++i) {
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) above[i] += __shfl_down(above[i], d, 32);
    if (t == 0) pos_e[pos * PPK_FOLDH_LADDER + i] = above[i] + 2u;
  }
}

// Codes.  Same grid; reads the count pass's bitmap and holder counts back.  Per position the shared values split in two
// classes, each ranked in value order: KEPT (more than H holders) and FOLDED (2 .. H).  Two codes per (position, sample):
//   kept_out  (one byte, for fold2_slice_kernel): 2 + rank of a kept value, 0 for every other -- the holder pair;
//   owed_out  (16 bits, for foldh_slice14_kernel): 2 + rank of a folded value, 0 for every other -- the temporary pair,
//             whose compare counts exactly the matches the holder pair cannot see.
// Padding samples get 0 in both.
__global__ void __launch_bounds__(256)
foldh_code_kernel(const uint64_t *__restrict__ skT, const unsigned *__restrict__ twice_in, const uint16_t *__restrict__ holders,
                  uint8_t *__restrict__ kept_out, uint16_t *__restrict__ owed_out, size_t n, size_t npad, unsigned H) {
  constexpr int SLOTS = PPK_FOLDH_SLOTS;
  __shared__ uint32_t twice[8][RANK_BMW];
  __shared__ uint16_t before[8][RANK_BMW];
  __shared__ uint16_t code[8][SLOTS];      // bit 15: kept; below it the rank within the class
  const int g = blockIdx.x & 7;
  const size_t kb = blockIdx.x >> 3;
  const uint64_t *src = skT + kb * RANK_BB * npad;
  const int pj = threadIdx.x >> 5, t = threadIdx.x & 31;
  const size_t pos = kb * 64 + (size_t)(g * 8 + pj);
  for (int w = t; w < RANK_BMW; w += 32) twice[pj][w] = twice_in[pos * RANK_BMW + w];
  __syncthreads();
  foldh_rank_bitmap(twice[pj], before[pj], t);
  {
    // thread t ranks slots [t * 32, t * 32 + 32) (slots past the position's shared values hold 0 holders: never read)
    constexpr int PER = SLOTS / 32;
    uint32_t kept = 0, folded = 0;
    for (int i = 0; i < PER; ++i) {
      const uint32_t c = holders[pos * SLOTS + t * PER + i];
      kept += c > H ? 1u : 0u;
      folded += c >= 2u && c <= H ? 1u : 0u;
    }
    uint32_t packed = kept | (folded << 16), incl = packed;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 32);
      if (t >= d) incl += up;
    }
    uint32_t run_k = (incl - packed) & 0xffffu, run_f = (incl - packed) >> 16;
    for (int i = 0; i < PER; ++i) {
      const uint32_t c = holders[pos * SLOTS + t * PER + i];
      if (c > H) code[pj][t * PER + i] = (uint16_t)(0x8000u | run_k++);
      else code[pj][t * PER + i] = (uint16_t)(c >= 2u ? run_f++ : 0x7fffu);
    }
  }
  __syncthreads();
  for (size_t smp = threadIdx.x; smp < npad; smp += 256) {
    uint32_t ck[8] = {0, 0, 0, 0, 0, 0, 0, 0}, co[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (smp < n) {
      uint32_t v[8];
      foldh_values(src, npad, smp, g, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w = v[j] >> 5, bit = 1u << (v[j] & 31u);
        if (twice[j][w] & bit) {
          const uint32_t slot = before[j][w] + __popc(twice[j][w] & (bit - 1u));
          const uint32_t c = slot < (uint32_t)SLOTS ? code[j][slot] : 0x7fffu;
          if (c & 0x8000u) ck[j] = 2u + (c & 0x7fffu);
          else if (c != 0x7fffu) co[j] = 2u + c;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t at = (kb * 64 + (size_t)(g * 8 + j)) * npad + smp;
      kept_out[at] = (uint8_t)ck[j];
      owed_out[at] = (uint16_t)co[j];
    }
  }
}

// The temporary pair in the raw 14-plane layout, positions in stored order: [k][block * 14 + plane][npad], byte g of
// both copies per workgroup and 256 samples (fold2_slice_kernel for 16-bit codes).  0 is 1 on the query side.
__global__ void __launch_bounds__(256)
foldh_slice14_kernel(const uint16_t *__restrict__ codes, uint8_t *__restrict__ out, uint8_t *__restrict__ out_q, size_t n,
                     size_t npad) {
  const int g = blockIdx.x & 7;
  const size_t kb = blockIdx.x >> 3;
  const size_t smp = (size_t)blockIdx.y * 256 + threadIdx.x;
  if (smp >= npad) return;
  uint32_t code[8], single = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    code[j] = codes[(kb * 64 + (size_t)(g * 8 + j)) * npad + smp];
    if (smp < n && code[j] == 0) single |= 1u << j;
  }
  uint8_t *dst = out + kb * (size_t)RANK_BB * npad * 8 + g, *dst_q = out_q + kb * (size_t)RANK_BB * npad * 8 + g;
#pragma unroll
  for (int b = 0; b < RANK_BB; ++b) {
    uint32_t byte = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) byte |= ((code[j] >> b) & 1u) << j;
    dst[((size_t)b * npad + smp) * 8] = (uint8_t)byte;
    dst_q[((size_t)b * npad + smp) * 8] = (uint8_t)(b == 0 ? byte | single : byte);
  }
}

// One band of the temporary pair's counts (the tile kernel's MODE_COUNTS rows: row * nk + k) into raw entries
// hi | lo << 24 | k << 48 | count << 52.  One workgroup per bucket -- 32 queries from q_begin + 32 * blockIdx.y, the 256
// refs of ref block blockIdx.x, thread t its ref -- so a bucket's count is its workgroup's total, written without an
// atomic, and the list is appended to through ONE reservation per workgroup (a reservation per wavefront, 780 000 adds
// to one address at the bench shape, took 8 ms).  Two passes over the bucket's 160 KB of counts: count, then write.
struct FoldhEmit {
  unsigned long long *raw;
  unsigned long long *count;    // entries appended so far (may pass cap: the caller then drops the pair)
  unsigned *bucket;             // entries per bucket (lo / 32) * rt + hi / 256
  unsigned long long cap;
  unsigned rt;
};
__global__ void __launch_bounds__(256)
foldh_emit_kernel(const uint32_t *__restrict__ counts, size_t n, size_t q_begin, size_t q_end, size_t row_base, int nk,
                  const FoldhEmit ev) {
  __shared__ uint32_t part[256];
  __shared__ unsigned long long base_s;
  const size_t q0 = q_begin + (size_t)blockIdx.y * 32, rf = (size_t)blockIdx.x * 256 + threadIdx.x;
  if ((size_t)blockIdx.x * 256 + 255 <= q0) return;      // (workgroup-uniform: no ref above the bucket's first query)
  const size_t q1 = q0 + 32 < q_end ? q0 + 32 : q_end;
  uint32_t mine = 0;
  if (rf < n)
    for (size_t qq = q0; qq < q1 && qq < rf; ++qq) {
      const uint32_t *c = counts + (qq * n - (qq * (qq + 1)) / 2 + (rf - qq - 1) - row_base) * (size_t)nk;
      for (int k = 0; k < nk; ++k) mine += c[k] != 0 ? 1u : 0u;
    }
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t up = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += up;
    __syncthreads();
  }
  const uint32_t total = part[255];
  if (total == 0) return;      // (workgroup-uniform)
  if (threadIdx.x == 0) {
    base_s = atomicAdd(ev.count, (unsigned long long)total);
    ev.bucket[(size_t)(q0 >> 5) * ev.rt + blockIdx.x] = total;
  }
  __syncthreads();
  unsigned long long at = base_s + (part[threadIdx.x] - mine);
  if (rf < n && mine)
    for (size_t qq = q0; qq < q1 && qq < rf; ++qq) {
      const uint32_t *c = counts + (qq * n - (qq * (qq + 1)) / 2 + (rf - qq - 1) - row_base) * (size_t)nk;
      for (int k = 0; k < nk; ++k)
        if (c[k] != 0) {
          if (at < ev.cap)
            ev.raw[at] = (unsigned long long)rf | ((unsigned long long)qq << 24) | ((unsigned long long)k << 48) |
                         ((unsigned long long)(c[k] & 4095u) << 52);
          ++at;
        }
    }
}
__global__ void __launch_bounds__(256)
foldh_scatter_kernel(const unsigned long long *__restrict__ raw, size_t total, const unsigned *__restrict__ off,
                     unsigned *__restrict__ cursor, uint32_t *__restrict__ ent, unsigned rt) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const unsigned long long e = raw[i];
  const uint32_t hi = (uint32_t)e & 0xffffffu, lo = (uint32_t)(e >> 24) & 0xffffffu, k = (uint32_t)(e >> 48) & 7u, c = (uint32_t)(e >> 52);
  const size_t b = (size_t)(lo >> 5) * rt + (hi >> 8);
  const unsigned at = off[b] + atomicAdd(cursor + b, 1u);
  if (at < off[b + 1]) ent[at] = (hi & 255u) | ((lo & 31u) << 8) | (k << 13) | (c << 16);
}

// ---- launchers and builders ------------------------------------------------------------------------------------------
// The rank codes of a transposed bbits = 14 database (rank_code_kernel): the count pass (d_max: 3 * (1 + nk * s64) +
// PPK_RANK_EXTRA + nk * s64 * 64 words, the D maxima, behind them the E and the E2 maxima, then the two-holder figures
// and E2 of every position), then -- with
// `d_out` -- the code planes: injective, or with `d_out_q` the folded pair (d_out the ref side).  Both only enqueue.
int ppk_launch_rank_count(const uint64_t *d_skT, size_t n, size_t npad, size_t nk, size_t s64, unsigned *d_max, hipStream_t s) {
  PPK_HIP(hipMemsetAsync(d_max, 0, (3 * (1 + nk * s64) + PPK_RANK_EXTRA + nk * s64 * 64) * sizeof(unsigned), s));
  hipLaunchKernelGGL((rank_code_kernel<false>), dim3((unsigned)(nk * s64 * 8)), dim3(256), 0, s, d_skT, nullptr, nullptr, d_max,
                     n, npad, (int)s64, 0, Fold2Emit{});
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}
int ppk_launch_rank_codes(const uint64_t *d_skT, uint64_t *d_out, uint64_t *d_out_q, size_t n, size_t npad, size_t nk,
                          size_t s64, int planes, hipStream_t s) {
  const dim3 grid((unsigned)(nk * s64 * 8)), block(256);
  if (d_out_q)
    hipLaunchKernelGGL((rank_code_kernel<true, true>), grid, block, 0, s, d_skT, reinterpret_cast<uint8_t *>(d_out),
                       reinterpret_cast<uint8_t *>(d_out_q), nullptr, n, npad, (int)s64, planes, Fold2Emit{});
  else
    hipLaunchKernelGGL((rank_code_kernel<true, false>), grid, block, 0, s, d_skT, reinterpret_cast<uint8_t *>(d_out), nullptr,
                       nullptr, n, npad, (int)s64, planes, Fold2Emit{});
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}
// The two-holder pair of `db` and its event list.  Everything is allocated here; a device too full for it, or a
// (pair, k) with more events than its field holds (*overflow), leaves the database without the pair.  With `order`
// (nk * 64 * s64 stored positions, a permutation per k) slot i of k holds stored position order[k * 64 * s64 + i]: the
// code pass then leaves byte codes per stored position and fold2_slice_kernel gathers them into the planes (one byte
// per (position, sample) of scratch, freed here).  Gathering inside the code pass would read every source word eight
// times, once per position of the workgroup's byte.
int ppk_build_fold2(ppk_db *db, int planes, size_t n_two, const std::vector<unsigned> *order, bool *overflow, hipStream_t s) {
  *overflow = false;
  const size_t copy_bytes = db->npad * db->nk * db->s64 * (size_t)planes * sizeof(uint64_t);
  const unsigned qt = (unsigned)(db->npad / 32), rt = (unsigned)(db->npad / 256);
  const size_t nb = (size_t)qt * rt, cap = n_two ? n_two : 1;
  unsigned long long *d_raw = nullptr;
  unsigned *d_cnt = nullptr;      // [nb] bucket counts / cursors, then the event counter and the overflow flag
  uint8_t *d_bytes = nullptr;     // `order`: the byte codes per stored position
  unsigned *d_order = nullptr;
  const size_t n_pos = db->nk * db->s64 * 64;
  PpkCoding &c = db->coding[PPK_CODING_FOLD2];
  auto drop = [&]() {
    (void)hipGetLastError();
    ppk_coding_free(c);
  };
  auto done = [&](int rc) {
    if (d_raw) (void)hipFree(d_raw);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_bytes) (void)hipFree(d_bytes);
    if (d_order) (void)hipFree(d_order);
    return rc;
  };
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&c.d_ref), copy_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c.d_qry), copy_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c.d_list), cap * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c.d_off), (nb + 1) * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_raw), cap * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_cnt), (nb + 2) * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (nb + 2) * sizeof(unsigned), s);
  if (order && order->size() != n_pos) order = nullptr;
  if (e == hipSuccess && order) e = hipMalloc(reinterpret_cast<void **>(&d_bytes), n_pos * db->npad);
  if (e == hipSuccess && order) e = hipMalloc(reinterpret_cast<void **>(&d_order), n_pos * sizeof(unsigned));
  if (e == hipSuccess && order) e = hipMemcpyAsync(d_order, order->data(), n_pos * sizeof(unsigned), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    drop();
    return done(PPK_OK);
  }
  const Fold2Emit ev = {d_raw, d_cnt + nb, d_cnt, (unsigned)cap, rt};
  hipLaunchKernelGGL((rank_code_kernel<true, true, true>), dim3((unsigned)(db->nk * db->s64 * 8)), dim3(256), 0, s, db->d_skT,
                     reinterpret_cast<uint8_t *>(c.d_ref), reinterpret_cast<uint8_t *>(c.d_qry), nullptr, db->n,
                     db->npad, (int)db->s64, planes, ev, d_bytes);
  if (order)
    hipLaunchKernelGGL(fold2_slice_kernel, dim3((unsigned)(db->nk * db->s64 * 8), (unsigned)(db->npad / 256)), dim3(256), 0, s,
                       d_bytes, d_order, reinterpret_cast<uint8_t *>(c.d_ref), reinterpret_cast<uint8_t *>(c.d_qry),
                       db->n, db->npad, (int)db->s64, planes);
  hipLaunchKernelGGL(fold2_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, c.d_off, nb);
  hipLaunchKernelGGL(fold2_scatter_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, d_raw, d_cnt + nb, (unsigned)cap,
                     c.d_off, d_cnt, static_cast<uint16_t *>(c.d_list), rt);
  hipLaunchKernelGGL(fold2_check_kernel, dim3((unsigned)nb), dim3(256), 0, s, static_cast<const uint16_t *>(c.d_list), c.d_off, d_cnt + nb + 1);
  unsigned tail[2] = {0, 0};      // events, overflow
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(tail, d_cnt + nb, sizeof(tail), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    drop();
    return done(ppk_fail(PPK_ERR_HIP, std::string("two-holder pair: ") + hipGetErrorString(e)));
  }
  if (tail[1] || tail[0] != n_two) {      // (a count that differs from the count pass's: never -- the list would be incomplete)
    *overflow = true;
    drop();
    return done(PPK_OK);
  }
  c.planes = c.stream_planes = planes;
  c.list_elem = sizeof(uint16_t);
  c.qt = qt;
  c.rt = rt;
  c.list_count = n_two;
  return done(PPK_OK);
}
// ---- the holder pair: creation -------------------------------------------------------------------------------------------
int ppk_foldh_count(const ppk_db *db, const unsigned *ladder, unsigned **d_twice, uint16_t **d_holders, std::vector<unsigned> *pos_e,
                    hipStream_t s) {
  const size_t n_pos = db->nk * db->s64 * 64;
  unsigned *d_e = nullptr;
  *d_twice = nullptr;
  *d_holders = nullptr;
  pos_e->assign(n_pos * PPK_FOLDH_LADDER, 0u);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(d_twice), n_pos * RANK_BMW * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(d_holders), n_pos * PPK_FOLDH_SLOTS * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_e), pos_e->size() * sizeof(unsigned));
  if (e == hipSuccess) {
    FoldhLadder l;
    for (int i = 0; i < PPK_FOLDH_LADDER; ++i) l.h[i] = ladder[i];
    hipLaunchKernelGGL(foldh_count_kernel, dim3((unsigned)(db->nk * db->s64 * 8)), dim3(256), 0, s, db->d_skT, *d_twice, *d_holders,
                       d_e, db->n, db->npad, l);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(pos_e->data(), d_e, pos_e->size() * sizeof(unsigned), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (d_e) (void)hipFree(d_e);
  if (e != hipSuccess) {      // (a device too full for the pass: no holder pair, nothing else changes)
    (void)hipGetLastError();
    if (*d_twice) (void)hipFree(*d_twice);
    if (*d_holders) (void)hipFree(*d_holders);
    *d_twice = nullptr;
    *d_holders = nullptr;
    pos_e->clear();
  }
  return PPK_OK;
}
int ppk_build_foldh(ppk_db *db, unsigned H, const unsigned *d_twice, const uint16_t *d_holders, size_t max_entries, hipStream_t s) {
  const size_t n = db->n, npad = db->npad, n_pos = db->nk * db->s64 * 64, n_kb = db->nk * db->s64;
  // (the copies keep PPK_FOLDH_CHUNK_PLANES planes of a block: no kept code reaches 2^4, PPK_FOLDH_MAX_CODES)
  const size_t copy_bytes = npad * n_kb * PPK_FOLDH_CHUNK_PLANES * sizeof(uint64_t), tmp_bytes = npad * n_kb * (size_t)RANK_BB * sizeof(uint64_t);
  const unsigned qt = (unsigned)(npad / 32), rt = (unsigned)(npad / 256);
  const size_t nb = (size_t)qt * rt, cap = max_entries ? max_entries : 1;
  // the counts of one band: at most 512 MB, whole blocks of 256 query rows, no more than a dispatch holds
  size_t band_q = ((size_t)512 << 20) / (n * db->nk * 4) / 256 * 256;
  if (band_q < 256) band_q = 256;
  if (band_q > ppk_rows_per_dispatch(db)) band_q = ppk_rows_per_dispatch(db);
  const size_t band_rows = ppk_rows_in_band(n, 0, 0, band_q < n ? band_q : n);      // (the first band is the longest)
  PpkCoding &c = db->coding[PPK_CODING_FOLDH];
  uint8_t *d_kept = nullptr;
  uint16_t *d_owed = nullptr;
  unsigned *d_order = nullptr, *d_cnt = nullptr;      // d_cnt: [nb] bucket counts / cursors, then the 64-bit entry counter
  uint64_t *d_tr = nullptr, *d_tq = nullptr;
  unsigned long long *d_raw = nullptr;
  void *d_band = nullptr;
  auto done = [&](int rc, bool keep) {
    for (void *ptr : {(void *)d_kept, (void *)d_owed, (void *)d_order, (void *)d_cnt, (void *)d_tr, (void *)d_tq, (void *)d_raw, d_band})
      if (ptr) (void)hipFree(ptr);
    if (!keep) {
      (void)hipGetLastError();
      ppk_coding_free(c);
    }
    return rc;
  };
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&c.d_ref), copy_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c.d_qry), copy_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c.d_off), (nb + 1) * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_kept), n_pos * npad);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_owed), n_pos * npad * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_order), n_pos * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_cnt), (nb + 2) * sizeof(unsigned) + 8);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_tr), tmp_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_tq), tmp_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_raw), cap * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&d_band, band_rows * db->nk * 4 + 256);
  if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (nb + 2) * sizeof(unsigned) + 8, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_order, c.order.data(), n_pos * sizeof(unsigned), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return done(PPK_OK, false);      // (a device too full: the pair only buys speed)
  const dim3 grid_pos((unsigned)(n_kb * 8)), grid_slice((unsigned)(n_kb * 8), (unsigned)(npad / 256));
  hipLaunchKernelGGL(foldh_code_kernel, grid_pos, dim3(256), 0, s, db->d_skT, d_twice, d_holders, d_kept, d_owed, n, npad, H);
  hipLaunchKernelGGL(fold2_slice_kernel, grid_slice, dim3(256), 0, s, d_kept, d_order, reinterpret_cast<uint8_t *>(c.d_ref),
                     reinterpret_cast<uint8_t *>(c.d_qry), n, npad, (int)db->s64, PPK_FOLDH_CHUNK_PLANES);
  hipLaunchKernelGGL(foldh_slice14_kernel, grid_slice, dim3(256), 0, s, d_owed, reinterpret_cast<uint8_t *>(d_tr),
                     reinterpret_cast<uint8_t *>(d_tq), n, npad);
  e = hipGetLastError();
  // (the entry counter sits behind the cursors, 8-byte aligned)
  unsigned long long *d_total = reinterpret_cast<unsigned long long *>(d_cnt + ((nb + 2) & ~(size_t)1));
  const FoldhEmit ev = {d_raw, d_total, d_cnt, (unsigned long long)cap, rt};
  for (size_t lo = 0; e == hipSuccess && lo + 1 < n; lo += band_q) {
    const size_t hi = lo + band_q < n ? lo + band_q : n;
    if (ppk_rows_in_band(n, 0, lo, hi) == 0) continue;
    const int rc = ppk_counts_band_raw(db, d_tr, d_tq, lo, hi, d_band, s);
    if (rc != PPK_OK) return done(rc, false);
    hipLaunchKernelGGL(foldh_emit_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((hi - lo + 31) / 32)), dim3(256), 0, s,
                       static_cast<const uint32_t *>(d_band), n, lo, hi, lo * n - (lo * (lo + 1)) / 2, (int)db->nk, ev);
    e = hipGetLastError();
  }
  unsigned long long total = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return done(ppk_fail(PPK_ERR_HIP, std::string("holder pair: ") + hipGetErrorString(e)), false);
  if (total > max_entries || total >= ((unsigned long long)1 << 32)) return done(PPK_OK, false);      // too dense to pay
  e = hipMalloc(reinterpret_cast<void **>(&c.d_list), (total ? total : 1) * sizeof(uint32_t));
  if (e != hipSuccess) return done(PPK_OK, false);
  hipLaunchKernelGGL(fold2_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, c.d_off, nb);
  if (total)
    hipLaunchKernelGGL(foldh_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_raw, (size_t)total,
                       c.d_off, d_cnt, static_cast<uint32_t *>(c.d_list), rt);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return done(ppk_fail(PPK_ERR_HIP, std::string("holder pair: ") + hipGetErrorString(e)), false);
  c.planes = 8;
  c.stream_planes = 4;
  c.holders = H;
  c.list_elem = sizeof(uint32_t);
  c.qt = qt;
  c.rt = rt;
  c.list_count = (size_t)total;
  return done(PPK_OK, true);
}

// ---- the description ---------------------------------------------------------------------------------------------------
void ppk_coding_free(PpkCoding &c) {
  for (void *ptr : {(void *)c.d_ref, c.d_qry != c.d_ref ? (void *)c.d_qry : nullptr, c.d_list, (void *)c.d_off})
    if (ptr) (void)hipFree(ptr);
  const PpkCodingKind kind = c.kind;
  c = PpkCoding();
  c.kind = kind;
}

bool ppk_coding_enabled(int kind) {
  const PpkConfig &cfg = ppk_config();
  const std::atomic<long long> *const option[PPK_CODINGS] = {&cfg.rank_planes, &cfg.rank_fold, &cfg.rank_fold2, &cfg.rank_foldh};
  return option[kind]->load() != 0;
}

void ppk_coding_launch_flags(const PpkCoding &c, unsigned *less1, unsigned *less2) {
  // the fewest planes a block of the sorted pairs may compare: "fold2_min_planes" 7 keeps the 6-plane blocks at 7,
  // "foldh_min_planes" 3 the 2-plane blocks at 3 and 4 every block at 4
  const long long min_planes = c.kind == PPK_CODING_FOLD2   ? ppk_config().fold2_min_planes.load()
                               : c.kind == PPK_CODING_FOLDH ? ppk_config().foldh_min_planes.load()
                                                            : 0;
  const bool use1 = ppk_config().rank_short.load() != 0 && !(c.kind == PPK_CODING_FOLDH && min_planes > 3);
  const bool use2 = use1 && min_planes <= c.stream_planes - 2;
  for (int k = 0; k < PPK_RANK_SHORT_WORDS; ++k) {
    less1[k] = use1 ? c.less1[k] : 0u;
    less2[k] = use2 ? c.less2[k] : 0u;
  }
}

// ---- the choice: pure functions, no device touched ---------------------------------------------------------------------
// D = the most distinct values any (k, bin) position holds over the samples decides the planes of the injective copy (8,
// 10 or 12; more than 4 096 values: no copy); a block that holds at most 2^(planes - 1) values per position has a zero
// top plane, and the tile kernel leaves that plane out there.  The count pass leaves a second figure per position: S,
// the values at least two samples hold there.  A value with a single holder matches nothing in a self job, so the folded
// pair gives all of them two reserved codes and spans E = S + 2 codes where the injective copy spans D.  The pair is built
// instead of the injective copy where it compares fewer planes over the blocks (option "rank_fold").  A third figure, S3,
// counts the values at least three samples hold.  The two-holder pair codes the values with exactly two holders like
// single-holder ones and spans E2 = S3 + 2 codes; what the compare then misses -- one match per such value, in one
// known pair -- the tile kernel adds back from an event list.  That costs three more small kernels, a second
// synchronisation and a fixed step per tile, so the default (option "rank_fold2" 1) takes it only where its plane sum is
// the lowest of the three AND the self job runs at least four rounds of tiles (a smaller job's time is its latency, not
// its compare stream).  Caps: at most five k, 8 planes, PPK_FOLD2_SLOTS two-holder values per position,
// PPK_FOLD2_MAX_PER_PAIR events per (pair, k); a database past any of them keeps the copies it would have had.
// The pass also leaves E2 of every position.  Counts and events do not depend on the order of a k's positions, so the
// two-holder pair stores them sorted by E2 (option "fold2_sort"): the wide positions share a few blocks and the rest
// compare 6 planes.  The choice among the codings does not look at the order: it keeps the sums over the stored blocks.
static int planes_for(unsigned codes) { return codes <= 256 ? 8 : codes <= 1024 ? 10 : codes <= 4096 ? 12 : 0; }
static bool flags_fit(size_t nk, size_t s64) { return nk < PPK_RANK_SHORT_WORDS && s64 <= 32; }
// The short flags of a coding in `planes` planes whose stored blocks span block_max[k * s64 + blk] codes, and the
// planes a self job compares over all blocks with it (no coding: bbits each)
static size_t short_flags(const unsigned *block_max, int planes, size_t nk, size_t s64, size_t bbits, unsigned *flags) {
  size_t sum = 0;
  for (size_t k = 0; k < nk; ++k)
    for (size_t b = 0; b < s64; ++b) {
      const bool is_short = planes && flags_fit(nk, s64) && block_max[k * s64 + b] <= (1u << (planes - 1));
      if (is_short) flags[k] |= 1u << b;
      sum += planes ? (size_t)(planes - (is_short ? 1 : 0)) : bbits;
    }
  return sum;
}
// Per k a stable sort of the positions by the codes they span, descending: ties keep their stored order.  Position i
// of k spans e[(k * nbins + i) * stride].
static void sort_by_span(const unsigned *e, size_t stride, size_t k, size_t nbins, bool sorted, unsigned *ord) {
  for (size_t i = 0; i < nbins; ++i) ord[i] = (unsigned)i;
  if (sorted)
    std::stable_sort(ord, ord + nbins, [&](unsigned a, unsigned b) { return e[(k * nbins + a) * stride] > e[(k * nbins + b) * stride]; });
}
// the widest position of block b of k's slots
static unsigned widest_of(const unsigned *e, size_t stride, size_t k, size_t nbins, const unsigned *ord, size_t b) {
  unsigned widest = 0;
  for (size_t i = 0; i < 64; ++i) widest = std::max(widest, e[(k * nbins + ord[b * 64 + i]) * stride]);
  return widest;
}
// the planes such a block streams of a pair that compares at most `top`: two fewer up to 2^(top - 2) codes, one up to 2^(top - 1)
static uint8_t stream_planes_for(unsigned widest, int top) {
  return (uint8_t)(widest <= (1u << (top - 2)) ? top - 2 : widest <= (1u << (top - 1)) ? top - 1 : top);
}
static void stream_flags(const uint8_t *stream, int top, size_t nk, size_t s64, unsigned *less1, unsigned *less2) {
  for (size_t k = 0; k < nk; ++k)
    for (size_t b = 0; b < s64; ++b) {
      if (stream[k * s64 + b] <= top - 1) less1[k] |= 1u << b;
      if (stream[k * s64 + b] <= top - 2) less2[k] |= 1u << b;
    }
}
static bool four_rounds(size_t n, int tile_slots) {
  const size_t npad = (n + PPK_NPAD - 1) / PPK_NPAD * PPK_NPAD;
  return (npad / 256) * (npad / 32) / 2 >= 4 * (size_t)tile_slots;
}

PpkCodingPlan ppk_plan_codings(const unsigned *counts, size_t n, size_t nk, size_t s64, size_t bbits, int tile_slots,
                               long long rank_fold, long long rank_fold2, long long fold2_sort, long long rank_foldh) {
  PpkCodingPlan pl = {};
  const size_t n_blocks = nk * s64, nbins = s64 * 64;
  const unsigned *extra = counts + 3 * (1 + n_blocks), *pos_e2 = extra + PPK_RANK_EXTRA;
  for (int c = 0; c < 3; ++c) {
    const unsigned *figure = counts + c * (1 + n_blocks);
    pl.planes[c] = planes_for(figure[0]);
    pl.sum[c] = short_flags(figure + 1, pl.planes[c], nk, s64, bbits, pl.less1[c]);
  }
  const size_t sum_d = pl.sum[0], sum_e = pl.sum[1], sum_e2 = pl.sum[2];
  const bool fold2_fits = pl.planes[2] == 8 && nk <= PPK_FOLD2_MAX_NK && extra[0] <= PPK_FOLD2_SLOTS && n < ((size_t)1 << 28);
  const bool fold2_pays = rank_fold != 0 && sum_e2 < sum_d && sum_e2 < (pl.planes[1] ? sum_e : (size_t)-1) && four_rounds(n, tile_slots);
  int *next = pl.chain;
  if (fold2_fits && rank_fold2 != 0 && (rank_fold2 == 2 || fold2_pays)) *next++ = PPK_CODING_FOLD2;
  if (pl.planes[1] && rank_fold != 0 && (rank_fold == 2 || sum_e < sum_d)) *next++ = PPK_CODING_FOLD;
  if (pl.planes[0]) *next++ = PPK_CODING_RANK;
  *next = -1;
  if (pl.chain[0] != PPK_CODING_FOLD2) return pl;
  pl.sorted = fold2_sort != 0;
  pl.order.resize(nk * nbins);
  pl.stream.resize(n_blocks);
  for (size_t k = 0; k < nk; ++k) {
    sort_by_span(pos_e2, 1, k, nbins, pl.sorted, pl.order.data() + k * nbins);
    for (size_t b = 0; b < s64; ++b) {
      // (shapes that keep no flags compare every block whole)
      pl.stream[k * s64 + b] = flags_fit(nk, s64) ? stream_planes_for(widest_of(pos_e2, 1, k, nbins, pl.order.data() + k * nbins, b), 8) : 8;
      pl.stream_sum += pl.stream[k * s64 + b];
    }
  }
  if (flags_fit(nk, s64)) stream_flags(pl.stream.data(), 8, nk, s64, pl.seven, pl.six);
  pl.try_holder = rank_foldh != 0 && flags_fit(nk, s64);
  return pl;
}

int ppk_holder_ladder(size_t n, size_t nk, size_t s64, size_t most_shared, long long foldh_holders, unsigned *ladder) {
  if (nk > PPK_FOLD2_MAX_NK || s64 > 32 || nk >= PPK_RANK_SHORT_WORDS || n >= ((size_t)1 << 24) || most_shared > PPK_FOLDH_SLOTS) return 0;
  for (int i = 0; i < PPK_FOLDH_LADDER; ++i) ladder[i] = 4u << i;
  if (foldh_holders > 0) ladder[0] = (unsigned)(foldh_holders < 65534 ? foldh_holders : 65534);
  return foldh_holders > 0 ? 1 : PPK_FOLDH_LADDER;
}
PpkHolderChoice ppk_choose_holder_impl(const unsigned *pos_e, const unsigned *ladder, int rungs, size_t n, size_t nk, size_t s64,
                                  int tile_slots, size_t fold2_sum, long long rank_foldh) {
  PpkHolderChoice c;
  const size_t nbins = s64 * 64;
  c.order.resize(nk * nbins);
  c.block_planes.resize(nk * s64);
  const bool take_any = rank_foldh == 2;
  for (int i = 0; i < rungs; ++i) {
    bool fits = true;
    size_t sum = 0;
    for (size_t k = 0; k < nk && fits; ++k) {
      unsigned *ord = c.order.data() + k * nbins;
      sort_by_span(pos_e + i, PPK_FOLDH_LADDER, k, nbins, true, ord);
      for (size_t b = 0; b < s64; ++b) {
        const unsigned widest = widest_of(pos_e + i, PPK_FOLDH_LADDER, k, nbins, ord, b);
        if (widest > PPK_FOLDH_MAX_CODES) fits = false;
        sum += c.block_planes[k * s64 + b] = stream_planes_for(widest, 4);
      }
    }
    if (fits && (take_any || (four_rounds(n, tile_slots) && sum * 10 <= fold2_sum * 6))) {
      c.H = ladder[i];
      const size_t pair_k = n * (n - 1) / 2 * nk;
      c.max_entries = take_any ? pair_k : pair_k / 16;
      return c;
    }
  }
  return c;
}

// The same two through the C ABI (tests on a machine without a GPU: nothing here touches a device)
extern "C" int ppk_choose_coding(const uint32_t *counts, size_t n_counts, size_t n, size_t nk, size_t sketchsize64, size_t bbits,
                                 int tile_slots, const long long *options, int *first, int *fallback, size_t *plane_sums,
                                 uint32_t *order, uint32_t *flags, uint8_t *stream_planes, size_t *stream_sum, int *try_holder) {
  if (!counts || !options || !first || !fallback || !plane_sums) return ppk_fail(PPK_ERR_ARG, "ppk_choose_coding: NULL argument");
  if (n < 1 || nk < 1 || sketchsize64 < 1 || tile_slots < 1 || n_counts != 3 * (1 + nk * sketchsize64) + PPK_RANK_EXTRA + nk * sketchsize64 * 64)
    return ppk_fail(PPK_ERR_ARG, "ppk_choose_coding: bad shape");
  const PpkCodingPlan pl = ppk_plan_codings(counts, n, nk, sketchsize64, bbits, tile_slots, options[0], options[1], options[2], options[3]);
  *first = pl.chain[0];
  *fallback = pl.chain[0] < 0 ? -1 : pl.chain[1];
  for (int c = 0; c < 3; ++c) plane_sums[c] = pl.sum[c];
  if (order) std::copy(pl.order.begin(), pl.order.end(), order);
  if (stream_planes) std::copy(pl.stream.begin(), pl.stream.end(), stream_planes);
  for (int k = 0; flags && k < PPK_RANK_SHORT_WORDS; ++k) flags[k] = pl.seven[k], flags[PPK_RANK_SHORT_WORDS + k] = pl.six[k];
  if (stream_sum) *stream_sum = pl.stream_sum;
  if (try_holder) *try_holder = pl.try_holder ? 1 : 0;
  return PPK_OK;
}
extern "C" int ppk_choose_holder(const uint32_t *pos_e, size_t n_pos_e, size_t n, size_t nk, size_t sketchsize64, int tile_slots,
                                 size_t most_shared, size_t fold2_sum, long long rank_foldh, long long foldh_holders,
                                 unsigned *holders, uint32_t *order, uint8_t *block_planes, size_t *max_entries) {
  if (!pos_e || !holders) return ppk_fail(PPK_ERR_ARG, "ppk_choose_holder: NULL argument");
  if (n < 1 || nk < 1 || sketchsize64 < 1 || tile_slots < 1 || n_pos_e != nk * sketchsize64 * 64 * PPK_FOLDH_LADDER)
    return ppk_fail(PPK_ERR_ARG, "ppk_choose_holder: bad shape");
  unsigned ladder[PPK_FOLDH_LADDER];
  const int rungs = rank_foldh != 0 ? ppk_holder_ladder(n, nk, sketchsize64, most_shared, foldh_holders, ladder) : 0;
  PpkHolderChoice c;
  if (rungs) c = ppk_choose_holder_impl(pos_e, ladder, rungs, n, nk, sketchsize64, tile_slots, fold2_sum, rank_foldh);
  *holders = c.H;
  if (c.H && order) std::copy(c.order.begin(), c.order.end(), order);
  if (c.H && block_planes) std::copy(c.block_planes.begin(), c.block_planes.end(), block_planes);
  if (max_entries) *max_entries = c.max_entries;
  return PPK_OK;
}

// ---- the execution ---------------------------------------------------------------------------------------------------
// The injective copy (one allocation for both sides) or the folded pair of `db` into `c`; enqueues.  A device too full
// leaves `c` without copies: they only buy speed, and the caller goes on to the next coding, at last the raw planes.
static int build_copies(const ppk_db *db, PpkCoding &c, int planes, hipStream_t s) {
  const size_t bytes = db->npad * db->nk * db->s64 * (size_t)planes * sizeof(uint64_t);
  const bool pair = c.kind == PPK_CODING_FOLD;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&c.d_ref), bytes);
  if (e == hipSuccess && pair) e = hipMalloc(reinterpret_cast<void **>(&c.d_qry), bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (c.d_ref) (void)hipFree(c.d_ref);
    c.d_ref = c.d_qry = nullptr;
    return PPK_OK;
  }
  if (!pair) c.d_qry = c.d_ref;
  return ppk_launch_rank_codes(db->d_skT, c.d_ref, pair ? c.d_qry : nullptr, db->n, db->npad, db->nk, db->s64, planes, s);
}
// The holder pair beside the two-holder pair (option "rank_foldh"), also where a (pair, k) had more events than the
// two-holder pair's field holds: its counts have no such cap.
static int try_holder(ppk_db *db, size_t most_shared, size_t fold2_sum, int tile_slots, hipStream_t s) {
  unsigned ladder[PPK_FOLDH_LADDER];
  const long long opt = ppk_config().rank_foldh.load();
  const int rungs = ppk_holder_ladder(db->n, db->nk, db->s64, most_shared, ppk_config().foldh_holders.load(), ladder);
  if (!rungs) return PPK_OK;
  unsigned *d_twice = nullptr;
  uint16_t *d_holders = nullptr;
  std::vector<unsigned> pos_e;
  int rc = ppk_foldh_count(db, ladder, &d_twice, &d_holders, &pos_e, s);
  if (rc != PPK_OK || pos_e.empty()) return rc;
  PpkHolderChoice choice = ppk_choose_holder_impl(pos_e.data(), ladder, rungs, db->n, db->nk, db->s64, tile_slots, fold2_sum, opt);
  if (choice.H) {
    PpkCoding &c = db->coding[PPK_CODING_FOLDH];
    c.order.swap(choice.order);
    rc = ppk_build_foldh(db, choice.H, d_twice, d_holders, choice.max_entries, s);
    if (rc == PPK_OK && c.planes) stream_flags(choice.block_planes.data(), 4, db->nk, db->s64, c.less1, c.less2);
  }
  (void)hipFree(d_twice);
  (void)hipFree(d_holders);
  return rc;
}

// Only a database whose self job runs whole tiles reads a coded copy (launch_v2), so only such a database pays for one.
// The count is read back: one synchronisation of `s` per database (the two-holder and holder pairs: one more each).
int ppk_db_build_codings(ppk_db *db, hipStream_t s) {
  if (!ppk_coding_enabled(PPK_CODING_RANK) || !ppk_self_job_takes_tiles(db)) return PPK_OK;
  const size_t n_blocks = db->nk * db->s64;
  std::vector<unsigned> counts(3 * (1 + n_blocks) + PPK_RANK_EXTRA + n_blocks * 64, 0u);      // (behind the figures: E2 per position)
  unsigned *d_max = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&d_max), counts.size() * sizeof(unsigned)) != hipSuccess) {
    (void)hipGetLastError();
    return PPK_OK;
  }
  int rc = ppk_launch_rank_count(db->d_skT, db->n, db->npad, db->nk, db->s64, d_max, s);
  if (rc == PPK_OK) {
    hipError_t e = hipMemcpyAsync(counts.data(), d_max, counts.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = ppk_fail(PPK_ERR_HIP, std::string("rank codes: ") + hipGetErrorString(e));
  }
  (void)hipFree(d_max);
  if (rc != PPK_OK) return rc;
  const PpkConfig &cfg = ppk_config();
  const int tile_slots = ppk_geometry(db->device).tile_slots;
  const PpkCodingPlan plan = ppk_plan_codings(counts.data(), db->n, db->nk, db->s64, db->bbits, tile_slots, cfg.rank_fold.load(),
                                              cfg.rank_fold2.load(), cfg.fold2_sort.load(), cfg.rank_foldh.load());
  unsigned *extra = counts.data() + 3 * (1 + n_blocks);      // most two-holder values of a position, all of them, cap hit
  bool built = false;
  for (const int *kind = plan.chain; rc == PPK_OK && !built && *kind >= 0; ++kind) {
    PpkCoding &c = db->coding[*kind];
    if (*kind == PPK_CODING_FOLD2) {
      bool overflow = false;
      rc = ppk_build_fold2(db, plan.planes[2], extra[1], plan.sorted ? &plan.order : nullptr, &overflow, s);
      extra[2] = overflow ? 1u : 0u;
      if (rc == PPK_OK && c.planes) {
        c.order = plan.order;
        std::copy(plan.seven, plan.seven + PPK_RANK_SHORT_WORDS, c.less1);
        std::copy(plan.six, plan.six + PPK_RANK_SHORT_WORDS, c.less2);
      }
      // (counts[1 + n_blocks] - 2: the most shared values of any position)
      if (rc == PPK_OK && plan.try_holder) rc = try_holder(db, counts[1 + n_blocks] - 2u, plan.stream_sum, tile_slots, s);
    } else {
      rc = build_copies(db, c, plan.planes[*kind], s);
      if (*kind == PPK_CODING_FOLD && c.d_ref) {
        c.planes = c.stream_planes = plan.planes[1];
        std::copy(plan.less1[1], plan.less1[1] + PPK_RANK_SHORT_WORDS, c.less1);
      }
    }
    built = c.d_ref != nullptr;      // (a holder pair beside a dropped two-holder pair leaves the next coding its turn)
  }
  // whatever was built, the injective copy's planes and flags are what the distinct values give
  bool any = false;
  for (const PpkCoding &c : db->coding) any = any || c.d_ref != nullptr;
  if (any) {
    PpkCoding &injective = db->coding[PPK_CODING_RANK];
    injective.planes = injective.stream_planes = plan.planes[0];
    std::copy(plan.less1[0], plan.less1[0] + PPK_RANK_SHORT_WORDS, injective.less1);
  }
  if (rc == PPK_OK) db->rank_counts.assign(counts.begin(), counts.begin() + 3 * (1 + n_blocks) + PPK_RANK_EXTRA);
  return rc;
}

// The injective copy of a database that was built with a pair alone: made when somebody asks for it
// (ppk_db_rank_read; a rectangular job of the handle against itself reads the raw planes until then).
static int ppk_db_build_injective(ppk_db *db) {
  PpkCoding &c = db->coding[PPK_CODING_RANK];
  if (c.d_ref) return PPK_OK;
  int rc = build_copies(db, c, c.planes, nullptr);
  if (rc == PPK_OK && !c.d_ref) return ppk_fail(PPK_ERR_HIP, "rank codes: the device has no room for the copy");
  hipError_t e = rc == PPK_OK ? hipDeviceSynchronize() : hipSuccess;
  if (rc == PPK_OK && e != hipSuccess) rc = ppk_fail(PPK_ERR_HIP, std::string("rank codes: ") + hipGetErrorString(e));
  if (rc != PPK_OK) {
    (void)hipFree(c.d_ref);
    c.d_ref = c.d_qry = nullptr;
  }
  return rc;
}

// ---- accessors: five helpers, one table of nouns -----------------------------------------------------------------------
static const char *const kNoun[PPK_CODINGS] = {"rank-coded copy", "folded pair", "two-holder pair", "holder pair"};
static const char *const kListNoun[PPK_CODINGS] = {"", "", "events (ppk_db_fold2_events)", "entries (ppk_db_foldh_entries)"};
static int fail_in(const char *fn, int code, const std::string &what) { return ppk_fail(code, std::string(fn) + ": " + what); }
// the argument and state checks every accessor opens with
static int coding_check(const char *fn, const ppk_db *db, const void *out, int kind, int which = 0) {
  if (!db || !out) return fail_in(fn, PPK_ERR_ARG, "NULL argument");
  if (which != 0 && which != 1) return fail_in(fn, PPK_ERR_ARG, "`which` is 0 (ref side) or 1 (query side)");
  if (!db->coding[kind].planes) return fail_in(fn, PPK_ERR_STATE, std::string("the database has no ") + kNoun[kind]);
  return PPK_OK;
}
static int coding_read(const char *fn, const ppk_db *db, int kind, int which, uint64_t *out, size_t words) {
  if (int rc = coding_check(fn, db, out, kind, which)) return rc;
  const PpkCoding &c = db->coding[kind];
  if (words != db->nk * db->s64 * (size_t)c.chunk_planes() * db->npad)
    return fail_in(fn, PPK_ERR_ARG, std::string("`words` is not nk * sketchsize64 * ") + (kind == PPK_CODING_FOLDH ? "chunk planes" : "planes") + " * padded samples");
  PPK_ENTER_DEVICE(guard, db->device);
  PPK_HIP(hipDeviceSynchronize());
  if (kind == PPK_CODING_RANK)
    if (int rc = ppk_db_build_injective(const_cast<ppk_db *>(db))) return rc;
  PPK_HIP(hipMemcpy(out, which ? c.d_qry : c.d_ref, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return PPK_OK;
}
// the planes of the STORED blocks under the coding's short rule: a function of the count pass's per-block maxima
// (figure `kind` of rank_counts: D, E, E2) and the planes
static int coding_block_planes(const char *fn, const ppk_db *db, int kind, uint8_t *out, size_t cap) {
  if (int rc = coding_check(fn, db, out, kind)) return rc;
  if (cap < db->nk * db->s64) return fail_in(fn, PPK_ERR_ARG, "`cap` is below nk * sketchsize64");
  unsigned flags[PPK_RANK_SHORT_WORDS] = {};
  const int planes = db->coding[kind].planes;
  short_flags(db->rank_counts.data() + kind * (1 + db->nk * db->s64) + 1, planes, db->nk, db->s64, db->bbits, flags);
  for (size_t k = 0; k < db->nk; ++k)
    for (size_t b = 0; b < db->s64; ++b) {
      const bool is_short = k < PPK_RANK_SHORT_WORDS && b < 32 && ((flags[k] >> b) & 1u);
      out[k * db->s64 + b] = (uint8_t)(planes - (is_short ? 1 : 0));
    }
  return PPK_OK;
}
// the planes a self job compares per block of slots under the launch options
static int coding_stream_planes(const char *fn, const ppk_db *db, int kind, uint8_t *out, size_t cap) {
  if (int rc = coding_check(fn, db, out, kind)) return rc;
  if (cap < db->nk * db->s64) return fail_in(fn, PPK_ERR_ARG, "`cap` is below nk * sketchsize64");
  const PpkCoding &c = db->coding[kind];
  unsigned less1[PPK_RANK_SHORT_WORDS], less2[PPK_RANK_SHORT_WORDS];
  ppk_coding_launch_flags(c, less1, less2);
  for (size_t k = 0; k < db->nk; ++k)
    for (size_t b = 0; b < db->s64; ++b) {
      const bool fits = k < PPK_RANK_SHORT_WORDS && b < 32;
      const bool one = fits && ((less1[k] >> b) & 1u), two = fits && ((less2[k] >> b) & 1u);
      out[k * db->s64 + b] = (uint8_t)(c.stream_planes - (two ? 2 : one ? 1 : 0));
    }
  return PPK_OK;
}
static int coding_position_order(const char *fn, const ppk_db *db, int kind, uint32_t *out, size_t cap) {
  if (int rc = coding_check(fn, db, out, kind)) return rc;
  const std::vector<unsigned> &order = db->coding[kind].order;
  if (cap < order.size()) return fail_in(fn, PPK_ERR_ARG, "`cap` is below nk * 64 * sketchsize64");
  std::copy(order.begin(), order.end(), out);
  return PPK_OK;
}
static size_t coding_list_size(const ppk_db *db, int kind, size_t *n_buckets) {
  const PpkCoding *c = db && db->coding[kind].planes ? &db->coding[kind] : nullptr;
  if (n_buckets) *n_buckets = c ? (size_t)c->qt * c->rt : 0;
  return c ? c->list_count : 0;
}
static int coding_list_read(const char *fn, const ppk_db *db, int kind, uint32_t *off, size_t n_off, void *list, size_t n_list) {
  if (int rc = coding_check(fn, db, off, kind)) return rc;
  const PpkCoding &c = db->coding[kind];
  if (n_off != (size_t)c.qt * c.rt + 1 || n_list != c.list_count || (n_list && !list))
    return fail_in(fn, PPK_ERR_ARG, std::string("sizes are buckets + 1 and ") + kListNoun[kind]);
  PPK_ENTER_DEVICE(guard, db->device);
  PPK_HIP(hipDeviceSynchronize());
  PPK_HIP(hipMemcpy(off, c.d_off, n_off * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_list) PPK_HIP(hipMemcpy(list, c.d_list, n_list * c.list_elem, hipMemcpyDeviceToHost));
  return PPK_OK;
}

extern "C" int ppk_db_rank_planes(const ppk_db *db) { return db ? db->coding[PPK_CODING_RANK].planes : 0; }
extern "C" int ppk_db_rank_read(const ppk_db *db, uint64_t *out, size_t words) { return coding_read(__func__, db, PPK_CODING_RANK, 0, out, words); }
extern "C" int ppk_db_rank_block_planes(const ppk_db *db, uint8_t *out, size_t cap) { return coding_block_planes(__func__, db, PPK_CODING_RANK, out, cap); }
extern "C" size_t ppk_db_rank_counts(const ppk_db *db, uint32_t *out, size_t cap) {
  if (!db) return 0;
  if (out && cap >= db->rank_counts.size()) std::copy(db->rank_counts.begin(), db->rank_counts.end(), out);
  return db->rank_counts.size();
}
extern "C" int ppk_db_fold_planes(const ppk_db *db) { return db ? db->coding[PPK_CODING_FOLD].planes : 0; }
extern "C" int ppk_db_fold_read(const ppk_db *db, int which, uint64_t *out, size_t words) { return coding_read(__func__, db, PPK_CODING_FOLD, which, out, words); }
extern "C" int ppk_db_fold_block_planes(const ppk_db *db, uint8_t *out, size_t cap) { return coding_block_planes(__func__, db, PPK_CODING_FOLD, out, cap); }
extern "C" int ppk_db_fold2_planes(const ppk_db *db) { return db ? db->coding[PPK_CODING_FOLD2].planes : 0; }
extern "C" int ppk_db_fold2_read(const ppk_db *db, int which, uint64_t *out, size_t words) { return coding_read(__func__, db, PPK_CODING_FOLD2, which, out, words); }
extern "C" int ppk_db_fold2_block_planes(const ppk_db *db, uint8_t *out, size_t cap) { return coding_block_planes(__func__, db, PPK_CODING_FOLD2, out, cap); }
extern "C" int ppk_db_fold2_stream_planes(const ppk_db *db, uint8_t *out, size_t cap) { return coding_stream_planes(__func__, db, PPK_CODING_FOLD2, out, cap); }
extern "C" int ppk_db_fold2_position_order(const ppk_db *db, uint32_t *out, size_t cap) { return coding_position_order(__func__, db, PPK_CODING_FOLD2, out, cap); }
extern "C" size_t ppk_db_fold2_events(const ppk_db *db, size_t *n_buckets) { return coding_list_size(db, PPK_CODING_FOLD2, n_buckets); }
extern "C" int ppk_db_fold2_events_read(const ppk_db *db, uint32_t *off, size_t n_off, uint16_t *ev, size_t n_ev) {
  return coding_list_read(__func__, db, PPK_CODING_FOLD2, off, n_off, ev, n_ev);
}
extern "C" unsigned ppk_db_foldh_holders(const ppk_db *db) { return db ? db->coding[PPK_CODING_FOLDH].holders : 0u; }
extern "C" int ppk_db_foldh_chunk_planes(const ppk_db *db) { return db ? db->coding[PPK_CODING_FOLDH].chunk_planes() : 0; }
extern "C" int ppk_db_foldh_read(const ppk_db *db, int which, uint64_t *out, size_t words) { return coding_read(__func__, db, PPK_CODING_FOLDH, which, out, words); }
extern "C" int ppk_db_foldh_stream_planes(const ppk_db *db, uint8_t *out, size_t cap) { return coding_stream_planes(__func__, db, PPK_CODING_FOLDH, out, cap); }
extern "C" int ppk_db_foldh_position_order(const ppk_db *db, uint32_t *out, size_t cap) { return coding_position_order(__func__, db, PPK_CODING_FOLDH, out, cap); }
extern "C" size_t ppk_db_foldh_entries(const ppk_db *db, size_t *n_buckets) { return coding_list_size(db, PPK_CODING_FOLDH, n_buckets); }
extern "C" int ppk_db_foldh_entries_read(const ppk_db *db, uint32_t *off, size_t n_off, uint32_t *ent, size_t n_ent) {
  return coding_list_read(__func__, db, PPK_CODING_FOLDH, off, n_off, ent, n_ent);
}
