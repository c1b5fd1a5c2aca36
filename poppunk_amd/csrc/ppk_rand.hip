// The sums of the contingency table between every level of one family of clusterings and every level of another,
// from which the Rand and adjusted Rand indices follow on the host.
//
//  - ppk_contingency_sums_dev : scripts/poppunk_calculate_rand_indices.py makes one sklearn call per pair of files (a
//    sparse contingency matrix each).  Here every quantity is an integer sum: per level the squared class sizes and
//    the number of labels, per pair of levels the squared cell sizes and the number of non-empty cells.  Integer
//    addition is associative, so the results are the same bits whatever route a segment takes and in whatever order
//    the partial sums land; there is no floating point on the device.
//    Stages (ppk_prof_stages names):
//      levels  once per level of either side: every label against [1, n] and the class histogram (the only global
//              atomics of the call, with the grouping below); one workgroup per level scans the histogram into segment
//              starts and dense ranks (labels in ascending order -> 0 .. K - 1), adds the squared sizes and lists the
//              classes longer than the wave route takes; every sample gets its dense rank, and the sample indices are
//              grouped by label (`order`).  The call's ONE synchronisation reads the first bad label and every level's
//              K and list length here: the host sizes the pair stage's grids from them.
//      pairs   per pair (x, y), in batches that keep the partial sums under the cap.  The level with more labels gives
//              the segments (its classes, contiguous in `order`), the other the ranks: sum n_ij^2 = the sum over samples
//              s of |{t in s's segment : rank_t = rank_s}|, and a cell is counted at its first sample.
//                wave    segments of up to rand_wave_max samples: one lane per sample; the ranks of the members that lie
//                        in the lane's own wave come through the cross-lane network, the others from memory
//                table   longer segments: a workgroup per (segment, window of ranks) counts the segment's ranks in an
//                        LDS table (integer LDS atomics): a member that finds `old` of its cell there before it adds
//                        2 * old + 1, which over a cell of v members is v^2, so the table is never read back; one
//                        window where the rank side has up to 8 192 labels
//              Every workgroup leaves one pair of 64-bit partial sums; `reduce` adds a pair's partials into its cell
//              of the two output matrices (both cells where B = A).
#include <string>
#include <vector>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;
constexpr int kTableThreads = 512;
constexpr int kTableItems = 4;
constexpr int kTableMax = 8192;        // int32 slots of the rank table (32 KiB: four workgroups per CU)
constexpr size_t kTableGrid = 4096;    // workgroups per pair the table route is given at most
constexpr int kMaxLevels = 1023;
constexpr unsigned kMaxGridY = 65535;

// what every kernel of the call reads: levels are numbered A's first, then B's (none where B = A)
struct RandArgs {
  const int32_t *a, *b;
  size_t n;
  int n_a, n_b, self;
  int32_t *ends;         // [levels][n + 1]: the histogram, then segment starts, then (after the grouping) segment ends:
                         // the samples of label c are order[ends[c - 1] .. ends[c])
  int32_t *order;        // [levels][n + 1]: dense rank by label until the grouping, then the sample indices by label
  int32_t *dense;        // [levels][n]: dense rank by sample
  int32_t *info;         // [levels][2]: K, entries of the level's list of long classes
  int32_t *big;          // [levels][big_cap]: the labels of the classes longer than wave_max
  size_t big_cap;
  int wave_max, window, no_windows;
};

__device__ __forceinline__ const int32_t *rand_level(const RandArgs &A, int g) {
  return g < A.n_a ? A.a + (size_t)g * A.n : A.b + (size_t)(g - A.n_a) * A.n;
}

// pair q -> (x, y): the rectangle row by row, or the triangle x < y where B = A
__host__ __device__ inline void rand_pair_xy(size_t q, int n_a, int n_b, int self, int *x, int *y) {
  if (!self) {
    *x = (int)(q / (size_t)n_b);
    *y = (int)(q % (size_t)n_b);
    return;
  }
  int r = 0;
  size_t left = q;
  while (left >= (size_t)(n_a - 1 - r)) {
    left -= (size_t)(n_a - 1 - r);
    ++r;
  }
  *x = r;
  *y = r + 1 + (int)left;
}

// the side that gives the segments (more labels; x on a tie), the side that gives the ranks, the rank windows
__host__ __device__ inline void rand_orient(int gx, int gy, int kx, int ky, int window, int *seg, int *tab,
                                            int *windows) {
  const bool y_seg = ky > kx;
  *seg = y_seg ? gy : gx;
  *tab = y_seg ? gx : gy;
  const int kt = y_seg ? kx : ky;
  *windows = kt > 0 ? (kt + window - 1) / window : 1;
}

__device__ __forceinline__ void rand_pair(const RandArgs &A, size_t q, int *seg, int *tab, int *windows) {
  int x, y;
  rand_pair_xy(q, A.n_a, A.n_b, A.self, &x, &y);
  const int gx = x, gy = A.self ? y : A.n_a + y;
  rand_orient(gx, gy, A.info[2 * gx], A.info[2 * gy], A.window, seg, tab, windows);
}

// adds (u, v) over the workgroup; thread 0 stores the pair at out[0], out[1]
template <int THREADS>
__device__ __forceinline__ void rand_block_store(long long u, long long v, long long *out) {
  __shared__ long long s_part[2 * (THREADS / 64)];
  u = wave_sum_all(u);
  v = wave_sum_all(v);
  if ((threadIdx.x & 63) == 0) {
    s_part[2 * (threadIdx.x >> 6)] = u;
    s_part[2 * (threadIdx.x >> 6) + 1] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long su = 0, sv = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      su += s_part[2 * w];
      sv += s_part[2 * w + 1];
    }
    out[0] = su;
    out[1] = sv;
  }
}

// Every lane of the wave calls this; key < 0: nothing to take.  Each lane takes one place in counter[key] and gets
// the counter's value before it; the lanes that share the first pending lane's key take theirs with one atomic (two
// rounds, as ps_wave_add of ppk_clusters.hip: a coarse level has a few labels and every sample adds to one of them),
// the rest lane by lane.
__device__ __forceinline__ int rand_wave_take(int32_t *counter, long long key) {
  const int lane = threadIdx.x & 63;
  int at = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const unsigned long long pend = __ballot(key >= 0);
    if (!pend) return at;                // (wave-uniform)
    const int leader = __ffsll((long long)pend) - 1;
    const long long k0 = __shfl(key, leader);
    const bool mine = key == k0;
    const unsigned long long group = __ballot(mine);
    int base = 0;
    if (lane == leader) base = atomicAdd(&counter[k0], __popcll(group));
    base = __shfl(base, leader);
    if (mine) {
      at = base + __popcll(group & ((1ull << lane) - 1));
      key = -1;
    }
  }
  if (key >= 0) at = atomicAdd(&counter[key], 1);
  return at;
}

// ends zeroed by the caller.  (The loops of the three per-sample kernels advance a whole workgroup at a time, so that
// every lane of a wave is there for the cross-lane steps.)
__global__ void __launch_bounds__(kThreads) rand_hist_kernel(RandArgs A, size_t count, unsigned long long *bad) {
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < count; base += (size_t)gridDim.x * blockDim.x) {
    const size_t k = base + threadIdx.x;
    long long key = -1;
    if (k < count) {
      const size_t g = k / A.n;
      const long long c = rand_level(A, (int)g)[k % A.n];
      if (c < 1 || c > (long long)A.n) atomicMin(bad, (unsigned long long)k);
      else key = (long long)(g * (A.n + 1) + (size_t)c);
    }
    (void)rand_wave_take(A.ends, key);
  }
}

// one workgroup per level: histogram -> segment starts (in place) and dense ranks; K, the squared sizes, the long classes
__global__ void __launch_bounds__(kScanThreads) rand_scan_kernel(RandArgs A, long long *sq_a, long long *sq_b,
                                                                 int32_t *labels_a, int32_t *labels_b) {
  __shared__ int s_start[kScanThreads / 64], s_rank[kScanThreads / 64];
  __shared__ int s_big;
  const int g = blockIdx.x;
  int32_t *ends = A.ends + (size_t)g * (A.n + 1);
  int32_t *rank = A.order + (size_t)g * (A.n + 1);
  int32_t *big = A.big + (size_t)g * A.big_cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_big = 0;
  int run_start = 0, run_rank = 0;       // (workgroup-uniform) the samples and the labels before this chunk
  long long sq = 0;
  for (size_t base = 1; base <= A.n; base += (size_t)kScanThreads * kScanItems) {
    const size_t c0 = base + (size_t)threadIdx.x * kScanItems;
    int cnt[kScanItems];
    int my_start = 0, my_rank = 0;
#pragma unroll
    for (int e = 0; e < kScanItems; ++e) {
      cnt[e] = c0 + e <= A.n ? ends[c0 + e] : 0;
      my_start += cnt[e];
      my_rank += cnt[e] > 0;
    }
    int inc_start = my_start, inc_rank = my_rank;      // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int us = __shfl_up(inc_start, o), ur = __shfl_up(inc_rank, o);
      if (lane >= o) {
        inc_start += us;
        inc_rank += ur;
      }
    }
    __syncthreads();                                   // (the totals of the chunk before have been read)
    if (lane == 63) {
      s_start[wave] = inc_start;
      s_rank[wave] = inc_rank;
    }
    __syncthreads();
    int at_start = run_start + inc_start - my_start, at_rank = run_rank + inc_rank - my_rank;
    int tot_start = 0, tot_rank = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
      if (w < wave) {
        at_start += s_start[w];
        at_rank += s_rank[w];
      }
      tot_start += s_start[w];
      tot_rank += s_rank[w];
    }
    run_start += tot_start;
    run_rank += tot_rank;
#pragma unroll
    for (int e = 0; e < kScanItems; ++e)
      if (c0 + e <= A.n) {
        ends[c0 + e] = at_start;
        if (cnt[e] > 0) {
          rank[c0 + e] = at_rank++;
          sq += (long long)cnt[e] * cnt[e];
          if (cnt[e] > A.wave_max) {
            const int slot = atomicAdd(&s_big, 1);
            if ((size_t)slot < A.big_cap) big[slot] = (int32_t)(c0 + e);
          }
        }
        at_start += cnt[e];
      }
  }
  __syncthreads();
  __shared__ long long s_sq[2];
  rand_block_store<kScanThreads>(sq, 0, s_sq);
  __syncthreads();
  if (threadIdx.x == 0) {
    A.info[2 * g] = run_rank;
    A.info[2 * g + 1] = s_big;
    if (g < A.n_a) {
      sq_a[g] = s_sq[0];
      labels_a[g] = run_rank;
      if (A.self && sq_b) sq_b[g] = s_sq[0];
      if (A.self && labels_b) labels_b[g] = run_rank;
    } else {
      sq_b[g - A.n_a] = s_sq[0];
      labels_b[g - A.n_a] = run_rank;
    }
  }
}

// a label outside [1, n] indexes nothing: the call fails on it after these have run
__global__ void __launch_bounds__(kThreads) rand_dense_kernel(RandArgs A, size_t count) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(k / A.n);
    const long long c = rand_level(A, g)[k % A.n];
    if (c >= 1 && c <= (long long)A.n) A.dense[k] = A.order[(size_t)g * (A.n + 1) + (size_t)c];
  }
}

// (after rand_dense_kernel: `order` stops holding ranks here)
__global__ void __launch_bounds__(kThreads) rand_group_kernel(RandArgs A, size_t count) {
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < count; base += (size_t)gridDim.x * blockDim.x) {
    const size_t k = base + threadIdx.x;
    const size_t g = k / A.n, s = k % A.n;
    long long key = -1;
    if (k < count) {
      const long long c = rand_level(A, (int)g)[s];
      if (c >= 1 && c <= (long long)A.n) key = (long long)(g * (A.n + 1) + (size_t)c);
    }
    const int pos = rand_wave_take(A.ends, key);
    if (key >= 0 && pos >= 0 && (size_t)pos < A.n) A.order[g * (A.n + 1) + (size_t)pos] = (int32_t)s;
  }
}

// grid: (n / 256 blocks of positions of the segment side's order) x (pairs of the batch)
__global__ void __launch_bounds__(kThreads) rand_wave_kernel(RandArgs A, size_t q0, long long *partial,
                                                             size_t stride) {
  int seg, tab, windows;
  rand_pair(A, q0 + blockIdx.y, &seg, &tab, &windows);
  const int32_t *ends = A.ends + (size_t)seg * (A.n + 1);
  const int32_t *order = A.order + (size_t)seg * (A.n + 1);
  const int32_t *ranks = A.dense + (size_t)tab * A.n;
  const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long long w0 = (long long)p - lane;
  long long a = 0, b = 0;
  int mine = -1;
  bool active = false;
  if (p < A.n) {
    const int32_t s = order[p];
    const int32_t c = rand_level(A, seg)[s];
    a = ends[c - 1];
    b = ends[c];
    mine = ranks[s];
    active = b - a <= (long long)A.wave_max || (A.no_windows && windows > 1);
  }
  int longest = active ? (int)(b - a) : 0;             // (wave-uniform after the rounds)
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(longest, o);
    longest = other > longest ? other : longest;
  }
  int same = 0, earlier = 0;
  for (int k = 0; k < longest; ++k) {
    const long long t = a + k;
    const bool valid = active && t < b;
    const long long src = t - w0;
    const bool in_wave = valid && src >= 0 && src < 64;
    int v = __shfl(mine, in_wave ? (int)src : lane);   // every lane of the wave takes part
    if (valid && !in_wave) v = ranks[order[t]];
    if (valid && v == mine) {
      ++same;
      earlier += t < (long long)p;
    }
  }
  rand_block_store<kThreads>(active ? same : 0, active && earlier == 0 ? 1 : 0,
                             partial + ((size_t)blockIdx.y * stride + blockIdx.x) * 2);
}

// grid: (up to kTableGrid workgroups, each taking the pair's (long class, window) units in turn) x (pairs of the
// batch); slot: behind the wave route's partials.  A member that finds `old` members of its cell before it adds
// 2 * old + 1 -- over a cell of v members that is v^2 -- and the one that finds none counts the cell, so the table is
// never read back: a unit costs its members and the zeroing of its window.
__global__ void __launch_bounds__(kTableThreads) rand_table_kernel(RandArgs A, size_t q0, long long *partial,
                                                                   size_t stride, size_t first) {
  __shared__ __attribute__((aligned(16))) int32_t table[kTableMax];
  int seg, tab, windows;
  rand_pair(A, q0 + blockIdx.y, &seg, &tab, &windows);
  // (workgroup-uniform) none where the wave route has taken the pair's long classes
  const size_t units = A.no_windows && windows > 1 ? 0 : (size_t)A.info[2 * seg + 1] * (size_t)windows;
  const int32_t *ends = A.ends + (size_t)seg * (A.n + 1);
  const int32_t *order = A.order + (size_t)seg * (A.n + 1);
  const int32_t *ranks = A.dense + (size_t)tab * A.n;
  const int n_ranks = A.info[2 * tab];
  long long sum = 0, cells = 0;
  for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int32_t c = A.big[(size_t)seg * A.big_cap + u / (size_t)windows];
    const int r0 = (int)(u % (size_t)windows) * A.window;
    const long long a = ends[c - 1], b = ends[c];
    const int wlen = n_ranks - r0 < A.window ? n_ranks - r0 : A.window;
    for (int k = threadIdx.x * 4; k < wlen; k += kTableThreads * 4)       // (kTableMax is a multiple of 4)
      *reinterpret_cast<int4 *>(&table[k]) = make_int4(0, 0, 0, 0);
    __syncthreads();
    // four members per thread and round: the index loads, then the rank loads, are in flight together
    for (long long base = a + threadIdx.x; base < b; base += (long long)kTableThreads * kTableItems) {
      int32_t member[kTableItems];
      int key[kTableItems];
#pragma unroll
      for (int e = 0; e < kTableItems; ++e) {
        const long long t = base + (long long)e * kTableThreads;
        member[e] = t < b ? order[t] : -1;
      }
#pragma unroll
      for (int e = 0; e < kTableItems; ++e) key[e] = member[e] >= 0 ? ranks[member[e]] - r0 : -1;
#pragma unroll
      for (int e = 0; e < kTableItems; ++e)
        if (key[e] >= 0 && key[e] < wlen) {
          const long long old = atomicAdd(&table[key[e]], 1);
          sum += 2 * old + 1;
          cells += old == 0;
        }
    }
    __syncthreads();                     // (the next unit zeroes the table)
  }
  rand_block_store<kTableThreads>(sum, cells, partial + ((size_t)blockIdx.y * stride + first + blockIdx.x) * 2);
}

// one workgroup per pair of the batch
__global__ void __launch_bounds__(kThreads) rand_reduce_kernel(RandArgs A, size_t q0, const long long *partial,
                                                               size_t stride, size_t used, long long *sq_cells,
                                                               long long *n_cells) {
  __shared__ long long s_out[2];
  const long long *mine = partial + (size_t)blockIdx.x * stride * 2;
  long long sum = 0, cells = 0;
  for (size_t k = threadIdx.x; k < used; k += kThreads) {
    sum += mine[2 * k];
    cells += mine[2 * k + 1];
  }
  rand_block_store<kThreads>(sum, cells, s_out);
  __syncthreads();
  if (threadIdx.x == 0) {
    int x, y;
    rand_pair_xy(q0 + blockIdx.x, A.n_a, A.n_b, A.self, &x, &y);
    sq_cells[(size_t)x * A.n_b + y] = s_out[0];
    n_cells[(size_t)x * A.n_b + y] = s_out[1];
    if (A.self) {
      sq_cells[(size_t)y * A.n_b + x] = s_out[0];
      n_cells[(size_t)y * A.n_b + x] = s_out[1];
    }
  }
}

// B = A: a level against itself has its classes for cells
__global__ void __launch_bounds__(kThreads) rand_diag_kernel(RandArgs A, const long long *sq_a, long long *sq_cells,
                                                             long long *n_cells) {
  const int x = blockIdx.x * kThreads + threadIdx.x;
  if (x < A.n_a) {
    sq_cells[(size_t)x * A.n_a + x] = sq_a[x];
    n_cells[(size_t)x * A.n_a + x] = A.info[2 * x];
  }
}

const char *kWho = "ppk_contingency_sums";

// the argument errors that need no device
int rand_check_args(const void *a, size_t n_a, const void *b, size_t n_b, size_t n, const void *sq_a, const void *sq_b,
                    const void *labels_a, const void *labels_b, const void *sq_cells, const void *n_cells) {
  const std::string who = kWho;
  if (!a || !sq_a || !labels_a || !sq_cells || !n_cells || (b && (!sq_b || !labels_b)))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (n == 0) return ppk_fail(PPK_ERR_ARG, who + ": n must be at least 1");
  if (n > (size_t)0x7ffffffe) return ppk_fail(PPK_ERR_ARG, who + ": n must be below 2^31 - 1");
  if (n_a == 0 || n_a > (size_t)kMaxLevels || (b && (n_b == 0 || n_b > (size_t)kMaxLevels)))
    return ppk_fail(PPK_ERR_ARG, who + ": n_a and n_b must be 1 .. 1023");
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_contingency_sums_dev(const int32_t *d_a, size_t n_a, const int32_t *d_b, size_t n_b, size_t n,
                                        long long *d_sq_a, long long *d_sq_b, int32_t *d_labels_a,
                                        int32_t *d_labels_b, long long *d_sq_cells, long long *d_n_cells,
                                        void *stream) {
  const std::string who = kWho;
  int rc = rand_check_args(d_a, n_a, d_b, n_b, n, d_sq_a, d_sq_b, d_labels_a, d_labels_b, d_sq_cells, d_n_cells);
  if (rc != PPK_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  const int self = d_b ? 0 : 1;
  if (self) n_b = n_a;
  const size_t levels = self ? n_a : n_a + n_b;
  const size_t n_pairs = self ? n_a * (n_a - 1) / 2 : n_a * n_b;

  // routing: a segment of up to wave_max samples goes lane by lane, a longer one through the rank table
  long long wave_max = ppk_config().rand_wave_max.load();
  if (wave_max < 0) wave_max = 0;
  if (wave_max > 0x7fffffff) wave_max = 0x7fffffff;
  long long window = ppk_config().rand_window.load();
  const int no_windows = window < 0 ? 1 : 0;
  if (window < 1 || window > kTableMax) window = kTableMax;
  const size_t big_cap = n / ((size_t)wave_max + 1) + 1;       // classes of more than wave_max samples, and one

  // the per-level state is laid out first (size known); the partial sums, in a slot of their own, once the levels have
  // been read
  RandArgs A{};
  A.a = d_a;
  A.b = d_b;
  A.n = n;
  A.n_a = (int)n_a;
  A.n_b = (int)n_b;
  A.self = self;
  A.big_cap = big_cap;
  A.wave_max = (int)wave_max;
  A.window = (int)window;
  A.no_windows = no_windows;
  const size_t wave_blocks = (n + kThreads - 1) / kThreads;
  unsigned long long *bad;
  long long *partial = nullptr;
  size_t batch = 1, stride = wave_blocks;
  size_t state_bytes = 0;
  rc = ppk_scratch_carve(dev, SLOT_RAND, [&](Carve &c) {
    c.take(bad, 1).take(A.info, 2 * levels).take(A.ends, levels * (n + 1)).take(A.order, levels * (n + 1))
        .take(A.dense, levels * n).take(A.big, levels * big_cap);
    state_bytes = c.at;
  });
  if (rc != PPK_OK) return rc;

  ppk_prof_stage("levels", s);
  const size_t count = levels * n;
  const unsigned level_grid = grid_for(count, kThreads * 4, 4096);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  PPK_HIP(hipMemsetAsync(A.ends, 0, levels * (n + 1) * sizeof(int32_t), s));
  hipLaunchKernelGGL(rand_hist_kernel, dim3(level_grid), dim3(kThreads), 0, s, A, count, bad);
  hipLaunchKernelGGL(rand_scan_kernel, dim3((unsigned)levels), dim3(kScanThreads), 0, s, A, d_sq_a, d_sq_b,
                     d_labels_a, d_labels_b);
  hipLaunchKernelGGL(rand_dense_kernel, dim3(level_grid), dim3(kThreads), 0, s, A, count);
  hipLaunchKernelGGL(rand_group_kernel, dim3(level_grid), dim3(kThreads), 0, s, A, count);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 8}, {A.info, levels * 8}}, &h);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    const size_t k = (size_t)h[0], g = k / n;
    const bool in_a = g < n_a;
    int32_t c = 0;
    PPK_HIP(hipMemcpy(&c, in_a ? d_a + k : d_b + (k - n_a * n), 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": side " + (in_a ? "a" : "b") + ", level " + std::to_string(in_a ? g : g - n_a) +
                                     ", sample " + std::to_string(k % n) + ": label " + std::to_string(c) +
                                     " outside [1, " + std::to_string(n) + "]");
  }
  std::vector<int> labels(levels), n_big(levels);
  for (size_t g = 0; g < levels; ++g) {
    labels[g] = (int)(h[1 + g] & 0xffffffffull);
    n_big[g] = (int)(h[1 + g] >> 32);
  }
  // the workgroups rand_table_kernel needs for a pair: one per (long class, window) unit, as it counts them
  auto units_of = [&](size_t q) -> size_t {
    int x, y, seg, tab, windows;
    rand_pair_xy(q, (int)n_a, (int)n_b, self, &x, &y);
    const int gx = x, gy = self ? y : (int)n_a + y;
    rand_orient(gx, gy, labels[gx], labels[gy], (int)window, &seg, &tab, &windows);
    const size_t units = no_windows && windows > 1 ? 0 : (size_t)n_big[seg] * (size_t)windows;
    return units < kTableGrid ? units : kTableGrid;    // (the workgroups that take them in turn)
  };
  size_t most_units = 0;
  for (size_t q = 0; q < n_pairs; ++q) {
    const size_t u = units_of(q);
    if (u > most_units) most_units = u;
  }

  if (self) {
    hipLaunchKernelGGL(rand_diag_kernel, dim3(grid_for(n_a, kThreads, 4)), dim3(kThreads), 0, s, A, d_sq_a, d_sq_cells,
                       d_n_cells);
  }
  if (n_pairs > 0) {
    // a batch: as many pairs as keep the state and the partial sums within four fifths of the cap (a scratch slot is
    // allocated with a quarter to spare, and the cap is on what is allocated); at least one
    stride = wave_blocks + most_units;
    const long long cap_mb = ppk_config().rand_scratch_mb.load();
    const size_t room = ((size_t)(cap_mb > 0 ? cap_mb : 0) << 20) / 5 * 4;
    batch = room > state_bytes ? (room - state_bytes) / (stride * 2 * sizeof(long long)) : 0;
    if (const long long force = ppk_config().rand_batch.load(); force > 0) batch = (size_t)force;
    if (batch < 1) batch = 1;
    if (batch > n_pairs) batch = n_pairs;
    if (batch > kMaxGridY) batch = kMaxGridY;
    rc = ppk_scratch_carve(dev, SLOT_RAND_SUMS, [&](Carve &c) { c.take(partial, batch * stride * 2); });
    if (rc != PPK_OK) return rc;
    for (size_t q0 = 0; q0 < n_pairs; q0 += batch) {
      const size_t q1 = q0 + batch < n_pairs ? q0 + batch : n_pairs;
      size_t units = 0;
      for (size_t q = q0; q < q1; ++q) {
        const size_t u = units_of(q);
        if (u > units) units = u;
      }
      ppk_prof_stage("wave", s);
      hipLaunchKernelGGL(rand_wave_kernel, dim3((unsigned)wave_blocks, (unsigned)(q1 - q0)), dim3(kThreads), 0, s, A, q0,
                         partial, stride);
      if (units > 0) {
        ppk_prof_stage("table", s);
        hipLaunchKernelGGL(rand_table_kernel, dim3((unsigned)units, (unsigned)(q1 - q0)), dim3(kTableThreads), 0, s, A,
                           q0, partial, stride, wave_blocks);
      }
      ppk_prof_stage("reduce", s);
      hipLaunchKernelGGL(rand_reduce_kernel, dim3((unsigned)(q1 - q0)), dim3(kThreads), 0, s, A, q0, partial, stride,
                         wave_blocks + units, d_sq_cells, d_n_cells);
    }
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_contingency_sums(const int32_t *a, size_t n_a, const int32_t *b, size_t n_b, size_t n,
                                    int device_id, long long *sq_a, long long *sq_b, int32_t *labels_a,
                                    int32_t *labels_b, long long *sq_cells, long long *n_cells) {
  const int rc0 = rand_check_args(a, n_a, b, n_b, n, sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells);
  if (rc0 != PPK_OK) return rc0;
  if (!b) n_b = n_a;
  const bool out_b = sq_b && labels_b;
  int32_t *d_a, *d_b, *d_labels_a, *d_labels_b;
  long long *d_sq_a, *d_sq_b, *d_sq_cells, *d_n_cells;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_a, n_a * n).take(d_b, b ? n_b * n : 0).take(d_sq_a, n_a).take(d_sq_b, n_b).take(d_labels_a, n_a)
        .take(d_labels_b, n_b).take(d_sq_cells, n_a * n_b).take(d_n_cells, n_a * n_b);
  }, [&]() -> int {
    PPK_HIP(hipMemcpy(d_a, a, n_a * n * 4, hipMemcpyHostToDevice));
    if (b) PPK_HIP(hipMemcpy(d_b, b, n_b * n * 4, hipMemcpyHostToDevice));
    const int rc = ppk_contingency_sums_dev(d_a, n_a, b ? d_b : nullptr, n_b, n, d_sq_a, d_sq_b, d_labels_a,
                                            d_labels_b, d_sq_cells, d_n_cells, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(sq_a, d_sq_a, n_a * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(labels_a, d_labels_a, n_a * 4, hipMemcpyDeviceToHost));
    if (out_b) {
      PPK_HIP(hipMemcpy(sq_b, d_sq_b, n_b * 8, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(labels_b, d_labels_b, n_b * 4, hipMemcpyDeviceToHost));
    }
    PPK_HIP(hipMemcpy(sq_cells, d_sq_cells, n_a * n_b * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(n_cells, d_n_cells, n_a * n_b * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}
