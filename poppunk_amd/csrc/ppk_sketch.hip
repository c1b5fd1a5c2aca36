// Sketching: codes of assemblies -> the bit-sliced bin sketches kernel 1 reads.  The rule
// ("poppunk_amd:sketch1": hash, bin, densify) is ppk_device.h's; this file is its schedule.
//
//   plan     one workgroup: the offsets checked, every sample cut into pieces of kWgPiece start positions, the pieces
//            of all samples numbered back to back (a sample without a start position still has one piece)
//   stats    a workgroup per piece: length, missing bases, base counts; the first code above 5
//   hash     a workgroup per (piece, k), drawn from a ticket: every lane rolls the two hashes through kLanePiece
//            consecutive start positions (k - 1 codes of warm-up: neighbouring pieces overlap by k - 1 codes) and keeps
//            the per-bin minima of the piece in LDS -- compare first, atomic only on an improvement -- then merges
//            them into the (sample, k) minima in global memory the same way.  Sketches of more bins than LDS holds
//            (option "sketch_lds_bins" lowers that) take their minima straight to global memory.
//   finish   a workgroup per (sample, k): filled bins counted, empty bins densified, values cut to bbits and
//            bit-sliced by ballot into the caller's buffer
// A minimum does not depend on the order it was taken in: the same bits for every cut, route and run.
//
// Read samples take the same plan, stats and finish and, in the place of hash, three passes of the same
// rolling loop (sketch_roll_units) with a sink each:
//   count    every k-mer adds one to its counters of the (sample, k) table, unless they show min_count already
//   select   the per-bin minima over the k-mers whose counters all reach min_count; occ and adm_occ
//   winners  the exact count of every bin's winner; on the exact route `check` then drops the winners that fall short
//            and the unit is selected and counted again above them, until none does
// Counts, minima and threshold tests of final values: the same bits for every cut, route, batch and run.
#include <algorithm>
#include <string>
#include <vector>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 512;                          // hash kernel: 8 waves
constexpr int kLanePiece = 128;                        // start positions a lane rolls through
constexpr int kWavePiece = 64 * kLanePiece;            // ... a wave: 8 192
constexpr int kWgPiece = (kThreads / 64) * kWavePiece; // ... a workgroup (one piece): 65 536
constexpr int kStatThreads = 256;
constexpr int kFinishThreads = 256;
constexpr int kPlanThreads = 1024;
constexpr size_t kLdsBytesMax = 159 * 1024;            // the minima of one (piece, k): 20 352 bins at most
constexpr size_t kLdsBytesDefault = 63 * 1024;         // ... where the opt-in to more than 64 KiB is refused
constexpr size_t kMinimaBytes = (size_t)512 << 20;     // the (sample, k) minima of one group of samples
constexpr size_t kMaxS64 = 4096;                       // finish keeps two ints per 64-bin block in LDS
constexpr unsigned long long kNone = ~0ull;

enum { CTL_BAD_OFFSET = 0, CTL_BAD_CODE = 1, CTL_TICKET = 2, CTL_FAILED = 3, CTL_WORDS = 4 };

struct SketchArgs {
  const uint8_t *codes;
  const long long *off;         // [n + 1]
  const long long *piece_start; // [n + 1]: pieces before each sample
  unsigned long long *ctl;
  unsigned long long *minima;   // [group][nk][nbins]
  size_t s0, s1;                // the group's samples
  int k0, k1;                   // ... and k-mer lengths, k[k0 .. k1): all of them, unless the group is part of one sample
  uint32_t nbins;
  int nk, strand_preserved;
  int k[PPK_MAX_NK];
};

// pieces of a sample of `len` codes
__device__ __forceinline__ long long pieces_of(long long len) { return len <= kWgPiece ? 1 : (len + kWgPiece - 1) / kWgPiece; }

__global__ void __launch_bounds__(kPlanThreads) sketch_plan_kernel(const long long *off, size_t n, long long *piece_start,
                                                                  unsigned long long *ctl) {
  __shared__ long long s_scan[kPlanThreads];
  __shared__ unsigned long long s_bad;
  __shared__ long long s_carry;
  const int t = threadIdx.x;
  if (t == 0) {
    s_bad = off[0] < 0 ? 0 : kNone;
    s_carry = 0;
  }
  __syncthreads();
  for (size_t base = 0; base < n; base += kPlanThreads) {
    const size_t i = base + t;
    long long v = 0;
    if (i < n) {
      const long long a = off[i], b = off[i + 1];
      if (b < a) atomicMin(&s_bad, (unsigned long long)(i + 1));
      v = pieces_of(b - a);
    }
    s_scan[t] = v;
    __syncthreads();
    for (int d = 1; d < kPlanThreads; d <<= 1) {
      const long long add = t >= d ? s_scan[t - d] : 0;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    const long long carry = s_carry;
    if (i < n) piece_start[i] = carry + s_scan[t] - v;
    __syncthreads();
    if (t == kPlanThreads - 1) s_carry = carry + s_scan[t];
    __syncthreads();
  }
  if (t == 0) piece_start[n] = s_carry;
  __syncthreads();
  if (s_bad != kNone) {      // offsets that do not ascend: no piece, nothing is read through them
    for (size_t i = t; i <= n; i += kPlanThreads) piece_start[i] = 0;
    if (t == 0) ctl[CTL_BAD_OFFSET] = s_bad;
  }
}

// the sample of piece p: the last s in [lo, hi) with piece_start[s] <= p
__device__ __forceinline__ size_t sample_of_piece(const long long *piece_start, size_t lo, size_t hi, long long p) {
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (piece_start[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kStatThreads) sketch_stats_kernel(const uint8_t *codes, const long long *off,
                                                                   const long long *piece_start, size_t n,
                                                                   unsigned long long *stats, unsigned long long *ctl) {
  const long long total = piece_start[n];
  for (long long p = blockIdx.x; p < total; p += gridDim.x) {
    const size_t s = sample_of_piece(piece_start, 0, n, p);
    const long long a = off[s] + (p - piece_start[s]) * kWgPiece;
    const long long b = a + kWgPiece < off[s + 1] ? a + kWgPiece : off[s + 1];
    unsigned long long cnt[5] = {0, 0, 0, 0, 0}, bad = kNone;
    for (long long i = a + threadIdx.x; i < b; i += kStatThreads) {
      const unsigned c = codes[i];
#pragma unroll
      for (unsigned x = 0; x < 5; ++x) cnt[x] += c == x;
      if (c > 5 && bad == kNone) bad = (unsigned long long)i;
    }
    unsigned long long *mine = stats + s * 6;
    unsigned long long all = 0;
#pragma unroll
    for (int x = 0; x < 5; ++x) all += cnt[x];
    wave_add(mine + 0, all);                 // length: every code below 5
    wave_add(mine + 1, cnt[4]);              // missing bases
#pragma unroll
    for (int x = 0; x < 4; ++x) wave_add(mine + 2 + x, cnt[x]);
    if (bad != kNone) atomicMin(ctl + CTL_BAD_CODE, bad);
  }
}

// the codes from an address on, eight to a load: aligned words, so that no load leaves the pages the codes lie in
struct CodeStream {
  const uint64_t *w;
  uint64_t cur;
  unsigned left;
  __device__ __forceinline__ void start(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned sh = (unsigned)(a & 7);
    w = reinterpret_cast<const uint64_t *>(a - sh);
    cur = *w++ >> (8 * sh);
    left = 8 - sh;
  }
  __device__ __forceinline__ unsigned next() {
    if (left == 0) {
      cur = *w++;
      left = 8;
    }
    const unsigned c = (unsigned)(cur & 0xff);
    cur >>= 8;
    --left;
    return c;
  }
};

// the dynamic LDS of the pass kernels
__device__ __forceinline__ unsigned long long *lds_words() {
  extern __shared__ unsigned long long s_dyn[];
  return s_dyn;
}

// The rolling loop every pass over the codes shares: workgroups draw units (piece, k) of the group from the ticket;
// every lane rolls the two hashes through its kLanePiece start positions and hands each valid k-mer's kept hash and
// bin to the pass's sink.  A sink has
//   open(A, s, ki, lu, len)  the unit's sample, k index, place in the group's scratch and sample length; false skips
//                            the unit (the answer is the same in every lane)
//   clear(A, tid)            its LDS state set, before a barrier
//   hit(A, h, bin)           one k-mer
//   close(A, tid)            after the lanes' loops, by every lane (it may hold barriers)
template <class Sink>
__device__ __forceinline__ void sketch_roll_units(const SketchArgs &A, Sink &sink) {
  __shared__ uint64_t s_terms[5][4];                    // ppk_sketch_terms of the codes 0 .. 4 at this unit's k
  __shared__ unsigned long long s_unit;
  const int tid = threadIdx.x;
  const unsigned nkg = (unsigned)(A.k1 - A.k0);
  const long long first_piece = A.piece_start[A.s0];
  const unsigned long long units = (unsigned long long)(A.piece_start[A.s1] - first_piece) * nkg;
  while (true) {
    __syncthreads();                                    // (the last unit's readers of s_unit, s_terms and the sink's LDS)
    if (tid == 0) s_unit = atomicAdd(A.ctl + CTL_TICKET, 1ull);
    __syncthreads();
    const unsigned long long u = s_unit;
    if (u >= units) return;
    const long long piece = first_piece + (long long)(u / nkg);
    const int ki = A.k0 + (int)(u % nkg), k = A.k[ki];
    const size_t s = sample_of_piece(A.piece_start, A.s0, A.s1, piece);
    const long long len = A.off[s + 1] - A.off[s];
    const long long p0 = (piece - A.piece_start[s]) * kWgPiece;      // the piece's start positions: [p0, p1)
    const long long p1 = p0 + kWgPiece < len - k + 1 ? p0 + kWgPiece : len - k + 1;
    if (p0 >= p1) continue;                              // (a sample shorter than k)
    if (!sink.open(A, s, ki, (s - A.s0) * (size_t)nkg + (size_t)(ki - A.k0), len)) continue;
    if (tid < 5) ppk_sketch_terms((unsigned)tid, k, s_terms[tid]);
    sink.clear(A, tid);
    __syncthreads();

    const long long q0 = p0 + (long long)tid * kLanePiece;           // this lane's start positions: [q0, q1)
    const long long q1 = q0 + kLanePiece < p1 ? q0 + kLanePiece : p1;
    if (q0 < q1) {
      const uint8_t *base = A.codes + A.off[s] + q0;
      CodeStream in, out;
      in.start(base);
      out.start(base);
      uint64_t f = 0, r = 0;
      int run = 0;                                        // codes below 4 in a row, up to the one that entered last
      for (int t = 0; t < k - 1; ++t) {                   // warm-up: the first k - 1 codes, nothing leaves
        const unsigned c = min(in.next(), 4u);
        ppk_sketch_roll(f, r, s_terms[c][0], s_terms[c][1], 0, 0);
        run = c < 4 ? run + 1 : 0;
      }
      unsigned o = 4;
      const int steps = (int)(q1 - q0);
      for (int t = 0; t < steps; ++t) {
        const unsigned c = min(in.next(), 4u);
        ppk_sketch_roll(f, r, s_terms[c][0], s_terms[c][1], s_terms[o][2], s_terms[o][3]);
        run = c < 4 ? run + 1 : 0;
        if (run >= k) {
          const uint64_t h = ppk_sketch_keep(ppk_sketch_pick(f, r, A.strand_preserved));
          sink.hit(A, h, ppk_sketch_bin(h, A.nbins));
        }
        o = min(out.next(), 4u);                          // (the code that leaves at the next step; its word holds
      }                                                   //  a code `in` has read already)
    }
    sink.close(A, tid);
  }
}

// The assemblies' pass: every k-mer may take its bin.  LDS: the piece's minima in LDS, merged at its end; otherwise
// every minimum straight to global memory
template <bool LDS>
struct MinSink {
  unsigned long long *gmin;
  __device__ __forceinline__ bool open(const SketchArgs &A, size_t, int, size_t lu, long long) {
    gmin = A.minima + lu * A.nbins;
    return true;
  }
  __device__ __forceinline__ void clear(const SketchArgs &A, int tid) {
    if (LDS)
      for (uint32_t b = tid; b < A.nbins; b += kThreads) lds_words()[b] = PPK_SKETCH_EMPTY;
  }
  __device__ __forceinline__ void hit(const SketchArgs &, uint64_t h, uint32_t bin) {
    // a bin's minimum stops improving after a handful of k-mers: most of them end at the compare
    if (LDS) {
      unsigned long long *s_min = lds_words();
      if (h < s_min[bin]) atomicMin(&s_min[bin], (unsigned long long)h);
    } else {
      if (h < gmin[bin]) atomicMin(&gmin[bin], (unsigned long long)h);
    }
  }
  __device__ __forceinline__ void close(const SketchArgs &A, int tid) {
    if (LDS) {
      __syncthreads();
      // (a plain load may return an older, higher minimum: then the atomic decides)
      for (uint32_t b = tid; b < A.nbins; b += kThreads) {
        const unsigned long long v = lds_words()[b];
        if (v != PPK_SKETCH_EMPTY && v < gmin[b]) atomicMin(&gmin[b], v);
      }
    }
  }
};

template <bool LDS>
__global__ void __launch_bounds__(kThreads) sketch_hash_kernel(SketchArgs A) {
  MinSink<LDS> sink;
  sketch_roll_units(A, sink);
}

// ---- read samples: count, select, winners ----
struct ReadsArgs {
  uint32_t *table;             // [group unit]: PPK_SKETCH_COUNT_ROWS rows of 2^bits counters, units `stride` apart
  unsigned long long *lo;      // [group unit][nbins] exact route: the least value a bin may still take
  unsigned long long *cnt;     // [group unit][nbins] the occurrences of the bin's current winner
  int *pending;                // [group unit] exact route: a bin of the unit failed the last round
  unsigned long long *kstats;  // the caller's [n][nk][4]: occ, adm_occ, filled, win_occ
  size_t stride;
  uint32_t min_count;
  int force_bits, exact, round, nk;
};

__device__ __forceinline__ int count_bits_of(const ReadsArgs &R, long long len) {
  return R.force_bits ? R.force_bits : ppk_sketch_count_bits(len);
}

// count: every occurrence adds one to its counters.  A counter only grows and is only ever asked "at least min_count?",
// so a lane reads it first and leaves it alone when it shows that much already: the answer is the same, and a k-mer
// seen a million times costs about min_count atomics.  (The load is an atomic one: a plain load may be served from
// the compute unit's own cache for the rest of the launch.)  32-bit counters of their own: nothing carries over.
struct CountSink {
  const ReadsArgs &R;
  uint32_t *tab;
  int bits;
  __device__ __forceinline__ bool open(const SketchArgs &, size_t, int, size_t lu, long long len) {
    tab = R.table + lu * R.stride;
    bits = count_bits_of(R, len);
    return true;
  }
  __device__ __forceinline__ void clear(const SketchArgs &, int) {}
  __device__ __forceinline__ void hit(const SketchArgs &, uint64_t h, uint32_t) {
#pragma unroll
    for (int r = 0; r < PPK_SKETCH_COUNT_ROWS; ++r) {
      uint32_t *p = tab + ((size_t)r << bits) + ppk_sketch_count_index(h, r, bits);
      if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < R.min_count) atomicAdd(p, 1u);
    }
  }
  __device__ __forceinline__ void close(const SketchArgs &, int) {}
};

__global__ void __launch_bounds__(kThreads) reads_count_kernel(SketchArgs A, ReadsArgs R) {
  CountSink sink{R};
  sketch_roll_units(A, sink);
}

// select: the per-bin minimum over the k-mers whose counters all reach min_count (and, in the exact route, that are
// not below the bin's floor).  The counters are final: an earlier launch wrote them.  STATS (the first round): every
// occurrence asks the table, and occ / adm_occ are counted; later rounds ask it only for a k-mer that would improve
// its bin.  The LDS copy of the minima starts from the group's, so that a bin that is settled stays silent.
template <bool LDS, bool STATS>
struct SelectSink {
  const ReadsArgs &R;
  unsigned long long *gmin;
  const unsigned long long *lo;
  const uint32_t *tab;
  int bits;
  size_t unit;
  unsigned long long occ, adm;
  __device__ __forceinline__ bool open(const SketchArgs &A, size_t s, int ki, size_t lu, long long len) {
    if (!STATS && !R.pending[lu]) return false;
    gmin = A.minima + lu * A.nbins;
    lo = R.lo + lu * A.nbins;
    tab = R.table + lu * R.stride;
    bits = count_bits_of(R, len);
    unit = s * (size_t)R.nk + (size_t)ki;
    occ = adm = 0;
    return true;
  }
  __device__ __forceinline__ void clear(const SketchArgs &A, int tid) {
    if (LDS)
      for (uint32_t b = tid; b < A.nbins; b += kThreads) lds_words()[b] = gmin[b];
  }
  __device__ __forceinline__ void hit(const SketchArgs &, uint64_t h, uint32_t bin) {
    unsigned long long *slot = LDS ? lds_words() + bin : gmin + bin;
    const bool better = h < *slot;
    bool ok = true;
    if (R.min_count > 1 && (STATS || better)) {
#pragma unroll
      for (int r = 0; r < PPK_SKETCH_COUNT_ROWS; ++r)
        ok = ok && tab[((size_t)r << bits) + ppk_sketch_count_index(h, r, bits)] >= R.min_count;
    }
    if (STATS) {
      ++occ;
      adm += ok;
    }
    if (ok && better && (!R.exact || h >= lo[bin])) atomicMin(slot, (unsigned long long)h);
  }
  __device__ __forceinline__ void close(const SketchArgs &A, int tid) {
    if (LDS) {
      __syncthreads();
      for (uint32_t b = tid; b < A.nbins; b += kThreads) {
        const unsigned long long v = lds_words()[b];
        if (v != PPK_SKETCH_EMPTY && v < gmin[b]) atomicMin(&gmin[b], v);
      }
    }
    if (STATS) {
      wave_add(R.kstats + unit * 4 + 0, occ);
      wave_add(R.kstats + unit * 4 + 1, adm);
    }
  }
};

template <bool LDS, bool STATS>
__global__ void __launch_bounds__(kThreads) reads_select_kernel(SketchArgs A, ReadsArgs R) {
  SelectSink<LDS, STATS> sink{R};
  sketch_roll_units(A, sink);
}

// winners: the exact count of every bin's candidate -- an occurrence whose kept hash equals it adds one.  LDS: the
// candidates [nbins] and 32-bit counts [nbins] of the piece (a piece has 65 536 start positions), merged at its end.
template <bool LDS>
struct WinSink {
  const ReadsArgs &R;
  const unsigned long long *gmin;
  unsigned long long *gcnt;
  __device__ __forceinline__ bool open(const SketchArgs &A, size_t, int, size_t lu, long long) {
    if (R.round > 0 && !R.pending[lu]) return false;
    gmin = A.minima + lu * A.nbins;
    gcnt = R.cnt + lu * A.nbins;
    return true;
  }
  __device__ __forceinline__ void clear(const SketchArgs &A, int tid) {
    if (LDS) {
      uint32_t *s_cnt = reinterpret_cast<uint32_t *>(lds_words() + A.nbins);
      for (uint32_t b = tid; b < A.nbins; b += kThreads) {
        lds_words()[b] = gmin[b];
        s_cnt[b] = 0;
      }
    }
  }
  __device__ __forceinline__ void hit(const SketchArgs &A, uint64_t h, uint32_t bin) {
    if (LDS) {
      if (h == lds_words()[bin]) atomicAdd(reinterpret_cast<uint32_t *>(lds_words() + A.nbins) + bin, 1u);
    } else {
      if (h == gmin[bin]) atomicAdd(&gcnt[bin], 1ull);
    }
  }
  __device__ __forceinline__ void close(const SketchArgs &A, int tid) {
    if (LDS) {
      __syncthreads();
      const uint32_t *s_cnt = reinterpret_cast<const uint32_t *>(lds_words() + A.nbins);
      for (uint32_t b = tid; b < A.nbins; b += kThreads)
        if (s_cnt[b]) atomicAdd(&gcnt[b], (unsigned long long)s_cnt[b]);
    }
  }
};

template <bool LDS>
__global__ void __launch_bounds__(kThreads) reads_winners_kernel(SketchArgs A, ReadsArgs R) {
  WinSink<LDS> sink{R};
  sketch_roll_units(A, sink);
}

// the exact route's verdict, a workgroup per unit of the group: a bin whose winner was seen fewer than min_count times
// loses it and may only take a higher value from now on.  A unit with such a bin is selected and counted again (all
// its counts start over); the least such unit of the whole call goes to the control words.
__global__ void __launch_bounds__(kFinishThreads) reads_check_kernel(unsigned long long *minima, ReadsArgs R, uint32_t nbins,
                                                                    size_t unit0, unsigned long long *ctl) {
  __shared__ int s_fails;
  const size_t lu = blockIdx.x;
  if (R.round > 0 && !R.pending[lu]) return;
  unsigned long long *gmin = minima + lu * nbins, *lo = R.lo + lu * nbins, *cnt = R.cnt + lu * nbins;
  if (threadIdx.x == 0) s_fails = 0;
  __syncthreads();
  int fails = 0;
  for (uint32_t b = threadIdx.x; b < nbins; b += kFinishThreads) fails += gmin[b] != PPK_SKETCH_EMPTY && cnt[b] < R.min_count;
  if (fails) atomicAdd(&s_fails, fails);
  __syncthreads();
  const int all = s_fails;
  if (threadIdx.x == 0) {
    R.pending[lu] = all > 0;
    if (all) atomicMin(ctl + CTL_FAILED, (unsigned long long)(unit0 + lu));
  }
  if (!all) return;
  for (uint32_t b = threadIdx.x; b < nbins; b += kFinishThreads) {
    if (gmin[b] != PPK_SKETCH_EMPTY && cnt[b] < R.min_count) {
      lo[b] = gmin[b] + 1;               // (a kept hash is never all ones)
      gmin[b] = PPK_SKETCH_EMPTY;
    }
    cnt[b] = 0;
  }
}

// filled and win_occ of every unit of the group, and the sample's length from the four integers of its largest k
__global__ void __launch_bounds__(kFinishThreads) reads_kstats_kernel(const unsigned long long *minima, ReadsArgs R,
                                                                     uint32_t nbins, size_t unit0, int length_k,
                                                                     unsigned long long *stats) {
  __shared__ unsigned long long s_sum[2];
  const size_t lu = blockIdx.x, unit = unit0 + lu;
  const unsigned long long *gmin = minima + lu * nbins, *cnt = R.cnt + lu * nbins;
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long filled = 0, win = 0;
  for (uint32_t b = threadIdx.x; b < nbins; b += kFinishThreads)
    if (gmin[b] != PPK_SKETCH_EMPTY) {
      ++filled;
      win += cnt[b];
    }
  wave_add(&s_sum[0], filled);
  wave_add(&s_sum[1], win);
  __syncthreads();
  if (threadIdx.x == 0) {
    R.kstats[unit * 4 + 2] = s_sum[0];
    R.kstats[unit * 4 + 3] = s_sum[1];
    if ((int)(unit % (size_t)R.nk) == length_k)
      stats[(unit / (size_t)R.nk) * 6] = (unsigned long long)ppk_sketch_reads_length(R.kstats[unit * 4 + 1], s_sum[0], s_sum[1]);
  }
}

__global__ void __launch_bounds__(kFinishThreads) sketch_finish_kernel(const unsigned long long *minima, size_t unit0,
                                                                      uint32_t s64, int bbits, uint64_t *sketches,
                                                                      int32_t *filled) {
  extern __shared__ int s_blocks[];     // [s64] the first non-empty bin of each 64-bin block (-1: none), [s64] the first
  __shared__ int s_filled;              //       non-empty bin of the blocks after it, cyclically (densify's `next`)
  int *s_first = s_blocks, *s_next = s_blocks + s64;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long *gmin = minima + (size_t)blockIdx.x * s64 * 64;
  const size_t unit = unit0 + blockIdx.x;                // (sample, k) of the whole call
  uint64_t *out = sketches + unit * s64 * (size_t)bbits;
  if (threadIdx.x == 0) s_filled = 0;
  __syncthreads();
  int count = 0;
  for (uint32_t blk = wave; blk < s64; blk += kFinishThreads / 64) {
    const uint64_t mask = __ballot(gmin[blk * 64 + lane] != PPK_SKETCH_EMPTY);
    if (lane == 0) s_first[blk] = mask ? (int)(blk * 64 + __builtin_ctzll(mask)) : -1;
    count += __builtin_popcountll(mask);
  }
  if (lane == 0 && count) atomicAdd(&s_filled, count);
  __syncthreads();
  if (wave == 0) {
    // two walks down the blocks: the first leaves the first non-empty bin of all in `carry`, which is what follows
    // the top block cyclically; the second writes every block's `next`
    int carry = -1;
    const int chunks = (int)((s64 + 63) / 64);
    for (int pass = 0; pass < 2; ++pass)
      for (int c = chunks - 1; c >= 0; --c) {
        const uint32_t blk = (uint32_t)c * 64 + lane;
        const int fv = blk < s64 ? s_first[blk] : -1;
        const uint64_t m = __ballot(fv >= 0);
        const uint64_t above = lane < 63 ? m >> (lane + 1) : 0;
        const int got = __shfl(fv, above ? (int)(lane + 1 + __builtin_ctzll(above)) : 0);
        if (pass == 1 && blk < s64) s_next[blk] = above ? got : carry;
        const int low = __shfl(fv, m ? (int)__builtin_ctzll(m) : 0);
        if (m) carry = low;
      }
  }
  __syncthreads();
  const int n_filled = s_filled;
  if (threadIdx.x == 0) filled[unit] = n_filled;
  const uint64_t value_mask = ((uint64_t)1 << bbits) - 1;
  for (uint32_t blk = wave; blk < s64; blk += kFinishThreads / 64) {
    const uint32_t bin = blk * 64 + lane;
    const unsigned long long v = gmin[bin];
    uint64_t val = 0;
    if (n_filled) {           // (no k-mer at all: the words are zero)
      const uint64_t mask = __ballot(v != PPK_SKETCH_EMPTY);
      const uint32_t src = ppk_sketch_densify_src(mask, lane, blk, (uint32_t)s_next[blk]);
      val = (src == bin ? v : gmin[src]) & value_mask;
    }
    uint64_t mine = 0;
    for (int b = 0; b < bbits; ++b) {
      const uint64_t word = __ballot((val >> b) & 1);
      if ((int)lane == b) mine = word;
    }
    if ((int)lane < bbits) out[(size_t)blk * bbits + lane] = mine;
  }
}

constexpr size_t kTableBytes = (size_t)512 << 20;      // the count tables of one group of (sample, k)
constexpr long long kMaxMinCount = 65535;
constexpr long long kMaxReadCodes = 0xffffffffll;      // a read sample's codes: what a 32-bit counter can hold

// the argument errors that need no device; reads: ppk_sketch_reads[_dev]'s, with its min_count and kstats
int sketch_check_args(const char *name, bool reads, const void *codes, const void *seq_off, const int32_t *kmers, size_t nk,
                      size_t s64, size_t bbits, int flags, int min_count, const void *sketches, const void *stats,
                      const void *kstats, const void *filled) {
  const std::string who = name;
  if (!codes || !seq_off || !kmers || !sketches || !stats || !filled || (reads && !kstats))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (nk < 1 || nk > PPK_MAX_NK) return ppk_fail(PPK_ERR_ARG, who + ": nk must be 1 .. " + std::to_string(PPK_MAX_NK));
  for (size_t i = 0; i < nk; ++i)
    if (kmers[i] < 3 || kmers[i] > 101)
      return ppk_fail(PPK_ERR_ARG, who + ": k-mer length " + std::to_string(kmers[i]) + " outside 3 .. 101");
  if (bbits != 14) return ppk_fail(PPK_ERR_ARG, who + ": bbits must be 14");
  if (s64 < 1) return ppk_fail(PPK_ERR_ARG, who + ": sketchsize64 must be at least 1");
  if (s64 > kMaxS64) return ppk_fail(PPK_ERR_ARG, who + ": sketchsize64 above " + std::to_string(kMaxS64));
  if (flags & ~(PPK_SKETCH_STRAND_PRESERVED | (reads ? PPK_SKETCH_EXACT : 0))) return ppk_fail(PPK_ERR_ARG, who + ": unknown flag");
  if (reads) {
    if (min_count < 1 || min_count > kMaxMinCount)
      return ppk_fail(PPK_ERR_ARG, who + ": min_count " + std::to_string(min_count) + " outside 1 .. " + std::to_string(kMaxMinCount));
    const long long bits = ppk_config().sketch_count_bits.load();
    if (bits != 0 && (bits < PPK_SKETCH_COUNT_BITS_MIN || bits > PPK_SKETCH_COUNT_BITS_MAX))
      return ppk_fail(PPK_ERR_ARG, who + ": option sketch_count_bits must be 0 or " + std::to_string(PPK_SKETCH_COUNT_BITS_MIN) +
                                       " .. " + std::to_string(PPK_SKETCH_COUNT_BITS_MAX));
    if (ppk_config().sketch_exact_rounds.load() < 1) return ppk_fail(PPK_ERR_ARG, who + ": option sketch_exact_rounds must be at least 1");
  }
  return PPK_OK;
}

int bad_offset_error(const char *who, size_t sample) {
  return ppk_fail(PPK_ERR_ARG, std::string(who) + ": offsets do not ascend at sample " + std::to_string(sample));
}

// what the plan and stats passes found wrong with the input, after the call's kernels: the stream is synchronised here
int sketch_input_errors(const char *name, int dev, hipStream_t s, const unsigned long long *ctl, const uint8_t *d_codes,
                        const long long *d_seq_off, size_t n, size_t sample_base, long long code_base) {
  const std::string who = name;
  const unsigned long long *h = nullptr;
  const int rc = ppk_read_back(dev, s, {{ctl, 16}}, &h);
  if (rc != PPK_OK) return rc;
  if (h[CTL_BAD_OFFSET] != kNone)
    return bad_offset_error(name, sample_base + (size_t)h[CTL_BAD_OFFSET] - (h[CTL_BAD_OFFSET] ? 1 : 0));
  if (h[CTL_BAD_CODE] != kNone) {
    const unsigned long long at = h[CTL_BAD_CODE];
    uint8_t c = 0;
    PPK_HIP(hipMemcpy(&c, d_codes + at, 1, hipMemcpyDeviceToHost));
    // its sample: the offsets ascend, so a search of the device array from the host side would do; one copy is simpler
    std::vector<long long> off(n + 1);
    PPK_HIP(hipMemcpy(off.data(), d_seq_off, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    const size_t smp = (size_t)(std::upper_bound(off.begin(), off.end(), (long long)at) - off.begin()) - 1;
    return ppk_fail(PPK_ERR_ARG, who + ": sample " + std::to_string(sample_base + smp) + ", position " +
                                     std::to_string((long long)at - off[smp]) + " (code " +
                                     std::to_string((long long)at + code_base) + "): code " + std::to_string((int)c) +
                                     " above 5");
  }
  return PPK_OK;
}

// the most bins a pass keeps in LDS at `bytes_per_bin`: as many as LDS holds, or option "sketch_lds_bins" if fewer
size_t lds_bins_of(size_t lds_cap, size_t bytes_per_bin) {
  size_t lds_bins = lds_cap / bytes_per_bin;
  if (const long long force = ppk_config().sketch_lds_bins.load(); force > 0 && (size_t)force < lds_bins)
    lds_bins = (size_t)force;
  return lds_bins;
}

// The device call on samples [sample_base, sample_base + n) of a larger job whose codes start code_base before
// d_codes: both only shift what an error message names.
int sketch_dev(const uint8_t *d_codes, const long long *d_seq_off, size_t n, const int32_t *kmers, size_t nk, size_t s64,
               size_t bbits, int flags, uint64_t *d_sketches, long long *d_stats, int32_t *d_filled, hipStream_t s,
               size_t sample_base, long long code_base) {
  if (n == 0) return PPK_OK;
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  if (int rc = ppk_check_arch(dev)) return rc;
  PpkCall call(dev, s);

  const size_t nbins = s64 * 64;
  // the route: the minima of a (piece, k) in LDS where they fit
  const size_t lds_cap = ppk_lds_opt_in(reinterpret_cast<const void *>(sketch_hash_kernel<true>), dev, (int)kLdsBytesMax)
                             ? kLdsBytesMax : kLdsBytesDefault;
  const bool lds = nbins <= lds_bins_of(lds_cap, 8);
  // the samples whose minima the scratch holds at once
  const size_t per_sample = nk * nbins * sizeof(unsigned long long);
  const size_t group = std::max<size_t>(1, std::min(n, kMinimaBytes / per_sample));

  SketchArgs A{};
  long long *piece_start;
  int rc = ppk_scratch_carve(dev, SLOT_SKETCH, [&](Carve &c) {
    c.take(A.ctl, CTL_WORDS).take(piece_start, n + 1).take(A.minima, group * nk * nbins);
  });
  if (rc != PPK_OK) return rc;
  A.codes = d_codes;
  A.off = d_seq_off;
  A.piece_start = piece_start;
  A.nbins = (uint32_t)nbins;
  A.nk = (int)nk;
  A.strand_preserved = flags & PPK_SKETCH_STRAND_PRESERVED ? 1 : 0;
  for (size_t i = 0; i < nk; ++i) A.k[i] = kmers[i];

  const PpkGeometry &g = ppk_geometry(dev);
  ppk_prof_stage("plan", s);
  PPK_HIP(hipMemsetAsync(A.ctl, 0xff, CTL_WORDS * 8, s));
  PPK_HIP(hipMemsetAsync(d_stats, 0, n * 6 * sizeof(long long), s));
  hipLaunchKernelGGL(sketch_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, d_seq_off, n, piece_start, A.ctl);
  hipLaunchKernelGGL(sketch_stats_kernel, dim3((unsigned)g.cus * 8), dim3(kStatThreads), 0, s, d_codes, d_seq_off,
                     piece_start, n, reinterpret_cast<unsigned long long *>(d_stats), A.ctl);
  // workgroups of the hash kernel: as many as are resident at once, each drawing units until none is left
  const size_t lds_bytes = lds ? nbins * 8 : 0;
  const unsigned per_cu = !lds ? 4 : lds_bytes <= 78 * 1024 ? 2 : 1;
  for (size_t s0 = 0; s0 < n; s0 += group) {
    const size_t s1 = std::min(n, s0 + group);
    A.s0 = s0;
    A.s1 = s1;
    A.k0 = 0;
    A.k1 = (int)nk;
    ppk_prof_stage("hash", s);
    PPK_HIP(hipMemsetAsync(A.minima, 0xff, (s1 - s0) * per_sample, s));
    PPK_HIP(hipMemsetAsync(A.ctl + CTL_TICKET, 0, 8, s));
    if (lds)
      hipLaunchKernelGGL(sketch_hash_kernel<true>, dim3((unsigned)g.cus * per_cu), dim3(kThreads), lds_bytes, s, A);
    else
      hipLaunchKernelGGL(sketch_hash_kernel<false>, dim3((unsigned)g.cus * per_cu), dim3(kThreads), 0, s, A);
    ppk_prof_stage("finish", s);
    hipLaunchKernelGGL(sketch_finish_kernel, dim3((unsigned)((s1 - s0) * nk)), dim3(kFinishThreads),
                       2 * s64 * sizeof(int), s, A.minima, s0 * nk, (uint32_t)s64, (int)bbits, d_sketches, d_filled);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return sketch_input_errors("ppk_sketch", dev, s, A.ctl, d_codes, d_seq_off, n, sample_base, code_base);
}

// a group of the read call: samples [s0, s1) at k[k0 .. k1), its count tables `stride` counters apart
struct ReadsGroup {
  size_t s0, s1;
  int k0, k1;
  size_t stride;
  size_t units() const { return (s1 - s0) * (size_t)(k1 - k0); }
};

// The read samples' device call.  h_off: the offsets on the host (the groups and their tables are planned from them).
int reads_dev(const uint8_t *d_codes, const long long *d_seq_off, const long long *h_off, size_t n, const int32_t *kmers,
              size_t nk, size_t s64, size_t bbits, int flags, int min_count, uint64_t *d_sketches, long long *d_stats,
              long long *d_kstats, int32_t *d_filled, hipStream_t s, size_t sample_base, long long code_base) {
  const char *name = "ppk_sketch_reads";
  const std::string who = name;
  if (n == 0) return PPK_OK;
  if (h_off[0] < 0) return bad_offset_error(name, sample_base);
  for (size_t i = 0; i < n; ++i) {
    if (h_off[i + 1] < h_off[i]) return bad_offset_error(name, sample_base + i);
    if (h_off[i + 1] - h_off[i] > kMaxReadCodes)
      return ppk_fail(PPK_ERR_ARG, who + ": sample " + std::to_string(sample_base + i) + " has more than " +
                                       std::to_string(kMaxReadCodes) + " codes");
  }
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  if (int rc = ppk_check_arch(dev)) return rc;
  PpkCall call(dev, s);

  const size_t nbins = s64 * 64;
  const bool exact = (flags & PPK_SKETCH_EXACT) && min_count > 1, counted = min_count > 1;
  const int force_bits = (int)ppk_config().sketch_count_bits.load();
  const long long max_rounds = ppk_config().sketch_exact_rounds.load();
  // the route: candidates and 32-bit counts of a (piece, k) in LDS where they fit (12 bytes a bin)
  bool opt_in = ppk_lds_opt_in(reinterpret_cast<const void *>(reads_select_kernel<true, true>), dev, (int)kLdsBytesMax);
  opt_in = ppk_lds_opt_in(reinterpret_cast<const void *>(reads_select_kernel<true, false>), dev, (int)kLdsBytesMax) && opt_in;
  opt_in = ppk_lds_opt_in(reinterpret_cast<const void *>(reads_winners_kernel<true>), dev, (int)kLdsBytesMax) && opt_in;
  const bool lds = nbins <= lds_bins_of(opt_in ? kLdsBytesMax : kLdsBytesDefault, 12);

  // the groups: whole samples while their minima, floors and counts (24 bytes a bin) and their tables fit the caps; a
  // sample whose tables alone do not fit goes a few k at a time
  const size_t max_units = std::max<size_t>(1, kMinimaBytes / (nbins * 24));
  auto stride_of = [&](size_t i) -> size_t {
    if (!counted) return 0;
    return (size_t)PPK_SKETCH_COUNT_ROWS << (force_bits ? force_bits : ppk_sketch_count_bits(h_off[i + 1] - h_off[i]));
  };
  std::vector<ReadsGroup> groups;
  for (size_t i = 0; i < n;) {
    const size_t own = stride_of(i);
    if (nk > max_units || nk * own * 4 > kTableBytes) {
      const size_t kper = std::max<size_t>(1, std::min(max_units, own ? kTableBytes / (own * 4) : max_units));
      for (size_t k0 = 0; k0 < nk; k0 += kper) groups.push_back({i, i + 1, (int)k0, (int)std::min(nk, k0 + kper), own});
      ++i;
      continue;
    }
    size_t e = i, stride = 0;
    while (e < n) {
      const size_t st = std::max(stride, stride_of(e)), units = (e + 1 - i) * nk;
      if (units > max_units || units * st * 4 > kTableBytes) break;
      stride = st;
      ++e;
    }
    groups.push_back({i, e, 0, (int)nk, stride});
    i = e;
  }
  size_t most_units = 1, most_table = 1;
  for (const ReadsGroup &gr : groups) {
    most_units = std::max(most_units, gr.units());
    most_table = std::max(most_table, gr.units() * gr.stride);
  }

  SketchArgs A{};
  ReadsArgs R{};
  long long *piece_start;
  int rc = ppk_scratch_carve(dev, SLOT_SKETCH, [&](Carve &c) {
    c.take(A.ctl, CTL_WORDS).take(piece_start, n + 1).take(A.minima, most_units * nbins).take(R.lo, most_units * nbins)
        .take(R.cnt, most_units * nbins).take(R.pending, most_units).take(R.table, most_table);
  });
  if (rc != PPK_OK) return rc;
  A.codes = d_codes;
  A.off = d_seq_off;
  A.piece_start = piece_start;
  A.nbins = (uint32_t)nbins;
  A.nk = (int)nk;
  A.strand_preserved = flags & PPK_SKETCH_STRAND_PRESERVED ? 1 : 0;
  int length_k = 0;                                       // the first of the largest k: the sample's length comes from it
  for (size_t i = 0; i < nk; ++i) {
    A.k[i] = kmers[i];
    if (kmers[i] > kmers[length_k]) length_k = (int)i;
  }
  R.kstats = reinterpret_cast<unsigned long long *>(d_kstats);
  R.min_count = (uint32_t)min_count;
  R.force_bits = force_bits;
  R.exact = exact ? 1 : 0;
  R.nk = (int)nk;

  const PpkGeometry &g = ppk_geometry(dev);
  ppk_prof_stage("plan", s);
  PPK_HIP(hipMemsetAsync(A.ctl, 0xff, CTL_WORDS * 8, s));
  PPK_HIP(hipMemsetAsync(d_stats, 0, n * 6 * sizeof(long long), s));
  PPK_HIP(hipMemsetAsync(d_kstats, 0, n * nk * 4 * sizeof(long long), s));
  hipLaunchKernelGGL(sketch_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, d_seq_off, n, piece_start, A.ctl);
  hipLaunchKernelGGL(sketch_stats_kernel, dim3((unsigned)g.cus * 8), dim3(kStatThreads), 0, s, d_codes, d_seq_off,
                     piece_start, n, reinterpret_cast<unsigned long long *>(d_stats), A.ctl);
  const size_t sel_bytes = lds ? nbins * 8 : 0, win_bytes = lds ? nbins * 12 : 0;
  const unsigned per_cu = !lds ? 4 : win_bytes <= 78 * 1024 ? 2 : 1;
  const dim3 grid((unsigned)g.cus * per_cu), block(kThreads);
  auto ticket = [&]() { return hipMemsetAsync(A.ctl + CTL_TICKET, 0, 8, s); };
  for (const ReadsGroup &gr : groups) {
    const size_t units = gr.units(), unit0 = gr.s0 * nk + (size_t)gr.k0;
    A.s0 = gr.s0;
    A.s1 = gr.s1;
    A.k0 = gr.k0;
    A.k1 = gr.k1;
    R.stride = gr.stride;
    PPK_HIP(hipMemsetAsync(A.minima, 0xff, units * nbins * 8, s));
    PPK_HIP(hipMemsetAsync(R.cnt, 0, units * nbins * 8, s));
    if (exact) {
      PPK_HIP(hipMemsetAsync(R.lo, 0, units * nbins * 8, s));
      PPK_HIP(hipMemsetAsync(R.pending, 0, units * sizeof(int), s));
    }
    if (counted) {
      ppk_prof_stage("count", s);
      PPK_HIP(hipMemsetAsync(R.table, 0, units * gr.stride * sizeof(uint32_t), s));
      PPK_HIP(ticket());
      hipLaunchKernelGGL(reads_count_kernel, grid, block, 0, s, A, R);
    }
    for (long long round = 0;; ++round) {
      R.round = (int)round;
      ppk_prof_stage("select", s);
      PPK_HIP(ticket());
      if (round == 0) {
        if (lds) hipLaunchKernelGGL((reads_select_kernel<true, true>), grid, block, sel_bytes, s, A, R);
        else hipLaunchKernelGGL((reads_select_kernel<false, true>), grid, block, 0, s, A, R);
      } else {
        if (lds) hipLaunchKernelGGL((reads_select_kernel<true, false>), grid, block, sel_bytes, s, A, R);
        else hipLaunchKernelGGL((reads_select_kernel<false, false>), grid, block, 0, s, A, R);
      }
      ppk_prof_stage("winners", s);
      PPK_HIP(ticket());
      if (lds) hipLaunchKernelGGL(reads_winners_kernel<true>, grid, block, win_bytes, s, A, R);
      else hipLaunchKernelGGL(reads_winners_kernel<false>, grid, block, 0, s, A, R);
      if (!exact) break;
      PPK_HIP(hipMemsetAsync(A.ctl + CTL_FAILED, 0xff, 8, s));
      hipLaunchKernelGGL(reads_check_kernel, dim3((unsigned)units), dim3(kFinishThreads), 0, s, A.minima, R,
                         (uint32_t)nbins, unit0, A.ctl);
      PPK_HIP(hipGetLastError());
      const unsigned long long *h = nullptr;
      rc = ppk_read_back(dev, s, {{A.ctl + CTL_FAILED, 8}}, &h);
      if (rc != PPK_OK) return rc;
      if (h[0] == kNone) break;
      if (round + 1 >= max_rounds) {
        ppk_prof_stage(nullptr, s);
        return ppk_fail(PPK_ERR_CAPACITY, who + ": sample " + std::to_string(sample_base + (size_t)(h[0] / nk)) + ", k " +
                                              std::to_string(kmers[h[0] % nk]) + ": bins still hold a k-mer below the minimum " +
                                              "count after " + std::to_string(max_rounds) +
                                              " exact rounds (option sketch_exact_rounds)");
      }
    }
    ppk_prof_stage("finish", s);
    hipLaunchKernelGGL(reads_kstats_kernel, dim3((unsigned)units), dim3(kFinishThreads), 0, s, A.minima, R, (uint32_t)nbins,
                       unit0, length_k, reinterpret_cast<unsigned long long *>(d_stats));
    hipLaunchKernelGGL(sketch_finish_kernel, dim3((unsigned)units), dim3(kFinishThreads), 2 * s64 * sizeof(int), s,
                       A.minima, unit0, (uint32_t)s64, (int)bbits, d_sketches, d_filled);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return sketch_input_errors(name, dev, s, A.ctl, d_codes, d_seq_off, n, sample_base, code_base);
}

// The host-array form of both calls (min_count 0: assemblies): device_id's frame around batches of whole samples -- as
// many as keep the codes of a batch under the cap (at least one), or a forced count
int sketch_host(const char *name, const uint8_t *codes, const long long *seq_off, size_t n, const int32_t *kmers, size_t nk,
                size_t sketchsize64, size_t bbits, int flags, int min_count, int device_id, uint64_t *sketches,
                long long *stats, long long *kstats, int32_t *filled) {
  if (n == 0) return PPK_OK;
  if (seq_off[0] < 0) return bad_offset_error(name, 0);
  for (size_t i = 0; i < n; ++i)
    if (seq_off[i + 1] < seq_off[i]) return bad_offset_error(name, i);
  const long long cap_mb = ppk_config().sketch_batch_mb.load();
  const long long cap = (cap_mb > 0 ? cap_mb : 1) << 20;
  const long long force = ppk_config().sketch_batch.load();
  std::vector<size_t> cuts{0};
  for (size_t i = 0; i < n;) {
    size_t e = i + 1;
    if (force > 0) e = std::min(n, i + (size_t)force);
    else
      while (e < n && seq_off[e + 1] - seq_off[i] <= cap) ++e;
    cuts.push_back(e);
    i = e;
  }
  size_t most_samples = 0;
  long long most_codes = 0;
  for (size_t b = 0; b + 1 < cuts.size(); ++b) {
    most_samples = std::max(most_samples, cuts[b + 1] - cuts[b]);
    most_codes = std::max(most_codes, seq_off[cuts[b + 1]] - seq_off[cuts[b]]);
  }
  const size_t words = nk * sketchsize64 * bbits;
  uint8_t *d_codes;
  long long *d_off, *d_stats, *d_kstats;
  uint64_t *d_sketches;
  int32_t *d_filled;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_codes, (size_t)most_codes + 8).take(d_off, most_samples + 1).take(d_sketches, most_samples * words)
        .take(d_stats, most_samples * 6).take(d_filled, most_samples * nk).take(d_kstats, kstats ? most_samples * nk * 4 : 0);
  }, [&]() -> int {
    std::vector<long long> off;
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
      const size_t b0 = cuts[b], m = cuts[b + 1] - b0;
      const long long c0 = seq_off[b0], bytes = seq_off[b0 + m] - c0;
      off.resize(m + 1);
      for (size_t i = 0; i <= m; ++i) off[i] = seq_off[b0 + i] - c0;
      int rc = PPK_OK;
      if (bytes > 0) rc = ppk_upload(device_id, d_codes, codes + c0, (size_t)bytes, nullptr);
      if (rc != PPK_OK) return rc;
      PPK_HIP(hipMemcpy(d_off, off.data(), (m + 1) * sizeof(long long), hipMemcpyHostToDevice));
      if (kstats)
        rc = reads_dev(d_codes, d_off, off.data(), m, kmers, nk, sketchsize64, bbits, flags, min_count, d_sketches, d_stats,
                       d_kstats, d_filled, nullptr, b0, c0);
      else
        rc = sketch_dev(d_codes, d_off, m, kmers, nk, sketchsize64, bbits, flags, d_sketches, d_stats, d_filled, nullptr,
                        b0, c0);
      if (rc != PPK_OK) return rc;
      PPK_HIP(hipMemcpy(sketches + b0 * words, d_sketches, m * words * 8, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(stats + b0 * 6, d_stats, m * 6 * sizeof(long long), hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(filled + b0 * nk, d_filled, m * nk * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (kstats) PPK_HIP(hipMemcpy(kstats + b0 * nk * 4, d_kstats, m * nk * 4 * sizeof(long long), hipMemcpyDeviceToHost));
    }
    return PPK_OK;
  });
}

}  // namespace

extern "C" int ppk_sketch_dev(const uint8_t *d_codes, const long long *d_seq_off, size_t n, const int32_t *kmers,
                              size_t nk, size_t sketchsize64, size_t bbits, int flags, uint64_t *d_sketches,
                              long long *d_stats, int32_t *d_filled, void *stream) {
  const int rc = sketch_check_args("ppk_sketch", false, d_codes, d_seq_off, kmers, nk, sketchsize64, bbits, flags, 0,
                                   d_sketches, d_stats, nullptr, d_filled);
  if (rc != PPK_OK) return rc;
  return sketch_dev(d_codes, d_seq_off, n, kmers, nk, sketchsize64, bbits, flags, d_sketches, d_stats, d_filled,
                    static_cast<hipStream_t>(stream), 0, 0);
}

extern "C" int ppk_sketch(const uint8_t *codes, const long long *seq_off, size_t n, const int32_t *kmers, size_t nk,
                          size_t sketchsize64, size_t bbits, int flags, int device_id, uint64_t *sketches,
                          long long *stats, int32_t *filled) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const int rc0 = sketch_check_args("ppk_sketch", false, codes, seq_off, kmers, nk, sketchsize64, bbits, flags, 0, sketches,
                                    stats, nullptr, filled);
  if (rc0 != PPK_OK) return rc0;
  return sketch_host("ppk_sketch", codes, seq_off, n, kmers, nk, sketchsize64, bbits, flags, 0, device_id, sketches, stats,
                     nullptr, filled);
}

extern "C" int ppk_sketch_reads_dev(const uint8_t *d_codes, const long long *d_seq_off, size_t n, const int32_t *kmers,
                                    size_t nk, size_t sketchsize64, size_t bbits, int flags, int min_count,
                                    uint64_t *d_sketches, long long *d_stats, long long *d_kstats, int32_t *d_filled,
                                    void *stream) {
  const int rc = sketch_check_args("ppk_sketch_reads", true, d_codes, d_seq_off, kmers, nk, sketchsize64, bbits, flags,
                                   min_count, d_sketches, d_stats, d_kstats, d_filled);
  if (rc != PPK_OK) return rc;
  if (n == 0) return PPK_OK;
  // the groups and their count tables are planned on the host: the offsets come down first
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<long long> off(n + 1);
  PPK_HIP(hipMemcpyAsync(off.data(), d_seq_off, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
  PPK_HIP(hipStreamSynchronize(s));
  return reads_dev(d_codes, d_seq_off, off.data(), n, kmers, nk, sketchsize64, bbits, flags, min_count, d_sketches, d_stats,
                   d_kstats, d_filled, s, 0, 0);
}

extern "C" int ppk_sketch_reads(const uint8_t *codes, const long long *seq_off, size_t n, const int32_t *kmers, size_t nk,
                                size_t sketchsize64, size_t bbits, int flags, int min_count, int device_id,
                                uint64_t *sketches, long long *stats, long long *kstats, int32_t *filled) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const int rc0 = sketch_check_args("ppk_sketch_reads", true, codes, seq_off, kmers, nk, sketchsize64, bbits, flags,
                                    min_count, sketches, stats, kstats, filled);
  if (rc0 != PPK_OK) return rc0;
  return sketch_host("ppk_sketch_reads", codes, seq_off, n, kmers, nk, sketchsize64, bbits, flags, min_count, device_id,
                     sketches, stats, kstats, filled);
}
