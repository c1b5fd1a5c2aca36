// Internal host declarations shared by the translation units of libppk_hip.so; the device and host-device
// arithmetic they share is ppk_device.h, included below.
// gfx950 / CDNA4 only (wave64); no other target is supported.
#pragma once

#include <sys/mman.h>

#include <atomic>
#include <functional>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/ppk.h"

#define PPK_MAX_NK 128         // k-mer lengths per query (the reference accepts k = 3 .. 101: PopPUNK/__main__.py)
#define PPK_LANES 64           // wavefront width on CDNA
#define PPK_NPAD 256           // sample axis padded to a multiple of this
#define PPK_RANK_SHORT_WORDS 16   // words of per-block "short" flags a launch carries (PpkCoding::less1): one per k, and one to spare
constexpr int PPK_MAX_DEVICES = 64;   // device ids the per-device tables hold: [0, PPK_MAX_DEVICES)

#include "ppk_device.h"

// The coded copies of a bbits = 14 database (ppk_coding.hip): the same sketches with every bin value replaced by a code
// among the values of its (k, bin) position, bit-sliced in `planes` planes: [(k*s64 + blk)*planes + plane][npad].  A
// self job counts the same matches from fewer planes (launch_v2 in ppk_dist.hip).  The kinds, in the order a launch
// prefers them from the last to the first (coded_planes):
enum PpkCodingKind {
  // Every value is its rank among the distinct values of its position, in 8, 10 or 12 planes: equal values have equal
  // codes and different values different ones.  One allocation serves both sides (d_ref == d_qry).  `planes` is what
  // the distinct values give whenever ANY coding was built; the copy itself (d_ref) is built at creation only where no
  // pair is, and otherwise on demand (ppk_db_rank_read; a rectangular job of the handle against itself reads the raw
  // planes until then): a launch asks for the pointer.  less1: bit blk of word k is set when no position of block
  // (k, blk) holds more than 2^(planes - 1) distinct values, so that the top code plane of the block is zero in every
  // sample and the tile kernel leaves it out (option "rank_short").  Flags are kept for nk < PPK_RANK_SHORT_WORDS and
  // s64 <= 32 (a word per k); other shapes have none.
  PPK_CODING_RANK = 0,
  // The folded pair, built INSTEAD of the injective copy where it compares fewer planes (option "rank_fold"): two
  // copies in `planes` planes.  A value that at least two samples hold at its position has the same code >= 2 in both;
  // a value with a single holder is 0 in d_ref and 1 in d_qry.  Only a triangular self job reads them, d_ref on the ref
  // side and d_qry on the query side: it compares two different samples, which a single-holder value can never match.
  // less1: the short flags of the pair.
  PPK_CODING_FOLD = 1,
  // The two-holder pair, built INSTEAD of the folded pair where it compares fewer planes still (option "rank_fold2"):
  // the same two copies, but a value with exactly two holders is coded like a single-holder one (0 / 1) and only the
  // values with at least three holders keep codes >= 2, so a position spans E2 = S3 + 2 codes.  A two-holder value can
  // match in exactly one pair of the triangular job (its higher holder as ref, its lower as query), which the compare
  // then under-counts by one: every such value is one EVENT (hi, lo, k), and the tile kernel adds the events of its
  // tile back at the top of its epilogue (FOLD2 in ppk_dist_tile.inc).  The list holds them, 16 bits each:
  // hi % 256 | (lo % 32) << 8 | k << 13.  At most PPK_FOLD2_MAX_PER_PAIR events per (pair, k) (a 6-bit field).
  // Neither a match count nor an event depends on the order of a k's positions, so the pair stores them sorted by
  // code span (option "fold2_sort"): slot i of k holds stored position order[k * 64 * s64 + i], E2 descending, ties by
  // stored position ascending (the identity with "fold2_sort" 0).  A block of SLOTS whose largest E2 is at most 128
  // compares 7 planes (less1), at most 64 compares 6 (less2 as well); along a sorted k the planes never increase.  The
  // 7-plane rule on the STORED blocks (ppk_db_fold2_block_planes and the choice among the codings) is a function of
  // rank_counts and is derived from them where it is asked for.
  PPK_CODING_FOLD2 = 2,
  // The holder pair, built BESIDE the two-holder pair where it compares far fewer planes (option "rank_foldh"): the
  // same two copies, but EVERY value with at most `holders` (H) holders is coded 0 / 1 and only the values with more
  // than H holders keep codes 2 + rank, so that a sorted block of 64 slots spans at most 16 codes and streams 4
  // (`stream_planes`), 3 (less1) or 2 (less2 as well) planes.  `planes` stays 8 -- the coding is the two-holder pair's
  // 8-plane one -- but planes 4 .. 7 are zero in every block and are not stored: the copies are laid out
  // [(k * s64 + blk) * 4 + plane][npad] (chunk_planes(): what a launch copies per block, half the bytes).  Slot i of k
  // holds stored position order[k * 64 * s64 + i] (E_H descending, ties by stored position).  What the compare then
  // misses is a COUNT per (pair, k): the matches on values with 2 .. H holders, found once at creation by comparing a
  // temporary pair that codes those values alone.  Non-zero counts are the 32-bit entries of the list:
  // hi % 256 | (lo % 32) << 8 | k << 13 | count << 16.
  PPK_CODING_FOLDH = 3,
  PPK_CODINGS = 4
};
#define PPK_FOLDH_CHUNK_PLANES 4     // planes the holder pair stores per chunk (PPK_FOLDH_MAX_CODES = 2^4 codes)
struct PpkCoding {
  PpkCodingKind kind = PPK_CODING_RANK;
  uint64_t *d_ref = nullptr, *d_qry = nullptr;      // the copies a launch reads on either side
  int planes = 0;                                   // of the layout; 0 = no such coding
  int stream_planes = 0;                            // the most a block compares: `planes`, 4 for the holder pair
  // the planes of a stored 64-bin chunk, [(k * s64 + blk) * chunk_planes() + plane][npad]: `planes` but for the holder pair
  int chunk_planes() const { return kind == PPK_CODING_FOLDH && planes ? PPK_FOLDH_CHUNK_PLANES : planes; }
  unsigned holders = 0;                             // H (holder pair)
  // per k the 64-bin blocks that compare one plane fewer than stream_planes, and two fewer
  unsigned less1[PPK_RANK_SHORT_WORDS] = {}, less2[PPK_RANK_SHORT_WORDS] = {};
  std::vector<unsigned> order;                      // slot order of the sorted pairs, empty elsewhere
  // the corrections of the tile kernel's epilogue, bucketed by (lo / 32, hi / 256): bucket b = (lo / 32) * rt +
  // hi / 256 holds elements d_off[b] .. d_off[b + 1] of d_list, list_elem (2 or 4) bytes each
  void *d_list = nullptr;
  unsigned *d_off = nullptr;                        // qt * rt + 1 offsets
  unsigned list_elem = 0, qt = 0, rt = 0;           // npad / 32, npad / 256
  size_t list_count = 0;
};
// releases what `c` holds on the current device and leaves it empty (its kind kept)
void ppk_coding_free(PpkCoding &c);

struct ppk_db {
  int device = 0;
  size_t n = 0, npad = 0, nk = 0, s64 = 0, bbits = 0, words = 0;   // words = s64*bbits per (sample,k)
  uint64_t *d_skT = nullptr;               // [(k*words + w)*npad + sample]
  uint16_t *d_clu = nullptr;               // [npad] or nullptr
  PpkCoding coding[PPK_CODINGS] = {{PPK_CODING_RANK}, {PPK_CODING_FOLD}, {PPK_CODING_FOLD2}, {PPK_CODING_FOLDH}};
  // what the count pass found (ppk_db_rank_counts): the maxima of D, E = S + 2 and E2 = S3 + 2 over all positions and
  // per (k, 64-bin block) -- 3 x (1 + nk * s64) words -- then PPK_RANK_EXTRA words: the most two-holder values of any
  // position, their number over all positions, and (after an attempt at the two-holder pair) whether a (pair, k) had
  // more events than its field holds.  Empty where no count pass ran.
  std::vector<unsigned> rank_counts;
};
constexpr int RANK_BB = 14;          // the one bbits with a coded copy (the tile kernels' V2_BB)
#define PPK_RANK_EXTRA 3
#define PPK_FOLD2_SLOTS 256          // two-holder values per position the code pass has LDS slots for
#define PPK_FOLD2_MAX_PER_PAIR 63    // events per (pair, k): a 6-bit field of the tile kernel's correction word
#define PPK_FOLDH_SLOTS 1024         // shared values per position the holder count pass has LDS counters for
#define PPK_FOLDH_LADDER 7           // the holder bounds the choice tries: 4, 8, ... 256
#define PPK_FOLDH_MAX_CODES 16       // codes a sorted block of the holder pair may span (4 planes)
#define PPK_FOLD2_MAX_NK 5           // five 6-bit fields per correction word; k in 3 bits of an event

// A database whose per-pair counts the tile kernels cannot hold: more k-mer lengths than the fit tables are laid
// out for, or more than 128 count bits at a bbits other than PopPUNK's 14 (the wide-k tile kernel is built for
// bbits = 14).  Such sketches take the two-pass counts route: plain distances and whole-matrix edge lists only.
inline bool ppk_unfused(const ppk_db *db) {
  int bits = 1;
  while (((size_t)1 << bits) <= db->s64 * 64) ++bits;
  return db->nk > PPK_MAX_NK || (db->nk * (size_t)bits > 128 && db->bbits != 14);
}

// Run-time options ---------------------------------------------------------------
// Every PPK_* environment knob is read ONCE, when the library is first used (ppk_config()); after
// that only ppk_set_option() changes a value.  None of the tuning knobs changes results (the experiments build's
// `ablate` skips work to time the rest); the
// two ext_* options select between the readings of pp-sketchlib behaviour that cannot be checked
// in this tree (DESIGN.md "[EXT] assumptions").
struct PpkConfig {
#ifdef PPK_EXPERIMENTS
  // -- experiments build only (make -C poppunk_amd/csrc experiments; tools/ab_*.py): the product library has neither
  //    these fields nor options of these names
  std::atomic<long long> ablate{0};             // PPK_ABLATE: skip 1 epilogue, 2 compare, 4 DMA, 8 barriers, 16 first-copy wait, 64 the interior tiles' table copy, 128 stores; 32 LDS-table path off
  std::atomic<long long> map{0};                // PPK_MAP: tile order of dist_kernel_v2 (0 = XCD-contiguous runs)
  std::atomic<long long> strip{1};              // PPK_STRIP: strip tiles for the ragged right edge
  std::atomic<long long> edge_list_keep{1};     // PPK_EDGE_LIST_KEEP: the fused host edge call keeps its device list buffer between calls (0: allocate + free per call, measurement)
#endif
  // -- product options
  std::atomic<long long> rank_planes{1};        // PPK_RANK_PLANES: a bbits = 14 database whose self job runs whole tiles keeps a rank-coded copy (PPK_CODING_RANK) and self jobs compare it (0: no copy is built, none is read; same bits)
  std::atomic<long long> rank_fold{1};          // PPK_RANK_FOLD: where folding every single-holder bin value into two reserved codes lets a self job compare fewer planes, the database keeps the folded pair (PPK_CODING_FOLD) instead of the injective copy (0: never; 2: whenever the folded codes fit 12 planes, gain or none -- tests; same bits).  Read at creation; 0 at launch leaves a built pair unread.
  std::atomic<long long> rank_fold2{1};         // PPK_RANK_FOLD2: where coding the two-holder bin values like single-holder ones (their one match per value added back in the tile kernel's epilogue from an event list) lets a large self job compare fewer planes than both other codings, the database keeps the two-holder pair (PPK_CODING_FOLD2) instead (0: never; 2: whenever the caps allow, any size, gain or none -- tests; same bits).  Read at creation; 0 at launch leaves a built pair unread.
  std::atomic<long long> fold2_sort{1};         // PPK_FOLD2_SORT: the two-holder pair stores the positions of each k sorted by the codes they span, so that most 64-bin blocks span at most 64 codes (0: positions as stored; same bits).  Read at creation.
  std::atomic<long long> fold2_min_planes{6};   // PPK_FOLD2_MIN_PLANES: a self job on the two-holder pair compares 6 planes in the blocks that span at most 64 codes (7: such blocks compare 7, as every block spanning at most 128 does; same bits).  Read at launch.
  std::atomic<long long> rank_foldh{1};         // PPK_RANK_FOLDH: where folding every bin value with at most H holders (their matches added back in the tile kernel's epilogue from a list of per-pair counts) cuts the two-holder pair's compare stream to 0.6 of its planes or less, the database keeps the holder pair (PPK_CODING_FOLDH) beside it and self jobs read that (0: never; 2: whenever the caps allow, any size, gain or none -- tests; same bits).  Read at creation; 0 at launch leaves a built pair unread.
  std::atomic<long long> foldh_holders{0};      // PPK_FOLDH_HOLDERS: the holder bound H of the holder pair (0: the smallest of 4, 8, ... 256 that qualifies; any other value forces that H).  Read at creation.
  std::atomic<long long> foldh_min_planes{2};   // PPK_FOLDH_MIN_PLANES: a self job on the holder pair compares 2 planes in the blocks that span at most 4 codes and 3 in those that span at most 8 (3, 4: no block compares fewer; same bits).  Read at launch.
  std::atomic<long long> rank_short{1};         // PPK_RANK_SHORT: a self job on a rank-coded database compares one plane fewer in the 64-bin blocks whose positions hold at most half the values the planes can code (0: every block compares all planes; same bits).  Read at launch.
  std::atomic<long long> lds_table{1};          // PPK_LDS_TABLE: interior tiles of the default sketch shape fit from the (E, F) table in LDS (0: the general statement everywhere; same bits)
  std::atomic<long long> ksplit{1200};           // PPK_KSPLIT: tile-count threshold (at 5 k) of the small-job path
  std::atomic<long long> ksplit_wide{215};      // PPK_KSPLIT_WIDE: the same threshold for sketches whose tiles are not fitted from the LDS table (never above ksplit)
  std::atomic<long long> ksplit_long{1};        // PPK_KSPLIT_LONG: sketches of sketchsize64 >= 32 take the k-split path at any job size its scratch allows (0: the tile-count thresholds only)
  std::atomic<long long> ksplit_fused{1};       // PPK_KSPLIT_FUSED: small jobs run ONE launch (the last unit of a tile fits it); 0 = counts pass + regression pass
  std::atomic<long long> wide_kpg{0};           // PPK_WIDE_KPG: k-mer lengths per window of the wide-k tile kernel (0 = as many as 128 bits hold; smaller values send narrower k lists through it: tests)
  std::atomic<long long> ksplit_slices{0};      // PPK_KSPLIT_SLICES: pieces each k is cut into on the small-job path (0 = chosen from the job's size; measurement)
  std::atomic<long long> chunk_rows{8ll << 20};     // PPK_CHUNK_ROWS: rows per device buffer of ppk_query
  std::atomic<long long> prefault_threads{8};   // PPK_PREFAULT_THREADS
  std::atomic<long long> db_cache{1};           // PPK_DB_CACHE: ppk_query keeps its resident databases / buffers
  std::atomic<long long> progress{1};           // PPK_PROGRESS: progress meter of long host calls on fd 2
  std::atomic<long long> host_trace{0};         // PPK_HOST_TRACE: timeline of a host query on fd 2 (measurement)
  std::atomic<long long> launch_tiles{8000000}; // PPK_LAUNCH_TILES: pair tiles per kernel launch (a dispatch holds < 2^32 work-items)
  std::atomic<long long> knn_warm{32};          // PPK_KNN_WARM: the neighbour mode opens with 1/knn_warm of its rows, then cuts the list (0 = off)
  std::atomic<long long> knn_cut{4};            // PPK_KNN_CUT: a staged neighbour job cuts its list at knn_cut * n * knn entries (0: only when half full)
  std::atomic<long long> ksplit_scratch_mb{2048};   // PPK_KSPLIT_SCRATCH_MB: what the one-launch k-split path's partial counts may take (per device, kept); jobs that would need more run through the tile kernel
  std::atomic<long long> ks_grid_pad{0};        // PPK_KS_GRID_PAD: 1 = the one-launch k-split grid is one column wider, which puts the units of a tile on different XCDs (tests of the hand-over)
  std::atomic<long long> knn_lane_lists{0};     // PPK_KNN_LANE_LISTS: 1 = the per-lane selection lists of ppk_knn_rect_dev (the form before the one list per wavefront; measurement)
  std::atomic<long long> sweep_window{1};       // PPK_SWEEP_WINDOW: the boundary sweeps' classify pass finds a row's count by bisection over nested boundaries (0: every boundary evaluated for every row it keeps; same results)
  std::atomic<long long> net_window{0};         // PPK_NET_WINDOW: vertex ids per LDS table window of the network sweep's triangle stage (0 = as many as LDS holds; small values force the windowed path: tests; same results)
  std::atomic<long long> bt_lds_max{0};        // PPK_BT_LDS_MAX: largest component whose Brandes state lives in LDS (0 = as many vertices as LDS holds; small values force the global-state path: tests; results within rounding)
  std::atomic<long long> bt_small_max{64};      // PPK_BT_SMALL_MAX: largest component Brandes gives one wave for all its sources (0 = none; at most 256; results within rounding)
  std::atomic<long long> dbscan_search{0};      // PPK_DBSCAN_SEARCH: the DBSCAN assignment's search: 0 = the grid from 1 024 training points up, 1 = the scan of every training point, 2 = the grid at any size (same labels)
  std::atomic<long long> refine_local{1};       // PPK_REFINE_LOCAL: refineFit's local search scores through the bracket handle (ppk_refine_local_*); 0 = every evaluation through ppk_refine_score_dev (same fit)
  std::atomic<long long> density_hot_table{1};  // PPK_DENSITY_HOT_TABLE: ppk_density_counts_dev adds through a per-workgroup LDS table of hot pixels in front of the global atomics (0: every row one global atomic; same counts)
  std::atomic<long long> density_kde_presum{0}; // PPK_DENSITY_KDE_PRESUM: ppk_density_kde_dev sums the terms of lanes of a wave that share a window of nodes before the LDS add, for groups of at least this many lanes (0: every lane adds its own terms; same sums)
  std::atomic<long long> pairs_scratch_mb{1024}; // PPK_PAIRS_SCRATCH_MB: what the scratch of one chunk of a pair list may take as allocated (ppk_dist_pairs_dev: 2 x pairs x the bytes of one sample's sketch, plus the counts, stays within four fifths of it; same results)
  std::atomic<long long> edge_rows_fused{1};    // PPK_EDGE_ROWS_FUSED: the edge calls with rows take them from the tile kernel's epilogue where ppk_edge_rows_fused allows (0: always the edge call followed by the list kernel; same results)
  std::atomic<long long> pairs_chunk{0};        // PPK_PAIRS_CHUNK: pairs per chunk of a pair list whatever the cap says (0 = from the cap; tests; same results)
  std::atomic<long long> silhouette_scratch_mb{1024}; // PPK_SILHOUETTE_SCRATCH_MB: what the band of square rows of ppk_silhouette_dev may take as allocated (float32 [band][n] stays within four fifths of it; at least one row; same results)
  std::atomic<long long> silhouette_band{0};    // PPK_SILHOUETTE_BAND: samples per band whatever the cap says (0 = from the cap; tests; same results)
  std::atomic<long long> silhouette_window{0};  // PPK_SILHOUETTE_WINDOW: labels per LDS table window of the silhouette's sums stage (0 = as many as the table holds, 4 096; small values force the windowed path: tests; same results)
  std::atomic<long long> rand_scratch_mb{1024}; // PPK_RAND_SCRATCH_MB: what ppk_contingency_sums_dev's per-level state and the partial sums of one batch of pairs may take as allocated (a batch holds as many pairs as keep both within four fifths of it; at least one; same results)
  std::atomic<long long> rand_batch{0};         // PPK_RAND_BATCH: pairs per batch whatever the cap says (0 = from the cap; tests; same results)
  std::atomic<long long> rand_wave_max{64};     // PPK_RAND_WAVE_MAX: classes of up to this many samples take the wave route of the pair stage, longer ones the LDS table (0 forbids the wave route; a value of at least n forces it for every class: tests; same results)
  std::atomic<long long> rand_window{0};        // PPK_RAND_WINDOW: ranks per LDS table window of the pair stage (0 = as many as the table holds, 8 192; small values force the windowed path: tests; -1 forbids it: the classes of a pair that would need more than one window take the wave route; same results)
  std::atomic<long long> lineage_scratch_mb{1024}; // PPK_LINEAGE_SCRATCH_MB: what the two key buffers of one band of rows of ppk_strain_knn_dev's long route may take as allocated (a band holds as many rows of a strain as keep both within four fifths of it; at least one; same results)
  std::atomic<long long> lineage_lds_keys{0};   // PPK_LINEAGE_LDS_KEYS: the longest row (members of the strain but one) ppk_strain_knn_dev sorts in LDS (0 = as many keys as its table holds, 4 096; smaller values send shorter strains through the long route: tests; rows of up to 64 keep the wave route; same results)
  std::atomic<long long> sketch_lds_bins{0};    // PPK_SKETCH_LDS_BINS: the most bins whose minima ppk_sketch_dev's hash kernel keeps in LDS (0 = as many as LDS holds, 20 352; smaller values send smaller sketches through the global-atomics route: tests; same bits)
  std::atomic<long long> sketch_batch_mb{1024}; // PPK_SKETCH_BATCH_MB: the codes of one batch of samples of the host call ppk_sketch (whole samples, at least one; same bits)
  std::atomic<long long> sketch_batch{0};       // PPK_SKETCH_BATCH: samples per batch whatever the cap says (0 = from the cap; tests; same bits)
  std::atomic<long long> sketch_count_bits{0};  // PPK_SKETCH_COUNT_BITS: the bits B of a row of ppk_sketch_reads' count table, 4 .. 26 (0 = ppk_sketch_count_bits of the sample's code count; part of the rule: another B admits other k-mers on the table route; tests)
  std::atomic<long long> sketch_exact_rounds{64}; // PPK_SKETCH_EXACT_ROUNDS: the most select passes of ppk_sketch_reads' exact route over one group of samples before it gives up with an error (same bits)
  std::atomic<long long> refs_scratch_mb{4096}; // PPK_REFS_SCRATCH_MB: the most MiB ppk_pick_refs' component-local bit matrices may take (sum of |V|^2 / 8 bytes); over it the call fails and names the largest component
  std::atomic<long long> refs_lds_bits{65536};  // PPK_REFS_LDS_BITS: ppk_pick_refs keeps a component's bitsets in LDS up to this many vertices, 64 .. 65536; beyond it in global scratch (same bits; tests)
  std::atomic<long long> knn_list{0};           // PPK_KNN_LIST: entries of the neighbour-candidate list (0 = sized from n and knn)
  std::atomic<long long> host_parts_rows{16 << 20};   // PPK_HOST_PARTS_ROWS: ... from this many rows up
  std::atomic<long long> host_parts{2};         // PPK_HOST_PARTS: worker threads of a one-device host query (>= 16 Mi rows)
  // [EXT] a4: 0 = the b-bit collision adjustment is never in effect (upstream as recalled: it is
  // gated on expected == 0, where it is the identity); 1 = applied when expected > 0
  std::atomic<long long> ext_collision_adjust{0};
  // [EXT] a6: 0 = the fit uses the k-mer lengths before the FIRST J < 5/s; 1 = it skips every such k
  std::atomic<long long> ext_fit_skip{0};
};
PpkConfig &ppk_config();

// Error plumbing -------------------------------------------------------------
void ppk_set_error(const std::string &msg);
const std::string &ppk_error();          // the calling thread's message
int ppk_fail(int code, const std::string &msg);

// PPK_ERR_ARG for an id outside [0, PPK_MAX_DEVICES): what every entry point that is given a device id, a device list
// or a handle carrying one asks before its first HIP call and before it touches any per-device state
int ppk_check_device(int dev);
int ppk_check_arch(int device_id);       // ... and gfx950 / wave64 or an error, cached per device (ppk_devstate.hip)
int ppk_check_pair(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, size_t q_begin, size_t q_end);
bool ppk_interrupted();                  // the ppk_set_interrupt_check check asks to stop (ppk_host.hip)

#define PPK_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess)                                                          \
      return ppk_fail(PPK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Set the device for the scope of one API call, restoring the caller's device.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// An entry point's device: the id checked, then the device selected for the scope
#define PPK_ENTER_DEVICE(guard, dev)                             \
  if (int rc_dev_ = ppk_check_device(dev)) return rc_dev_;       \
  DeviceGuard guard(dev);                                        \
  if (!guard.ok) return ppk_fail(PPK_ERR_HIP, "cannot select device " + std::to_string(dev))

// One device's turn in a release loop: the first holder that has something to free there calls enter(), which selects
// the device and drains it -- once, however many holders follow.
struct PpkDeviceVisit {
  explicit PpkDeviceVisit(int d) : dev(d) {}
  void enter();
  const int dev;
  std::unique_ptr<DeviceGuard> guard;
};
// what ppk_host.hip keeps on visit.dev (upload ring, assign and query buffers), each under its own lock; the resident
// databases of the host queries on every device
void ppk_host_bufs_release(PpkDeviceVisit &visit);
void ppk_db_cache_clear();

// Device geometry (ppk_dist.hip): read once per device, never assumed ----------
struct PpkGeometry {
  int cus;              // compute units (hipDeviceProp_t::multiProcessorCount)
  unsigned xcd_shift;   // log2 of the XCD count (hipDeviceAttributeNumberOfXccs, rounded down to a power of two)
  int tile_slots;       // 512-thread workgroups of the pair-tile kernel resident at once (occupancy x cus: 512 on
                        // MI355X in SPX mode -- the "round" every tile-count rule of the route choice is stated in)
};
const PpkGeometry &ppk_geometry(int dev);      // cached in the device's state (ppk_devstate.hip)
PpkGeometry ppk_measure_geometry(int dev);     // ... from this, once per device (ppk_dist.hip: it names the tile kernel)

// Route of one band of pair tiles (ppk_dist.hip: ppk_choose_route) -------------
enum PpkRoute {
  PPK_ROUTE_TILE = 0,                // one workgroup per 256 x 32 pair tile, fit in its epilogue
  PPK_ROUTE_KSPLIT_ONE_LAUNCH = 1,   // nk * slices workgroups per tile, the last one fits it
  PPK_ROUTE_KSPLIT_TWO_PASS = 2,     // counts pass + regression pass
  PPK_ROUTE_TILE_WIDE = 3,           // the tile kernel with its count register windowed (more than 128 count bits)
  PPK_ROUTE_COUNTS_UNFUSED = 4       // raw counts to scratch + generic regression (bbits != 14 with > 128 count bits)
};
struct PpkRouteShape {
  size_t n_ref, q_rows, rows;   // refs, query rows of the band, distance rows of the band
  int self, nk, s64, cnt_bits, bbits;
  int mask, knn;                // fused boundary mode / neighbour mode
};
struct PpkRouteKnobs {          // ppk_set_option values (tile counts are stated for 512 workgroup slots)
  long long ksplit, ksplit_wide, ksplit_long, ksplit_fused, ksplit_slices, wide_kpg;
  size_t scratch_cap;           // bytes the k-split path's partial counts may take
};
struct PpkRouteChoice {
  int route, slices, from_parts;
  size_t tiles, limit, scratch_bytes;
};
PpkRouteChoice ppk_choose_route_impl(const PpkRouteShape &sh, const PpkGeometry &g, const PpkRouteKnobs &k);
bool ppk_self_job_takes_tiles(const ppk_db *db);      // (ppk_dist.hip) the one job shape that reads a coded copy
// one band of raw-plane match counts (MODE_COUNTS of the tile kernel) of a self job of `db`'s shape, ref side d_r, query
// side d_q: what ppk_coding.hip needs of the distance file; enqueues only
int ppk_counts_band_raw(const ppk_db *db, const uint64_t *d_r, const uint64_t *d_q, size_t q_begin, size_t q_end, void *d_cnt,
                        hipStream_t s);

// ---- the coded copies (ppk_coding.hip) ----
// What ppk_db_create builds, as a pure function of the count pass's read-back (`counts`: the layout
// ppk_launch_rank_count leaves -- 3 x (1 + nk * s64) maxima of D, E, E2, PPK_RANK_EXTRA words, E2 of every position),
// the shape, the device's tile_slots and the options rank_fold, rank_fold2, fold2_sort, rank_foldh.  No device touched.
struct PpkCodingPlan {
  int planes[3];                                   // of the codings of D, E and E2 (8, 10, 12; 0: past 4 096 codes)
  unsigned less1[3][PPK_RANK_SHORT_WORDS];         // their short flags on the stored blocks
  size_t sum[3];                                   // the planes a self job compares over all blocks with each (none: bbits)
  // the codings to try, in this order, until one is built; ends with -1 (the raw planes).  A coding is dropped where
  // the device is too full for it, the two-holder pair also where a (pair, k) overflows its event field.
  int chain[PPK_CODINGS];
  // chain[0] == PPK_CODING_FOLD2 only: the pair's slot order ("fold2_sort" 0: the identity), the flags and planes of
  // its sorted blocks (8, 7, 6), their sum, and whether the holder pair is to be tried beside it
  bool sorted;
  std::vector<unsigned> order;
  unsigned seven[PPK_RANK_SHORT_WORDS], six[PPK_RANK_SHORT_WORDS];
  std::vector<uint8_t> stream;
  size_t stream_sum;
  bool try_holder;
};
PpkCodingPlan ppk_plan_codings(const unsigned *counts, size_t n, size_t nk, size_t s64, size_t bbits, int tile_slots,
                               long long rank_fold, long long rank_fold2, long long fold2_sort, long long rank_foldh);
// The holder pair's bound.  ppk_holder_ladder: the bounds the count pass is to try (option "foldh_holders": that one
// alone), 0 where a cap refuses the pair outright -- more than five k, sketchsize64 > 32, nk >= PPK_RANK_SHORT_WORDS,
// n >= 2^24, more than PPK_FOLDH_SLOTS shared values at a position.  ppk_choose_holder_impl: the smallest of them for which,
// with each k's positions sorted by E_H (descending, ties by stored position), every block of 64 slots spans at most
// 16 codes -- and, under the default rule, the stream plane sum (2, 3 or 4 per block) is at most 0.6 of the two-holder
// pair's and the self job runs at least four rounds of tiles: a smaller saving does not pay for the creation pass.
// Option "rank_foldh" 2 takes the first H whose blocks fit, and lifts the cap on the entries from a sixteenth of the
// (pair, k) to all of them.  pos_e: E_H at [(k * 64 * s64 + position) * PPK_FOLDH_LADDER + rung].  H 0: no pair.
struct PpkHolderChoice {
  unsigned H = 0;
  std::vector<unsigned> order;             // [k][slot]
  std::vector<uint8_t> block_planes;       // [k][block]: 2, 3 or 4
  size_t max_entries = 0;
};
int ppk_holder_ladder(size_t n, size_t nk, size_t s64, size_t most_shared, long long foldh_holders, unsigned *ladder);
PpkHolderChoice ppk_choose_holder_impl(const unsigned *pos_e, const unsigned *ladder, int rungs, size_t n, size_t nk, size_t s64,
                                  int tile_slots, size_t fold2_sum, long long rank_foldh);
// the execution: the count pass, the plan, and the codings it names with their fallbacks; synchronises `s`
int ppk_db_build_codings(ppk_db *db, hipStream_t s);
// whether the options in force let a launch read coding `kind` ("rank_planes", "rank_fold", "rank_fold2", "rank_foldh")
bool ppk_coding_enabled(int kind);
// the flag words a launch on `c` carries under the options in force ("rank_short", "fold2_min_planes",
// "foldh_min_planes"; read at launch: one database runs either way)
void ppk_coding_launch_flags(const PpkCoding &c, unsigned *less1, unsigned *less2);

// Profiling hooks (ppk_prof_*) -------------------------------------------------
void ppk_prof_begin(hipStream_t s);
void ppk_prof_end(hipStream_t s);
void ppk_set_kernel_name(const char *name);
void ppk_prof_stage(const char *name, hipStream_t s);      // named stages of the multi-kernel entry points (nullptr ends)

// Kernel 2 / compaction (ppk_boundary.hip) ------------------------------------
enum EdgeLayout {
  EDGE_LINEAR_SELF = 0,     // bit b of word w <-> condensed row 64*w + b
  EDGE_LINEAR_NONSELF = 1,  // row = q*n_ref + r
  EDGE_TILED_SELF = 2,      // word (q - q_begin)*n_rtiles + rt, bit = r - 64*rt
  EDGE_TILED_NONSELF = 3,
  EDGE_ROWS = 4,            // linear; emit the row index itself (uint64 array)
  EDGE_COO_SEGMENTS = 5     // seg_words-long linear self masks back to back; emit i[], j[], segment[]
};

struct EdgeGeom {
  int layout;
  size_t n_rows;     // linear layouts: number of rows
  size_t n_samples;  // self: n (condensed)
  size_t n_ref;      // non-self: refs per query row
  size_t q_begin;    // tiled layouts
  size_t n_rtiles;   // tiled layouts
  long long int_offset;
  size_t seg_words;         // EDGE_COO_SEGMENTS: mask words per segment
  long long *coo_j;         // EDGE_COO_SEGMENTS: second and third output arrays (first = d_edges)
  long long *coo_seg;
  size_t seg_blocks;        // EDGE_COO_SEGMENTS with counts from the producer: compaction blocks per segment (seg_words / 256)
  unsigned long long *seg_totals;      // ... and room for one total per segment (device)
  int pair_interleaved;     // linear layouts: the mask came from mask_from_dist_counted_kernel (even / odd rows of 128 in word pairs)
};

// Workspace sizes / launchers; all enqueue on `s` and never synchronise.
size_t ppk_mask_words_linear(size_t n_rows);
size_t ppk_compact_ws_bytes(size_t n_words);
int ppk_launch_all_tuples(size_t n_entries, size_t num_ref, size_t num_queries, int self, long long int_offset,
                          long long *d_edges, hipStream_t s);
int ppk_launch_compact(const uint64_t *d_mask, size_t n_words, const EdgeGeom &g, void *d_ws,
                       long long *d_edges, size_t cap, unsigned long long *d_n_edges,
                       hipStream_t s, bool counted = false);
// a tiled mask whose producer staged the row of every set bit (the tile kernel's rows modes): the edges as above, and
// row e of d_rows (float [cap][2]) = the staged row of edge e; d_word_base: per mask word, where its first row is staged
int ppk_launch_compact_rows(const uint64_t *d_mask, size_t n_words, const EdgeGeom &g, void *d_ws, long long *d_edges,
                            size_t cap, unsigned long long *d_n_edges, const void *d_stage,
                            const unsigned long long *d_word_base, size_t stage_cap, float *d_rows, hipStream_t s);
int ppk_launch_assign(const float *d_dist, size_t n_rows, int slope, float x_max, float y_max,
                      float *d_out, hipStream_t s);
// BGMM assignment: labels and / or responsibilities (ppk_bgmm.hip)
int ppk_launch_bgmm_assign(const float *d_dist, size_t n_rows, const ppk_bgmm &m, int32_t *d_labels, float *d_resp,
                           hipStream_t s);

// The row test of a row-linear edge list: a float32 [n, 2] distance matrix (LINE, BGMM, QC) or an int32 label array
// (LABEL: generate_tuples).  Only the kind's own fields are read.
struct RowTest {
  enum Kind { LINE, BGMM, QC, LABEL } kind;
  int slope, inclusive;    // LINE: the refine line (src/boundary.cpp:82-95)
  float x_max, y_max;
  ppk_bgmm bgmm;           // BGMM: the row's label == bgmm.within_label
  int mode;                // QC: 0 distance too long (x > max_pi | y > max_a), 1 zero distance (x == 0 | y == 0)
  float max_pi, max_a;
  int within_label;        // LABEL: assign[row] == within_label
};
// The edge list of the rows that pass `t`, on the current device: n_ref == 0 a self (condensed) matrix, otherwise
// n_ref refs per query row.  The row count must fit the layout, except for LABEL, which takes it as it comes (as
// src/boundary.cpp:104 does).  A 16-byte aligned matrix takes the counted, pair-interleaved mask pass.
int ppk_row_edges(const void *d_rows, size_t n_rows, size_t n_ref, long long int_offset, const RowTest &t,
                  long long *d_edges, size_t cap, unsigned long long *d_n_edges, hipStream_t s);
// the model into scratch slot SLOT_BGMM of `dev`, enqueued on `s` (the caller holds a PpkCall)
int ppk_bgmm_to_device(int dev, const ppk_bgmm &m, const ppk_bgmm **d_model, hipStream_t s);

// ---- per-device state ------------------------------------------------------------------------------------------
// A per-device table.  The entry points have asked ppk_check_device: an id that still arrives out of range is a bug
// in this library, and the process stops there instead of reading another device's state.
template <typename T>
class PpkPerDevice {
  T v_[PPK_MAX_DEVICES];

 public:
  T &at(int dev) {
    if (dev < 0 || dev >= PPK_MAX_DEVICES) abort();
    return v_[dev];
  }
  template <typename F>
  void each(F &&f) {
    for (int d = 0; d < PPK_MAX_DEVICES; ++d) f(d, v_[d]);
  }
};

// Grow-only blocks of device / pinned host memory, on the current device.  grow(): nothing when the block holds
// `bytes` already; otherwise the device is synchronised (earlier work may still use the old block), the block freed and
// bytes + slack allocated.  A failed allocation leaves the block released and its size 0.
struct PpkDeviceBuf {
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t grow(size_t want, size_t slack = 0);
  void release();      // (the caller has synchronised)
};
struct PpkPinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t grow(size_t want, size_t slack = 0, unsigned flags = hipHostMallocDefault);
  void release();
};
// an untimed event, created where *e is still null; release destroys and clears it
hipError_t ppk_event_get(hipEvent_t *e);
void ppk_event_release(hipEvent_t *e);

// A ticket a kernel publishes into coherent pinned memory, polled by the host.  ONE counter per device for every user
// (with a counter each, one could hand out a number the pinned word still holds from another's last call, and the wait
// would return before the kernel had run); a zeroed 256-byte block per (device, user): their layouts differ.  The
// caller holds the device's PpkCall: one call at a time.
enum PpkTicketUser { PPK_TICKET_KNN_COUNT = 0, PPK_TICKET_SWEEP_CTRL = 1, PPK_TICKET_USERS = 2 };
void *ppk_ticket_block(int dev, PpkTicketUser user);      // null: no pinned memory
unsigned long long ppk_next_ticket(int dev);
// Polls `word` for `ticket` for at most budget_us, asking the stream every 1024 spins whether it has ended or failed;
// then drains the stream and looks once more.  `what`: the error message of a ticket that never came.
int ppk_wait_ticket(hipStream_t s, const volatile unsigned long long *word, unsigned long long ticket, long long budget_us,
                    const char *what);

// grow-only per-device scratch (ppk_devstate.hip)
enum { SLOT_LUT = 0, SLOT_MASK = 1, SLOT_WS = 2, SLOT_ITER_A = 3, SLOT_ITER_B = 4, SLOT_ITER_C = 5,
       SLOT_BOUNDS = 6, SLOT_HOST_IN = 7,      // HOST_IN: the uploaded input of a host-array call
       SLOT_TICKETS = 8,                       // one counter per tile of a k-split job: zero when allocated, left zero by every launch
       SLOT_WIDE = 9,                          // spill-slot pool of the wide-k tile kernel: its first page (the slot bitmap) zero when allocated, left zero by every launch
       SLOT_BGMM = 10,                         // the device copy of a ppk_bgmm that the fused BGMM edge call's tile kernels read
       SLOT_NET = 11,                          // the network sweep's counters, buckets, sorted adjacency and temp storage
       SLOT_NET_BT = 12,                       // its betweenness stage: relabelling, the local adjacency, the plan
       SLOT_NET_WORK = 13,                     // ... and one graph's partial sums and global-state slab (sized after its plan)
       SLOT_MST = 14,                          // the minimum spanning forest's ranks, labels and temp storage
       SLOT_NJ = 15,                           // neighbour joining's float64 triangles, row sums and best slots
       SLOT_EMBED = 16,                        // the embedding's sampling weights and prefix, Q32.32 deltas, Eq
       SLOT_DBSCAN = 17,                       // the DBSCAN fit's Boruvka state and sort storage; the labels behind its edge list
       SLOT_BGMM_FIT = 18,                     // the BGMM fit's per-workgroup partial sums, its sums, counters and k-means labels
       SLOT_SPARSE = 19,                       // extend's and lowerRank's row starts, sort pairs, counts, offsets and temp storage
       SLOT_REFINE = 20,                       // the refine fit's bit matrix, union-find parents and counters (one boundary at a time)
       SLOT_CLUSTERS = 21,                     // the cluster pair sums' first-bad-row / first-bad-number words
       SLOT_ASSIGN = 22,                       // the query links' counters, segment starts, overflow list and first ranks
       SLOT_ASSIGN_SORT = 23,                  // ... and, on the sort route only, its (query, label) keys, flags and temp storage
       SLOT_DENSITY = 24,                      // the density grids' coordinates, scale keys and first-offender words
       SLOT_PAIRS = 25,                        // a pair list's first-bad-pair word, sample flags and slots, the chunk's row image, ids and counts
       SLOT_SILHOUETTE = 26,                   // the silhouette's first-offender words, label histogram and band of square rows
       SLOT_RAND = 27,                         // the contingency sums' first-offender word and per-level state: segment ends, grouped sample indices, dense ranks, long classes
       SLOT_RAND_SUMS = 28,                    // ... and one batch of pairs' partial sums (sized after the levels have been read: growing a slot moves it)
       SLOT_LINEAGE = 29,                      // the strain lineages' first-offender words, id owners, segment and route tables, one band's key buffers and temp storage; the ranks' counts and offsets
       SLOT_SKETCH = 30,                       // the sketcher's control words, piece table and one group of samples' per-bin minima (read samples: floors, winner counts and count tables too)
       SLOT_REFS = 31,                         // the reference pick's control words, union-find parents, component layout, BFS parents, ranks and temp storage
       SLOT_REFS_BITS = 32,                    // ... and the component-local bit matrices with the large components' bitsets (sized after the layout has been read: growing a slot moves it)
       SLOT_EDGE_ROWS = 33,                    // the edge calls with rows: the reservation counter, a staging position per mask word (8 B) and the staged rows (8 B per edge of the caller's cap)
       SLOT_COUNT = 34 };
int ppk_scratch_get(int dev, int slot, size_t bytes, void **out);
// The fit tables in SLOT_LUT.  ppk_lut_ready: whether the tables of `key` (k list, random table, sketch size, options)
// already stand at `d_lut`; if not, none count as valid until the calling thread's launcher has enqueued lut_kernel
// for them and said so with ppk_lut_commit.  Inside a PpkCall scope of `dev`.
bool ppk_lut_ready(int dev, uint64_t key, const void *d_lut);
void ppk_lut_commit(int dev, const void *d_lut);
// Scope of one entry point that uses the scratch of `dev`: holds that device's (recursive) mutex and
// names the stream the call enqueues on, so that a slot last used on another stream is waited for
// (see ppk_devstate.hip).  ppk_scratch_get fails outside such a scope.
class PpkCall {
 public:
  PpkCall(int dev, hipStream_t s);
  ~PpkCall();
  PpkCall(const PpkCall &) = delete;
  PpkCall &operator=(const PpkCall &) = delete;

 private:
  int dev_, prev_dev_;
  hipStream_t prev_s_;
  unsigned long long prev_touched_;
};

// ---- host-side frame of every module but the distance queries and sweeps (ppk_host.hip, ppk_iterate.hip: their
// results may not fit the caller's buffer, see ppk_host_result): network, MST, NJ, embed, DBSCAN, BGMM, square, sparse
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// blocks of `per_block` items each: at least 1, at most `cap`
inline unsigned grid_for(size_t items, size_t per_block, unsigned cap) {
  size_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g < cap ? g : cap);
}

// A scratch layout, written once as a function of a Carve and run twice: on a null base to measure (`at` is the
// total), then on the block to bind.  Each take(p, count) points p at the next buffer, `count` elements rounded up to
// 256 bytes; `at` is the offset of the one after it.
struct Carve {
  char *base = nullptr;
  size_t at = 0;
  template <typename T>
  Carve &take(T *&p, size_t count) {
    p = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += align256(count * sizeof(T));
    return *this;
  }
};
template <typename Layout>
int ppk_scratch_carve(int dev, int slot, Layout &&layout) {
  Carve c;
  layout(c);
  void *base = nullptr;
  const int rc = ppk_scratch_get(dev, slot, c.at, &base);
  if (rc != PPK_OK) return rc;
  c = Carve{static_cast<char *>(base)};
  layout(c);
  return PPK_OK;
}

// The call's one synchronisation: the copies, in order, into the device's grow-only pinned read-back block (back to
// back at 8-byte offsets), then one hipStreamSynchronize of `s`.  *words: the block, valid until the next read-back
// on the device.  Inside a PpkCall scope of `dev` only.
struct PpkCopy {
  const void *src;
  size_t bytes;
};
int ppk_read_back(int dev, hipStream_t s, std::initializer_list<PpkCopy> copies, const unsigned long long **words);
// ends and offset index (o: 0 without d_off, may be null then) of edge k of a device edge stream, for an error message
bool ppk_read_edge(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off, size_t k,
                   long long *i, long long *j, long long *o);
// hipFuncSetAttribute(kernel, MaxDynamicSharedMemorySize, bytes) once per (kernel, device): whether it took
bool ppk_lds_opt_in(const void *kernel, int dev, int bytes);

// The host-array twin of a device entry point: `device` selected and its PpkCall scope held (null stream) around
// SLOT_HOST_IN carved by `layout` and `body` (the uploads, the device call and the downloads).
template <typename Layout, typename Body>
int ppk_host_frame(int device, Layout &&layout, Body &&body) {
  PPK_ENTER_DEVICE(guard, device);
  PpkCall call(device, nullptr);
  const int rc = ppk_scratch_carve(device, SLOT_HOST_IN, layout);
  return rc != PPK_OK ? rc : body();
}

void ppk_query_cache_clear();
// host entry points with a data-dependent result size (ppk_host.hip): one pass; a result that did not
// fit the caller's buffer stays parked on the device for the calling thread's ppk_parked_fetch
uint64_t ppk_token(const void *bytes, size_t len, uint64_t seed);
int ppk_host_result(int arrays, int device, size_t guess, size_t cap, size_t *n_out,
                    const std::function<int(size_t, void **, unsigned long long *)> &compute,
                    const std::function<int(const void *, size_t, size_t)> &copy_out);
void ppk_parked_clear();

// neighbours from kernel 1's tiles (ppk_square.hip): state = {count, cap, vals_off} + uint32 bounds[n]
int ppk_launch_knn_state_init(void *d_state, size_t n, unsigned long long cap, unsigned long long vals_off,
                              int reset_bounds, hipStream_t s);
int ppk_knn_from_candidates(int dev, const uint32_t *d_keys, const uint64_t *d_vals, size_t count, size_t n,
                            int knn, long long *d_i, long long *d_j, float *d_dist, hipStream_t s,
                            long long missing_j = 0);
int ppk_knn_compact(int dev, uint32_t *d_keys, uint64_t *d_vals, size_t count, size_t n, int knn, void *d_state,
                    long long *d_i, long long *d_j, float *d_dist, hipStream_t s);
int ppk_knn_band_dev(const ppk_db *db, const ppk_db *qry, const int32_t *kmers, const float *random_tbl, size_t n_clu,
                     int flags, int knn, int dist_col, size_t q_begin, size_t q_end, long long missing_j, long long *d_i,
                     long long *d_j, float *d_dist, unsigned long long *n_candidates, void *stream);
size_t ppk_rows_per_dispatch(const ppk_db *ref);     // query rows one kernel launch may cover (ppk_launch_dist)

// One call of kernel 1 (ppk_dist.hip): a band of query rows of `qry` (null: a self job of `ref`) against `ref`.  A
// caller sets the fields it means; the boundary's defaults are those of a call without one.
struct DistJob {
  const ppk_db *ref = nullptr, *qry = nullptr;
  const int32_t *kmers = nullptr;
  const float *d_rtab = nullptr;      // random-match table (null: none, n_clu = 1)
  size_t n_clu = 1;
  int flags = 0;
  size_t q_begin = 0, q_end = 0;
  void *d_out = nullptr;              // rows of the band; neighbour mode: the candidate arrays
  unsigned long long *d_n_failed = nullptr;
  uint64_t *d_mask = nullptr;         // edge bitmask of the fused boundary modes; neighbour mode: KnnState + bounds
  int slope = 2;                      // the boundary (src/boundary.cpp:42-58); plain distances are divided by the scales
  float x_max = 0.f, y_max = 0.f, scale_x = 1.f, scale_y = 1.f;
  int inclusive = 1;
  double *d_lut = nullptr;            // the log-J table's place, built by the call unless lut_ready
  bool lut_ready = false;
  const int *knn_args = nullptr;      // neighbour mode: {knn, distance column}
  const ppk_bgmm *d_bgmm = nullptr;   // device copy of the model whose label test fills d_mask instead of the line
  // with d_mask, the rows modes (ppk_edge_rows_fused said yes): float2 [rows_cap] staging, a staging position per mask
  // word (parallel to d_mask) and the zeroed reservation counter
  void *d_rows_stage = nullptr;
  unsigned long long *d_rows_base = nullptr, *d_rows_count = nullptr;
  size_t rows_cap = 0;
  hipStream_t s = nullptr;
};
// enqueues only; a band of more rows than one dispatch holds goes out as several launches
int ppk_launch_dist(const DistJob &job);
// whether an edge call with rows over this band takes the rows from the tile kernel's epilogue (else: the two-step)
bool ppk_edge_rows_fused(const ppk_db *ref, const ppk_db *qry, size_t q_begin, size_t q_end);

// Kernel 1 for a list of pairs (ppk_dist.hip, ppk_dist_pairs_dev): validated ids in, rows of d_out out.  The caller
// holds the PpkCall and has staged the tables; synchronises `s` once (the check of the ids).
struct PairsJob {
  const ppk_db *ref = nullptr, *qry = nullptr;
  const int32_t *kmers = nullptr;
  const float *d_rtab = nullptr;
  size_t n_clu = 1;
  int flags = 0;
  const long long *d_i = nullptr, *d_j = nullptr;
  size_t stride = 1, n_pairs = 0;
  long long int_offset = 0;
  void *d_out = nullptr;
  unsigned long long *d_n_failed = nullptr;
  double *d_lut = nullptr;
  bool lut_ready = false;
  hipStream_t s = nullptr;
};
int ppk_launch_pairs(const PairsJob &job);

// ---- helper threads ----------------------------------------------------------------
// A host call uses a dozen short-lived helpers (page touchers, per-device workers, hash lanes); starting
// a thread costs 30-100 us and jitters to several hundred, which is the scale of the call's whole start-up.
// They are therefore taken from a grow-only pool of parked threads (ppk_host.hip).  A task's completion is
// the ticket's flag; ppk_pool_wait spins with yield (tasks here last from 0.1 to 10 ms).  A forked child
// starts with an empty pool of its own.
typedef std::shared_ptr<std::atomic<int>> PpkTicket;
PpkTicket ppk_pool_run(std::function<void()> fn);
void ppk_pool_wait(const PpkTicket &t);

// ---- uploads of pageable host arrays ---------------------------------------------------
// hipMemcpy from PAGEABLE host memory goes through the runtime's bounce buffer with one thread copying:
// ~20 GB/s on this host, a third of the link, and several copies in flight do not help (tools/
// ab_k2_threads.py).  ppk_upload stages the array itself: helper threads copy 32 MB pieces into a pinned ring
// (kept per device) and each piece goes on as an asynchronous DMA while the next is being copied.  Returns
// when the last host piece has been copied (the caller may re-use `h_src`); the DMAs are ordered on `s`.
int ppk_upload(int device, void *d_dst, const void *h_src, size_t bytes, hipStream_t s);

// ---- pre-touching of host result arrays -------------------------------------------
// A result lands in the caller's (normally freshly allocated, not yet touched) pageable array:
// its first-touch page faults -- one per 4 KB, taken serially by the runtime's staging copy --
// cost more than the PCIe transfer (10k genomes: 29 ms per ppk_query call against 14 with the
// pages touched).  A few threads therefore write the first byte of every page, front to back in
// interleaved 2 MB blocks, while the inputs upload and the first chunk computes; a download waits
// until the blocks under it are done (a toucher never writes behind a download).
class HostToucher {
 public:
  // `segments` (optional): byte ranges [first, second) of the array in the order they will be needed (the
  // sub-bands of several worker entries interleave); without them the array is touched front to back.
  HostToucher(void *out, size_t total_bytes, std::vector<std::pair<size_t, size_t>> segments = {})
      : out_(out), total_(total_bytes) {
    int nt = (int)ppk_config().prefault_threads.load();
    if (nt > 64) nt = 64;
    if (!out || total_bytes < ((size_t)8 << 20) || nt < 0) nt = 0;
    nt_ = nt;
    n_blocks_ = (total_bytes + kBlock - 1) / kBlock;
    if (nt > 0 && !segments.empty()) {
      // the 2 MB blocks in the order of the segments that (first) overlap them
      order_.reserve(n_blocks_);
      std::vector<char> taken(n_blocks_, 0);
      for (const auto &sg : segments) {
        const size_t e = sg.second < total_bytes ? sg.second : total_bytes;
        if (e > sg.first)
          for (size_t blk = sg.first / kBlock; blk <= (e - 1) / kBlock && blk < n_blocks_; ++blk)
            if (!taken[blk]) {
              taken[blk] = 1;
              order_.push_back(blk);
            }
        seg_end_.push_back(order_.size());
      }
      for (size_t blk = 0; blk < n_blocks_; ++blk)
        if (!taken[blk]) order_.push_back(blk);
    }
    done_ = std::vector<std::atomic<size_t>>((size_t)(nt > 0 ? nt : 1));
    for (auto &a : done_) a.store(0);
    // the first helper advises the kernel and starts the others: the constructor itself returns at once (the
    // advice on 400 MB plus eight thread starts were 0.2 ms in front of the first kernel launch)
    if (nt > 0) lead_ = ppk_pool_run([this]() { lead(); });
  }
  ~HostToucher() { join(); }
  HostToucher(const HostToucher &) = delete;
  HostToucher &operator=(const HostToucher &) = delete;
  // every page of [0, end_byte) has been touched (front-to-back order only)
  void wait(size_t end_byte) {
    if (!nt_) return;
    size_t need = (end_byte + kBlock - 1) / kBlock;
    if (!order_.empty()) need = n_blocks_;      // (a caller mixing the two forms waits for everything)
    wait_blocks(need);
  }
  // every page of segment i (and of all segments before it in the order) has been touched
  void wait_segment(size_t i) {
    if (!nt_) return;
    wait_blocks(i < seg_end_.size() ? seg_end_[i] : n_blocks_);
  }
  void join() {
    if (lead_) ppk_pool_wait(lead_);
    lead_.reset();
  }

 private:
  static constexpr size_t kBlock = (size_t)2 << 20;
  void wait_blocks(size_t need) {
    if (need > n_blocks_) need = n_blocks_;
    for (int t = 0; t < nt_; ++t) {
      const size_t mine = need > (size_t)t ? (need - (size_t)t + (size_t)nt_ - 1) / (size_t)nt_ : 0;
      while (done_[(size_t)t].load(std::memory_order_acquire) < mine) std::this_thread::yield();
    }
  }
  void lead() {
    // transparent huge pages for the (whole 2 MB blocks of the) result: a first touch then maps
    // 2 MB at a time -- measured on the MI355X host: 400 MB touched by 8 threads in 2.5 ms against
    // 35 ms with 4 KB pages (tools/ubench_host_out.hip).  numpy asks for the same on its own large
    // allocations; other callers' arrays get it here.  Advice only: failure is harmless.
    const size_t a0 = ((size_t)out_ + kBlock - 1) / kBlock * kBlock, a1 = ((size_t)out_ + total_) / kBlock * kBlock;
    if (a1 > a0) (void)madvise(reinterpret_cast<void *>(a0), a1 - a0, MADV_HUGEPAGE);
    std::vector<PpkTicket> helpers;
    for (int t = 1; t < nt_; ++t) helpers.push_back(ppk_pool_run([this, t]() { run(t); }));
    run(0);
    for (auto &h : helpers) ppk_pool_wait(h);
  }
  void run(int t) {
    volatile char *base = static_cast<volatile char *>(out_);
    size_t done = 0;
    for (size_t pos = (size_t)t; pos < n_blocks_; pos += (size_t)nt_) {
      const size_t blk = order_.empty() ? pos : order_[pos];
      const size_t b0 = blk * kBlock, b1 = b0 + kBlock < total_ ? b0 + kBlock : total_;
      base[b0] = 0;
      for (size_t a = (((size_t)out_ + b0) / 4096 + 1) * 4096 - (size_t)out_; a < b1; a += 4096) base[a] = 0;
      done_[(size_t)t].store(++done, std::memory_order_release);
    }
  }
  void *out_;
  size_t total_, n_blocks_ = 0;
  int nt_ = 0;
  std::vector<size_t> order_, seg_end_;
  std::vector<std::atomic<size_t>> done_;
  PpkTicket lead_;
};

