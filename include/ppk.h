/*
 * ppk.h -- C ABI of libppk_hip.so, the MI355X (gfx950) core/accessory distance
 * engine for PopPUNK.  Plain pointers and sizes only; no exceptions cross this
 * boundary (every call returns 0 on success, a PPK_ERR_* code otherwise, and
 * ppk_last_error() gives the message for the calling thread).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the bacpop/PopPUNK checkout; [EXT] = the un-vendored
 * pp-sketchlib dependency that PopPUNK reaches through that call site).
 *
 * Conventions
 *  - Sketches on the host: uint64 [n][nk][sketchsize64*bbits], i.e. for every
 *    sample the per-k datasets of the sketch HDF5 file (PopPUNK/web.py:14-61)
 *    concatenated in klist order.  Word [blk*bbits + b] holds bit b of bins
 *    64*blk .. 64*blk+63.
 *  - Distance rows (PopPUNK/utils.py:199-226, src/boundary.cpp:22-37):
 *      self    : row <-> (i<j), row-major upper triangle ("condensed");
 *                sample i is the "query", sample j the "ref";
 *      non-self: row = q*n_ref + r.
 *  - "d_" arguments are device pointers on the database's device; `stream` is
 *    a hipStream_t passed as void* (NULL = the default stream).  Device entry
 *    points only enqueue work; they do not synchronise.
 *
 * CONTRACT SURFACE vs EXTRAS.  Everything here is the hot path of SURVEY.md section 8 (kernel 1, kernel 2, the
 * sweeps, long <-> square, kNN, distance QC, the database-file reader) EXCEPT the entry points tagged
 *     [OUTSIDE SURVEY 8]
 * below: ppk_generate_all_tuples[_dev], ppk_lower_rank, ppk_extend, ppk_extend_sketches[_dbs].  Those mirror
 * the rest of the reference's extension module (src/boundary.cpp:125-150, src/extend.cpp:52-246), which SURVEY.md
 * section 2 marks out of scope.  Their CPU oracles (oracle/oracle.py) are restatements made by READING the
 * reference source -- src/extend.cpp needs Eigen and pybind11 to build, absent here -- so their parity is
 * UNPINNED; the only way to pin them is the `poppunk_refine` half of tools/pin_upstream.py on a machine with the
 * reference's extension installed.  They are kept working and tested, and not developed further.
 */
#ifndef PPK_H
#define PPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPK_OK 0
#define PPK_ERR_ARG 1      /* bad argument                                   */
#define PPK_ERR_HIP 2      /* a HIP runtime call failed / no usable device   */
#define PPK_ERR_CAPACITY 3 /* caller-provided output too small               */
#define PPK_ERR_STATE 4    /* call sequence error                            */
#define PPK_ERR_INTERRUPTED 5 /* the interrupt check asked to stop (Ctrl-C)   */
#define PPK_REFINE_NOT_NESTED 6 /* ppk_refine_local_create_dev: the two lines form no bracket (use ppk_refine_score_dev) */

/* flags of ppk_query / ppk_dist_dev: the random_correct and jaccard booleans of
 * pp_sketchlib.queryDatabase (PopPUNK/sketchlib.py:528-537,:547-566) */
#define PPK_FLAG_RANDOM_CORRECT 1
#define PPK_FLAG_JACCARD 2
/* output raw equal-bin counts, uint32 [n_pairs][nk] (parity testing: the
 * integer half of the path must be bit-identical to the CPU) */
#define PPK_FLAG_COUNTS 4

/* Threading: entry points may be called from any host thread.  Device entry points share
 * grow-only per-device scratch (log-J table, edge bitmask, sort buffers): each holds the
 * device's mutex while it enqueues, and a scratch block last used on another stream is waited
 * for (an event) before it is re-used, so calls on different streams are ordered where they
 * share scratch and concurrent elsewhere.  The host-buffer query (ppk_query, ppk_query_dbs) runs
 * one call at a time, like the blocking binding it replaces; inside a call every listed device has
 * its own worker thread. */
const char *ppk_last_error(void);
/* frees the per-device scratch, ppk_query's cached resident databases and its result buffers
 * (synchronises each device that holds any) */
int ppk_release_scratch(void);
const char *ppk_version(void); /* replaces pp_sketchlib.version (PopPUNK/sketchlib.py:34) */
int ppk_device_count(int *n);

/* Run-time options.  Each has a PPK_<NAME> environment variable that is read ONCE, when the library is first
 * used; afterwards only ppk_set_option changes it.  None changes a result except the two [EXT] switches.  Every one
 * of them is drawn by the randomised campaign (tests/soak_case.py).
 *   kernel 1
 *     "ksplit" (1200), "ksplit_wide" (215)  tile-count threshold (at 5 k) below which a job runs one workgroup per
 *                       (tile, k) -- the small-job path; the second applies to sketch shapes whose
 *                       tiles are not fitted from the LDS table (from sketchsize64 16 up the threshold is at least
 *                       700 tiles whatever nk: measured, profiles/r05/ksplit_s1024_other_shapes.txt); 0 = off
 *     "ksplit_long" (1)    sketches of sketchsize64 >= 32 (PopPUNK's default is 156) take that path at ANY job size
 *                          whose scratch stays below 4 GB -- one k at a time keeps a k of the database in the Infinity
 *                          Cache and short units fill the last round of workgroup slots; distances and the fused
 *                          edge list alike; 0 = the tile-count thresholds only
 *     "ksplit_fused" (1)   small jobs run ONE launch (the tile's last unit fits it); 0 = counts pass + fit pass
 *     "ksplit_slices" (0)  pieces each k is cut into on the small-job path (0 = from the job's size)
 *     "ksplit_scratch_mb" (2 048)  what the one-launch k-split path's partial counts may take (16 KB per tile and unit,
 *                          kept per device); a job that would need more -- or that the device cannot give it -- runs
 *                          through the tile kernel, which needs none
 *     "ks_grid_pad" (0)    1 = the one-launch k-split grid is one (empty) column wider: the workgroups of a tile
 *                          then run on different XCDs, which is what its hand-over is written for and what the
 *                          default, multiple-of-8 grid never does (tests; same results, no measurable cost)
 *     "lds_table" (1)      interior tiles of the default shape (3-5 k, s = 1024) fit from the (E, F) table in LDS
 *     "wide_kpg" (0)       k-mer lengths per window of the wide-k tile kernel (0 = as many as 128 count bits hold;
 *                          a smaller value sends narrower k lists through that kernel)
 *     "launch_tiles" (8 000 000)  pair tiles per kernel launch: a dispatch holds fewer than 2^32 work-items, so bands
 *                          of more tiles -- 370 000 genomes against themselves and up -- go out as several launches
 *   pair lists (ppk_dist_pairs_dev)
 *     "pairs_scratch_mb" (1 024)  what the scratch of one chunk of the list (its row image and counts) may take as
 *                          allocated: a chunk holds as many pairs as keep 2 x pairs x (bytes of one sample's sketch)
 *                          within four fifths of it (a scratch slot is allocated with a quarter to spare); at least one
 *     "pairs_chunk" (0)    pairs per chunk, whatever the cap says (0 = from the cap; tests)
 *   edge lists with rows (ppk_dist_edges_rows_dev, ppk_dist_bgmm_edges_rows_dev)
 *     "edge_rows_fused" (1)  the rows come out of the tile kernel's own epilogue where the band runs whole tiles of the
 *                          plain packed kernels; 0 = always the edge call followed by the list kernel (same results)
 *   neighbours from tiles
 *     "knn_list" (0 = sized from n and knn), "knn_warm" (32), "knn_cut" (4)  the candidate list, its staged
 *                          opening and where it is cut back to the best knn per sample
 *     "knn_lane_lists" (0) 1 = ppk_knn_rect_dev / ppk_knn_dev select with one sorted list per LANE (the form before the
 *                          one list per wavefront; kept so that the two can be timed side by side)
 *   boundary sweeps
 *     "sweep_window" (1)   the classify pass of ppk_threshold_iterate_1d/2d_dev finds how many boundaries hold a row by
 *                          bisection when the boundaries are nested outwards (refine's sweeps are); 0 = every boundary
 *                          is evaluated for every row the filter keeps (same results; the GPU suite runs both)
 *   refine fit
 *     "refine_local" (1)   refineFit's local search scores its evaluations through the bracket handle
 *                          (ppk_refine_local_*); 0 = every evaluation through ppk_refine_score_dev (same fit)
 *   density grids
 *     "density_hot_table" (1)  ppk_density_counts_dev adds through a per-workgroup LDS table of hot pixels in front of
 *                          the global atomics; 0 = one global atomic per row (same counts)
 *     "density_kde_presum" (0)  ppk_density_kde_dev sums the terms of lanes of a wave whose rows share a window of
 *                          nodes before the LDS add, for groups of at least this many lanes (at most 64); 0 = every
 *                          lane adds its own terms (same sums)
 *   silhouette (ppk_silhouette_dev; exercised by its own GPU tests, not by the campaign)
 *     "silhouette_scratch_mb" (1 024)  what the band of square rows may take as allocated: a band holds as many samples
 *                          as keep float32 [band][n] within four fifths of it; at least one
 *     "silhouette_band" (0)    samples per band, whatever the cap says (0 = from the cap; tests)
 *     "silhouette_window" (0)  labels per LDS table window of the sums stage (0 = as many as the table holds, 4 096;
 *                          small values force the windowed path: tests)
 *   reference picking (ppk_pick_refs_dev; exercised by its own GPU tests, not by the campaign)
 *     "refs_scratch_mb" (4 096)  the most MiB the component-local bit matrices may take (the sum of |V|^2 / 8 bytes over
 *                          the components of 3 or more vertices); over it the call fails with PPK_ERR_CAPACITY and names
 *                          the largest component (a row-compressed adjacency is not built)
 *     "refs_lds_bits" (65 536)  a component's bitsets live in LDS up to this many vertices, 64 .. 65 536, and in global
 *                          scratch beyond (the same bits; small values force the global route: tests)
 *   contingency sums (ppk_contingency_sums_dev; exercised by its own GPU tests, not by the campaign)
 *     "rand_scratch_mb" (1 024)  what the per-level state and one batch of pairs' partial sums may take as allocated: a
 *                          batch holds as many pairs as keep both within four fifths of it; at least one
 *     "rand_batch" (0)     pairs per batch, whatever the cap says (0 = from the cap; tests)
 *     "rand_wave_max" (64) classes of up to this many samples take the wave route of the pair stage, longer ones the
 *                          LDS table; 0 forbids the wave route, a value of at least n forces it for every class (tests)
 *     "rand_window" (0)    ranks per LDS table window of the pair stage (0 = as many as the table holds, 8 192; small
 *                          values force the windowed path: tests); -1 forbids the windowed path: the classes of a pair
 *                          that would need more than one window take the wave route.  A single table cannot be forced
 *                          beyond the 8 192 ranks it holds.
 *   strain lineages (ppk_strain_knn_dev; exercised by its own GPU tests, not by the campaign)
 *     "lineage_scratch_mb" (1 024)  what the two key buffers of one band of rows of the long route may take as
 *                          allocated: a band holds as many rows of a strain as keep both within four fifths of it; at
 *                          least one
 *     "lineage_lds_keys" (0)   the longest row (members of the strain but one) sorted in LDS (0 = as many keys as the
 *                          table holds, 4 096; smaller values send shorter strains through the long route: tests; rows
 *                          of up to 64 keys keep the wave route)
 *   sketching (ppk_sketch_dev, ppk_sketch; exercised by their own GPU tests, not by the campaign)
 *     "sketch_lds_bins" (0)    the most bins whose minima the hash kernel keeps in LDS (0 = as many as LDS holds,
 *                          20 352; smaller values send smaller sketches through the global-atomics route: tests)
 *     "sketch_batch_mb" (1 024)  the codes of one batch of whole samples of the host call (at least one sample)
 *     "sketch_batch" (0)   samples per batch, whatever the cap says (0 = from the cap; tests)
 *     "sketch_count_bits" (0)  read samples: the bits B of a row of the count table, 4 .. 26 (0 = from the sample's own
 *                          code count; PART OF THE RULE -- another B admits other k-mers on the table route; tests)
 *     "sketch_exact_rounds" (64)  read samples: the most select passes of the exact route over one group before the
 *                          call gives up with PPK_ERR_CAPACITY
 *   host calls
 *     "chunk_rows" (8 Mi)  rows per sub-band of a host query (about an eighth of the job, at least 1 Mi, below 16 Mi
 *                          rows); also scales the pieces of the fused host edge call
 *     "host_parts" (2), "host_parts_rows" (16 Mi)  worker entries of a ONE-device host query of at least that many
 *                          rows: one download is in flight while the next is being set up
 *     "prefault_threads" (8)  helper threads that touch the pages of a fresh result array ahead of the downloads
 *     "db_cache" (1)       ppk_query / ppk_query_edges keep their resident databases and buffers between calls
 *     "progress" (1)       progress meter of long host calls on file descriptor 2
 *     "host_trace" (0)     a timeline of every host query (launches, page touching, downloads) on file descriptor 2
 *   [EXT] readings of pp-sketchlib behaviour that this tree cannot verify:
 *     "ext_collision_adjust" 0 (default): the b-bit collision adjustment of calc_intersize is
 *                              never in effect (upstream gates it on expected == 0, as recalled);
 *                            1: applied when expected = nbins >> bbits is > 0
 *     "ext_fit_skip"         0 (default): the regression uses the k-mer lengths before the first
 *                              J < 5/nbins; 1: it skips every such k and keeps the rest
 * Not options of this library: the ablation mask ("ablate"), the rejected tile orders ("map"), "strip" and
 * "edge_list_keep" exist only in the experiments build (make -C poppunk_amd/csrc experiments ->
 * libppk_hip_exp.so, loaded by the measurement tools through tools/_exp.py). */
int ppk_set_option(const char *name, long long value);
int ppk_get_option(const char *name, long long *value);

/* Interrupts and progress of the long host calls (ppk_query, ppk_query_dbs), the contract of the
 * bindings they replace: the reference's C++ loops poll PyErr_CheckSignals and stop on Ctrl-C
 * (src/extend.cpp:263,:284-286; pp-sketchlib the same [EXT]) and print a progress meter to stderr,
 * which PopPUNK silences with an fd-level redirect around re-queries (PopPUNK/utils.py:61-83,
 * PopPUNK/sketchlib.py:546).
 *  - `check` (NULL = none) is called from the calling thread -- between sub-bands (every ~64 MB of
 *    results, a few ms) when it does the work itself, every ~0.2 ms while worker threads do (several
 *    device entries); a non-zero return abandons the call: nothing more is launched, the devices are
 *    drained, PPK_ERR_INTERRUPTED is returned.  The Python mirror passes a check that lets Python's
 *    signal handlers run.
 *  - option "progress" (default 1): jobs of more than a few sub-bands write "\rProgress (GPU): nn.n%"
 *    to file descriptor 2 with write(2): fd-level redirection silences it. */
int ppk_set_interrupt_check(int (*check)(void));

/* ------------------------------------------------------------------------
 * Resident sketch database: the flat bin-sketch array of one sample list,
 * copied to HBM once and re-laid out as [k][word][sample] so that a
 * wavefront reads 64 samples' copies of one word with one coalesced access.
 * Replaces the per-call HDF5 -> Reference objects -> device copy that
 * pp_sketchlib.queryDatabase does internally [EXT] (call sites
 * PopPUNK/sketchlib.py:528-537,:584-593).
 * `clu` (nullable) gives each sample's random-match cluster id (the
 * /random group written by pp_sketchlib.addRandom, PopPUNK/sketchlib.py:437-473).
 * `src_on_device` != 0: `sk` is already a device pointer on `device_id`.
 */
typedef struct ppk_db ppk_db;

int ppk_db_create(int device_id, const uint64_t *sk, size_t n, size_t nk,
                  size_t sketchsize64, size_t bbits, const uint16_t *clu,
                  int src_on_device, void *stream, ppk_db **out);
void ppk_db_destroy(ppk_db *db);
size_t ppk_db_size(const ppk_db *db);
/* A bbits = 14 database whose self job runs whole pair tiles (option "ksplit" and the job's size decide) also keeps
 * a rank-coded copy: every bin value replaced by its rank among the distinct values of its (k, bin) position over the
 * database's samples, in 8, 10 or 12 bit-planes instead of 14 (the smallest that hold the ranks; none beyond 4 096
 * distinct values).  Equal values keep equal codes and different values different ones, so a self job on such a
 * database counts the same matches, and returns the same bits, from fewer planes.  Costs up to 12/14 of the
 * database's memory again and one pass at creation; option "rank_planes" 0 (PPK_RANK_PLANES) builds and reads none.
 * ppk_db_rank_planes: the planes of the copy, 0 without one.  ppk_db_rank_read (tests): the copy as it lies,
 * [k][block * planes + plane][padded samples (a multiple of 256)] uint64, `words` = its exact length.
 * A 64-bin block none of whose positions holds more than 2^(planes - 1) distinct values is "short": the top plane of
 * its codes is zero in every sample, and a self job compares planes - 1 planes there (the copy keeps all of them).
 * Option "rank_short" 0 (PPK_RANK_SHORT), read at launch, compares every plane of every block: same bits.
 * ppk_db_rank_block_planes: the planes compared per block under "rank_short" 1, out[k * sketchsize64 + block] = planes
 * or planes - 1; `cap` >= nk * sketchsize64 bytes.  An error without a coded copy. */
int ppk_db_rank_planes(const ppk_db *db);
int ppk_db_rank_read(const ppk_db *db, uint64_t *out, size_t words);
int ppk_db_rank_block_planes(const ppk_db *db, uint8_t *out, size_t cap);
/* The folded pair.  A bin value that exactly one sample holds at its (k, bin) position can match nothing in a self job,
 * yet takes a code of its own in the copy above.  Where that lets a self job compare fewer planes over all blocks, the
 * database keeps two coded copies instead of the one: a value with at least two holders gets the code 2 + its rank among
 * such values of its position in both, and every single-holder value gets 0 in the ref-side copy and 1 in the query-side
 * one.  A position then spans E = S + 2 codes (S: its values with at least two holders); the planes and the short blocks
 * follow from E as they follow from the distinct values above.  A triangular self job compares two different samples, one
 * from each copy, so every count and every bit is that of the raw planes; a job of a handle against itself as the query
 * does not read the pair.  Costs 2 x planes/14 of the database's memory.  Option "rank_fold" (PPK_RANK_FOLD, default 1),
 * read at creation: 0 never builds the pair, 2 builds it whenever the codes fit 12 planes (tests); 0 at launch leaves a
 * built pair unread (raw planes).  ppk_db_rank_planes and ppk_db_rank_block_planes report what the distinct values give
 * either way, and ppk_db_rank_read builds the injective copy on demand where only the pair was built.
 * ppk_db_fold_planes: the planes of the pair, 0 without one.  ppk_db_fold_block_planes, ppk_db_fold_read (which: 0 the
 * ref side, 1 the query side): as their rank_ namesakes, an error without a pair. */
int ppk_db_fold_planes(const ppk_db *db);
int ppk_db_fold_block_planes(const ppk_db *db, uint8_t *out, size_t cap);
int ppk_db_fold_read(const ppk_db *db, int which, uint64_t *out, size_t words);
/* The two-holder pair.  Almost every value the folded pair still codes has exactly two holders: a chance collision, which
 * can match in exactly one pair of the triangular job (its higher holder as ref, its lower as query).  Where that lets a
 * large self job compare fewer planes than both codings above, the database keeps this pair instead: a value with at
 * least three holders gets 2 + its rank among such values, every other value 0 in the ref-side copy and 1 in the
 * query-side one, so a position spans E2 = S3 + 2 codes.  The compare then counts every two-holder value's one match
 * short; the database lists them as events (hi, lo, k), bucketed by (lo / 32, hi / 256), and the tile kernel adds a
 * tile's events to its counts before the fit: every count and every bit is that of the raw planes.  Built only at 8
 * planes, at most five k, at most 256 two-holder values per position and 63 events per (pair, k); a database past a cap
 * keeps the copies above.  Option "rank_fold2" (PPK_RANK_FOLD2, default 1), read at creation: 1 builds the pair where
 * its plane sum over the blocks is the lowest of the three codings, "rank_fold" is not 0 and the self job runs at least
 * four rounds of tiles; 0 never; 2 whenever the caps allow (tests).  0 at launch leaves a built pair unread.
 * ppk_db_fold2_planes / _block_planes / _read: as their fold_ namesakes.  ppk_db_fold2_events: the number of events
 * (and of buckets: (padded samples / 32) x (padded samples / 256)); ppk_db_fold2_events_read: the buckets + 1 offsets,
 * bucket (lo / 32) * (padded samples / 256) + hi / 256, and the events, hi % 256 | (lo % 32) << 8 | k << 13, in no
 * order within a bucket.  ppk_db_rank_counts: what the count pass found, 3 x (1 + nk * sketchsize64) words -- for the
 * distinct values D, E = S + 2 and E2 = S3 + 2 the maximum over all positions, then per (k, block) -- and three more:
 * the most two-holder values of a position, their number over all positions, 1 if the per-pair cap was hit; returns the
 * words there are (0: no count pass ran) and fills `out` if `cap` holds them.
 * Neither a count nor an event depends on the order of a k's positions, so the pair stores them sorted by E2, descending,
 * ties by stored position ascending (option "fold2_sort", PPK_FOLD2_SORT, default 1, read at creation; 0 keeps the
 * stored order): the few wide positions share the first blocks of a k and the rest span at most 64 codes, which the
 * tile kernel compares in 6 planes (option "fold2_min_planes", PPK_FOLD2_MIN_PLANES, default 6, read at launch; 7 stops
 * at 7 planes).  ppk_db_fold2_position_order: out[k * 64 * sketchsize64 + i] = the stored position slot i of k holds.
 * ppk_db_fold2_stream_planes: the planes a self job compares per block of SLOTS under the options in force, 8 where the
 * block's largest E2 is above 128, 7 above 64, else 6.  ppk_db_fold2_block_planes stays the 8 / 7 rule on the STORED
 * blocks, and ppk_db_fold2_read returns the planes as they lie, in slot order. */
int ppk_db_fold2_planes(const ppk_db *db);
int ppk_db_fold2_block_planes(const ppk_db *db, uint8_t *out, size_t cap);
int ppk_db_fold2_stream_planes(const ppk_db *db, uint8_t *out, size_t cap);
int ppk_db_fold2_position_order(const ppk_db *db, uint32_t *out, size_t cap);
int ppk_db_fold2_read(const ppk_db *db, int which, uint64_t *out, size_t words);
size_t ppk_db_fold2_events(const ppk_db *db, size_t *n_buckets);
int ppk_db_fold2_events_read(const ppk_db *db, uint32_t *off, size_t n_off, uint16_t *ev, size_t n_ev);
size_t ppk_db_rank_counts(const ppk_db *db, uint32_t *out, size_t cap);
/* The holder pair, built BESIDE the two-holder pair (option "rank_foldh", PPK_RANK_FOLDH, default 1, read at creation; 0
 * never, 2 whenever the caps allow -- tests; 0 at launch leaves a built pair unread): every value with at most H holders
 * at its (k, bin) position is coded 0 on the ref side and 1 on the query side, and only the values with more than H
 * holders keep codes 2 + rank.  The positions of each k are sorted by E_H = (values with more than H holders) + 2,
 * descending, ties by stored position; a block of 64 slots then spans at most 16 codes and the tile kernel compares 4, 3
 * (at most 8 codes) or 2 (at most 4) planes of the 4 the pair stores per block (option "foldh_min_planes", PPK_FOLDH_MIN_PLANES, default 2,
 * read at launch: 3 or 4 keep every block at that many or more).  What a (pair, k) is owed -- its matches on values with
 * 2 .. H holders -- is found once, at creation, by comparing a temporary pair that codes those values alone, and kept as
 * 32-bit entries hi % 256 | (lo % 32) << 8 | k << 13 | count << 16 in the buckets of the two-holder pair's events; the
 * tile kernel adds its tile's entries to the counts before the fit, so every count and every bit is that of the raw
 * planes.  H is the smallest of 4, 8, ... 256 (option "foldh_holders", PPK_FOLDH_HOLDERS, default 0; another value
 * forces that H) whose sorted blocks fit 16 codes and, under the default rule, whose stream plane sum is at most 0.6 of
 * the two-holder pair's on a self job of at least four rounds of tiles; more entries than a sixteenth of the self job's
 * (pair, k) leave the database without the pair ("rank_foldh" 2: more than all of them).  Caps: those of the two-holder
 * pair, fewer than 2^24 samples, at most 1 024 shared values per position.
 * ppk_db_foldh_holders: H, 0 without the pair.  ppk_db_foldh_stream_planes / _position_order / _read: as their fold2_
 * namesakes; ppk_db_foldh_chunk_planes: the planes a stored block holds and _read returns, 4 (the codes are those of an
 * 8-plane coding whose planes 4 .. 7 are zero everywhere and are not kept), 0 without the pair: `words` of _read is
 * nk * sketchsize64 * chunk planes * padded samples.  ppk_db_foldh_entries / _entries_read: as ppk_db_fold2_events /
 * _events_read, 32 bits per entry. */
unsigned ppk_db_foldh_holders(const ppk_db *db);
int ppk_db_foldh_chunk_planes(const ppk_db *db);
int ppk_db_foldh_stream_planes(const ppk_db *db, uint8_t *out, size_t cap);
int ppk_db_foldh_position_order(const ppk_db *db, uint32_t *out, size_t cap);
int ppk_db_foldh_read(const ppk_db *db, int which, uint64_t *out, size_t words);
size_t ppk_db_foldh_entries(const ppk_db *db, size_t *n_buckets);
int ppk_db_foldh_entries_read(const ppk_db *db, uint32_t *off, size_t n_off, uint32_t *ent, size_t n_ent);

/* Number of distance rows for rows q in [q_begin, q_end) (self: n_qry == 0). */
size_t ppk_rows_in_band(size_t n_ref, size_t n_qry, size_t q_begin, size_t q_end);
/* Split the query axis into n_parts bands of (nearly) equal pair count, band
 * edges multiples of 64: bounds[0..n_parts] (the pair-tile split of the N^2
 * space across GPUs). */
int ppk_band_split(size_t n_ref, size_t n_qry, int n_parts, size_t *bounds);

/* ------------------------------------------------------------------------
 * Kernel 1 on resident sketches: match counts at each k -> Jaccard ->
 * random-match correction -> regression of log J on k -> (core, accessory).
 * Replaces the hot loop inside pp_sketchlib.queryDatabase [EXT]
 * (PopPUNK/sketchlib.py:528-537 self, :584-593 ref x query).
 *   qry == NULL        : self comparison of `ref`
 *   kmers              : host int32 [nk] (klist)
 *   random_tbl         : host float [nk][n_clu][n_clu] or NULL
 *   [q_begin, q_end)   : band of query rows to compute (a GPU's share)
 *   d_out              : device; float [rows][2] (core, accessory), or
 *                        float [rows][nk] with PPK_FLAG_JACCARD, or
 *                        uint32 [rows][nk] with PPK_FLAG_COUNTS;
 *                        rows = ppk_rows_in_band(...), band-relative.
 *   d_n_failed         : device uint64 (nullable), incremented by the number
 *                        of pairs with < 2 usable k (they get (0,0)).
 */
int ppk_dist_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                 const float *random_tbl, size_t n_clu, int flags,
                 size_t q_begin, size_t q_end, void *d_out,
                 unsigned long long *d_n_failed, void *stream);

/* Fused kernel 1 + boundary: distances never leave the CU; each wavefront
 * ballots the edge predicate and a compaction pass emits the edge list in
 * reference row order.  Replaces queryDatabase -> (X/scale) ->
 * poppunk_refine.assignThreshold -> generateTuples
 * (PopPUNK/models.py:1065-1091, PopPUNK/network.py:1180-1184) or
 * -> poppunk_refine.edgeThreshold (PopPUNK/refine.py:535), without the
 * [n_pairs,2] matrix.  `inclusive` != 0 selects edgeThreshold's `<= 0`
 * predicate (src/boundary.cpp:88), 0 selects assign == -1 (`< 0`,
 * src/boundary.cpp:70-76 with within_label -1, PopPUNK/models.py:801).
 * Edges are int64 pairs (i,j), i<j; self: sample indices; non-self:
 * (r, n_ref + q) (src/boundary.cpp:113-114).
 *   d_edges / cap      : device int64 [cap][2]
 *   d_n_edges          : device uint64, receives the total edge count of the
 *                        band (may exceed cap; only the first cap are stored)
 */
int ppk_dist_edges_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                       const float *random_tbl, size_t n_clu, int flags,
                       size_t q_begin, size_t q_end, int slope, float x_max,
                       float y_max, float scale_x, float scale_y, int inclusive,
                       long long *d_edges, size_t cap,
                       unsigned long long *d_n_edges,
                       unsigned long long *d_n_failed, void *stream);

/* ppk_dist_edges_dev, and with every edge its distances: what process_weights, a minimum spanning tree or a refine fit
 * read of a fused edge list, without a second pass over the sketches.  d_edges, *d_n_edges, cap and d_n_failed are
 * exactly what ppk_dist_edges_dev gives (same order: reference row order).
 *   d_rows             : device float [cap][2]; row e = the UNSCALED (core, accessory) of edge e, the bits ppk_dist_dev
 *                        writes into that pair's row of the dense result (same databases, k list, random table, flags
 *                        and ext_* options; (0, 0) for a pair with fewer than two usable k).  The scales only enter
 *                        the boundary test.  Calls with the same input give the same bytes.
 *                        When *d_n_edges > cap, d_edges holds the first cap edges and d_rows is UNSPECIFIED: run again
 *                        with the exact size.  NULL: PPK_ERR_ARG.
 * A band of whole tiles of the plain packed kernels (two to four count dwords, not k-split, no wide k window -- a
 * 10 000-genome self job and up) emits the rows from the same pass: 8 bytes of scratch per mask word (one word per
 * query row and 64 refs) and 8 per edge of cap.  Every other shape runs ppk_dist_edges_dev and then the list kernel of
 * ppk_dist_pairs_dev on its edges (one more synchronisation): the same bits.  Option "edge_rows_fused" 0 forces that
 * two-step; ppk_last_kernel_name() tells which ran ("...,rows>" / "... + pairs list"). */
int ppk_dist_edges_rows_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                            const float *random_tbl, size_t n_clu, int flags,
                            size_t q_begin, size_t q_end, int slope, float x_max,
                            float y_max, float scale_x, float scale_y, int inclusive,
                            long long *d_edges, float *d_rows, size_t cap,
                            unsigned long long *d_n_edges,
                            unsigned long long *d_n_failed, void *stream);

/* Kernel 1 for a LIST of pairs: the rows ppk_dist_dev would write for them, without the matrix.  What the reference
 * looks up in its dense matrix -- scripts/poppunk_add_weights.py, process_weights (PopPUNK/network.py:646-674), the
 * subsample a model is fitted on (PopPUNK/models.py:246-254,:520-534) -- is computed here from the resident sketches.
 *   pair p             : (d_i[p*stride], d_j[p*stride]), device int64, stride 1 or 2 (an int64 [m][2] edge list goes
 *                        in unchanged).  Ids are edge ids as in ppk_edge_weights_dev: with a = min - int_offset and
 *                        b = max - int_offset, qry == NULL: samples a < b of `ref`; otherwise ref sample a < n_ref and
 *                        query b - n_ref.  Either orientation, duplicates allowed.
 *   d_out              : row p belongs to pair p: float [n_pairs][2], or float [n_pairs][nk] with PPK_FLAG_JACCARD,
 *                        or uint32 [n_pairs][nk] with PPK_FLAG_COUNTS; the bits ppk_dist_dev writes into that pair's
 *                        row of the dense result (same databases, k list, random table, flags and ext_* options).
 *   d_n_failed         : device uint64 (nullable), incremented once per listed occurrence of a pair with < 2 usable k.
 * The ids are checked on the device before a sketch is read through them: PPK_ERR_ARG, naming the first offending
 * pair, for an id out of range, a == b in a self job, or both ids on one side of a ref x query job; d_out is then
 * untouched.  That check's read-back is the call's one synchronisation; the list is then worked through in chunks
 * (options "pairs_scratch_mb", "pairs_chunk") whose scratch does not grow with the list.  n_pairs == 0 is a no-op. */
int ppk_dist_pairs_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl,
                       size_t n_clu, int flags, const long long *d_i, const long long *d_j, size_t stride,
                       size_t n_pairs, long long int_offset, void *d_out, unsigned long long *d_n_failed,
                       void *stream);
/* Host arrays (i, j int64 [n_pairs]; out as d_out; n_failed nullable, set, not incremented), on the databases'
 * device; blocking. */
int ppk_dist_pairs(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl, size_t n_clu,
                   int flags, const long long *i, const long long *j, size_t n_pairs, long long int_offset, void *out,
                   unsigned long long *n_failed);

/* ------------------------------------------------------------------------
 * N processes, N GPUs of one node, ONE result matrix ("peers write directly at final
 * offsets via ... IPC").  The root rank allocates the [n_pairs][2] matrix with ppk_window_alloc and exports it;
 * every other rank opens the 64-byte handle (sent through any channel: a broadcast, a file) and passes
 * `d_window + (first row of its band) * row bytes` as ppk_dist_dev's d_out: its kernel then stores its rows
 * straight into the root's HBM over its own xGMI link -- no send buffer, no gather, no collective on the data
 * path.  A step is complete on the root once every rank's stream has drained (a barrier).  There is no
 * counterpart in the reference (one process, one device: pp_sketchlib's device_id, PopPUNK/sketchlib.py:536).
 *   ppk_window_alloc : a device allocation of its own, FINE-GRAINED (hipExtMallocWithFlags): peers' stores are
 *                      coherent with the owner's later reads by hardware, not by the timing of a cache flush; not
 *                      from any caching allocator, so that the handle covers exactly it; freed by ppk_window_free
 *                      (not by ppk_release_scratch).  UNVERIFIED ACROSS DEVICES: the window has only ever run with
 *                      both ranks on one GPU (no multi-GPU box was available to the builder)
 *   ppk_window_export: handle of an allocation made by ppk_window_alloc in THIS process
 *   ppk_window_open  : maps another process's allocation for `device` (peer access is enabled by the mapping);
 *                      PPK_ERR_HIP when the two devices cannot reach each other -- the caller then gathers
 *   ppk_window_close : unmaps (the owner's allocation stays)
 */
#define PPK_WINDOW_HANDLE_BYTES 64
int ppk_window_alloc(int device, size_t bytes, void **d_window);
int ppk_window_free(int device, void *d_window);
int ppk_window_export(int device, const void *d_window, unsigned char handle[PPK_WINDOW_HANDLE_BYTES]);
int ppk_window_open(int device, const unsigned char handle[PPK_WINDOW_HANDLE_BYTES], void **d_window);
int ppk_window_close(int device, void *d_window);

/* ------------------------------------------------------------------------
 * Kernel 2 on a resident [n_rows][2] float32 distance buffer.
 */
/* replaces poppunk_refine.assignThreshold (src/python_bindings.cpp:18-25,:79-83;
 * src/boundary.cpp:60-80): out float [n_rows] in {-1, 0, +1} */
int ppk_assign_threshold_dev(const float *d_dist, size_t n_rows, int slope,
                             float x_max, float y_max, float *d_out, void *stream);

/* replaces poppunk_refine.edgeThreshold (src/python_bindings.cpp:27-32,:85-90;
 * src/boundary.cpp:82-95) when n_ref == 0 (self/condensed rows), and the
 * assignThreshold + generateTuples(non-self) pair when n_ref > 0
 * (row = q*n_ref + r -> (r, n_ref+q)).  Stable: edges come out in row order. */
int ppk_edge_threshold_dev(const float *d_dist, size_t n_rows, size_t n_ref,
                           int slope, float x_max, float y_max, int inclusive,
                           long long *d_edges, size_t cap,
                           unsigned long long *d_n_edges, void *stream);

/* replaces poppunk_refine.generateTuples (src/python_bindings.cpp:34-40,:92-96;
 * src/boundary.cpp:97-123): rows with assignments[row] == within_label. */
int ppk_generate_tuples_dev(const int32_t *d_assign, size_t n_rows, int within_label,
                            int self, size_t num_ref, long long int_offset,
                            long long *d_edges, size_t cap,
                            unsigned long long *d_n_edges, void *stream);

/* [OUTSIDE SURVEY 8]  replaces poppunk_refine.generateAllTuples (src/python_bindings.cpp:42-47,:98-101;
 * src/boundary.cpp:125-150; caller PopPUNK/network.py:1087, the dense network): every pair.  self: the
 * condensed rows in order, (i, j) + int_offset; else the reference's loop nest as it stands -- entry
 * j*num_queries + i = (i, j + num_ref) for j < num_ref, i < num_queries, no offset.  The count is known
 * beforehand: *n_edges = n(n-1)/2 or num_ref*num_queries, PPK_ERR_CAPACITY (nothing written) below it. */
int ppk_generate_all_tuples_dev(size_t num_ref, size_t num_queries, int self, long long int_offset,
                                long long *d_edges, size_t cap, size_t *n_edges, void *stream);

/* Distance-QC edge lists: replaces the numpy masks +
 * generateTuples of qcDistMat (PopPUNK/qc.py:332-337 mode 0: core > max_pi or
 * accessory > max_a; qc.py:349-354 mode 1: core == 0 or accessory == 0) on the
 * resident matrix; n_ref == 0 self, else row = q*n_ref + r. */
int ppk_qc_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, int mode, float max_pi,
                     float max_a, long long *d_edges, size_t cap,
                     unsigned long long *d_n_edges, void *stream);

/* ------------------------------------------------------------------------
 * Assignment with a fitted BGMM model (PopPUNK's default --fit-model bgmm; --use-model and poppunk_assign against
 * such a fit).  Replaces BGMMFit.assign -> assign_samples -> log_likelihood / log_multivariate_normal_density
 * (PopPUNK/models.py:411-465, :138-192; PopPUNK/bgmm.py:100-176) and, for the edge lists, the
 * construct_network_from_assignments -> generateTuples that follows it (PopPUNK/__main__.py:643-652,
 * PopPUNK/network.py:1170-1184; poppunk_assign: PopPUNK/assign.py:600, PopPUNK/network.py:1384,:1425-1433).
 * Fitting the mixture (PopPUNK/bgmm.py:20-70) is the section "BGMM fit" below.
 * For a row x = (core, accessory):
 *   xs = x / scale                   in the dtype numpy promotes to (models.py:246-254: PopPUNK's scale is float32,
 *                                    so float32 / float32; a float64 scale gives a float64 quotient)
 *   lpr_c = log w_c - 0.5 (|L_c^-1 (xs - mu_c)|^2 + 2 log 2pi + 2 sum log diag L_c)     in float64
 *   label = argmax_c lpr_c (the first on ties; = argmax of the responsibilities, models.py:181-187)
 *   resp_c = exp(lpr_c - logsumexp(lpr)) as float32 (values=True, models.py:434-437)
 * L_c = chol(cov_c), lower; when cov_c is not positive-definite chol(cov_c + 1e-7 I), and when that fails too the
 * fit is refused (bgmm.py:131-172).
 * A model has 1 <= K <= PPK_BGMM_MAX_K components.  ppk_bgmm is plain data owned by the caller: the device entry
 * points take its values at the call (by kernel argument, or one small copy the library makes on the call's stream),
 * so it may be changed or freed as soon as the call returns. */
#define PPK_BGMM_MAX_K 16
typedef struct ppk_bgmm {
  int K;                          /* components */
  int within_label;               /* the label whose rows are edges (BGMMFit.within_label, models.py:359-375) */
  int scale_is_f64;               /* 0: xs = float32(x / scale_f32), 1: xs = double(x) / scale_f64 */
  int n_jitter;                   /* components that took the 1e-7 fallback (information) */
  float scale_f32[2];
  double scale_f64[2];
  double mean[PPK_BGMM_MAX_K][2];
  double chol[PPK_BGMM_MAX_K][3];      /* L00, L10, L11 of the (possibly jittered) covariance */
  double inv_diag[PPK_BGMM_MAX_K][2];  /* 1 / L00, 1 / L11 */
  double log_const[PPK_BGMM_MAX_K];    /* log w_c - 0.5 (2 log 2pi + 2 sum log diag L_c) */
  /* what the kernels evaluate: z = L_c^-1 (xs - mu_c) as z0 = xs a0 + b0, z1 = ys p + (z0 q + r), i.e.
   * {a0, b0, p, q, r} = {1/L00, -mu0/L00, 1/L11, -L10/L11, -mu1/L11}, and lpr_c = log_const - 0.5 (z0^2 + z1^2),
   * each step one fused multiply-add in double */
  double lin[PPK_BGMM_MAX_K][5];
  int jitter[PPK_BGMM_MAX_K];          /* 1 where the 1e-7 fallback was taken */
} ppk_bgmm;

/* The model as the kernels need it, from the arrays of <prefix>_fit.npz (BGMMFit.load, models.py:359-375): weights
 * double [K], means double [K][2], covariances double [K][2][2], scale double [2] (the stored values; scale_is_f64
 * != 0 when the npz holds them as float64).  Host only, no device is touched.  PPK_ERR_ARG for K outside
 * [1, PPK_BGMM_MAX_K], within_label outside [0, K), a non-positive scale, or a covariance that is not positive-definite
 * even with 1e-7 on its diagonal (the reference's ValueError). */
int ppk_bgmm_prepare(int K, const double *weights, const double *means, const double *covariances,
                     const double *scale, int scale_is_f64, int within_label, ppk_bgmm *out);

/* On a resident [n_rows][2] float32 distance buffer: d_labels int32 [n_rows] (nullable), d_resp float [n_rows][K]
 * (nullable: labels only, no transcendental is evaluated); at least one of the two. */
int ppk_bgmm_assign_dev(const float *d_dist, size_t n_rows, const ppk_bgmm *model, int32_t *d_labels,
                        float *d_resp, void *stream);

/* The rows whose label is model->within_label as an edge list, element for element what ppk_bgmm_assign_dev followed by
 * ppk_generate_tuples_dev(labels, within_label, n_ref == 0, n_ref, int_offset, ...) gives: n_ref == 0 self
 * (condensed rows -> (i, j) + int_offset), else row = q*n_ref + r -> (r + int_offset, n_ref + q + int_offset)
 * (src/boundary.cpp:97-123).  Stable; *d_n_edges the total, only the first cap stored; size rules as
 * ppk_edge_threshold_dev. */
int ppk_bgmm_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, const ppk_bgmm *model,
                       long long int_offset, long long *d_edges, size_t cap,
                       unsigned long long *d_n_edges, void *stream);

/* Fused kernel 1 + BGMM assignment: ppk_dist_edges_dev with the label test in the place of the boundary
 * (queryDatabase -> BGMMFit.assign -> generateTuples without the [n_pairs, 2] matrix).  Arguments and output as
 * ppk_dist_edges_dev; the list equals ppk_dist_dev -> ppk_bgmm_edges_dev on the same band (int_offset 0). */
int ppk_dist_bgmm_edges_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                            const float *random_tbl, size_t n_clu, int flags, size_t q_begin, size_t q_end,
                            const ppk_bgmm *model, long long *d_edges, size_t cap,
                            unsigned long long *d_n_edges, unsigned long long *d_n_failed, void *stream);
/* ... and with every edge its unscaled (core, accessory) row: d_rows and everything about it as in
 * ppk_dist_edges_rows_dev. */
int ppk_dist_bgmm_edges_rows_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                 const float *random_tbl, size_t n_clu, int flags, size_t q_begin, size_t q_end,
                                 const ppk_bgmm *model, long long *d_edges, float *d_rows, size_t cap,
                                 unsigned long long *d_n_edges, unsigned long long *d_n_failed, void *stream);

/* Host form, several devices: ppk_query_edges_dbs with the BGMM label test -- the same band split, pieces (option
 * "chunk_rows"), concatenation in row order and PPK_ERR_CAPACITY -> ppk_parked_fetch hand-over; the list does not
 * depend on the number of devices or pieces. */
int ppk_query_bgmm_edges_dbs(const ppk_db *const *refs, const ppk_db *const *qrys, int n_dev,
                             const int32_t *kmers, const float *random_tbl, size_t n_clu, int flags,
                             const ppk_bgmm *model, long long *ij_out, size_t cap, size_t *n_edges,
                             unsigned long long *n_failed);

/* Host arrays: dist float [n_rows][2] -> labels int32 [n_rows] (nullable) and resp float [n_rows][K] (nullable), on
 * device_id (BGMMFit.assign(X) of the Python mirror; blocking). */
int ppk_bgmm_assign(const float *dist, size_t n_rows, const ppk_bgmm *model, int device_id, int32_t *labels,
                    float *resp);

/* ------------------------------------------------------------------------
 * BGMM fit: PopPUNK's default --fit-model bgmm, BGMMFit.fit -> fit2dMultiGaussian (PopPUNK/models.py:305-338,
 * PopPUNK/bgmm.py:20-45): sklearn's BayesianGaussianMixture(n_components = K, n_init = 5, covariance_type = 'full',
 * weight_concentration_prior = 0.1, mean_precision_prior = 0.1, mean_prior = [0, 0]) with its defaults for the rest
 * (weight_concentration_prior_type = 'dirichlet_process', degrees_of_freedom_prior = 2, reg_covar = 1e-6, tol = 1e-3,
 * max_iter = 100).  What that computes (variational EM, sklearn/mixture/_bayesian_mixture.py and _base.py, 1.7),
 * restated; this restatement is the definition here:
 *   Training rows: xs = float32(x / scale_f32) (the in-place float32 division of ClusterFit.fit, models.py:246-254;
 *   ppk_bgmm's rule for scale_is_f64 == 0), widened to float64.  Everything below is float64 (sklearn itself would run
 *   in float32 on float32 input).  n rows, K components, d = 2, eps = 2^-52.
 *   W0 = np.cov of the training rows (divisor n - 1); m0, beta0, nu0, gamma0 = mean_prior, mean_precision_prior,
 *   degrees_of_freedom_prior, weight_concentration_prior.
 *   Statistics of responsibilities r[i][k]:  nk = sum_i r + 10 eps;  xk = sum_i r x / nk;
 *     sk = sum_i r (x - xk)(x - xk)^T / nk + reg_covar I.
 *   M-step:
 *     M1  a_k = 1 + nk,  b_k = gamma0 + (nk_{K-1} + ... + nk_{k+1}), added from the last component down
 *     M2  beta_k = beta0 + nk,  mean_k = (beta0 m0 + nk xk) / beta_k
 *     M3  nu_k = nu0 + nk,  cov_k = (W0 + nk (sk + beta0 / beta_k (xk - m0)(xk - m0)^T)) / nu_k
 *     M4  L_k = chol(cov_k), lower; not positive-definite: the fit is refused (sklearn's ValueError)
 *     M5  weights_k = a_k / (a_k + b_k) prod_{j<k} b_j / (a_j + b_j), then divided by their sum (stick-breaking)
 *   E-step, per row:  z = L_k^-1 (xs - mean_k),  with psi = digamma
 *     E[log w_k] = psi(a_k) - psi(a_k + b_k) + sum_{j<k} (psi(b_j) - psi(a_j + b_j))
 *     w_k = E[log w_k] - 0.5 (d log 2pi + |z|^2) - sum log diag L_k - 0.5 d log nu_k
 *           + 0.5 (d log 2 + psi(nu_k / 2) + psi((nu_k - 1) / 2) - d / beta_k)
 *     log r_k = w_k - logsumexp_k w_k (max + log sum exp(w - max)),  r_k = exp(log r_k)
 *   Lower bound (sklearn's, without the constant terms), from the NEW parameters and the E-step's log r:
 *     B   c_k = -sum log diag L_k - 0.5 d log nu_k
 *         bound = - sum_ik r log r + sum_k (nu_k c_k + nu_k d/2 log 2 + lgamma(nu_k / 2) + lgamma((nu_k - 1) / 2))
 *                 + sum_k betaln(a_k, b_k) - 0.5 d sum_k log beta_k
 *   Initialisation: the M-step of one-hot responsibilities (labels).  Then per iteration E-step -> M-step -> bound;
 *   stop when |bound - previous bound| < tol (the previous bound of the first iteration is -inf) or after max_iter
 *   iterations; of n_init runs the one with the greatest bound, the first on ties, converged or not.
 *   covariances are cov_k: already divided by the degrees of freedom, as sklearn's covariances_.
 * The labels of a run are given (init_labels: one run), or come from
 *   [EXT] this library's own initialisation, which stands where sklearn draws k-means from numpy's global random
 *   [EXT] state (not reproducible): Lloyd's iterations on the device from K given centres per run -- pass t labels
 *   [EXT] every training row with its nearest centre under (d2, index of centre), d2 = dx dx + dy dy in IEEE double
 *   [EXT] with nothing fused, and moves every centre to the mean of its rows (an emptied centre keeps its place); the
 *   [EXT] iterations stop after the first pass in which no label changed, or after PPK_BGMM_KMEANS_MAX_ITER passes;
 *   [EXT] the labels of the last pass initialise the run.  The centres of run r are drawn by the caller (the Python
 *   [EXT] package: k-means++ with numpy.random.default_rng(seed + r) on a bounded sample, poppunk_amd/bgmm.py).
 * On the device one pass (ppk_bgmm_stats_dev) evaluates the E-step and returns, per component, the seven sums
 *   S r, S r dx, S r dy, S r dx dx, S r dx dy, S r dy dy, S r log r     with (dx, dy) = xs - pivot_k,
 * the pivot being the component's current mean; the host finishes nk = S r + 10 eps, m = S r d / nk, xk = pivot + m,
 * sk = S r d d^T / nk - m m^T (2 - S r / nk) + reg_covar I, which is the centred form above exactly in exact
 * arithmetic (raw moments about 0 would cancel), then M1-M5 and B.  The sums are added in a fixed order (no
 * floating-point atomics, a grid that depends on the row count only): the same rows give the same bits on every call,
 * whether they are a whole matrix or named by an index list inside a larger one. */
#define PPK_BGMM_FIT_STATS 7
#define PPK_BGMM_FIT_MAX_ITER 1024
#define PPK_BGMM_FIT_MAX_INIT 32
#define PPK_BGMM_KMEANS_MAX_ITER 50
typedef struct ppk_bgmm_fit_params {
  int K;                                /* components, 1 .. PPK_BGMM_MAX_K */
  int max_iter;                         /* 0 .. PPK_BGMM_FIT_MAX_ITER; 0 returns the state after initialisation */
  int n_init;                           /* runs when centres are given, 1 .. PPK_BGMM_FIT_MAX_INIT */
  int reserved;
  double weight_concentration_prior;    /* gamma0 */
  double mean_precision_prior;          /* beta0 */
  double mean_prior[2];                 /* m0 */
  double degrees_of_freedom_prior;      /* nu0 > 1 */
  double reg_covar;
  double tol;
} ppk_bgmm_fit_params;
/* fit2dMultiGaussian's values: {K, 100, 5, 0.1, 0.1, (0, 0), 2, 1e-6, 1e-3}. */
int ppk_bgmm_fit_params_default(int K, ppk_bgmm_fit_params *out);

/* The variational state after an M-step, and what the next E-step evaluates from it. */
typedef struct ppk_bgmm_state {
  int K;
  int reserved;
  double weight_conc_a[PPK_BGMM_MAX_K], weight_conc_b[PPK_BGMM_MAX_K];   /* sklearn's weight_concentration_ */
  double mean_precision[PPK_BGMM_MAX_K];
  double means[PPK_BGMM_MAX_K][2];
  double dof[PPK_BGMM_MAX_K];                 /* degrees_of_freedom_ */
  double covariances[PPK_BGMM_MAX_K][4];      /* covariances_, row-major 2 x 2 */
  double chol[PPK_BGMM_MAX_K][3];             /* L00, L10, L11 */
  double weights[PPK_BGMM_MAX_K];
  double lin[PPK_BGMM_MAX_K][5];              /* z = L^-1 (xs - mean) as fused multiply-adds: ppk_bgmm::lin */
  double log_const[PPK_BGMM_MAX_K];           /* w_k + 0.5 |z|^2 */
} ppk_bgmm_state;

typedef struct ppk_bgmm_fit_result {
  ppk_bgmm_state state;                 /* of the best run */
  int n_iter, converged;                /* of the best run */
  int best_init, n_init_run;            /* which run won; how many were made */
  unsigned long long n_train;
  double lower_bound;                   /* -inf when max_iter = 0 */
  double cov_prior[4];                  /* W0 */
  double train_mean[2];
  double init_lower_bound[PPK_BGMM_FIT_MAX_INIT];
  int init_n_iter[PPK_BGMM_FIT_MAX_INIT];
  int kmeans_iter[PPK_BGMM_FIT_MAX_INIT];     /* passes of the own initialisation (0 with given labels) */
  double lower_bounds[PPK_BGMM_FIT_MAX_ITER]; /* the best run's bound after each of its n_iter iterations */
} ppk_bgmm_fit_result;

/* out = {sizeof(ppk_bgmm_fit_params), sizeof(ppk_bgmm_state), sizeof(ppk_bgmm_fit_result)} as this library was built:
 * a binding checks its own layouts against them. */
int ppk_bgmm_fit_struct_sizes(size_t out[3]);

/* digamma(x) for x > 0 (NaN otherwise): the recurrence up to x >= 10, then the asymptotic series.  Host only. */
double ppk_bgmm_digamma(double x);

/* The M-step and the bound from one pass's sums: stats double [K][PPK_BGMM_FIT_STATS] about pivot double [K][2],
 * cov_prior double [4].  lower_bound_out nullable.  Host only, no device is touched.  PPK_ERR_ARG for params outside
 * their ranges, a non-finite sum, or a covariance that lost positive-definiteness (M4). */
int ppk_bgmm_mstep(const ppk_bgmm_fit_params *params, const double *stats, const double *pivot,
                   const double *cov_prior, ppk_bgmm_state *state_out, double *lower_bound_out);

/* One E-step + statistics pass over the training rows of a resident [n_rows][2] float32 matrix: all of them
 * (d_index NULL), or the n_index rows an int64 device list names, in its order (an entry outside [0, n_rows) is a
 * precondition violation: it contributes nothing and nothing is read out of bounds).  scale float [2] (host).
 * d_stats double [K][PPK_BGMM_FIT_STATS] about pivot = state->means.  No synchronisation. */
int ppk_bgmm_stats_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index,
                       const float *scale, const ppk_bgmm_state *state, double *d_stats, void *stream);

/* One pass of the own initialisation: d_labels int32 [n] is read and rewritten with the nearest of centres double
 * [K][2] (host); *d_changed (device) = how many labels changed; d_stats as above with r = the one-hot labels and
 * pivot = centres (new centre = centre + S r d / S r).  No synchronisation. */
int ppk_bgmm_kmeans_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index,
                        const float *scale, int K, const double *centres, int32_t *d_labels, double *d_stats,
                        unsigned *d_changed, void *stream);

/* The fit.  Exactly one of d_init_labels (device int32 per training row: one run) and init_centres (host double
 * [params->n_init][K][2]: the own initialisation, one run per set) is given.  Synchronises the stream once per pass
 * (the sums are needed on the host for the stop test).  PPK_ERR_ARG, the message naming the cause: K outside
 * [1, PPK_BGMM_MAX_K], fewer than 2 training rows or fewer than K, a label outside [0, K), a non-finite row (the first
 * is named), an index outside the matrix, a non-positive scale, a covariance that lost positive-definiteness. */
int ppk_bgmm_fit_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index, const float *scale,
                     const int32_t *d_init_labels, const double *init_centres, const ppk_bgmm_fit_params *params,
                     ppk_bgmm_fit_result *result, void *stream);
/* Host arrays, on device_id; blocking.  The training rows are uploaded in the order of the index list, so the result
 * equals ppk_bgmm_fit_dev's through the same list bit for bit. */
int ppk_bgmm_fit(const float *rows, size_t n_rows, const long long *index, size_t n_index, const float *scale,
                 const int32_t *init_labels, const double *init_centres, const ppk_bgmm_fit_params *params,
                 int device_id, ppk_bgmm_fit_result *result);

/* ------------------------------------------------------------------------
 * DBSCAN: fitting and assigning PopPUNK's --fit-model dbscan (HDBSCAN; DBSCANFit, PopPUNK/models.py:468-783,
 * PopPUNK/dbscan.py:20-66).  The device computes the core distances and the minimum spanning tree of the mutual
 * reachability graph, and assigns rows with a fitted model; the hierarchy between the two (single linkage, condensed
 * tree, excess-of-mass selection) is sequential and lives on the host (poppunk_amd/dbscan.py).
 * Training points P: float32 [n][2], already divided by the model's scale.  m = min_samples and c = min_cluster_size
 * in PopPUNK's (the hdbscan package's) meaning; sklearn's HDBSCAN counts the point itself, so this m is its m + 1.
 *   d2(a, b)    = (double)(ax - bx)^2 + (double)(ay - by)^2: float32 widened, then IEEE double operations, none
 *                 fused.  Everything is ordered on d2; d = sqrt(d2) only where a lambda is formed.
 *   core2[a]    = the m-th smallest d2(a, b) over b != a (duplicates count; m <= n - 1 or PPK_ERR_ARG)
 *   mr2(a, b)   = max(core2[a], core2[b], d2(a, b))
 *   edges are ordered by (mr2, min(a, b), max(a, b)), a total order.  Ties in mr2 are the rule (every neighbour
 *   inside a point's core distance ties exactly) and decide labels, so the order is part of the definition; the
 *   minimum spanning tree is the unique one under it and is emitted sorted by it.
 * Host: union-find over the sorted edges -> single-linkage tree -> condensed tree for c -> stabilities -> excess of
 * mass with allow_single_cluster = False, cluster_selection_epsilon = 0, no max_cluster_size (the rules of
 * sklearn/cluster/_hdbscan/_tree.pyx), lambda = 1 / d and +inf at d = 0.  Labels: -1 noise, clusters numbered in
 * increasing order of their smallest member.  A fit keeps core2, every point's condensed-tree parent and the lambda at
 * which it leaves it, and per condensed cluster (0 is the root) its parent, its birth lambda and its label: the label
 * of the selected cluster at or above it, -1 when there is none.
 * Assignment of a row x = (core, accessory), q = x / scale (float32 / float32; with a float64 scale the float64
 * quotient rounded to float32, the training points' type):
 *   [EXT] the five steps below restate hdbscan/prediction.py (approximate_predict -> _find_neighbor_and_lambda ->
 *   [EXT] _find_cluster_and_probability) from memory; that package is not available to check against.
 *   1. [EXT] order the training points by (d2(q, t), t); N = the first 2m of them (all, if n < 2m)
 *   2. [EXT] r2 = d2 of the (m + 1)-th (0-based position m; the last, if n <= m)
 *   3. [EXT] t* = the first t of N in that order that minimises w2 = max(core2[t], r2, d2(q, t));
 *      [EXT] lambda_q = 1 / sqrt(w2), or DBL_MAX when w2 = 0
 *   4. [EXT] start at t*'s condensed-tree parent; if lambda(t*) > lambda_q, climb while the cluster is not the root
 *      [EXT] and its birth lambda >= lambda_q
 *   5. [EXT] label = that cluster's label (see above: a cluster below a selected one carries the selected one's)
 *   The tie rule of step 1 (by training index) is this library's; a k-d tree's is unspecified.
 * The per-row search goes through a uniform grid over the training points kept in the model; it
 * certifies per row that no point outside the cells it read can precede or tie the 2m nearest, and scans everything
 * otherwise, so the labels are those of the definition whatever the structure (option dbscan_search: 1 = always the
 * plain scan, 2 = the grid at any size). */
/* d_pts float32 [n][2] -> d_core2 double [n]; bit for bit np.partition of the full float64 row. */
int ppk_dbscan_core_dev(const float *d_pts, size_t n, int min_samples, double *d_core2, void *stream);
/* The n - 1 edges (d_a < d_b, d_mr2) of the minimum spanning tree, sorted under the total order.  No
 * synchronisation. */
int ppk_dbscan_mst_dev(const float *d_pts, const double *d_core2, size_t n, int32_t *d_a, int32_t *d_b,
                       double *d_mr2, void *stream);
/* Both from and to host arrays (core2 [n]; a, b, mr2 [n - 1]); blocking. */
int ppk_dbscan_fit(const float *pts, size_t n, int min_samples, int device_id, double *core2, int32_t *a,
                   int32_t *b, double *mr2);

/* A fitted model on device_id: copies of the host arrays above (pts float32 [n][2], core2, pt_cluster, pt_lambda
 * [n]; cl_parent, cl_birth, cl_label [n_cl], cluster 0 the root with parent -1 and every parent before its child),
 * the scale (double [2]; scale_is_f64 as ppk_bgmm_prepare) and the label whose rows are edges.  PPK_ERR_ARG for
 * n outside [1, 2^31), min_samples < 1, a non-positive scale or tree arrays that do not form a rooted tree. */
typedef struct ppk_dbscan ppk_dbscan;
int ppk_dbscan_create(const float *pts, const double *core2, size_t n, int min_samples, const int32_t *pt_cluster,
                      const double *pt_lambda, const int32_t *cl_parent, const double *cl_birth,
                      const int32_t *cl_label, size_t n_cl, const double *scale, int scale_is_f64, int within_label,
                      int device_id, ppk_dbscan **out);
void ppk_dbscan_destroy(ppk_dbscan *model);
/* d_dist float32 [n_rows][2] -> d_labels int32 [n_rows], on the model's device. */
int ppk_dbscan_assign_dev(const float *d_dist, size_t n_rows, const ppk_dbscan *model, int32_t *d_labels,
                          void *stream);
/* ppk_dbscan_assign_dev + ppk_generate_tuples_dev(labels, within_label, n_ref == 0, n_ref, int_offset, ...), element
 * for element, stable, the same cap / PPK_ERR_CAPACITY rules (the shared row-test edge-list path). */
int ppk_dbscan_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, const ppk_dbscan *model,
                         long long int_offset, long long *d_edges, size_t cap, unsigned long long *d_n_edges,
                         void *stream);
/* Rows, since the model was created, whose search ended as a scan of every training point (rows far outside the
 * training cloud; every row with option dbscan_search = 1 is NOT counted: that kernel has no search).  Blocking. */
int ppk_dbscan_stats(const ppk_dbscan *model, unsigned long long *rows_scanned);
/* Host arrays, in chunks of 4 Mi rows; blocking. */
int ppk_dbscan_assign(const float *dist, size_t n_rows, const ppk_dbscan *model, int32_t *labels);

/* ------------------------------------------------------------------------
 * Boundary sweeps of --fit-model refine (SURVEY.md 8f "next" rows), on a
 * resident self/condensed [n_rows][2] float32 distance buffer.  Outputs are
 * three int64 arrays (i, j, offset index), element for element the vectors
 * the reference returns; *d_n_out receives the total (only the first cap
 * entries are stored).  These two entry points synchronise the stream once
 * (the intermediate candidate count sizes a sort).  At most 1023 offsets per call (the
 * reference's callers pass 40 and 20; its loops have no limit).
 */
/* Which form of the sweeps' classify pass a list of boundaries (x_max[o], y_max[o]) takes; no device is touched (the
 * unit test of that choice, tests/test_host_logic.py).  out = {mode (0 / 1: slope 0 / 1, 2: fast slope 2, 3: the
 * reference's line_dist as it stands), early-exit filter, bisection over nested boundaries, guessed end indices (evenly
 * spaced parallel boundaries, the 1-D sweep only: one_d != 0)}. */
int ppk_sweep_plan(const float *x_max, const float *y_max, size_t n_off, int slope, int one_d, int out[4]);
/* The boundaries of a 1-D sweep: (x_max[o], y_max[o]) of offset o along the line (x0, y0) -> (x1, y1), with the
 * float / double mix of src/boundary.cpp:161-186 -- the one statement of them, which ppk_threshold_iterate_1d_dev
 * reads too.  Host arrays of n_off entries (offsets sorted ascending, at most 1023); no device is touched. */
int ppk_sweep_boundaries_1d(const double *offsets, size_t n_off, int slope, float x0, float y0, float x1, float y1,
                            float *x_max, float *y_max);
/* The sweep level of LISTED rows: d_level[p] (device int32 [n_rows]) = the offset index the two sweeps below assign to a
 * row with the coordinates of row p of d_rows (device float [n_rows][2], any list: 4-byte alignment is enough) -- the
 * first of the boundaries (x_max[o], y_max[o]) (HOST arrays, n_off <= 1023) that holds it -- and n_off for a row that
 * none of them lists.  The sweeps' own per-row statement, every boundary evaluated; enqueues only. */
int ppk_sweep_levels_dev(const float *d_rows, size_t n_rows, const float *x_max, const float *y_max, size_t n_off,
                         int slope, int32_t *d_level, void *stream);

/* replaces poppunk_refine.thresholdIterate1D (src/python_bindings.cpp:49-60;
 * src/boundary.cpp:154-210; caller PopPUNK/refine.py:190-200).  `offsets`
 * (host, sorted ascending) are distances along the line (x0,y0)->(x1,y1). */
int ppk_threshold_iterate_1d_dev(const float *d_dist, size_t n_rows, const double *offsets,
                                 size_t n_off, int slope, float x0, float y0, float x1,
                                 float y1, long long *d_i, long long *d_j, long long *d_off,
                                 size_t cap, unsigned long long *d_n_out, void *stream);
/* replaces poppunk_refine.thresholdIterate2D (src/python_bindings.cpp:62-73;
 * src/boundary.cpp:212-237; caller PopPUNK/refine.py:587-593).  `x_max`
 * (host, sorted ascending), fixed y_max, slope 2. */
int ppk_threshold_iterate_2d_dev(const float *d_dist, size_t n_rows, const float *x_max,
                                 size_t n_off, float y_max, long long *d_i, long long *d_j,
                                 long long *d_off, size_t cap, unsigned long long *d_n_out,
                                 void *stream);

/* ------------------------------------------------------------------------
 * Fitting the refine boundary: the network counts of ONE boundary, what refine's local search
 * (scipy's bounded minimiser around newNetwork, PopPUNK/refine.py:221-232,:476-548) asks for per evaluation.
 * d_dist: a resident self/condensed float32 [n_rows][2] matrix, n_rows = n(n-1)/2 >= 1, 8-byte aligned.
 * d_stats: device int64 [4] = {edges, connected components, triangles, connected triples} of the graph over n vertices
 * of every row with line_dist <= 0 (edgeThreshold's rows, inclusive): bit for bit ppk_edge_threshold_dev followed by
 * ppk_network_sweep_dev at one offset.  No edge list is formed.  Integer atomics only: the same input gives the same
 * counts on every call.  Synchronises the stream once (the read-back of the counts: they are written on return). */
int ppk_refine_score_dev(const float *d_dist, size_t n_rows, int slope, float x_max, float y_max, long long *d_stats,
                         void *stream);
/* host arrays: dist float32 [n_rows][2], stats int64 [4]; blocking */
int ppk_refine_score(const float *dist, size_t n_rows, int slope, float x_max, float y_max, int device_id,
                     long long *stats);
/* The same counts for every line between two nested lines, from a handle that does the common work once.
 * create: (x_lo, y_lo) the inner and (x_hi, y_hi) the outer line; x_lo <= x_hi and y_lo <= y_hi (slope 0: only the x
 * pair is read, slope 1: only the y pair; slope 2 also needs x_lo, y_lo >= 2^-40 and finite intercepts).  Otherwise
 * PPK_REFINE_NOT_NESTED (a status of its own, *out = NULL): the caller scores with ppk_refine_score_dev.  One pass
 * sorts the rows into base (edges of every line of the bracket), never (of none) and candidates (kept with their
 * coordinates, in row order); the base graph stays resident in the handle (n^2 / 8 bytes).  The matrix is not read
 * after create returns.  Synchronises the stream (the candidate count sizes the handle).
 * eval: d_stats as ppk_refine_score_dev gives for the same line, all four counts, for every line with
 * x_lo <= x_max <= x_hi and y_lo <= y_max <= y_hi (slope 0: x only, slope 1: y only); PPK_ERR_ARG outside.  Changes
 * nothing in the handle; synchronises the stream once.
 * stats: split[3] = rows that are {base, candidates, never}; host only. */
typedef struct ppk_refine_local ppk_refine_local;
int ppk_refine_local_create_dev(const float *d_dist, size_t n_rows, int slope, float x_lo, float y_lo, float x_hi,
                                float y_hi, void *stream, ppk_refine_local **out);
void ppk_refine_local_destroy(ppk_refine_local *handle);
int ppk_refine_local_stats(const ppk_refine_local *handle, unsigned long long *split);
int ppk_refine_local_eval_dev(const ppk_refine_local *handle, float x_max, float y_max, long long *d_stats,
                              void *stream);

/* ------------------------------------------------------------------------
 * Network scores of the sweeps.  For vertices 0 .. n_vertices-1 and G_t = the graph of every edge
 * whose offset index is <= t, d_stats[t] = {|E(G_t)|, connected components of G_t (isolated vertices included),
 * triangles T, connected triples W = sum_v d_v (d_v - 1) / 2}: the integers networkSummary derives its score from
 * (PopPUNK/network.py:1204-1307 without betweenness: density = E / (0.5 n (n - 1)), transitivity = 3T / W) at every
 * step of refine.growNetwork (PopPUNK/refine.py:375-474), which grows the graph offset by offset.
 *  - edges: d_i[k * stride], d_j[k * stride] (stride 1: separate arrays; 2: an int64 [m][2] edge list, d_j = d_i + 1),
 *    in any order, i > j allowed; d_off[k] their offset indices (NULL: every edge at offset 0, n_off must be 1
 *    unless there are no edges).
 *  - PPK_ERR_ARG, ppk_last_error() naming one offending edge: an id outside [0, n_vertices), a self-loop, an offset
 *    index outside [0, n_off).  Also PPK_ERR_ARG: n_off 0 or > 1023, n_vertices or n_edges >= 2^31.
 *  - an unordered pair given twice is a precondition violation: the counts are then unspecified (nothing is read or
 *    written out of bounds).  No edges: {0, n, 0, 0} for every t.
 *  - labels_at >= 0: d_labels int32 [n_vertices] = the components of G_{labels_at}, numbered in the order of their
 *    smallest vertex (scipy.sparse.csgraph.connected_components; replaces distfile.clusters_from_edges on the device).
 * Synchronises the stream once (the per-offset edge counts size the batches).
 * (Replaces the networkSummary calls of growNetwork: graph-tool's label_components / global_clustering,
 * network.py:1258-1264, or cugraph's, network.py:1236-1249.) */
int ppk_network_sweep_dev(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                          size_t n_edges, size_t n_vertices, size_t n_off, long long labels_at, long long *d_stats,
                          int32_t *d_labels, void *stream);
/* Host arrays: i, j, off int64 [n_edges] (off nullable as above) -> stats int64 [n_off][4], labels int32 [n_vertices]
 * (when labels_at >= 0), on device_id; blocking.  (The same replacement, for callers holding numpy arrays.) */
int ppk_network_sweep(const long long *i, const long long *j, const long long *off, size_t n_edges,
                      size_t n_vertices, size_t n_off, int device_id, long long labels_at, long long *stats,
                      int32_t *labels);

/* ------------------------------------------------------------------------
 * Network summary with betweenness: ppk_network_sweep_dev's edge stream, arguments, validation and
 * error messages, and its d_stats [n_off][4] bit for bit (the same stages), plus for every G_t:
 *  - d_bt double [n_off][2] = {mean, size-weighted mean} over the components of G_t with more than 3 vertices of each
 *    component's maximum normalised vertex betweenness; 0 when there is no such component.
 *  - d_scored int64 [n_off] (nullable) = the number of those components.
 *  - values_at >= 0: d_values double [n_vertices] = every vertex's normalised betweenness in G_{values_at}, within
 *    its own component (0 in components of 3 or fewer vertices).
 * BC(v) = sum over sources s of v's component of delta_s(v) / ((n_c - 1)(n_c - 2)), exact Brandes: networkx's
 * betweenness_centrality(normalized=True) (a star's centre 1, the inner vertices of a 4-vertex path 2/3).  That
 * graph-tool's betweenness(norm=True) gives the same values is UNVERIFIED.  Deterministic: the same input, in any edge
 * order, gives the same bits on every call.  Offsets without edges of their own repeat the row before them.
 * Synchronises the stream once for the counts and once per offset that adds edges (its components size the launch).
 * (Replaces networkSummary(G, calc_betweenness=True), PopPUNK/network.py:1204-1307, graph-tool branch: the
 * label_components / global_clustering calls, :1258-1264, and the per-component vertex_betweenness, :1288-1307,
 * network.py:1309-1312 -- for every step of growNetwork with score_idx > 0, PopPUNK/refine.py:452-457.) */
int ppk_network_summary_dev(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                            size_t n_edges, size_t n_vertices, size_t n_off, long long values_at, long long *d_stats,
                            double *d_bt, long long *d_scored, double *d_values, void *stream);
/* Host arrays: i, j, off int64 [n_edges] (off nullable) -> stats int64 [n_off][4], bt double [n_off][2], scored int64
 * [n_off] (nullable), values double [n_vertices] (when values_at >= 0), on device_id; blocking.  (The same
 * replacement, for callers holding numpy arrays: print_network_summary, network.py:616-643.) */
int ppk_network_summary(const long long *i, const long long *j, const long long *off, size_t n_edges,
                        size_t n_vertices, size_t n_off, int device_id, long long values_at, long long *stats,
                        double *bt, long long *scored, double *values);

/* ------------------------------------------------------------------------
 * Network summary with betweenness from sampled sources: ppk_network_summary_dev's edge stream,
 * arguments, validation, limits and error messages (with this call's name in front), its d_stats bit for bit, and its
 * d_bt / d_scored / d_values computed from at most bt_sources (k >= 1) sources per component.  Per scored component
 * of n_c vertices:
 *  - n_c <= k: every vertex is a source; the values are ppk_network_summary_dev's bit for bit.
 *  - n_c > k: [EXT] the k vertices of smallest (h, v), v the global vertex id and h the high 32 bits of
 *    fmix64(seed + (v + 1) * 0x9E3779B97F4A7C15), fmix64 = splitmix64's finaliser.  The rule is this project's own
 *    (cugraph draws from its own generator); it depends on (seed, ids, component membership) alone: any edge order
 *    and any call give the same sample, and a merged component's sample is a subset of the union of its parts'.
 *    BC(v) = (sum over the sampled s of delta_s(v)) * n_c / (k * ((n_c - 1)(n_c - 2))), evaluated in double as
 *    (S * n_c) / (k * ((n_c - 1) * (n_c - 2))): networkx 3.4.2's _rescale for betweenness_centrality(G, k=k).
 * flags: 0, or PPK_BT_WHOLE_GRAPH: d_values becomes every vertex's betweenness in the whole graph G_{values_at},
 * networkx's betweenness_centrality(G, normalized=True) on a disconnected graph: every component of at least 3
 * vertices is scored and the divisor is (n - 1)(n - 2), n = n_vertices (sampled: S * n_c / (k * ((n - 1)(n - 2))));
 * all 0 when n <= 2.  d_bt and d_scored stay the per-component summary.  That graph-tool normalises the same way is
 * UNVERIFIED.  No float atomics: the same input, in any edge order, gives the same bits on every call.
 * PPK_ERR_ARG for bt_sources == 0 and for unknown flag bits.
 * (Replaces the device branch of networkSummary, betweenness_centrality(k=betweenness_sample, normalized=True) for
 * components of at least betweenness_sample vertices, PopPUNK/network.py:1272-1287; with PPK_BT_WHOLE_GRAPH,
 * vertex_betweenness(G, norm=True), network.py:1310-1313, as poppunk_assign --betweenness calls it, assign.py:646-651.) */
#define PPK_BT_WHOLE_GRAPH 1
int ppk_network_summary_sampled_dev(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                                    size_t n_edges, size_t n_vertices, size_t n_off, long long values_at,
                                    long long *d_stats, double *d_bt, long long *d_scored, double *d_values,
                                    size_t bt_sources, unsigned long long seed, int flags, void *stream);
/* Host arrays, as ppk_network_summary; blocking. */
int ppk_network_summary_sampled(const long long *i, const long long *j, const long long *off, size_t n_edges,
                                size_t n_vertices, size_t n_off, int device_id, long long values_at, long long *stats,
                                double *bt, long long *scored, double *values, size_t bt_sources,
                                unsigned long long seed, int flags);

/* ------------------------------------------------------------------------
 * Cluster numbers: ppk_network_sweep_dev's edge stream, validation, limits and error messages (the
 * entry point's own name in front), and for every G_t:
 *  - d_clusters int32 [n_off][n_vertices]: d_clusters[t][v] = printClusters' number, 1-based, of vertex v in G_t.
 *    Components are taken in the order of their smallest vertex and ranked by len - rankdata(sizes, 'ordinal')
 *    (PopPUNK/network.py:1538-1545, graph-tool branch): by size descending, and among equal sizes by component index
 *    DESCENDING -- among singletons the highest vertex id gets the smallest number.  That graph-tool's
 *    label_components numbers components by their lowest vertex is UNVERIFIED (graph-tool is not installed here).
 *  - d_n_clusters int32 [n_off]: the number of clusters of G_t.
 * An offset without edges of its own repeats the row before it; no edges at all: every row is n_vertices - v.
 * n_off == 1 (d_off NULL) is the one-graph form.  Integer arithmetic only: the same input, in any edge order, gives the
 * same bits on every call.  Synchronises the stream once (the per-offset edge counts size the batches).
 * (Replaces the label_components / rankdata block of printClusters, network.py:1538-1545, for one graph, and for every
 * graph growNetwork(write_clusters=...) prints, PopPUNK/refine.py:458-470, under multi_refine, refine.py:247-330.) */
int ppk_cluster_sweep_dev(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                          size_t n_edges, size_t n_vertices, size_t n_off, int32_t *d_clusters, int32_t *d_n_clusters,
                          void *stream);
/* Host arrays: i, j, off int64 [n_edges] (off nullable) -> clusters int32 [n_off][n_vertices], n_clusters int32
 * [n_off], on device_id; blocking.  (The same replacement, for callers holding numpy arrays.) */
int ppk_cluster_sweep(const long long *i, const long long *j, const long long *off, size_t n_edges, size_t n_vertices,
                      size_t n_off, int device_id, int32_t *clusters, int32_t *n_clusters);

/* Pair sums of a nested family of clusterings, one pass over a resident self/condensed float32
 * [n_rows][2] matrix, n_rows = n(n-1)/2.  d_levels int32 [n_levels][n]: cluster numbers in [1, n]; NESTED (the caller's
 * precondition): two vertices together at level t are together at every later level -- rows of ppk_cluster_sweep_dev's
 * d_clusters are.  For every row (i, j): t* = the first level with d_levels[t][i] == d_levels[t][j] (none: the row adds
 * nothing), c = d_levels[t*][i]; d_sum[t*][c] += llrint((double)d_dist[row][col] * 2^shift), d_cnt[t*][c] += 1.
 * d_sum, d_cnt int64 [n_levels][n + 1] (column 0 unused), zeroed by the call.  The total over the pairs of a cluster at
 * level t is the sum of the buckets of its sub-clusters at levels <= t (poppunk_amd.iterate does that on the host).
 * Integer accumulation: the same bits on every call.  With shift = min(40, 62 - ceil_log2(n_rows)) no sum passes 2^62
 * and a cluster's mean differs from the float64 mean of the same float32 values by at most 2^-(shift + 1).
 * PPK_ERR_ARG, ppk_last_error() naming the first offender: a value that is NaN, infinite or outside [0, 1]; a cluster
 * number outside [1, n].  Also PPK_ERR_ARG: col not 0 or 1, n_rows not n(n-1)/2, shift outside [0, 40] or above
 * 62 - ceil_log2(n_rows), n_levels 0 or > 1023.  Synchronises the stream once (the read-back of the first offender).
 * (Replaces the per-cluster pp_sketchlib.queryDatabase + np.mean of scripts/poppunk_iterate.py:184-197.) */
int ppk_cluster_pair_sums_dev(const float *d_dist, size_t n_rows, int col, const int32_t *d_levels, size_t n_levels,
                              int shift, long long *d_sum, long long *d_cnt, void *stream);
/* Host arrays: dist float32 [n_rows][2], levels int32 [n_levels][n] -> sum, cnt int64 [n_levels][n + 1], on device_id;
 * blocking. */
int ppk_cluster_pair_sums(const float *dist, size_t n_rows, int col, const int32_t *levels, size_t n_levels, int shift,
                          int device_id, long long *sum, long long *cnt);

/* ------------------------------------------------------------------------
 * Silhouette: the silhouette of every sample under every level of a family of clusterings, from a
 * resident self/condensed float32 [n_rows][2] matrix, n_rows = n(n-1)/2, n >= 3.  d_labels int32 [n_levels][n]: cluster
 * numbers in [1, n]; rows of ppk_cluster_sweep_dev's d_clusters qualify.  The numbers may have gaps and the levels need
 * not be nested.
 * Distance of a pair, d(i, j), from its row (x0, x1), by `metric`:
 *     0  core, x0                        1  accessory, x1
 *     2  "euclidean": the float32 sqrtf(x0*x0 + x1*x1), un-fused, the root correctly rounded -- the statement
 *        ppk_edge_weights_dev / ppk_row_norms_dev make for process_weights
 *     3  "difference": the float32 fabsf(x0 - x1).  [EXT], unpinned: what the script's euclidean(distRow[0],
 *        distRow[1]) gave under scipy releases whose euclidean accepted scalars; not recorded.
 * Accumulation: q(i, j) = llrint((double)d(i, j) * 2^shift); T[i][c] = the sum of q(i, j) over j != i with label c;
 * cnt[c] = the samples with label c.  shift = min(40, 61 - ceil_log2(n)) keeps every sum below 2^62 (a distance is at
 * most sqrt 2).  The sums are integers: the same bits on every call and in any order.
 * Per sample i (label ci) and level, in float64, un-fused, exactly these operations:
 *     a = ((double)T[i][ci] * 2^-shift) / (double)(cnt[ci] - 1)
 *     b = the minimum over c != ci with cnt[c] > 0 of ((double)T[i][c] * 2^-shift) / (double)cnt[c]
 *     s = (b - a) / max(a, b);  s = 0 when max(a, b) == 0;  a = b = s = 0 when cnt[ci] == 1
 * (sklearn.metrics.silhouette_samples' rules, its nan_to_num included).  a and b differ from the float64 means of the
 * same float32 distances by at most 2^-(shift + 1) + n * 2^-53 * max d each.
 * Per level t: d_n_labels[t] = its distinct labels; the level is valid iff 2 <= n_labels <= n - 1 (sklearn's
 * check_number_of_labels); an invalid level gets d_valid[t] = 0 and its rows of a, b, s filled with NaN -- not an error,
 * and the other levels are unaffected.  d_a, d_b, d_s double [n_levels][n]; d_a and d_b may be NULL.
 * PPK_ERR_ARG, ppk_last_error() naming the first offender: a distance (either column, whatever the metric) that is NaN,
 * infinite or outside [0, 1]; a label outside [1, n].  Also PPK_ERR_ARG, before any device is touched: metric outside
 * 0 .. 3, shift outside [0, 40] or above 61 - ceil_log2(n), n_levels 0 or > 1023, n_rows not n(n-1)/2, n < 3, a NULL
 * array.  Synchronises the stream once (the read-back of the first offender, before the sums).  The square matrix is
 * never built: samples are taken in bands whose float32 [band][n] rows stay below option "silhouette_scratch_mb".
 * (Replaces the X_mat loop + sklearn.metrics.silhouette_score of scripts/poppunk_calculate_silhouette.py:57-84, for
 * every level of a sweep in one call.) */
int ppk_silhouette_dev(const float *d_dist, size_t n_rows, int metric, const int32_t *d_labels, size_t n_levels,
                       int shift, double *d_a, double *d_b, double *d_s, int32_t *d_n_labels, int32_t *d_valid,
                       void *stream);
/* Host arrays: dist float32 [n_rows][2], labels int32 [n_levels][n] -> a, b (nullable), s double [n_levels][n],
 * n_labels, valid int32 [n_levels], on device_id; blocking. */
int ppk_silhouette(const float *dist, size_t n_rows, int metric, const int32_t *labels, size_t n_levels, int shift,
                   int device_id, double *a, double *b, double *s, int32_t *n_labels, int32_t *valid);

/* ------------------------------------------------------------------------
 * Contingency sums: what the Rand and adjusted Rand indices between two clusterings of the same n
 * samples are made of, for every level of a family A against every level of a family B in one call.  d_a int32
 * [n_a][n], d_b int32 [n_b][n]: cluster numbers in [1, n]; rows of ppk_cluster_sweep_dev's d_clusters qualify.  The
 * numbers may have gaps and the levels need not be nested.  d_b == NULL means B = A (n_b is then taken as n_a, and
 * d_sq_b / d_labels_b may be NULL): every level against every level, each pair computed once.
 *     d_sq_a[x]        long long [n_a]: the sum over the labels of level x of (class size)^2
 *     d_labels_a[x]    int32 [n_a]: the distinct labels of level x          (d_sq_b, d_labels_b: the same of B, [n_b])
 *     d_sq_cells[x][y] long long [n_a][n_b]: the sum over the non-empty cells of the contingency table of n_ij^2
 *     d_n_cells[x][y]  long long [n_a][n_b]: the non-empty cells; level x refines level y iff it equals d_labels_a[x]
 * All of them are integers, exact (every sum is at most n^2 < 2^62), the same bits on every call and for every value
 * of the routing options; nothing on the device is floating point.  poppunk_amd.scores turns them into sklearn's
 * pair_confusion_matrix, rand_score and adjusted_rand_score and the reference script's rand_index_score.
 * PPK_ERR_ARG, before any device is touched: a NULL required array, n == 0, n >= 2^31 - 1, n_a == 0, more than 1 023
 * levels on a side.  PPK_ERR_ARG, ppk_last_error() naming the first offender ("side a, level 2, sample 17: label 0
 * outside [1, 100]"; A's levels come before B's): a label outside [1, n].  Synchronises the stream once (the read-back
 * of the first offender and of every level's label count, before the pair stage).  Scratch: 12 bytes per (level,
 * sample) of state, and the pairs' partial sums in batches, under option "rand_scratch_mb".
 * (Replaces the per-pair sklearn calls of scripts/poppunk_calculate_rand_indices.py:138-141.) */
int ppk_contingency_sums_dev(const int32_t *d_a, size_t n_a, const int32_t *d_b, size_t n_b, size_t n,
                             long long *d_sq_a, long long *d_sq_b, int32_t *d_labels_a, int32_t *d_labels_b,
                             long long *d_sq_cells, long long *d_n_cells, void *stream);
/* Host arrays of the same shapes (b == NULL: B = A; sq_b and labels_b may then be NULL), on device_id; blocking. */
int ppk_contingency_sums(const int32_t *a, size_t n_a, const int32_t *b, size_t n_b, size_t n, int device_id,
                         long long *sq_a, long long *sq_b, int32_t *labels_a, int32_t *labels_b, long long *sq_cells,
                         long long *n_cells);

/* ------------------------------------------------------------------------
 * Lineages within every strain: the neighbour lists and rank prefixes LineageFit builds inside each
 * strain (poppunk_lineages --create-db, PopPUNK/lineages.py:156-326), for all strains in one call each, from the
 * resident self/condensed float32 [n(n-1)/2][2] matrix.
 * Strains: d_members int64 [m] (device), the strains' member lists back to back -- global sample ids, each list in the
 * strain's LOCAL order, which is the caller's (it need not ascend, and strains may interleave in id space); seg_off
 * int64 [n_strains + 1], a HOST array: strain s is d_members[seg_off[s] .. seg_off[s + 1]), n_s members.  A sample in
 * no strain does not appear.  PPK_ERR_ARG before any device is touched: a NULL array, seg_off[0] != 0, a strain of
 * fewer than 2 members ("strain 3 has 1 members: a strain needs at least 2").  PPK_ERR_ARG, ppk_last_error() naming the
 * first offender by position: an id outside [0, n) ("strain 1, member 4: sample 700 outside [0, 700)"), an id that an
 * earlier position holds ("strain 2, member 0: sample 17 is already member 5 of strain 0").
 *
 * ppk_strain_knn_dev: for every member, its d_s = min(depth, n_s - 1) nearest members of its own strain in
 * get_kNN_distances' order (src/extend.cpp:248-289): ascending distance (column dist_col), ties by local column, the
 * member itself skipped; -0.0 ties with and is returned as 0.0.  d_i, d_j int64, d_out float32 [nnz], nnz = the sum of
 * n_s * d_s: strain by strain, local row by local row, (local row, local column, distance).  Row r of strain s is bit
 * for bit what ppk_knn_dev gives on the square of that strain's pruned matrix.  No limit on depth or n_s but memory
 * (and fewer than 2^31 members per strain).  Synchronises the stream once: the check of the member lists, before
 * anything is indexed by them (nnz itself is known to the caller beforehand).  Routes: the header of ppk_lineage.hip.
 * [get_kNN_distances is C++ that cannot be compiled in this tree (Eigen is missing): parity with it is unpinned, as
 * for ppk_knn_dev, with which this call agrees bit for bit -- OUTSIDE SURVEY 8 stays as marked below.]
 *
 * ppk_strain_ranks_dev: lowerRank's rule (src/extend.cpp:128-246, as ppk_lower_rank states it: kNN + 1 entries without
 * count_unique_distances, `prev` starting at 0.0, steps of at least epsilon in float32) applied to the sorted lists
 * d_j / d_dist of ppk_strain_knn_dev (same seg_off and depth; distances unfloored), for every rank of `ranks` (HOST
 * int32 [n_ranks], at least 1, ascending, n_ranks <= 1 023) at once.  On a sorted row the rule keeps a prefix:
 *     d_prefix int32 [n_ranks][m]: d_prefix[q][g] = the entries of the row of position g that rank q keeps
 * and the family is nested in the rank.  The level stream, *n_out entries in the order (position, place in the row):
 * (d_pos_i, d_pos_j, d_level) int64, positions into d_members, level = a rank index; d_level_dist (nullable) float32,
 * the entry's distance.  Every unordered pair appears at most once:
 *     reciprocal_only == 0: a pair kept in either direction, at the lowest rank index at which either is kept; from the
 *         lower row (i < j) where both directions are kept under the last rank, else as the one direction has it
 *     reciprocal_only != 0: i < j, both directions kept, at the later of the two levels -- the entries of level <= q,
 *         in stream order, are lowerRank's reciprocal output for rank q
 * so (d_pos_i, d_pos_j, d_level) is an edge stream for ppk_cluster_sweep_dev with n_vertices = m, n_off = n_ranks.
 * Positions keep local order inside a segment, so a strain's printClusters number of a member is the dense rank of its
 * number among the numbers of its segment.  PPK_ERR_CAPACITY with *n_out set when the stream exceeds cap (worst case
 * nnz).  PPK_ERR_ARG naming the first row with a column outside its strain or equal to the row.  Compare and integer arithmetic only: the
 * same bits on every call.  Synchronises the stream once (the stream's length, before it is written). */
int ppk_strain_knn_dev(const float *d_dist, size_t n, int dist_col, const long long *d_members,
                       const long long *seg_off, size_t n_strains, size_t depth, long long *d_i, long long *d_j,
                       float *d_out, void *stream);
int ppk_strain_ranks_dev(const long long *d_j, const float *d_dist, const long long *seg_off, size_t n_strains,
                         size_t depth, const int32_t *ranks, size_t n_ranks, int reciprocal_only,
                         int count_unique_distances, float epsilon, int32_t *d_prefix, long long *d_pos_i,
                         long long *d_pos_j, long long *d_level, float *d_level_dist, size_t cap, size_t *n_out,
                         void *stream);
/* Host arrays of the same shapes (dist float32 [n(n-1)/2][2], members int64 [m]), on device_id; blocking. */
int ppk_strain_knn(const float *dist, size_t n, int dist_col, const long long *members, const long long *seg_off,
                   size_t n_strains, size_t depth, int device_id, long long *i_out, long long *j_out, float *d_out);
int ppk_strain_ranks(const long long *j, const float *dist, const long long *seg_off, size_t n_strains, size_t depth,
                     const int32_t *ranks, size_t n_ranks, int reciprocal_only, int count_unique_distances,
                     float epsilon, int device_id, int32_t *prefix, long long *pos_i, long long *pos_j,
                     long long *level, float *level_dist, size_t cap, size_t *n_out);

/* ppk_strain_extend_dev: poppunk_refine.extend (src/extend.cpp:52-126, as ppk_extend states it) inside
 * every strain at once -- a query batch added to the stored neighbour lists of the strains it was assigned to
 * (poppunk_lineages --query-db, PopPUNK/lineages.py:329-466; LineageFit.extend, PopPUNK/models.py:1337-1389).
 * References: d_members / seg_off as above, ids in [0, n_ref).  Queries: d_queries int64 [mq] (device) with qry_off
 * int64 [n_strains + 1] (HOST): ids in [0, n_qry), strain by strain in the caller's order; a strain may have none; ids
 * need not ascend.  Stored lists d_nn_j int64 / d_nn_d float32: the layout ppk_strain_knn_dev writes for (seg_off,
 * depth), local columns, every row non-decreasing in distance.  d_qr float32 [n_qry * n_ref][2], row q * n_ref + r
 * (query-major); d_qq float32 [n_qry(n_qry-1)/2][2], the long form over all queries (NULL allowed when no strain has two
 * queries; d_queries and d_qr NULL allowed when there is no query at all).  Values read from d_qr and d_qq below
 * `floor` become `floor`; stored values are taken as they are.
 * Output: strain s has n'_s = n_s + q_s local rows, the members in member order then its queries in list order, each
 * with min(depth, n'_s - 1) entries (local row, local column, distance): the layout of ppk_strain_knn_dev for the
 * segment sizes n'_s, so what ppk_strain_ranks_dev takes with those segments.  A row is the merge of the query side
 * (the strain's queries in list order, stably sorted by distance) and the stored side (a member's stored row as stored;
 * for a query the members in member order, stably sorted), the query side first on a tie, the sample itself skipped by
 * index, the first `depth` kept; -0.0 ties with and is returned as 0.0.  Row for row it is bit for bit what ppk_extend
 * returns for that strain alone with knn = depth.  A strain without queries comes back as its stored lists.
 * PPK_ERR_ARG before any device is touched for the segment errors above, qry_off[0] != 0 or descending, a strain of two
 * queries with d_qq NULL.  PPK_ERR_ARG naming the first offender -- the members first, then the queries, then the
 * stored lists: "strain 1, member 4: sample 700 outside [0, 700)", "strain 2, query 0: query 17 is already query 1 of
 * strain 0", "strain 3, row 2, entry 5: column 9 outside [0, 9)" / "column 2 is the row itself" / "the distance is below
 * the entry before it".  Synchronises the stream once, for these checks, before anything is indexed through the lists.
 * Routes and options as ppk_strain_knn_dev, by the n'_s - 1 candidates of a row.  [parity with src/extend.cpp unpinned,
 * as for ppk_extend: OUTSIDE SURVEY 8 stays as marked below.] */
int ppk_strain_extend_dev(const long long *d_members, const long long *seg_off, const long long *d_queries,
                          const long long *qry_off, size_t n_strains, const long long *d_nn_j, const float *d_nn_d,
                          const float *d_qr, const float *d_qq, size_t n_ref, size_t n_qry, int dist_col, float floor,
                          size_t depth, long long *d_i, long long *d_j, float *d_out, void *stream);
/* Host arrays of the same shapes, on device_id; blocking. */
int ppk_strain_extend(const long long *members, const long long *seg_off, const long long *queries,
                      const long long *qry_off, size_t n_strains, const long long *nn_j, const float *nn_d,
                      const float *qr, const float *qq, size_t n_ref, size_t n_qry, int dist_col, float floor,
                      size_t depth, int device_id, long long *i_out, long long *j_out, float *d_out);

/* ------------------------------------------------------------------------
 * Density grids of a resident float32 [n_rows][2] matrix: the two layers of the fit plots, each one
 * streaming pass with integer accumulation -- the same bits on every call and for any row order.  The matrix need not
 * be condensed (a ref x query matrix works).
 *
 * ppk_density_kde_dev: the Epanechnikov sums on the nodes (gx[a], gy[b]).  Rows read: d_idx[0 .. n_idx) (int64, any
 * order, repeats allowed) or, d_idx NULL, every row.  gx [nx], gy [ny]: HOST doubles, strictly ascending (the call
 * places them in its scratch); scale: two HOST floats, or NULL for the column maxima of the rows read, taken on the
 * device as float32 (np.amax(X, axis = 0)); scale_used (nullable): the two floats the call divided by.  For every row
 * read (x, y):  xs = x / scale[0], ys = y / scale[1] (IEEE float32 divisions: the reference's `X /= scale` on a float32
 * array), px = (double)xs, py = (double)ys, and for every cell (a, b)
 *     dx = px - gx[a], dy = py - gy[b], d2 = dx*dx + dy*dy (two products, one add, un-fused),
 *     t = 1.0 - d2 * inv_h2 with inv_h2 = 1.0 / (h*h) computed once on the host,
 *     t > 0:  d_sum[a][b] += llrint(t * 2^shift).
 * d_sum int64 [nx][ny], zeroed by the call.  sklearn's density is d_sum * 2^-shift * 2 / (pi h^2 N).  A row visits
 * only the cells inside [px - hw, px + hw] x [py - hw, py + hw], hw = h (1 + 2^-20): a superset of the cells with
 * t > 0 for any h and any spacing.  nx * ny + nx + ny <= PPK_DENSITY_KDE_MAX_CELLS: a workgroup keeps the grid and its
 * coordinates in LDS, 8 bytes each, two workgroups to a CU (100 x 100 takes 10 200); the error message states the limit.
 * PPK_ERR_ARG, ppk_last_error() naming the first offender in the order the rows are read (the position in d_idx, or
 * the row), whichever kind it is: an index outside [0, n_rows); a non-finite value in a row read.  Also PPK_ERR_ARG: scale or h not finite or not positive (h*h and 1/(h*h) must be finite and positive too), a
 * grid not finite or not strictly ascending, nx * ny zero or the grid above the limit, shift outside [0, 40] or above
 * 62 - ceil_log2(rows read), a NULL array.  Synchronises the stream once (the offenders and the scale).
 * (Replaces KernelDensity(bandwidth, kernel='epanechnikov').fit(X) and score_samples(xy) of plot_scatter,
 * PopPUNK/plot.py:62-66, and with d_idx the sklearn.utils.shuffle copy of :50-51.) */
#define PPK_DENSITY_KDE_MAX_CELLS 10240
int ppk_density_kde_dev(const float *d_dist, size_t n_rows, const long long *d_idx, size_t n_idx, const float *scale,
                        const double *gx, size_t nx, const double *gy, size_t ny, double h, int shift,
                        long long *d_sum, float *scale_used, void *stream);
/* Host arrays: dist float32 [n_rows][2], idx int64 [n_idx] (nullable) -> sum int64 [nx][ny], on device_id; blocking. */
int ppk_density_kde(const float *dist, size_t n_rows, const long long *idx, size_t n_idx, const float *scale,
                    const double *gx, size_t nx, const double *gy, size_t ny, double h, int shift, int device_id,
                    long long *sum, float *scale_used);

/* ppk_density_counts_dev: which pixels of a uniform raster hold a row, per label -- the scatter layer.  For every row
 * (x, y): ix = floor(((double)x - x0) * inv_dx), iy = floor(((double)y - y0) * inv_dy); ix outside [0, nx) or iy
 * outside [0, ny): *d_outside += 1 and nothing else; otherwise d_counts[slot][iy][ix] += 1 with slot = d_label[row] -
 * label_lo (d_label NULL: slot 0, and n_slots must be 1).  d_label int32 [n_rows]: what ppk_bgmm_assign_dev and
 * ppk_dbscan_assign_dev write.  d_counts uint32 [n_slots][ny][nx] and d_outside int64 [1], zeroed by the call.
 * Limits: n_rows < 2^32, 1 <= n_slots <= 32, 1 <= nx, ny <= 4096, n_slots * nx * ny <= 2^26.
 * PPK_ERR_ARG, ppk_last_error() naming the first row at fault: a non-finite value; a label outside [label_lo,
 * label_lo + n_slots).  Also PPK_ERR_ARG: x0 / y0 not finite, inv_dx / inv_dy not finite or not positive, a limit
 * passed, a NULL array.  Synchronises the stream once.
 * (Replaces the one-marker-per-row plt.scatter / plt.plot calls of plot_results, plot_dbscan_results and
 * plot_refined_results, PopPUNK/plot.py:221, :275, :330-331, for matrices too large to draw row by row.) */
int ppk_density_counts_dev(const float *d_dist, size_t n_rows, const int32_t *d_label, int label_lo, int n_slots,
                           double x0, double inv_dx, size_t nx, double y0, double inv_dy, size_t ny,
                           uint32_t *d_counts, long long *d_outside, void *stream);
/* Host arrays: dist float32 [n_rows][2], label int32 [n_rows] (nullable) -> counts uint32 [n_slots][ny][nx], outside
 * int64 [1], on device_id; blocking. */
int ppk_density_counts(const float *dist, size_t n_rows, const int32_t *label, int label_lo, int n_slots, double x0,
                       double inv_dx, size_t nx, double y0, double inv_dy, size_t ny, int device_id,
                       uint32_t *counts, long long *outside);

/* ------------------------------------------------------------------------
 * Queries against an existing clustering.  Vertices 0 .. n_ref-1 are references, n_ref .. n_ref+n_qry-1
 * queries: the ids ppk_dist_edges_dev, ppk_*_edges_dev and ppk_generate_tuples_dev emit for a query-vs-reference job.
 * The edge stream is d_i[k * stride], d_j[k * stride] (stride 1 or 2), either orientation, any order.  d_ref_label int32
 * [n_ref]: two references with equal labels are in one component of the loaded network; any values in [0, n_ref), not
 * necessarily dense or ordered.  For assignment the reference network matters only through these labels, so neither
 * call reads its edges.  Integer arithmetic only: the same input, in any edge order, gives the same bits on every call.
 * PPK_ERR_ARG, ppk_last_error() naming the first offender, nothing further launched: a label outside [0, n_ref), a
 * vertex id outside [0, n_ref + n_qry), a self-loop.  Also PPK_ERR_ARG: max_links outside 1 .. 64, n_ref + n_qry >=
 * 2^31, n_edges >= 2^31, stride not 1 or 2, a NULL array.
 *
 * ppk_query_links_dev: per query q (vertex n_ref + q), over its query-reference edges (edges with both ends on one
 * side are skipped, so the stream ppk_cluster_extend_dev takes can be passed as it is):
 *  - d_degree int32 [n_qry]: the number of those edges (a repeated edge counts every time);
 *  - d_n_links int32 [n_qry]: the exact number of distinct labels among the references it is linked to;
 *  - d_links int32 [n_qry][max_links]: the max_links smallest of those labels, ascending, padded with -1.
 * A stream whose query-reference edges are non-decreasing in the query (every producer's row order; skipped edges
 * after them, or none) is not sorted: one wave per query keeps the distinct labels of its segment in an LDS set of
 * PPK_ASSIGN_SET_CAP entries.  A query with more distinct labels than that goes onto an overflow list, whose (query,
 * label) keys are radix-sorted and made unique; any other stream takes that sort route for every query.
 * Synchronises the stream once (the first offender and whether the stream is ordered), and once more on the ordered
 * route for the length of the overflow list.
 * (Replaces the per-query set walk of qcQueryAssignments, PopPUNK/qc.py:372-417, and, with `serial`, the per-query
 * graph copy + label_components of assign_query_hdf5, PopPUNK/assign.py:696-722.) */
#define PPK_ASSIGN_SET_CAP 128
int ppk_query_links_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges,
                        const int32_t *d_ref_label, size_t n_ref, size_t n_qry, int max_links, int32_t *d_degree,
                        int32_t *d_n_links, int32_t *d_links, void *stream);
/* Host arrays: i, j int64 [n_edges], ref_label int32 [n_ref] -> degree, n_links int32 [n_qry], links int32
 * [n_qry][max_links], on device_id; blocking. */
int ppk_query_links(const long long *i, const long long *j, size_t n_edges, const int32_t *ref_label, size_t n_ref,
                    size_t n_qry, int max_links, int device_id, int32_t *degree, int32_t *n_links, int32_t *links);

/* ppk_cluster_extend_dev: printClusters' number (ppk_cluster_sweep_dev's d_clusters, one graph) of each of the n_ref +
 * n_qry vertices of (the loaded network + these edges): bit for bit what ppk_cluster_sweep_dev gives on the explicit
 * union of the reference network's edges and the stream, provided d_ref_label holds that network's components.
 * d_numbers int32 [n_ref + n_qry], d_n_clusters int32 [1].  The union-find is seeded from the labels (every reference
 * under the smallest reference of its label, every query its own root), one union launch runs over the stream
 * (query-query and reference-reference edges included), and the ranking is the cluster sweep's: O(n + n_edges) work
 * whatever the reference network's edge count.  Synchronises the stream once.
 * (Replaces addQueryToNetwork's edge insertion into the loaded graph, PopPUNK/network.py:1315-1442, followed by
 * printClusters' label_components / rankdata block, network.py:1538-1545, in assign_query_hdf5, PopPUNK/assign.py:
 * 628-660.) */
int ppk_cluster_extend_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges,
                           const int32_t *d_ref_label, size_t n_ref, size_t n_qry, int32_t *d_numbers,
                           int32_t *d_n_clusters, void *stream);
/* Host arrays: i, j int64 [n_edges], ref_label int32 [n_ref] -> numbers int32 [n_ref + n_qry], n_clusters int32 [1],
 * on device_id; blocking. */
int ppk_cluster_extend(const long long *i, const long long *j, size_t n_edges, const int32_t *ref_label, size_t n_ref,
                       size_t n_qry, int device_id, int32_t *numbers, int32_t *n_clusters);

/* ------------------------------------------------------------------------
 * Reference genomes of a cluster network ([EXT]): extractReferences, PopPUNK/network.py:283-487, as a
 * deterministic rule (graph-tool's clique order and list(frozenset)[0] are implementation-defined).  Edges
 * d_i[k * stride], d_j[k * stride] (stride 1 or 2 as above) over vertices 0 .. n_vertices-1: every unordered pair once
 * or several times, either orientation, no self-loop.  d_existing, d_merged uint8 [n_vertices] flags (non-zero = set),
 * either may be NULL.
 *  1. components of G;
 *  2. fast == 0, per component V: |V| <= 2, its lowest vertex becomes a reference unconditionally; else R = V and,
 *     while R is non-empty: s = min R, K = {s}, C = N(s) & R; while C is non-empty: v = min C, K += v, C &= N(v); if K
 *     holds no reference (existing or picked), s becomes one; R -= K;
 *  3. fast == 1 instead: a component without an existing reference gets its |V| / 10 + 1 lowest vertices, and a
 *     component with m > 0 merged queries the m / 3 + 1 lowest of them;
 *  4. repair: in a component whose references fall into more than one component of G[references], a breadth-first
 *     search of G from r0, its lowest reference (a vertex's parent: its lowest neighbour in the level before); every
 *     vertex on the parent path of every reference outside r0's component of G[references] becomes a reference.
 * Outputs: d_is_ref uint8 [n_vertices] (0 / 1); d_ref_edges int64 [n_edges][2] (NULL to skip): the edges with both ends
 * references, in stream order and orientation, renumbered by rank among the references (the first counts[1] rows are
 * written); d_counts int64 [8]: references, reference edges, components, cliques removed, references from cliques
 * (fast: from rule 3's first half), references from components of one or two vertices (fast: from merged queries),
 * references added by the repair, components repaired -- counts 4 .. 6 count vertices NEWLY flagged, so
 * counts[0] = existing + counts[4] + counts[5] + counts[6].  Integer arithmetic; the same edges in any order give the
 * same bits.  PPK_ERR_ARG names the first offending edge; PPK_ERR_CAPACITY: option "refs_scratch_mb".  Synchronises
 * the stream once. */
int ppk_pick_refs_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges, size_t n_vertices,
                      const uint8_t *d_existing, const uint8_t *d_merged, int fast, uint8_t *d_is_ref,
                      long long *d_ref_edges, long long *d_counts, void *stream);
/* Host arrays: i, j int64 [n_edges], existing / merged uint8 [n_vertices] or NULL -> is_ref uint8 [n_vertices],
 * ref_edges int64 [n_edges][2] (nullable; counts[1] rows written), counts int64 [8], on device_id; blocking. */
int ppk_pick_refs(const long long *i, const long long *j, size_t n_edges, size_t n_vertices, const uint8_t *existing,
                  const uint8_t *merged, int fast, int device_id, uint8_t *is_ref, long long *ref_edges,
                  long long *counts);

/* ------------------------------------------------------------------------
 * Minimum spanning forests.  Edges d_i[k * stride], d_j[k * stride] (stride 1: separate arrays; 2:
 * an int64 [m][2] edge list, d_j = d_i + 1), weights d_w[k], over vertices 0 .. n_vertices-1; i > j, parallel edges and
 * both orientations of a pair allowed.  Edges are totally ordered by (w, min(i, j), max(i, j), k), -0.0 read as +0.0;
 * under that order the minimum spanning forest is unique (Kruskal with a stable sort on the key), and it is what this
 * returns:
 *  - d_tree int64 [min(n_edges, n_vertices - 1)]: the input indices k of the forest's edges, ascending;
 *    *d_n_tree = how many (n_vertices - components).
 *  - d_labels int32 [n_vertices] (nullable): components numbered in the order of their smallest vertex
 *    (scipy.sparse.csgraph.connected_components; ppk_network_sweep_dev's labels_at).
 * Deterministic: the same input gives the same bits on every call; a permuted input gives the same (min, max, w) set.
 * PPK_ERR_ARG, ppk_last_error() naming one offending edge: an id outside [0, n_vertices), a self-loop, a NaN or
 * infinite weight.  Also PPK_ERR_ARG: n_vertices or n_edges >= 2^31.  No edges: *d_n_tree = 0 and every vertex its own
 * component.  Synchronises the stream once (the validation's read-back); none between the Boruvka rounds.
 * (Replaces gt.min_spanning_tree in generate_minimum_spanning_tree, PopPUNK/network.py:1747-1750, or cugraph's
 * minimum_spanning_tree, network.py:2146 and PopPUNK/sparse_mst.py:111.) */
int ppk_mst_dev(const long long *d_i, const long long *d_j, size_t stride, const float *d_w, size_t n_edges,
                size_t n_vertices, long long *d_tree, unsigned long long *d_n_tree, int32_t *d_labels, void *stream);
/* Host arrays: i, j int64 [n_edges], w float32 [n_edges] -> tree int64 [min(n_edges, n_vertices - 1)], *n_tree, labels
 * int32 [n_vertices] (nullable), on device_id; blocking. */
int ppk_mst(const long long *i, const long long *j, const float *w, size_t n_edges, size_t n_vertices, int device_id,
            long long *tree, unsigned long long *n_tree, int32_t *labels);
/* process_weights (PopPUNK/network.py:646-674) of a model edge list: d_w[k] = column 0 (weights_type 0, core), column 1
 * (1, accessory) or the float32 sqrtf(x0*x0 + x1*x1), un-fused (2, euclidean: np.linalg.norm(x, axis=1)) of the row of
 * d_dist float32 [n_rows][2] that edge k = (i, j) came from.  With a = min(i, j) - int_offset, b = max(i, j) - int_offset:
 * n_ref == 0 (self): the condensed row of (a, b); otherwise row = (b - n_ref) * n_ref + a, the inverse of
 * generate_tuples' non-self mapping.  PPK_ERR_ARG naming the edge: an edge with no row in the matrix; also a row count
 * that is not n(n-1)/2 (self) or a multiple of n_ref.  Synchronises the stream once (the check's read-back).
 * (Replaces process_weights(distMat[assignments == within_label], weights_type) of generate_network_from_distances,
 * network.py:2108-2117.) */
int ppk_edge_weights_dev(const float *d_dist, size_t n_rows, const long long *d_i, const long long *d_j, size_t stride,
                         size_t n_edges, size_t n_ref, long long int_offset, int weights_type, float *d_w, void *stream);
/* The "euclidean" weights of rows that are the edges' own already (ppk_dist_pairs_dev of the edge list): d_w[k] = the
 * same un-fused float32 statement on row k of d_rows float32 [n_rows][2].  Enqueues only. */
int ppk_row_norms_dev(const float *d_rows, size_t n_rows, float *d_w, void *stream);

/* ------------------------------------------------------------------------
 * Neighbour-joining trees.  Exact neighbour joining of n samples' core distances, with the join and
 * tie rule of Biopython's DistanceTreeConstructor.nj.  Only the strictly lower triangle D[a][b], a > b, is read, the
 * diagonal taken as 0: src_kind PPK_NJ_SQUARE, d_src float32 [n][n] row-major (stride, col ignored); PPK_NJ_LONG, the
 * condensed upper triangle read at d_src[e * stride + col] as ppk_long_to_square_dev reads it.  Working values are
 * float64, un-fused.  r active nodes sit in slots in sample order; while r > 2, with nd[x] = S[x] / (r - 2):
 *  - join the active pair a > b of least Q = (D[a,b] - nd[a]) - nd[b]; of equal Q (-0.0 == +0.0) the least a, then b;
 *  - len_a = ((D[a,b] + nd[a]) - nd[b]) / 2, len_b = D[a,b] - len_a;
 *  - slot b becomes the new node, D'[b,k] = ((D[a,k] + D[b,k]) - D[a,b]) / 2; slot a is removed;
 *  - row sums (this library's rule, not Biopython's recomputation): S'[k] = ((S[k] - D[a,k]) - D[b,k]) + D'[b,k],
 *    S'[b] = ((S[a] + S[b]) - r * D[a,b]) / 2; initially S[k] = sum of D[k][j], j = 0 .. n-1 ascending, from +0.0.
 * Output, n >= 2: d_join int64 [n-1][2], d_len float64 [n-1][2].  Row t < n-2: join t's node ids (a, b) -- sample ids
 * 0 .. n-1, or n + t' for the node join t' made -- and (len_a, len_b).  Row n-2: the final edge, the ids of the two
 * nodes left (slot 1, slot 0) and its length D[1,0] in both length columns.  n = 1 writes nothing.
 * Deterministic: the same input gives the same bits on every call.  PPK_ERR_ARG, ppk_last_error() naming the entry: a
 * NaN or infinite lower-triangle entry; also n = 0 or n >= 2^31.  Synchronises the stream once (the check's read-back);
 * none between joins.  PPK_ERR_INTERRUPTED when the interrupt check asks (polled every 256 joins).
 * (Replaces DistanceTreeConstructor().nj(pdm) in generate_nj_tree, PopPUNK/trees.py:186-189, and its rapidnj branch.) */
#define PPK_NJ_SQUARE 0
#define PPK_NJ_LONG 1
int ppk_nj_dev(const float *d_src, int src_kind, size_t stride, size_t col, size_t n, long long *d_join, double *d_len,
               void *stream);
/* Host arrays: square float32 [n][n] -> join int64 [n-1][2], len float64 [n-1][2], on device_id; blocking. */
int ppk_nj(const float *square, size_t n, int device_id, long long *join, double *len);

/* ------------------------------------------------------------------------
 * Stochastic cluster embeddings: 2-D coordinates of n samples from their k nearest neighbours, the
 * loop of mandrake's SCE as this library defines it.  Input: neighbour lists in get_kNN_distances form, d_i, d_j int64
 * [n*k], d_dist float32 [n*k]: entry e of row i = e / k, 2 <= n < 2^31, 1 <= k <= n - 1 (callers clamp k to n - 1).
 * Node weights are all ones.  PPK_ERR_ARG, ppk_last_error() naming the first bad entry e, its i and j: i[e] != e / k
 * (rows not grouped), j outside [0, n), j == i, a NaN, infinite or negative distance (ppk_embed_dev: a P outside
 * [0, 1]).  Both device calls synchronise the stream once (the check's read-back).
 *
 * ppk_embed_weights_dev -> d_P float64 [n*k] and d_c uint64 [n*k] (nullable):
 *  - the distances are divided by their root mean square (left as they are when every one is 0) [EXT];
 *  - per row, x_j = d_j^2 - min_j d_j^2 and beta by float64 bisection from beta = 1 (doubling while no upper bound is
 *    known) on H(beta) = ln Z + beta sum_j p_j x_j / Z, p_j = exp(-beta x_j), Z = sum_j p_j, toward H = ln(perplexity):
 *    H > target raises beta.  It stops once hi - lo <= hi * 2^-48, or after 256 steps: a row that cannot reach the
 *    target (equal distances, zero distances of duplicates) ends at beta = 2^-256 or 2^256, finite.  K <= perplexity
 *    takes beta = 2^-256 without the bisection (at K == perplexity H is within rounding of the target up to
 *    beta ~ 1e-8, and the comparison would follow the last bit of log);
 *  - P[e] = (p_j / Z) / n (sum P = 1), c[e] = rint(P[e] * 2^52), the integer sampling weight of edge e.
 *
 * ppk_embed_dev: P (as above, or any P in [0, 1] whose weights c = rint(P * 2^52) can be summed in 64 bits: PPK_ERR_ARG
 * naming the sum once sum(c >> 20) >= 2^43, that is for every sum of c from 2^63 + n k 2^20 and for none below 2^63,
 * a sum of P of 2048; and PPK_ERR_ARG when every c is 0) + lists + seed -> d_Y float64 [n][2].  With W = min(workers, n)
 * workers per iteration (the cap that keeps small n stable) and T = max(1, rint(max_iter / W))
 * iterations (ties to even), every draw from the counter-based generator of ppk_embed.hip
 * (splitmix64 finaliser over seed, iteration, worker and draw):
 *  - Y starts uniform in +-1e-4; Eq = 1;
 *  - iteration t, learning rate eta = eta0 * max(1 - t / (T - 1), 1e-4) (T = 1: eta0): each worker draws one edge,
 *    upper_bound(prefix(c), mulhi64(r, sum c)), as its attractive pair (i, j), and n_repu (<= 127) pairs
 *    (mulhi64(r, n), mulhi64(r', n)) as repulsive pairs, skipping k == l.  For every pair (k, l), from the
 *    iteration's snapshot of Y: dY = y_k - y_l, q = 1 / (1 + |dY|^2), g = -4q (attractive) or 4q^2 / Eq
 *    (repulsive) [EXT]; gain = (eta g) dY, each coordinate clipped to +-0.1, is added to y_k and subtracted from
 *    y_l as int64 Q32.32 rint(gain * 2^32);
 *  - after the iteration, Y += deltas * 2^-32 and Eq = (Eq nsq + qsum) / (nsq + qcount), nsq = n(n - 1), qsum the
 *    Q32.32 sum of the repulsive pairs' q (2^-32 units), qcount how many repulsive pairs were not skipped [EXT].
 * Float64 throughout, un-fused, IEEE division.  Deterministic: integer accumulation only, so the same input gives the
 * same bits on every call, and the host restatement of these rules gives them too.  PPK_ERR_INTERRUPTED when the
 * interrupt check asks (polled every 256 iterations).  No synchronisation between iterations.
 * (Replaces poppunk_refine.get_kNN_distances + SCE.wtsne / wtsne_gpu_fp32 in generate_embedding,
 * PopPUNK/mandrake.py:66-111.) */
int ppk_embed_weights_dev(const long long *d_i, const long long *d_j, const float *d_dist, size_t n, size_t k,
                          double perplexity, double *d_P, unsigned long long *d_c, void *stream);
int ppk_embed_dev(const long long *d_i, const long long *d_j, const double *d_P, size_t n, size_t k,
                  unsigned long long seed, long long max_iter, int n_repu, double eta0, long long workers,
                  double *d_Y, void *stream);
/* Host arrays: i, j int64 [n*k], dist float32 [n*k] -> P float64 [n*k] (nullable), Y float64 [n][2], on device_id;
 * ppk_embed_weights_dev then ppk_embed_dev; blocking.  max_iter >= 1, 1 <= workers <= 2^24. */
int ppk_embed(const long long *i, const long long *j, const float *dist, size_t n, size_t k, double perplexity,
              unsigned long long seed, long long max_iter, int n_repu, double eta0, long long workers, int device_id,
              double *P, double *Y);

/* ------------------------------------------------------------------------
 * Host-buffer convenience wrappers (what a pybind11/ctypes drop-in binds):
 * upload, run on `devices[0..n_dev)` (the pair space is band-split across
 * them), copy back.  Blocking.
 */
/* replaces pp_sketchlib.queryDatabase(ref_db_name, query_db_name, rList, qList,
 * klist, random_correct, jaccard, num_threads, use_gpu, device_id) after the
 * HDF5 read (PopPUNK/sketchlib.py:528-537; positional order pinned by
 * test/test-update-gpu.py:85-86).  n_qry == 0 => self.  out: float
 * [n_pairs][2] or [n_pairs][nk] (PPK_FLAG_JACCARD) or uint32 (PPK_FLAG_COUNTS).
 * The result is produced in sub-bands through two alternating device buffers of
 * about 64 MB (sub-band c downloads while c+1 computes), so device memory use is
 * bounded by the sketches plus those buffers for any job size -- the
 * device-memory chunking of pp-sketchlib's CUDA path [EXT].  `out` is written by this call only; a few
 * helper threads touch its pages ahead of the download (option "prefault_threads", default 8, 0 = off).
 * The resident form of the sketches and the two buffers are KEPT between calls, keyed by the host
 * pointer, the dimensions and a 64-bit hash of EVERY word of the array (computed on the helper threads,
 * ~0.6 ms per 90 MB, WHILE the job already runs on the resident copy; checked before the call returns):
 * an array rewritten in place, or another one at a recycled address, is uploaded again and the job run
 * again -- there is no stale-answer mode.  Option "db_cache" 0 turns the cache off; ppk_release_scratch
 * frees it; at most 4 databases per device are kept, and they are dropped first when device memory
 * runs out.  A caller that knows its data's identity avoids the hash altogether by holding ppk_db
 * handles and calling ppk_query_dbs (what the Python mirror does).
 * Several devices: ONE HOST WORKER THREAD PER LISTED DEVICE uploads (or finds resident) the sketches,
 * computes its share of the pair space and downloads it into its disjoint row range of `out`, all
 * devices side by side -- each GPU's PCIe link carries its own share (a copy into pageable memory
 * blocks the issuing thread, hence threads, not just streams).  This is the multi-GPU route of a
 * single-process caller (PopPUNK passes one device_id; the mirror reads PPK_DEVICES=0,1,...).  The
 * interrupt check and the progress meter run on the calling thread.
 */
int ppk_query(const uint64_t *ref_sk, size_t n_ref, const uint64_t *qry_sk,
              size_t n_qry, const int32_t *kmers, size_t nk, size_t sketchsize64,
              size_t bbits, const float *random_tbl, const uint16_t *ref_clu,
              const uint16_t *qry_clu, size_t n_clu, int flags, const int *devices,
              int n_dev, void *out, unsigned long long *n_failed);

/* The same with the sketches already resident: refs[d] (and qrys[d]; qrys == NULL => self) is the
 * database as created by ppk_db_create on the d-th device, one per device, all of the same samples.
 * Nothing is uploaded, hashed or looked up; device d computes its share and sends it to its rows of
 * the host array `out` through its two persistent sub-band buffers, the devices side by side on one
 * worker thread each.  What the Python mirror of queryDatabase calls for a database it has loaded
 * (it keys the handles by file, modification time, names and k list: poppunk_assign against one
 * reference database; every --plot-fit re-query, PopPUNK/sketchlib.py:547-564). */
int ppk_query_dbs(const ppk_db *const *refs, const ppk_db *const *qrys, int n_dev,
                  const int32_t *kmers, const float *random_tbl, size_t n_clu, int flags,
                  void *out, unsigned long long *n_failed);
/* one device: ppk_query_dbs(&ref, qry ? &qry : NULL, 1, ...) */
int ppk_query_db(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                 const float *random_tbl, size_t n_clu, int flags, void *out,
                 unsigned long long *n_failed);
/* What the last ppk_query / ppk_query_dbs of the process ran side by side (measurement, tests):
 * vals[0] device entries, [1] worker threads (0 = ran on the calling thread), [2] most result
 * downloads in flight at one time, [3] most sketch uploads in flight at one time, [4] wall ms of the
 * device phase, [5] longest upload ms, [6] longest per-device ms, [7] ppk_query calls since the process
 * began that ran a second time because their resident copy proved stale. */
int ppk_query_last_stats(double *vals, int n);

int ppk_assign_threshold(const float *dist, size_t n_rows, int slope, float x_max,
                         float y_max, int device_id, float *out);

/* Edge lists have a data-dependent size: *n_edges always receives the total;
 * PPK_ERR_CAPACITY is returned when it exceeds cap (nothing is written).  The call that reports
 * PPK_ERR_CAPACITY has already computed the whole list: it stays parked on the device for the calling
 * thread, which fetches it with ppk_parked_fetch into a buffer of that size -- "ask the size, then
 * fetch" costs one upload and one device pass (also for the two sweeps below).  The hand-over is
 * explicit: no call is ever answered from a parked result, so a rewritten or recycled input array
 * cannot meet a stale list; calling the same entry point again with more room simply recomputes.  Every
 * thread has its own slot: a parked result is dropped by the SAME thread's next call of this family, by its
 * fetch and by ppk_release_scratch -- never by another thread's call, so concurrent callers do not disturb
 * each other's hand-over (at most 16 threads hold one at a time; the oldest goes first). */
int ppk_edge_threshold(const float *dist, size_t n_rows, size_t n_ref, int slope,
                       float x_max, float y_max, int inclusive, int device_id,
                       long long *ij_out, size_t cap, size_t *n_edges);
int ppk_generate_tuples(const int32_t *assignments, size_t n_rows, int within_label,
                        int self, size_t num_ref, long long int_offset, int device_id,
                        long long *ij_out, size_t cap, size_t *n_edges);
/* [OUTSIDE SURVEY 8] host form of ppk_generate_all_tuples_dev */
int ppk_generate_all_tuples(size_t num_ref, size_t num_queries, int self, long long int_offset,
                            int device_id, long long *ij_out, size_t cap, size_t *n_edges);
/* replaces the numpy masks + .tolist() + poppunk_refine.generateTuples of qcDistMat on a HOST matrix
 * (PopPUNK/qc.py:332-337: core > max_pi or accessory > max_a; :349-354: core == 0 or accessory == 0), both
 * lists from one upload: `modes` bit 0 = the long-distance list, bit 1 = the zero-distance list, written one
 * after the other to ij_out; *n_edges = entries of both, *n_first = entries of the first list asked for.
 * n_ref == 0: self (condensed) matrix, else row = q*n_ref + r as in ppk_edge_threshold. */
int ppk_qc_edges(const float *dist, size_t n_rows, size_t n_ref, int modes, float max_pi,
                 float max_a, int device_id, long long *ij_out, size_t cap, size_t *n_edges,
                 size_t *n_first);
/* The result the calling thread's last ppk_edge_threshold / ppk_generate_tuples / ppk_qc_edges (out0 = int64 [n][2];
 * out1, out2 ignored) or ppk_threshold_iterate_1d / _2d (out0, out1, out2 = i, j, offset index, int64
 * [n] each) call parked when it returned PPK_ERR_CAPACITY.  cap = room in entries; *n_out (nullable)
 * receives the entry count.  PPK_ERR_STATE when this thread has nothing parked; the result is freed by
 * a successful fetch. */
int ppk_parked_fetch(long long *out0, long long *out1, long long *out2, size_t cap, size_t *n_out);

/* Sketches in, edge list out, on one or several devices: queryDatabase -> (X / scale) ->
 * poppunk_refine.assignThreshold -> generateTuples (PopPUNK/models.py:1065-1091,
 * PopPUNK/network.py:1180-1184), or -> poppunk_refine.edgeThreshold (PopPUNK/refine.py:535), as ONE host
 * call in which the [n_pairs, 2] matrix never exists, on the device or on the host: every listed device
 * runs ppk_dist_edges_dev on its band of query rows (ppk_band_split; one worker thread per device),
 * 16 bytes per EDGE cross PCIe instead of 8 bytes per PAIR, and the bands' lists are concatenated in
 * device-list order = reference row order (src/boundary.cpp:101-118), so the list does not depend on the
 * number of devices.  slope / x_max / y_max / scale / inclusive as in ppk_dist_edges_dev; ij_out int64
 * [cap][2], *n_edges the total; with too little room the finished list is parked (on the host) for
 * ppk_parked_fetch, as above.  A device works through its band in pieces whose edge bitmask stays below
 * 2 GiB (option "chunk_rows" scales it), so the job size is bounded by the edge list, not by n^2 bits.
 * Any k list runs here (more than 128 count bits per pair: the wide-k tile kernel); only sketches with a bbits other
 * than PopPUNK's 14 AND more than 128 count bits -- nothing PopPUNK writes -- keep the band in one piece.
 *   ppk_query_edges_dbs : refs[d] / qrys[d] (qrys NULL = self) = the same database resident on each device
 *   ppk_query_edges     : host sketch arrays as in ppk_query; the resident copies come from (and stay in)
 *                         ppk_query's cache, every word hashed before anything runs */
int ppk_query_edges_dbs(const ppk_db *const *refs, const ppk_db *const *qrys, int n_dev,
                        const int32_t *kmers, const float *random_tbl, size_t n_clu, int flags,
                        int slope, float x_max, float y_max, float scale_x, float scale_y,
                        int inclusive, long long *ij_out, size_t cap, size_t *n_edges,
                        unsigned long long *n_failed);
int ppk_query_edges(const uint64_t *ref_sk, size_t n_ref, const uint64_t *qry_sk, size_t n_qry,
                    const int32_t *kmers, size_t nk, size_t sketchsize64, size_t bbits,
                    const float *random_tbl, const uint16_t *ref_clu, const uint16_t *qry_clu,
                    size_t n_clu, int flags, int slope, float x_max, float y_max, float scale_x,
                    float scale_y, int inclusive, const int *devices, int n_dev, long long *ij_out,
                    size_t cap, size_t *n_edges, unsigned long long *n_failed);

/* ------------------------------------------------------------------------
 * [OUTSIDE SURVEY 8: every entry point of this block; oracle restated by reading, parity unpinned]
 * The sparse neighbour matrices of the lineage models (COO triplets, rows ascending; int64 indices,
 * float32 distances; host arrays).  Outputs in row order as the reference concatenates them; *n_out
 * always receives the entry count, PPK_ERR_CAPACITY when it exceeds cap (worst cases below).
 */
/* replaces poppunk_refine.lowerRank(rr_mat, n_samples, kNN, reciprocal_only, count_unique_distances,
 * lineage_resolution, num_threads) (src/python_bindings.cpp:121-128; src/extend.cpp:128-246; caller
 * PopPUNK/models.py:1177): per row, entries in stable order of distance, the sample itself skipped, kept
 * while the count of kept entries -- or, with count_unique_distances, of distinct distances (steps of at
 * least epsilon) -- is <= kNN (so kNN + 1 entries without it, as in the reference); reciprocal_only keeps
 * (i, j), i < j, whose (j, i) was kept too.  Worst case nnz entries. */
int ppk_lower_rank(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
                   size_t n_samples, size_t knn, int reciprocal_only, int count_unique_distances,
                   float epsilon, int device_id, long long *i_out, long long *j_out, float *d_out,
                   size_t cap, size_t *n_out);
/* replaces poppunk_refine.extend(rr_mat, qq_mat, qr_mat, kNN, num_threads) (src/python_bindings.cpp:114-119;
 * src/extend.cpp:52-126; caller PopPUNK/models.py:1367): the kNN nearest of every reference (its sparse row
 * merged with its n_qry distances to the queries, qr_rect float32 [n_ref][n_qry]) and of every query (its
 * distances to the references merged with its row of qq_square, float32 [n_qry][n_qry]); stable order of
 * distance, the query side first on a tie, the sample itself skipped; queries are numbered n_ref + q.
 * Worst case kNN * (n_ref + n_qry) entries. */
int ppk_extend(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
               const float *qq_square, const float *qr_rect, size_t n_ref, size_t n_qry, size_t knn,
               int device_id, long long *i_out, long long *j_out, float *d_out, size_t cap,
               size_t *n_out);

/* poppunk_refine.extend with the sketches in the place of its two dense matrices: `ref` / `qry` are resident
 * databases on one device, the query x reference rectangle and the query square PopPUNK computes for the call
 * (queryDatabase twice, longToSquare, PopPUNK/models.py:1355-1365) never exist -- the tiles deliver every
 * reference's kNN nearest queries, every query's kNN nearest references and kNN nearest queries, which is all
 * extend's merge can keep.  Distances are the kernel's (no 1e-10 floor: apply it to the output, it preserves
 * the order); rr_* as in ppk_extend; knn <= 32, bbits = 14.  Output as ppk_extend, worst case
 * kNN * (n_ref + n_qry). */
int ppk_extend_sketches(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
                        const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl,
                        size_t n_clu, int flags, int knn, int dist_col, long long *i_out, long long *j_out,
                        float *d_out, size_t cap, size_t *n_out);
/* ... on several devices: refs[d] / qrys[d] = the two databases resident on device d; both passes are cut into
 * bands of query rows, one per device, and the bands' lists merged as ppk_query_knn_dbs merges them. */
int ppk_extend_sketches_dbs(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
                            const ppk_db *const *refs, const ppk_db *const *qrys, int n_dev,
                            const int32_t *kmers, const float *random_tbl, size_t n_clu, int flags, int knn,
                            int dist_col, long long *i_out, long long *j_out, float *d_out, size_t cap,
                            size_t *n_out);

/* ------------------------------------------------------------------------
 * Long <-> square distance transforms and k nearest neighbours (SURVEY.md 8f
 * rank 2).  "Long" = condensed upper triangle in PopPUNK row order; element e
 * of a long vector is read at d_long[e*stride + col], so a column of the
 * resident [n_pairs][2] matrix is used in place (stride 2, col 0/1).
 */
/* replaces pp_sketchlib.longToSquare(distVec, num_threads) [EXT]
 * (PopPUNK/utils.py:393-396): symmetric n x n, zero diagonal */
int ppk_long_to_square_dev(const float *d_long, size_t stride, size_t col, size_t n,
                           float *d_square, void *stream);
/* replaces pp_sketchlib.longToSquareMulti(distVec, query_ref_distVec,
 * query_query_distVec, num_threads) [EXT] (PopPUNK/utils.py:398-405):
 * (n_ref+n_qry)^2 matrix from the ref-ref, query-ref (row = q*n_ref + r) and
 * query-query long vectors */
int ppk_long_to_square_multi_dev(const float *d_rr, const float *d_qr, const float *d_qq,
                                 size_t stride, size_t col, size_t n_ref, size_t n_qry,
                                 float *d_square, void *stream);
/* replaces pp_sketchlib.squareToLong(distMat, num_threads) [EXT]
 * (PopPUNK/network.py:2133-2134) */
int ppk_square_to_long_dev(const float *d_square, size_t n, float *d_long, void *stream);
/* replaces poppunk_refine.get_kNN_distances(distMat, kNN, dist_col, num_threads)
 * (src/extend.cpp:248-289): per row the kNN smallest entries other than the row
 * itself, ties by column index; outputs [n*kNN] (i, j, dist) */
int ppk_knn_dev(const float *d_square, size_t n, int knn, long long *d_i, long long *d_j,
                float *d_dist, void *stream);
/* the same on a rows x cols block of distances (e.g. one band of a ref x query result,
 * element (i, c) at d_block[(i*n_cols + c)*stride + col]); row i is sample self_offset + i,
 * whose own column is skipped.  Lets k nearest neighbours be taken band by band straight
 * from kernel 1 without ever holding the n x n matrix. */
int ppk_knn_rect_dev(const float *d_block, size_t stride, size_t col, size_t n_rows,
                     size_t n_cols, size_t self_offset, int knn, long long *d_i, long long *d_j,
                     float *d_dist, void *stream);
/* k nearest neighbours of every sample of a database straight from kernel 1's tiles: what
 * get_kNN_distances(longToSquare(queryDatabase(...)[:, dist_col]), kNN) gives (callers
 * PopPUNK/models.py:1215-1222, PopPUNK/assign.py:680-686), with the upper triangle compared once
 * and neither the square nor the long-form distance matrix ever materialised.  Each tile emits a
 * pair's distance as a neighbour candidate of both its samples while it beats a per-sample bound that
 * tightens as tiles finish; a sort by sample and a per-sample selection (ties by column index, as
 * the reference's stable sort, src/extend.cpp:266-279) finish.  knn <= 32; bbits = 14.  Outputs
 * [n*knn] (i, j, dist) on the device; *n_candidates (host, nullable) receives the number of
 * candidates the tiles emitted.  Synchronises the stream (the candidate count sizes the sort). */
int ppk_knn_sketches_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                         size_t n_clu, int flags, int knn, int dist_col, long long *d_i,
                         long long *d_j, float *d_dist, unsigned long long *n_candidates,
                         void *stream);
/* One band [q_begin, q_end) of the triangle's rows (the unit of multi-GPU sharding, ppk_band_split): the best
 * knn per sample among the band's pairs -- a pair belongs to the band of its smaller sample and is a candidate
 * for both of its samples -- with unfilled slots marked j = -1.  Merging the bands' lists per sample by
 * (distance bits, j) gives ppk_knn_sketches_dev's result (engine.knn_sharded; ppk_query_knn_dbs does it for
 * the devices of one process). */
int ppk_knn_sketches_band_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                              size_t n_clu, int flags, int knn, int dist_col, size_t q_begin,
                              size_t q_end, long long *d_i, long long *d_j, float *d_dist,
                              unsigned long long *n_candidates, void *stream);
/* The same for a reference x query job, one pass over the rectangle: outputs [(n_ref + n_qry) * knn]; sample
 * s < n_ref is reference s and its neighbours are its knn nearest QUERIES (numbered n_ref + q), sample n_ref + q
 * is query q and its neighbours are its knn nearest REFERENCES -- the two dense sides of poppunk_refine.extend's
 * merge (src/extend.cpp:52-126), see ppk_extend_sketches. */
int ppk_knn_sketches_rq_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                            const float *random_tbl, size_t n_clu, int flags, int knn, int dist_col,
                            long long *d_i, long long *d_j, float *d_dist,
                            unsigned long long *n_candidates, void *stream);

/* The same as a HOST call on one or several devices: every listed device takes a band of the triangle's rows
 * (a pair is a candidate for both of its samples, so the bands' per-sample lists merge into the whole job's),
 * the lists -- knn entries per sample and device -- come to the host and are merged per sample in the
 * reference's stable order.  Outputs host arrays [n*knn]: i (the sample, repeated), j, dist; a sample with
 * fewer than knn other samples keeps (i, 0, 0.0) in its last slots as in src/extend.cpp:266-279.
 *   ppk_query_knn_dbs : dbs[d] = the database resident on device d
 *   ppk_query_knn     : host sketch array as in ppk_query (resident copies from / into its cache) */
int ppk_query_knn_dbs(const ppk_db *const *dbs, int n_dev, const int32_t *kmers, const float *random_tbl,
                      size_t n_clu, int flags, int knn, int dist_col, long long *i_out,
                      long long *j_out, float *d_out);
int ppk_query_knn(const uint64_t *sk, size_t n, const int32_t *kmers, size_t nk, size_t sketchsize64,
                  size_t bbits, const float *random_tbl, const uint16_t *clu, size_t n_clu, int flags,
                  int knn, int dist_col, const int *devices, int n_dev, long long *i_out,
                  long long *j_out, float *d_out);
/* The same in two pieces, for N GPUs (engine.knn_sharded): every rank emits the neighbour candidates of
 * its band of query rows [q_begin, q_end) -- (sample, distance bits << 32 | other sample) for BOTH
 * samples of each pair in the band -- into d_keys / d_vals (capacity `cap`; *n_candidates (host) gets
 * the total, PPK_ERR_CAPACITY if it exceeds cap); the lists are concatenated in any order and one rank
 * selects every sample's knn smallest (distance, column) keys from them.  ppk_knn_candidates_dev
 * synchronises the stream. */
int ppk_knn_candidates_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                           size_t n_clu, int flags, int knn, int dist_col, size_t q_begin,
                           size_t q_end, unsigned *d_keys, unsigned long long *d_vals, size_t cap,
                           unsigned long long *n_candidates, void *stream);
int ppk_knn_select_dev(const unsigned *d_keys, const unsigned long long *d_vals, size_t count,
                       size_t n, int knn, long long *d_i, long long *d_j, float *d_dist,
                       void *stream);
/* replaces the per-row Python copy loop of PopPUNK.qc.prune_distance_matrix
 * (PopPUNK/qc.py:58-83): the long-form (condensed, PopPUNK row order) matrix of the
 * samples keep[0] < keep[1] < ... out of n; `cols` floats per row (2 for distances) */
int ppk_prune_long_dev(const float *d_long, size_t n, size_t cols, const long long *d_keep,
                       size_t n_keep, float *d_out, void *stream);
/* replaces the boolean row mask of PopPUNK.qc.prune_query_distance_matrix
 * (PopPUNK/qc.py:121-135): the n_ref-row blocks (row = q*n_ref + r) of the kept queries */
int ppk_prune_query_rows_dev(const float *d_qr, size_t n_ref, size_t cols,
                             const long long *d_keep, size_t n_keep, float *d_out,
                             void *stream);
/* host-buffer forms */
int ppk_prune_long(const float *dist, size_t n, size_t cols, const long long *keep,
                   size_t n_keep, int device_id, float *out);
int ppk_long_to_square(const float *vec, size_t n, int device_id, float *square);
int ppk_long_to_square_multi(const float *rr, const float *qr, const float *qq, size_t n_ref,
                             size_t n_qry, int device_id, float *square);
/* replaces the body of PopPUNK.utils.update_distance_matrices (PopPUNK/utils.py:357-408): BOTH square
 * matrices (core, accessory) from the two-column long matrices [rows][2] as PopPUNK holds them -- one upload of
 * each, the kernels read the columns in place.  qr == NULL and n_qry == 0: refs only (its longToSquare branch);
 * else rr [n_ref(n_ref-1)/2][2], qr [n_qry*n_ref][2] (row = q*n_ref + r), qq [n_qry(n_qry-1)/2][2] (may be NULL
 * when n_qry == 1) -> two (n_ref+n_qry)^2 matrices (its longToSquareMulti branch). */
int ppk_long_to_square2(const float *rr, const float *qr, const float *qq, size_t n_ref, size_t n_qry,
                        int device_id, float *core_square, float *acc_square);
int ppk_square_to_long(const float *square, size_t n, int device_id, float *vec);
int ppk_knn(const float *square, size_t n, int knn, int device_id, long long *i_out,
            long long *j_out, float *dist_out);

/* host-buffer forms of the two sweeps (PPK_ERR_CAPACITY when *n_out > cap) */
int ppk_threshold_iterate_1d(const float *dist, size_t n_rows, const double *offsets,
                             size_t n_off, int slope, float x0, float y0, float x1, float y1,
                             int device_id, long long *i_out, long long *j_out,
                             long long *off_out, size_t cap, size_t *n_out);
int ppk_threshold_iterate_2d(const float *dist, size_t n_rows, const float *x_max, size_t n_off,
                             float y_max, int device_id, long long *i_out, long long *j_out,
                             long long *off_out, size_t cap, size_t *n_out);

/* ------------------------------------------------------------------------
 * Sketch database files: bulk read of `<db>/<db>.h5` (layout PopPUNK/web.py:14-61:
 * /sketches/<sample>/<k> uint64 datasets, attributes sketchsize64, bbits, kmers, length,
 * missing_bases, base_freq on the sample group).  Replaces the per-sample, per-k h5py reads of
 * PopPUNK/sketchlib.py:86-88,:124-133,:155-158,:197-214,:672-690 and the HighFive reads inside
 * pp_sketchlib.queryDatabase(ref_db_name, query_db_name, rList, qList, ...) [EXT], which takes database
 * PREFIXES and opens the files itself (PopPUNK/sketchlib.py:520,:528-537).  Host code; needs no device.
 *   backend 0 = choose: 1 the direct reader (the file is mmap-ed and its superblock-0/1, version-1
 *     object-header, symbol-table-group, contiguous-dataset structures -- what h5py and HighFive write by
 *     default -- are read in place by several threads: < 1 us per dataset); when the file holds anything
 *     else, 2: libhdf5's C API, dlopen-ed ($HDF5_LIB, the loader path, ppk_h5_set_library), one H5Fopen,
 *     per sample one H5Gopen2 and nk H5Dopen2 + H5Dread into the caller's array (~23 us per dataset).
 *     1 or 2 force that backend (PPK_ERR_STATE when the direct reader does not read the file).
 *   names: `n` NUL-terminated strings back to back.  ppk_h5_names gives every sample of the file in
 *     name order (what h5py's keys() yields); *need = bytes, buf may be NULL to ask.
 *   ppk_h5_params: sketchsize64 / bbits / kmers attributes of `sample` (NULL = the first).
 *   ppk_h5_read: out uint64 [n][nk][words] in the order of `names` and `kmers`, words = sketchsize64*bbits
 *     (a dataset of another length is an error, as are a missing sample or k: messages as the Python
 *     reader's); lengths / missing int64 [n], base_freq double [n][4] (NaN where the attribute is absent
 *     or not of length 4) -- each nullable; threads 0 = default.
 */
typedef struct ppk_h5 ppk_h5;
int ppk_h5_set_library(const char *libhdf5_path);
int ppk_h5_open(const char *path, int backend, ppk_h5 **out);
void ppk_h5_close(ppk_h5 *h);
int ppk_h5_backend(const ppk_h5 *h);
const char *ppk_h5_declined(const ppk_h5 *h); /* why the direct reader passed the file on ("" if it did not) */
int ppk_h5_has_random(const ppk_h5 *h);       /* a /random group is present (PopPUNK/sketchlib.py:461-466) */
size_t ppk_h5_count(ppk_h5 *h);
int ppk_h5_names(ppk_h5 *h, char *buf, size_t cap, size_t *need);
int ppk_h5_params(ppk_h5 *h, const char *sample, size_t *sketchsize64, size_t *bbits, int64_t *kmers,
                  size_t kmers_cap, size_t *n_kmers);
/* codon_phased attribute of /sketches (PopPUNK/sketchlib.py:120-121): 1 / 0, -1 when absent */
int ppk_h5_codon_phased(const ppk_h5 *h);
/* sketchsize64 / bbits / kmers of EVERY sample, file order: int64 [count], int64 [count], int64 [count][kmers_cap],
 * size_t [count] (number of k-mer lengths stored; 0 = attribute absent) -- the consistency checks of
 * getSketchSize / getKmersFromReferenceDatabase (PopPUNK/sketchlib.py:109-168) in one native pass */
/* count_cap: rows the arrays hold.  PPK_ERR_CAPACITY when the file lists more samples than that -- also when the
 * direct reader hands the file to libhdf5 in the middle of the pass and the library's listing (every link) is longer
 * than the one the arrays were sized from (hard links only): re-list (ppk_h5_count / ppk_h5_names) and call again. */
int ppk_h5_all_params(ppk_h5 *h, size_t count_cap, int64_t *sketchsize64, int64_t *bbits, int64_t *kmers,
                      size_t kmers_cap, size_t *n_kmers);
int ppk_h5_read(ppk_h5 *h, const char *names, size_t n, const int32_t *kmers, size_t nk, size_t words,
                uint64_t *out, int64_t *lengths, int64_t *missing, double *base_freq, int threads);

/* ------------------------------------------------------------------------
 * Sketching: the codes of n assemblies -> their bin sketches, in the layout every other entry point
 * reads.  [EXT] The rule -- 64-bit ntHash with seeds recalled from memory, bin = floor(h * nbins / 2^64), the bin's
 * minimum cut to its low bbits bits, an empty bin filled from the nearest non-empty bin above it, cyclically -- is this
 * project's own ("poppunk_amd:sketch1"): pp-sketchlib is not in the tree, and sketches made here are NOT bit-compatible
 * with databases it wrote.  The whole rule is three device functions of poppunk_amd/csrc/ppk_device.h.
 *     d_codes    uint8: 0-3 = A, C, G, T; 4 = any other residue; 5 = contig break.  A k-mer is hashed when its k
 *                codes are all below 4.
 *     d_seq_off  long long [n + 1]: sample i is d_codes[d_seq_off[i] .. d_seq_off[i + 1]); ascending, from 0 or above
 *     kmers      int32 [nk] (host): 3 .. 101 each, nk <= 128
 *     flags      PPK_SKETCH_STRAND_PRESERVED: the forward hash alone, not min(forward, reverse complement)
 *     d_sketches uint64 [n][nk][sketchsize64 * bbits], word [blk * bbits + b] = bit b of bins 64 blk .. 64 blk + 63
 *     d_stats    long long [n][6]: length (codes below 5), missing bases (codes 4), then the counts of A, C, G, T
 *     d_filled   int32 [n][nk]: the non-empty bins before empty ones were filled; 0 = the sample has no k-mer of that
 *                length, and its words are all zero
 * The same bits on every call, for every cut of the sequences and for every value of the routing options.
 * PPK_ERR_ARG, before any device is touched: a NULL array, nk outside 1 .. 128, a k-mer length outside 3 .. 101, bbits
 * other than 14, sketchsize64 below 1 or above 4 096, an unknown flag.  PPK_ERR_ARG, ppk_last_error() naming the first
 * offender: offsets that do not ascend ("offsets do not ascend at sample 3"), a code above 5 ("sample 2, position 17
 * (code 1234): code 9 above 5").  The kernels are enqueued on `stream`, which is then synchronised once for that check.
 * Scratch: 8 bytes per (sample, k, bin) for groups of samples of up to 512 MiB.
 * (Replaces the sketching half of pp_sketchlib.constructDatabase [EXT], call site PopPUNK/sketchlib.py:410-422.) */
#define PPK_SKETCH_STRAND_PRESERVED 1
int ppk_sketch_dev(const uint8_t *d_codes, const long long *d_seq_off, size_t n, const int32_t *kmers, size_t nk,
                   size_t sketchsize64, size_t bbits, int flags, uint64_t *d_sketches, long long *d_stats,
                   int32_t *d_filled, void *stream);
/* Host arrays of the same shapes, on device_id; blocking.  The codes go up through pinned staging in batches of whole
 * samples of at most option "sketch_batch_mb" MiB (at least one sample; "sketch_batch" forces the count). */
int ppk_sketch(const uint8_t *codes, const long long *seq_off, size_t n, const int32_t *kmers, size_t nk,
               size_t sketchsize64, size_t bbits, int flags, int device_id, uint64_t *sketches, long long *stats,
               int32_t *filled);

/* ------------------------------------------------------------------------
 * Sketching read sets: as above -- the same hash, bin, bin value, densify and layout, so that a sketch
 * of reads and a sketch of an assembly are comparable -- but a k-mer may enter a bin only when it was seen at least
 * min_count times in the sample.  All n samples are reads: every read is a contig (a code 5 between reads).
 * A k-mer's count is the number of valid start positions of the sample whose kept hash equals its own (both strands
 * together unless strand-preserved; counts are of 64-bit hash values).
 *   table route (default)  [EXT: rows, remix and default B are this project's own; upstream's count-min table is
 *                recalled, not pinned]  2 rows of 2^B 32-bit counters; a counter holds the sum of the counts of the
 *                hashes that index it (ppk_sketch_count_index of ppk_device.h); a k-mer is admitted when both its
 *                counters reach min_count.  A superset of the exact route's k-mers: no true k-mer is dropped.
 *                B = ppk_sketch_count_bits(the sample's code count): 12 .. 26; option "sketch_count_bits" forces it.
 *   exact route (PPK_SKETCH_EXACT)  a k-mer is admitted when its count reaches min_count.  The table is the first
 *                filter; every bin's winner is then counted exactly, a bin whose winner falls short takes the next
 *                admitted value above it, and so on until no bin fails: at most option "sketch_exact_rounds" select
 *                passes per group of samples, else PPK_ERR_CAPACITY naming the first failing sample and k ("sample 0,
 *                k 13: bins still hold a k-mer below the minimum count after 4 exact rounds").
 *   min_count 1  admits everything and builds no table: words and filled are bit for bit those of ppk_sketch.
 * A bin's value is the least admitted kept hash that falls in it; d_filled counts the bins with one.
 *     min_count  1 .. 65 535
 *     d_kstats   long long [n][nk][4]: occ (valid start positions), adm_occ (those whose k-mer passes the count table;
 *                all of them at min_count 1; on BOTH routes the table's verdict -- exact counts exist for winners
 *                only), filled, win_occ (the sum of the exact counts of the bins' winning k-mers)
 *     d_stats    as above, except length: the winners are a uniform sample of the admitted distinct k-mers, so
 *                adm_occ * filled / win_occ estimates their number; length is that estimate at the largest k, rounded
 *                half up (ppk_sketch_reads_length), 0 when nothing was admitted.  The other five count all read bases.
 * The same bits on every call, for every cut of the codes, every batch and every routing option: a counter only grows
 * and is only asked "at least min_count?", so skipping the atomic once it shows min_count changes no answer.
 * PPK_ERR_ARG before any device is touched: everything ppk_sketch checks, min_count outside 1 .. 65 535, an unknown flag,
 * option "sketch_count_bits" outside 0, 4 .. 26; later: a sample of more than 2^32 - 1 codes (32-bit counters).
 * Scratch: per (sample, k) of a group 24 bytes per bin (minimum, floor, winner count; groups of up to 512 MiB) and
 * 2 x 2^B x 4 bytes of counters (groups of up to 512 MiB; a sample whose tables alone exceed that goes a few k at a time).
 * ppk_sketch_reads_dev copies the n + 1 offsets to the host first (the groups are planned there), then enqueues on
 * `stream`; the exact route synchronises it once per round. */
#define PPK_SKETCH_EXACT 2
int ppk_sketch_reads_dev(const uint8_t *d_codes, const long long *d_seq_off, size_t n, const int32_t *kmers, size_t nk,
                         size_t sketchsize64, size_t bbits, int flags, int min_count, uint64_t *d_sketches,
                         long long *d_stats, long long *d_kstats, int32_t *d_filled, void *stream);
/* Host arrays of the same shapes, on device_id; blocking; batches as ppk_sketch ("sketch_batch_mb", "sketch_batch"). */
int ppk_sketch_reads(const uint8_t *codes, const long long *seq_off, size_t n, const int32_t *kmers, size_t nk,
                     size_t sketchsize64, size_t bbits, int flags, int min_count, int device_id, uint64_t *sketches,
                     long long *stats, long long *kstats, int32_t *filled);

/* ------------------------------------------------------------------------
 * Measurement hooks (bench.py): when enabled, the dominant kernel of each
 * ppk_dist*_dev call is bracketed by hipEvents on its own stream.
 */
int ppk_prof_enable(int on);
/* Sum of elapsed ms and number of bracketed launches since the last reset;
 * synchronises the recorded events. */
int ppk_prof_read(double *total_ms, long long *n_launches, int reset);
/* name of the kernel variant the last ppk_dist*_dev call launched */
const char *ppk_last_kernel_name(void);
/* The kernel shape a band of pair tiles would run through, as a pure function of the job (refs, query rows of the band,
 * self, k-mer lengths, sketchsize64, bbits, fused-boundary / neighbour mode), the device (compute units, XCDs, resident
 * 512-thread workgroups of the tile kernel: 256 / 8 / 512 on MI355X in SPX mode) and seven options in this order:
 * ksplit, ksplit_wide, ksplit_long, ksplit_fused, ksplit_slices, wide_kpg, scratch bytes allowed.  No device is touched.
 * route: 0 tile kernel, 1 k-split in one launch, 2 k-split counts pass + regression pass, 3 tile kernel with a windowed
 * count register, 4 raw counts + generic regression.  (Replaces nothing of the reference: the dispatch of kernel 1.) */
int ppk_choose_route(size_t n_ref, size_t q_rows, int self, int nk, int sketchsize64, int bbits, int mask, int knn,
                     int cus, int xcds, int tile_slots, const long long *knobs, int *route, int *slices, size_t *tiles,
                     size_t *limit);
/* Which coded copies ppk_db_create builds, as a pure function of what its count pass reads back (counts: n_counts =
 * 3 x (1 + nk * sketchsize64) + 3 + nk * sketchsize64 * 64 words -- the ppk_db_rank_counts layout, then E2 of every
 * position [k][64 * sketchsize64]), the shape, the device's resident tile workgroups and four options in this order:
 * rank_fold, rank_fold2, fold2_sort, rank_foldh.  No device is touched.  first: the coding tried first, fallback: the
 * one tried if that is dropped (device full, or a (pair, k) past the event field) -- 0 the injective copy, 1 the folded
 * pair, 2 the two-holder pair, -1 the raw planes.  plane_sums[3]: the planes a self job compares over the stored blocks
 * with the codings of D, E and E2.  With first == 2, and each where not NULL: order[nk * 64 * sketchsize64] the
 * two-holder pair's slot order, flags[2 * 16] the per-k words of its 7-plane and then its 6-plane blocks,
 * stream_planes[nk * sketchsize64] and their sum, and whether the holder pair is to be tried beside it. */
int ppk_choose_coding(const uint32_t *counts, size_t n_counts, size_t n, size_t nk, size_t sketchsize64, size_t bbits,
                      int tile_slots, const long long *options, int *first, int *fallback, size_t *plane_sums,
                      uint32_t *order, uint32_t *flags, uint8_t *stream_planes, size_t *stream_sum, int *try_holder);
/* The holder bound H of the holder pair (holders: 0 = no pair), as a pure function of E_H per position and ladder rung
 * (pos_e[(k * 64 * sketchsize64 + position) * 7 + rung], rungs H = 4, 8, ... 256; with foldh_holders > 0 rung 0 is that
 * H and the only one read), the shape, the resident tile workgroups, the most shared values of any position, the
 * two-holder pair's stream plane sum and the options rank_foldh and foldh_holders.  No device is touched.  With a pair:
 * order[nk * 64 * sketchsize64] its slot order, block_planes[nk * sketchsize64] of 2, 3 or 4, max_entries the cap on
 * its entries. */
int ppk_choose_holder(const uint32_t *pos_e, size_t n_pos_e, size_t n, size_t nk, size_t sketchsize64, int tile_slots,
                      size_t most_shared, size_t fold2_sum, long long rank_foldh, long long foldh_holders,
                      unsigned *holders, uint32_t *order, uint8_t *block_planes, size_t *max_entries);
/* Named stages of the multi-kernel entry points (the sweeps of src/boundary.cpp:154-237, neighbours of
 * src/extend.cpp:248-289, the QC lists of PopPUNK/qc.py:330-354, long <-> square): when enabled, one hipEvent between
 * stages on the call's stream.  ppk_prof_stages_read writes "name<TAB>total ms<TAB>count" lines in first-seen order
 * (synchronises the recorded events); PPK_ERR_CAPACITY when buf is too small (what fits is written). */
int ppk_prof_stages_enable(int on);
int ppk_prof_stages_read(char *buf, size_t cap, int reset);

#ifdef __cplusplus
}
#endif
#endif /* PPK_H */
