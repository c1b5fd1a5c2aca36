// C-ABI entry points of libppk_hip.so (declared in include/ppk.h): errors, options, resident databases and the DEVICE
// entry points of kernels 1 and 2 (what is kept per device: ppk_devstate.hip).  The host-buffer entry points (what
// PopPUNK itself calls: worker threads, uploads, downloads, what is kept between calls) are in ppk_host.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <map>
#include <mutex>
#include <vector>

#include "ppk_internal.h"

// launcher defined in ppk_dist.hip
int ppk_launch_transpose(const uint64_t *d_in, uint64_t *d_out, size_t n, size_t cols, size_t npad,
                         hipStream_t s);

// ---- errors ---------------------------------------------------------------
static thread_local std::string g_err;
void ppk_set_error(const std::string &msg) { g_err = msg; }
const std::string &ppk_error() { return g_err; }
int ppk_fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
extern "C" const char *ppk_last_error(void) { return g_err.c_str(); }
#ifndef PPK_SRC_HASH
#define PPK_SRC_HASH "unhashed"
#endif
// "... src:<hash>": sha256 (16 hex digits) of the library's sources at build time (csrc/Makefile HASHED)
extern "C" const char *ppk_version(void) { return "poppunk_amd 0.5.0 (gfx950) src:" PPK_SRC_HASH; }

// ---- run-time options: PPK_* environment read once, then ppk_set_option only ------------------
namespace {
struct OptionEntry {
  const char *name, *env;
  std::atomic<long long> PpkConfig::*field;
};
const OptionEntry kOptions[] = {
#ifdef PPK_EXPERIMENTS
    // measured-and-rejected alternatives and the ablation mask: libppk_hip_exp.so only (make experiments)
    {"ablate", "PPK_ABLATE", &PpkConfig::ablate},
    {"map", "PPK_MAP", &PpkConfig::map},
    {"strip", "PPK_STRIP", &PpkConfig::strip},
    {"edge_list_keep", "PPK_EDGE_LIST_KEEP", &PpkConfig::edge_list_keep},
#endif
    {"rank_planes", "PPK_RANK_PLANES", &PpkConfig::rank_planes},
    {"rank_short", "PPK_RANK_SHORT", &PpkConfig::rank_short},
    {"rank_fold", "PPK_RANK_FOLD", &PpkConfig::rank_fold},
    {"rank_fold2", "PPK_RANK_FOLD2", &PpkConfig::rank_fold2},
    {"fold2_sort", "PPK_FOLD2_SORT", &PpkConfig::fold2_sort},
    {"fold2_min_planes", "PPK_FOLD2_MIN_PLANES", &PpkConfig::fold2_min_planes},
    {"rank_foldh", "PPK_RANK_FOLDH", &PpkConfig::rank_foldh},
    {"foldh_holders", "PPK_FOLDH_HOLDERS", &PpkConfig::foldh_holders},
    {"foldh_min_planes", "PPK_FOLDH_MIN_PLANES", &PpkConfig::foldh_min_planes},
    {"lds_table", "PPK_LDS_TABLE", &PpkConfig::lds_table},
    {"ksplit", "PPK_KSPLIT", &PpkConfig::ksplit},
    {"ksplit_slices", "PPK_KSPLIT_SLICES", &PpkConfig::ksplit_slices},
    {"wide_kpg", "PPK_WIDE_KPG", &PpkConfig::wide_kpg},
    {"ksplit_wide", "PPK_KSPLIT_WIDE", &PpkConfig::ksplit_wide},
    {"ksplit_long", "PPK_KSPLIT_LONG", &PpkConfig::ksplit_long},
    {"ksplit_fused", "PPK_KSPLIT_FUSED", &PpkConfig::ksplit_fused},
    {"chunk_rows", "PPK_CHUNK_ROWS", &PpkConfig::chunk_rows},
    {"prefault_threads", "PPK_PREFAULT_THREADS", &PpkConfig::prefault_threads},
    {"db_cache", "PPK_DB_CACHE", &PpkConfig::db_cache},
    {"progress", "PPK_PROGRESS", &PpkConfig::progress},
    {"launch_tiles", "PPK_LAUNCH_TILES", &PpkConfig::launch_tiles},
    {"knn_lane_lists", "PPK_KNN_LANE_LISTS", &PpkConfig::knn_lane_lists},
    {"ks_grid_pad", "PPK_KS_GRID_PAD", &PpkConfig::ks_grid_pad},
    {"ksplit_scratch_mb", "PPK_KSPLIT_SCRATCH_MB", &PpkConfig::ksplit_scratch_mb},
    {"pairs_scratch_mb", "PPK_PAIRS_SCRATCH_MB", &PpkConfig::pairs_scratch_mb},
    {"pairs_chunk", "PPK_PAIRS_CHUNK", &PpkConfig::pairs_chunk},
    {"edge_rows_fused", "PPK_EDGE_ROWS_FUSED", &PpkConfig::edge_rows_fused},
    {"silhouette_scratch_mb", "PPK_SILHOUETTE_SCRATCH_MB", &PpkConfig::silhouette_scratch_mb},
    {"silhouette_band", "PPK_SILHOUETTE_BAND", &PpkConfig::silhouette_band},
    {"silhouette_window", "PPK_SILHOUETTE_WINDOW", &PpkConfig::silhouette_window},
    {"rand_scratch_mb", "PPK_RAND_SCRATCH_MB", &PpkConfig::rand_scratch_mb},
    {"rand_batch", "PPK_RAND_BATCH", &PpkConfig::rand_batch},
    {"rand_wave_max", "PPK_RAND_WAVE_MAX", &PpkConfig::rand_wave_max},
    {"rand_window", "PPK_RAND_WINDOW", &PpkConfig::rand_window},
    {"lineage_scratch_mb", "PPK_LINEAGE_SCRATCH_MB", &PpkConfig::lineage_scratch_mb},
    {"lineage_lds_keys", "PPK_LINEAGE_LDS_KEYS", &PpkConfig::lineage_lds_keys},
    {"sketch_lds_bins", "PPK_SKETCH_LDS_BINS", &PpkConfig::sketch_lds_bins},
    {"sketch_batch_mb", "PPK_SKETCH_BATCH_MB", &PpkConfig::sketch_batch_mb},
    {"sketch_batch", "PPK_SKETCH_BATCH", &PpkConfig::sketch_batch},
    {"sketch_count_bits", "PPK_SKETCH_COUNT_BITS", &PpkConfig::sketch_count_bits},
    {"sketch_exact_rounds", "PPK_SKETCH_EXACT_ROUNDS", &PpkConfig::sketch_exact_rounds},
    {"refs_scratch_mb", "PPK_REFS_SCRATCH_MB", &PpkConfig::refs_scratch_mb},
    {"refs_lds_bits", "PPK_REFS_LDS_BITS", &PpkConfig::refs_lds_bits},
    {"knn_list", "PPK_KNN_LIST", &PpkConfig::knn_list},
    {"knn_warm", "PPK_KNN_WARM", &PpkConfig::knn_warm},
    {"knn_cut", "PPK_KNN_CUT", &PpkConfig::knn_cut},
    {"sweep_window", "PPK_SWEEP_WINDOW", &PpkConfig::sweep_window},
    {"net_window", "PPK_NET_WINDOW", &PpkConfig::net_window},
    {"bt_lds_max", "PPK_BT_LDS_MAX", &PpkConfig::bt_lds_max},
    {"bt_small_max", "PPK_BT_SMALL_MAX", &PpkConfig::bt_small_max},
    {"dbscan_search", "PPK_DBSCAN_SEARCH", &PpkConfig::dbscan_search},
    {"refine_local", "PPK_REFINE_LOCAL", &PpkConfig::refine_local},
    {"density_hot_table", "PPK_DENSITY_HOT_TABLE", &PpkConfig::density_hot_table},
    {"density_kde_presum", "PPK_DENSITY_KDE_PRESUM", &PpkConfig::density_kde_presum},
    {"host_parts", "PPK_HOST_PARTS", &PpkConfig::host_parts},
    {"host_parts_rows", "PPK_HOST_PARTS_ROWS", &PpkConfig::host_parts_rows},
    {"host_trace", "PPK_HOST_TRACE", &PpkConfig::host_trace},
    {"ext_collision_adjust", "PPK_EXT_COLLISION_ADJUST", &PpkConfig::ext_collision_adjust},
    {"ext_fit_skip", "PPK_EXT_FIT_SKIP", &PpkConfig::ext_fit_skip},
};
}  // namespace

PpkConfig &ppk_config() {
  static PpkConfig cfg;
  static std::once_flag once;
  std::call_once(once, []() {
    for (const OptionEntry &o : kOptions)
      if (const char *e = getenv(o.env))
        if (*e) (cfg.*(o.field)).store(atoll(e));
  });
  return cfg;
}

extern "C" int ppk_set_option(const char *name, long long value) {
  if (!name) return ppk_fail(PPK_ERR_ARG, "option name is NULL");
  for (const OptionEntry &o : kOptions)
    if (!strcmp(name, o.name)) {
      (ppk_config().*(o.field)).store(value);
      return PPK_OK;
    }
  return ppk_fail(PPK_ERR_ARG, std::string("unknown option: ") + name);
}

extern "C" int ppk_get_option(const char *name, long long *value) {
  if (!name || !value) return ppk_fail(PPK_ERR_ARG, "option name / value is NULL");
  for (const OptionEntry &o : kOptions)
    if (!strcmp(name, o.name)) {
      *value = (ppk_config().*(o.field)).load();
      return PPK_OK;
    }
  return ppk_fail(PPK_ERR_ARG, std::string("unknown option: ") + name);
}

extern "C" int ppk_device_count(int *n) {
  if (!n) return ppk_fail(PPK_ERR_ARG, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return ppk_fail(PPK_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *n = c;
  return PPK_OK;
}

// ---- profiling hooks ---------------------------------------------------------
namespace {
struct Prof {
  std::mutex mu;
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  hipEvent_t cur_start = nullptr;
  double total_ms = 0.0;
  long long launches = 0;
  std::string kernel_name;
} g_prof;

void prof_fold_locked() {
  for (auto &pr : g_prof.pending) {
    float ms = 0.0f;
    if (hipEventSynchronize(pr.second) == hipSuccess &&
        hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
      g_prof.total_ms += ms;
      g_prof.launches += 1;
    }
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  g_prof.pending.clear();
}
}  // namespace

void ppk_set_kernel_name(const char *name) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.kernel_name = name;
}

void ppk_prof_begin(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (!g_prof.on) return;
  if (g_prof.pending.size() >= 512) prof_fold_locked();
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_prof.cur_start = e;
}

void ppk_prof_end(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (!g_prof.on || !g_prof.cur_start) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_prof.pending.emplace_back(g_prof.cur_start, e);
  g_prof.cur_start = nullptr;
}

extern "C" int ppk_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = on != 0;
  return PPK_OK;
}

// ---- named stages (the multi-kernel entry points: sweeps, neighbours, QC lists, long <-> square) ----
// ppk_prof_stage(name, s) records ONE event on s: it ends the stage before it and starts `name`
// (nullptr: only ends).  Nothing is recorded unless ppk_prof_stages_enable(1).
namespace {
struct StageProf {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> ev;          // ev[i] .. ev[i + 1] brackets stage nm[i] ("" = not a stage)
  std::vector<std::string> nm;
  std::vector<std::string> order;      // first-seen order of the names
  std::map<std::string, std::pair<double, long long>> acc;
} g_stage;

void stage_fold_locked() {
  for (size_t i = 0; i + 1 < g_stage.ev.size(); ++i) {
    if (g_stage.nm[i].empty()) continue;
    float ms = 0.0f;
    if (hipEventSynchronize(g_stage.ev[i + 1]) == hipSuccess &&
        hipEventElapsedTime(&ms, g_stage.ev[i], g_stage.ev[i + 1]) == hipSuccess) {
      auto it = g_stage.acc.find(g_stage.nm[i]);
      if (it == g_stage.acc.end()) {
        g_stage.order.push_back(g_stage.nm[i]);
        it = g_stage.acc.emplace(g_stage.nm[i], std::make_pair(0.0, 0LL)).first;
      }
      it->second.first += ms;
      it->second.second += 1;
    }
  }
  // the last event may still open a stage: keep it
  const bool open = !g_stage.nm.empty() && !g_stage.nm.back().empty();
  const size_t keep = open ? g_stage.ev.size() - 1 : g_stage.ev.size();
  for (size_t i = 0; i < keep; ++i) (void)hipEventDestroy(g_stage.ev[i]);
  if (open) {
    hipEvent_t e = g_stage.ev.back();
    std::string n = g_stage.nm.back();
    g_stage.ev.assign(1, e);
    g_stage.nm.assign(1, n);
  } else {
    g_stage.ev.clear();
    g_stage.nm.clear();
  }
}
}  // namespace

void ppk_prof_stage(const char *name, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_stage.mu);
  if (!g_stage.on) return;
  if (g_stage.ev.size() >= 1024) stage_fold_locked();
  if (!name && (g_stage.nm.empty() || g_stage.nm.back().empty())) return;      // nothing open
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_stage.ev.push_back(e);
  g_stage.nm.push_back(name ? name : "");
}

extern "C" int ppk_prof_stages_enable(int on) {
  std::lock_guard<std::mutex> lk(g_stage.mu);
  g_stage.on = on != 0;
  return PPK_OK;
}

extern "C" int ppk_prof_stages_read(char *buf, size_t cap, int reset) {
  std::lock_guard<std::mutex> lk(g_stage.mu);
  stage_fold_locked();
  std::string out;
  for (const std::string &n : g_stage.order) {
    const auto &a = g_stage.acc[n];
    char line[256];
    snprintf(line, sizeof line, "%s\t%.6f\t%lld\n", n.c_str(), a.first, a.second);
    out += line;
  }
  if (buf && cap) {
    const size_t k = out.size() < cap - 1 ? out.size() : cap - 1;
    memcpy(buf, out.data(), k);
    buf[k] = 0;
  }
  if (reset) {
    g_stage.acc.clear();
    g_stage.order.clear();
  }
  return out.size() + 1 > cap && buf ? ppk_fail(PPK_ERR_CAPACITY, "stage table does not fit the buffer") : (int)PPK_OK;
}

extern "C" int ppk_prof_read(double *total_ms, long long *n_launches, int reset) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  prof_fold_locked();
  if (total_ms) *total_ms = g_prof.total_ms;
  if (n_launches) *n_launches = g_prof.launches;
  if (reset) {
    g_prof.total_ms = 0.0;
    g_prof.launches = 0;
  }
  return PPK_OK;
}

extern "C" const char *ppk_last_kernel_name(void) {
  static thread_local std::string copy;
  std::lock_guard<std::mutex> lk(g_prof.mu);
  copy = g_prof.kernel_name;
  return copy.c_str();
}

// ---- geometry helpers -----------------------------------------------------------
static inline size_t row_start_self(size_t q, size_t n) { return q * n - (q * (q + 1)) / 2; }

extern "C" size_t ppk_rows_in_band(size_t n_ref, size_t n_qry, size_t q_begin, size_t q_end) {
  if (q_end <= q_begin) return 0;
  if (n_qry == 0) {
    if (q_end > n_ref) q_end = n_ref;
    if (q_begin >= q_end) return 0;
    return row_start_self(q_end, n_ref) - row_start_self(q_begin, n_ref);
  }
  if (q_end > n_qry) q_end = n_qry;
  if (q_begin >= q_end) return 0;
  return (q_end - q_begin) * n_ref;
}

extern "C" int ppk_band_split(size_t n_ref, size_t n_qry, int n_parts, size_t *bounds) {
  if (n_parts < 1 || !bounds) return ppk_fail(PPK_ERR_ARG, "bad band split arguments");
  const size_t nq = n_qry ? n_qry : n_ref;
  const size_t total = ppk_rows_in_band(n_ref, n_qry, 0, nq);
  bounds[0] = 0;
  for (int p = 1; p < n_parts; ++p) {
    const double target = (double)total * (double)p / (double)n_parts;
    size_t q;
    if (n_qry == 0) {
      // rows before q: q*n - q(q+1)/2 = target  ->  q = ((2n-1) - sqrt((2n-1)^2 - 8 target)) / 2
      const double b = 2.0 * (double)n_ref - 1.0;
      const double disc = b * b - 8.0 * target;
      q = (size_t)((b - std::sqrt(disc > 0 ? disc : 0.0)) / 2.0);
    } else {
      q = (size_t)(target / (double)n_ref);
    }
    q = (q + 32) / 64 * 64;  // band edges on 64-query tile boundaries
    if (q > nq) q = nq;
    if (q < bounds[p - 1]) q = bounds[p - 1];
    bounds[p] = q;
  }
  bounds[n_parts] = nq;
  return PPK_OK;
}

// ---- resident sketch database --------------------------------------------------
extern "C" int ppk_db_create(int device_id, const uint64_t *sk, size_t n, size_t nk,
                             size_t sketchsize64, size_t bbits, const uint16_t *clu,
                             int src_on_device, void *stream, ppk_db **out) {
  if (!out) return ppk_fail(PPK_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!sk || n == 0 || nk == 0 || sketchsize64 == 0 || bbits == 0 || bbits > 64)
    return ppk_fail(PPK_ERR_ARG, "ppk_db_create: empty or invalid sketch dimensions");
  if (sketchsize64 * 64 >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, "ppk_db_create: sketch too large");
  if (n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_db_create: too many samples (sample indices are 32-bit)");
  PPK_ENTER_DEVICE(guard, device_id);
  if (int rc_arch = ppk_check_arch(device_id)) return rc_arch;
  hipStream_t s = static_cast<hipStream_t>(stream);

  ppk_db *db = new ppk_db();
  db->device = device_id;
  db->n = n;
  db->npad = (n + PPK_NPAD - 1) / PPK_NPAD * PPK_NPAD;
  db->nk = nk;
  db->s64 = sketchsize64;
  db->bbits = bbits;
  db->words = sketchsize64 * bbits;
  const size_t cols = nk * db->words;
  const size_t in_bytes = n * cols * sizeof(uint64_t);
  const size_t out_bytes = db->npad * cols * sizeof(uint64_t);

  auto bail = [&](int code, const std::string &msg) {
    ppk_db_destroy(db);
    return ppk_fail(code, msg);
  };
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&db->d_skT), out_bytes);
  if (e != hipSuccess) return bail(PPK_ERR_HIP, std::string("hipMalloc(sketches): ") + hipGetErrorString(e));

  const uint64_t *d_in = sk;
  uint64_t *d_stage = nullptr;
  if (!src_on_device) {
    e = hipMalloc(reinterpret_cast<void **>(&d_stage), in_bytes);
    if (e != hipSuccess) return bail(PPK_ERR_HIP, std::string("hipMalloc(stage): ") + hipGetErrorString(e));
    if (ppk_upload(device_id, d_stage, sk, in_bytes, s) != PPK_OK) {
      const std::string why = g_err;
      (void)hipFree(d_stage);
      return bail(PPK_ERR_HIP, "upload of the sketches: " + why);
    }
    d_in = d_stage;
  }
  int rc = ppk_launch_transpose(d_in, db->d_skT, n, cols, db->npad, s);
  if (rc == PPK_OK && clu) {
    e = hipMalloc(reinterpret_cast<void **>(&db->d_clu), db->npad * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemsetAsync(db->d_clu, 0, db->npad * sizeof(uint16_t), s);
    if (e == hipSuccess && src_on_device)
      e = hipMemcpyAsync(db->d_clu, clu, n * sizeof(uint16_t), hipMemcpyDeviceToDevice, s);
    else if (e == hipSuccess && ppk_upload(device_id, db->d_clu, clu, n * sizeof(uint16_t), s) != PPK_OK)
      e = hipErrorUnknown;
    if (e != hipSuccess) rc = PPK_ERR_HIP;
  }
  // the coded copies of a self job that runs whole tiles (ppk_coding.hip): the count pass, the choice, the copies
  if (rc == PPK_OK) rc = ppk_db_build_codings(db, s);
  // the staging copy must outlive the transpose; the host-source path blocks here
  if (d_stage) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_stage);
  }
  if (rc != PPK_OK) return bail(rc, std::string("ppk_db_create failed: ") + g_err);
  *out = db;
  return PPK_OK;
}

extern "C" void ppk_db_destroy(ppk_db *db) {
  if (!db) return;
  DeviceGuard guard(db->device);
  if (db->d_skT) (void)hipFree(db->d_skT);
  for (PpkCoding &c : db->coding) ppk_coding_free(c);
  if (db->d_clu) (void)hipFree(db->d_clu);
  delete db;
}

extern "C" size_t ppk_db_size(const ppk_db *db) { return db ? db->n : 0; }

// ---- kernel 1, device entry points -------------------------------------------------
int ppk_check_pair(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, size_t q_begin,
                   size_t q_end) {
  if (!ref || !kmers) return ppk_fail(PPK_ERR_ARG, "ref database / kmers missing");
  if (int rc = ppk_check_device(ref->device)) return rc;
  if (qry) {
    if (qry->device != ref->device) return ppk_fail(PPK_ERR_ARG, "ref and query databases on different devices");
    if (qry->nk != ref->nk || qry->s64 != ref->s64 || qry->bbits != ref->bbits)
      return ppk_fail(PPK_ERR_ARG, "ref and query sketches have different k-mer lists or sketch sizes");
  }
  const size_t nq = qry ? qry->n : ref->n;
  if (q_begin > q_end || q_end > nq) return ppk_fail(PPK_ERR_ARG, "query band out of range");
  return PPK_OK;
}

namespace {
// random table (host) -> device copy placed after the LUT in the LUT scratch.  *lut_ready: the
// tables of an identical earlier call (same k list, random table, sketch size, options) are still
// there -- the launcher then skips lut_kernel (one launch and one H2D copy less per call: what a
// 1 000-genome query or a plot-fit re-query mostly consists of).
int stage_tables(const ppk_db *ref, const int32_t *kmers, const float *random_tbl, size_t n_clu, int flags,
                 hipStream_t s, double **d_lut, float **d_rtab, bool *lut_ready) {
  const size_t nbins = ref->s64 * 64;
  const size_t C = n_clu ? n_clu : 1;
  // log-J table + the (E, F) pairs of the fit's fast path behind it (ppk_dist.hip lut_kernel)
  const size_t lut_bytes = 3 * C * C * ref->nk * (nbins + 1) * sizeof(double);
  const size_t tab_bytes = C * C * ref->nk * sizeof(float);
  const bool use_tbl = (flags & PPK_FLAG_RANDOM_CORRECT) && random_tbl;
  void *base = nullptr;
  int rc = ppk_scratch_get(ref->device, SLOT_LUT, lut_bytes + tab_bytes + 256, &base);
  if (rc != PPK_OK) return rc;
  *d_lut = static_cast<double *>(base);
  float *t = reinterpret_cast<float *>(static_cast<char *>(base) + ((lut_bytes + 255) / 256) * 256);
  *d_rtab = use_tbl ? t : nullptr;
  const long long dims[8] = {(long long)ref->nk, (long long)ref->s64, (long long)ref->bbits, (long long)C,
                             use_tbl ? 1 : 0, ppk_config().ext_collision_adjust.load(), 0, 0};
  uint64_t key = ppk_token(dims, sizeof(dims), 21);
  key = ppk_token(kmers, ref->nk * sizeof(int32_t), key);
  if (use_tbl) key = ppk_token(random_tbl, tab_bytes, key);
  *lut_ready = ppk_lut_ready(ref->device, key, base);
  if (!*lut_ready && use_tbl) PPK_HIP(hipMemcpyAsync(t, random_tbl, tab_bytes, hipMemcpyHostToDevice, s));
  return PPK_OK;
}

}  // namespace

bool ppk_read_edge(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off, size_t k,
                   long long *i, long long *j, long long *o) {
  if (o) *o = 0;
  return hipMemcpy(i, d_i + k * stride, 8, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(j, d_j + k * stride, 8, hipMemcpyDeviceToHost) == hipSuccess &&
         (!d_off || hipMemcpy(o, d_off + k, 8, hipMemcpyDeviceToHost) == hipSuccess);
}

// ---- one result matrix, N processes (ppk.h) -----------------------------------------------------------
static_assert(sizeof(hipIpcMemHandle_t) == PPK_WINDOW_HANDLE_BYTES, "hipIpcMemHandle_t is not 64 bytes");

extern "C" int ppk_window_alloc(int device, size_t bytes, void **d_window) {
  if (!d_window || bytes == 0) return ppk_fail(PPK_ERR_ARG, "window: no size / no output pointer");
  PPK_ENTER_DEVICE(g, device);
  // FINE-GRAINED device memory: peers store into it over xGMI while the owner's kernels read it later.  Those stores
  // arrive at the owner's memory side, not through its L2s; with a plain (coarse-grained) allocation a line of the
  // window that an earlier kernel of the owner left in one of its eight L2s could be served stale afterwards -- only
  // a stream synchronisation and a barrier separate a peer's store from the owner's read, and neither invalidates
  // anything.  Fine-grained memory is kept coherent at system scope by the hardware (the owner's accesses are
  // write-through / re-validated), so visibility does not rest on when a cache happens to be flushed.  (Round-4
  // advisor finding; the window has so far only run with both ranks on ONE GPU)
  void *p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return ppk_fail(PPK_ERR_HIP, std::string("hipExtMallocWithFlags(window, fine-grained): ") + hipGetErrorString(e));
  }
  *d_window = p;
  return PPK_OK;
}

extern "C" int ppk_window_free(int device, void *d_window) {
  if (!d_window) return PPK_OK;
  PPK_ENTER_DEVICE(g, device);
  (void)hipDeviceSynchronize();
  PPK_HIP(hipFree(d_window));
  return PPK_OK;
}

extern "C" int ppk_window_export(int device, const void *d_window, unsigned char handle[PPK_WINDOW_HANDLE_BYTES]) {
  if (!d_window || !handle) return ppk_fail(PPK_ERR_ARG, "window: null argument");
  PPK_ENTER_DEVICE(g, device);
  hipIpcMemHandle_t h;
  hipError_t e = hipIpcGetMemHandle(&h, const_cast<void *>(d_window));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return ppk_fail(PPK_ERR_HIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e));
  }
  memcpy(handle, &h, sizeof(h));
  return PPK_OK;
}

extern "C" int ppk_window_open(int device, const unsigned char handle[PPK_WINDOW_HANDLE_BYTES], void **d_window) {
  if (!d_window || !handle) return ppk_fail(PPK_ERR_ARG, "window: null argument");
  PPK_ENTER_DEVICE(g, device);
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  void *p = nullptr;
  hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess || !p) {
    (void)hipGetLastError();
    return ppk_fail(PPK_ERR_HIP, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
  }
  *d_window = p;
  return PPK_OK;
}

extern "C" int ppk_window_close(int device, void *d_window) {
  if (!d_window) return PPK_OK;
  PPK_ENTER_DEVICE(g, device);
  (void)hipDeviceSynchronize();
  hipError_t e = hipIpcCloseMemHandle(d_window);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return ppk_fail(PPK_ERR_HIP, std::string("hipIpcCloseMemHandle: ") + hipGetErrorString(e));
  }
  return PPK_OK;
}

extern "C" int ppk_dist_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                            const float *random_tbl, size_t n_clu, int flags, size_t q_begin,
                            size_t q_end, void *d_out, unsigned long long *d_n_failed,
                            void *stream) {
  int rc = ppk_check_pair(ref, qry, kmers, q_begin, q_end);
  if (rc != PPK_OK) return rc;
  // an empty band (also: the last self row, which pairs with nothing) is a no-op
  if (ppk_rows_in_band(ref->n, qry ? qry->n : 0, q_begin, q_end) == 0) return PPK_OK;
  if (!d_out) return ppk_fail(PPK_ERR_ARG, "d_out is NULL");
  DeviceGuard guard(ref->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PpkCall call(ref->device, s);
  double *d_lut = nullptr;
  float *d_rtab = nullptr;
  bool lut_ready = false;
  rc = stage_tables(ref, kmers, random_tbl, n_clu, flags, s, &d_lut, &d_rtab, &lut_ready);
  if (rc != PPK_OK) return rc;
  DistJob job;
  job.ref = ref, job.qry = qry, job.kmers = kmers, job.d_rtab = d_rtab, job.n_clu = d_rtab ? n_clu : 1, job.flags = flags;
  job.q_begin = q_begin, job.q_end = q_end, job.d_out = d_out, job.d_n_failed = d_n_failed;
  job.d_lut = d_lut, job.lut_ready = lut_ready, job.s = s;
  return ppk_launch_dist(job);
}

extern "C" int ppk_dist_pairs_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl,
                                  size_t n_clu, int flags, const long long *d_i, const long long *d_j, size_t stride,
                                  size_t n_pairs, long long int_offset, void *d_out, unsigned long long *d_n_failed,
                                  void *stream) {
  int rc = ppk_check_pair(ref, qry, kmers, 0, 0);
  if (rc != PPK_OK) return rc;
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: stride must be 1 or 2");
  if (n_pairs == 0) return PPK_OK;
  if (!d_i || !d_j || !d_out) return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: NULL array");
  if (n_pairs >= ((size_t)1 << 40)) return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: n_pairs must be < 2^40");
  PPK_ENTER_DEVICE(guard, ref->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PpkCall call(ref->device, s);
  PairsJob job;
  float *d_rtab = nullptr;
  rc = stage_tables(ref, kmers, random_tbl, n_clu, flags, s, &job.d_lut, &d_rtab, &job.lut_ready);
  if (rc != PPK_OK) return rc;
  job.d_rtab = d_rtab;
  job.ref = ref, job.qry = qry, job.kmers = kmers, job.n_clu = job.d_rtab ? n_clu : 1, job.flags = flags;
  job.d_i = d_i, job.d_j = d_j, job.stride = stride, job.n_pairs = n_pairs, job.int_offset = int_offset;
  job.d_out = d_out, job.d_n_failed = d_n_failed, job.s = s;
  return ppk_launch_pairs(job);
}

extern "C" int ppk_dist_pairs(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl,
                              size_t n_clu, int flags, const long long *i, const long long *j, size_t n_pairs,
                              long long int_offset, void *out, unsigned long long *n_failed) {
  if (!ref) return ppk_fail(PPK_ERR_ARG, "ref database / kmers missing");
  if (n_failed) *n_failed = 0;
  if (n_pairs && (!i || !j || !out)) return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: NULL array");
  const size_t row_words = (flags & (PPK_FLAG_COUNTS | PPK_FLAG_JACCARD)) ? ref->nk : 2;
  long long *d_i, *d_j;
  uint32_t *d_out;
  unsigned long long *d_nf;
  return ppk_host_frame(ref->device, [&](Carve &c) {
    c.take(d_i, n_pairs).take(d_j, n_pairs).take(d_out, n_pairs * row_words).take(d_nf, 1);
  }, [&]() -> int {
    if (n_pairs) {
      PPK_HIP(hipMemcpy(d_i, i, n_pairs * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_pairs * 8, hipMemcpyHostToDevice));
    }
    PPK_HIP(hipMemset(d_nf, 0, 8));
    const int rc = ppk_dist_pairs_dev(ref, qry, kmers, random_tbl, n_clu, flags, d_i, d_j, 1, n_pairs, int_offset, d_out,
                                      d_nf, nullptr);
    if (rc != PPK_OK) return rc;
    if (n_pairs) PPK_HIP(hipMemcpy(out, d_out, n_pairs * row_words * 4, hipMemcpyDeviceToHost));
    if (n_failed) PPK_HIP(hipMemcpy(n_failed, d_nf, 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// The two-step of the edge calls with rows: the unscaled rows of the first min(*d_n_edges, cap) edges of a finished edge
// call, through the list kernel (one read-back of the count; failures were counted by the edge call)
static int rows_of_edges(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl, size_t n_clu,
                         int flags, const long long *d_edges, size_t cap, const unsigned long long *d_n_edges, float *d_rows,
                         hipStream_t s) {
  const unsigned long long *h = nullptr;
  int rc = ppk_read_back(ref->device, s, {{d_n_edges, 8}}, &h);
  if (rc != PPK_OK) return rc;
  const size_t n = h[0] < cap ? (size_t)h[0] : cap;
  if (n == 0) return PPK_OK;
  if (n >= ((size_t)1 << 40)) return ppk_fail(PPK_ERR_ARG, "edge rows: the list kernel takes fewer than 2^40 pairs");
  PairsJob job;
  float *d_rtab = nullptr;
  rc = stage_tables(ref, kmers, random_tbl, n_clu, flags, s, &job.d_lut, &d_rtab, &job.lut_ready);
  if (rc != PPK_OK) return rc;
  job.d_rtab = d_rtab;
  job.ref = ref, job.qry = qry, job.kmers = kmers, job.n_clu = d_rtab ? n_clu : 1, job.flags = flags;
  job.d_i = d_edges, job.d_j = d_edges + 1, job.stride = 2, job.n_pairs = n, job.int_offset = 0;
  job.d_out = d_rows, job.d_n_failed = nullptr, job.s = s;
  rc = ppk_launch_pairs(job);
  if (rc != PPK_OK) return rc;
  ppk_set_kernel_name((std::string(ppk_last_kernel_name()) + " + pairs list").c_str());
  return PPK_OK;
}

// The fused edge list of a band: the line boundary (model == NULL) or the label test of a BGMM model.  want_rows: the
// unscaled (core, accessory) row of every edge into d_rows as well -- from the tile kernel's rows modes where
// ppk_edge_rows_fused says so, else by the two-step (rows_of_edges); the same bits either way.
static int dist_edges_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers, const float *random_tbl,
                          size_t n_clu, int flags, size_t q_begin, size_t q_end, int slope, float x_max, float y_max,
                          float scale_x, float scale_y, int inclusive, const ppk_bgmm *model, long long *d_edges,
                          float *d_rows, bool want_rows, size_t cap, unsigned long long *d_n_edges,
                          unsigned long long *d_n_failed, void *stream) {
  int rc = ppk_check_pair(ref, qry, kmers, q_begin, q_end);
  if (rc != PPK_OK) return rc;
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  if (want_rows && !d_rows) return ppk_fail(PPK_ERR_ARG, "d_rows is NULL");
  if (slope < 0 || slope > 2) return ppk_fail(PPK_ERR_ARG, "slope must be 0, 1 or 2");
  if (flags & (PPK_FLAG_JACCARD | PPK_FLAG_COUNTS))
    return ppk_fail(PPK_ERR_ARG, "edge output excludes the jaccard/counts flags");
  DeviceGuard guard(ref->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PpkCall call(ref->device, s);
  if (q_begin == q_end) {
    PPK_HIP(hipMemsetAsync(d_n_edges, 0, sizeof(unsigned long long), s));
    return PPK_OK;
  }
  double *d_lut = nullptr;
  float *d_rtab = nullptr;
  bool lut_ready = false;
  rc = stage_tables(ref, kmers, random_tbl, n_clu, flags, s, &d_lut, &d_rtab, &lut_ready);
  if (rc != PPK_OK) return rc;
  DistJob job;
  job.ref = ref, job.qry = qry, job.kmers = kmers, job.d_rtab = d_rtab, job.n_clu = d_rtab ? n_clu : 1, job.flags = flags;
  job.d_n_failed = d_n_failed, job.d_lut = d_lut, job.s = s;
  job.slope = slope, job.x_max = x_max, job.y_max = y_max, job.scale_x = scale_x, job.scale_y = scale_y, job.inclusive = inclusive;
  {
    // sketches the tile kernels cannot fit (ppk_unfused: bbits other than 14 with more than 128 count bits --
    // nothing PopPUNK writes): distances (pre-divided by scale) go to scratch and the row-linear edge kernel
    // runs on them, whole matrices only
    if (ppk_unfused(ref)) {
      const size_t nq = qry ? qry->n : ref->n;
      if (q_begin != 0 || q_end != nq)
        return ppk_fail(PPK_ERR_ARG, "edge lists of a band need bbits = 14 or nk * count bits <= 128");
      const size_t rows = ppk_rows_in_band(ref->n, qry ? qry->n : 0, 0, nq);
      void *d_dist = nullptr;
      rc = ppk_scratch_get(ref->device, SLOT_ITER_B, rows * 8 + 8, &d_dist);
      if (rc != PPK_OK) return rc;
      job.q_begin = 0, job.q_end = nq, job.d_out = d_dist;
      rc = ppk_launch_dist(job);
      if (rc != PPK_OK) return rc;
      RowTest t = {};
      t.kind = model ? RowTest::BGMM : RowTest::LINE;
      if (model) t.bgmm = *model;
      t.slope = slope, t.inclusive = inclusive, t.x_max = x_max, t.y_max = y_max;
      rc = ppk_row_edges(d_dist, rows, qry ? ref->n : 0, 0, t, d_edges, cap, d_n_edges, s);
      if (rc != PPK_OK || !want_rows) return rc;
      return rows_of_edges(ref, qry, kmers, random_tbl, n_clu, flags, d_edges, cap, d_n_edges, d_rows, s);
    }
  }
  const bool fused_rows = want_rows && ppk_edge_rows_fused(ref, qry, q_begin, q_end);
  const size_t n_rtiles = (ref->n + 63) / 64;
  const size_t n_words = (q_end - q_begin) * n_rtiles;
  void *d_mask = nullptr, *d_ws = nullptr;
  rc = ppk_scratch_get(ref->device, SLOT_MASK, n_words * sizeof(uint64_t), &d_mask);
  if (rc != PPK_OK) return rc;
  rc = ppk_scratch_get(ref->device, SLOT_WS, ppk_compact_ws_bytes(n_words), &d_ws);
  if (rc != PPK_OK) return rc;
  const ppk_bgmm *d_model = nullptr;
  if (model && (rc = ppk_bgmm_to_device(ref->device, *model, &d_model, s)) != PPK_OK) return rc;
  PPK_HIP(hipMemsetAsync(d_mask, 0, n_words * sizeof(uint64_t), s));
  job.q_begin = q_begin, job.q_end = q_end, job.d_mask = static_cast<uint64_t *>(d_mask);
  job.lut_ready = lut_ready, job.d_bgmm = d_model;
  // the rows modes' scratch: 8 bytes per mask word (where a word's first row is staged) and 8 bytes per edge of the
  // caller's cap (the staged rows), behind the reservation counter
  unsigned long long *d_rows_count = nullptr, *d_word_base = nullptr;
  float2 *d_stage = nullptr;
  if (fused_rows) {
    rc = ppk_scratch_carve(ref->device, SLOT_EDGE_ROWS, [&](Carve &c) {
      c.take(d_rows_count, 1).take(d_word_base, n_words).take(d_stage, cap ? cap : 1);
    });
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemsetAsync(d_rows_count, 0, sizeof(unsigned long long), s));
    job.d_rows_stage = d_stage, job.d_rows_base = d_word_base, job.d_rows_count = d_rows_count, job.rows_cap = cap;
  }
  rc = ppk_launch_dist(job);
  if (rc != PPK_OK) return rc;
  EdgeGeom g = {};
  g.layout = qry ? EDGE_TILED_NONSELF : EDGE_TILED_SELF;
  g.n_ref = ref->n;
  g.q_begin = q_begin;
  g.n_rtiles = n_rtiles;
  g.int_offset = 0;
  if (fused_rows)
    return ppk_launch_compact_rows(static_cast<const uint64_t *>(d_mask), n_words, g, d_ws, d_edges, cap, d_n_edges, d_stage,
                                   d_word_base, cap, d_rows, s);
  rc = ppk_launch_compact(static_cast<const uint64_t *>(d_mask), n_words, g, d_ws, d_edges, cap, d_n_edges, s);
  if (rc != PPK_OK || !want_rows) return rc;
  return rows_of_edges(ref, qry, kmers, random_tbl, n_clu, flags, d_edges, cap, d_n_edges, d_rows, s);
}

extern "C" int ppk_dist_edges_rows_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                       const float *random_tbl, size_t n_clu, int flags, size_t q_begin,
                                       size_t q_end, int slope, float x_max, float y_max, float scale_x,
                                       float scale_y, int inclusive, long long *d_edges, float *d_rows, size_t cap,
                                       unsigned long long *d_n_edges, unsigned long long *d_n_failed,
                                       void *stream) {
  return dist_edges_dev(ref, qry, kmers, random_tbl, n_clu, flags, q_begin, q_end, slope, x_max, y_max, scale_x,
                        scale_y, inclusive, nullptr, d_edges, d_rows, true, cap, d_n_edges, d_n_failed, stream);
}

extern "C" int ppk_dist_edges_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                  const float *random_tbl, size_t n_clu, int flags, size_t q_begin,
                                  size_t q_end, int slope, float x_max, float y_max, float scale_x,
                                  float scale_y, int inclusive, long long *d_edges, size_t cap,
                                  unsigned long long *d_n_edges, unsigned long long *d_n_failed,
                                  void *stream) {
  return dist_edges_dev(ref, qry, kmers, random_tbl, n_clu, flags, q_begin, q_end, slope, x_max, y_max, scale_x,
                        scale_y, inclusive, nullptr, d_edges, nullptr, false, cap, d_n_edges, d_n_failed, stream);
}

static int check_bgmm(const ppk_bgmm *model) {
  if (!model) return ppk_fail(PPK_ERR_ARG, "model is NULL");
  if (model->K < 1 || model->K > PPK_BGMM_MAX_K || model->within_label < 0 || model->within_label >= model->K)
    return ppk_fail(PPK_ERR_ARG, "the BGMM model is not prepared (ppk_bgmm_prepare)");
  return PPK_OK;
}

extern "C" int ppk_dist_bgmm_edges_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                       const float *random_tbl, size_t n_clu, int flags, size_t q_begin,
                                       size_t q_end, const ppk_bgmm *model, long long *d_edges, size_t cap,
                                       unsigned long long *d_n_edges, unsigned long long *d_n_failed,
                                       void *stream) {
  if (int rc = check_bgmm(model)) return rc;
  return dist_edges_dev(ref, qry, kmers, random_tbl, n_clu, flags, q_begin, q_end, 2, 0.f, 0.f, 1.f, 1.f, 0, model,
                        d_edges, nullptr, false, cap, d_n_edges, d_n_failed, stream);
}

extern "C" int ppk_dist_bgmm_edges_rows_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                            const float *random_tbl, size_t n_clu, int flags, size_t q_begin,
                                            size_t q_end, const ppk_bgmm *model, long long *d_edges, float *d_rows,
                                            size_t cap, unsigned long long *d_n_edges, unsigned long long *d_n_failed,
                                            void *stream) {
  if (int rc = check_bgmm(model)) return rc;
  return dist_edges_dev(ref, qry, kmers, random_tbl, n_clu, flags, q_begin, q_end, 2, 0.f, 0.f, 1.f, 1.f, 0, model,
                        d_edges, d_rows, true, cap, d_n_edges, d_n_failed, stream);
}

// k nearest neighbours of every sample straight from the resident sketches: kernel 1's tiles emit
// neighbour candidates under per-sample bounds (ppk_dist.hip MODE_KNN), a sort by sample and a per-sample
// selection finish (ppk_square.hip).  The upper triangle is compared ONCE and neither the n x n matrix
// nor the [n_pairs, 2] matrix ever exists: memory is the sketches + a few dozen candidates per sample.
// [q_begin, q_end): the band of the triangle's rows this call compares -- a pair belongs to the band of its
// smaller sample and is a candidate for both of its samples, so the per-sample lists of several bands (several
// devices) merge into the whole job's.  missing_j: what an unfilled slot gets as j (0: the reference's filler;
// -1: a mark the merge can see).
// qry (nullable): a ref x query job -- the samples are the n_ref refs followed by the n_qry queries (sample
// n_ref + q), every ref's neighbours are queries and every query's are refs; outputs hold (n_ref + n_qry) * knn.

// A device word read back without draining the stream: a one-thread kernel copies it into a pinned block and leaves
// the caller's ticket behind it; the host polls the ticket (a blocking synchronisation on torch's current stream
// returned ~28 us after the work had ended: the sweeps, profiles/NOTES_r06.md section 6), for at most ~5 ms -- a piece of
// a large neighbour job runs longer --, then waits for the stream as before.
namespace {
struct PinnedWord {
  unsigned long long value, ticket;
};
__global__ void publish_word_kernel(const unsigned long long *__restrict__ src, PinnedWord *__restrict__ dst,
                                    unsigned long long ticket) {
  dst->value = *src;
  __threadfence_system();
  __hip_atomic_store(&dst->ticket, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int read_device_word(int dev, const unsigned long long *d_word, unsigned long long *out, hipStream_t s) {
  PinnedWord *b = static_cast<PinnedWord *>(ppk_ticket_block(dev, PPK_TICKET_KNN_COUNT));
  if (!b) return ppk_fail(PPK_ERR_HIP, "hipHostMalloc failed");
  const unsigned long long ticket = ppk_next_ticket(dev);
  hipLaunchKernelGGL(publish_word_kernel, dim3(1), dim3(1), 0, s, d_word, b, ticket);
  PPK_HIP(hipGetLastError());
  if (int rc = ppk_wait_ticket(s, &b->ticket, ticket, 5000, "the count did not arrive")) return rc;
  *out = b->value;
  return PPK_OK;
}
}  // namespace

int ppk_knn_band_dev(const ppk_db *db, const ppk_db *qry, const int32_t *kmers, const float *random_tbl, size_t n_clu,
                     int flags, int knn, int dist_col, size_t q_begin, size_t q_end, long long missing_j, long long *d_i,
                     long long *d_j, float *d_dist, unsigned long long *n_candidates, void *stream) {
  if (n_candidates) *n_candidates = 0;
  int rc = ppk_check_pair(db, qry, kmers, q_begin, q_end);
  if (rc != PPK_OK) return rc;
  if (knn < 1 || knn > 32) return ppk_fail(PPK_ERR_ARG, "knn must be in [1, 32]");
  if (dist_col != 0 && dist_col != 1) return ppk_fail(PPK_ERR_ARG, "dist_col must be 0 (core) or 1 (accessory)");
  if (!d_i || !d_j || !d_dist) return ppk_fail(PPK_ERR_ARG, "NULL output buffer");
  if (flags & (PPK_FLAG_JACCARD | PPK_FLAG_COUNTS)) return ppk_fail(PPK_ERR_ARG, "neighbours are taken from distances");
  if (db->n + (qry ? qry->n : 0) >= ((size_t)1 << 32)) return ppk_fail(PPK_ERR_ARG, "too many samples");
  DeviceGuard guard(db->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PpkCall call(db->device, s);
  const size_t n = db->n + (qry ? qry->n : 0);                     // samples with a neighbour list
  double *d_lut = nullptr;
  float *d_rtab = nullptr;
  bool lut_ready = false;
  rc = stage_tables(db, kmers, random_tbl, n_clu, flags, s, &d_lut, &d_rtab, &lut_ready);
  if (rc != PPK_OK) return rc;
  void *d_state = nullptr;
  rc = ppk_scratch_get(db->device, SLOT_ITER_A, 3 * sizeof(unsigned long long) + n * 4 + 256, &d_state);
  if (rc != PPK_OK) return rc;
  const size_t all = qry ? 2 * db->n * qry->n : n * (n - 1);       // two candidates per pair at most
  // Measured (k = 5): ~200 / 530 / 1 000 candidates per sample at 10k / 50k / 100k samples.  A bound is the
  // k-th smallest of ONE tile's candidates (bounds are not merged across tiles: that would need a
  // lock per sample), so it settles near the (k / 256) / (tiles per row) quantile rather than at the
  // true k-th distance; 12 bytes per candidate make that a non-issue (1.8 GB of scratch at 100k).
  // (Tried: three launches of growing size so that the bulk runs under settled bounds -- emitted more,
  // not less, in the first two.)
  // Large jobs go piece by piece (a dispatch holds < 2^32 work-items: ppk_rows_per_dispatch): when the list
  // has filled half its room, or a piece did not fit, the list is cut down to the best knn per sample -- which
  // also sets every bound to the true k-th distance so far -- and the job goes on.  A million genomes run
  // in a few dozen pieces with a list of at most 2^31 entries, whatever n^2 is.
  size_t cap = n * (size_t)(256 + 256 * knn);
  if (cap < ((size_t)1 << 20)) cap = (size_t)1 << 20;
  if (cap > all) cap = all;
  if (cap == 0) cap = 1;
  const size_t sort_limit = (size_t)0x7fffffff - 1024;             // one radix sort takes fewer than 2^31 items
  if (cap > sort_limit) cap = sort_limit;
  if (const long long want = ppk_config().knn_list.load(); want > 0) cap = (size_t)want;   // (tests: a short list)
  // the least a list must hold: the best knn per sample (what a cut leaves) plus what the smallest piece -- 64
  // query rows, two tiles per 256 refs -- can emit when no bound filters anything (all distances equal):
  // 32 * knn for its queries and 2 * 256 * knn for its refs per tile, 4.25 n knn in all
  const size_t floor_entries = 6 * n * (size_t)knn + 8192;
  if (floor_entries > sort_limit) return ppk_fail(PPK_ERR_ARG, "neighbours from tiles: 6 * n * knn must stay below 2^31");
  if (cap < floor_entries) cap = floor_entries;
  if (cap > all) cap = all;
  if (cap > sort_limit) cap = sort_limit;
  if (cap == 0) cap = 1;
  const int knn_args[2] = {knn, dist_col};
  void *d_cand = nullptr;
  size_t vals_off = 0;
  auto room = [&](size_t entries) {        // (re)allocates the list for `entries`; only while it is empty
    vals_off = (entries * 4 + 255) & ~(size_t)255;
    return ppk_scratch_get(db->device, SLOT_ITER_B, vals_off + entries * 8 + 256, &d_cand);
  };
  rc = room(cap);
  if (rc != PPK_OK) return rc;
  rc = ppk_launch_knn_state_init(d_state, n, cap, vals_off, 1, s);
  if (rc != PPK_OK) return rc;
  auto read_count = [&](unsigned long long *c) {
    return read_device_word(db->device, static_cast<const unsigned long long *>(d_state), c, s);
  };
  auto set_count = [&](unsigned long long c) {
    PPK_HIP(hipMemcpyAsync(d_state, &c, sizeof(c), hipMemcpyHostToDevice, s));
    PPK_HIP(hipStreamSynchronize(s));
    return (int)PPK_OK;
  };
  auto keys = [&]() { return static_cast<uint32_t *>(d_cand); };
  auto vals = [&]() { return reinterpret_cast<uint64_t *>(static_cast<char *>(d_cand) + vals_off); };
  unsigned long long count = 0;
  size_t piece = ppk_rows_per_dispatch(db);
  // A bound that comes from ONE tile is the k-th smallest of 256 (a query's) or 32 (a ref's) distances; the
  // k-th smallest of a few thousand is far lower.  So a job of some size opens with a few percent of its rows,
  // cuts the list -- which sets every bound to the k-th distance among those -- and runs the rest under them:
  // at 100 000 genomes the stream drops from 940 (k = 5) / 3 400 (10) / 11 000 (20) candidates per sample.
  const long long warm_opt = ppk_config().knn_warm.load();
  size_t warm = 0;        // rows of the opening piece (0: none)
  const bool big = q_end - q_begin >= 16384 || ppk_config().knn_list.load() > 0;   // small jobs: one pass, as ever
  if (warm_opt != 0 && big) {
    warm = (q_end - q_begin) / (size_t)(warm_opt > 0 ? warm_opt : 32) / 64 * 64;
    if (warm < 64) warm = 64;
  }
  // Pieces: at most what one dispatch holds (`piece`).  The opening piece runs without any bound, so it is
  // also kept below what the list can take in the worst case -- every tile emitting knn candidates for each of
  // its 32 queries and 2 * min(knn, 16) for each of its 256 refs (a million genomes, k = 10: 3 200 rows; one of
  // 31 000 emitted 7.9 G candidates into a list of 2.1 G).  Once bounds exist a piece emits a small fraction of
  // that, so the length doubles after every piece that used less than a quarter of the free room.
  const size_t r_tiles = (db->n + 255) / 256;
  const size_t worst_per_tile = 32 * (size_t)knn + 512 * (size_t)(knn < 16 ? knn : 16);
  auto rows_that_fit = [&](unsigned long long held) {
    size_t rows = (size_t)((cap - (size_t)held) / worst_per_tile / r_tiles) * 32 / 64 * 64;
    return rows < 64 ? (size_t)64 : rows;
  };
  size_t cur = piece;
  if (warm && warm < cur) cur = warm;
  if (big && rows_that_fit(0) < cur && q_end - q_begin > rows_that_fit(0)) cur = rows_that_fit(0);
  const bool staged = cur < q_end - q_begin && cur < piece;      // the job opens with a short piece and a cut
  DistJob job;
  job.ref = db, job.qry = qry, job.kmers = kmers, job.d_rtab = d_rtab, job.n_clu = d_rtab ? n_clu : 1, job.flags = flags;
  job.d_mask = static_cast<uint64_t *>(d_state), job.knn_args = knn_args;
  job.d_lut = d_lut, job.lut_ready = lut_ready, job.s = s;
  for (size_t lo = q_begin; lo < q_end && n > 1;) {
    const size_t this_piece = cur;
    const size_t hi = lo + this_piece < q_end ? lo + this_piece : q_end;
    const unsigned long long before = count;
    job.q_begin = lo, job.q_end = hi, job.d_out = d_cand;      // (`room` may have moved the list)
    rc = ppk_launch_dist(job);
    if (rc != PPK_OK) return rc;
    job.lut_ready = true;
    rc = read_count(&count);
    if (rc != PPK_OK) return rc;
    if (ppk_config().host_trace.load())
      fprintf(stderr, "[ppk knn] rows %zu..%zu: list %llu -> %llu of %zu%s\n", lo, hi, before, count, cap,
              count > cap ? " (does not fit)" : "");
    if (count > cap) {
      // the piece did not fit: what it wrote is dropped (a second copy of a pair would break the selection),
      // room is made, and the piece runs again -- under the bounds it has tightened meanwhile
      const unsigned long long wanted = count - before;
      rc = set_count(before);
      if (rc != PPK_OK) return rc;
      count = before;
      if (before > n * (unsigned long long)knn) {
        rc = ppk_knn_compact(db->device, keys(), vals(), (size_t)before, n, knn, d_state, d_i, d_j, d_dist, s);
        if (rc != PPK_OK) return rc;
        count = n * (unsigned long long)knn;
      } else if (before == 0 && cap < sort_limit && cap < all) {
        cap = (size_t)wanted + (size_t)wanted / 4 + 1024;           // an empty list: simply more room
        if (cap > sort_limit) cap = sort_limit;
        if (cap > all) cap = all;
        rc = room(cap);
        if (rc == PPK_OK) rc = ppk_launch_knn_state_init(d_state, n, cap, vals_off, 0, s);
        if (rc != PPK_OK) return rc;
      } else if (cur > 64) {
        cur = (cur / 2 + 63) / 64 * 64;                             // nothing left to drop: smaller pieces
      } else {
        return ppk_fail(PPK_ERR_CAPACITY, "neighbour candidates keep overflowing their buffer");
      }
      continue;
    }
    const bool opening = staged && lo == q_begin;
    const unsigned long long emitted = count - before;
    const size_t lo_piece = lo;
    lo = hi;
    if (emitted < (cap - (size_t)before) / 4 && cur < piece) {
      // The next piece: at least twice this one; after a piece that ran under real bounds, as many rows as -- at four
      // times this piece's candidates per pair -- fill a quarter of the free room (the pieces of a staged job used to
      // double one by one: six launches, each with its tail and its read-back, where three do).
      size_t next = cur * 2;
      if (!opening && hi > lo_piece) {
        auto pairs_of = [&](size_t a, size_t b) {      // pairs of query rows [a, b)
          return qry ? (double)(b - a) * (double)db->n : 0.5 * ((double)b * (double)(b - 1) - (double)a * (double)(a - 1));
        };
        const double rate = 4.0 * ((double)emitted + 1.0) / (pairs_of(lo_piece, hi) + 1.0);
        const double room = 0.25 * (double)(cap - (size_t)count);
        size_t rows = cur;
        while (rows < piece && pairs_of(hi, hi + rows * 2 < q_end ? hi + rows * 2 : q_end) * rate < room) rows *= 2;
        if (rows > next) next = rows;
      }
      cur = next < piece ? next : piece;
    }
    // cut when the list is half full -- or, in a staged job, as soon as it holds 16 lists' worth: a cut costs a
    // sort of what is there and leaves every bound at the true k-th distance so far, after which a piece emits a
    // small fraction of what it did (1 M genomes: 300 M per 65 000 rows before the second cut, 5 M after)
    const unsigned long long lists = (unsigned long long)ppk_config().knn_cut.load() * n * (unsigned long long)knn;
    const unsigned long long cut_at = staged && lists > 0 && lists < cap / 2 ? lists : cap / 2;
    if (lo < q_end && (count > cut_at || opening) && count > n * (unsigned long long)knn) {
      rc = ppk_knn_compact(db->device, keys(), vals(), (size_t)count, n, knn, d_state, d_i, d_j, d_dist, s);
      if (rc != PPK_OK) return rc;
      count = n * (unsigned long long)knn;
    }
  }
  if (n_candidates) *n_candidates = count;
  return ppk_knn_from_candidates(db->device, keys(), vals(), (size_t)count, n, knn, d_i, d_j, d_dist, s, missing_j);
}

extern "C" int ppk_knn_sketches_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                                    size_t n_clu, int flags, int knn, int dist_col, long long *d_i,
                                    long long *d_j, float *d_dist, unsigned long long *n_candidates,
                                    void *stream) {
  return ppk_knn_band_dev(db, nullptr, kmers, random_tbl, n_clu, flags, knn, dist_col, 0, db ? db->n : 0, 0, d_i, d_j,
                          d_dist, n_candidates, stream);
}

// One band of the triangle's rows (multi-GPU: a band per rank): the best knn per sample among the band's pairs,
// unfilled slots marked j = -1; the bands' lists merge into the whole job's (a pair belongs to one band).
extern "C" int ppk_knn_sketches_band_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                                         size_t n_clu, int flags, int knn, int dist_col, size_t q_begin,
                                         size_t q_end, long long *d_i, long long *d_j, float *d_dist,
                                         unsigned long long *n_candidates, void *stream) {
  return ppk_knn_band_dev(db, nullptr, kmers, random_tbl, n_clu, flags, knn, dist_col, q_begin, q_end, -1, d_i, d_j,
                          d_dist, n_candidates, stream);
}

// ref x query: the knn nearest QUERIES of every reference (samples 0 .. n_ref-1, neighbours numbered n_ref + q)
// and the knn nearest REFERENCES of every query (samples n_ref + q), from one pass over the rectangle's tiles.
extern "C" int ppk_knn_sketches_rq_dev(const ppk_db *ref, const ppk_db *qry, const int32_t *kmers,
                                       const float *random_tbl, size_t n_clu, int flags, int knn, int dist_col,
                                       long long *d_i, long long *d_j, float *d_dist,
                                       unsigned long long *n_candidates, void *stream) {
  if (!qry) return ppk_fail(PPK_ERR_ARG, "ppk_knn_sketches_rq_dev: the query database is missing");
  return ppk_knn_band_dev(ref, qry, kmers, random_tbl, n_clu, flags, knn, dist_col, 0, qry->n, 0, d_i, d_j, d_dist,
                          n_candidates, stream);
}

// The two halves of the above for N GPUs: each rank emits the candidates of ITS band of query rows
// (a pair is emitted by the rank whose band holds its smaller sample, for both of its samples), the
// candidate lists are gathered, and one rank selects.  Bounds are per call: a band knows nothing of
// the others' -- the union is still a superset of every true neighbour list.
extern "C" int ppk_knn_candidates_dev(const ppk_db *db, const int32_t *kmers, const float *random_tbl,
                                      size_t n_clu, int flags, int knn, int dist_col, size_t q_begin,
                                      size_t q_end, unsigned *d_keys, unsigned long long *d_vals, size_t cap,
                                      unsigned long long *n_candidates, void *stream) {
  if (!n_candidates) return ppk_fail(PPK_ERR_ARG, "n_candidates is NULL");
  *n_candidates = 0;
  int rc = ppk_check_pair(db, nullptr, kmers, q_begin, q_end);
  if (rc != PPK_OK) return rc;
  if (knn < 1 || knn > 32) return ppk_fail(PPK_ERR_ARG, "knn must be in [1, 32]");
  if (dist_col != 0 && dist_col != 1) return ppk_fail(PPK_ERR_ARG, "dist_col must be 0 (core) or 1 (accessory)");
  if (cap && (!d_keys || !d_vals)) return ppk_fail(PPK_ERR_ARG, "NULL candidate buffer");
  if (flags & (PPK_FLAG_JACCARD | PPK_FLAG_COUNTS)) return ppk_fail(PPK_ERR_ARG, "neighbours are taken from distances");
  DeviceGuard guard(db->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PpkCall call(db->device, s);
  const size_t n = db->n;
  if (ppk_rows_in_band(n, 0, q_begin, q_end) == 0) return PPK_OK;
  double *d_lut = nullptr;
  float *d_rtab = nullptr;
  bool lut_ready = false;
  rc = stage_tables(db, kmers, random_tbl, n_clu, flags, s, &d_lut, &d_rtab, &lut_ready);
  if (rc != PPK_OK) return rc;
  void *d_state = nullptr;
  rc = ppk_scratch_get(db->device, SLOT_ITER_A, 3 * sizeof(unsigned long long) + n * 4 + 256, &d_state);
  if (rc != PPK_OK) return rc;
  // the kernel addresses the value array relative to the key array (modulo 2^64)
  const unsigned long long vals_off = (unsigned long long)(reinterpret_cast<char *>(d_vals) - reinterpret_cast<char *>(d_keys));
  rc = ppk_launch_knn_state_init(d_state, n, cap, vals_off, 1, s);
  if (rc != PPK_OK) return rc;
  const int knn_args[2] = {knn, dist_col};
  DistJob job;
  job.ref = db, job.kmers = kmers, job.d_rtab = d_rtab, job.n_clu = d_rtab ? n_clu : 1, job.flags = flags;
  job.q_begin = q_begin, job.q_end = q_end, job.d_out = d_keys, job.d_mask = static_cast<uint64_t *>(d_state);
  job.knn_args = knn_args, job.d_lut = d_lut, job.lut_ready = lut_ready, job.s = s;
  rc = ppk_launch_dist(job);
  if (rc != PPK_OK) return rc;
  unsigned long long count = 0;
  rc = read_device_word(db->device, static_cast<const unsigned long long *>(d_state), &count, s);
  if (rc != PPK_OK) return rc;
  *n_candidates = count;
  if (count > cap) return ppk_fail(PPK_ERR_CAPACITY, "candidate buffers too small: need " + std::to_string(count));
  return PPK_OK;
}

extern "C" int ppk_knn_select_dev(const unsigned *d_keys, const unsigned long long *d_vals, size_t count,
                                  size_t n, int knn, long long *d_i, long long *d_j, float *d_dist,
                                  void *stream) {
  if (knn < 1 || knn > 32) return ppk_fail(PPK_ERR_ARG, "knn must be in [1, 32]");
  if (!d_i || !d_j || !d_dist || (count && (!d_keys || !d_vals))) return ppk_fail(PPK_ERR_ARG, "NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  return ppk_knn_from_candidates(dev, d_keys, reinterpret_cast<const uint64_t *>(d_vals), count, n, knn, d_i,
                                 d_j, d_dist, s);
}

// ---- kernel 2, device entry points -------------------------------------------------
extern "C" int ppk_assign_threshold_dev(const float *d_dist, size_t n_rows, int slope, float x_max,
                                        float y_max, float *d_out, void *stream) {
  if (slope < 0 || slope > 2) return ppk_fail(PPK_ERR_ARG, "slope must be 0, 1 or 2");
  if (n_rows && (!d_dist || !d_out)) return ppk_fail(PPK_ERR_ARG, "NULL distance/output buffer");
  return ppk_launch_assign(d_dist, n_rows, slope, x_max, y_max, d_out, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_edge_threshold_dev(const float *d_dist, size_t n_rows, size_t n_ref, int slope,
                                      float x_max, float y_max, int inclusive, long long *d_edges,
                                      size_t cap, unsigned long long *d_n_edges, void *stream) {
  if (slope < 0 || slope > 2) return ppk_fail(PPK_ERR_ARG, "slope must be 0, 1 or 2");
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  RowTest t = {};
  t.kind = RowTest::LINE;
  t.slope = slope, t.inclusive = inclusive, t.x_max = x_max, t.y_max = y_max;
  return ppk_row_edges(d_dist, n_rows, n_ref, 0, t, d_edges, cap, d_n_edges, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_bgmm_assign_dev(const float *d_dist, size_t n_rows, const ppk_bgmm *model, int32_t *d_labels,
                                   float *d_resp, void *stream) {
  if (int rc = check_bgmm(model)) return rc;
  if (n_rows == 0) return PPK_OK;
  if (!d_labels && !d_resp) return ppk_fail(PPK_ERR_ARG, "neither labels nor responsibilities asked for");
  if (!d_dist) return ppk_fail(PPK_ERR_ARG, "NULL distance buffer");
  return ppk_launch_bgmm_assign(d_dist, n_rows, *model, d_labels, d_resp, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_bgmm_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, const ppk_bgmm *model,
                                  long long int_offset, long long *d_edges, size_t cap,
                                  unsigned long long *d_n_edges, void *stream) {
  if (int rc = check_bgmm(model)) return rc;
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  RowTest t = {};
  t.kind = RowTest::BGMM;
  t.bgmm = *model;
  return ppk_row_edges(d_dist, n_rows, n_ref, int_offset, t, d_edges, cap, d_n_edges, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_qc_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, int mode,
                                float max_pi, float max_a, long long *d_edges, size_t cap,
                                unsigned long long *d_n_edges, void *stream) {
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  if (mode != 0 && mode != 1) return ppk_fail(PPK_ERR_ARG, "mode must be 0 (long) or 1 (zero)");
  RowTest t = {};
  t.kind = RowTest::QC;
  t.mode = mode, t.max_pi = max_pi, t.max_a = max_a;
  return ppk_row_edges(d_dist, n_rows, n_ref, 0, t, d_edges, cap, d_n_edges, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_generate_tuples_dev(const int32_t *d_assign, size_t n_rows, int within_label,
                                       int self, size_t num_ref, long long int_offset,
                                       long long *d_edges, size_t cap,
                                       unsigned long long *d_n_edges, void *stream) {
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  if (!self && num_ref == 0) return ppk_fail(PPK_ERR_ARG, "num_ref must be > 0 when self is false");
  RowTest t = {};
  t.kind = RowTest::LABEL;
  t.within_label = within_label;
  return ppk_row_edges(d_assign, n_rows, self ? 0 : num_ref, int_offset, t, d_edges, cap, d_n_edges,
                       static_cast<hipStream_t>(stream));
}

extern "C" int ppk_generate_all_tuples_dev(size_t num_ref, size_t num_queries, int self, long long int_offset,
                                           long long *d_edges, size_t cap, size_t *n_edges, void *stream) {
  if (!n_edges) return ppk_fail(PPK_ERR_ARG, "n_edges is NULL");
  const size_t n = self ? (num_ref ? num_ref * (num_ref - 1) / 2 : 0) : num_ref * num_queries;
  *n_edges = n;
  if (n == 0) return PPK_OK;
  if (n > cap) return ppk_fail(PPK_ERR_CAPACITY, "output too small: need " + std::to_string(n));
  if (!d_edges) return ppk_fail(PPK_ERR_ARG, "d_edges is NULL");
  return ppk_launch_all_tuples(n, num_ref, num_queries, self ? 1 : 0, int_offset, d_edges,
                               static_cast<hipStream_t>(stream));
}

uint64_t ppk_token(const void *bytes, size_t len, uint64_t seed) {
  const unsigned char *b = static_cast<const unsigned char *>(bytes);
  uint64_t h = 1469598103934665603ull ^ seed;
  for (size_t i = 0; i < len; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h ? h : 1;
}
