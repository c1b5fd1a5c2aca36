// Fitting and assigning PopPUNK's DBSCAN (HDBSCAN) model on gfx950 (include/ppk.h "DBSCAN").
//
// Everything is ordered on the squared distance d2(a, b) = (double)(ax - bx)^2 + (double)(ay - by)^2, the float32
// coordinates widened first and then the IEEE double operations numpy performs on the same arrays, none of them
// fused (-ffp-contract=off).  A non-negative double orders as its bit pattern read as an unsigned integer, which is
// what every comparison below is made on.
//
//  - dbscan_core_kernel    : core2[a], the m-th smallest d2(a, b) over b != a.  A selection, not a sort: the 64-bit
//                            image of the answer is found two bits a pass, each pass one count of the whole row
//                            against three thresholds.  64 rows a workgroup, one per lane; the four waves split every
//                            LDS tile of training points between them and add their counts.
//  - Boruvka on the implicit complete graph (ppk_dbscan_mst_dev): per round
//      dbscan_nearest_kernel : every point's least edge (mr2, partner) into another component, the same tiling with
//                              core2 and component ids beside the points
//      dbscan_comp_w / _pair : the per-component minimum of the 128-bit key (mr2 bits, lo, hi) in two integer
//                              atomicMin steps (first the weight, then lo << 32 | hi among the points that hold it)
//      dbscan_hook_kernel    : every root hooks along its edge (of a mutual pair the larger root under the smaller)
//                              and appends the edge; dbscan_jump_kernel compresses, as ppk_mst.hip does
//    then two stable rocPRIM radix sorts put the n - 1 edges in the total order.
//  - dbscan_assign_grid_kernel : one wave per row.  The row's square of grid cells is grown until it holds 1.5 x 2m
//                            points, the same selection runs on the square's points only (the cell-sorted copy makes
//                            every grid row of the square one contiguous run, read coalesced), and the result stands
//                            if the 2m-th distance found lies strictly inside the square's margin: then no point
//                            outside can precede or tie any of the 2m nearest.  Otherwise the square is regrown
//                            once from the distance found (which bounds the true one), and failing that the row
//                            scans everything.  Ties at the 2m-th distance are cut by original index, as defined.
//  - dbscan_assign_kernel  : the plain exact scan (option dbscan_search = 1; the yardstick, and what models of fewer
//                            than 1 024 points use): one row per lane, every training point per row.  The same
//                            two-bit selection finds d2 of the row's (m + 1)-th and 2m-th nearest training points in
//                            shared passes, one more pass takes the arg-min of max(core2[t], r2, d2) over the 2m
//                            nearest under the (d2, t) order, and the walk up the condensed tree gives the label.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include <string>
#include <vector>

#include "ppk_internal.h"

struct ppk_dbscan {
  int device;
  size_t n, n_cl;
  int min_samples, within_label, scale_is_f64;
  float scale_f32[2];
  double scale_f64[2];
  char *d_block;               // one allocation: everything below
  const float2 *d_pts;
  const double *d_core2, *d_pt_lambda, *d_cl_birth;
  const int32_t *d_pt_cluster, *d_cl_parent, *d_cl_label;
  // the search structure of the assignment: the training points bucketed on a uniform g x g grid over their bounding
  // box, a cell-sorted copy (points, core2, original index) and the cells' first positions (g * g + 1)
  int g;
  double gx0, gy0, gwx, gwy, geps;
  const float2 *d_spts;
  const double *d_score2;
  const int32_t *d_sidx, *d_cell;
  unsigned long long *d_full;  // rows whose search ended as a scan of every training point (ppk_dbscan_stats)
};

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 64;        // rows of a workgroup of the fit kernels: one per lane, the waves split the columns
constexpr int kTile = 2048;      // training points per LDS tile
constexpr int kHops = 16;
constexpr unsigned long long kNone = ~0ull;

__device__ __forceinline__ double d2_of(float2 a, float2 b) {
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y;
  return dx * dx + dy * dy;
}
__device__ __forceinline__ double d2_of(double2 q, float2 b) {
  const double dx = q.x - (double)b.x, dy = q.y - (double)b.y;
  return dx * dx + dy * dy;
}
__device__ __forceinline__ unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }

// ---- core distances --------------------------------------------------------------------------------------------
// rank: 0-based position in the row sorted WITH the point itself (its own 0 is first or ties the first), so the m-th
// smallest over b != a is position m.
__global__ void __launch_bounds__(kBlock) dbscan_core_kernel(const float2 *__restrict__ pts, size_t n, unsigned rank,
                                                             double *__restrict__ core2) {
  __shared__ float2 tile[kTile];
  __shared__ unsigned cnt[3][4][kRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * kRows + lane;
  const float2 a = row < n ? pts[row] : make_float2(0.f, 0.f);
  unsigned long long prefix = 0;
  for (int shift = 62; shift >= 0; shift -= 2) {
    const unsigned long long t1 = prefix | (1ull << shift), t2 = prefix | (2ull << shift), t3 = prefix | (3ull << shift);
    unsigned c1 = 0, c2 = 0, c3 = 0;
    for (size_t base = 0; base < n; base += kTile) {
      const int len = (int)(n - base < (size_t)kTile ? n - base : (size_t)kTile);
      __syncthreads();
      for (int i = threadIdx.x; i < len; i += kBlock) tile[i] = pts[base + i];
      __syncthreads();
      const int per = (len + 3) / 4, lo = wave * per, hi = lo + per < len ? lo + per : len;
      for (int j = lo; j < hi; ++j) {
        const unsigned long long k = key_of(d2_of(a, tile[j]));
        c1 += k < t1;
        c2 += k < t2;
        c3 += k < t3;
      }
    }
    cnt[0][wave][lane] = c1;
    cnt[1][wave][lane] = c2;
    cnt[2][wave][lane] = c3;
    __syncthreads();
    unsigned s1 = 0, s2 = 0, s3 = 0;
    for (int w = 0; w < 4; ++w) {
      s1 += cnt[0][w][lane];
      s2 += cnt[1][w][lane];
      s3 += cnt[2][w][lane];
    }
    // the answer is >= a threshold exactly when no more than `rank` keys lie below it
    prefix |= (unsigned long long)((s1 <= rank) + (s2 <= rank) + (s3 <= rank)) << shift;
    // cnt is rewritten only after the next pass's tile barriers (n >= 1: at least one tile)
  }
  if (wave == 0 && row < n) core2[row] = __longlong_as_double((long long)prefix);
}

// ---- Boruvka ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) dbscan_init_kernel(int *comp, unsigned long long *cw, unsigned long long *cp,
                                                             size_t n) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    comp[v] = (int)v;
    cw[v] = kNone;
    cp[v] = kNone;
  }
}

// pw[a], pb[a]: the least (mr2 bits, b) over every b of another component.  For one a the order of its edges by
// (lo, hi) is the order of b, so the first least b in ascending order is the least edge under the total order.
constexpr int kTileM = 1024;
__global__ void __launch_bounds__(kBlock) dbscan_nearest_kernel(const float2 *__restrict__ pts,
                                                                const double *__restrict__ core2,
                                                                const int *__restrict__ comp, size_t n,
                                                                const unsigned *__restrict__ n_done,
                                                                unsigned long long *__restrict__ pw, int *__restrict__ pb) {
  if (*n_done == (unsigned)(n - 1)) return;
  __shared__ float2 tp[kTileM];
  __shared__ double tc[kTileM];
  __shared__ int tk[kTileM];
  __shared__ unsigned long long bw[4][kRows];
  __shared__ int bb[4][kRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * kRows + lane;
  const bool live = row < n;
  const float2 a = live ? pts[row] : make_float2(0.f, 0.f);
  const double ca = live ? core2[row] : 0.0;
  const int mine = live ? comp[row] : -1;
  unsigned long long best = kNone;
  int bidx = -1;
  for (size_t base = 0; base < n; base += kTileM) {
    const int len = (int)(n - base < (size_t)kTileM ? n - base : (size_t)kTileM);
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += kBlock) {
      tp[i] = pts[base + i];
      tc[i] = core2[base + i];
      tk[i] = comp[base + i];
    }
    __syncthreads();
    const int per = (len + 3) / 4, lo = wave * per, hi = lo + per < len ? lo + per : len;
    for (int j = lo; j < hi; ++j) {
      const double d2 = d2_of(a, tp[j]);
      const double cb = tc[j];
      const double mr = fmax(fmax(ca, cb), d2);
      const unsigned long long k = key_of(mr);
      if (tk[j] != mine && k < best) {
        best = k;
        bidx = (int)base + j;
      }
    }
  }
  bw[wave][lane] = best;
  bb[wave][lane] = bidx;
  __syncthreads();
  if (wave == 0 && live) {
    for (int w = 1; w < 4; ++w) {
      const unsigned long long k = bw[w][lane];
      const int b = bb[w][lane];
      if (k < best || (k == best && k != kNone && b < bidx)) {
        best = k;
        bidx = b;
      }
    }
    pw[row] = best;
    pb[row] = bidx;
  }
}

__device__ __forceinline__ unsigned long long pair_of(int a, int b) {
  const unsigned long long lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
  return (lo << 32) | hi;
}

__global__ void __launch_bounds__(kBlock) dbscan_comp_w_kernel(const unsigned long long *pw, const int *comp, size_t n,
                                                               unsigned long long *cw) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long k = pw[v];
    if (k != kNone && cw[comp[v]] > k) atomicMin(&cw[comp[v]], k);
  }
}

__global__ void __launch_bounds__(kBlock) dbscan_comp_pair_kernel(const unsigned long long *pw, const int *pb,
                                                                  const int *comp, size_t n,
                                                                  const unsigned long long *cw, unsigned long long *cp) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long k = pw[v];
    if (k == kNone || k != cw[comp[v]]) continue;
    const unsigned long long p = pair_of((int)v, pb[v]);
    if (cp[comp[v]] > p) atomicMin(&cp[comp[v]], p);
  }
}

// pw is emptied here for the next round (a finished tree leaves every slot empty, and the reductions idle)
__global__ void __launch_bounds__(kBlock) dbscan_hook_kernel(const int *comp, size_t n, const unsigned long long *cw,
                                                             const unsigned long long *cp, int *dst,
                                                             unsigned long long *pw, unsigned *n_done, int *e_lo,
                                                             int *e_hi, unsigned long long *e_w) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int c = comp[v];
    int to = c;
    pw[v] = kNone;
    if (c == (int)v && cw[v] != kNone) {
      const unsigned long long p = cp[v];
      const int lo = (int)(p >> 32), hi = (int)(p & 0xffffffffull);
      const int other = comp[lo] == c ? comp[hi] : comp[lo];
      const bool mutual = cw[other] == cw[v] && cp[other] == p;
      if (!(mutual && (int)v < other)) {
        to = other;
        const unsigned slot = atomicAdd(n_done, 1u);
        if (slot < (unsigned)(n - 1)) {
          e_lo[slot] = lo;
          e_hi[slot] = hi;
          e_w[slot] = cw[v];
        }
      }
    }
    dst[v] = to;
  }
}

__global__ void __launch_bounds__(kBlock) dbscan_jump_kernel(const int *src, int *dst, size_t n, unsigned long long *cw,
                                                             unsigned long long *cp, int pass) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    if (pass == 0) {
      cw[v] = kNone;
      cp[v] = kNone;
    }
    int x = src[v];
    for (int h = 0; h < kHops; ++h) {
      const int y = src[x];
      if (y == x) break;
      x = y;
    }
    dst[v] = x;
  }
}

__global__ void __launch_bounds__(kBlock) dbscan_pair_key_kernel(const int *e_lo, const int *e_hi, size_t m,
                                                                 unsigned long long *keys, int *vals) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    keys[k] = ((unsigned long long)(unsigned)e_lo[k] << 32) | (unsigned)e_hi[k];
    vals[k] = (int)k;
  }
}

__global__ void __launch_bounds__(kBlock) dbscan_w_key_kernel(const unsigned long long *e_w, const int *idx, size_t m,
                                                              unsigned long long *keys) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (size_t)gridDim.x * blockDim.x)
    keys[p] = e_w[idx[p]];
}

__global__ void __launch_bounds__(kBlock) dbscan_emit_kernel(const int *e_lo, const int *e_hi,
                                                             const unsigned long long *e_w, const int *order, size_t m,
                                                             int32_t *a, int32_t *b, double *mr2) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x) {
    const int k = order[r];
    a[r] = e_lo[k];
    b[r] = e_hi[k];
    mr2[r] = __longlong_as_double((long long)e_w[k]);
  }
}

// ---- assignment --------------------------------------------------------------------------------------------------
struct AssignModel {
  const float2 *pts;
  const double *core2, *pt_lambda, *cl_birth;
  const int32_t *pt_cluster, *cl_parent, *cl_label;
  unsigned n, rank_r, rank_k;     // 0-based positions of r2 and of the last of N in the row's sorted distances
  int scale_is_f64;
  float scale_f32[2];
  double scale_f64[2];
};

__global__ void __launch_bounds__(kBlock) dbscan_assign_kernel(const float2 *__restrict__ dist, size_t n_rows,
                                                               const AssignModel m, int32_t *__restrict__ labels) {
  __shared__ float2 tp[kTile];
  __shared__ double tc[kTile];
  const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = row < n_rows;
  double2 q = make_double2(0.0, 0.0);
  if (live) {
    const float2 d = dist[row];
    ppk_bgmm_scaled(d.x, d.y, m, q.x, q.y);      // x / scale in the dtype numpy promotes to
  }
  const unsigned n = m.n;
  // d2 of position rank_r (r2) and of position rank_k (the last of N), two bits a pass, one d2 per pair for both
  unsigned long long pr = 0, pk = 0;
  for (int shift = 62; shift >= 0; shift -= 2) {
    const unsigned long long r1 = pr | (1ull << shift), r2t = pr | (2ull << shift), r3 = pr | (3ull << shift);
    const unsigned long long k1 = pk | (1ull << shift), k2t = pk | (2ull << shift), k3 = pk | (3ull << shift);
    unsigned a1 = 0, a2 = 0, a3 = 0, b1 = 0, b2 = 0, b3 = 0;
    for (unsigned base = 0; base < n; base += kTile) {
      const int len = (int)(n - base < (unsigned)kTile ? n - base : (unsigned)kTile);
      __syncthreads();
      for (int i = threadIdx.x; i < len; i += kBlock) tp[i] = m.pts[base + i];
      __syncthreads();
      for (int j = 0; j < len; ++j) {
        const unsigned long long k = key_of(d2_of(q, tp[j]));
        a1 += k < r1;
        a2 += k < r2t;
        a3 += k < r3;
        b1 += k < k1;
        b2 += k < k2t;
        b3 += k < k3;
      }
    }
    pr |= (unsigned long long)((a1 <= m.rank_r) + (a2 <= m.rank_r) + (a3 <= m.rank_r)) << shift;
    pk |= (unsigned long long)((b1 <= m.rank_k) + (b2 <= m.rank_k) + (b3 <= m.rank_k)) << shift;
  }
  // N: every t below pk, and the first (rank_k + 1 - #below) of those at pk by index.  One ascending pass counts
  // the ones at pk as they come and keeps the least (w2, d2, t).
  unsigned below = 0;
  for (unsigned base = 0; base < n; base += kTile) {
    const int len = (int)(n - base < (unsigned)kTile ? n - base : (unsigned)kTile);
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += kBlock) tp[i] = m.pts[base + i];
    __syncthreads();
    for (int j = 0; j < len; ++j) below += key_of(d2_of(q, tp[j])) < pk;
  }
  const unsigned quota = m.rank_k + 1 - below;
  unsigned at = 0;
  unsigned long long best_w = kNone, best_d = kNone;
  int best_t = -1;
  for (unsigned base = 0; base < n; base += kTile) {
    const int len = (int)(n - base < (unsigned)kTile ? n - base : (unsigned)kTile);
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += kBlock) {
      tp[i] = m.pts[base + i];
      tc[i] = m.core2[base + i];
    }
    __syncthreads();
    for (int j = 0; j < len; ++j) {
      const unsigned long long k = key_of(d2_of(q, tp[j]));
      bool in = k < pk;
      if (k == pk) {
        in = at < quota;
        ++at;
      }
      const unsigned long long c = key_of(tc[j]);
      unsigned long long w = c > pr ? c : pr;
      w = w > k ? w : k;
      if (in && (w < best_w || (w == best_w && k < best_d))) {
        best_w = w;
        best_d = k;
        best_t = (int)base + j;
      }
    }
  }
  if (!live) return;
  if (best_t < 0) {                 // unreachable: N is never empty
    labels[row] = -1;
    return;
  }
  const double w2 = __longlong_as_double((long long)best_w);
  const double lq = w2 > 0.0 ? 1.0 / sqrt(w2) : DBL_MAX;
  int cl = m.pt_cluster[best_t];
  if (m.pt_lambda[best_t] > lq)
    while (cl != 0 && m.cl_birth[cl] >= lq) cl = m.cl_parent[cl];
  labels[row] = m.cl_label[cl];
}

// ---- assignment through the grid ---------------------------------------------------------------------------------
struct GridModel {
  AssignModel am;
  const float2 *spts;
  const double *score2;
  const int32_t *sidx, *cell;
  unsigned long long *full;
  int g;
  double x0, y0, wx, wy, eps;
};

// every point of the square [cx0, cx1] x [cy0, cy1], the lanes striding each grid row's run
#define PPK_SQUARE_FOR(i)                                                        \
  for (int cy_ = cy0; cy_ <= cy1; ++cy_)                                         \
    for (int i = gm.cell[cy_ * g + cx0] + lane, e_ = gm.cell[cy_ * g + cx1 + 1]; i < e_; i += 64)

__global__ void __launch_bounds__(kBlock) dbscan_assign_grid_kernel(const float2 *__restrict__ dist, size_t n_rows,
                                                                    const GridModel gm, int32_t *__restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;                       // whole waves leave; nothing below synchronises the workgroup
  const AssignModel &m = gm.am;
  const float2 d = dist[row];
  double2 q;
  ppk_bgmm_scaled(d.x, d.y, m, q.x, q.y);
  const int g = gm.g;
  const double fx = (q.x - gm.x0) / gm.wx, fy = (q.y - gm.y0) / gm.wy;
  const int cxq = fx >= 0.0 ? (fx < (double)g ? (int)fx : g - 1) : 0;     // a NaN row lands in cell 0 and never certifies
  const int cyq = fy >= 0.0 ? (fy < (double)g ? (int)fy : g - 1) : 0;
  const unsigned need = m.rank_k + 1;
  unsigned target = need + need / 2 + 8;
  if (target > m.n) target = m.n;
  int r = 0, cx0 = 0, cx1 = 0, cy0 = 0, cy1 = 0;
  bool all = false;
  unsigned long long pr = 0, pk = 0;
  for (int attempt = 0;; ++attempt) {
    for (;;) {
      cx0 = cxq - r > 0 ? cxq - r : 0;
      cy0 = cyq - r > 0 ? cyq - r : 0;
      cx1 = cxq + r < g - 1 ? cxq + r : g - 1;
      cy1 = cyq + r < g - 1 ? cyq + r : g - 1;
      all = cx0 == 0 && cy0 == 0 && cx1 == g - 1 && cy1 == g - 1;
      unsigned c = 0;
      for (int cy = cy0 + lane; cy <= cy1; cy += 64) c += (unsigned)(gm.cell[cy * g + cx1 + 1] - gm.cell[cy * g + cx0]);
      if (all || wave_sum_all(c) >= target) break;
      r += 1 + r / 4;
    }
    pr = 0;
    pk = 0;
    for (int shift = 62; shift >= 0; shift -= 2) {
      const unsigned long long r1 = pr | (1ull << shift), r2t = pr | (2ull << shift), r3 = pr | (3ull << shift);
      const unsigned long long k1 = pk | (1ull << shift), k2t = pk | (2ull << shift), k3 = pk | (3ull << shift);
      unsigned a1 = 0, a2 = 0, a3 = 0, b1 = 0, b2 = 0, b3 = 0;
      PPK_SQUARE_FOR(i) {
        const unsigned long long k = key_of(d2_of(q, gm.spts[i]));
        a1 += k < r1;
        a2 += k < r2t;
        a3 += k < r3;
        b1 += k < k1;
        b2 += k < k2t;
        b3 += k < k3;
      }
      a1 = wave_sum_all(a1);
      a2 = wave_sum_all(a2);
      a3 = wave_sum_all(a3);
      b1 = wave_sum_all(b1);
      b2 = wave_sum_all(b2);
      b3 = wave_sum_all(b3);
      pr |= (unsigned long long)((a1 <= m.rank_r) + (a2 <= m.rank_r) + (a3 <= m.rank_r)) << shift;
      pk |= (unsigned long long)((b1 <= m.rank_k) + (b2 <= m.rank_k) + (b3 <= m.rank_k)) << shift;
    }
    if (all) break;
    // every point outside the square is at least `margin` away (sides on the grid's border have nothing beyond them);
    // the slack covers the rounding of the cell boundaries and of d2
    double margin = INFINITY;
    if (cx0 > 0) margin = fmin(margin, q.x - (gm.x0 + (double)cx0 * gm.wx));
    if (cx1 < g - 1) margin = fmin(margin, (gm.x0 + (double)(cx1 + 1) * gm.wx) - q.x);
    if (cy0 > 0) margin = fmin(margin, q.y - (gm.y0 + (double)cy0 * gm.wy));
    if (cy1 < g - 1) margin = fmin(margin, (gm.y0 + (double)(cy1 + 1) * gm.wy) - q.y);
    const double safe = margin * (1.0 - 1e-9) - gm.eps;
    const double dk2 = __longlong_as_double((long long)pk);
    if (safe > 0.0 && dk2 < safe * safe) break;
    // the distance found bounds the true one from above: a square whose margin exceeds it must certify
    const double rr = (sqrt(dk2) * (1.0 + 1e-9) + 2.0 * gm.eps) / fmin(gm.wx, gm.wy) + 2.0;
    if (attempt == 0 && rr < (double)g) {
      r = (int)rr > r ? (int)rr : r + 1;
      target = 0;
    } else {
      r = g;
    }
  }
  if (all && lane == 0) atomicAdd(gm.full, 1ull);
  // N: everything below pk, and of the ties at pk the first by original index
  unsigned below = 0, ties = 0;
  PPK_SQUARE_FOR(i) {
    const unsigned long long k = key_of(d2_of(q, gm.spts[i]));
    below += k < pk;
    ties += k == pk;
  }
  below = wave_sum_all(below);
  ties = wave_sum_all(ties);
  const unsigned quota = m.rank_k + 1 - below;
  unsigned last_idx = 0xffffffffu;
  if (ties > quota) {
    unsigned pi = 0;
    for (int shift = 30; shift >= 0; shift -= 2) {
      const unsigned t1 = pi | (1u << shift), t2 = pi | (2u << shift), t3 = pi | (3u << shift);
      unsigned c1 = 0, c2 = 0, c3 = 0;
      PPK_SQUARE_FOR(i) {
        if (key_of(d2_of(q, gm.spts[i])) != pk) continue;
        const unsigned t = (unsigned)gm.sidx[i];
        c1 += t < t1;
        c2 += t < t2;
        c3 += t < t3;
      }
      c1 = wave_sum_all(c1);
      c2 = wave_sum_all(c2);
      c3 = wave_sum_all(c3);
      pi |= (unsigned)((c1 <= quota - 1) + (c2 <= quota - 1) + (c3 <= quota - 1)) << shift;
    }
    last_idx = pi;
  }
  unsigned long long best_w = kNone, best_d = kNone;
  unsigned best_t = 0xffffffffu;
  PPK_SQUARE_FOR(i) {
    const unsigned long long k = key_of(d2_of(q, gm.spts[i]));
    const unsigned t = (unsigned)gm.sidx[i];
    if (!(k < pk || (k == pk && t <= last_idx))) continue;
    const unsigned long long c = key_of(gm.score2[i]);
    unsigned long long w = c > pr ? c : pr;
    w = w > k ? w : k;
    if (w < best_w || (w == best_w && (k < best_d || (k == best_d && t < best_t)))) {
      best_w = w;
      best_d = k;
      best_t = t;
    }
  }
  for (int o = 32; o; o >>= 1) {
    const unsigned long long ow = __shfl_xor(best_w, o), od = __shfl_xor(best_d, o);
    const unsigned ot = __shfl_xor(best_t, o);
    if (ow < best_w || (ow == best_w && (od < best_d || (od == best_d && ot < best_t)))) {
      best_w = ow;
      best_d = od;
      best_t = ot;
    }
  }
  if (lane != 0) return;
  if (best_t == 0xffffffffu) {      // unreachable: N is never empty
    labels[row] = -1;
    return;
  }
  const double w2 = __longlong_as_double((long long)best_w);
  const double lq = w2 > 0.0 ? 1.0 / sqrt(w2) : DBL_MAX;
  int cl = m.pt_cluster[best_t];
  if (m.pt_lambda[best_t] > lq)
    while (cl != 0 && m.cl_birth[cl] >= lq) cl = m.cl_parent[cl];
  labels[row] = m.cl_label[cl];
}
#undef PPK_SQUARE_FOR

int check_model(const ppk_dbscan *m, const char *what) {
  if (!m || !m->d_block || m->n < 1 || m->n_cl < 1)
    return ppk_fail(PPK_ERR_ARG, std::string(what) + ": the model is not a ppk_dbscan_create handle");
  return PPK_OK;
}

int launch_assign(const float *d_dist, size_t n_rows, const ppk_dbscan *model, int32_t *d_labels, hipStream_t s) {
  if (n_rows == 0) return PPK_OK;
  if (n_rows > (size_t)0x7fffffff * 4) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_assign: too many rows for one call");
  AssignModel am;
  am.pts = model->d_pts;
  am.core2 = model->d_core2;
  am.pt_lambda = model->d_pt_lambda;
  am.cl_birth = model->d_cl_birth;
  am.pt_cluster = model->d_pt_cluster;
  am.cl_parent = model->d_cl_parent;
  am.cl_label = model->d_cl_label;
  const size_t n = model->n, ms = (size_t)model->min_samples;
  am.n = (unsigned)n;
  am.rank_r = (unsigned)(ms < n ? ms : n - 1);
  am.rank_k = (unsigned)((2 * ms < n ? 2 * ms : n) - 1);
  am.scale_is_f64 = model->scale_is_f64;
  for (int i = 0; i < 2; ++i) {
    am.scale_f32[i] = model->scale_f32[i];
    am.scale_f64[i] = model->scale_f64[i];
  }
  // option dbscan_search: 0 = the grid from 1 024 training points up (below that a wave per row is mostly idle lanes),
  // 1 = the scan, 2 = the grid; the labels do not depend on it
  const long long search = ppk_config().dbscan_search.load();
  if (search == 1 || (search == 0 && n < 1024)) {
    hipLaunchKernelGGL(dbscan_assign_kernel, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       reinterpret_cast<const float2 *>(d_dist), n_rows, am, d_labels);
  } else {
    GridModel gm;
    gm.am = am;
    gm.spts = model->d_spts;
    gm.score2 = model->d_score2;
    gm.sidx = model->d_sidx;
    gm.cell = model->d_cell;
    gm.full = model->d_full;
    gm.g = model->g;
    gm.x0 = model->gx0;
    gm.y0 = model->gy0;
    gm.wx = model->gwx;
    gm.wy = model->gwy;
    gm.eps = model->geps;
    hipLaunchKernelGGL(dbscan_assign_grid_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(kBlock), 0, s,
                       reinterpret_cast<const float2 *>(d_dist), n_rows, gm, d_labels);
  }
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_dbscan_core_dev(const float *d_pts, size_t n, int min_samples, double *d_core2, void *stream) {
  if (!d_pts || !d_core2) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_core: NULL array");
  if (n > (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_core: n must be < 2^31");
  if (min_samples < 1) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_core: min_samples must be at least 1");
  if (n < 2 || (size_t)min_samples > n - 1)
    return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_core: min_samples " + std::to_string(min_samples) + " needs at least " +
                                     std::to_string((size_t)min_samples + 1) + " points, there are " + std::to_string(n));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dbscan_core_kernel, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kBlock), 0, s,
                     reinterpret_cast<const float2 *>(d_pts), n, (unsigned)min_samples, d_core2);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_dbscan_mst_dev(const float *d_pts, const double *d_core2, size_t n, int32_t *d_a, int32_t *d_b,
                                  double *d_mr2, void *stream) {
  if (n > (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_mst: n must be < 2^31");
  if (n < 1) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_mst: no points");
  if (n == 1) return PPK_OK;
  if (!d_pts || !d_core2 || !d_a || !d_b || !d_mr2) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_mst: NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n - 1;
  const int rounds = ceil_log2(n);
  int passes = 1;
  while (passes < 8 && ((size_t)1 << (4 * passes)) < n) ++passes;
  if (!(passes & 1)) ++passes;
  size_t tmp = 0;
  PPK_HIP(rocprim::radix_sort_pairs(nullptr, tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (int *)nullptr, (int *)nullptr, m, 0u, 64u, s));
  unsigned *n_done;
  unsigned long long *pw, *cw, *cp, *e_w, *ka, *kb;
  int *pb, *ca, *cb, *e_lo, *e_hi, *va, *vb;
  char *d_tmp;
  int rc = ppk_scratch_carve(dev, SLOT_DBSCAN, [&](Carve &c) {
    c.take(n_done, 1).take(pw, n).take(cw, n).take(cp, n).take(e_w, n).take(ka, n).take(kb, n);
    c.take(pb, n).take(ca, n).take(cb, n).take(e_lo, n).take(e_hi, n).take(va, n).take(vb, n).take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;
  const float2 *pts = reinterpret_cast<const float2 *>(d_pts);
  const unsigned gn = grid_for(n, kBlock, 4096), gr = (unsigned)((n + kRows - 1) / kRows);

  ppk_prof_stage("boruvka", s);
  PPK_HIP(hipMemsetAsync(n_done, 0, 4, s));
  PPK_HIP(hipMemsetAsync(pw, 0xff, n * 8, s));
  hipLaunchKernelGGL(dbscan_init_kernel, dim3(gn), dim3(kBlock), 0, s, ca, cw, cp, n);
  PPK_HIP(hipGetLastError());
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(dbscan_nearest_kernel, dim3(gr), dim3(kBlock), 0, s, pts, d_core2, ca, n, n_done, pw, pb);
    hipLaunchKernelGGL(dbscan_comp_w_kernel, dim3(gn), dim3(kBlock), 0, s, pw, ca, n, cw);
    hipLaunchKernelGGL(dbscan_comp_pair_kernel, dim3(gn), dim3(kBlock), 0, s, pw, pb, ca, n, cw, cp);
    hipLaunchKernelGGL(dbscan_hook_kernel, dim3(gn), dim3(kBlock), 0, s, ca, n, cw, cp, cb, pw, n_done, e_lo, e_hi, e_w);
    for (int p = 0; p < passes; ++p)
      hipLaunchKernelGGL(dbscan_jump_kernel, dim3(gn), dim3(kBlock), 0, s, (p & 1) ? ca : cb, (p & 1) ? cb : ca, n, cw,
                         cp, p);
    PPK_HIP(hipGetLastError());
  }

  // (lo, hi) first, then a stable sort on the weight: the total order
  ppk_prof_stage("sort", s);
  const unsigned gm = grid_for(m, kBlock, 4096);
  hipLaunchKernelGGL(dbscan_pair_key_kernel, dim3(gm), dim3(kBlock), 0, s, e_lo, e_hi, m, ka, va);
  PPK_HIP(hipGetLastError());
  size_t tb = tmp;
  PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, ka, kb, va, vb, m, 0u, 64u, s));
  hipLaunchKernelGGL(dbscan_w_key_kernel, dim3(gm), dim3(kBlock), 0, s, e_w, vb, m, ka);
  PPK_HIP(hipGetLastError());
  tb = tmp;
  PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, ka, kb, vb, va, m, 0u, 64u, s));
  hipLaunchKernelGGL(dbscan_emit_kernel, dim3(gm), dim3(kBlock), 0, s, e_lo, e_hi, e_w, va, m, d_a, d_b, d_mr2);
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_dbscan_fit(const float *pts, size_t n, int min_samples, int device_id, double *core2, int32_t *a,
                              int32_t *b, double *mr2) {
  if (!pts || !core2 || (n > 1 && (!a || !b || !mr2))) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_fit: NULL array");
  if (n > (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_fit: n must be < 2^31");
  if (int rc = ppk_check_arch(device_id)) return rc;
  float *d_pts;
  double *d_core2, *d_mr2;
  int32_t *d_a, *d_b;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_pts, 2 * n).take(d_core2, n).take(d_mr2, n).take(d_a, n).take(d_b, n);
  }, [&]() -> int {
    PPK_HIP(hipMemcpy(d_pts, pts, n * 8, hipMemcpyHostToDevice));
    int rc = ppk_dbscan_core_dev(d_pts, n, min_samples, d_core2, nullptr);
    if (rc != PPK_OK) return rc;
    rc = ppk_dbscan_mst_dev(d_pts, d_core2, n, d_a, d_b, d_mr2, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(core2, d_core2, n * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(a, d_a, (n - 1) * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(b, d_b, (n - 1) * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(mr2, d_mr2, (n - 1) * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_dbscan_create(const float *pts, const double *core2, size_t n, int min_samples,
                                 const int32_t *pt_cluster, const double *pt_lambda, const int32_t *cl_parent,
                                 const double *cl_birth, const int32_t *cl_label, size_t n_cl, const double *scale,
                                 int scale_is_f64, int within_label, int device_id, ppk_dbscan **out) {
  if (int rc = ppk_check_device(device_id)) return rc;
  if (!pts || !core2 || !pt_cluster || !pt_lambda || !cl_parent || !cl_birth || !cl_label || !scale || !out)
    return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: NULL argument");
  if (n < 1 || n > (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: n must be in [1, 2^31)");
  if (n_cl < 1 || n_cl > n) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: n_cl must be in [1, n]");
  if (min_samples < 1) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: min_samples must be at least 1");
  for (int i = 0; i < 2; ++i)
    if (!(scale[i] > 0.0) || !std::isfinite(scale[i])) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: scale must be positive");
  // the walk up the tree ends only at the root: every parent must lie before its child, every point in a cluster
  if (cl_parent[0] != -1) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: cluster 0 must be the root (parent -1)");
  for (size_t k = 1; k < n_cl; ++k)
    if (cl_parent[k] < 0 || (size_t)cl_parent[k] >= k)
      return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: cluster " + std::to_string(k) + " has no earlier parent");
  for (size_t p = 0; p < n; ++p)
    if (pt_cluster[p] < 0 || (size_t)pt_cluster[p] >= n_cl)
      return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: point " + std::to_string(p) + " is in no cluster");
  if (int rc = ppk_check_arch(device_id)) return rc;
  PPK_ENTER_DEVICE(guard, device_id);
  ppk_dbscan *m = new ppk_dbscan();
  m->device = device_id;
  m->n = n;
  m->n_cl = n_cl;
  m->min_samples = min_samples;
  m->within_label = within_label;
  m->scale_is_f64 = scale_is_f64 ? 1 : 0;
  for (int i = 0; i < 2; ++i) {
    m->scale_f64[i] = scale[i];
    m->scale_f32[i] = (float)scale[i];
  }
  // the grid: about four points a cell, over the bounding box
  double x0 = pts[0], x1 = pts[0], y0 = pts[1], y1 = pts[1];
  for (size_t p = 0; p < n; ++p) {
    const double x = pts[2 * p], y = pts[2 * p + 1];
    if (!std::isfinite(x) || !std::isfinite(y)) {
      delete m;
      return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_create: point " + std::to_string(p) + " is not finite");
    }
    x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1, y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
  }
  int g = (int)std::sqrt((double)n / 4.0);
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  m->g = g;
  m->gx0 = x0;
  m->gy0 = y0;
  m->gwx = x1 > x0 ? (x1 - x0) / g : 1.0;
  m->gwy = y1 > y0 ? (y1 - y0) / g : 1.0;
  m->geps = 1e-9 * (m->gwx > m->gwy ? m->gwx : m->gwy) * g;
  std::vector<int32_t> cell_of(n), cell_start((size_t)g * g + 1, 0), sidx(n);
  for (size_t p = 0; p < n; ++p) {
    int cx = (int)std::floor(((double)pts[2 * p] - x0) / m->gwx), cy = (int)std::floor(((double)pts[2 * p + 1] - y0) / m->gwy);
    cx = cx < 0 ? 0 : (cx > g - 1 ? g - 1 : cx);
    cy = cy < 0 ? 0 : (cy > g - 1 ? g - 1 : cy);
    cell_of[p] = cy * g + cx;
    ++cell_start[(size_t)cell_of[p] + 1];
  }
  for (size_t k = 0; k < (size_t)g * g; ++k) cell_start[k + 1] += cell_start[k];
  {
    std::vector<int32_t> at(cell_start.begin(), cell_start.end() - 1);
    for (size_t p = 0; p < n; ++p) sidx[at[cell_of[p]]++] = (int32_t)p;      // ascending original index inside a cell
  }
  std::vector<float> spts(2 * n);
  std::vector<double> score2(n);
  for (size_t i = 0; i < n; ++i) {
    spts[2 * i] = pts[2 * (size_t)sidx[i]];
    spts[2 * i + 1] = pts[2 * (size_t)sidx[i] + 1];
    score2[i] = core2[sidx[i]];
  }
  Carve c;
  float2 *p_spts = nullptr;
  double *p_score2 = nullptr;
  int32_t *p_sidx = nullptr, *p_cell = nullptr;
  unsigned long long *p_full = nullptr;
  float2 *p_pts = nullptr;
  double *p_core2 = nullptr, *p_lambda = nullptr, *p_birth = nullptr;
  int32_t *p_cluster = nullptr, *p_parent = nullptr, *p_label = nullptr;
  auto layout = [&](Carve &cv) {
    cv.take(p_pts, n).take(p_core2, n).take(p_lambda, n).take(p_birth, n_cl);
    cv.take(p_cluster, n).take(p_parent, n_cl).take(p_label, n_cl);
    cv.take(p_spts, n).take(p_score2, n).take(p_sidx, n).take(p_cell, cell_start.size()).take(p_full, 1);
  };
  layout(c);
  if (hipMalloc(reinterpret_cast<void **>(&m->d_block), c.at) != hipSuccess) {
    delete m;
    return ppk_fail(PPK_ERR_HIP, "ppk_dbscan_create: hipMalloc failed");
  }
  c = Carve{m->d_block};
  layout(c);
  const bool ok = hipMemcpy(p_pts, pts, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_core2, core2, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_lambda, pt_lambda, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_birth, cl_birth, n_cl * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_cluster, pt_cluster, n * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_parent, cl_parent, n_cl * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_label, cl_label, n_cl * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_spts, spts.data(), n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_score2, score2.data(), n * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_sidx, sidx.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p_cell, cell_start.data(), cell_start.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(p_full, 0, 8) == hipSuccess;
  if (!ok) {
    (void)hipFree(m->d_block);
    delete m;
    return ppk_fail(PPK_ERR_HIP, "ppk_dbscan_create: upload failed");
  }
  m->d_pts = p_pts;
  m->d_core2 = p_core2;
  m->d_pt_lambda = p_lambda;
  m->d_cl_birth = p_birth;
  m->d_pt_cluster = p_cluster;
  m->d_cl_parent = p_parent;
  m->d_cl_label = p_label;
  m->d_spts = p_spts;
  m->d_score2 = p_score2;
  m->d_sidx = p_sidx;
  m->d_cell = p_cell;
  m->d_full = p_full;
  *out = m;
  return PPK_OK;
}

extern "C" void ppk_dbscan_destroy(ppk_dbscan *m) {
  if (!m) return;
  if (m->d_block) {
    DeviceGuard guard(m->device);
    (void)hipFree(m->d_block);
  }
  delete m;
}

extern "C" int ppk_dbscan_stats(const ppk_dbscan *model, unsigned long long *rows_scanned) {
  if (int rc = check_model(model, "ppk_dbscan_stats")) return rc;
  if (!rows_scanned) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_stats: NULL argument");
  PPK_ENTER_DEVICE(guard, model->device);
  PPK_HIP(hipDeviceSynchronize());
  PPK_HIP(hipMemcpy(rows_scanned, model->d_full, 8, hipMemcpyDeviceToHost));
  return PPK_OK;
}

extern "C" int ppk_dbscan_assign_dev(const float *d_dist, size_t n_rows, const ppk_dbscan *model, int32_t *d_labels,
                                     void *stream) {
  if (int rc = check_model(model, "ppk_dbscan_assign")) return rc;
  if (n_rows == 0) return PPK_OK;
  if (!d_dist || !d_labels) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_assign: NULL buffer");
  return launch_assign(d_dist, n_rows, model, d_labels, static_cast<hipStream_t>(stream));
}

extern "C" int ppk_dbscan_edges_dev(const float *d_dist, size_t n_rows, size_t n_ref, const ppk_dbscan *model,
                                    long long int_offset, long long *d_edges, size_t cap,
                                    unsigned long long *d_n_edges, void *stream) {
  if (int rc = check_model(model, "ppk_dbscan_edges")) return rc;
  if (!d_n_edges) return ppk_fail(PPK_ERR_ARG, "d_n_edges is NULL");
  if (n_rows && !d_dist) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_edges: NULL distance buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  int32_t *d_lab;
  int rc = ppk_scratch_carve(dev, SLOT_DBSCAN, [&](Carve &c) { c.take(d_lab, n_rows + 1); });
  if (rc != PPK_OK) return rc;
  if ((rc = launch_assign(d_dist, n_rows, model, d_lab, s)) != PPK_OK) return rc;
  return ppk_generate_tuples_dev(d_lab, n_rows, model->within_label, n_ref == 0 ? 1 : 0, n_ref, int_offset, d_edges,
                                 cap, d_n_edges, stream);
}

// DBSCANFit.assign(X) of the Python mirror: chunks of 4 Mi rows uploaded, assigned and fetched in turn.
extern "C" int ppk_dbscan_assign(const float *dist, size_t n_rows, const ppk_dbscan *model, int32_t *labels) {
  if (int rc = check_model(model, "ppk_dbscan_assign")) return rc;
  if (n_rows == 0) return PPK_OK;
  if (!dist || !labels) return ppk_fail(PPK_ERR_ARG, "ppk_dbscan_assign: NULL buffer");
  const size_t chunk = (size_t)4 << 20;
  const size_t buf_rows = n_rows < chunk ? n_rows : chunk;
  float *d_in;
  int32_t *d_lab;
  return ppk_host_frame(model->device, [&](Carve &c) { c.take(d_in, 2 * buf_rows).take(d_lab, buf_rows); }, [&]() -> int {
    for (size_t r0 = 0; r0 < n_rows; r0 += chunk) {
      const size_t rows = n_rows - r0 < chunk ? n_rows - r0 : chunk;
      PPK_HIP(hipMemcpy(d_in, dist + 2 * r0, rows * 8, hipMemcpyHostToDevice));
      const int rc = launch_assign(d_in, rows, model, d_lab, nullptr);
      if (rc != PPK_OK) return rc;
      PPK_HIP(hipMemcpy(labels + r0, d_lab, rows * 4, hipMemcpyDeviceToHost));
    }
    return PPK_OK;
  });
}
