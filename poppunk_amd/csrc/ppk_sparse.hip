// The sparse neighbour matrices of the lineage models: poppunk_refine.extend and lowerRank
// (src/extend.cpp:52-246; callers PopPUNK/models.py:1177,:1367) on the MI355X.
//
// Both are "per sample, the first few entries of a short list in stable order of distance".  The
// reference sorts every row with a stable sort on the CPU and walks it; here every candidate gets a 64-bit
// key -- order-preserving code of the float32 distance << 32 | its place in the reference's tie order --
// the rows are sorted side by side by one segmented radix sort (hipCUB), and one thread per row does the
// reference's walk over the head of its sorted row.  Row counts -> exclusive scan -> the (i, j, dist)
// triplets in row order, as the reference concatenates its per-row vectors.
//
// Nothing is allocated per call: the work buffers are one layout of scratch slot SLOT_SPARSE (sparse_work), the
// uploaded inputs and the result triplets -- at a bound known before anything runs -- one layout of SLOT_HOST_IN
// (ppk_host_frame).  A call synchronises twice: for the bad-rows flag and for the number of triplets.
#include <hipcub/hipcub.hpp>

#include "ppk_internal.h"

namespace {

__device__ __forceinline__ float dist_of(uint64_t key) { return ord_inv((unsigned)(key >> 32)); }

// rows of a row-sorted COO: entries of row r are [start[r], start[r+1]) (src/extend.cpp:15-38); flag[0] is
// raised when the row indices are not ascending or leave [0, n_rows)
__global__ void __launch_bounds__(256)
row_start_kernel(const long long *__restrict__ ri, size_t nnz, size_t n_rows, int *__restrict__ start,
                 int *__restrict__ flag) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t <= n_rows) {
    size_t lo = 0, hi = nnz;
    while (lo < hi) {                       // first entry whose row is >= t
      const size_t mid = (lo + hi) / 2;
      if ((size_t)ri[mid] < t) lo = mid + 1;
      else hi = mid;
    }
    start[t] = (int)(t == n_rows ? nnz : lo);
  }
  if (t < nnz) {
    const long long r = ri[t];
    if (r < 0 || (size_t)r >= n_rows || (t + 1 < nnz && ri[t + 1] < r)) flag[0] = 1;
  }
}

// ---- lowerRank ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
lr_keys_kernel(const long long *__restrict__ ri, const float *__restrict__ rd, size_t nnz,
               const int *__restrict__ start, uint64_t *__restrict__ keys, int *__restrict__ vals) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const unsigned pos = (unsigned)(e - (size_t)start[ri[e]]);
  keys[e] = ((uint64_t)ord_of(rd[e]) << 32) | pos;      // equal distances: the earlier entry first
  vals[e] = (int)e;
}

// the reference's walk over one sorted row (src/extend.cpp:156-186); WRITE = false only counts
template <bool WRITE>
__global__ void __launch_bounds__(256)
lr_walk_kernel(const uint64_t *__restrict__ skeys, const int *__restrict__ svals, const long long *__restrict__ rj,
               const int *__restrict__ start, size_t n_rows, unsigned long long knn, int count_unique, float epsilon,
               unsigned long long *__restrict__ count, const unsigned long long *__restrict__ offs,
               long long *__restrict__ oi, long long *__restrict__ oj, float *__restrict__ od) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  unsigned long long kept = 0, unique = 0;
  float prev = 0.0f;
  const unsigned long long base = WRITE ? offs[i] : 0;
  for (int e = start[i]; e < start[i + 1]; ++e) {
    const long long j = rj[svals[e]];
    const float dist = dist_of(skeys[e]);
    if (j == (long long)i) continue;
    if (count_unique) {
      if (fabsf(__fsub_rn(dist, prev)) >= epsilon) {
        ++unique;
        prev = dist;
      }
    } else {
      unique = kept;
    }
    if (unique > knn) break;
    if (WRITE) {
      oi[base + kept] = (long long)i;
      oj[base + kept] = j;
      od[base + kept] = dist;
    }
    ++kept;
  }
  if (!WRITE) count[i] = kept;
}

// reciprocal_only (src/extend.cpp:197-236): of the kept entries, (i, j) with i < j whose (j, i) was kept
template <bool WRITE>
__global__ void __launch_bounds__(256)
lr_recip_kernel(const long long *__restrict__ kj, const float *__restrict__ kd,
                const unsigned long long *__restrict__ koffs, size_t n_rows, unsigned long long *__restrict__ count,
                const unsigned long long *__restrict__ offs, long long *__restrict__ oi, long long *__restrict__ oj,
                float *__restrict__ od) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  unsigned long long kept = 0;
  const unsigned long long base = WRITE ? offs[i] : 0;
  for (unsigned long long e = koffs[i]; e < koffs[i + 1]; ++e) {
    const long long j = kj[e];
    if (j <= (long long)i || (size_t)j >= n_rows) continue;
    bool back = false;
    for (unsigned long long f = koffs[j]; f < koffs[j + 1] && !back; ++f) back = kj[f] == (long long)i;
    if (!back) continue;
    if (WRITE) {
      oi[base + kept] = (long long)i;
      oj[base + kept] = j;
      od[base + kept] = kd[e];
    }
    ++kept;
  }
  if (!WRITE) count[i] = kept;
}

// ---- extend ------------------------------------------------------------------------------------------
// Row i < n_ref: its n_qry distances to the queries (tie order: query index), then its sparse entries (tie
// order: place in the row, after every query on a tie: the merge of src/extend.cpp:96-99 takes the query
// side when the two heads are equal).  Row n_ref + q: its row of the query square first (queries), then its
// column of the rectangle (references), same rule.
__global__ void __launch_bounds__(256)
ext_seg_kernel(const int *__restrict__ start, size_t n_ref, size_t n_qry, size_t nnz, int *__restrict__ seg) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n_ref + n_qry) return;
  seg[i] = i <= n_ref ? (int)(i * n_qry + (size_t)start[i < n_ref ? i : n_ref])
                      : (int)(n_ref * n_qry + nnz + (i - n_ref) * (n_ref + n_qry));
}

__global__ void __launch_bounds__(256)
ext_ref_dense_kernel(const float *__restrict__ qr, size_t n_ref, size_t n_qry, const int *__restrict__ seg,
                     uint64_t *__restrict__ keys, int *__restrict__ vals) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_ref * n_qry) return;
  const size_t i = t / n_qry, q = t % n_qry;
  const size_t at = (size_t)seg[i] + q;
  keys[at] = ((uint64_t)ord_of(qr[t]) << 32) | (unsigned)q;
  vals[at] = (int)(n_ref + q);
}

__global__ void __launch_bounds__(256)
ext_ref_sparse_kernel(const long long *__restrict__ ri, const long long *__restrict__ rj, const float *__restrict__ rd,
                      size_t nnz, size_t n_qry, const int *__restrict__ start, const int *__restrict__ seg,
                      uint64_t *__restrict__ keys, int *__restrict__ vals) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const size_t i = (size_t)ri[e];
  const unsigned pos = (unsigned)(e - (size_t)start[i]);
  const size_t at = (size_t)seg[i] + n_qry + pos;
  keys[at] = ((uint64_t)ord_of(rd[e]) << 32) | 0x80000000u | pos;
  vals[at] = (int)rj[e];
}

__global__ void __launch_bounds__(256)
ext_qry_kernel(const float *__restrict__ qq, const float *__restrict__ qr, size_t n_ref, size_t n_qry,
               const int *__restrict__ seg, uint64_t *__restrict__ keys, int *__restrict__ vals) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t w = n_ref + n_qry;
  if (t >= n_qry * w) return;
  const size_t q = t / w, c = t % w;
  const size_t at = (size_t)seg[n_ref + q] + c;
  if (c < n_qry) {
    keys[at] = ((uint64_t)ord_of(qq[q * n_qry + c]) << 32) | (unsigned)c;
    vals[at] = (int)(n_ref + c);
  } else {
    const size_t r = c - n_qry;
    keys[at] = ((uint64_t)ord_of(qr[r * n_qry + q]) << 32) | 0x80000000u | (unsigned)r;
    vals[at] = (int)r;
  }
}

// the first kNN entries of a sorted row that are not the row's own sample (src/extend.cpp:112-121)
template <bool WRITE>
__global__ void __launch_bounds__(256)
ext_pick_kernel(const uint64_t *__restrict__ skeys, const int *__restrict__ svals, const int *__restrict__ seg,
                size_t n_rows, unsigned long long knn, unsigned long long *__restrict__ count,
                const unsigned long long *__restrict__ offs, long long *__restrict__ oi, long long *__restrict__ oj,
                float *__restrict__ od) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  unsigned long long kept = 0;
  const unsigned long long base = WRITE ? offs[i] : 0;
  for (int e = seg[i]; e < seg[i + 1] && kept < knn; ++e) {
    const long long j = svals[e];
    if (j == (long long)i) continue;
    if (WRITE) {
      oi[base + kept] = (long long)i;
      oj[base + kept] = j;
      od[base + kept] = dist_of(skeys[e]);
    }
    ++kept;
  }
  if (!WRITE) count[i] = kept;
}


// hipCUB's two entry points as both calls use them; tmp == nullptr only sizes `bytes`
hipError_t sort_rows(void *tmp, size_t &bytes, const uint64_t *kin, uint64_t *kout, const int *vin, int *vout,
                     size_t items, size_t n_rows, const int *seg, const int *seg_end, hipStream_t s) {
  return hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)items, (int)n_rows, seg,
                                                     seg_end, 0, 64, s);
}
hipError_t scan_counts(void *tmp, size_t &bytes, const unsigned long long *count, unsigned long long *sums, size_t n,
                       hipStream_t s) {
  return hipcub::DeviceScan::InclusiveSum(tmp, bytes, count, sums, (int)n, s);
}

// The work buffers of one call, all of SLOT_SPARSE and carved ONCE (a second carve that grew the slot would free the
// block under the first one's pointers): row starts, sort segments, the bad-rows flag, both key / value pairs, row
// counts and offsets, what `more` appends, and hipCUB's temporary storage for the sort and the scan.
struct SparseWork {
  int *start, *seg, *flag;
  uint64_t *kin, *kout;
  int *vin, *vout;
  unsigned long long *cnt, *offs;
  char *tmp;
  size_t tmp_bytes;
};
template <typename More>
int sparse_work(int dev, SparseWork &w, size_t starts, size_t segs, size_t items, size_t rows, hipStream_t s,
                More &&more) {
  size_t sort_tmp = 0, scan_tmp = 0;
  PPK_HIP(sort_rows(nullptr, sort_tmp, nullptr, nullptr, nullptr, nullptr, items, rows, nullptr, nullptr, s));
  PPK_HIP(scan_counts(nullptr, scan_tmp, nullptr, nullptr, rows, s));
  w.tmp_bytes = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
  return ppk_scratch_carve(dev, SLOT_SPARSE, [&](Carve &c) {
    c.take(w.start, starts).take(w.seg, segs).take(w.flag, 1).take(w.kin, items).take(w.kout, items);
    c.take(w.vin, items).take(w.vout, items).take(w.cnt, rows).take(w.offs, rows + 1);
    more(c);
    c.take(w.tmp, w.tmp_bytes + 256);
  });
}

// w.start of a row-sorted COO.  The one read-back in front of the totals: a matrix whose rows do not ascend gives
// garbage starts, so it is refused here, before any kernel indexes by them.
int row_starts(int dev, const SparseWork &w, const long long *d_ri, size_t nnz, size_t n_rows, const char *limit,
               hipStream_t s) {
  PPK_HIP(hipMemsetAsync(w.flag, 0, 4, s));
  const size_t most = nnz > n_rows + 1 ? nnz : n_rows + 1;
  hipLaunchKernelGGL(row_start_kernel, dim3(grid_for(most, 256, ~0u)), dim3(256), 0, s, d_ri, nnz, n_rows, w.start,
                     w.flag);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if (int rc = ppk_read_back(dev, s, {{w.flag, 4}}, &h)) return rc;
  if ((int)h[0])
    return ppk_fail(PPK_ERR_ARG, std::string("sparse matrix: row indices must be ascending and below ") + limit);
  return PPK_OK;
}

// counts[n] -> offsets[n + 1] (exclusive)
int offsets_of(const SparseWork &w, const unsigned long long *count, unsigned long long *offs, size_t n,
               hipStream_t s) {
  PPK_HIP(hipMemsetAsync(offs, 0, (n + 1) * 8, s));
  size_t bytes = w.tmp_bytes;
  PPK_HIP(scan_counts(w.tmp, bytes, count, offs + 1, n, s));
  return PPK_OK;
}

// lowerRank of device arrays: the triplets into d_oi / d_oj / d_od (room for nnz each: a row keeps no more than it
// has), their number into *total (host) -- the call's second and last synchronisation
int lower_rank_dev(const long long *d_ri, const long long *d_rj, const float *d_rd, size_t nnz, size_t n,
                   unsigned long long knn, int reciprocal_only, int count_unique, float epsilon, long long *d_oi,
                   long long *d_oj, float *d_od, unsigned long long *total, hipStream_t s) {
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  SparseWork w;
  // what the walk keeps: the result itself, or (as many at most) the reciprocal pass's input
  long long *ki = d_oi, *kj = d_oj;
  float *kd = d_od;
  unsigned long long *offs2 = nullptr;
  int rc = sparse_work(dev, w, n + 1, 0, nnz, n, s, [&](Carve &c) {
    if (reciprocal_only) c.take(ki, nnz).take(kj, nnz).take(kd, nnz).take(offs2, n + 1);
  });
  if (rc == PPK_OK) rc = row_starts(dev, w, d_ri, nnz, n, "n_samples", s);
  if (rc != PPK_OK) return rc;
  hipLaunchKernelGGL(lr_keys_kernel, dim3(grid_for(nnz, 256, ~0u)), dim3(256), 0, s, d_ri, d_rd, nnz, w.start, w.kin,
                     w.vin);
  PPK_HIP(hipGetLastError());
  size_t bytes = w.tmp_bytes;
  PPK_HIP(sort_rows(w.tmp, bytes, w.kin, w.kout, w.vin, w.vout, nnz, n, w.start, w.start + 1, s));
  const dim3 grid(grid_for(n, 256, ~0u));
  hipLaunchKernelGGL(lr_walk_kernel<false>, grid, dim3(256), 0, s, w.kout, w.vout, d_rj, w.start, n, knn, count_unique,
                     epsilon, w.cnt, nullptr, nullptr, nullptr, nullptr);
  if ((rc = offsets_of(w, w.cnt, w.offs, n, s)) != PPK_OK) return rc;
  hipLaunchKernelGGL(lr_walk_kernel<true>, grid, dim3(256), 0, s, w.kout, w.vout, d_rj, w.start, n, knn, count_unique,
                     epsilon, nullptr, w.offs, ki, kj, kd);
  PPK_HIP(hipGetLastError());
  const unsigned long long *d_total = w.offs + n;
  if (reciprocal_only) {
    // (the walk's counts have been scanned: w.cnt is free again)
    hipLaunchKernelGGL(lr_recip_kernel<false>, grid, dim3(256), 0, s, kj, kd, w.offs, n, w.cnt, nullptr, nullptr,
                       nullptr, nullptr);
    if ((rc = offsets_of(w, w.cnt, offs2, n, s)) != PPK_OK) return rc;
    hipLaunchKernelGGL(lr_recip_kernel<true>, grid, dim3(256), 0, s, kj, kd, w.offs, n, nullptr, offs2, d_oi, d_oj,
                       d_od);
    PPK_HIP(hipGetLastError());
    d_total = offs2 + n;
  }
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{d_total, 8}}, &h)) != PPK_OK) return rc;
  *total = h[0];
  return PPK_OK;
}

// extend of device arrays: the triplets into d_oi / d_oj / d_od (room for min(items, n_rows * knn) each), their
// number into *total (host) -- the call's second and last synchronisation
int extend_dev(const long long *d_ri, const long long *d_rj, const float *d_rd, size_t nnz, const float *d_qq,
               const float *d_qr, size_t n_ref, size_t n_qry, unsigned long long knn, long long *d_oi, long long *d_oj,
               float *d_od, unsigned long long *total, hipStream_t s) {
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t n_rows = n_ref + n_qry, items = n_ref * n_qry + nnz + n_qry * n_rows;
  SparseWork w;
  int rc = sparse_work(dev, w, n_ref + 1, n_rows + 1, items, n_rows, s, [](Carve &) {});
  if (rc == PPK_OK) rc = row_starts(dev, w, d_ri, nnz, n_ref, "the number of references", s);
  if (rc != PPK_OK) return rc;
  hipLaunchKernelGGL(ext_seg_kernel, dim3(grid_for(n_rows + 1, 256, ~0u)), dim3(256), 0, s, w.start, n_ref, n_qry, nnz,
                     w.seg);
  if (n_ref * n_qry)
    hipLaunchKernelGGL(ext_ref_dense_kernel, dim3(grid_for(n_ref * n_qry, 256, ~0u)), dim3(256), 0, s, d_qr, n_ref,
                       n_qry, w.seg, w.kin, w.vin);
  if (nnz)
    hipLaunchKernelGGL(ext_ref_sparse_kernel, dim3(grid_for(nnz, 256, ~0u)), dim3(256), 0, s, d_ri, d_rj, d_rd, nnz,
                       n_qry, w.start, w.seg, w.kin, w.vin);
  if (n_qry)
    hipLaunchKernelGGL(ext_qry_kernel, dim3(grid_for(n_qry * n_rows, 256, ~0u)), dim3(256), 0, s, d_qq, d_qr, n_ref,
                       n_qry, w.seg, w.kin, w.vin);
  PPK_HIP(hipGetLastError());
  size_t bytes = w.tmp_bytes;
  PPK_HIP(sort_rows(w.tmp, bytes, w.kin, w.kout, w.vin, w.vout, items, n_rows, w.seg, w.seg + 1, s));
  const dim3 grid(grid_for(n_rows, 256, ~0u));
  hipLaunchKernelGGL(ext_pick_kernel<false>, grid, dim3(256), 0, s, w.kout, w.vout, w.seg, n_rows, knn, w.cnt, nullptr,
                     nullptr, nullptr, nullptr);
  if ((rc = offsets_of(w, w.cnt, w.offs, n_rows, s)) != PPK_OK) return rc;
  hipLaunchKernelGGL(ext_pick_kernel<true>, grid, dim3(256), 0, s, w.kout, w.vout, w.seg, n_rows, knn, nullptr, w.offs,
                     d_oi, d_oj, d_od);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{w.offs + n_rows, 8}}, &h)) != PPK_OK) return rc;
  *total = h[0];
  return PPK_OK;
}

int check_coo(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz) {
  if (nnz && (!rr_i || !rr_j || !rr_d)) return ppk_fail(PPK_ERR_ARG, "sparse matrix: NULL array");
  if (nnz >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "sparse matrix: fewer than 2^31 entries supported");
  return PPK_OK;
}

int copy_out(const long long *d_oi, const long long *d_oj, const float *d_od, unsigned long long total,
             long long *i_out, long long *j_out, float *d_out, size_t cap, size_t *n_out) {
  *n_out = (size_t)total;
  if (total > cap) return ppk_fail(PPK_ERR_CAPACITY, "output too small: need " + std::to_string(total));
  if (!total) return PPK_OK;
  if (!i_out || !j_out || !d_out) return ppk_fail(PPK_ERR_ARG, "NULL output");
  PPK_HIP(hipMemcpy(i_out, d_oi, total * 8, hipMemcpyDeviceToHost));
  PPK_HIP(hipMemcpy(j_out, d_oj, total * 8, hipMemcpyDeviceToHost));
  PPK_HIP(hipMemcpy(d_out, d_od, total * 4, hipMemcpyDeviceToHost));
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_lower_rank(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
                              size_t n_samples, size_t knn, int reciprocal_only, int count_unique_distances,
                              float epsilon, int device_id, long long *i_out, long long *j_out, float *d_out,
                              size_t cap, size_t *n_out) {
  if (!n_out) return ppk_fail(PPK_ERR_ARG, "n_out is NULL");
  *n_out = 0;
  if (int rc = check_coo(rr_i, rr_j, rr_d, nnz)) return rc;
  if (n_samples == 0 || nnz == 0) return PPK_OK;
  if (n_samples >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, "too many samples");
  long long *d_ri, *d_rj, *d_oi, *d_oj;
  float *d_rd, *d_od;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_ri, nnz).take(d_rj, nnz).take(d_rd, nnz).take(d_oi, nnz).take(d_oj, nnz).take(d_od, nnz);
  }, [&]() -> int {
    int rc = ppk_check_arch(device_id);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_ri, rr_i, nnz * 8, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_rj, rr_j, nnz * 8, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_rd, rr_d, nnz * 4, nullptr);
    unsigned long long total = 0;
    if (rc == PPK_OK)
      rc = lower_rank_dev(d_ri, d_rj, d_rd, nnz, n_samples, knn, reciprocal_only, count_unique_distances, epsilon,
                          d_oi, d_oj, d_od, &total, nullptr);
    return rc != PPK_OK ? rc : copy_out(d_oi, d_oj, d_od, total, i_out, j_out, d_out, cap, n_out);
  });
}

extern "C" int ppk_extend(const long long *rr_i, const long long *rr_j, const float *rr_d, size_t nnz,
                          const float *qq_square, const float *qr_rect, size_t n_ref, size_t n_qry, size_t knn,
                          int device_id, long long *i_out, long long *j_out, float *d_out, size_t cap,
                          size_t *n_out) {
  if (!n_out) return ppk_fail(PPK_ERR_ARG, "n_out is NULL");
  *n_out = 0;
  if (int rc = check_coo(rr_i, rr_j, rr_d, nnz)) return rc;
  const size_t n_rows = n_ref + n_qry;
  if (n_rows == 0 || knn == 0) return PPK_OK;
  if (n_qry && (!qq_square || (n_ref && !qr_rect))) return ppk_fail(PPK_ERR_ARG, "ppk_extend: NULL dense matrix");
  const size_t items = n_ref * n_qry + nnz + n_qry * (n_ref + n_qry);
  if (items >= (size_t)0x7fffffff || n_rows >= (size_t)0x7fffffff)
    return ppk_fail(PPK_ERR_ARG, "ppk_extend: fewer than 2^31 candidate distances supported (n_ref*n_qry + nnz + n_qry*(n_ref+n_qry))");
  if (items == 0) return PPK_OK;      // references alone and an empty sparse matrix: no candidate, no entry
  // a row keeps at most knn of its candidates
  const size_t most = knn < items && n_rows * knn < items ? n_rows * knn : items;
  long long *d_ri, *d_rj, *d_oi, *d_oj;
  float *d_rd, *d_qq, *d_qr, *d_od;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_ri, nnz).take(d_rj, nnz).take(d_rd, nnz).take(d_qq, n_qry * n_qry).take(d_qr, n_ref * n_qry);
    c.take(d_oi, most).take(d_oj, most).take(d_od, most);
  }, [&]() -> int {
    int rc = ppk_check_arch(device_id);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_ri, rr_i, nnz * 8, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_rj, rr_j, nnz * 8, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_rd, rr_d, nnz * 4, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_qq, qq_square, n_qry * n_qry * 4, nullptr);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_qr, qr_rect, n_ref * n_qry * 4, nullptr);
    unsigned long long total = 0;
    if (rc == PPK_OK)
      rc = extend_dev(d_ri, d_rj, d_rd, nnz, d_qq, d_qr, n_ref, n_qry, knn, d_oi, d_oj, d_od, &total, nullptr);
    return rc != PPK_OK ? rc : copy_out(d_oi, d_oj, d_od, total, i_out, j_out, d_out, cap, n_out);
  });
}
