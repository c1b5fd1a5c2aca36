// The state libppk_hip.so keeps per device, shared by its translation units (declared in ppk_internal.h): the one
// device-id check, the grow-only blocks, the scratch slots with the PpkCall scope that guards them, the read-back
// block, the fit tables' key, the LDS opt-ins, the arch verdict, the geometry and the polled ticket blocks.
// Host code only: no kernel is defined here.
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>

#include "ppk_internal.h"

int ppk_check_device(int dev) {
  if (dev >= 0 && dev < PPK_MAX_DEVICES) return PPK_OK;
  return ppk_fail(PPK_ERR_ARG, "device id " + std::to_string(dev) + " out of range [0, " + std::to_string(PPK_MAX_DEVICES) + ")");
}

// ---- grow-only blocks, lazily created events ------------------------------------------------------------------------
hipError_t PpkDeviceBuf::grow(size_t want, size_t slack) {
  if (bytes >= want) return hipSuccess;
  if (p) (void)hipDeviceSynchronize();      // earlier launches may still read the old block
  release();
  const hipError_t e = hipMalloc(&p, want + slack);
  if (e == hipSuccess) bytes = want + slack;
  else p = nullptr;
  return e;
}
void PpkDeviceBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}

hipError_t PpkPinnedBuf::grow(size_t want, size_t slack, unsigned flags) {
  if (bytes >= want) return hipSuccess;
  if (p) (void)hipDeviceSynchronize();      // an earlier copy may still be on its way into the old block
  release();
  const hipError_t e = hipHostMalloc(&p, want + slack, flags);
  if (e == hipSuccess) bytes = want + slack;
  else p = nullptr;
  return e;
}
void PpkPinnedBuf::release() {
  if (p) (void)hipHostFree(p);
  p = nullptr;
  bytes = 0;
}

hipError_t ppk_event_get(hipEvent_t *e) { return *e ? hipSuccess : hipEventCreateWithFlags(e, hipEventDisableTiming); }
void ppk_event_release(hipEvent_t *e) {
  if (*e) (void)hipEventDestroy(*e);
  *e = nullptr;
}

void PpkDeviceVisit::enter() {
  if (guard) return;
  guard.reset(new DeviceGuard(dev));
  (void)hipDeviceSynchronize();
}

// ---- the table --------------------------------------------------------------------------------------------------------
namespace {
// Per-device scratch (log-J table, edge bitmask, sort buffers ...): grow-only blocks shared by all
// calls on a device.  Two rules make that safe for any caller:
//  * every entry point that touches scratch holds the device's (recursive) mutex for the length of
//    the call -- it only enqueues, so that is microseconds -- through a PpkCall scope, which also
//    names the stream the call enqueues on;
//  * a slot remembers, as an event recorded when the call that used it returns, the last work
//    enqueued on it; a later call on a DIFFERENT stream makes its stream wait for that event
//    before it re-uses (or re-allocates) the block.  Calls on one stream are ordered anyway.
struct Scratch {
  PpkDeviceBuf buf;
  hipEvent_t ev = nullptr;      // recorded after the last call that used the slot
  hipStream_t last = nullptr;   // ... on this stream
  bool recorded = false;
};
std::mutex g_arch_mu, g_geometry_mu;
struct DevState {
  std::recursive_mutex mu;      // held by a PpkCall scope
  // -- guarded by mu:
  Scratch slot[SLOT_COUNT];
  // the fit tables sitting in SLOT_LUT: key of what they were built from (0 = nothing valid) and the
  // block they sit in -- a call with the same k list, random table and options skips the rebuild
  uint64_t lut_key = 0;
  const void *lut_ptr = nullptr;
  PpkPinnedBuf read_back;                         // the block of ppk_read_back
  std::map<const void *, bool> lds_opt_in;        // the kernels' dynamic-LDS opt-ins (ppk_lds_opt_in)
  // The polled ticket blocks, one per user, and the counter they share.  Like the read-back block these pinned blocks
  // are never freed: ppk_release_scratch returns device memory, and a pinned word may still be named by a kernel.
  PpkPinnedBuf ticket_block[PPK_TICKET_USERS];
  unsigned long long tickets = 0;
  // -- guarded by g_arch_mu:
  int arch_verdict = 0;                           // 0 unknown, 1 ok, -1 refused
  std::string arch_why;
  // -- written once under g_geometry_mu, read after geometry_ready:
  PpkGeometry geometry = {};
  std::atomic<int> geometry_ready{0};
};
PpkPerDevice<DevState> g_dev;

struct CallCtx {
  int dev = -1;
  hipStream_t s = nullptr;
  unsigned long long touched = 0;     // one bit per scratch slot
};
thread_local CallCtx tl_call;
thread_local uint64_t tl_lut_pending_key = 0;
thread_local const void *tl_lut_pending_ptr = nullptr;
}  // namespace

int ppk_scratch_get(int dev, int slot, size_t bytes, void **out) {
  if (int rc = ppk_check_device(dev)) return rc;
  if (slot < 0 || slot >= SLOT_COUNT) return ppk_fail(PPK_ERR_ARG, "internal: no such scratch slot");
  if (tl_call.dev != dev) return ppk_fail(PPK_ERR_STATE, "internal: scratch requested outside a PpkCall scope");
  DevState &ds = g_dev.at(dev);
  Scratch &s = ds.slot[slot];
  if (s.recorded && s.last != tl_call.s) {
    // the previous user ran on another stream: order this call's work after it
    hipError_t e = hipStreamWaitEvent(tl_call.s, s.ev, 0);
    if (e != hipSuccess) (void)hipDeviceSynchronize();
  }
  if (s.buf.bytes < bytes) {
    if (slot == SLOT_LUT) {          // the tables a later call might re-use go with the block
      ds.lut_key = 0;
      ds.lut_ptr = nullptr;
    }
    hipError_t e = s.buf.grow(bytes, bytes / 4 + 4096);
    if (e != hipSuccess) return ppk_fail(PPK_ERR_HIP, std::string("hipMalloc(scratch): ") + hipGetErrorString(e));
    // the per-tile counters of the k-split kernel start at zero and every launch leaves them there
    if (slot == SLOT_TICKETS && hipMemset(s.buf.p, 0, s.buf.bytes) != hipSuccess) return ppk_fail(PPK_ERR_HIP, "hipMemset(scratch) failed");
    // the slot bitmap of the wide-k kernel likewise
    if (slot == SLOT_WIDE && hipMemset(s.buf.p, 0, 4096) != hipSuccess) return ppk_fail(PPK_ERR_HIP, "hipMemset(scratch) failed");
  }
  tl_call.touched |= 1ull << slot;
  *out = s.buf.p;
  return PPK_OK;
}

int ppk_read_back(int dev, hipStream_t s, std::initializer_list<PpkCopy> copies, const unsigned long long **words) {
  if (int rc = ppk_check_device(dev)) return rc;
  if (tl_call.dev != dev) return ppk_fail(PPK_ERR_STATE, "internal: read-back requested outside a PpkCall scope");
  size_t bytes = 0;
  for (const PpkCopy &c : copies) bytes += (c.bytes + 7) & ~(size_t)7;
  PpkPinnedBuf &block = g_dev.at(dev).read_back;
  const hipError_t e = block.grow(align256(bytes), align256(bytes) / 4 + 4096);      // as the scratch slots grow
  if (e != hipSuccess) return ppk_fail(PPK_ERR_HIP, std::string("hipHostMalloc(read-back): ") + hipGetErrorString(e));
  char *at = static_cast<char *>(block.p);
  for (const PpkCopy &c : copies) {
    PPK_HIP(hipMemcpyAsync(at, c.src, c.bytes, hipMemcpyDeviceToHost, s));
    at += (c.bytes + 7) & ~(size_t)7;
  }
  PPK_HIP(hipStreamSynchronize(s));
  *words = static_cast<const unsigned long long *>(block.p);
  return PPK_OK;
}

bool ppk_lds_opt_in(const void *kernel, int dev, int bytes) {
  if (ppk_check_device(dev) != PPK_OK) return false;
  DevState &ds = g_dev.at(dev);
  std::lock_guard<std::recursive_mutex> lk(ds.mu);
  auto it = ds.lds_opt_in.find(kernel);
  if (it != ds.lds_opt_in.end()) return it->second;
  const bool ok = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  (void)hipGetLastError();
  ds.lds_opt_in[kernel] = ok;
  return ok;
}

bool ppk_lut_ready(int dev, uint64_t key, const void *d_lut) {
  DevState &ds = g_dev.at(dev);
  if (ds.lut_key == key && ds.lut_ptr == d_lut) return true;
  ds.lut_key = 0;        // nothing valid until the launcher has really built the tables (ppk_lut_commit)
  tl_lut_pending_key = key;
  tl_lut_pending_ptr = d_lut;
  return false;
}

// lut_kernel has been enqueued for the tables ppk_lut_ready announced: they may be re-used
void ppk_lut_commit(int dev, const void *d_lut) {
  if (tl_lut_pending_ptr != d_lut) return;
  g_dev.at(dev).lut_key = tl_lut_pending_key;
  g_dev.at(dev).lut_ptr = d_lut;
}

PpkCall::PpkCall(int dev, hipStream_t s) : dev_(dev), prev_dev_(tl_call.dev), prev_s_(tl_call.s), prev_touched_(tl_call.touched) {
  g_dev.at(dev_).mu.lock();
  tl_call.dev = dev_;
  tl_call.s = s;
  tl_call.touched = 0;
}

PpkCall::~PpkCall() {
  for (int k = 0; k < SLOT_COUNT; ++k) {
    if (!(tl_call.touched & (1ull << k))) continue;
    Scratch &sc = g_dev.at(dev_).slot[k];
    if (ppk_event_get(&sc.ev) != hipSuccess) sc.ev = nullptr;
    sc.recorded = sc.ev && hipEventRecord(sc.ev, tl_call.s) == hipSuccess;
    sc.last = tl_call.s;
  }
  // an enclosing scope on the same device (a host wrapper calling a device entry point) has
  // touched what its callee touched
  const unsigned long long mine = tl_call.touched;
  tl_call.dev = prev_dev_;
  tl_call.s = prev_s_;
  tl_call.touched = prev_touched_ | (prev_dev_ == dev_ ? mine : 0ull);
  g_dev.at(dev_).mu.unlock();
}

// Everything kept on a device goes in one visit: the device is selected and drained once, by the first holder that
// has something to free (PpkDeviceVisit), and each holder releases under the lock that guards it.
extern "C" int ppk_release_scratch(void) {
  ppk_db_cache_clear();
  ppk_parked_clear();
  g_dev.each([](int d, DevState &ds) {
    PpkDeviceVisit visit(d);
    ppk_host_bufs_release(visit);
    std::lock_guard<std::recursive_mutex> lk(ds.mu);
    for (Scratch &sc : ds.slot) {
      if (!sc.buf.p && !sc.ev) continue;
      visit.enter();
      sc.buf.release();
      ppk_event_release(&sc.ev);
      sc = Scratch();      // (its stream and "recorded" too)
    }
    // a re-allocated block commonly comes back at the same address: without this the next call with the
    // same k list and table would take the freed tables for valid (ppk_lut_ready) and skip lut_kernel
    ds.lut_key = 0;
    ds.lut_ptr = nullptr;
  });
  return PPK_OK;
}

// ---- the only supported target: gfx950 (MI355X), wave64 ---------------------------------------
// Every kernel in this library is compiled for gfx950 alone and the tile kernels are fixed-register
// wave64 instruction streams; on anything else the launches would fail with "no kernel image" (or
// worse).  Checked once per device, loudly.
int ppk_check_arch(int device_id) {
  if (int rc = ppk_check_device(device_id)) return rc;
  DevState &ds = g_dev.at(device_id);
  std::lock_guard<std::mutex> lk(g_arch_mu);
  if (ds.arch_verdict == 0) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) {
      ds.arch_why = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
      ds.arch_verdict = -1;
    } else if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 || prop.warpSize != 64) {
      ds.arch_why = std::string("device ") + std::to_string(device_id) + " is " + prop.gcnArchName +
                    " (wavefront " + std::to_string(prop.warpSize) +
                    "): libppk_hip.so is built for gfx950 / wave64 (MI355X) only";
      ds.arch_verdict = -1;
    } else {
      ds.arch_verdict = 1;
    }
  }
  if (ds.arch_verdict < 0) return ppk_fail(PPK_ERR_HIP, ds.arch_why);
  return PPK_OK;
}

// the device's geometry, measured once (ppk_measure_geometry, ppk_dist.hip)
const PpkGeometry &ppk_geometry(int dev) {
  DevState &ds = g_dev.at(dev);
  if (ds.geometry_ready.load(std::memory_order_acquire)) return ds.geometry;
  std::lock_guard<std::mutex> lk(g_geometry_mu);
  if (!ds.geometry_ready.load(std::memory_order_relaxed)) {
    ds.geometry = ppk_measure_geometry(dev);
    ds.geometry_ready.store(1, std::memory_order_release);
  }
  return ds.geometry;
}

// ---- the polled ticket (ppk_internal.h) ----------------------------------------------------------------------------
void *ppk_ticket_block(int dev, PpkTicketUser user) {
  PpkPinnedBuf &b = g_dev.at(dev).ticket_block[user];
  // coherent host memory: the host reads it while the stream is still running
  if (!b.p && b.grow(256, 0, hipHostMallocCoherent) == hipSuccess) memset(b.p, 0, 256);
  return b.p;
}

unsigned long long ppk_next_ticket(int dev) { return ++g_dev.at(dev).tickets; }

int ppk_wait_ticket(hipStream_t s, const volatile unsigned long long *word, unsigned long long ticket, long long budget_us,
                    const char *what) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0;; ++spin) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == ticket) return PPK_OK;
    if ((spin & 1023u) == 1023u) {
      if (hipStreamQuery(s) != hipErrorNotReady) break;      // done, or failed: let the drain say which
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(budget_us)) break;
    }
    __builtin_ia32_pause();
  }
  PPK_HIP(hipStreamSynchronize(s));
  if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != ticket) return ppk_fail(PPK_ERR_HIP, what);
  return PPK_OK;
}
