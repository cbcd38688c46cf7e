// What a plan owns on the device and builds on first use: the buffer owner (DevBuf), the state of a
// lazily built schedule (Lazy); and what plans share per device or process: the order of single
// launches (FusedSerial) and the pool of watchdog report words.  Included by ntt_plan.cpp alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "plan_knobs.hpp"

namespace {

// One device allocation: move-only, a pointer and its byte count, freed when its owner goes.  A plan's
// buffers are its members, so none can be left off a list of frees; ~PlanImpl makes the plan's device
// current before they go and ~PlanBase restores the caller's after.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  ~DevBuf() { reset(); }
  // a fresh allocation of `bytes` (what was held is freed first); on failure the buffer is empty and
  // the sticky HIP error is cleared, so that the next launch check does not report it
  bool alloc(size_t bytes) {
    reset();
    if (hipMalloc(&p_, bytes) != hipSuccess) {
      p_ = nullptr;
      (void)hipGetLastError();
      return false;
    }
    bytes_ = bytes;
    return true;
  }
  // at least `bytes`: nothing when already that large, else free and allocate (contents are not kept)
  bool grow(size_t bytes) { return (p_ && bytes <= bytes_) || alloc(bytes); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  template <class T = uint32_t>
  T* get() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// State built on a plan's first use of it: not tried, ready, or unavailable (tried once, never again)
class Lazy {
 public:
  template <class Build>
  bool ready(Build&& build) {
    if (s_ == kNotTried) s_ = build() ? kReady : kUnavailable;
    return s_ == kReady;
  }
 private:
  enum : uint8_t { kNotTried, kReady, kUnavailable } s_ = kNotTried;
};

// ------------------------------------------------------------------------------ single-launch order
// The single launches (k_fused3 / k_fused3b / k_fused3bi / k_fused2b / k_fused2bi) wait across
// workgroups, so each assumes its workgroups own the device: two of them enqueued on two streams could
// have their workgroups dispatched interleaved, each holding part of the CUs, and both would wait for
// the other's workgroups until the watchdog gave up (NTT_ERR_DEVICE).  The library therefore orders
// them per device, under one lock: a single launch on another stream than the device's previous one
// first makes its stream wait for everything enqueued so far on that previous stream (an event
// recorded there at this moment), which includes the previous single launch.  Launches on one stream
// are in order already and pay nothing: an event recorded after every launch cost 4.5 us of device time
// per call (a marker packet behind the kernel; profiles/r06_c2/).  A previous stream that has been
// destroyed (hipStreamGetFlags fails) has finished its work.  Work of other kinds is not ordered.
// (The in-place forms also check residency before their first store, for CUs held by anything else:
// ntt_kernels_impl.hpp residency_wait.)
class FusedSerial {
 public:
  FusedSerial(int device, hipStream_t st) : lk_(mu()), s_(knob::fused_order() ? slot(device) : nullptr), st_(st) {
    if (!s_ || !s_->used || s_->last == st) return;
    unsigned fl = 0;
    if (hipStreamGetFlags(s_->last, &fl) != hipSuccess) {  // gone: its work is done
      (void)hipGetLastError();
      return;
    }
    if (!s_->ev && hipEventCreateWithFlags(&s_->ev, hipEventDisableTiming) != hipSuccess) {
      s_->ev = nullptr;
      (void)hipGetLastError();
      return;
    }
    if (hipEventRecord(s_->ev, s_->last) == hipSuccess) (void)hipStreamWaitEvent(st, s_->ev, 0);
  }
  void done(hipError_t launched) {
    if (!s_ || launched != hipSuccess) return;
    s_->last = st_;
    s_->used = true;
  }

 private:
  struct Slot {
    hipStream_t last = nullptr;  // the stream of the device's latest single launch
    bool used = false;
    hipEvent_t ev = nullptr;     // process-lifetime, like the plan cache
  };
  static std::mutex& mu() {
    static std::mutex* m = new std::mutex;
    return *m;
  }
  static Slot* slot(int device) {
    static Slot* slots = new Slot[64];
    return (device >= 0 && device < 64) ? &slots[device] : nullptr;
  }
  std::lock_guard<std::mutex> lk_;
  Slot* s_;
  hipStream_t st_;
};

// ------------------------------------------------------------------------------ watchdog words
// One 4-KiB mapped, coherent pinned page per 1024 plans that use inter-workgroup waits; a plan takes
// a 4-byte slot when it first builds such a schedule and returns it when destroyed.  The pages are
// never freed: nothing is released during process teardown, where the HIP runtime (and a profiler
// such as rocprofv3) may already be gone.
static std::mutex g_watch_mu;
static std::vector<uint32_t*> g_watch_free;
static uint32_t* watch_slot_acquire() {
  std::lock_guard<std::mutex> lk(g_watch_mu);
  if (g_watch_free.empty()) {
    void* page = nullptr;
    if (hipHostMalloc(&page, 4096, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess)
      return nullptr;
    auto* w = static_cast<uint32_t*>(page);
    for (int i = 1023; i >= 0; --i) {
      w[i] = 0u;
      g_watch_free.push_back(w + i);
    }
  }
  uint32_t* s = g_watch_free.back();
  g_watch_free.pop_back();
  *s = 0u;
  return s;
}
static void watch_slot_release(uint32_t* s) {
  if (!s) return;
  std::lock_guard<std::mutex> lk(g_watch_mu);
  g_watch_free.push_back(s);
}

}  // namespace
