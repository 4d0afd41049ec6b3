// Bookkeeping of the dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) per (kernel, device): which pairs have been
// raised above the 64 KB every kernel starts with, and to how many bytes.  The attribute belongs to a kernel ON A DEVICE, so a
// per-process flag leaves every device after the first at 64 KB.  Nothing from HIP in here: crct_lds_limit (crct_internal.h,
// streams.hip) asks needs_raise, sets the attribute and calls record; tests/test_lds_limit_cpu.py runs this header alone.
//
// A fixed open-addressed table of atomics: the look-up on the launch path takes no lock (forward runs on the caller's thread, backward
// on autograd's).  A kernel beyond MAX_KERNELS or a device beyond MAX_DEVICES is never recorded and so always "needs raising": slow, not wrong.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace crct {

constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024;

class LdsLimits {
 public:
  static constexpr int MAX_KERNELS = 256;      // a power of two (slot_of); the library holds ~60 kernels that go above 64 KB
  static constexpr int MAX_DEVICES = 16;

  // does a launch of `kern` on `device` with up to `bytes` of dynamic LDS need the attribute raised first?
  bool needs_raise(const void* kern, int device, size_t bytes) const {
    if (bytes <= LDS_DEFAULT_LIMIT) return false;
    if (device < 0 || device >= MAX_DEVICES) return true;
    for (unsigned i = slot_of(kern), n = 0; n < MAX_KERNELS; ++n, i = (i + 1) & (MAX_KERNELS - 1)) {
      const void* k = rows_[i].kern.load(std::memory_order_acquire);
      if (k == kern) return rows_[i].limit[device].load(std::memory_order_acquire) < bytes;
      if (!k) return true;
    }
    return true;
  }

  // the attribute of (kern, device) has been set to `bytes`
  void record(const void* kern, int device, size_t bytes) {
    if (device < 0 || device >= MAX_DEVICES) return;
    for (unsigned i = slot_of(kern), n = 0; n < MAX_KERNELS; ++n, i = (i + 1) & (MAX_KERNELS - 1)) {
      const void* k = rows_[i].kern.load(std::memory_order_acquire);
      if (!k && rows_[i].kern.compare_exchange_strong(k, kern, std::memory_order_acq_rel)) k = kern;      // (on failure k = the winner's kernel)
      if (k != kern) continue;
      std::atomic<size_t>& lim = rows_[i].limit[device];
      size_t old = lim.load(std::memory_order_relaxed);
      while (old < bytes && !lim.compare_exchange_weak(old, bytes, std::memory_order_release, std::memory_order_relaxed)) {}
      return;
    }
  }

 private:
  struct Row {
    std::atomic<const void*> kern{nullptr};
    std::atomic<size_t> limit[MAX_DEVICES] = {};
  };
  static unsigned slot_of(const void* kern) { return (unsigned)(((uintptr_t)kern >> 4) * 0x9E3779B97F4A7C15ull >> 40) & (MAX_KERNELS - 1); }
  Row rows_[MAX_KERNELS];
};

}  // namespace crct
