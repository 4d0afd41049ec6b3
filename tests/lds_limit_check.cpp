// Stand-alone check of cqa-crct_amd/csrc/lds_limit.h (built and run by tests/test_lds_limit_cpu.py with the host compiler: no HIP).
// Prints one "<case> ok" / "<case> FAIL" line per case; the exit status is the number of failures.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "lds_limit.h"

namespace {
int failures = 0;
void check(const char* name, bool ok) {
  printf("%s %s\n", name, ok ? "ok" : "FAIL");
  failures += !ok;
}
constexpr size_t KB = 1024;
char kernels[8];      // eight distinct addresses stand for eight kernels
}  // namespace

int main() {
  static crct::LdsLimits t;
  const void *k = &kernels[0], *k2 = &kernels[1];
  check("first_use_needs_raise", t.needs_raise(k, 0, 96 * KB));
  t.record(k, 0, 96 * KB);
  check("recorded_key_is_settled", !t.needs_raise(k, 0, 96 * KB) && !t.needs_raise(k, 0, 80 * KB));
  check("other_device_needs_raise", t.needs_raise(k, 1, 96 * KB));
  check("more_bytes_need_raise_again", t.needs_raise(k, 0, 150 * KB));
  t.record(k, 0, 150 * KB);
  t.record(k, 0, 96 * KB);      // a lower record never lowers the limit
  check("limit_only_rises", !t.needs_raise(k, 0, 150 * KB) && t.needs_raise(k, 0, 160 * KB));
  check("second_kernel_is_independent", t.needs_raise(k2, 0, 96 * KB) && !t.needs_raise(k, 0, 96 * KB));
  t.record(k2, 0, 96 * KB);
  check("second_kernel_settled", !t.needs_raise(k2, 0, 96 * KB) && t.needs_raise(k2, 1, 96 * KB));
  bool small = true;
  for (size_t b : {size_t(0), size_t(1), 48 * KB, 64 * KB})
    for (int d : {0, 1, 5}) small = small && !t.needs_raise(k, d, b) && !t.needs_raise(&kernels[7], d, b);
  check("up_to_64k_never_needs_raise", small && t.needs_raise(&kernels[7], 0, 64 * KB + 1));
  check("device_out_of_range_always_needs_raise", (t.record(k, crct::LdsLimits::MAX_DEVICES, 96 * KB), t.needs_raise(k, crct::LdsLimits::MAX_DEVICES, 96 * KB)) &&
                                                      (t.record(k, -1, 96 * KB), t.needs_raise(k, -1, 96 * KB)));

  // two threads: disjoint keys (each its own kernels on device 2) and equal keys (kernels 2..5 on device 3, rising sizes), many times over
  static crct::LdsLimits a, b;      // a: filled by two threads at once; b: the same records from one thread
  auto fill = [](crct::LdsLimits& t, int who) {
    for (int rep = 0; rep < 2000; ++rep)
      for (int i = 2; i < 6; ++i) {
        if ((i & 1) == who) t.record(&kernels[i], 2, (100 + i) * KB);
        t.record(&kernels[i], 3, (70 + (rep + who) % 60) * KB);
      }
  };
  std::thread t0(fill, std::ref(a), 0), t1(fill, std::ref(a), 1);
  t0.join();
  t1.join();
  fill(b, 0);
  fill(b, 1);
  bool same = true, expected = true;
  for (int i = 0; i < 8; ++i)
    for (int d = 0; d < 5; ++d)
      for (size_t kb = 64; kb <= 161; ++kb) same = same && a.needs_raise(&kernels[i], d, kb * KB) == b.needs_raise(&kernels[i], d, kb * KB);
  for (int i = 2; i < 6; ++i)
    expected = expected && !a.needs_raise(&kernels[i], 2, (100 + i) * KB) && a.needs_raise(&kernels[i], 2, (101 + i) * KB) &&
               !a.needs_raise(&kernels[i], 3, 129 * KB) && a.needs_raise(&kernels[i], 3, 130 * KB) && a.needs_raise(&kernels[i], 0, 96 * KB);
  check("two_threads_same_state_as_one", same);
  check("two_threads_expected_limits", expected);

  // the launch path's pattern: one thread looks keys up while another records them (first use of the row included); an answer
  // may go from "needs raising" to "settled" and never back
  static crct::LdsLimits c;
  static std::atomic<bool> done{false};
  bool monotone = true;
  std::thread reader([&monotone] {
    bool settled[4] = {};
    for (bool last = false; !last;) {
      last = done.load(std::memory_order_acquire);
      for (int i = 0; i < 4; ++i) {
        const bool need = c.needs_raise(&kernels[2 + i], 4, 120 * KB);
        if (settled[i] && need) monotone = false;
        settled[i] = !need;
      }
    }
    for (bool s : settled) monotone = monotone && s;      // the last look came after the last record
  });
  for (size_t kb = 65; kb <= 160; ++kb)
    for (int i = 0; i < 4; ++i) c.record(&kernels[2 + i], 4, kb * KB);
  done.store(true, std::memory_order_release);
  reader.join();
  check("lookup_during_record_goes_settled_once", monotone);

  // more kernels than rows: the ones that found no row keep needing the raise, the recorded ones stay settled
  static crct::LdsLimits full;
  static char many[crct::LdsLimits::MAX_KERNELS + 8];
  for (char& m : many) full.record(&m, 0, 96 * KB);
  int settled = 0;
  for (char& m : many) settled += !full.needs_raise(&m, 0, 96 * KB);
  check("full_table_degrades_to_always_raise", settled == crct::LdsLimits::MAX_KERNELS);
  return failures;
}
