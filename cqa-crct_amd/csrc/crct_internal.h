// Internal declarations shared by the kernel translation units and the step engine.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "../../include/crct_hip.h"

void crct_set_error(const char* fmt, ...);
#define CRCT_CHECK_HIP(expr)                                                          \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      crct_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)
#define CRCT_REQUIRE(cond, ...)                 \
  do {                                          \
    if (!(cond)) {                              \
      crct_set_error(__VA_ARGS__);              \
      return 2;                                 \
    }                                           \
  } while (0)

// whether a GEMM configuration id (CrctGemmArgs.tile) is built (gemm.hip, k_configs)
bool crct_gemm_config_built(int id);
// the configuration of the step engine's fp8 weight gradients, given what the site policy asks for (-1: nothing)
int crct_gemm_fp8_wgrad_step_config(int asked);
// The two GEMM launches (gemm.hip), behind the validation of the C entry points (engine.cpp, gemm_check).
// One problem with its LayerNorm addend (CrctGemmLnAddend; ln == NULL or ln->mean == NULL: none).
hipError_t crct_gemm_launch(const CrctGemmArgs& g, const CrctGemmLnAddend* ln, hipStream_t s);
// n problems in one grid where they qualify, else one by one.
struct CrctGemmGroup {
  const CrctGemmArgs* gs;          // the n problems
  const CrctGemmLnAddend* ln;      // NULL, or one entry per problem (mean == NULL: none for that problem)
  int n;
  const uint8_t* keep;             // NULL, or one flag per problem: only the flagged ones are launched, as members of the group all n form
  int target_wgs;                  // > 0: a grouped bf16 weight-gradient launch runs as a persistent grid of about that many workgroups
                                   // (gemm.hip, group_grid); 0: one workgroup per tile; < 0: the library's default (crct_gemm_group_target_workgroups)
};
hipError_t crct_gemm_launch_grouped(const CrctGemmGroup& grp, hipStream_t s);
// streams.hip: three streams on hardware queues other than main's (+ a second one on the last queue), found by probing
int crct_streams_place(hipStream_t main, hipStream_t out[4], int* n_classes);

// out[0] = inv_n * sum_r loss[r] in a fixed order, one workgroup (lm_head.hip): the mean of the masked-LM loss and of the masked-region loss
void crct_loss_mean(const float* loss, float* out, int R, float inv_n, hipStream_t s);

// upper bound of the workgroup count of the LayerNorm-backward style kernels (4 rows per workgroup and pass):
// sizes the column-partials scratch [partials][blocks][H]
#define CRCT_LN_BWD_MAX_BLOCKS 256

// ---- live stamps of EVERY kernel the library launches (crct_prof_enable(2); bench.py config.critical_path): while armed, a launch is
// dispatched with a start / stop event pair (hipExtLaunchKernelGGL: the begin / end stamps of that kernel, what rocprofv3's kernel
// trace reports) and remembered with its stream.  Off (the product): one predictable branch per launch.
bool crct_stamp_begin(hipStream_t s, hipEvent_t* start, hipEvent_t* stop);      // streams.hip; false = stamping is off
void crct_stamp_adopt(hipStream_t s, hipEvent_t start, hipEvent_t stop);        // a GEMM launch that carries its own event pair (gemm.hip)
void crct_stamp_enable(int on);
void crct_stamp_reset(void);
#ifdef CRCT_GEMM_LAB
// LAB build only (make lab -> tools/lab/libcrct_lab.so, never the package's library): launches whose kernel name contains one of the
// comma-separated entries of $CRCT_LAB_SKIP ("name" or "name@k", k = ordinal of the stream in order of first use) are LEFT OUT --
// wrong results, timing only: what the step gains when a class of kernels costs nothing (tools/lab/step_sensitivity.sh).
bool crct_lab_skip(const void* kern, hipStream_t s);
#endif
// Before a launch with more than 64 KB of dynamic LDS: `bytes` = the most `kern` is ever launched with.  Raises the kernel's limit on
// the CURRENT device unless it already stands at least there (lds_limit.h: per kernel and device, from any host thread).  The launch
// stream must belong to the current device, as it does under PyTorch's device guard: the runtime sets the attribute there and nowhere
// else.  Up to 64 KB: no runtime call; above: hipGetDevice, and hipFuncSetAttribute the first time per device.
hipError_t crct_lds_limit_raise(const void* kern, size_t bytes);      // streams.hip
// One hipGetDevice for a whole forward / backward instead of one per launch above 64 KB (several hundred per step, ~0.1 us each):
// while a scope lives, crct_lds_limit on THIS thread takes the device from it.  Only around code that never calls hipSetDevice.
class CrctDeviceScope {
 public:
  CrctDeviceScope();
  ~CrctDeviceScope();
  CrctDeviceScope(const CrctDeviceScope&) = delete;
  CrctDeviceScope& operator=(const CrctDeviceScope&) = delete;
 private:
  int outer_;
};
template <class K>
inline hipError_t crct_lds_limit(K kern, size_t bytes) {
  return bytes <= 64 * 1024 ? hipSuccess : crct_lds_limit_raise(reinterpret_cast<const void*>(kern), bytes);
}
template <class K, class... A>
inline void crct_launch(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... a) {
#ifdef CRCT_GEMM_LAB
  if (crct_lab_skip((const void*)kern, s)) return;
#endif
  hipEvent_t e0, e1;
  if (crct_stamp_begin(s, &e0, &e1)) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, s, e0, e1, 0u, a...);
  else hipLaunchKernelGGL(kern, grid, block, lds, s, a...);
}
