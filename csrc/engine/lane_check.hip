// Device half of the lane-policy exerciser (lane_check.h): one block of one
// 64-lane wavefront runs a named case under WavePar, the host runs the same
// source under SeqPar, and lane_policy_check() hands both results to the
// caller (tests/test_lane_policy.py compares them with an independent oracle).
// Every length and index is validated on the host (lane_plan) before the
// launch; the kernel indexes only what that validation bounded.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "wave_par.h"
#include "sm_split.h"
#include "lane_check.h"

namespace asim {

// the per-warp field under WavePar: a WarpReg<T> loaded from the array
template <class T, int N>
struct LaneReg<WavePar, T, N> {
  WarpReg<T> r;
  __device__ __forceinline__ explicit LaneReg(T (&arr)[N]) { r.load(arr); }
  __device__ __forceinline__ typename WarpReg<T>::Ref operator[](int w) { return r[w]; }
  __device__ __forceinline__ void store(T (&arr)[N]) { r.store(arr); }
};

__global__ __launch_bounds__(64) void lane_check_kernel(LaneArgs a, uint8_t* hbm_scratch, int scratch_hbm, SMState* st0,
                                                        SMState* st1, int split) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLaneScratch];
  for (int i = (int)threadIdx.x; i < kLaneScratch; i += 64) lds[i] = kLaneCanary;
  __syncthreads();
  a.scratch = scratch_hbm ? hbm_scratch : lds;
  if (!st0) {
    lane_case_prim<WavePar>(a);
  } else if (split) {
    SmSplit sp(*st0, *st1);
    lane_case_state<WavePar>(a, sp);
  } else {
    lane_case_state<WavePar>(a, *st0);
  }
}

namespace {
void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("lane_policy_check: ") + what + ": " + hipGetErrorString(e));
}
struct DevBuf {
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { hip_ok(hipMalloc(&p, bytes ? bytes : 16), "hipMalloc"); }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};
}  // namespace

LaneCheckResult lane_policy_check(const std::string& name, int n, const std::vector<uint64_t>& val,
                                  const std::vector<uint64_t>& m) {
  const LanePlan p = lane_plan(name, n, val, m);  // throws on any bad length / index
  LaneCheckResult r;
  lane_check_host(p, n, val, m, r);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return r;
  }
  DevBuf d_val(val.size() * 8), d_m(m.size() * 8), d_out(p.nout * 8), d_scr(kLaneScratch);
  if (!val.empty()) hip_ok(hipMemcpy(d_val.p, val.data(), val.size() * 8, hipMemcpyHostToDevice), "copy values");
  if (!m.empty()) hip_ok(hipMemcpy(d_m.p, m.data(), m.size() * 8, hipMemcpyHostToDevice), "copy mask");
  hip_ok(hipMemset(d_out.p, 0, p.nout ? p.nout * 8 : 16), "clear outputs");
  hip_ok(hipMemset(d_scr.p, kLaneCanary, kLaneScratch), "fill scratch");
  std::unique_ptr<DevBuf> st0, st1;
  std::vector<uint64_t> img;
  if (p.state) {
    img.assign(sizeof(SMState) / 8, 0);
    lane_fill_pattern(img, lane_state_seed(p, val));
    st0.reset(new DevBuf(sizeof(SMState)));
    hip_ok(hipMemcpy(st0->p, img.data(), sizeof(SMState), hipMemcpyHostToDevice), "copy state");
    if (p.split) {  // hot prefix and cold tail from two images of the same pattern
      st1.reset(new DevBuf(sizeof(SMState)));
      hip_ok(hipMemcpy(st1->p, img.data(), sizeof(SMState), hipMemcpyHostToDevice), "copy state");
    }
  }
  LaneArgs a{p.id, p.sub, n, (const uint64_t*)d_val.p, (int)val.size(), (const uint64_t*)d_m.p, (int)m.size(),
             (uint64_t*)d_out.p, nullptr};
  hipLaunchKernelGGL(lane_check_kernel, dim3(1), dim3(64), 0, 0, a, (uint8_t*)d_scr.p, p.scratch_hbm ? 1 : 0,
                     st0 ? (SMState*)st0->p : nullptr, st1 ? (SMState*)st1->p : nullptr, p.split ? 1 : 0);
  hip_ok(hipGetLastError(), "launch");
  hip_ok(hipDeviceSynchronize(), "kernel");
  r.wave.assign(p.nout, 0);
  if (p.nout) hip_ok(hipMemcpy(r.wave.data(), d_out.p, p.nout * 8, hipMemcpyDeviceToHost), "copy outputs");
  if (p.state) {
    std::vector<uint64_t> h0(img.size()), h1;
    hip_ok(hipMemcpy(h0.data(), st0->p, sizeof(SMState), hipMemcpyDeviceToHost), "copy state back");
    r.wave_state = h0;
    if (p.split) {
      h1.resize(img.size());
      hip_ok(hipMemcpy(h1.data(), st1->p, sizeof(SMState), hipMemcpyDeviceToHost), "copy state tail back");
      const size_t hot = kSmHotBytes / 8;
      std::copy(h1.begin() + hot, h1.end(), r.wave_state.begin() + hot);
      r.stray = !std::equal(h0.begin() + hot, h0.end(), img.begin() + hot) ||
                !std::equal(h1.begin(), h1.begin() + hot, img.begin());
    }
  }
  r.ran = true;
  return r;
}

}  // namespace asim
