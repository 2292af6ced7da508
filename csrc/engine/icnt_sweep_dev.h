// What the five network sweep kernels and their launch paths share
// (icnt_sweep.hip, icnt_rr_sweep.hip, icnt_net_sweep.hip, icnt_cl_sweep.hip,
// icnt_cln_sweep.hip; included by those five only): on the device the router pass of one unit with the placement
// of its per-(unit, VC) words, on the host the chunk's device block with its
// copies, and the kernels' resource query.  The chunk's layout is
// icnt_sweep_layout.h.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "engine.h"
#include "icnt_sweep_layout.h"
#include "wave_par.h"
#include "../model/icnt_router_par.h"

namespace asim {

#define LDS_AS __attribute__((address_space(3)))
typedef LDS_AS uint32_t lds_u32;

// One unit's router pass of np > 0 packets, by the whole workgroup.  hot_lds:
// the words vhead / vcnt / vown / vout / vocc are five U * V slices of the
// launch's dynamic LDS at `hot_words` (the host sized it for the chunk's
// largest U * V), behind LDS-typed pointers; otherwise they stay in the
// unit's scratch.  The pass initialises them itself and nothing reads them
// after it, so consecutive passes of a workgroup reuse them.  Leaves the
// activity, the guard status and the deadlocked packets in *o.
__device__ __forceinline__ void sweep_pass(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, uint32_t np,
                                           SweepOut* o, uint64_t step_cap, int hot_lds, uint32_t* hot_words) {
  uint32_t lost = 0;
  if (hot_lds) {
    const uint32_t uv = d.U * d.V;
    lds_u32* h = (lds_u32*)hot_words;
    const RtHot<lds_u32*> hv{h, h + uv, h + 2 * uv, h + 3 * uv, h + 4 * uv};
    lost = rt_simulate_par_hot<WavePar>(c, d, st, w, hv, np, o->act, &o->status, step_cap);
  } else {
    lost = rt_simulate_par<WavePar>(c, d, st, w, np, o->act, &o->status, step_cap);
  }
  WavePar::one([&] { o->deadlocked = lost; });
}

// The closed-loop pass of one unit (model/icnt_closed.h), same placement rule.
__device__ __forceinline__ void sweep_pass_closed(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w,
                                                  const RtClosed& cl, SweepOut* o, uint64_t step_cap, int hot_lds,
                                                  uint32_t* hot_words) {
  uint32_t lost = 0;
  if (hot_lds) {
    const uint32_t uv = d.U * d.V;
    lds_u32* h = (lds_u32*)hot_words;
    const RtHot<lds_u32*> hv{h, h + uv, h + 2 * uv, h + 3 * uv, h + 4 * uv};
    lost = rt_simulate_par_closed<WavePar>(c, d, st, w, hv, cl, o->act, &o->status, step_cap);
  } else {
    const RtHot<uint32_t*> hv{w.vhead, w.vcnt, w.vown, w.vout, w.vocc};
    lost = rt_simulate_par_closed<WavePar>(c, d, st, w, hv, cl, o->act, &o->status, step_cap);
  }
  WavePar::one([&] { o->deadlocked = lost; });
}

inline void hip_ok(const char* who, hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
}

// The device block of one chunk, cleared.  `who` prefixes every error.
// std::logic_error unless the layout is exactly what the driver accounted:
// the fixed part plus the sum of the units' `*_bytes`.
class SweepChunk {
 public:
  SweepChunk(const char* who, const ChunkLayout& l, uint64_t accounted) : who_(who) {
    if (l.bytes != accounted)
      throw std::logic_error(std::string(who) + ": the chunk takes " + std::to_string(l.bytes) + " bytes, " +
                             std::to_string(accounted) + " were accounted");
    base_ = static_cast<char*>(gpu_pool_alloc(l.bytes));
    const hipError_t e = hipMemset(base_, 0, l.bytes);
    if (e != hipSuccess) gpu_pool_release(base_);
    ok(e, "clear the chunk");
  }
  ~SweepChunk() { gpu_pool_release(base_); }
  SweepChunk(const SweepChunk&) = delete;
  SweepChunk& operator=(const SweepChunk&) = delete;

  char* base() const { return base_; }
  template <class T>
  T* at(uint64_t off) const {
    return reinterpret_cast<T*>(base_ + off);
  }
  void ok(hipError_t e, const char* what) const { hip_ok(who_, e, what); }
  void up(void* dst, const void* src, size_t bytes) const {
    if (bytes) ok(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "copy to the device");
  }
  void up(uint64_t off, const void* src, size_t bytes) const { up(base_ + off, src, bytes); }
  void down(void* dst, const void* src, size_t bytes) const {
    if (bytes) ok(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "copy from the device");
  }

  // a network's configuration and tables to where place_net() put them;
  // the tables' device addresses, null unless the network is an anynet
  struct Tables {
    const uint32_t *rt_off = nullptr, *rt_links = nullptr;
    const uint16_t *lat = nullptr, *inj_lat = nullptr;
  };
  Tables up_net(const NetOff& o, const OpenLoopNet& net) const {
    up(o.cfg, &net.c, sizeof(SimCfg));
    up(o.roff, net.rt_off.data(), net.rt_off.size() * 4);
    up(o.rlinks, net.rt_links.data(), net.rt_links.size() * 4);
    up(o.lat, net.lat.data(), net.lat.size() * 2);
    up(o.ilat, net.inj_lat.data(), net.inj_lat.size() * 2);
    if (!net.anynet) return Tables();
    return Tables{at<uint32_t>(o.roff), at<uint32_t>(o.rlinks), at<uint16_t>(o.lat), at<uint16_t>(o.ilat)};
  }

  // after the launch: its error, the kernel's, and the n output records
  std::vector<SweepOut> finish(size_t n, uint64_t o_out) const {
    ok(hipGetLastError(), "launch");
    ok(hipDeviceSynchronize(), "kernel");
    std::vector<SweepOut> outs(n);
    down(outs.data(), base_ + o_out, n * sizeof(SweepOut));
    return outs;
  }

  // one pass's output record, final state and the arrivals of its np packets
  void fetch_raw(OpenLoopRaw& r, const SweepOut& o, const RtDims& d, uint64_t st_off, const uint64_t* d_tarr,
                 size_t np) const {
    for (int k = 0; k < RT_ACT_COUNT; ++k) r.act[k] = o.act[k];
    r.deadlocked = o.deadlocked;
    r.status = o.status;
    r.state.assign(rt_state_words(d), 0);
    down(r.state.data(), base_ + st_off, r.state.size() * 8);
    r.tarr.assign(np, 0);
    down(r.tarr.data(), d_tarr, np * 8);
  }

 private:
  const char* who_;
  char* base_ = nullptr;
};

// the work arrays of a pass as device addresses
inline RtWork device_work(const SweepChunk& ch, const RtDims& d, uint64_t scr_off) {
  RtWork w;
  rt_carve(d, ch.at<uint32_t>(scr_off), &w);
  return w;
}

// registers, LDS and scratch of a kernel (code-object metadata through the
// HIP function attributes); empty without a device
inline std::map<std::string, uint64_t> sweep_kernel_info(const void* fn) {
  std::map<std::string, uint64_t> m;
  hipFuncAttributes fa;
  if (!gpu_engine_available() || hipFuncGetAttributes(&fa, fn) != hipSuccess) {
    (void)hipGetLastError();
    return m;
  }
  m["num_regs"] = (uint64_t)fa.numRegs;
  m["scratch_bytes_per_lane"] = (uint64_t)fa.localSizeBytes;
  m["lds_bytes"] = (uint64_t)fa.sharedSizeBytes;
  m["max_threads_per_block"] = (uint64_t)fa.maxThreadsPerBlock;
  return m;
}

}  // namespace asim
