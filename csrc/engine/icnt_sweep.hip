// Open-loop network sweeps on the device (icnt_sweep.h): one 64-lane
// workgroup per sweep point runs rt_simulate_par<WavePar> on that point's
// configuration, dimensions, state and scratch in HBM.  No grid barrier, no
// persistence: the points are independent, so the kernel needs neither
// co-residency nor a slot of the cycle engine's CU pool.
//
// The per-(unit, VC) words vhead / vcnt / vown / vout / vocc live in LDS,
// behind LDS-typed pointers (their loads wait for LDS traffic only), when the
// five arrays of U * V words fit kIcntSweepLdsBytes; otherwise, or on request,
// they stay in the point's scratch in HBM like everything else.  The pass
// initialises them itself, and nothing reads them after it, so nothing is
// copied in or out.  Both placements give the same results.
//
// Every offset and size is computed and bounded on the host: a point's
// packets and flits are its RtDims' capacities (np <= d.np, np * pf <= d.nf),
// and the kernel indexes only what rt_carve(d) laid out.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "engine.h"
#include "icnt_sweep.h"
#include "wave_par.h"
#include "../model/icnt_router_par.h"

namespace asim {

struct SweepPt {
  RtDims d;
  uint32_t np, pf;
  uint64_t st_off, scr_off;  // bytes from the chunk's base
};
struct SweepOut {
  uint64_t act[8];
  uint32_t deadlocked, status;
};
static_assert(RT_ACT_COUNT <= 8, "SweepOut holds the activity counters");

namespace {
constexpr uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
}  // namespace

#define LDS_AS __attribute__((address_space(3)))
typedef LDS_AS uint32_t lds_u32;

__global__ __launch_bounds__(64) void icnt_sweep_kernel(const SimCfg* cfg, const SweepPt* pts, SweepOut* outs,
                                                        char* base, const uint32_t* rt_off, const uint32_t* rt_links,
                                                        const uint16_t* lat, const uint16_t* inj_lat,
                                                        uint64_t step_cap, int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: 5 * U * V words (the host sized the launch)
  const SweepPt pt = pts[blockIdx.x];
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  w.rt_off = rt_off;
  w.rt_links = rt_links;
  w.lat = lat;
  w.inj_lat = inj_lat;
  uint64_t* st = reinterpret_cast<uint64_t*>(base + pt.st_off);
  SweepOut* o = outs + blockIdx.x;
  WavePar::each((int)pt.np, [&](int p) { w.nfl[p] = pt.pf; });
  WavePar::sync();
  uint32_t lost = 0;
  if (pt.np && hot_lds) {
    const uint32_t uv = pt.d.U * pt.d.V;
    lds_u32* h = (lds_u32*)hot_words;
    const RtHot<lds_u32*> hv{h, h + uv, h + 2 * uv, h + 3 * uv, h + 4 * uv};
    lost = rt_simulate_par_hot<WavePar>(*cfg, pt.d, st, w, hv, pt.np, o->act, &o->status, step_cap);
  } else if (pt.np) {
    lost = rt_simulate_par<WavePar>(*cfg, pt.d, st, w, pt.np, o->act, &o->status, step_cap);
  }
  WavePar::one([&] { o->deadlocked = lost; });
}

namespace {

void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("icnt sweep: ") + what + ": " + hipGetErrorString(e));
}

struct PoolBlock {
  void* p = nullptr;
  explicit PoolBlock(size_t bytes) : p(gpu_pool_alloc(bytes)) {}
  ~PoolBlock() { gpu_pool_release(p); }
  PoolBlock(const PoolBlock&) = delete;
  PoolBlock& operator=(const PoolBlock&) = delete;
};

}  // namespace

uint64_t icnt_sweep_point_bytes(const OpenLoopPoint& pt) {
  return align16(rt_state_words(pt.d) * 8) + align16(rt_carve(pt.d, nullptr, nullptr) * 4) + align16(sizeof(SweepPt)) +
         align16(sizeof(SweepOut));
}

uint64_t icnt_sweep_budget_bytes(uint64_t mem_budget_mb) {
  if (mem_budget_mb) return mem_budget_mb << 20;
  size_t free_b = 0, total_b = 0;
  hip_ok(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
  // what the engine's allocator holds cached comes back on demand
  const uint64_t cached = gpu_pool_stats()["cached_dev"];
  return (uint64_t)((double)(free_b + cached) * kIcntSweepFreeShare);
}

bool icnt_sweep_run_chunk(const OpenLoopNet& net, const std::vector<OpenLoopPoint>& pts, uint64_t step_cap,
                          bool allow_lds, std::vector<OpenLoopRaw>& raws) {
  const size_t n = pts.size();
  raws.assign(n, OpenLoopRaw());
  if (!n) return false;
  // one network per chunk: every point has the same U and V
  const uint64_t hot_bytes = 5ull * pts[0].d.U * pts[0].d.V * 4;
  for (const OpenLoopPoint& p : pts)
    if (p.d.U != pts[0].d.U || p.d.V != pts[0].d.V) throw std::invalid_argument("icnt sweep: one network per chunk");
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  // layout: descriptors, results, configuration, anynet tables, then per point state and scratch
  std::vector<SweepPt> h_pts(n);
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = off;
    off += align16(bytes);
    return o;
  };
  const uint64_t o_pts = take(n * sizeof(SweepPt)), o_out = take(n * sizeof(SweepOut)), o_cfg = take(sizeof(SimCfg));
  const uint64_t o_roff = take(net.rt_off.size() * 4), o_rlinks = take(net.rt_links.size() * 4),
                 o_lat = take(net.lat.size() * 2), o_ilat = take(net.inj_lat.size() * 2);
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopPoint& p = pts[i];
    if (p.np > p.d.np || (uint64_t)p.np * p.pf > p.d.nf || p.src.size() != p.np || p.dst.size() != p.np ||
        p.tinj.size() != p.np)
      throw std::invalid_argument("icnt sweep: a point's packets exceed its dimensions");
    h_pts[i].d = p.d;
    h_pts[i].np = p.np;
    h_pts[i].pf = p.pf;
    h_pts[i].st_off = take(rt_state_words(p.d) * 8);
    h_pts[i].scr_off = take(rt_carve(p.d, nullptr, nullptr) * 4);
  }
  PoolBlock blk(off);
  char* base = static_cast<char*>(blk.p);
  hip_ok(hipMemset(base, 0, off), "clear the chunk");
  hip_ok(hipMemcpy(base + o_pts, h_pts.data(), n * sizeof(SweepPt), hipMemcpyHostToDevice), "copy descriptors");
  hip_ok(hipMemcpy(base + o_cfg, &net.c, sizeof(SimCfg), hipMemcpyHostToDevice), "copy configuration");
  auto up = [&](uint64_t o, const void* src, size_t bytes) {
    if (bytes) hip_ok(hipMemcpy(base + o, src, bytes, hipMemcpyHostToDevice), "copy tables");
  };
  up(o_roff, net.rt_off.data(), net.rt_off.size() * 4);
  up(o_rlinks, net.rt_links.data(), net.rt_links.size() * 4);
  up(o_lat, net.lat.data(), net.lat.size() * 2);
  up(o_ilat, net.inj_lat.data(), net.inj_lat.size() * 2);
  std::vector<RtWork> dw(n);  // the points' work arrays as device addresses
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopPoint& p = pts[i];
    rt_carve(p.d, reinterpret_cast<uint32_t*>(base + h_pts[i].scr_off), &dw[i]);
    if (!p.np) continue;
    hip_ok(hipMemcpy(dw[i].src, p.src.data(), (size_t)p.np * 4, hipMemcpyHostToDevice), "copy sources");
    hip_ok(hipMemcpy(dw[i].dst, p.dst.data(), (size_t)p.np * 4, hipMemcpyHostToDevice), "copy destinations");
    hip_ok(hipMemcpy(dw[i].tinj, p.tinj.data(), (size_t)p.np * 8, hipMemcpyHostToDevice), "copy injection times");
  }
  const bool an = net.anynet;
  hipLaunchKernelGGL(icnt_sweep_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     reinterpret_cast<const SimCfg*>(base + o_cfg), reinterpret_cast<const SweepPt*>(base + o_pts),
                     reinterpret_cast<SweepOut*>(base + o_out), base,
                     an ? reinterpret_cast<const uint32_t*>(base + o_roff) : nullptr,
                     an ? reinterpret_cast<const uint32_t*>(base + o_rlinks) : nullptr,
                     an ? reinterpret_cast<const uint16_t*>(base + o_lat) : nullptr,
                     an ? reinterpret_cast<const uint16_t*>(base + o_ilat) : nullptr, step_cap, hot_lds ? 1 : 0);
  hip_ok(hipGetLastError(), "launch");
  hip_ok(hipDeviceSynchronize(), "kernel");
  std::vector<SweepOut> h_out(n);
  hip_ok(hipMemcpy(h_out.data(), base + o_out, n * sizeof(SweepOut), hipMemcpyDeviceToHost), "copy results");
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopPoint& p = pts[i];
    OpenLoopRaw& r = raws[i];
    for (int k = 0; k < RT_ACT_COUNT; ++k) r.act[k] = h_out[i].act[k];
    r.deadlocked = h_out[i].deadlocked;
    r.status = h_out[i].status;
    r.state.assign(rt_state_words(p.d), 0);
    hip_ok(hipMemcpy(r.state.data(), base + h_pts[i].st_off, r.state.size() * 8, hipMemcpyDeviceToHost), "copy state");
    r.tarr.assign(p.np, 0);
    if (p.np) hip_ok(hipMemcpy(r.tarr.data(), dw[i].tarr, (size_t)p.np * 8, hipMemcpyDeviceToHost), "copy arrivals");
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_sweep_kernel_info() {
  std::map<std::string, uint64_t> m;
  hipFuncAttributes fa;
  if (!gpu_engine_available() || hipFuncGetAttributes(&fa, (const void*)icnt_sweep_kernel) != hipSuccess) {
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
