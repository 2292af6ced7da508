// One packet list over many networks on the device (icnt_sweep.h): one
// 64-lane workgroup per network.  Unlike icnt_sweep_kernel and icnt_rr_kernel,
// which take one configuration per launch, every workgroup reads its own
// SimCfg, RtDims, offsets and anynet tables from its descriptor, so one launch
// replays a captured list on a whole set of candidate networks.
//
// The list (src, dst, bytes, tinj) is uploaded once per chunk.  Each unit
// fills its own work arrays from it, lane-strided, and derives a packet's
// flits from its bytes with that unit's flit size:
//   nfl = min(rt_flits(c, bytes), rt_flits(c, kRtMaxPktBytes))
// (the host computed the same numbers to size and bound the unit).
//
// The per-(unit, VC) words go in LDS under the kIcntSweepLdsBytes rule, applied
// to the LARGEST 5 * U * V words among the chunk's networks, for which the
// launch's dynamic LDS is sized: every workgroup carves its own U * V out of
// it.  If the largest does not fit, the whole chunk keeps them in HBM.
//
// Every offset and size is computed and bounded on the host (icnt_net_run_chunk
// checks each unit before anything is uploaded): a unit's packets and flits
// are its RtDims' capacities, every node index is below its N, and the kernel
// indexes only the list's np entries and what rt_carve(d) laid out.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "engine.h"
#include "icnt_sweep.h"
#include "wave_par.h"
#include "../model/icnt_router_par.h"

namespace asim {

struct NetPt {
  RtDims d;
  uint32_t np, anynet;
  // bytes from the chunk's base
  uint64_t cfg_off, st_off, scr_off, roff_off, rlinks_off, lat_off, ilat_off;
};
struct NetOut {
  uint64_t act[8];
  uint32_t deadlocked, status;
};
static_assert(RT_ACT_COUNT <= 8, "NetOut holds the activity counters");

#define LDS_AS __attribute__((address_space(3)))
typedef LDS_AS uint32_t lds_u32;

__global__ __launch_bounds__(64) void icnt_net_kernel(const NetPt* pts, NetOut* outs, char* base,
                                                      const uint32_t* l_src, const uint32_t* l_dst,
                                                      const uint32_t* l_bytes, const uint64_t* l_tinj,
                                                      uint64_t step_cap, int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: the chunk's largest 5 * U * V words (the host sized the launch)
  const NetPt pt = pts[blockIdx.x];
  NetOut* o = outs + blockIdx.x;
  if (!pt.np) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  const SimCfg& c = *reinterpret_cast<const SimCfg*>(base + pt.cfg_off);
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  if (pt.anynet) {
    w.rt_off = reinterpret_cast<const uint32_t*>(base + pt.roff_off);
    w.rt_links = reinterpret_cast<const uint32_t*>(base + pt.rlinks_off);
    w.lat = reinterpret_cast<const uint16_t*>(base + pt.lat_off);
    w.inj_lat = reinterpret_cast<const uint16_t*>(base + pt.ilat_off);
  }
  // this network's packets from the shared list
  const uint32_t nfl_max = rt_flits(c, kRtMaxPktBytes);
  WavePar::each((int)pt.np, [&](int i) {
    const uint32_t nfl = rt_flits(c, l_bytes[i]);
    w.src[i] = l_src[i];
    w.dst[i] = l_dst[i];
    w.tinj[i] = l_tinj[i];
    w.nfl[i] = nfl < nfl_max ? nfl : nfl_max;
  });
  WavePar::sync();
  uint64_t* st = reinterpret_cast<uint64_t*>(base + pt.st_off);
  uint32_t lost = 0;
  if (hot_lds) {
    const uint32_t uv = pt.d.U * pt.d.V;
    lds_u32* h = (lds_u32*)hot_words;
    const RtHot<lds_u32*> hv{h, h + uv, h + 2 * uv, h + 3 * uv, h + 4 * uv};
    lost = rt_simulate_par_hot<WavePar>(c, pt.d, st, w, hv, pt.np, o->act, &o->status, step_cap);
  } else {
    lost = rt_simulate_par<WavePar>(c, pt.d, st, w, pt.np, o->act, &o->status, step_cap);
  }
  WavePar::one([&] { o->deadlocked = lost; });
}

namespace {

constexpr uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("icnt network sweep: ") + what + ": " + hipGetErrorString(e));
}

struct PoolBlock {
  void* p = nullptr;
  explicit PoolBlock(size_t bytes) : p(gpu_pool_alloc(bytes)) {}
  ~PoolBlock() { gpu_pool_release(p); }
  PoolBlock(const PoolBlock&) = delete;
  PoolBlock& operator=(const PoolBlock&) = delete;
};

void check_list(const NetList& l) {
  if (!l.src || !l.dst || !l.bytes || !l.tinj) throw std::invalid_argument("icnt network sweep: the packet list is missing");
  const size_t n = l.src->size();
  if (l.dst->size() != n || l.bytes->size() != n || l.tinj->size() != n || n > 0x7fffffffu)
    throw std::invalid_argument("icnt network sweep: the packet list's arrays differ in length");
}

// std::invalid_argument unless everything the kernel will index lies inside
// what the unit's dimensions and tables lay out
void check_unit(const NetList& l, const NetUnit& u, size_t index) {
  auto bad = [&](const char* what) {
    throw std::invalid_argument("icnt network sweep: network " + std::to_string(index) + "'s " + what);
  };
  if (!u.net || !u.pt) bad("description is missing");
  const OpenLoopNet& net = *u.net;
  const OpenLoopPoint& p = *u.pt;
  const size_t np = l.src->size();
  if (p.np != np || p.np > p.d.np) bad("packets exceed its dimensions");
  if (p.nfl.size() != np) bad("flit counts differ in length");
  if (p.d.N != net.N || p.d.U != p.d.N + p.d.L || !p.d.V || !p.d.B || !p.d.H) bad("dimensions are not the network's");
  if (!net.c.flit_size) bad("flit size is zero");
  const uint32_t nfl_max = rt_flits(net.c, kRtMaxPktBytes);
  uint64_t flits = 0;
  for (size_t i = 0; i < np; ++i) {
    const uint32_t s = (*l.src)[i], d = (*l.dst)[i];
    if (s >= p.d.N || d >= p.d.N || s == d) bad("packet has a node out of range");
    // what the device will compute
    const uint32_t nfl = std::min(rt_flits(net.c, (*l.bytes)[i]), nfl_max);
    if (nfl != p.nfl[i]) bad("flit counts are not those of its flit size");
    flits += nfl;
  }
  if (flits > p.d.nf) bad("flits exceed its dimensions");
  if (net.anynet) {
    if (net.rt_off.size() != (size_t)net.N * net.N + 1 || net.lat.size() != p.d.L || net.inj_lat.size() != net.N)
      bad("route tables do not match its dimensions");
    for (size_t k = 0; k + 1 < net.rt_off.size(); ++k) {
      if (net.rt_off[k] > net.rt_off[k + 1] || net.rt_off[k + 1] - net.rt_off[k] > p.d.H) bad("routes exceed its longest route");
    }
    if (net.rt_off.back() != net.rt_links.size()) bad("route tables are inconsistent");
    for (uint32_t x : net.rt_links)
      if (x >= p.d.L) bad("route names a link out of range");
  }
}

}  // namespace

uint64_t icnt_net_list_bytes(const NetList& l) {
  const uint64_t n = l.src ? l.src->size() : 0;
  return 3 * align16(n * 4) + align16(n * 8);
}

uint64_t icnt_net_unit_bytes(const NetUnit& u) {
  const OpenLoopNet& net = *u.net;
  const RtDims& d = u.pt->d;
  return align16(rt_state_words(d) * 8) + align16(rt_carve(d, nullptr, nullptr) * 4) + align16(sizeof(NetPt)) +
         align16(sizeof(NetOut)) + align16(sizeof(SimCfg)) + align16(net.rt_off.size() * 4) +
         align16(net.rt_links.size() * 4) + align16(net.lat.size() * 2) + align16(net.inj_lat.size() * 2);
}

bool icnt_net_run_chunk(const NetList& list, const std::vector<NetUnit>& units, uint64_t step_cap, bool allow_lds,
                        std::vector<OpenLoopRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, OpenLoopRaw());
  if (!n) return false;
  check_list(list);
  for (size_t i = 0; i < n; ++i) check_unit(list, units[i], i);
  // the launch's LDS: the largest network of the chunk
  const uint64_t hot_bytes = icnt_net_hot_bytes(units);
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  // layout: descriptors, results, the list, then per unit its configuration,
  // anynet tables, state and scratch
  const size_t np = list.src->size();
  std::vector<NetPt> h_pts(n);
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = off;
    off += align16(bytes);
    return o;
  };
  const uint64_t o_pts = take(n * sizeof(NetPt)), o_out = take(n * sizeof(NetOut));
  const uint64_t o_src = take(np * 4), o_dst = take(np * 4), o_bytes = take(np * 4), o_tinj = take(np * 8);
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopNet& net = *units[i].net;
    NetPt& h = h_pts[i];
    h = NetPt();
    h.d = units[i].pt->d;
    h.np = (uint32_t)np;
    h.anynet = net.anynet ? 1 : 0;
    h.cfg_off = take(sizeof(SimCfg));
    h.roff_off = take(net.rt_off.size() * 4);
    h.rlinks_off = take(net.rt_links.size() * 4);
    h.lat_off = take(net.lat.size() * 2);
    h.ilat_off = take(net.inj_lat.size() * 2);
    h.st_off = take(rt_state_words(h.d) * 8);
    h.scr_off = take(rt_carve(h.d, nullptr, nullptr) * 4);
  }
  PoolBlock blk(off);
  char* base = static_cast<char*>(blk.p);
  hip_ok(hipMemset(base, 0, off), "clear the chunk");
  auto up = [&](uint64_t dst, const void* src, size_t bytes) {
    if (bytes) hip_ok(hipMemcpy(base + dst, src, bytes, hipMemcpyHostToDevice), "copy to the device");
  };
  up(o_pts, h_pts.data(), n * sizeof(NetPt));
  up(o_src, list.src->data(), np * 4);
  up(o_dst, list.dst->data(), np * 4);
  up(o_bytes, list.bytes->data(), np * 4);
  up(o_tinj, list.tinj->data(), np * 8);
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopNet& net = *units[i].net;
    up(h_pts[i].cfg_off, &net.c, sizeof(SimCfg));
    up(h_pts[i].roff_off, net.rt_off.data(), net.rt_off.size() * 4);
    up(h_pts[i].rlinks_off, net.rt_links.data(), net.rt_links.size() * 4);
    up(h_pts[i].lat_off, net.lat.data(), net.lat.size() * 2);
    up(h_pts[i].ilat_off, net.inj_lat.data(), net.inj_lat.size() * 2);
  }
  hipLaunchKernelGGL(icnt_net_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     reinterpret_cast<const NetPt*>(base + o_pts), reinterpret_cast<NetOut*>(base + o_out), base,
                     reinterpret_cast<const uint32_t*>(base + o_src), reinterpret_cast<const uint32_t*>(base + o_dst),
                     reinterpret_cast<const uint32_t*>(base + o_bytes),
                     reinterpret_cast<const uint64_t*>(base + o_tinj), step_cap, hot_lds ? 1 : 0);
  hip_ok(hipGetLastError(), "launch");
  hip_ok(hipDeviceSynchronize(), "kernel");
  std::vector<NetOut> h_out(n);
  hip_ok(hipMemcpy(h_out.data(), base + o_out, n * sizeof(NetOut), hipMemcpyDeviceToHost), "copy results");
  for (size_t i = 0; i < n; ++i) {
    OpenLoopRaw& x = raws[i];
    for (int k = 0; k < RT_ACT_COUNT; ++k) x.act[k] = h_out[i].act[k];
    x.deadlocked = h_out[i].deadlocked;
    x.status = h_out[i].status;
    x.state.assign(rt_state_words(h_pts[i].d), 0);
    x.tarr.assign(np, 0);
    RtWork dw;  // the unit's work arrays as device addresses
    rt_carve(h_pts[i].d, reinterpret_cast<uint32_t*>(base + h_pts[i].scr_off), &dw);
    if (!x.state.empty())
      hip_ok(hipMemcpy(x.state.data(), base + h_pts[i].st_off, x.state.size() * 8, hipMemcpyDeviceToHost), "copy state");
    if (np) hip_ok(hipMemcpy(x.tarr.data(), dw.tarr, np * 8, hipMemcpyDeviceToHost), "copy arrivals");
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_net_kernel_info() {
  std::map<std::string, uint64_t> m;
  hipFuncAttributes fa;
  if (!gpu_engine_available() || hipFuncGetAttributes(&fa, (const void*)icnt_net_kernel) != hipSuccess) {
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
