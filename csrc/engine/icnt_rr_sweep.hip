// Packet-list replay and request-reply points on the device (icnt_sweep.h):
// one 64-lane workgroup per unit.  A unit's packets carry their own flit
// counts (uploaded, not filled from one number per point), and a
// request-reply unit runs, in the one workgroup and the one launch,
//   1. the router pass on the request subnet's state,
//   2. rt_reply_build<WavePar> (model/icnt_reqreply.h): the reply subnet's
//      injection schedule from the request arrivals, sorted on the device,
//   3. the router pass on the reply subnet's state
// as a loop over the subnet, so the pass is instantiated once per placement
// of the per-(unit, VC) words, as in icnt_sweep_kernel.  Those words go in LDS
// under the same kIcntSweepLdsBytes rule; the reply pass reuses them, because
// a pass initialises them itself and nothing reads them after it.
//
// Every offset and size is computed and bounded on the host (icnt_rr_run_chunk
// checks each unit before anything is uploaded): a subnet's packets and flits
// are its RtDims' capacities, every node index is below N, and the kernel
// indexes only what rt_carve(d) and the unit's three np-word arrays laid out.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "engine.h"
#include "icnt_sweep.h"
#include "wave_par.h"
#include "../model/icnt_reqreply.h"
#include "../model/icnt_router_par.h"

namespace asim {

struct RrPt {
  RtDims d[2];
  uint32_t np, nsub;          // packets; subnets to run (1: replay, 2: request-reply)
  uint32_t fl_read, fl_write;
  uint64_t delay;
  uint64_t st_off[2], scr_off[2], aux_off;  // bytes from the chunk's base; aux: kind, reply_of, tmp (np words each)
};
struct RrOut {
  uint64_t act[2][8];
  uint32_t deadlocked[2], status[2];
};
static_assert(RT_ACT_COUNT <= 8, "RrOut holds the activity counters");

#define LDS_AS __attribute__((address_space(3)))
typedef LDS_AS uint32_t lds_u32;

__global__ __launch_bounds__(64) void icnt_rr_kernel(const SimCfg* cfg, const RrPt* pts, RrOut* outs, char* base,
                                                     const uint32_t* rt_off, const uint32_t* rt_links,
                                                     const uint16_t* lat, const uint16_t* inj_lat, uint64_t step_cap,
                                                     int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: 5 * U * V words (the host sized the launch)
  const RrPt pt = pts[blockIdx.x];
  RrOut* o = outs + blockIdx.x;
  if (!pt.np) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  uint32_t* aux = reinterpret_cast<uint32_t*>(base + pt.aux_off);
  for (uint32_t sub = 0; sub < pt.nsub; ++sub) {
    RtWork w;
    rt_carve(pt.d[sub], reinterpret_cast<uint32_t*>(base + pt.scr_off[sub]), &w);
    w.rt_off = rt_off;
    w.rt_links = rt_links;
    w.lat = lat;
    w.inj_lat = inj_lat;
    if (sub) {
      RtWork q;  // the request pass's arrays
      rt_carve(pt.d[0], reinterpret_cast<uint32_t*>(base + pt.scr_off[0]), &q);
      rt_reply_build<WavePar>(pt.np, RtReplyIn{q.src, q.dst, aux, q.tarr}, RtReplyOut{w.src, w.dst, w.nfl, w.tinj},
                              pt.fl_read, pt.fl_write, pt.delay, aux + pt.np, aux + 2ull * pt.np);
    }
    uint64_t* st = reinterpret_cast<uint64_t*>(base + pt.st_off[sub]);
    uint32_t lost = 0;
    if (hot_lds) {
      const uint32_t uv = pt.d[sub].U * pt.d[sub].V;
      lds_u32* h = (lds_u32*)hot_words;
      const RtHot<lds_u32*> hv{h, h + uv, h + 2 * uv, h + 3 * uv, h + 4 * uv};
      lost = rt_simulate_par_hot<WavePar>(*cfg, pt.d[sub], st, w, hv, pt.np, o->act[sub], &o->status[sub], step_cap);
    } else {
      lost = rt_simulate_par<WavePar>(*cfg, pt.d[sub], st, w, pt.np, o->act[sub], &o->status[sub], step_cap);
    }
    WavePar::one([&] { o->deadlocked[sub] = lost; });
    WavePar::sync();
    // a pass cut off by its guard leaves no arrivals to reply to
    if (WavePar::uni(o->status[sub]) != RT_STATUS_OK) return;
  }
}

namespace {

constexpr uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("icnt replay: ") + what + ": " + hipGetErrorString(e));
}

struct PoolBlock {
  void* p = nullptr;
  explicit PoolBlock(size_t bytes) : p(gpu_pool_alloc(bytes)) {}
  ~PoolBlock() { gpu_pool_release(p); }
  PoolBlock(const PoolBlock&) = delete;
  PoolBlock& operator=(const PoolBlock&) = delete;
};

// std::invalid_argument unless everything the kernel will index lies inside
// what the unit's dimensions lay out
void check_unit(const OpenLoopNet& net, const RrUnit& u) {
  auto bad = [](const char* what) { throw std::invalid_argument(std::string("icnt replay: a unit's ") + what); };
  if (!u.req) bad("packet list is missing");
  const OpenLoopPoint& p = *u.req;
  if (p.np > p.d.np || p.np > 0x7fffffffu) bad("packets exceed its dimensions");
  if (p.src.size() != p.np || p.dst.size() != p.np || p.tinj.size() != p.np || p.nfl.size() != p.np)
    bad("arrays differ in length");
  if (p.d.N != net.N) bad("network is not the chunk's");
  uint64_t flits = 0;
  for (uint32_t i = 0; i < p.np; ++i) {
    if (p.src[i] >= p.d.N || p.dst[i] >= p.d.N || p.src[i] == p.dst[i]) bad("packet has a node out of range");
    if (!p.nfl[i]) bad("packet has no flits");
    flits += p.nfl[i];
  }
  if (flits > p.d.nf) bad("flits exceed its dimensions");
  if (!u.reply) return;
  const RtDims& r = u.d_rep;
  if (r.N != p.d.N || r.L != p.d.L || r.U != p.d.U || r.V != p.d.V || r.B != p.d.B || r.H != p.d.H)
    bad("reply subnet is another network");
  if (!u.kind || u.kind->size() != p.np) bad("kinds differ in length");
  if (!u.fl_read || !u.fl_write) bad("reply has no flits");
  const uint64_t fl = u.fl_read > u.fl_write ? u.fl_read : u.fl_write;
  if (p.np > r.np || (uint64_t)p.np * fl > r.nf) bad("replies exceed their dimensions");
}

}  // namespace

uint64_t icnt_rr_unit_bytes(const RrUnit& u) {
  const OpenLoopPoint& p = *u.req;
  uint64_t b = align16(rt_state_words(p.d) * 8) + align16(rt_carve(p.d, nullptr, nullptr) * 4) +
               align16(3ull * p.np * 4) + align16(sizeof(RrPt)) + align16(sizeof(RrOut));
  if (u.reply) b += align16(rt_state_words(u.d_rep) * 8) + align16(rt_carve(u.d_rep, nullptr, nullptr) * 4);
  return b;
}

bool icnt_rr_run_chunk(const OpenLoopNet& net, const std::vector<RrUnit>& units, uint64_t step_cap, bool allow_lds,
                       std::vector<RrRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, RrRaw());
  if (!n) return false;
  for (const RrUnit& u : units) check_unit(net, u);
  // one network per chunk: every unit has the same U and V
  const RtDims& d0 = units[0].req->d;
  const uint64_t hot_bytes = 5ull * d0.U * d0.V * 4;
  for (const RrUnit& u : units)
    if (u.req->d.U != d0.U || u.req->d.V != d0.V) throw std::invalid_argument("icnt replay: one network per chunk");
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  // layout: descriptors, results, configuration, anynet tables, then per unit
  // and subnet state and scratch, and the unit's kind / reply_of / tmp words
  std::vector<RrPt> h_pts(n);
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = off;
    off += align16(bytes);
    return o;
  };
  const uint64_t o_pts = take(n * sizeof(RrPt)), o_out = take(n * sizeof(RrOut)), o_cfg = take(sizeof(SimCfg));
  const uint64_t o_roff = take(net.rt_off.size() * 4), o_rlinks = take(net.rt_links.size() * 4),
                 o_lat = take(net.lat.size() * 2), o_ilat = take(net.inj_lat.size() * 2);
  for (size_t i = 0; i < n; ++i) {
    const RrUnit& u = units[i];
    RrPt& h = h_pts[i];
    h = RrPt();
    h.d[0] = u.req->d;
    h.d[1] = u.reply ? u.d_rep : u.req->d;
    h.np = u.req->np;
    h.nsub = u.reply ? 2 : 1;
    h.fl_read = u.fl_read;
    h.fl_write = u.fl_write;
    h.delay = u.delay;
    for (uint32_t s = 0; s < h.nsub; ++s) {
      h.st_off[s] = take(rt_state_words(h.d[s]) * 8);
      h.scr_off[s] = take(rt_carve(h.d[s], nullptr, nullptr) * 4);
    }
    h.aux_off = take(3ull * h.np * 4);
  }
  PoolBlock blk(off);
  char* base = static_cast<char*>(blk.p);
  hip_ok(hipMemset(base, 0, off), "clear the chunk");
  hip_ok(hipMemcpy(base + o_pts, h_pts.data(), n * sizeof(RrPt), hipMemcpyHostToDevice), "copy descriptors");
  hip_ok(hipMemcpy(base + o_cfg, &net.c, sizeof(SimCfg), hipMemcpyHostToDevice), "copy configuration");
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) hip_ok(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "copy to the device");
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) hip_ok(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "copy from the device");
  };
  up(base + o_roff, net.rt_off.data(), net.rt_off.size() * 4);
  up(base + o_rlinks, net.rt_links.data(), net.rt_links.size() * 4);
  up(base + o_lat, net.lat.data(), net.lat.size() * 2);
  up(base + o_ilat, net.inj_lat.data(), net.inj_lat.size() * 2);
  std::vector<RtWork> dw(2 * n);  // the subnets' work arrays as device addresses
  for (size_t i = 0; i < n; ++i) {
    const RrUnit& u = units[i];
    const OpenLoopPoint& p = *u.req;
    for (uint32_t s = 0; s < h_pts[i].nsub; ++s)
      rt_carve(h_pts[i].d[s], reinterpret_cast<uint32_t*>(base + h_pts[i].scr_off[s]), &dw[2 * i + s]);
    const size_t np = p.np;
    up(dw[2 * i].src, p.src.data(), np * 4);
    up(dw[2 * i].dst, p.dst.data(), np * 4);
    up(dw[2 * i].nfl, p.nfl.data(), np * 4);
    up(dw[2 * i].tinj, p.tinj.data(), np * 8);
    if (u.reply) up(base + h_pts[i].aux_off, u.kind->data(), np * 4);
  }
  const bool an = net.anynet;
  hipLaunchKernelGGL(icnt_rr_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     reinterpret_cast<const SimCfg*>(base + o_cfg), reinterpret_cast<const RrPt*>(base + o_pts),
                     reinterpret_cast<RrOut*>(base + o_out), base,
                     an ? reinterpret_cast<const uint32_t*>(base + o_roff) : nullptr,
                     an ? reinterpret_cast<const uint32_t*>(base + o_rlinks) : nullptr,
                     an ? reinterpret_cast<const uint16_t*>(base + o_lat) : nullptr,
                     an ? reinterpret_cast<const uint16_t*>(base + o_ilat) : nullptr, step_cap, hot_lds ? 1 : 0);
  hip_ok(hipGetLastError(), "launch");
  hip_ok(hipDeviceSynchronize(), "kernel");
  std::vector<RrOut> h_out(n);
  hip_ok(hipMemcpy(h_out.data(), base + o_out, n * sizeof(RrOut), hipMemcpyDeviceToHost), "copy results");
  for (size_t i = 0; i < n; ++i) {
    const size_t np = units[i].req->np;
    RrRaw& r = raws[i];
    for (uint32_t s = 0; s < h_pts[i].nsub; ++s) {
      OpenLoopRaw& x = s ? r.rep : r.req;
      for (int k = 0; k < RT_ACT_COUNT; ++k) x.act[k] = h_out[i].act[s][k];
      x.deadlocked = h_out[i].deadlocked[s];
      x.status = h_out[i].status[s];
      x.state.assign(rt_state_words(h_pts[i].d[s]), 0);
      down(x.state.data(), base + h_pts[i].st_off[s], x.state.size() * 8);
      x.tarr.assign(np, 0);
      down(x.tarr.data(), dw[2 * i + s].tarr, np * 8);
    }
    if (!units[i].reply) continue;
    r.reply_of.assign(np, 0);
    r.rep_src.assign(np, 0);
    r.rep_dst.assign(np, 0);
    r.rep_nfl.assign(np, 0);
    r.rep_tinj.assign(np, 0);
    down(r.reply_of.data(), base + h_pts[i].aux_off + np * 4, np * 4);
    down(r.rep_src.data(), dw[2 * i + 1].src, np * 4);
    down(r.rep_dst.data(), dw[2 * i + 1].dst, np * 4);
    down(r.rep_nfl.data(), dw[2 * i + 1].nfl, np * 4);
    down(r.rep_tinj.data(), dw[2 * i + 1].tinj, np * 8);
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_rr_kernel_info() {
  std::map<std::string, uint64_t> m;
  hipFuncAttributes fa;
  if (!gpu_engine_available() || hipFuncGetAttributes(&fa, (const void*)icnt_rr_kernel) != hipSuccess) {
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
