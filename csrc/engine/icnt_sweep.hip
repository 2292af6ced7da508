// Open-loop network sweeps on the device (icnt_sweep.h): one 64-lane
// workgroup per sweep point runs rt_simulate_par<WavePar> on that point's
// configuration, dimensions, state and scratch in HBM.  No grid barrier, no
// persistence: the points are independent, so the kernel needs neither
// co-residency nor a slot of the cycle engine's CU pool.
//
// This file holds what is particular to open-loop points: a point's packets
// all have the one flit count, filled on the device.  The chunk's layout is
// icnt_sweep_layout.h; the pass with its LDS placement (sweep_pass), the
// chunk's device block and copies (SweepChunk) and the resource query are
// icnt_sweep_dev.h, shared with icnt_rr_sweep.hip and icnt_net_sweep.hip.
//
// The per-(unit, VC) words vhead / vcnt / vown / vout / vocc live in LDS when
// the five arrays of U * V words fit kIcntSweepLdsBytes; otherwise, or on
// request, they stay in the point's scratch in HBM like everything else.
// Both placements give the same results.
//
// Every offset and size is computed and bounded on the host: a point's
// packets and flits are its RtDims' capacities (np <= d.np, np * pf <= d.nf),
// and the kernel indexes only what rt_carve(d) laid out.
#include "icnt_sweep_dev.h"

namespace asim {

__global__ __launch_bounds__(64) void icnt_sweep_kernel(const SimCfg* cfg, const SweepPt* pts, SweepOut* outs,
                                                        char* base, const uint32_t* rt_off, const uint32_t* rt_links,
                                                        const uint16_t* lat, const uint16_t* inj_lat,
                                                        uint64_t step_cap, int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: 5 * U * V words (the host sized the launch)
  const SweepPtFields pt = pts[blockIdx.x];
  if (!pt.np) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  w.rt_off = rt_off;
  w.rt_links = rt_links;
  w.lat = lat;
  w.inj_lat = inj_lat;
  WavePar::each((int)pt.np, [&](int p) { w.nfl[p] = pt.pf; });
  WavePar::sync();
  sweep_pass(*cfg, pt.d, reinterpret_cast<uint64_t*>(base + pt.st_off), w, pt.np, outs + blockIdx.x, step_cap, hot_lds,
             hot_words);
}

uint64_t icnt_sweep_budget_bytes(uint64_t mem_budget_mb) {
  if (mem_budget_mb) return mem_budget_mb << 20;
  size_t free_b = 0, total_b = 0;
  hip_ok("icnt sweep", hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
  // what the engine's allocator holds cached comes back on demand
  const uint64_t cached = gpu_pool_stats()["cached_dev"];
  return (uint64_t)((double)(free_b + cached) * kIcntSweepFreeShare);
}

bool icnt_sweep_run_chunk(const OpenLoopNet& net, const std::vector<OpenLoopPoint>& pts, uint64_t step_cap,
                          bool allow_lds, std::vector<OpenLoopRaw>& raws) {
  const size_t n = pts.size();
  raws.assign(n, OpenLoopRaw());
  if (!n) return false;
  ChunkLayout l;
  l.records<SweepPt>(n);
  const NetOff o_net = place_net(l, net);
  std::vector<SweepPt> h_pts(n);
  uint64_t hot_bytes = 0, accounted = icnt_sweep_net_bytes(net);
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopPoint& p = pts[i];
    // one network per chunk: every point has the same U and V
    if (p.d.U != pts[0].d.U || p.d.V != pts[0].d.V) throw std::invalid_argument("icnt sweep: one network per chunk");
    if (p.np > p.d.np || (uint64_t)p.np * p.pf > p.d.nf || p.src.size() != p.np || p.dst.size() != p.np ||
        p.tinj.size() != p.np)
      throw std::invalid_argument("icnt sweep: a point's packets exceed its dimensions");
    h_pts[i] = place_point(l, p);
    hot_bytes = std::max(hot_bytes, icnt_hot_bytes(p.d));
    accounted += icnt_sweep_point_bytes(p);
  }
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  const SweepChunk ch("icnt sweep", l, accounted);
  ch.up(l.o_pts, h_pts.data(), n * sizeof(SweepPt));
  const SweepChunk::Tables t = ch.up_net(o_net, net);
  std::vector<RtWork> dw(n);  // the points' work arrays as device addresses
  for (size_t i = 0; i < n; ++i) {
    const OpenLoopPoint& p = pts[i];
    dw[i] = device_work(ch, p.d, h_pts[i].scr_off);
    ch.up(dw[i].src, p.src.data(), (size_t)p.np * 4);
    ch.up(dw[i].dst, p.dst.data(), (size_t)p.np * 4);
    ch.up(dw[i].tinj, p.tinj.data(), (size_t)p.np * 8);
  }
  hipLaunchKernelGGL(icnt_sweep_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     ch.at<const SimCfg>(o_net.cfg), ch.at<const SweepPt>(l.o_pts), ch.at<SweepOut>(l.o_out), ch.base(),
                     t.rt_off, t.rt_links, t.lat, t.inj_lat, step_cap, hot_lds ? 1 : 0);
  const std::vector<SweepOut> outs = ch.finish(n, l.o_out);
  for (size_t i = 0; i < n; ++i) ch.fetch_raw(raws[i], outs[i], pts[i].d, h_pts[i].st_off, dw[i].tarr, pts[i].np);
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_sweep_kernel_info() { return sweep_kernel_info((const void*)icnt_sweep_kernel); }

}  // namespace asim
