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
//
// This file holds what is particular to network units: the fill from the
// shared list and the list and unit checks.  The chunk's layout is
// icnt_sweep_layout.h; the pass (sweep_pass), the chunk's device block and
// copies (SweepChunk) and the resource query are icnt_sweep_dev.h.
#include "icnt_sweep_dev.h"

namespace asim {

__global__ __launch_bounds__(64) void icnt_net_kernel(const NetPt* pts, SweepOut* outs, char* base,
                                                      const uint32_t* l_src, const uint32_t* l_dst,
                                                      const uint32_t* l_bytes, const uint64_t* l_tinj,
                                                      uint64_t step_cap, int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: the chunk's largest 5 * U * V words (the host sized the launch)
  const NetPt pt = pts[blockIdx.x];
  if (!pt.np) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  const SimCfg& c = *reinterpret_cast<const SimCfg*>(base + pt.net.cfg);
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  if (pt.anynet) {
    w.rt_off = reinterpret_cast<const uint32_t*>(base + pt.net.roff);
    w.rt_links = reinterpret_cast<const uint32_t*>(base + pt.net.rlinks);
    w.lat = reinterpret_cast<const uint16_t*>(base + pt.net.lat);
    w.inj_lat = reinterpret_cast<const uint16_t*>(base + pt.net.ilat);
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
  sweep_pass(c, pt.d, reinterpret_cast<uint64_t*>(base + pt.st_off), w, pt.np, outs + blockIdx.x, step_cap, hot_lds,
             hot_words);
}

namespace {

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

bool icnt_net_run_chunk(const NetList& list, const std::vector<NetUnit>& units, uint64_t step_cap, bool allow_lds,
                        std::vector<OpenLoopRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, OpenLoopRaw());
  if (!n) return false;
  check_list(list);
  const size_t np = list.src->size();
  ChunkLayout l;
  l.records<NetPt>(n);
  const ListOff o_list = place_list(l, np);
  std::vector<NetPt> h_pts(n);
  uint64_t accounted = icnt_net_list_bytes(list);
  for (size_t i = 0; i < n; ++i) {
    check_unit(list, units[i], i);
    h_pts[i] = place_net_unit(l, units[i]);
    accounted += icnt_net_unit_bytes(units[i]);
  }
  // the launch's LDS: the largest network of the chunk
  const uint64_t hot_bytes = icnt_net_hot_bytes(units);
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  const SweepChunk ch("icnt network sweep", l, accounted);
  ch.up(l.o_pts, h_pts.data(), n * sizeof(NetPt));
  ch.up(o_list.src, list.src->data(), np * 4);
  ch.up(o_list.dst, list.dst->data(), np * 4);
  ch.up(o_list.bytes, list.bytes->data(), np * 4);
  ch.up(o_list.tinj, list.tinj->data(), np * 8);
  for (size_t i = 0; i < n; ++i) ch.up_net(h_pts[i].net, *units[i].net);
  hipLaunchKernelGGL(icnt_net_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     ch.at<const NetPt>(l.o_pts), ch.at<SweepOut>(l.o_out), ch.base(), ch.at<const uint32_t>(o_list.src),
                     ch.at<const uint32_t>(o_list.dst), ch.at<const uint32_t>(o_list.bytes),
                     ch.at<const uint64_t>(o_list.tinj), step_cap, hot_lds ? 1 : 0);
  const std::vector<SweepOut> outs = ch.finish(n, l.o_out);
  for (size_t i = 0; i < n; ++i)
    ch.fetch_raw(raws[i], outs[i], h_pts[i].d, h_pts[i].st_off, device_work(ch, h_pts[i].d, h_pts[i].scr_off).tarr, np);
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_net_kernel_info() { return sweep_kernel_info((const void*)icnt_net_kernel); }

}  // namespace asim
