// Closed-loop request-reply points on the device (icnt_sweep.h): one 64-lane
// workgroup per point runs the closed-loop router pass (model/icnt_closed.h,
// rt_simulate_par_closed<WavePar>) over the doubled network: both subnets on
// one clock, the requests' deliveries creating the replies and the replies'
// deliveries opening the nodes' issue gates inside the one pass.  The whole
// grid of a sweep (window x pattern x seed) is one launch per chunk.  The
// per-(unit, VC) words go in LDS under the kIcntSweepLdsBytes rule; the
// doubled network has twice the units, so they fit less often.
//
// This file holds what is particular to these units: the closed-loop arrays
// and the unit and table checks.  The chunk's layout is icnt_sweep_layout.h;
// the pass (sweep_pass_closed), the chunk's device block and copies
// (SweepChunk) and the resource query are icnt_sweep_dev.h.
//
// Every offset and size is computed and bounded on the host (icnt_cl_run_chunk
// checks the tables and each unit before anything is uploaded): every node is
// below d.N, a request runs on subnet 0 and its reply on subnet 1 between the
// same two nodes, every route of the table is at most d.H links below d.L,
// the flits fit d.nf, and the kernel indexes only what rt_carve(d) and
// rt_cl_carve(d, nq) laid out.  The pass's loop guard (rt_cl_step_cap) ends a
// pass that does not finish.
#include "icnt_sweep_dev.h"

namespace asim {

__global__ __launch_bounds__(64) void icnt_cl_kernel(const SimCfg* cfg, const ClPt* pts, SweepOut* outs, char* base,
                                                     const uint32_t* rt_off, const uint32_t* rt_links,
                                                     const uint16_t* lat, const uint16_t* inj_lat, uint64_t step_cap,
                                                     int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: 5 * U * V words (the host sized the launch)
  const ClPt pt = pts[blockIdx.x];
  if (!pt.nq) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  w.rt_off = rt_off;
  w.rt_links = rt_links;
  w.lat = lat;
  w.inj_lat = inj_lat;
  RtClosed cl;
  cl.window = pt.window;
  cl.delay = pt.delay;
  if (pt.svc_off) {  // the memory endpoint (0: rule 2's reply_delay)
    cl.mem = 1;
    cl.svc = reinterpret_cast<const uint32_t*>(base + pt.svc_off);
  }
  rt_cl_carve(pt.d, pt.nq, reinterpret_cast<uint32_t*>(base + pt.cl_off), &cl);
  sweep_pass_closed(*cfg, pt.d, reinterpret_cast<uint64_t*>(base + pt.st_off), w, cl, outs + blockIdx.x, step_cap,
                    hot_lds, hot_words);
}

namespace {

[[noreturn]] void bad(const char* what) { throw std::invalid_argument(std::string("icnt closed loop: ") + what); }

// the doubled network's tables: one offset per node pair, every route at most
// H links, every link (bit 31: the dateline class) below L
void check_tables(const OpenLoopNet& net, const RtDims& d) {
  const uint64_t pairs = (uint64_t)d.N * d.N;
  if (!net.anynet || d.N != net.N || d.L != net.an_L || d.H != net.an_H) bad("the network is not a table network");
  if (net.rt_off.size() != pairs + 1 || net.rt_off[0] != 0) bad("the route table has the wrong size");
  for (uint64_t i = 0; i < pairs; ++i) {
    if (net.rt_off[i + 1] < net.rt_off[i] || net.rt_off[i + 1] - net.rt_off[i] > d.H) bad("a route is too long");
  }
  if (net.rt_off[pairs] != net.rt_links.size()) bad("the route table has the wrong size");
  for (uint32_t l : net.rt_links)
    if ((l & 0x7fffffffu) >= d.L) bad("a route has a link out of range");
  if (!net.lat.empty() && (net.lat.size() != d.L || net.inj_lat.size() != d.N)) bad("the latency tables have the wrong size");
  if (net.lat.empty() != net.inj_lat.empty()) bad("the latency tables have the wrong size");
}

// std::invalid_argument unless everything the kernel will index lies inside
// what the unit's dimensions lay out
void check_unit(const OpenLoopNet& net, const ClUnit& u) {
  const RtDims& d = u.d;
  if (!u.src || !u.dst || !u.nfl || !u.tinj) bad("a unit's packet list is missing");
  if (u.nq > 0x3fffffffu || 2ull * u.nq > d.np) bad("a unit's packets exceed its dimensions");
  const size_t n2 = 2 * (size_t)u.nq;
  if (u.src->size() != n2 || u.dst->size() != n2 || u.nfl->size() != n2 || u.tinj->size() != u.nq)
    bad("a unit's arrays differ in length");
  if (!u.occ != !u.lat || (u.occ && (u.occ->size() != u.nq || u.lat->size() != u.nq)))
    bad("a unit's occupancy and latency arrays differ in length from its requests");
  if (u.occ)
    for (uint32_t i = 0; i < u.nq; ++i)
      if ((*u.occ)[i] > kRtClMemMax || (*u.lat)[i] > kRtClMemMax) bad("a unit's occupancy or latency is above 2^24");
  if (d.N != net.N || d.N % 2 || d.L != net.an_L || d.U != d.N + d.L || d.H != net.an_H || !d.V || !d.B)
    bad("a unit's network is not the chunk's");
  const uint32_t n = d.N / 2;
  uint64_t flits = 0;
  for (uint32_t i = 0; i < u.nq; ++i) {
    const uint32_t s = (*u.src)[i], t = (*u.dst)[i];
    if (s >= n || t >= n || s == t) bad("a request has a node out of range");
    if ((*u.src)[u.nq + i] != n + t || (*u.dst)[u.nq + i] != n + s) bad("a reply does not answer its request");
    if (!(*u.nfl)[i] || !(*u.nfl)[u.nq + i]) bad("a packet has no flits");
    if (i && (*u.tinj)[i] < (*u.tinj)[i - 1]) bad("the requests are not in time order");
    if (net.rt_off[(uint64_t)s * d.N + t + 1] == net.rt_off[(uint64_t)s * d.N + t] ||
        net.rt_off[(uint64_t)(n + t) * d.N + n + s + 1] == net.rt_off[(uint64_t)(n + t) * d.N + n + s])
      bad("a packet has no route");
    flits += (uint64_t)(*u.nfl)[i] + (*u.nfl)[u.nq + i];
  }
  if (flits > d.nf) bad("a unit's flits exceed its dimensions");
}

}  // namespace

bool icnt_cl_run_chunk(const OpenLoopNet& net, const std::vector<ClUnit>& units, uint64_t step_cap, bool allow_lds,
                       std::vector<ClRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, ClRaw());
  if (!n) return false;
  check_tables(net, units[0].d);
  ChunkLayout l;
  l.records<ClPt>(n);
  const NetOff o_net = place_net(l, net);
  std::vector<ClPt> h_pts(n);
  uint64_t hot_bytes = 0, accounted = icnt_sweep_net_bytes(net);
  for (size_t i = 0; i < n; ++i) {
    check_unit(net, units[i]);
    if (units[i].d.V != units[0].d.V) bad("one network per chunk");
    h_pts[i] = place_cl_unit(l, units[i]);
    hot_bytes = std::max(hot_bytes, icnt_hot_bytes(units[i].d));
    accounted += icnt_cl_unit_bytes(units[i]);
  }
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  const SweepChunk ch("icnt closed loop", l, accounted);
  ch.up(l.o_pts, h_pts.data(), n * sizeof(ClPt));
  SweepChunk::Tables t = ch.up_net(o_net, net);
  if (net.lat.empty()) t.lat = t.inj_lat = nullptr;  // the uniform channel latency
  std::vector<RtWork> dw(n);
  std::vector<RtClosed> dc(n);
  for (size_t i = 0; i < n; ++i) {
    const ClUnit& u = units[i];
    dw[i] = device_work(ch, h_pts[i].d, h_pts[i].scr_off);
    rt_cl_carve(h_pts[i].d, u.nq, ch.at<uint32_t>(h_pts[i].cl_off), &dc[i]);
    const size_t n2 = 2 * (size_t)u.nq;
    ch.up(dw[i].src, u.src->data(), n2 * 4);
    ch.up(dw[i].dst, u.dst->data(), n2 * 4);
    ch.up(dw[i].nfl, u.nfl->data(), n2 * 4);
    ch.up(dw[i].tinj, u.tinj->data(), (size_t)u.nq * 8);  // (the replies' are written by the pass)
    if (u.occ) {
      ch.up(h_pts[i].svc_off, u.occ->data(), (size_t)u.nq * 4);
      ch.up(h_pts[i].svc_off + (uint64_t)u.nq * 4, u.lat->data(), (size_t)u.nq * 4);
    }
  }
  hipLaunchKernelGGL(icnt_cl_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     ch.at<const SimCfg>(o_net.cfg), ch.at<const ClPt>(l.o_pts), ch.at<SweepOut>(l.o_out), ch.base(),
                     t.rt_off, t.rt_links, t.lat, t.inj_lat, step_cap, hot_lds ? 1 : 0);
  const std::vector<SweepOut> outs = ch.finish(n, l.o_out);
  for (size_t i = 0; i < n; ++i) {
    const size_t nq = units[i].nq;
    ch.fetch_raw(raws[i].pass, outs[i], h_pts[i].d, h_pts[i].st_off, dw[i].tarr, 2 * nq);
    raws[i].tiss.assign(nq, 0);
    ch.down(raws[i].tiss.data(), dc[i].tiss, nq * 8);
    if (units[i].occ) {
      raws[i].created.assign(nq, 0);
      ch.down(raws[i].created.data(), dw[i].tinj + nq, nq * 8);
    }
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_cl_kernel_info() { return sweep_kernel_info((const void*)icnt_cl_kernel); }

}  // namespace asim
