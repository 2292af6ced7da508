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
// under the same kIcntSweepLdsBytes rule; the reply pass reuses them.
//
// This file holds what is particular to these units: the uploaded flit
// counts, the two-subnet loop and the unit checks.  The chunk's layout is
// icnt_sweep_layout.h; the pass (sweep_pass), the chunk's device block and
// copies (SweepChunk) and the resource query are icnt_sweep_dev.h.
//
// Every offset and size is computed and bounded on the host (icnt_rr_run_chunk
// checks each unit before anything is uploaded): a subnet's packets and flits
// are its RtDims' capacities, every node index is below N, and the kernel
// indexes only what rt_carve(d) and the unit's three np-word arrays laid out.
#include "icnt_sweep_dev.h"
#include "../model/icnt_reqreply.h"

namespace asim {

__global__ __launch_bounds__(64) void icnt_rr_kernel(const SimCfg* cfg, const RrPt* pts, SweepOut* outs, char* base,
                                                     const uint32_t* rt_off, const uint32_t* rt_links,
                                                     const uint16_t* lat, const uint16_t* inj_lat, uint64_t step_cap,
                                                     int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: 5 * U * V words (the host sized the launch)
  const RrPt pt = pts[blockIdx.x];
  SweepOut* o = outs + 2 * (size_t)blockIdx.x;  // one record per subnet
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
    sweep_pass(*cfg, pt.d[sub], reinterpret_cast<uint64_t*>(base + pt.st_off[sub]), w, pt.np, o + sub, step_cap,
               hot_lds, hot_words);
    WavePar::sync();
    // a pass cut off by its guard leaves no arrivals to reply to
    if (WavePar::uni(o[sub].status) != RT_STATUS_OK) return;
  }
}

namespace {

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

bool icnt_rr_run_chunk(const OpenLoopNet& net, const std::vector<RrUnit>& units, uint64_t step_cap, bool allow_lds,
                       std::vector<RrRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, RrRaw());
  if (!n) return false;
  ChunkLayout l;
  l.records<RrPt>(n, 2);
  const NetOff o_net = place_net(l, net);
  std::vector<RrPt> h_pts(n);
  uint64_t hot_bytes = 0, accounted = icnt_sweep_net_bytes(net);
  for (size_t i = 0; i < n; ++i) {
    const RrUnit& u = units[i];
    check_unit(net, u);
    // one network per chunk: every unit has the same U and V (its reply subnet too: check_unit)
    if (u.req->d.U != units[0].req->d.U || u.req->d.V != units[0].req->d.V)
      throw std::invalid_argument("icnt replay: one network per chunk");
    h_pts[i] = place_rr_unit(l, u);
    hot_bytes = std::max(hot_bytes, icnt_hot_bytes(u.req->d));
    accounted += icnt_rr_unit_bytes(u);
  }
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  const SweepChunk ch("icnt replay", l, accounted);
  ch.up(l.o_pts, h_pts.data(), n * sizeof(RrPt));
  const SweepChunk::Tables t = ch.up_net(o_net, net);
  std::vector<RtWork> dw(2 * n);  // the subnets' work arrays as device addresses
  for (size_t i = 0; i < n; ++i) {
    const RrUnit& u = units[i];
    const OpenLoopPoint& p = *u.req;
    for (uint32_t s = 0; s < h_pts[i].nsub; ++s) dw[2 * i + s] = device_work(ch, h_pts[i].d[s], h_pts[i].scr_off[s]);
    const size_t np = p.np;
    ch.up(dw[2 * i].src, p.src.data(), np * 4);
    ch.up(dw[2 * i].dst, p.dst.data(), np * 4);
    ch.up(dw[2 * i].nfl, p.nfl.data(), np * 4);
    ch.up(dw[2 * i].tinj, p.tinj.data(), np * 8);
    if (u.reply) ch.up(h_pts[i].aux_off, u.kind->data(), np * 4);
  }
  hipLaunchKernelGGL(icnt_rr_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     ch.at<const SimCfg>(o_net.cfg), ch.at<const RrPt>(l.o_pts), ch.at<SweepOut>(l.o_out), ch.base(),
                     t.rt_off, t.rt_links, t.lat, t.inj_lat, step_cap, hot_lds ? 1 : 0);
  const std::vector<SweepOut> outs = ch.finish(2 * n, l.o_out);
  for (size_t i = 0; i < n; ++i) {
    const size_t np = units[i].req->np;
    const RrPt& h = h_pts[i];
    RrRaw& r = raws[i];
    for (uint32_t s = 0; s < h.nsub; ++s)
      ch.fetch_raw(s ? r.rep : r.req, outs[2 * i + s], h.d[s], h.st_off[s], dw[2 * i + s].tarr, np);
    if (!units[i].reply) continue;
    r.reply_of.assign(np, 0);
    r.rep_src.assign(np, 0);
    r.rep_dst.assign(np, 0);
    r.rep_nfl.assign(np, 0);
    r.rep_tinj.assign(np, 0);
    ch.down(r.reply_of.data(), ch.base() + h.aux_off + np * 4, np * 4);
    ch.down(r.rep_src.data(), dw[2 * i + 1].src, np * 4);
    ch.down(r.rep_dst.data(), dw[2 * i + 1].dst, np * 4);
    ch.down(r.rep_nfl.data(), dw[2 * i + 1].nfl, np * 4);
    ch.down(r.rep_tinj.data(), dw[2 * i + 1].tinj, np * 8);
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_rr_kernel_info() { return sweep_kernel_info((const void*)icnt_rr_kernel); }

}  // namespace asim
