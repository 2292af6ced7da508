// One request list, closed loop, over many networks and windows on the device
// (icnt_sweep.h): one 64-lane workgroup per (network, window) unit runs the
// closed-loop router pass (model/icnt_closed.h,
// rt_simulate_par_closed<WavePar>) over that network's doubled network.  As in
// icnt_net_kernel every workgroup reads its own SimCfg, RtDims, offsets and
// tables from its descriptor, so one launch runs an application's captured
// requests on a whole grid of candidate networks and windows.
//
// The list (src, dst, request bytes, reply bytes, creation times) is uploaded
// once per chunk.  Each unit fills its own 2 * nq packets from it, lane-strided
// (rt_cl_fill_list), deriving both packets' flits from their bytes with that
// unit's flit size:
//   nfl = min(rt_flits(c, bytes), rt_flits(c, kRtMaxPktBytes))
// (the host computed the same numbers to size and bound the unit).  The memory
// endpoint's per-request occupancy and latency arrays, when the list has them,
// are uploaded with it; a unit reads them (CL_MEM_LIST), uses its descriptor's
// two scalars for every request (CL_MEM_ALL) or takes rule 2's reply_delay.
//
// The per-(unit, VC) words go in LDS under the kIcntSweepLdsBytes rule, applied
// to the LARGEST 5 * U * V words among the chunk's doubled networks, for which
// the launch's dynamic LDS is sized: every workgroup carves its own U * V out
// of it.  If the largest does not fit, the whole chunk keeps them in HBM.
//
// Every offset and size is computed and bounded on the host (icnt_cln_run_chunk
// checks the list and each unit before anything is uploaded): every node is
// below the unit's single network's node count, so a request runs on subnet 0
// and its reply on subnet 1, every route of the unit's table is at most d.H
// links below d.L, the flits fit d.nf, and the kernel indexes only the list's
// nq entries and what rt_carve(d) and rt_cl_carve(d, nq) laid out.  The pass's
// loop guard (rt_cl_step_cap) ends a pass that does not finish.
//
// This file holds what is particular to these units: the unit's own tables and
// the list, table and unit checks.  The chunk's layout is icnt_sweep_layout.h;
// the pass (sweep_pass_closed), the chunk's device block and copies
// (SweepChunk) and the resource query are icnt_sweep_dev.h.
#include "icnt_sweep_dev.h"

namespace asim {

__global__ __launch_bounds__(64) void icnt_cln_kernel(const ClNetPt* pts, SweepOut* outs, char* base,
                                                      const uint32_t* l_src, const uint32_t* l_dst,
                                                      const uint32_t* l_req_bytes, const uint32_t* l_reply_bytes,
                                                      const uint64_t* l_tcreate, const uint32_t* l_svc,
                                                      uint64_t step_cap, int hot_lds) {
  extern __shared__ uint32_t hot_words[];  // hot_lds: the chunk's largest 5 * U * V words (the host sized the launch)
  const ClNetPt pt = pts[blockIdx.x];
  if (!pt.nq) return;  // (the chunk was cleared: no activity, nothing lost, status OK)
  const SimCfg& c = *reinterpret_cast<const SimCfg*>(base + pt.net.cfg);
  RtWork w;
  rt_carve(pt.d, reinterpret_cast<uint32_t*>(base + pt.scr_off), &w);
  w.rt_off = reinterpret_cast<const uint32_t*>(base + pt.net.roff);
  w.rt_links = reinterpret_cast<const uint32_t*>(base + pt.net.rlinks);
  if (pt.net.lat) {  // (0: the uniform channel latency)
    w.lat = reinterpret_cast<const uint16_t*>(base + pt.net.lat);
    w.inj_lat = reinterpret_cast<const uint16_t*>(base + pt.net.ilat);
  }
  RtClosed cl;
  cl.window = pt.window;
  cl.delay = pt.delay;
  if (pt.mem != CL_MEM_OFF) {
    cl.mem = 1;
    cl.occ_all = pt.occ;
    cl.lat_all = pt.lat;
    if (pt.mem == CL_MEM_LIST) cl.svc = l_svc;
  }
  rt_cl_carve(pt.d, pt.nq, reinterpret_cast<uint32_t*>(base + pt.cl_off), &cl);
  // this network's packets from the shared list
  RtClList l;
  l.src = l_src;
  l.dst = l_dst;
  l.req_bytes = l_req_bytes;
  l.reply_bytes = l_reply_bytes;
  l.tcreate = l_tcreate;
  l.nq = pt.nq;
  rt_cl_fill_list<WavePar>(c, l, pt.d.N / 2, w);
  WavePar::sync();
  sweep_pass_closed(c, pt.d, reinterpret_cast<uint64_t*>(base + pt.st_off), w, cl, outs + blockIdx.x, step_cap, hot_lds,
                    hot_words);
}

namespace {

void check_list(const ClList& l) {
  if (!l.src || !l.dst || !l.req_bytes || !l.reply_bytes || !l.tcreate)
    throw std::invalid_argument("icnt closed-loop network sweep: the request list is missing");
  const size_t n = l.src->size();
  if (l.dst->size() != n || l.req_bytes->size() != n || l.reply_bytes->size() != n || l.tcreate->size() != n ||
      n > 0x3fffffffu)
    throw std::invalid_argument("icnt closed-loop network sweep: the request list's arrays differ in length");
  for (size_t i = 1; i < n; ++i)
    if ((*l.tcreate)[i] < (*l.tcreate)[i - 1])
      throw std::invalid_argument("icnt closed-loop network sweep: the requests are not in time order");
  if (!l.occ != !l.lat || (l.occ && (l.occ->size() != n || l.lat->size() != n)))
    throw std::invalid_argument("icnt closed-loop network sweep: the occupancy and latency arrays differ in length from the list");
  if (l.occ)
    for (size_t i = 0; i < n; ++i)
      if ((*l.occ)[i] > kRtClMemMax || (*l.lat)[i] > kRtClMemMax)
        throw std::invalid_argument("icnt closed-loop network sweep: an occupancy or latency is above 2^24");
}

// std::invalid_argument unless everything the kernel will index lies inside
// what the unit's dimensions and tables lay out.  tables: check the doubled
// network's tables too (false: this unit has the network of the unit before
// it, which was checked)
void check_unit(const ClList& l, const ClnUnit& u, size_t index, bool tables) {
  auto bad = [&](const char* what) {
    throw std::invalid_argument("icnt closed-loop network sweep: unit " + std::to_string(index) + "'s " + what);
  };
  if (!u.dbl || !u.nfl) bad("description is missing");
  const OpenLoopNet& net = *u.dbl;
  const RtDims& d = u.d;
  const size_t nq = l.src->size();
  if (u.nq != nq || 2 * nq > d.np) bad("packets exceed its dimensions");
  if (u.nfl->size() != 2 * nq) bad("flit counts differ in length");
  if (u.mem > CL_MEM_LIST || (u.mem == CL_MEM_LIST && !l.occ)) bad("memory point needs the list's occupancy and latency");
  if (u.mem == CL_MEM_ALL && (u.occ > kRtClMemMax || u.lat > kRtClMemMax)) bad("occupancy or latency is above 2^24");
  if (!net.anynet || d.N != net.N || d.N % 2 || d.L != net.an_L || d.U != d.N + d.L || d.H != net.an_H || !d.V ||
      !d.B || !d.H)
    bad("dimensions are not its doubled network's");
  if (!net.c.flit_size) bad("flit size is zero");
  const uint64_t pairs = (uint64_t)d.N * d.N;
  if (tables) {
    // one offset per node pair, every route at most H links, every link (bit 31: the dateline class) below L
    if (net.rt_off.size() != pairs + 1 || net.rt_off[0] != 0) bad("route table has the wrong size");
    for (uint64_t i = 0; i < pairs; ++i)
      if (net.rt_off[i + 1] < net.rt_off[i] || net.rt_off[i + 1] - net.rt_off[i] > d.H) bad("routes exceed its longest route");
    if (net.rt_off[pairs] != net.rt_links.size()) bad("route table has the wrong size");
    for (uint32_t x : net.rt_links)
      if ((x & 0x7fffffffu) >= d.L) bad("route names a link out of range");
    if (net.lat.empty() != net.inj_lat.empty() ||
        (!net.lat.empty() && (net.lat.size() != d.L || net.inj_lat.size() != d.N)))
      bad("latency tables have the wrong size");
  }
  const uint32_t n = d.N / 2, nfl_max = rt_flits(net.c, kRtMaxPktBytes);
  uint64_t flits = 0;
  for (size_t i = 0; i < nq; ++i) {
    const uint32_t s = (*l.src)[i], t = (*l.dst)[i];
    if (s >= n || t >= n || s == t) bad("request has a node out of range");
    // what the device will compute
    const uint32_t fq = std::min(rt_flits(net.c, (*l.req_bytes)[i]), nfl_max);
    const uint32_t fp = std::min(rt_flits(net.c, (*l.reply_bytes)[i]), nfl_max);
    if (fq != (*u.nfl)[i] || fp != (*u.nfl)[nq + i]) bad("flit counts are not those of its flit size");
    if (net.rt_off[(uint64_t)s * d.N + t + 1] == net.rt_off[(uint64_t)s * d.N + t] ||
        net.rt_off[(uint64_t)(n + t) * d.N + n + s + 1] == net.rt_off[(uint64_t)(n + t) * d.N + n + s])
      bad("packet has no route");
    flits += (uint64_t)fq + fp;
  }
  if (flits > d.nf) bad("flits exceed its dimensions");
}

}  // namespace

bool icnt_cln_run_chunk(const ClList& list, const std::vector<ClnUnit>& units, uint64_t step_cap, bool allow_lds,
                        std::vector<ClRaw>& raws) {
  const size_t n = units.size();
  raws.assign(n, ClRaw());
  if (!n) return false;
  check_list(list);
  const size_t nq = list.src->size();
  ChunkLayout l;
  l.records<ClNetPt>(n);
  const ClListOff o_list = place_cl_list(l, nq, list.occ != nullptr);
  std::vector<ClNetPt> h_pts(n);
  uint64_t accounted = icnt_cln_list_bytes(list);
  for (size_t i = 0; i < n; ++i) {
    check_unit(list, units[i], i, !i || units[i].dbl != units[i - 1].dbl);
    h_pts[i] = place_cln_unit(l, units[i]);
    accounted += icnt_cln_unit_bytes(units[i]);
  }
  // the launch's LDS: the largest doubled network of the chunk
  const uint64_t hot_bytes = icnt_cln_hot_bytes(units);
  const bool hot_lds = allow_lds && hot_bytes <= kIcntSweepLdsBytes;
  const SweepChunk ch("icnt closed-loop network sweep", l, accounted);
  ch.up(l.o_pts, h_pts.data(), n * sizeof(ClNetPt));
  ch.up(o_list.req.src, list.src->data(), nq * 4);
  ch.up(o_list.req.dst, list.dst->data(), nq * 4);
  ch.up(o_list.req.bytes, list.req_bytes->data(), nq * 4);
  ch.up(o_list.req.tinj, list.tcreate->data(), nq * 8);
  ch.up(o_list.reply_bytes, list.reply_bytes->data(), nq * 4);
  if (list.occ) {
    ch.up(o_list.svc, list.occ->data(), nq * 4);
    ch.up(o_list.svc + nq * 4, list.lat->data(), nq * 4);
  }
  for (size_t i = 0; i < n; ++i) ch.up_net(h_pts[i].net, *units[i].dbl);  // (empty latency tables: nothing is copied)
  hipLaunchKernelGGL(icnt_cln_kernel, dim3((unsigned)n), dim3(64), hot_lds ? (size_t)hot_bytes : 0, 0,
                     ch.at<const ClNetPt>(l.o_pts), ch.at<SweepOut>(l.o_out), ch.base(),
                     ch.at<const uint32_t>(o_list.req.src), ch.at<const uint32_t>(o_list.req.dst),
                     ch.at<const uint32_t>(o_list.req.bytes), ch.at<const uint32_t>(o_list.reply_bytes),
                     ch.at<const uint64_t>(o_list.req.tinj), ch.at<const uint32_t>(o_list.svc),
                     step_cap, hot_lds ? 1 : 0);
  const std::vector<SweepOut> outs = ch.finish(n, l.o_out);
  for (size_t i = 0; i < n; ++i) {
    const RtWork dw = device_work(ch, h_pts[i].d, h_pts[i].scr_off);
    ch.fetch_raw(raws[i].pass, outs[i], h_pts[i].d, h_pts[i].st_off, dw.tarr, 2 * nq);
    RtClosed dc;
    rt_cl_carve(h_pts[i].d, (uint32_t)nq, ch.at<uint32_t>(h_pts[i].cl_off), &dc);
    raws[i].tiss.assign(nq, 0);
    ch.down(raws[i].tiss.data(), dc.tiss, nq * 8);
    if (units[i].mem != CL_MEM_OFF) {
      raws[i].created.assign(nq, 0);
      ch.down(raws[i].created.data(), dw.tinj + nq, nq * 8);
    }
  }
  return hot_lds;
}

std::map<std::string, uint64_t> icnt_cln_kernel_info() { return sweep_kernel_info((const void*)icnt_cln_kernel); }

}  // namespace asim
