// Closed-loop request-reply traffic with bounded windows: the rules a router
// pass needs on top of RtCtx (icnt_router.h, which includes this file after
// RtCtx) when a request's delivery creates its reply and a reply's delivery
// lets its node issue again.  Reference: intersim2/batchtrafficmanager.cpp
// (sim_type = batch: batch_size, max_outstanding_requests).
//
// The pass runs over the doubled network: two disjoint copies of one network,
// nodes [0, N) with links [0, L) the request subnet and nodes [N, 2N) with
// links [L, 2L) the reply subnet, routes from tables (RtWork::rt_off).  It
// holds 2 * nq packets:
//   request i       src[i] -> dst[i]          i in [0, nq), time-ordered
//   reply  nq + i   N + dst[i] -> N + src[i]  flits by the request's kind
// A reply's source, destination and flits are known up front (rt_cl_fill_reply;
// rt_cl_fill_list for a request list in bytes); its injection time is not.
//
// Rules (one element each, like RtCtx's members; the drivers decide the order
// and the parallelism):
//  1. Issue gate (rt_cl_gate).  Node s issues its requests in list order.
//     Request k is issued at the smallest cycle t >= max(tinj[k], tiss[k-1])
//     at which fewer than `window` of the node's earlier requests are
//     outstanding; a request is outstanding from its issue until the arrival
//     of its reply's tail at s, and a reply arriving at t frees its slot for
//     t.  window 0: unlimited.  From its issue on a request is an ordinary
//     packet of its node's source queue with injection time tiss (w.tinj is
//     overwritten: before the issue it holds the creation time).  Several
//     requests of a node may issue in one cycle.  Booksim issues at most one
//     packet per node and cycle and lets a pending reply take the node's
//     injection slot; here the reply leaves from the other subnet's terminal.
//  2. Reply creation (rt_cl_delivered, a request).  A request whose tail is
//     delivered with arrival arr creates its reply with tinj = arr + delay at
//     the tail of node N + dst's source queue.  Arrivals at a node come over
//     its one ejection link and strictly increase, so the tail append keeps
//     the queue in (time, packet) order.
//  2m. Reply creation with a memory endpoint (cl.mem set; rt_cl_delivered).
//     The memory node n = N + dst is one server, first come first served, with
//     a pipelined latency behind it.  Request i holds the server for occ[i]
//     cycles and its reply leaves lat[i] cycles after the server is done:
//       start   = max(arr, busy[n])
//       busy[n] = start + occ[i]
//       ready   = busy[n] + lat[i]
//       tinj    = ready                    if n created no reply yet
//                 max(ready, last[n] + 1)  otherwise
//       last[n] = tinj
//     busy[n] starts at 0.  The last line is a modelling choice: replies leave
//     a node in the order their requests arrived, so a fast reply can be held
//     one cycle behind a slow older one (the cycle simulation's L2 returns
//     replies in completion order).  It keeps a node's creation times strictly
//     increasing when latencies differ, so the tail append still keeps the
//     queue in (time, packet) order and the source-list key, source_time and
//     the next-event scan need no sorted insert.  With occ = 0 and lat = delay
//     for every request this is rule 2: a node's arrivals strictly increase,
//     so busy never exceeds arr and the hold never binds.  occ and lat are
//     read-only inputs (svc: [nq] each, or one pair of scalars for every request);
//     busy[n] and last[n] belong to the lane of the packet delivered at n.
//  3. Release (rt_cl_delivered, a reply).  The reply's arrival is queued on
//     its requester's release list, in time order for the same reason, and
//     applied by the gate at the top of the cycle it falls due.
//
// The source list.  Open loop, a source is listed from the start, in the
// order of the sources' first packets, until its queue runs empty for good.
// The list's order decides the order of the active list and so of the request
// list, which the maximum-size allocator depends on.  To give that order here,
// a source is listed from its first packet (a request node at setup, a reply
// node when its first reply is created: rt_cl_list_source inserts it by the
// key (time, packet) of that packet) until it has injected the last packet it
// will ever have (`left`), also while its queue is empty.  With an unlimited
// window the pass then is, subnet by subnet, the open-loop request-reply pass
// (for the allocators whose matching does not depend on unit indices, which
// the doubled network renumbers -- not wavefront and PIM -- and for whole
// internal speedups: a fractional one adds its extra pass per loop iteration,
// and this pass iterates through the union of both subnets' busy cycles).
//
// Events: besides the sources', units' and credits' times the next-event scan
// sees rt_cl_gate_time: the creation time of a node's next request while its
// gate is open, its earliest queued release while it is closed.  These add at
// most 2 * nq event times to a pass (rt_cl_step_cap).  A memory endpoint adds
// none: it moves a reply's creation time, which is the source event of that
// packet already counted among the injections, and a pass still ends no later
// than after one event per counted item.
#pragma once

namespace asim {

// the largest occupancy and latency of rule 2m: the times of the 25 million
// requests a pass may hold stay far inside 64 bits
constexpr uint32_t kRtClMemMax = 1u << 24;

// parameters and work arrays of a closed-loop pass; d.N is the doubled network's
struct RtClosed {
  uint32_t nq = 0;      // requests (the pass has 2 * nq packets)
  uint32_t window = 0;  // outstanding requests per node, 0: unlimited
  uint64_t delay = 0;   // request arrival to reply creation
  uint64_t* tiss = nullptr;  // [nq] issue time, ~0: not issued
  uint32_t *gnext = nullptr, *rnext = nullptr;  // [nq] a node's next request; its next queued release
  // [d.N] next request to issue, last request (setup), release list, requests
  // outstanding, packets still to inject, the first packet ever queued
  uint32_t *ghead = nullptr, *gtail = nullptr, *rhead = nullptr, *rtail = nullptr, *out = nullptr, *left = nullptr,
           *sfirst = nullptr;
  // rule 2m (mem 0: rule 2, nothing below is read)
  uint32_t mem = 0;
  uint32_t occ_all = 0, lat_all = 0;  // every request's, when svc is null
  // [2 * nq] per request, read only (not carved): occ[i] = svc[i], lat[i] = svc[nq + i]
  const uint32_t* svc = nullptr;
  // [2 * d.N] node n's busy (the server is free from) and last (the last creation, ~0: none) at 2 * n, 2 * n + 1
  uint64_t* node = nullptr;
};

// carve the closed-loop arrays out of `base` (nullptr: size only); u32 words
SIM_HDI uint64_t rt_cl_carve(const RtDims& d, uint32_t nq, uint32_t* base, RtClosed* cl) {
  uint64_t off = 0;
  auto take32 = [&](uint64_t n) -> uint32_t* {
    uint32_t* p = base ? base + off : nullptr;
    off += n;
    return p;
  };
  RtClosed t = cl ? *cl : RtClosed();
  t.nq = nq;
  t.tiss = reinterpret_cast<uint64_t*>(take32(2ull * nq));  // (base is 8-byte aligned)
  t.node = reinterpret_cast<uint64_t*>(take32(4ull * d.N));
  t.gnext = take32(nq);
  t.rnext = take32(nq);
  t.ghead = take32(d.N);
  t.gtail = take32(d.N);
  t.rhead = take32(d.N);
  t.rtail = take32(d.N);
  t.out = take32(d.N);
  t.left = take32(d.N);
  t.sfirst = take32(d.N);
  if (cl) *cl = t;
  return (off + 1) & ~1ull;
}

SIM_HDI uint64_t rt_cl_step_cap(const RtDims& d, uint64_t flits, uint32_t nq) {
  return rt_step_cap(d, flits) + kRtGuardFactor * 2ull * nq;
}

// reply nq + i of request i on an n-node network: src / dst / nfl of the pass
SIM_HDI void rt_cl_fill_reply(uint32_t* src, uint32_t* dst, uint32_t* nfl, uint32_t nq, uint32_t i, uint32_t n,
                              uint32_t write, uint32_t fl_read, uint32_t fl_write) {
  src[nq + i] = n + dst[i];
  dst[nq + i] = n + src[i];
  nfl[nq + i] = write ? fl_write : fl_read;
}

// A request list in bytes (for example the requests of an -icnt_capture file,
// icnt/capture.py request_list): request i goes from src[i] to dst[i] with
// req_bytes[i] bytes, is created at tcreate[i] (non-decreasing) and is
// answered by reply_bytes[i] bytes.  What a packet weighs in flits depends on
// the network that carries it.
struct RtClList {
  const uint32_t *src = nullptr, *dst = nullptr, *req_bytes = nullptr, *reply_bytes = nullptr;
  const uint64_t* tcreate = nullptr;
  uint32_t nq = 0;
};

// the pass's 2 * nq packets from the list, for the network of c (n nodes per
// subnet), a lane per request: w.src / w.dst / w.nfl of both packets and the
// request's w.tinj (its creation time until its issue).  Flits as a
// many-networks replay derives them (engine/icnt_net_sweep.hip):
//   nfl = min(rt_flits(c, bytes), rt_flits(c, kRtMaxPktBytes))
// The caller syncs before the pass.
template <class P>
SIM_HDI void rt_cl_fill_list(const SimCfg& c, const RtClList& l, uint32_t n, const RtWork& w) {
  const uint32_t nq = l.nq, nfl_max = rt_flits(c, kRtMaxPktBytes);
  P::each((int)nq, [&](int i) {
    const uint32_t s = l.src[i], t = l.dst[i];
    const uint32_t fq = rt_flits(c, l.req_bytes[i]), fp = rt_flits(c, l.reply_bytes[i]);
    w.src[i] = s;
    w.dst[i] = t;
    w.tinj[i] = l.tcreate[i];
    w.nfl[i] = fq < nfl_max ? fq : nfl_max;
    w.src[nq + i] = n + t;
    w.dst[nq + i] = n + s;
    w.nfl[nq + i] = fp < nfl_max ? fp : nfl_max;
  });
}

// packet p to the tail of node s's source queue
SIM_HDI void rt_cl_enqueue(const RtWork& w, uint32_t s, uint32_t p) {
  if (w.shead[s] == kRtNone) w.shead[s] = p;
  else w.next[w.stail[s]] = p;
  w.stail[s] = p;
}

// setup, single-threaded, after init_packet of every packet: the nodes'
// request lists and packet counts; the request nodes enter the source list
// in the order of their first requests
template <class CX>
SIM_HDI void rt_cl_setup(const CX& cx, const RtClosed& cl, uint32_t& nsrc) {
  const RtWork& w = cx.w;
  for (uint32_t s = 0; s < cx.N; ++s) {
    cl.ghead[s] = cl.gtail[s] = cl.rhead[s] = cl.rtail[s] = cl.sfirst[s] = kRtNone;
    cl.out[s] = cl.left[s] = 0;
    if (cl.mem) {
      cl.node[2 * s] = 0;
      cl.node[2 * s + 1] = ~0ull;
    }
  }
  for (uint32_t i = 0; i < cl.nq; ++i) {
    const uint32_t s = w.src[i];
    cl.tiss[i] = ~0ull;
    cl.gnext[i] = cl.rnext[i] = kRtNone;
    if (cl.ghead[s] == kRtNone) {
      cl.ghead[s] = cl.sfirst[s] = i;
      w.sflag[s] = 1;
      w.slist[nsrc++] = s;
    } else {
      cl.gnext[cl.gtail[s]] = i;
    }
    cl.gtail[s] = i;
    ++cl.left[s];
    ++cl.left[w.src[cl.nq + i]];
  }
}

// rule 1 and the due part of rule 3 for node s at the top of cycle `now`
template <class CX>
SIM_HDI void rt_cl_gate(const CX& cx, const RtClosed& cl, uint32_t s, uint64_t now) {
  const RtWork& w = cx.w;
  for (uint32_t r; (r = cl.rhead[s]) != kRtNone && w.tarr[cl.nq + r] <= now;) {
    --cl.out[s];
    cl.rhead[s] = cl.rnext[r];
  }
  for (uint32_t p; (p = cl.ghead[s]) != kRtNone && w.tinj[p] <= now && (!cl.window || cl.out[s] < cl.window);) {
    cl.tiss[p] = now;
    w.tinj[p] = now;
    ++cl.out[s];
    cl.ghead[s] = cl.gnext[p];
    rt_cl_enqueue(w, s, p);
  }
}

// the next time node s's gate can do anything (~0: never without another event)
template <class CX>
SIM_HDI uint64_t rt_cl_gate_time(const CX& cx, const RtClosed& cl, uint32_t s) {
  const uint32_t p = cl.ghead[s];
  if (p == kRtNone) return ~0ull;
  if (!cl.window || cl.out[s] < cl.window) return cx.w.tinj[p];
  const uint32_t r = cl.rhead[s];
  return r == kRtNone ? ~0ull : cx.w.tarr[cl.nq + r];
}

// a listed source s stays listed while it has packets to inject, queued or not
SIM_HDI bool rt_cl_listed(const RtClosed& cl, uint32_t s) { return cl.left[s] != 0; }
// source s injected the last flit of a packet
SIM_HDI void rt_cl_injected(const RtClosed& cl, uint32_t s) { --cl.left[s]; }

// rule 2m: the creation time of the reply of request i, delivered at memory
// node n with arrival arr
SIM_HDI uint64_t rt_cl_mem_serve(const RtClosed& cl, uint32_t i, uint32_t n, uint64_t arr) {
  const uint64_t oc = cl.svc ? cl.svc[i] : cl.occ_all, la = cl.svc ? cl.svc[cl.nq + i] : cl.lat_all;
  uint64_t* w = cl.node + 2 * (uint64_t)n;
  const uint64_t b = w[0], done = (arr > b ? arr : b) + oc, last = w[1];
  uint64_t t = done + la;
  if (last != ~0ull && t <= last) t = last + 1;
  w[0] = done;
  w[1] = t;
  return t;
}

// rules 2 and 3: the tail of packet p was delivered (w.tarr[p] is set).
// Returns the reply node that queued its first packet and is to be listed
// (rt_cl_list_source), else kRtNone.  Two packets delivered in one switch pass
// arrive at different nodes, so they touch different queues, lists and
// memory-endpoint words.
template <class CX>
SIM_HDI uint32_t rt_cl_delivered(const CX& cx, const RtClosed& cl, uint32_t p) {
  const RtWork& w = cx.w;
  if (p < cl.nq) {
    const uint32_t q = cl.nq + p, n = w.src[q];
    w.tinj[q] = cl.mem ? rt_cl_mem_serve(cl, p, n, w.tarr[p]) : w.tarr[p] + cl.delay;
    rt_cl_enqueue(w, n, q);
    if (cl.sfirst[n] != kRtNone) return kRtNone;
    cl.sfirst[n] = q;
    return n;
  }
  const uint32_t i = p - cl.nq, s = w.src[i];
  if (cl.rhead[s] == kRtNone) cl.rhead[s] = i;
  else cl.rnext[cl.rtail[s]] = i;
  cl.rtail[s] = i;
  return kRtNone;
}

// list source n by the (time, packet) key of its first packet; single-threaded
template <class CX>
SIM_HDI void rt_cl_list_source(const CX& cx, const RtClosed& cl, uint32_t n, uint32_t& nsrc) {
  const RtWork& w = cx.w;
  const uint32_t fp = cl.sfirst[n];
  uint32_t i = nsrc++;
  for (; i > 0; --i) {
    const uint32_t o = cl.sfirst[w.slist[i - 1]];
    if (w.tinj[o] < w.tinj[fp] || (w.tinj[o] == w.tinj[fp] && o < fp)) break;
    w.slist[i] = w.slist[i - 1];
  }
  w.slist[i] = n;
  w.sflag[n] = 1;
}

}  // namespace asim
