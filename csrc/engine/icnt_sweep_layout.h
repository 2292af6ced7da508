// The layout of one chunk of a network sweep launch (icnt_sweep.h), plain C++
// for the HIP build and the CPU-only build alike: what the host fills and the
// kernels read (the descriptors SweepPt / RrPt / NetPt / ClPt / ClNetPt and the
// output record SweepOut), and the ONE routine per kind that places a unit
// into a chunk.
// The driver budgets with `*_bytes`, which places a unit into an empty layout
// and reads the total; `*_run_chunk` places the same units with the same
// routine and allocates the total, so what is accounted is what is allocated
// (SweepChunk, icnt_sweep_dev.h, refuses a block of any other size).
//
// A chunk is: the descriptors, the output records, the fixed part (the
// network of a one-network kind, the shared list of a many-networks kind),
// then what each unit placed.  Every piece starts on 16 bytes, and the records
// are multiples of 16 bytes, so n units cost n times one unit.
#pragma once
#include <cstddef>
#include <cstdint>

#include "icnt_sweep.h"

namespace asim {

// what a pass leaves besides its state and arrivals
struct alignas(16) SweepOut {
  uint64_t act[8];
  uint32_t deadlocked, status;
};
static_assert(RT_ACT_COUNT <= 8, "SweepOut holds the activity counters");

struct ChunkLayout {
  uint64_t bytes = 0, o_pts = 0, o_out = 0;
  uint64_t take(uint64_t n) {
    const uint64_t o = bytes;
    bytes += (n + 15) & ~15ull;
    return o;
  }
  // the descriptor and output arrays of n units, `outs` output records each
  template <class Pt>
  void records(size_t n, size_t outs = 1) {
    o_pts = take(n * sizeof(Pt));
    o_out = take(n * outs * sizeof(SweepOut));
  }
};

// offsets are bytes from the chunk's base
struct SweepPtFields {
  RtDims d;
  uint32_t np, pf;
  uint64_t st_off, scr_off;
};
// (56 bytes of fields in a 64-byte record: the kernel copies the fields only,
// a copy of the whole record costs it 16 bytes of scratch per lane)
struct alignas(16) SweepPt : SweepPtFields {};
struct alignas(16) RrPt {
  RtDims d[2];
  uint32_t np, nsub;  // packets; subnets to run (1: replay, 2: request-reply)
  uint32_t fl_read, fl_write;
  uint64_t delay;
  uint64_t st_off[2], scr_off[2], aux_off;  // aux: kind, reply_of, tmp (np words each)
};
struct NetOff {  // a network: its configuration and anynet tables (empty otherwise)
  uint64_t cfg, roff, rlinks, lat, ilat;
};
struct alignas(16) NetPt {
  RtDims d;
  uint32_t np, anynet;
  NetOff net;
  uint64_t st_off, scr_off;
};
struct alignas(16) ClPt {  // a closed-loop point on the doubled network
  RtDims d;
  uint32_t nq, window;
  uint64_t delay;
  uint64_t st_off, scr_off, cl_off;  // cl: rt_cl_carve(d, nq)
  uint64_t svc_off;                  // the memory endpoint's 2 * nq words (occupancies, latencies); 0 (never a unit's offset): off
};
// a closed-loop unit of a many-networks chunk: one (network, window, memory point) on
// its own doubled network.  net: the unit's SimCfg and doubled route tables;
// net.lat / net.ilat 0 (the descriptors' offset, never a table's): the
// uniform channel latency
struct alignas(16) ClNetPt {
  RtDims d;
  uint32_t nq, window;
  uint64_t delay;
  NetOff net;
  uint64_t st_off, scr_off, cl_off;  // cl: rt_cl_carve(d, nq)
  uint32_t mem, occ, lat, pad_;      // ClMem; CL_MEM_ALL: every request's occupancy and latency
};
struct ListOff {  // the shared list of a many-networks chunk
  uint64_t src, dst, bytes, tinj;
};
struct ClListOff {  // the shared request list of a closed-loop many-networks chunk
  ListOff req;      // src, dst, request bytes, creation times
  uint64_t reply_bytes;
  uint64_t svc;  // the memory endpoint's occupancies, then latencies (no bytes when the list has none)
};
static_assert(sizeof(SweepOut) % 16 == 0 && sizeof(SweepPt) % 16 == 0 && sizeof(RrPt) % 16 == 0 &&
                  sizeof(NetPt) % 16 == 0 && sizeof(ClPt) % 16 == 0 && sizeof(ClNetPt) % 16 == 0,
              "per-unit sums of the record arrays are exact");

// ---- the fixed part of a chunk ----

inline NetOff place_net(ChunkLayout& l, const OpenLoopNet& net) {
  NetOff o;
  o.cfg = l.take(sizeof(SimCfg));
  o.roff = l.take(net.rt_off.size() * 4);
  o.rlinks = l.take(net.rt_links.size() * 4);
  o.lat = l.take(net.lat.size() * 2);
  o.ilat = l.take(net.inj_lat.size() * 2);
  return o;
}

inline ListOff place_list(ChunkLayout& l, uint64_t np) {
  ListOff o;
  o.src = l.take(np * 4);
  o.dst = l.take(np * 4);
  o.bytes = l.take(np * 4);
  o.tinj = l.take(np * 8);
  return o;
}

inline ClListOff place_cl_list(ChunkLayout& l, uint64_t nq, bool mem) {
  ClListOff o;
  o.req = place_list(l, nq);
  o.reply_bytes = l.take(nq * 4);
  o.svc = l.take(mem ? 2 * nq * 4 : 0);
  return o;
}

// ---- a unit: its state and scratch, and its descriptor ----

inline void place_pass(ChunkLayout& l, const RtDims& d, uint64_t& st_off, uint64_t& scr_off) {
  st_off = l.take(rt_state_words(d) * 8);
  scr_off = l.take(rt_carve(d, nullptr, nullptr) * 4);
}

inline SweepPt place_point(ChunkLayout& l, const OpenLoopPoint& p) {
  SweepPt h{};
  h.d = p.d;
  h.np = p.np;
  h.pf = p.pf;
  place_pass(l, h.d, h.st_off, h.scr_off);
  return h;
}

inline RrPt place_rr_unit(ChunkLayout& l, const RrUnit& u) {
  RrPt h{};
  h.d[0] = u.req->d;
  h.d[1] = u.reply ? u.d_rep : u.req->d;
  h.np = u.req->np;
  h.nsub = u.reply ? 2 : 1;
  h.fl_read = u.fl_read;
  h.fl_write = u.fl_write;
  h.delay = u.delay;
  for (uint32_t s = 0; s < h.nsub; ++s) place_pass(l, h.d[s], h.st_off[s], h.scr_off[s]);
  h.aux_off = l.take(3ull * h.np * 4);
  return h;
}

inline NetPt place_net_unit(ChunkLayout& l, const NetUnit& u) {
  NetPt h{};
  h.d = u.pt->d;
  h.np = u.pt->np;
  h.anynet = u.net->anynet ? 1 : 0;
  h.net = place_net(l, *u.net);
  place_pass(l, h.d, h.st_off, h.scr_off);
  return h;
}

inline ClPt place_cl_unit(ChunkLayout& l, const ClUnit& u) {
  ClPt h{};
  h.d = u.d;
  h.nq = u.nq;
  h.window = u.window;
  h.delay = u.delay;
  place_pass(l, h.d, h.st_off, h.scr_off);
  h.cl_off = l.take(rt_cl_carve(h.d, h.nq, nullptr, nullptr) * 4);
  if (u.occ) h.svc_off = l.take(2ull * h.nq * 4);
  return h;
}

inline ClNetPt place_cln_unit(ChunkLayout& l, const ClnUnit& u) {
  ClNetPt h{};
  h.d = u.d;
  h.nq = u.nq;
  h.window = u.window;
  h.delay = u.delay;
  h.mem = u.mem;
  h.occ = u.occ;
  h.lat = u.lat;
  h.net = place_net(l, *u.dbl);
  if (u.dbl->lat.empty()) h.net.lat = h.net.ilat = 0;
  place_pass(l, h.d, h.st_off, h.scr_off);
  h.cl_off = l.take(rt_cl_carve(h.d, h.nq, nullptr, nullptr) * 4);
  return h;
}

// ---- what the driver budgets with ----

// device bytes of a chunk besides its units: the network of an open-loop or
// replay chunk, the list of a many-networks chunk
inline uint64_t icnt_sweep_net_bytes(const OpenLoopNet& net) {
  ChunkLayout l;
  place_net(l, net);
  return l.bytes;
}
inline uint64_t icnt_net_list_bytes(const NetList& list) {
  ChunkLayout l;
  place_list(l, list.src ? list.src->size() : 0);
  return l.bytes;
}
inline uint64_t icnt_cln_list_bytes(const ClList& list) {
  ChunkLayout l;
  place_cl_list(l, list.src ? list.src->size() : 0, list.occ != nullptr);
  return l.bytes;
}

// device bytes a unit adds to a chunk (records, state, scratch; a network
// unit's configuration and tables, a closed-loop network unit's doubled ones)
inline uint64_t icnt_sweep_point_bytes(const OpenLoopPoint& pt) {
  ChunkLayout l;
  l.records<SweepPt>(1);
  place_point(l, pt);
  return l.bytes;
}
inline uint64_t icnt_rr_unit_bytes(const RrUnit& u) {
  ChunkLayout l;
  l.records<RrPt>(1, 2);
  place_rr_unit(l, u);
  return l.bytes;
}
inline uint64_t icnt_cl_unit_bytes(const ClUnit& u) {
  ChunkLayout l;
  l.records<ClPt>(1);
  place_cl_unit(l, u);
  return l.bytes;
}
inline uint64_t icnt_net_unit_bytes(const NetUnit& u) {
  ChunkLayout l;
  l.records<NetPt>(1);
  place_net_unit(l, u);
  return l.bytes;
}

inline uint64_t icnt_cln_unit_bytes(const ClnUnit& u) {
  ChunkLayout l;
  l.records<ClNetPt>(1);
  place_cln_unit(l, u);
  return l.bytes;
}

}  // namespace asim
