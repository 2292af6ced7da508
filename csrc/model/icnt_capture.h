// -icnt_capture: the cycle engines' network traffic as a packet list.
//
// Every SM-to-L2 request and every L2-to-SM reply crosses the per-epoch
// mailboxes exactly once (a packet the destination cannot take yet waits in
// its backlog ring after it left the mailbox), so one record per mailbox
// packet is the whole traffic.  The records carry the packet as the router
// pass sees it (rt_cell, rt_fill_packet) plus its size in bytes, from which
// a replay on another network derives that network's flit count.
//
// Capture file, little-endian:
//
//   IcntCapHeader (64 bytes)
//     u64 magic        "ASIMICAP" (kIcntCapMagic)
//     u32 version      kIcntCapVersion
//     u32 rec_bytes    sizeof(IcntCapRec) = 24
//     u32 nodes        nodes of the capturing network (-network_mode 1: the
//                      topology's; local crossbar: n_clusters + n_subpart)
//     u32 n_clusters   cluster c is node c
//     u32 n_subpart    L2 sub-partition s is node n_clusters + s
//     u32 flit_size    bytes per flit of the capturing network
//     u64 per_icnt     interconnect clock period, femtoseconds
//     u64 count[2]     records of the request subnet, of the reply subnet
//     u64 reserved     0
//   IcntCapRec[count[0]]   the request subnet
//   IcntCapRec[count[1]]   the reply subnet
//
// Per subnet the records are ordered by epoch, then mailbox cell, then slot:
// the order in which rt_epoch_run and icnt_contend gather.  `tinj` is the
// injection time in interconnect cycles, read before a contention pass adds
// its delay to Pkt::t.
#pragma once
#include "icnt_router.h"

namespace asim {

constexpr uint64_t kIcntCapMagic = 0x50414349'4d495341ull;  // "ASIMICAP"
constexpr uint32_t kIcntCapVersion = 1;

struct IcntCapHeader {
  uint64_t magic;
  uint32_t version, rec_bytes;
  uint32_t nodes, n_clusters, n_subpart, flit_size;
  uint64_t per_icnt;
  uint64_t count[2];
  uint64_t reserved;
};
static_assert(sizeof(IcntCapHeader) == 64, "capture header is 64 bytes");

struct IcntCapRec {
  uint64_t tinj;   // injection time, interconnect cycles
  uint32_t src, dst;  // nodes
  uint16_t bytes;  // Pkt::size
  uint16_t flits;  // rt_flits(c, bytes) on the capturing network
  uint8_t type;    // PktType
  uint8_t subnet;  // 0 request, 1 reply
  uint16_t pad;
};
static_assert(sizeof(IcntCapRec) == 24, "capture record is 24 bytes");

// one subnet's log: `n` records so far of `cap`; `off` is the gather's scan
// scratch, one word per mailbox cell.  Each subnet has a log of its own, so
// two blocks appending one subnet each never share a counter.
struct IcntCapLog {
  IcntCapRec* rec;
  uint32_t* off;
  uint32_t n, cap;
};

// the GPU engine's capture block in HBM: the logs, and the mailboxes by
// [direction][parity] with their capacities (what the append reads).  A
// launch that ended only because the logs were full is continued by the next
// one: `carry` tells it to start from the destination masks the last epoch
// decision left in `mask` (request 0..1, reply 2..3) instead of a launch's
// usual "every destination", so that the engine does, gather for gather, what
// the one longer launch without capture does, and the state images agree.
struct IcntCapDev {
  IcntCapLog log[2];
  const Pkt* box[2][2];
  const uint32_t* cnt[2][2];
  uint32_t cap[2];
  uint32_t carry;
  uint32_t stop;      // the kernel: the launch ended for a reason of its own (a trace refill), not at its epoch count
  uint32_t cfg_slot;  // the engine's configuration slot
  uint32_t both;      // block 0 appends both subnets (else block 1 the reply subnet)
  uint64_t mask[4];
};

// records one epoch can add to a subnet's log at most
SIM_HDI uint64_t icnt_cap_epoch_max(const SimCfg& c, uint32_t cap) { return (uint64_t)c.n_sm * c.n_subpart * cap; }

SIM_HDI uint32_t icnt_cap_nodes(const SimCfg& c) {
  return c.icnt_mode == 1 ? (uint32_t)icnt_node_count(c) : c.n_clusters + c.n_subpart;
}

// Append the packets of one subnet's mailboxes (direction dir: 0 request,
// 1 reply) to its log, in cell then slot order: the gather of
// rt_epoch_run_par (a scan over the cells' counts, then each cell fills its
// own range).  The caller guarantees room for icnt_cap_epoch_max records.
template <class P>
SIM_HDN void icnt_capture_append(const SimCfg& c, uint32_t dir, const Pkt* box, const uint32_t* cnt, uint32_t cap,
                                 IcntCapLog* log) {
  const uint32_t ncell = c.n_sm * c.n_subpart;
  auto cell_n = [&](int cell) -> uint32_t { return cnt[cell] < cap ? cnt[cell] : cap; };
  uint32_t* off = log->off;
  const uint32_t np = P::scan((int)ncell, cell_n, [&](int cell, uint32_t x) { off[cell] = x; });
  if (!np) return;
  P::sync();
  const uint32_t n0 = P::uni(log->n);
  IcntCapRec* out = log->rec + n0;
  P::each((int)ncell, [&](int ci) {
    const uint32_t cell = (uint32_t)ci, n = cell_n(ci);
    if (!n) return;
    const RtCell ce = rt_cell(c, dir, cell);
    const uint64_t lat = icnt_pkt_lat_fs(c, ce.sm, ce.sub);
    const uint32_t o = off[cell];
    for (uint32_t j = 0; j < n; ++j) {
      const Pkt& p = box[(uint64_t)cell * cap + j];
      IcntCapRec r;
      r.tinj = fdiv(p.t > lat ? p.t - lat : 0, c.dv_icnt);
      r.src = ce.a;
      r.dst = ce.b;
      r.bytes = p.size;
      r.flits = (uint16_t)rt_flits(c, p.size);
      r.type = p.type;
      r.subnet = (uint8_t)dir;
      r.pad = 0;
      out[o + j] = r;
    }
  });
  P::sync();
  P::one([&] { log->n = n0 + np; });
  P::sync();
}

}  // namespace asim
