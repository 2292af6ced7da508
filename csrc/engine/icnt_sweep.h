// Open-loop network sweeps on the GPU (icnt_sweep.hip): one 64-lane
// wavefront per sweep point runs the lane-parallel router pass
// (model/icnt_router_par.h) on that point's scratch in HBM.  The caller
// (driver/icnt_bench.cc icnt_open_loop_batch) packs the points into chunks
// under a memory budget; one chunk is one launch.  A second kernel
// (icnt_rr_sweep.hip) takes packet lists with per-packet sizes and
// request-reply points, both subnets of a point in one wavefront; a third
// (icnt_net_sweep.hip) one packet list over many networks; a fourth
// (icnt_cl_sweep.hip) closed-loop points on the doubled network; a fifth
// (icnt_cln_sweep.hip) one request list, closed loop, over many networks and
// windows.  What the launch paths share lives in two headers: icnt_sweep_layout.h (plain C++,
// every build) has a chunk's layout, the descriptors and the `*_bytes` the
// caller budgets with; icnt_sweep_dev.h (the .hip files only) has the
// pass with its LDS placement, the chunk's device block and the resource
// query.  Host-only builds link the stub in gpu_stub.cc.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../driver/icnt_bench.h"

namespace asim {

// bytes of one chunk: mem_budget_mb, or kIcntSweepFreeShare of the free
// device memory when it is 0
constexpr double kIcntSweepFreeShare = 0.5;  // the rest is left to the process's other engines
uint64_t icnt_sweep_budget_bytes(uint64_t mem_budget_mb);

// the per-(unit, VC) words of a pass, 5 * U * V of them, go to LDS when the
// largest of a chunk fits this much (the default dynamic LDS limit of a
// launch; an 8x8 mesh with 2 VCs takes 15 KB)
constexpr uint64_t kIcntSweepLdsBytes = 48 * 1024;
inline uint64_t icnt_hot_bytes(const RtDims& d) { return 5ull * d.U * d.V * 4; }

// one launch: grid = the chunk's points, 64 lanes each.  raws[i] is point
// i's arrivals, final state, activity, deadlocked packets and guard status.
// allow_lds false keeps the per-(unit, VC) words in HBM; returns whether
// they were in LDS.
bool icnt_sweep_run_chunk(const OpenLoopNet& net, const std::vector<OpenLoopPoint>& pts, uint64_t step_cap,
                          bool allow_lds, std::vector<OpenLoopRaw>& raws);

// registers, LDS and scratch of the kernel (code-object metadata through the
// HIP function attributes); empty without a device
std::map<std::string, uint64_t> icnt_sweep_kernel_info();

// ---- packet lists and request-reply points (icnt_rr_kernel) ----

// one unit of a launch: a packet list with per-packet sizes on the request
// subnet (req->nfl) and, with `reply`, its replies on the second subnet,
// built and ordered on the device (model/icnt_reqreply.h) between the passes
struct RrUnit {
  const OpenLoopPoint* req = nullptr;
  bool reply = false;
  RtDims d_rep{};                               // the reply pass's dimensions (np = req->np)
  const std::vector<uint32_t>* kind = nullptr;  // per request: 1 a write, 0 a read
  uint32_t fl_read = 1, fl_write = 1;           // reply flits by kind
  uint64_t delay = 0;                           // arrival to reply injection
};

// what a unit leaves: the request pass and, for a reply unit, the reply
// schedule and its pass
struct RrRaw {
  OpenLoopRaw req, rep;
  std::vector<uint32_t> reply_of, rep_src, rep_dst, rep_nfl;
  std::vector<uint64_t> rep_tinj;
};

// one launch: grid = the chunk's units, 64 lanes each, both subnets of a unit
// in the one workgroup.  Same LDS rule and return value as icnt_sweep_run_chunk.
bool icnt_rr_run_chunk(const OpenLoopNet& net, const std::vector<RrUnit>& units, uint64_t step_cap, bool allow_lds,
                       std::vector<RrRaw>& raws);

std::map<std::string, uint64_t> icnt_rr_kernel_info();

// ---- one packet list over many networks (icnt_net_kernel, icnt_net_sweep.hip) ----

// the list every unit of a chunk replays: uploaded once per chunk; a unit's
// flit counts come from `bytes` and its own network's flit size, on the device
struct NetList {
  const std::vector<uint32_t>*src = nullptr, *dst = nullptr, *bytes = nullptr;
  const std::vector<uint64_t>* tinj = nullptr;
};

// one unit of a launch: a network and the list as a point of it (pt->nfl: the
// flit counts the host derived, which the device must reproduce)
struct NetUnit {
  const OpenLoopNet* net = nullptr;
  const OpenLoopPoint* pt = nullptr;
};

// the dynamic LDS of a chunk's launch: the largest 5 * U * V words among its
// networks (every workgroup carves its own U * V out of it)
inline uint64_t icnt_net_hot_bytes(const std::vector<NetUnit>& units) {
  uint64_t b = 0;
  for (const NetUnit& u : units) b = std::max(b, icnt_hot_bytes(u.pt->d));
  return b;
}

// one launch: grid = the chunk's networks, 64 lanes each; every workgroup
// reads its own configuration, dimensions and tables from its descriptor.
// The dynamic LDS is sized for the largest 5 * U * V words of the chunk: in
// LDS if that fits kIcntSweepLdsBytes (and allow_lds), else in HBM for the
// whole chunk.  Returns whether they were in LDS.
bool icnt_net_run_chunk(const NetList& list, const std::vector<NetUnit>& units, uint64_t step_cap, bool allow_lds,
                        std::vector<OpenLoopRaw>& raws);

std::map<std::string, uint64_t> icnt_net_kernel_info();

// ---- closed-loop points (icnt_cl_kernel, icnt_cl_sweep.hip) ----

// one unit of a launch: a closed-loop point's 2 * nq packets on the doubled
// network (requests, then their replies: model/icnt_closed.h) with the
// requests' creation times
struct ClUnit {
  RtDims d{};  // the doubled network's pass
  uint32_t nq = 0, window = 0;
  uint64_t delay = 0;
  const std::vector<uint32_t>*src = nullptr, *dst = nullptr, *nfl = nullptr;  // 2 * nq each
  const std::vector<uint64_t>* tinj = nullptr;                               // nq
  // the memory endpoint (model/icnt_closed.h rule 2m): both null, rule 2's
  // `delay`; else every request's occupancy and latency, nq each
  const std::vector<uint32_t>*occ = nullptr, *lat = nullptr;
};

// the memory endpoint of a many-networks unit
enum ClMem : uint32_t { CL_MEM_OFF = 0, CL_MEM_ALL = 1, CL_MEM_LIST = 2 };

// what a unit leaves: the pass (tarr of the 2 * nq packets), the issue times
// and, with a memory endpoint, the replies' creation times
struct ClRaw {
  OpenLoopRaw pass;
  std::vector<uint64_t> tiss, created;
};

// one launch over the doubled network `net` (tables, `lat` / `inj_lat` empty
// for the uniform channel latency): grid = the chunk's units, 64 lanes each.
// Same LDS rule and return value as icnt_sweep_run_chunk.
bool icnt_cl_run_chunk(const OpenLoopNet& net, const std::vector<ClUnit>& units, uint64_t step_cap, bool allow_lds,
                       std::vector<ClRaw>& raws);

std::map<std::string, uint64_t> icnt_cl_kernel_info();

// ---- one request list, closed loop, over many networks and windows (icnt_cln_kernel, icnt_cln_sweep.hip) ----

// the request list every unit of a chunk runs: uploaded once per chunk; a
// unit's flit counts come from the bytes and its own network's flit size, on
// the device (model/icnt_closed.h rt_cl_fill_list)
struct ClList {
  const std::vector<uint32_t>*src = nullptr, *dst = nullptr, *req_bytes = nullptr, *reply_bytes = nullptr;
  const std::vector<uint64_t>* tcreate = nullptr;
  // optional, both or neither: per-request occupancy and latency of the
  // memory endpoint, for the units with mem == CL_MEM_LIST
  const std::vector<uint32_t>*occ = nullptr, *lat = nullptr;
};

// one unit of a launch: a (network, window, memory point).  dbl: the network's doubled
// network (tables; `lat` / `inj_lat` empty for the uniform channel latency),
// which the unit places for itself; nfl: the 2 * nq flit counts the host
// derived, which the device must reproduce
struct ClnUnit {
  const OpenLoopNet* dbl = nullptr;
  RtDims d{};  // the doubled network's pass
  uint32_t nq = 0, window = 0;
  uint64_t delay = 0;
  const std::vector<uint32_t>* nfl = nullptr;
  // CL_MEM_OFF: `delay`; CL_MEM_ALL: occ / lat for every request; CL_MEM_LIST: the list's arrays
  uint32_t mem = CL_MEM_OFF, occ = 0, lat = 0;
};

// the dynamic LDS of a chunk's launch: the largest 5 * U * V words among its
// units' doubled networks (every workgroup carves its own U * V out of it)
inline uint64_t icnt_cln_hot_bytes(const std::vector<ClnUnit>& units) {
  uint64_t b = 0;
  for (const ClnUnit& u : units) b = std::max(b, icnt_hot_bytes(u.d));
  return b;
}

// one launch: grid = the chunk's (network, window) units, 64 lanes each; every
// workgroup reads its own configuration, dimensions and tables from its
// descriptor and fills its packets from the shared list.  Same LDS rule and
// return value as icnt_net_run_chunk.
bool icnt_cln_run_chunk(const ClList& list, const std::vector<ClnUnit>& units, uint64_t step_cap, bool allow_lds,
                        std::vector<ClRaw>& raws);

std::map<std::string, uint64_t> icnt_cln_kernel_info();

}  // namespace asim
