// Open-loop synthetic traffic, packet-list replay, request-reply traffic and
// closed-loop request-reply traffic through the router model (icnt_bench.cc).
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../model/config.h"
#include "../model/icnt_router.h"

namespace asim {

struct OpenLoopParams {
  std::string traffic = "uniform";  // uniform, transpose, bitcomp, bitrev, shuffle, tornado, neighbor
  double rate = 0.1;                // offered flits per node per cycle
  uint32_t packet_flits = 1;
  uint64_t cycles = 2000, warmup = 500;
  uint64_t seed = 1;
};

struct OpenLoopResult {
  uint32_t nodes = 0;
  uint64_t packets = 0, measured_packets = 0;
  double offered = 0, accepted = 0;         // flits per node per cycle over the measurement window
  double drain_throughput = 0;              // all flits / node / cycle from the first injection to the last ejection
  double avg_latency = 0, max_latency = 0;  // creation to tail ejection, cycles
  double zero_load_latency = 0;             // the same packets' uncontended traversal
  uint32_t deadlocked = 0;
  // router activity (icnt_router.h RtAct order) and the energy of the run by
  // component (Booksim's power module role; per-event energies from the
  // .icnt file's power_* keys), pJ, and the average network power, W
  uint64_t activity[8] = {};
  double e_buffer = 0, e_xbar = 0, e_link = 0, e_alloc = 0, e_leak = 0, power_w = 0;
  // on request (icnt_open_loop_batch): every packet's arrival and the final state words of the pass
  std::vector<uint64_t> arrivals, state;
};

// icnt_text: a Booksim .icnt file's text (topology, router pipeline and
// microarchitecture keys)
OpenLoopResult icnt_open_loop(const std::string& icnt_text, const OpenLoopParams& p);

// ---- the three steps of a run: prepare, simulate, summarise ----

// the network of an .icnt file: the router configuration and, for anynet, the
// explicit route and latency tables (empty otherwise)
struct OpenLoopNet {
  SimCfg c{};
  std::map<std::string, std::string> kv;
  bool anynet = false;
  uint32_t N = 0;           // nodes
  uint32_t an_L = 0, an_H = 1;  // anynet: links and longest route
  std::vector<uint32_t> rt_off, rt_links;
  std::vector<uint16_t> lat, inj_lat;
};

// one point's injection schedule and pass dimensions
struct OpenLoopPoint {
  OpenLoopParams prm;
  uint32_t pf = 1, np = 0;
  RtDims d{};
  std::vector<uint32_t> src, dst;
  std::vector<uint64_t> tinj;
  std::vector<uint32_t> nfl;  // per-packet flits (replay, request-reply); empty: pf for every packet
  uint32_t flits(uint32_t i) const { return nfl.empty() ? pf : nfl[i]; }
};

// what a router pass leaves
struct OpenLoopRaw {
  std::vector<uint64_t> tarr, state;
  uint64_t act[RT_ACT_COUNT] = {};
  uint32_t deadlocked = 0;
  uint32_t status = 0;  // icnt_router_par.h RtStatus
};

OpenLoopNet icnt_open_loop_net(const std::string& icnt_text);
OpenLoopPoint icnt_open_loop_prepare(const OpenLoopNet& net, const OpenLoopParams& p);
OpenLoopResult icnt_open_loop_summarise(const OpenLoopNet& net, const OpenLoopPoint& pt, const OpenLoopRaw& raw);

struct OpenLoopBatchOpts {
  bool arrivals = false;       // keep arrivals and state in every result
  uint64_t mem_budget_mb = 0;  // gpu: device memory of one chunk (0: from the free device memory)
  uint64_t step_cap = 0;       // tests only: the loop guard's cap (cpu-par and gpu; 0: rt_step_cap)
  bool lds = true;             // gpu: the per-(unit, VC) words in LDS when they fit (false: always HBM)
};

// how the last gpu batch of this process was packed
struct OpenLoopBatchStats {
  uint64_t chunks = 0, max_chunk_points = 0, max_chunk_bytes = 0, budget_bytes = 0;
  uint64_t lds_chunks = 0;  // launches with the per-(unit, VC) words in LDS
};
OpenLoopBatchStats icnt_open_loop_last_batch();

// every point of `points` through one engine: "cpu" (rt_simulate), "cpu-par"
// (rt_simulate_par<SeqPar>) or "gpu" (engine/icnt_sweep.hip, one wavefront
// per point).  One result per point, in order.  std::invalid_argument: a bad
// point or engine name, or a point larger than the memory budget;
// std::runtime_error: no usable device, or a pass cut off by its loop guard.
std::vector<OpenLoopResult> icnt_open_loop_batch(const std::string& icnt_text,
                                                 const std::vector<OpenLoopParams>& points,
                                                 const std::string& engine = "cpu",
                                                 const OpenLoopBatchOpts& opts = OpenLoopBatchOpts());

// ---- packet-list replay: one subnet, per-packet sizes ----

// a packet list the caller brings (for example one dumped from a cycle
// simulation): packet i goes from src[i] to dst[i] with flits[i] flits and is
// created at cycle tinj[i]; any order
struct ReplayList {
  std::vector<uint32_t> src, dst, flits;
  std::vector<uint64_t> tinj;
};
constexpr uint64_t kReplayMaxPackets = 50'000'000ull;

// every list through one engine, like icnt_open_loop_batch; the summary's
// window is [warmup, cycles), cycles 0: the list's last injection + 1.
// std::invalid_argument, naming the list and the packet: a node out of range,
// src == dst, flits 0 or above rt_flits(c, kRtMaxPktBytes), arrays of unequal
// length, more than kReplayMaxPackets packets.
std::vector<OpenLoopResult> icnt_replay_batch(const std::string& icnt_text, const std::vector<ReplayList>& lists,
                                              const std::string& engine = "cpu",
                                              const OpenLoopBatchOpts& opts = OpenLoopBatchOpts(),
                                              uint64_t cycles = 0, uint64_t warmup = 0);

// ---- one packet list over many networks ----

// a packet list in bytes (for example a subnet of an -icnt_capture file,
// model/icnt_capture.h): what a packet weighs in flits depends on the network
// that replays it.  nodes: the node count the list was made for (0: unknown)
struct ReplayBytesList {
  uint32_t nodes = 0;
  std::vector<uint32_t> src, dst, bytes;
  std::vector<uint64_t> tinj;
};

// the list through every network of icnt_texts, one result per network in
// order.  Network i replays it with
//   flits = min(rt_flits(c_i, bytes), rt_flits(c_i, kRtMaxPktBytes)).
// "cpu" is the defining form, a loop of single-network icnt_replay_batch
// calls; "cpu-par" the lane-parallel pass on the host; "gpu" one wavefront per
// network, as many networks per launch as the memory budget takes
// (engine/icnt_net_sweep.hip).  std::invalid_argument, naming the network: a
// node count other than the list's (when the list states one), or a packet
// that icnt_replay_batch would refuse.
std::vector<OpenLoopResult> icnt_replay_networks(const ReplayBytesList& list,
                                                 const std::vector<std::string>& icnt_texts,
                                                 const std::string& engine = "cpu",
                                                 const OpenLoopBatchOpts& opts = OpenLoopBatchOpts(),
                                                 uint64_t cycles = 0, uint64_t warmup = 0);

// the dynamic LDS (bytes) one gpu launch over these networks takes for the
// per-(unit, VC) words, the chunk's largest 5 * U * V words: they are in LDS
// when this fits kIcntSweepLdsBytes.  Host work only.
uint64_t icnt_replay_networks_lds_bytes(const std::vector<std::string>& icnt_texts);

// ---- request-reply points: two subnets ----

// Reads and writes travel on the request subnet; each one's delivery creates,
// `reply_delay` cycles later, a reply of the other size from the destination
// back to the source on the reply subnet (model/icnt_reqreply.h).  The two
// subnets are independent networks of the same .icnt file (the arrangement of
// the reference's gputrafficmanager.cpp); unlike Booksim's single-queue
// _IssuePacket, a pending reply does not hold back its node's requests.
struct RequestReplyParams {
  std::string traffic = "uniform";
  double rate = 0.1;  // flits per node per cycle over both subnets
  uint64_t cycles = 2000, warmup = 500;
  uint64_t seed = 1;
  double write_fraction = 0.5;
  uint32_t read_request_size = 1, read_reply_size = 1, write_request_size = 1, write_reply_size = 1;  // flits
  uint64_t reply_delay = 0;  // the destination's service time, cycles
  uint32_t mem_nodes = 0;    // M > 0: nodes 0 .. N-M-1 issue, to the uniformly drawn memory nodes N-M .. N-1
};

struct RequestReplyResult {
  OpenLoopResult request, reply;
  uint64_t reads = 0, writes = 0;
  // request creation to reply tail arrival, over the requests created at or after warmup
  double round_trip_latency = 0, max_round_trip_latency = 0;
  uint32_t deadlocked = 0;  // both subnets
  // on request (opts.arrivals): both schedules; request.arrivals / .state and reply.arrivals / .state hold the rest
  std::vector<uint32_t> request_src, request_dst, request_flits, reply_of, reply_src, reply_dst, reply_flits;
  std::vector<uint64_t> request_tinj, reply_tinj;
};

// the request subnet's schedule of every point (what the batch call simulates):
// kind[i] is 1 for a write; host work only
struct RequestReplySchedule {
  std::vector<uint32_t> src, dst, flits, kind;
  std::vector<uint64_t> tinj;
};
std::vector<RequestReplySchedule> icnt_request_reply_schedule(const std::string& icnt_text,
                                                              const std::vector<RequestReplyParams>& points);

std::vector<RequestReplyResult> icnt_request_reply_batch(const std::string& icnt_text,
                                                         const std::vector<RequestReplyParams>& points,
                                                         const std::string& engine = "cpu",
                                                         const OpenLoopBatchOpts& opts = OpenLoopBatchOpts());

// ---- closed-loop request-reply points: bounded windows (model/icnt_closed.h) ----

// A node keeps at most `max_outstanding` requests in flight and issues the
// next one when a reply has come back (Booksim's batchtrafficmanager.cpp:
// sim_type = batch, batch_size, max_outstanding_requests).  Both subnets
// advance on one clock: one router pass over the doubled network, two
// disjoint copies of the .icnt file's network.  Differences from Booksim: a
// node may issue several requests in one cycle, and a pending reply leaves
// from the reply subnet's terminal instead of taking the node's injection
// slot.  Two kinds of point:
//   rate   (batch_size 0) the request list of a RequestReplyParams point with
//          the same fields; with max_outstanding 0 the point is that point
//   batch  every issuing node creates batch_size requests at cycle 0,
//          destinations from the pattern, kinds from write_fraction
// The memory endpoint (model/icnt_closed.h rule 2m): with read_occupancy,
// write_occupancy or write_reply_delay set, a memory node is one server that a
// read holds for read_occupancy cycles and a write for write_occupancy, with
// reply_delay (a write: write_reply_delay) cycles of pipelined latency behind
// it, and replies leave a node in the order their requests arrived.  With all
// three unset the reply is created reply_delay after the arrival, as before.
struct ClosedLoopParams {
  std::string traffic = "uniform";
  uint64_t seed = 1;
  double write_fraction = 0.5;
  uint32_t read_request_size = 1, read_reply_size = 1, write_request_size = 1, write_reply_size = 1;  // flits
  uint64_t reply_delay = 0;
  uint32_t mem_nodes = 0;
  uint32_t max_outstanding = 0;  // requests in flight per node, 0: unlimited
  double rate = 0.1;             // rate points
  uint64_t cycles = 2000, warmup = 500;
  uint32_t batch_size = 0;   // > 0: a batch point
  uint32_t batch_count = 1;  // only 1 is modelled
  uint32_t read_occupancy = 0, write_occupancy = 0;  // cycles a request holds its memory node
  int64_t write_reply_delay = -1;                    // a write's latency; < 0: reply_delay
};

// what the memory endpoint did to a point, over the measured requests (the
// model off: mem_time = reply_delay, the rest 0)
struct ClosedLoopMemStats {
  double mem_time = 0, max_mem_time = 0;  // reply creation - request arrival
  double mem_wait = 0;                    // service start - arrival: the queue in front of the server
  double mem_hold = 0;                    // creation - (service end + latency): the in-order return
  // a node's summed occupancy over the batch time (rate points: the measured
  // requests' over the measurement window), over the nodes that served a request
  double mem_utilisation = 0, max_mem_utilisation = 0;
  uint32_t mem_nodes_used = 0;
};

struct ClosedLoopResult {
  uint32_t nodes = 0, issuers = 0;  // of one subnet; the nodes that hold requests
  uint64_t requests = 0, measured = 0, reads = 0, writes = 0;
  uint64_t batch_time = 0;  // the last reply's arrival (batch points; 0 otherwise)
  // over the measured requests (rate points: created at or after warmup), from the issue time
  double request_latency = 0, reply_latency = 0, round_trip_latency = 0, max_round_trip_latency = 0;
  double issue_stall = 0, max_issue_stall = 0;  // issue - creation
  // flits per node and cycle ejected on each subnet: in [warmup, cycles) for a
  // rate point, over the batch time for a batch point
  double accepted_request = 0, accepted_reply = 0;
  double avg_outstanding = 0;  // requests in flight per issuing node, averaged over cycle 0 to the last reply
  uint64_t first_finish = 0, last_finish = 0;  // the earliest and latest issuing node's last reply
  uint32_t deadlocked = 0;
  uint64_t activity[8] = {};  // both subnets (RtAct order)
  double e_buffer = 0, e_xbar = 0, e_link = 0, e_alloc = 0, e_leak = 0, power_w = 0;
  // on request (opts.arrivals): the request list, every request's issue time,
  // both arrival arrays by request, the doubled network's state words
  std::vector<uint32_t> request_src, request_dst, request_flits, kind;
  std::vector<uint64_t> request_tinj, tiss, request_arrivals, reply_arrivals, state;
  ClosedLoopMemStats mem;
  std::vector<uint64_t> reply_created;  // on request: every reply's creation time
};

// every point through one engine: "cpu" (rt_simulate_closed), "cpu-par"
// (rt_simulate_par_closed<SeqPar>) or "gpu" (engine/icnt_cl_sweep.hip, one
// wavefront per point).  std::invalid_argument, naming the key: routing
// functions min_adapt and valiant (their routes are no tables), batch_count
// above 1, mem_nodes that leave no issuer, a network of more than
// kClosedLoopMaxNodes nodes; std::runtime_error: a pass cut off by its loop
// guard (opts.step_cap applies to every engine here).
constexpr uint32_t kClosedLoopMaxNodes = 1024;
std::vector<ClosedLoopResult> icnt_closed_loop_batch(const std::string& icnt_text,
                                                     const std::vector<ClosedLoopParams>& points,
                                                     const std::string& engine = "cpu",
                                                     const OpenLoopBatchOpts& opts = OpenLoopBatchOpts());

// ---- one request list, closed loop, over many networks and windows ----

// a request list in bytes (for example the requests of an -icnt_capture file
// with their replies' sizes, icnt/capture.py request_list): request i goes
// from src[i] to dst[i] with req_bytes[i] bytes, is created at tcreate[i]
// (non-decreasing, so a node's requests are in issue order) and is answered
// by a reply of reply_bytes[i] bytes.  nodes: the node count the list was made
// for (0: unknown).  occupancy / latency: optional, both or neither, the
// memory endpoint's per-request cycles for the memory point `list`
struct ClosedLoopList {
  uint32_t nodes = 0;
  std::vector<uint32_t> src, dst, req_bytes, reply_bytes;
  std::vector<uint64_t> tcreate;
  std::vector<uint32_t> occupancy, latency;
};

// a point of the memory axis: (occupancy, latency) for every request, or the
// list's own arrays
struct ClosedLoopMemPoint {
  bool list = false;
  uint32_t occupancy = 0, latency = 0;
};

// a (network, window) point: every request is measured (as for a batch point
// of icnt_closed_loop_batch) and batch_time is the last reply's arrival, the
// time the list's requests take on that network when a node may keep `window`
// of them in flight
struct ClosedLoopNetResult {
  uint32_t network = 0, window = 0;  // index into icnt_texts; 0: unlimited
  // the memory point: its index into mem_points (-1: the call had none), and the point
  int32_t mem_point = -1;
  bool mem_list = false;
  uint32_t mem_occupancy = 0, mem_latency = 0;
  uint32_t nodes = 0, issuers = 0;
  uint64_t requests = 0, measured = 0;
  uint64_t request_flits = 0, reply_flits = 0;  // the list's totals on this network
  uint64_t batch_time = 0;
  double request_latency = 0, reply_latency = 0, round_trip_latency = 0, max_round_trip_latency = 0;
  double issue_stall = 0, max_issue_stall = 0;
  double accepted_request = 0, accepted_reply = 0;
  double avg_outstanding = 0;
  uint64_t first_finish = 0, last_finish = 0;
  uint32_t deadlocked = 0;
  uint64_t activity[8] = {};
  double e_buffer = 0, e_xbar = 0, e_link = 0, e_alloc = 0, e_leak = 0, power_w = 0;
  // on request (opts.arrivals): every request's issue time, both arrival
  // arrays by request, this network's flit counts, the doubled network's state words
  std::vector<uint32_t> request_flit_counts, reply_flit_counts;
  std::vector<uint64_t> tiss, request_arrivals, reply_arrivals, state;
  ClosedLoopMemStats mem;
  std::vector<uint64_t> reply_created;  // on request: every reply's creation time
};

// the list through every network of icnt_texts under every window of
// `windows`, one closed-loop pass each (model/icnt_closed.h) on the network's
// doubled network; one result per (network, window), network-major.  With
// mem_points every (network, window) also runs under every memory point
// (model/icnt_closed.h rule 2m), network-major, then window, then memory
// point; without, reply_delay answers every request as before.  Network i
// carries both packets of a request with
//   flits = min(rt_flits(c_i, bytes), rt_flits(c_i, kRtMaxPktBytes))
// (model/icnt_closed.h rt_cl_fill_list).  "cpu" is the defining form, a loop
// of single passes (rt_simulate_closed); "cpu-par" the lane-parallel pass on
// the host; "gpu" one wavefront per (network, window), as many per launch as
// the memory budget takes (engine/icnt_cln_sweep.hip).  std::invalid_argument,
// naming the network: a node count other than list.nodes (when it states one),
// src == dst or a node out of range, a decreasing tcreate, arrays of unequal
// length (occupancy and latency included), an occupancy or latency above
// kRtClMemMax = 2^24, the memory point `list` without both arrays, more than
// kReplayMaxPackets / 2 requests, and what
// icnt_closed_loop_batch refuses of a network; std::runtime_error: a pass cut
// off by its loop guard (opts.step_cap applies to every engine).
std::vector<ClosedLoopNetResult> icnt_closed_loop_networks(const ClosedLoopList& list,
                                                           const std::vector<std::string>& icnt_texts,
                                                           const std::vector<uint32_t>& windows,
                                                           uint64_t reply_delay = 0, const std::string& engine = "cpu",
                                                           const OpenLoopBatchOpts& opts = OpenLoopBatchOpts(),
                                                           const std::vector<ClosedLoopMemPoint>& mem_points = {});

// the dynamic LDS (bytes) one gpu launch over these networks takes for the
// per-(unit, VC) words: the largest 5 * U * V words among their doubled
// networks; in LDS when this fits kIcntSweepLdsBytes.  Host work only.
uint64_t icnt_closed_loop_networks_lds_bytes(const std::vector<std::string>& icnt_texts);

}  // namespace asim
