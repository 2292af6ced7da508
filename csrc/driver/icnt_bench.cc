// Open-loop synthetic-traffic runs of the router model (Booksim's standalone
// mode: reference intersim2/main.cpp + trafficmanager.cpp + traffic.cpp +
// injection.cpp).  Every node injects Bernoulli packets at `rate` flits per
// cycle towards the traffic pattern's destination for `cycles` cycles; the
// packets are simulated to their arrival in one pass of the router model
// (model/icnt_router.h), which is exact here because the whole injection
// schedule is known up front.  Latency is creation to tail ejection (source
// queueing included), accepted throughput the flits ejected during the
// measurement window [warmup, cycles) per node and cycle.
//
// Two more kinds of run share the pass and the summary (second half of this
// file): packet lists the caller brings, every packet with its own flit count
// (icnt_replay_batch), and request-reply points over two subnets, where a
// request's arrival creates its reply at the destination (reference
// trafficmanager.cpp _IssuePacket / _GeneratePacket; icnt_request_reply_batch,
// model/icnt_reqreply.h).  The last part is the closed loop: request-reply
// points whose nodes keep a bounded number of requests in flight, both subnets
// on one clock in one pass over the doubled network (reference
// batchtrafficmanager.cpp; icnt_closed_loop_batch, model/icnt_closed.h), for
// synthetic points on one network and for a request list the caller brings on
// many networks and windows (icnt_closed_loop_networks).
#include "icnt_bench.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "../config/icnt_config.h"
#include "../engine/engine.h"
#include "../engine/icnt_sweep_layout.h"
#include "../model/icnt_router.h"
#include "../model/icnt_reqreply.h"
#include "../model/icnt_router_par.h"

namespace asim {

namespace {

// splitmix64: a small deterministic generator (same stream on every host)
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

uint32_t log2_exact(uint32_t n) {
  uint32_t b = 0;
  while ((1u << b) < n) ++b;
  if ((1u << b) != n) throw std::invalid_argument("bit-permutation traffic needs a power-of-two node count");
  return b;
}

// destination of node s under the pattern (Booksim traffic.cpp names)
uint32_t destination(const std::string& t, uint32_t s, uint32_t N, uint32_t k, uint32_t n, Rng& r) {
  if (t == "uniform") {
    for (;;) {
      const uint32_t d = (uint32_t)(r.next() % N);
      if (d != s || N == 1) return d;
    }
  }
  if (t == "bitcomp") return ~s & ((1u << log2_exact(N)) - 1);
  if (t == "transpose") {
    const uint32_t b = log2_exact(N);
    if (b % 2) throw std::invalid_argument("transpose traffic needs an even number of address bits");
    const uint32_t h = b / 2, m = (1u << h) - 1;
    return ((s & m) << h) | (s >> h);
  }
  if (t == "bitrev") {
    const uint32_t b = log2_exact(N);
    uint32_t d = 0;
    for (uint32_t i = 0; i < b; ++i) d |= ((s >> i) & 1u) << (b - 1 - i);
    return d;
  }
  if (t == "shuffle") {
    const uint32_t b = log2_exact(N);
    return ((s << 1) | (s >> (b - 1))) & (N - 1);
  }
  if (t == "tornado" || t == "neighbor") {
    // per dimension of a k-ary n-cube: half way round (tornado) or the next router
    uint32_t d = 0, pw = 1, x = s;
    for (uint32_t i = 0; i < n; ++i, pw *= k) {
      const uint32_t xi = x % k;
      const uint32_t yi = t == "tornado" ? (xi + (k + 1) / 2 - 1) % k : (xi + 1) % k;
      d += yi * pw;
      x /= k;
    }
    return d % N;
  }
  throw std::invalid_argument("unknown traffic pattern '" + t + "'");
}

// Booksim anynet network file (reference intersim2/networks/anynet.cpp
// grammar): lines "router R  router X [latency]  node n [latency] ...";
// router-router channels are bidirectional, the latency given for one
// direction (the other defaults to 1 cycle unless listed too); a node's
// latency serves its injection and ejection channels.  Links: ejection link
// n (node n's router -> node n) first, then the router-router channels.
// Routes: fewest (router delay + channel latency) by Dijkstra, ties to the
// lower router index.
struct AnyNet {
  uint32_t N = 0, R = 0, H = 1;
  std::vector<uint32_t> node_router, off, route;
  std::vector<uint16_t> lat, inj_lat;
};

AnyNet build_anynet(const std::string& text, uint32_t hop) {
  AnyNet a;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> rr;  // (from, to) router channel -> latency
  std::map<uint32_t, std::pair<uint32_t, uint32_t>> nodes;  // node -> (router, latency)
  std::istringstream in(text);
  std::string line;
  auto lat_of = [](std::vector<std::string>& t, size_t& i) -> uint32_t {
    if (i + 1 < t.size() && isdigit((unsigned char)t[i + 1][0])) return (uint32_t)std::stoul(t[++i]);
    return 1;
  };
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::vector<std::string> t;
    for (std::string x; ls >> x;) t.push_back(x);
    if (t.size() < 2 || t[0] != "router") continue;
    const uint32_t r = (uint32_t)std::stoul(t[1]);
    a.R = std::max(a.R, r + 1);
    for (size_t i = 2; i + 1 < t.size(); ++i) {
      const std::string kind = t[i];
      const uint32_t id = (uint32_t)std::stoul(t[++i]);
      const uint32_t l = lat_of(t, i);
      if (kind == "router") {
        rr[{r, id}] = l;
        a.R = std::max(a.R, id + 1);
      } else if (kind == "node") {
        nodes[id] = {r, l};
      } else {
        throw std::invalid_argument("anynet: expected 'router' or 'node', got '" + kind + "'");
      }
    }
  }
  for (auto& e : std::map<std::pair<uint32_t, uint32_t>, uint32_t>(rr))
    if (!rr.count({e.first.second, e.first.first})) rr[{e.first.second, e.first.first}] = 1;
  a.N = nodes.empty() ? 0 : nodes.rbegin()->first + 1;
  if (a.N == 0 || nodes.size() != a.N) throw std::invalid_argument("anynet: nodes must be numbered 0.. without gaps");
  a.node_router.resize(a.N);
  a.inj_lat.resize(a.N);
  a.lat.resize(a.N);
  for (auto& n : nodes) {
    a.node_router[n.first] = n.second.first;
    a.inj_lat[n.first] = a.lat[n.first] = (uint16_t)std::min<uint32_t>(n.second.second, 65535);
  }
  // router channels: link ids after the N ejection links
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> out(a.R);  // router -> (to, link)
  for (auto& e : rr) {
    out[e.first.first].push_back({e.first.second, (uint32_t)a.lat.size()});
    a.lat.push_back((uint16_t)std::min<uint32_t>(e.second, 65535));
  }
  // Dijkstra from every router (small networks: O(R^2) per source)
  std::vector<std::vector<uint32_t>> via(a.R, std::vector<uint32_t>(a.R, ~0u));  // [src][dst] -> link into dst
  for (uint32_t s0 = 0; s0 < a.R; ++s0) {
    std::vector<uint64_t> dist(a.R, ~0ull);
    std::vector<char> done(a.R, 0);
    dist[s0] = 0;
    for (uint32_t it = 0; it < a.R; ++it) {
      uint32_t u = ~0u;
      for (uint32_t x = 0; x < a.R; ++x)
        if (!done[x] && dist[x] != ~0ull && (u == ~0u || dist[x] < dist[u])) u = x;
      if (u == ~0u) break;
      done[u] = 1;
      for (auto& e : out[u]) {
        const uint64_t nd = dist[u] + hop + a.lat[e.second];
        if (nd < dist[e.first]) {
          dist[e.first] = nd;
          via[s0][e.first] = e.second;
        }
      }
    }
  }
  std::vector<uint32_t> from(a.lat.size(), 0);
  for (uint32_t r = 0; r < a.R; ++r)
    for (auto& e : out[r]) from[e.second] = r;
  a.off.assign((size_t)a.N * a.N + 1, 0);
  for (uint32_t x = 0; x < a.N; ++x)
    for (uint32_t y = 0; y < a.N; ++y) {
      const uint32_t rs = a.node_router[x], rd = a.node_router[y];
      std::vector<uint32_t> path;
      for (uint32_t r = rd; r != rs;) {
        const uint32_t l = via[rs][r];
        if (l == ~0u) throw std::invalid_argument("anynet: router " + std::to_string(rd) + " unreachable");
        path.push_back(l);
        r = from[l];
      }
      std::reverse(path.begin(), path.end());
      path.push_back(y);  // the ejection link into node y
      a.route.insert(a.route.end(), path.begin(), path.end());
      a.off[(size_t)x * a.N + y + 1] = (uint32_t)a.route.size();
      a.H = std::max<uint32_t>(a.H, (uint32_t)path.size());
    }
  return a;
}

// the pass's work arrays over `scratch`, with the point's packets in them
RtWork load_point(const OpenLoopNet& net, const OpenLoopPoint& pt, std::vector<uint32_t>& scratch) {
  scratch.assign(rt_carve(pt.d, nullptr, nullptr), 0);
  RtWork w;
  rt_carve(pt.d, scratch.data(), &w);
  if (net.anynet) {
    w.rt_off = net.rt_off.data();
    w.rt_links = net.rt_links.data();
    w.lat = net.lat.data();
    w.inj_lat = net.inj_lat.data();
  }
  for (uint32_t i = 0; i < pt.np; ++i) {
    w.src[i] = pt.src[i];
    w.dst[i] = pt.dst[i];
    w.nfl[i] = pt.flits(i);
    w.tinj[i] = pt.tinj[i];
  }
  return w;
}

// the router pass of one point on the host: rt_simulate, or the lane-parallel
// pass under the sequential lane policy
OpenLoopRaw simulate_host(const OpenLoopNet& net, const OpenLoopPoint& pt, bool par, uint64_t step_cap) {
  OpenLoopRaw raw;
  raw.state.assign(rt_state_words(pt.d), 0);
  std::vector<uint32_t> scratch;
  const RtWork w = load_point(net, pt, scratch);
  if (pt.np) {
    raw.deadlocked = par ? rt_simulate_par<SeqPar>(net.c, pt.d, raw.state.data(), w, pt.np, raw.act, &raw.status, step_cap)
                         : rt_simulate(net.c, pt.d, raw.state.data(), w, pt.np, raw.act);
  }
  raw.tarr.assign(w.tarr, w.tarr + pt.np);
  return raw;
}

// network energy of a pass from its activity (Booksim power_module.cpp's
// terms: input buffers, crossbar, channels, allocators, buffer leakage), pJ,
// and the average power over the cycles to `last`; the per-event energies are
// .icnt keys with ~22 nm Orion-class defaults
struct NetEnergy {
  double buffer, xbar, link, alloc, leak, power_w;
};
NetEnergy net_energy(const OpenLoopNet& net, const RtDims& d, const uint64_t* act, uint64_t last) {
  auto num = [&](const char* k, double dflt) {
    auto it = net.kv.find(k);
    return it == net.kv.end() ? dflt : strtod(it->second.c_str(), nullptr);
  };
  NetEnergy r;
  const double bits = 8.0 * net.c.flit_size;
  r.buffer = num("power_buffer_pj_per_bit", 0.08) * bits * (double)(act[RT_ACT_BUF_WRITE] + act[RT_ACT_BUF_READ]);
  r.xbar = num("power_xbar_pj_per_bit", 0.06) * bits * (double)act[RT_ACT_BUF_READ];
  r.link = num("power_link_pj_per_bit_mm", 0.15) * num("power_link_mm", 1.0) * bits *
           (double)(act[RT_ACT_LINK] + act[RT_ACT_EJECT]);
  r.alloc = num("power_alloc_pj_per_request", 0.5) * (double)act[RT_ACT_SA_REQ];
  const double ghz = num("power_clock_ghz", 1.0), t_ns = (double)(last + 1) / ghz;
  // leakage: uW per buffered flit slot of every input VC
  r.leak = num("power_buffer_leak_uw_per_flit", 0.5) * 1e-6 * (double)d.U * d.V * d.B * t_ns * 1e3;
  const double e = r.buffer + r.xbar + r.link + r.alloc + r.leak;
  r.power_w = t_ns > 0 ? e * 1e-12 / (t_ns * 1e-9) : 0;
  return r;
}

OpenLoopBatchStats g_last;  // of the last batch call (one caller at a time)

void check_status(const OpenLoopRaw& raw, size_t index, const char* who = "icnt_open_loop_batch: point ") {
  if (raw.status != RT_STATUS_OK)
    throw std::runtime_error(who + std::to_string(index) + ": the router pass exceeded its step cap (loop guard)");
}

void check_engine(const std::string& who, const std::string& engine) {
  if (engine != "cpu" && engine != "cpu-par" && engine != "gpu")
    throw std::invalid_argument(who + ": engine must be cpu, cpu-par or gpu, not '" + engine + "'");
  if (engine == "gpu" && !gpu_engine_available())
    throw std::runtime_error(who + ": engine 'gpu' needs a HIP device, and none is usable");
}

// the dimensions of a pass of np packets of at most max_flits flits
RtDims list_dims(const OpenLoopNet& net, uint32_t np, uint32_t max_flits) {
  RtDims d = rt_dims(net.c, np ? np : 1, max_flits ? max_flits : 1);
  if (net.anynet) {
    d.N = net.N;
    d.L = net.an_L;
    d.U = d.N + d.L;
    d.H = net.an_H;
  }
  return d;
}

// a pass's result: its guard status checked (`who` and the index name it),
// its summary and, on request, its arrivals and state
OpenLoopResult finish(const char* who, size_t index, const OpenLoopNet& net, const OpenLoopPoint& pt, OpenLoopRaw& raw,
                      bool arrivals) {
  check_status(raw, index, who);
  OpenLoopResult r = icnt_open_loop_summarise(net, pt, raw);
  if (arrivals) {
    r.arrivals = std::move(raw.tarr);
    r.state = std::move(raw.state);
  }
  return r;
}

// gpu: n items are prepared one after the other and packed into chunks under
// the memory budget; a full chunk is one launch, then finished and dropped.
// `fixed`: the device bytes of a chunk besides its items.  prep(i): item i;
// bytes(item): what it adds to a chunk; run(chunk, raws): the launch, true
// with the per-(unit, VC) words in LDS; done(item, raw): its result.
// std::invalid_argument, "<subject> <i> needs ...": an item that no chunk holds.
template <class Item, class Raw, class Prep, class Bytes, class Run, class Done>
void pack_chunks(const std::string& subject, const OpenLoopBatchOpts& opts, uint64_t fixed, size_t n, Prep prep,
                 Bytes bytes, Run run, Done done) {
  const uint64_t budget = icnt_sweep_budget_bytes(opts.mem_budget_mb);
  g_last = OpenLoopBatchStats();
  g_last.budget_bytes = budget;
  std::vector<Item> chunk;
  uint64_t used = fixed;
  auto flush = [&] {
    if (chunk.empty()) return;
    std::vector<Raw> raws;
    if (run(chunk, raws)) ++g_last.lds_chunks;
    ++g_last.chunks;
    g_last.max_chunk_points = std::max<uint64_t>(g_last.max_chunk_points, chunk.size());
    g_last.max_chunk_bytes = std::max(g_last.max_chunk_bytes, used);
    for (size_t i = 0; i < chunk.size(); ++i) done(chunk[i], raws[i]);
    chunk.clear();
    used = fixed;
  };
  for (size_t i = 0; i < n; ++i) {
    Item it = prep(i);
    const uint64_t need = bytes(it);
    if (fixed + need > budget)
      throw std::invalid_argument(subject + " " + std::to_string(i) + " needs " +
                                  std::to_string((fixed + need + (1u << 20) - 1) >> 20) + " MB, the memory budget is " +
                                  std::to_string(budget >> 20) + " MB");
    if (used + need > budget) flush();
    used += need;
    chunk.push_back(std::move(it));
  }
  flush();
}

}  // namespace

OpenLoopNet icnt_open_loop_net(const std::string& icnt_text) {
  OpenLoopNet net;
  SimCfg& c = net.c;
  c.flit_size = 32;
  net.kv = parse_booksim_config(icnt_text);
  const auto& kv = net.kv;
  net.anynet = kv.count("topology") && kv.at("topology") == "anynet";
  uint64_t nodes = 0;
  if (net.anynet) {
    // the router microarchitecture and pipeline from the file, the network
    // from its network_file
    auto k2 = kv;
    k2["topology"] = "fly";
    k2["k"] = "2";
    k2["n"] = "1";
    apply_topology(c, k2);
    if (!kv.count("network_file")) throw std::invalid_argument("anynet needs network_file");
    std::ifstream f(kv.at("network_file"));
    if (!f.good()) throw std::invalid_argument("cannot open anynet network_file '" + kv.at("network_file") + "'");
    std::stringstream ss;
    ss << f.rdbuf();
    AnyNet an = build_anynet(ss.str(), c.hop_icnt);
    nodes = an.N;
    net.an_L = (uint32_t)an.lat.size();
    net.an_H = an.H;
    net.rt_off = std::move(an.off);
    net.rt_links = std::move(an.route);
    net.lat = std::move(an.lat);
    net.inj_lat = std::move(an.inj_lat);
  } else {
    nodes = apply_topology(c, kv);
  }
  if (c.rt_alloc == 0xff) throw std::invalid_argument("sw_allocator not modelled");
  c.link_contention = 2;
  if (nodes > (1u << 20)) throw std::invalid_argument("topology too large");
  net.N = (uint32_t)nodes;
  return net;
}

OpenLoopPoint icnt_open_loop_prepare(const OpenLoopNet& net, const OpenLoopParams& prm) {
  const SimCfg& c = net.c;
  const uint32_t N = net.N;
  const bool anynet = net.anynet;
  OpenLoopPoint pt;
  pt.prm = prm;
  const uint32_t pf = prm.packet_flits ? prm.packet_flits : 1;
  pt.pf = pf;
  if (prm.rate < 0 || prm.rate > 1) throw std::invalid_argument("rate must be 0..1 flits per node per cycle");
  if (prm.warmup >= prm.cycles) throw std::invalid_argument("warmup must be shorter than the run");
  // the injection schedule
  Rng r{prm.seed * 0x2545f4914f6cdd1dull + 1};
  std::vector<uint32_t>&src = pt.src, &dst = pt.dst;
  std::vector<uint64_t>& tinj = pt.tinj;
  const double p_pkt = prm.rate / pf;
  for (uint64_t t = 0; t < prm.cycles; ++t)
    for (uint32_t s = 0; s < N; ++s)
      if (r.uniform() < p_pkt) {
        const uint32_t d = destination(prm.traffic, s, N, anynet ? N : c.topo_k, anynet ? 1u : c.topo_n, r);
        if (d == s) continue;  // a fixed point of a permutation sends nothing
        src.push_back(s);
        dst.push_back(d);
        tinj.push_back(t);
      }
  const uint64_t np64 = src.size();
  if (np64 > 50'000'000ull) throw std::invalid_argument("too many packets for one pass");
  const uint32_t np = (uint32_t)np64;
  pt.np = np;
  pt.d = list_dims(net, np, pf);
  return pt;
}

OpenLoopResult icnt_open_loop_summarise(const OpenLoopNet& net, const OpenLoopPoint& pt, const OpenLoopRaw& raw) {
  const SimCfg& c = net.c;
  const auto& kv = net.kv;
  const OpenLoopParams& prm = pt.prm;
  const bool anynet = net.anynet;
  const uint32_t N = net.N, np = pt.np;
  const RtDims& d = pt.d;
  const std::vector<uint32_t>&src = pt.src, &dst = pt.dst;
  const std::vector<uint64_t>& tinj = pt.tinj;
  const uint64_t* act = raw.act;
  OpenLoopResult res;
  res.nodes = N;
  res.packets = np;
  res.deadlocked = raw.deadlocked;
  for (int i = 0; i < RT_ACT_COUNT; ++i) res.activity[i] = act[i];
  double lat = 0, zero = 0;
  uint64_t meas = 0, meas_flits = 0, total = 0, ejected = 0, last = 0;  // (flit sums: exact in a double)
  for (uint32_t i = 0; i < np; ++i) {
    const uint64_t a = raw.tarr[i];
    last = std::max(last, a);
    const uint32_t pf = pt.flits(i);
    total += pf;
    if (a >= prm.warmup && a < prm.cycles) ejected += pf;
    if (tinj[i] >= prm.warmup) {
      lat += (double)(a - tinj[i]);
      if (anynet) {
        // injection channel + per router its delay and its output channel
        uint64_t z = net.inj_lat[src[i]] + (pf - 1);
        const size_t pr = (size_t)src[i] * N + dst[i];
        for (uint32_t k = net.rt_off[pr]; k < net.rt_off[pr + 1]; ++k) z += c.hop_icnt + net.lat[net.rt_links[k]];
        zero += (double)z;
      } else {
        zero += (double)rt_uncontended(c, icnt_routers(c, src[i], dst[i]), pf);
      }
      ++meas;
      meas_flits += pf;
      res.max_latency = std::max<double>(res.max_latency, (double)(a - tinj[i]));
    }
  }
  const double window = (double)(prm.cycles - prm.warmup) * N;
  res.offered = (double)meas_flits / window;
  res.accepted = (double)ejected / window;
  res.avg_latency = meas ? lat / meas : 0;
  res.zero_load_latency = meas ? zero / meas : 0;
  res.measured_packets = meas;
  // above saturation the window sees the network before its queues settle;
  // the drain rate is the bottleneck's (open loop, every packet delivered)
  res.drain_throughput = np && last ? (double)total / ((double)N * (double)(last + 1)) : 0;
  const NetEnergy e = net_energy(net, d, act, last);
  res.e_buffer = e.buffer;
  res.e_xbar = e.xbar;
  res.e_link = e.link;
  res.e_alloc = e.alloc;
  res.e_leak = e.leak;
  res.power_w = e.power_w;
  return res;
}

OpenLoopBatchStats icnt_open_loop_last_batch() { return g_last; }

OpenLoopResult icnt_open_loop(const std::string& icnt_text, const OpenLoopParams& prm) {
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  const OpenLoopPoint pt = icnt_open_loop_prepare(net, prm);
  return icnt_open_loop_summarise(net, pt, simulate_host(net, pt, false, 0));
}

std::vector<OpenLoopResult> icnt_open_loop_batch(const std::string& icnt_text,
                                                 const std::vector<OpenLoopParams>& points,
                                                 const std::string& engine, const OpenLoopBatchOpts& opts) {
  check_engine("icnt_open_loop_batch", engine);
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  std::vector<OpenLoopResult> out;
  out.reserve(points.size());
  const char* who = "icnt_open_loop_batch: point ";
  g_last = OpenLoopBatchStats();
  if (engine != "gpu") {
    for (const OpenLoopParams& p : points) {
      const OpenLoopPoint pt = icnt_open_loop_prepare(net, p);
      OpenLoopRaw raw = simulate_host(net, pt, engine == "cpu-par", opts.step_cap);
      out.push_back(finish(who, out.size(), net, pt, raw, opts.arrivals));
    }
    return out;
  }
  pack_chunks<OpenLoopPoint, OpenLoopRaw>(
      "icnt_open_loop_batch: point", opts, icnt_sweep_net_bytes(net), points.size(),
      [&](size_t i) { return icnt_open_loop_prepare(net, points[i]); }, icnt_sweep_point_bytes,
      [&](const std::vector<OpenLoopPoint>& chunk, std::vector<OpenLoopRaw>& raws) {
        return icnt_sweep_run_chunk(net, chunk, opts.step_cap, opts.lds, raws);
      },
      [&](OpenLoopPoint& pt, OpenLoopRaw& raw) { out.push_back(finish(who, out.size(), net, pt, raw, opts.arrivals)); });
  return out;
}

// ---- packet-list replay and request-reply points ----

namespace {

// pack_chunks for the items of icnt_rr_run_chunk; unit(item): its RrUnit
template <class Item, class Prep, class Unit, class Done>
void rr_gpu_batch(const std::string& subject, const OpenLoopNet& net, size_t n, const OpenLoopBatchOpts& opts,
                  Prep prep, Unit unit, Done done) {
  pack_chunks<Item, RrRaw>(
      subject, opts, icnt_sweep_net_bytes(net), n, prep, [&](const Item& it) { return icnt_rr_unit_bytes(unit(it)); },
      [&](const std::vector<Item>& chunk, std::vector<RrRaw>& raws) {
        std::vector<RrUnit> units;
        for (const Item& it : chunk) units.push_back(unit(it));
        return icnt_rr_run_chunk(net, units, opts.step_cap, opts.lds, raws);
      },
      done);
}

// a checked packet list as a point of the pass; `index` names it in errors
OpenLoopPoint replay_prepare(const OpenLoopNet& net, const ReplayList& l, size_t index, uint64_t cycles,
                             uint64_t warmup) {
  const std::string who = "icnt_replay_batch: list " + std::to_string(index);
  const size_t n = l.src.size();
  if (l.dst.size() != n || l.flits.size() != n || l.tinj.size() != n)
    throw std::invalid_argument(who + ": src, dst, flits and tinj differ in length");
  if (n > kReplayMaxPackets) throw std::invalid_argument(who + ": too many packets for one pass");
  const uint32_t max_fl = rt_flits(net.c, kRtMaxPktBytes);
  uint32_t top = 1;
  uint64_t last = 0;
  for (size_t i = 0; i < n; ++i) {
    const std::string pk = who + ", packet " + std::to_string(i);
    if (l.src[i] >= net.N || l.dst[i] >= net.N)
      throw std::invalid_argument(pk + ": node out of range (the network has " + std::to_string(net.N) + ")");
    if (l.src[i] == l.dst[i]) throw std::invalid_argument(pk + ": source and destination are the same node");
    if (!l.flits[i] || l.flits[i] > max_fl)
      throw std::invalid_argument(pk + ": flits must be 1.." + std::to_string(max_fl));
    top = std::max(top, l.flits[i]);
    last = std::max(last, l.tinj[i]);
  }
  OpenLoopPoint pt;
  pt.prm.traffic = "replay";
  pt.prm.rate = 0;
  pt.prm.cycles = cycles ? cycles : last + 1;
  pt.prm.warmup = warmup;
  if (pt.prm.warmup >= pt.prm.cycles) throw std::invalid_argument(who + ": warmup must be shorter than the run");
  pt.np = (uint32_t)n;
  pt.src = l.src;
  pt.dst = l.dst;
  pt.nfl = l.flits;
  pt.tinj = l.tinj;
  pt.d = list_dims(net, pt.np, top);  // nf = np * the largest packet
  return pt;
}

// a request-reply point: the request schedule with its kinds, and the reply
// subnet's dimensions
struct RrPoint {
  RequestReplyParams prm;
  OpenLoopPoint req;
  std::vector<uint32_t> kind;  // per request: 1 a write
  RtDims d_rep{};
  uint64_t reads = 0, writes = 0;
};

RrPoint rr_prepare(const OpenLoopNet& net, const RequestReplyParams& prm, size_t index,
                   const char* fn = "icnt_request_reply_batch") {
  const std::string who = std::string(fn) + ": point " + std::to_string(index);
  const SimCfg& c = net.c;
  const uint32_t N = net.N, M = prm.mem_nodes;
  if (prm.rate < 0 || prm.rate > 1) throw std::invalid_argument(who + ": rate must be 0..1 flits per node per cycle");
  if (prm.warmup >= prm.cycles) throw std::invalid_argument(who + ": warmup must be shorter than the run");
  if (!(prm.write_fraction >= 0 && prm.write_fraction <= 1))
    throw std::invalid_argument(who + ": write_fraction must be 0..1");
  const uint32_t max_fl = rt_flits(c, kRtMaxPktBytes);
  for (uint32_t sz : {prm.read_request_size, prm.read_reply_size, prm.write_request_size, prm.write_reply_size})
    if (!sz || sz > max_fl) throw std::invalid_argument(who + ": packet sizes must be 1.." + std::to_string(max_fl) + " flits");
  if (M >= N) throw std::invalid_argument(who + ": mem_nodes must leave a node to issue");
  if (M && prm.traffic != "uniform") throw std::invalid_argument(who + ": mem_nodes needs uniform traffic");
  RrPoint pt;
  pt.prm = prm;
  OpenLoopPoint& q = pt.req;
  q.prm.traffic = prm.traffic;
  q.prm.rate = prm.rate;
  q.prm.cycles = prm.cycles;
  q.prm.warmup = prm.warmup;
  q.prm.seed = prm.seed;
  // the request schedule: the generator and loop of icnt_open_loop_prepare,
  // with the packet probability over the average packet of both subnets
  // (reference trafficmanager.cpp:197-200) and a kind draw per kept packet
  const uint32_t avg = std::max<uint32_t>(
      1, (prm.read_request_size + prm.read_reply_size + prm.write_request_size + prm.write_reply_size) / 2);
  const double p_pkt = prm.rate / avg;
  const uint32_t issuers = N - M;
  Rng r{prm.seed * 0x2545f4914f6cdd1dull + 1};
  for (uint64_t t = 0; t < prm.cycles; ++t)
    for (uint32_t s = 0; s < issuers; ++s)
      if (r.uniform() < p_pkt) {
        const uint32_t d = M ? N - M + (uint32_t)(r.next() % M)
                             : destination(prm.traffic, s, N, net.anynet ? N : c.topo_k, net.anynet ? 1u : c.topo_n, r);
        if (d == s) continue;  // a fixed point of a permutation sends nothing
        const uint32_t wr = r.uniform() < prm.write_fraction ? 1u : 0u;
        q.src.push_back(s);
        q.dst.push_back(d);
        q.tinj.push_back(t);
        q.nfl.push_back(wr ? prm.write_request_size : prm.read_request_size);
        pt.kind.push_back(wr);
        ++(wr ? pt.writes : pt.reads);
      }
  if (q.src.size() > kReplayMaxPackets) throw std::invalid_argument(who + ": too many packets for one pass");
  q.np = (uint32_t)q.src.size();
  q.d = list_dims(net, q.np, std::max(prm.read_request_size, prm.write_request_size));
  pt.d_rep = list_dims(net, q.np, std::max(prm.read_reply_size, prm.write_reply_size));
  return pt;
}

RrUnit rr_unit(const RrPoint& pt) {
  RrUnit u;
  u.req = &pt.req;
  u.reply = true;
  u.d_rep = pt.d_rep;
  u.kind = &pt.kind;
  u.fl_read = pt.prm.read_reply_size;
  u.fl_write = pt.prm.write_reply_size;
  u.delay = pt.prm.reply_delay;
  return u;
}

// the reply subnet's point from the schedule in `raw`
OpenLoopPoint rr_reply_point(const RrPoint& pt, const RrRaw& raw) {
  OpenLoopPoint p;
  p.prm = pt.req.prm;
  p.np = pt.req.np;
  p.d = pt.d_rep;
  p.src = raw.rep_src;
  p.dst = raw.rep_dst;
  p.nfl = raw.rep_nfl;
  p.tinj = raw.rep_tinj;
  return p;
}

// both subnets of a point on the host.  cpu: the reply order by a plain
// std::stable_sort, the independent form of model/icnt_reqreply.h's rule;
// cpu-par: rt_reply_build under the sequential lane policy
RrRaw rr_host(const OpenLoopNet& net, const RrPoint& pt, bool par, uint64_t step_cap, size_t index) {
  RrRaw raw;
  const uint32_t np = pt.req.np;
  raw.req = simulate_host(net, pt.req, par, step_cap);
  check_status(raw.req, index, "icnt_request_reply_batch: point ");
  raw.reply_of.assign(np, 0);
  raw.rep_src.assign(np, 0);
  raw.rep_dst.assign(np, 0);
  raw.rep_nfl.assign(np, 0);
  raw.rep_tinj.assign(np, 0);
  const RequestReplyParams& prm = pt.prm;
  if (par) {
    const RtReplyIn rq{pt.req.src.data(), pt.req.dst.data(), pt.kind.data(), raw.req.tarr.data()};
    const RtReplyOut rp{raw.rep_src.data(), raw.rep_dst.data(), raw.rep_nfl.data(), raw.rep_tinj.data()};
    std::vector<uint32_t> tmp(np);
    rt_reply_build<SeqPar>(np, rq, rp, prm.read_reply_size, prm.write_reply_size, prm.reply_delay,
                           raw.reply_of.data(), tmp.data());
  } else {
    for (uint32_t i = 0; i < np; ++i) raw.reply_of[i] = i;
    std::stable_sort(raw.reply_of.begin(), raw.reply_of.end(),
                     [&](uint32_t a, uint32_t b) { return raw.req.tarr[a] < raw.req.tarr[b]; });
    for (uint32_t j = 0; j < np; ++j) {
      const uint32_t i = raw.reply_of[j];
      raw.rep_src[j] = pt.req.dst[i];
      raw.rep_dst[j] = pt.req.src[i];
      raw.rep_nfl[j] = pt.kind[i] ? prm.write_reply_size : prm.read_reply_size;
      raw.rep_tinj[j] = raw.req.tarr[i] + prm.reply_delay;
    }
  }
  raw.rep = simulate_host(net, rr_reply_point(pt, raw), par, step_cap);
  return raw;
}

RequestReplyResult rr_finish(const OpenLoopNet& net, RrPoint& pt, RrRaw& raw, bool arrivals, size_t index) {
  check_status(raw.req, index, "icnt_request_reply_batch: point ");
  check_status(raw.rep, index, "icnt_request_reply_batch: point ");
  RequestReplyResult res;
  const OpenLoopPoint rep = rr_reply_point(pt, raw);
  res.request = icnt_open_loop_summarise(net, pt.req, raw.req);
  res.reply = icnt_open_loop_summarise(net, rep, raw.rep);
  res.reads = pt.reads;
  res.writes = pt.writes;
  res.deadlocked = raw.req.deadlocked + raw.rep.deadlocked;
  double sum = 0;
  uint64_t meas = 0;
  for (uint32_t j = 0; j < rep.np; ++j) {
    const uint32_t i = raw.reply_of[j];
    if (pt.req.tinj[i] < pt.prm.warmup) continue;
    const double rt = (double)(raw.rep.tarr[j] - pt.req.tinj[i]);
    sum += rt;
    ++meas;
    res.max_round_trip_latency = std::max(res.max_round_trip_latency, rt);
  }
  res.round_trip_latency = meas ? sum / meas : 0;
  if (arrivals) {
    res.request.arrivals = std::move(raw.req.tarr);
    res.request.state = std::move(raw.req.state);
    res.reply.arrivals = std::move(raw.rep.tarr);
    res.reply.state = std::move(raw.rep.state);
    res.request_src = std::move(pt.req.src);
    res.request_dst = std::move(pt.req.dst);
    res.request_flits = std::move(pt.req.nfl);
    res.request_tinj = std::move(pt.req.tinj);
    res.reply_of = std::move(raw.reply_of);
    res.reply_src = std::move(raw.rep_src);
    res.reply_dst = std::move(raw.rep_dst);
    res.reply_flits = std::move(raw.rep_nfl);
    res.reply_tinj = std::move(raw.rep_tinj);
  }
  return res;
}

}  // namespace

std::vector<OpenLoopResult> icnt_replay_batch(const std::string& icnt_text, const std::vector<ReplayList>& lists,
                                              const std::string& engine, const OpenLoopBatchOpts& opts, uint64_t cycles,
                                              uint64_t warmup) {
  check_engine("icnt_replay_batch", engine);
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  std::vector<OpenLoopResult> out;
  out.reserve(lists.size());
  auto done = [&](const OpenLoopPoint& pt, OpenLoopRaw& raw) {
    out.push_back(finish("icnt_replay_batch: list ", out.size(), net, pt, raw, opts.arrivals));
  };
  g_last = OpenLoopBatchStats();
  if (engine != "gpu") {
    for (size_t i = 0; i < lists.size(); ++i) {
      const OpenLoopPoint pt = replay_prepare(net, lists[i], i, cycles, warmup);
      OpenLoopRaw raw = simulate_host(net, pt, engine == "cpu-par", opts.step_cap);
      done(pt, raw);
    }
    return out;
  }
  rr_gpu_batch<OpenLoopPoint>(
      "icnt_replay_batch: list", net, lists.size(), opts,
      [&](size_t i) { return replay_prepare(net, lists[i], i, cycles, warmup); },
      [](const OpenLoopPoint& pt) {
        RrUnit u;
        u.req = &pt;
        return u;
      },
      [&](OpenLoopPoint& pt, RrRaw& raw) { done(pt, raw.req); });
  return out;
}

std::vector<OpenLoopResult> icnt_replay_networks(const ReplayBytesList& list,
                                                 const std::vector<std::string>& icnt_texts, const std::string& engine,
                                                 const OpenLoopBatchOpts& opts, uint64_t cycles, uint64_t warmup) {
  check_engine("icnt_replay_networks", engine);
  const size_t n = list.src.size();
  if (list.dst.size() != n || list.bytes.size() != n || list.tinj.size() != n)
    throw std::invalid_argument("icnt_replay_networks: src, dst, bytes and tinj differ in length");
  if (n > kReplayMaxPackets) throw std::invalid_argument("icnt_replay_networks: too many packets for one pass");
  auto who = [](size_t i) { return "icnt_replay_networks: network " + std::to_string(i); };
  // the list as network i replays it: that network's flits from the bytes
  auto flits_for = [&](const OpenLoopNet& net, size_t i) {
    if (list.nodes && net.N != list.nodes)
      throw std::invalid_argument(who(i) + " has " + std::to_string(net.N) + " nodes, the packet list is for " +
                                  std::to_string(list.nodes));
    const uint32_t max_fl = rt_flits(net.c, kRtMaxPktBytes);
    ReplayList l;
    l.src = list.src;
    l.dst = list.dst;
    l.tinj = list.tinj;
    l.flits.resize(n);
    for (size_t k = 0; k < n; ++k) l.flits[k] = std::min(rt_flits(net.c, list.bytes[k]), max_fl);
    return l;
  };
  std::vector<OpenLoopResult> out;
  out.reserve(icnt_texts.size());
  if (engine != "gpu") {
    for (size_t i = 0; i < icnt_texts.size(); ++i) {
      try {
        const ReplayList l = flits_for(icnt_open_loop_net(icnt_texts[i]), i);
        out.push_back(std::move(icnt_replay_batch(icnt_texts[i], {l}, engine, opts, cycles, warmup)[0]));
      } catch (const std::invalid_argument& e) {
        const std::string m = e.what();
        throw std::invalid_argument(m.rfind(who(i), 0) == 0 ? m : who(i) + ": " + m);
      }
    }
    g_last = OpenLoopBatchStats();
    return out;
  }
  // gpu: the networks are prepared one after the other and packed into
  // chunks under the memory budget (the list's device copy counts once per
  // chunk); a full chunk is one launch
  struct Item {
    OpenLoopNet net;
    OpenLoopPoint pt;
  };
  const NetList nl{&list.src, &list.dst, &list.bytes, &list.tinj};
  pack_chunks<Item, OpenLoopRaw>(
      "icnt_replay_networks: network", opts, icnt_net_list_bytes(nl), icnt_texts.size(),
      [&](size_t i) {
        Item it;
        try {
          it.net = icnt_open_loop_net(icnt_texts[i]);
          it.pt = replay_prepare(it.net, flits_for(it.net, i), 0, cycles, warmup);
        } catch (const std::invalid_argument& e) {
          const std::string m = e.what();
          throw std::invalid_argument(m.rfind(who(i), 0) == 0 ? m : who(i) + ": " + m);
        }
        return it;
      },
      [](const Item& it) { return icnt_net_unit_bytes(NetUnit{&it.net, &it.pt}); },
      [&](const std::vector<Item>& chunk, std::vector<OpenLoopRaw>& raws) {
        std::vector<NetUnit> units;
        for (const Item& it : chunk) units.push_back(NetUnit{&it.net, &it.pt});
        return icnt_net_run_chunk(nl, units, opts.step_cap, opts.lds, raws);
      },
      [&](Item& it, OpenLoopRaw& raw) {
        out.push_back(finish("icnt_replay_networks: network ", out.size(), it.net, it.pt, raw, opts.arrivals));
      });
  return out;
}

uint64_t icnt_replay_networks_lds_bytes(const std::vector<std::string>& icnt_texts) {
  std::vector<OpenLoopNet> nets;
  std::vector<OpenLoopPoint> pts(icnt_texts.size());
  for (const std::string& t : icnt_texts) nets.push_back(icnt_open_loop_net(t));
  std::vector<NetUnit> units;
  for (size_t i = 0; i < nets.size(); ++i) {
    pts[i].d = list_dims(nets[i], 1, 1);
    units.push_back(NetUnit{&nets[i], &pts[i]});
  }
  return icnt_net_hot_bytes(units);
}

std::vector<RequestReplySchedule> icnt_request_reply_schedule(const std::string& icnt_text,
                                                              const std::vector<RequestReplyParams>& points) {
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  std::vector<RequestReplySchedule> out;
  for (size_t i = 0; i < points.size(); ++i) {
    RrPoint pt = rr_prepare(net, points[i], i);
    RequestReplySchedule s;
    s.src = std::move(pt.req.src);
    s.dst = std::move(pt.req.dst);
    s.flits = std::move(pt.req.nfl);
    s.kind = std::move(pt.kind);
    s.tinj = std::move(pt.req.tinj);
    out.push_back(std::move(s));
  }
  return out;
}

std::vector<RequestReplyResult> icnt_request_reply_batch(const std::string& icnt_text,
                                                         const std::vector<RequestReplyParams>& points,
                                                         const std::string& engine, const OpenLoopBatchOpts& opts) {
  check_engine("icnt_request_reply_batch", engine);
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  std::vector<RequestReplyResult> out;
  out.reserve(points.size());
  g_last = OpenLoopBatchStats();
  if (engine != "gpu") {
    for (size_t i = 0; i < points.size(); ++i) {
      RrPoint pt = rr_prepare(net, points[i], i);
      RrRaw raw = rr_host(net, pt, engine == "cpu-par", opts.step_cap, i);
      out.push_back(rr_finish(net, pt, raw, opts.arrivals, i));
    }
    return out;
  }
  rr_gpu_batch<RrPoint>(
      "icnt_request_reply_batch: point", net, points.size(), opts,
      [&](size_t i) { return rr_prepare(net, points[i], i); }, rr_unit,
      [&](RrPoint& pt, RrRaw& raw) { out.push_back(rr_finish(net, pt, raw, opts.arrivals, out.size())); });
  return out;
}

// ---- closed-loop points ----

namespace {

// The doubled network of `net`: nodes [0, N) with links [0, L) and a second,
// disjoint copy on nodes [N, 2N) with links [L, 2L), as a table network.  A
// built-in topology's routes are enumerated with RtCtx::init_packet itself
// (bit 31 of a word keeps the torus dateline class; the pass copies table
// words raw); its channel latency stays uniform (lat / inj_lat empty).
OpenLoopNet doubled_net(const OpenLoopNet& net) {
  const char* who = "icnt_closed_loop_batch: ";
  if (net.c.rt_route == 1 || net.c.rt_route == 2)
    throw std::invalid_argument(std::string(who) + "routing_function " + (net.c.rt_route == 1 ? "min_adapt" : "valiant") +
                                " has no route tables (min_adapt and valiant are not modelled in closed loop)");
  if (net.kv.count("batch_count") && strtoull(net.kv.at("batch_count").c_str(), nullptr, 10) > 1)
    throw std::invalid_argument(std::string(who) + "batch_count above 1 is not modelled");
  const uint32_t N = net.N;
  if (N > kClosedLoopMaxNodes)
    throw std::invalid_argument(std::string(who) + "the network has " + std::to_string(N) + " nodes, at most " +
                                std::to_string(kClosedLoopMaxNodes) + " are supported");
  const RtDims d1 = list_dims(net, 1, 1);
  const uint32_t L = d1.L;
  OpenLoopNet b;
  b.c = net.c;
  b.kv = net.kv;
  b.anynet = true;
  b.N = 2 * N;
  b.an_L = 2 * L;
  b.an_H = d1.H;
  // the single network's routes, pair by pair
  std::vector<uint32_t> off((size_t)N * N + 1, 0), links;
  if (net.anynet) {
    off = net.rt_off;
    links = net.rt_links;
  } else {
    std::vector<uint32_t> scratch(rt_carve(d1, nullptr, nullptr), 0);
    std::vector<uint64_t> st(rt_state_words(d1), 0);
    RtWork w;
    rt_carve(d1, scratch.data(), &w);
    const RtCtx<RtHot<uint32_t*>> cx(net.c, d1, st.data(), w, RtHot<uint32_t*>{w.vhead, w.vcnt, w.vown, w.vout, w.vocc});
    for (uint32_t a = 0; a < N; ++a)
      for (uint32_t t = 0; t < N; ++t) {
        if (a != t) {
          w.src[0] = a;
          w.dst[0] = t;
          w.nfl[0] = 1;
          w.tinj[0] = 0;
          cx.init_packet(0, 0);
          links.insert(links.end(), w.route, w.route + w.nh[0]);
        }
        off[(size_t)a * N + t + 1] = (uint32_t)links.size();
      }
  }
  b.rt_off.assign((size_t)b.N * b.N + 1, 0);
  b.rt_links.reserve(2 * links.size());
  for (uint32_t a = 0; a < b.N; ++a)
    for (uint32_t t = 0; t < b.N; ++t) {
      const uint32_t sa = a / N, sb = t / N;
      if (sa == sb) {
        const size_t p1 = (size_t)(a % N) * N + t % N;
        for (uint32_t k = off[p1]; k < off[p1 + 1]; ++k) b.rt_links.push_back(links[k] + sa * L);
      }
      b.rt_off[(size_t)a * b.N + t + 1] = (uint32_t)b.rt_links.size();
    }
  if (net.anynet) {
    b.lat = net.lat;
    b.lat.insert(b.lat.end(), net.lat.begin(), net.lat.end());
    b.inj_lat = net.inj_lat;
    b.inj_lat.insert(b.inj_lat.end(), net.inj_lat.begin(), net.inj_lat.end());
  }
  return b;
}

// a closed-loop point: the request list with its kinds, then the pass's
// packets on the doubled network
struct ClPoint {
  ClosedLoopParams prm;
  OpenLoopPoint req;           // on the single network
  std::vector<uint32_t> kind;  // per request: 1 a write
  uint64_t reads = 0, writes = 0;
  uint32_t issuers = 0;
  RtDims d{};                          // the doubled network's pass
  std::vector<uint32_t> src, dst, nfl;  // its 2 * nq packets
  // the memory endpoint (model/icnt_closed.h rule 2m): CL_MEM_OFF, CL_MEM_ALL
  // (occ_all / lat_all for every request) or CL_MEM_LIST (per request: the
  // call's list's arrays, ext_*, else this point's own)
  uint32_t mem = CL_MEM_OFF, occ_all = 0, lat_all = 0;
  std::vector<uint32_t> occ, lat;
  const std::vector<uint32_t>*ext_occ = nullptr, *ext_lat = nullptr;
  int32_t mem_index = -1;  // of a many-networks call's memory points
};

const std::vector<uint32_t>* cl_occ(const ClPoint& pt) {
  return pt.mem != CL_MEM_LIST ? nullptr : pt.ext_occ ? pt.ext_occ : &pt.occ;
}
const std::vector<uint32_t>* cl_lat(const ClPoint& pt) {
  return pt.mem != CL_MEM_LIST ? nullptr : pt.ext_lat ? pt.ext_lat : &pt.lat;
}

ClPoint cl_prepare(const OpenLoopNet& net, const OpenLoopNet& dbl, const ClosedLoopParams& prm, size_t index) {
  const char* fn = "icnt_closed_loop_batch";
  const std::string who = std::string(fn) + ": point " + std::to_string(index);
  if (prm.batch_count > 1) throw std::invalid_argument(who + ": batch_count above 1 is not modelled");
  RequestReplyParams rp;
  rp.traffic = prm.traffic;
  rp.rate = prm.batch_size ? 0 : prm.rate;
  rp.cycles = prm.batch_size ? 1 : prm.cycles;
  rp.warmup = prm.batch_size ? 0 : prm.warmup;
  rp.seed = prm.seed;
  rp.write_fraction = prm.write_fraction;
  rp.read_request_size = prm.read_request_size;
  rp.read_reply_size = prm.read_reply_size;
  rp.write_request_size = prm.write_request_size;
  rp.write_reply_size = prm.write_reply_size;
  rp.reply_delay = prm.reply_delay;
  rp.mem_nodes = prm.mem_nodes;
  // a rate point's request list is rr_prepare's; a batch point's checks are (rate 0: no packets)
  RrPoint rr = rr_prepare(net, rp, index, fn);
  ClPoint pt;
  pt.prm = prm;
  const uint32_t N = net.N, M = prm.mem_nodes;
  pt.issuers = N - M;
  if (prm.batch_size) {
    if ((uint64_t)prm.batch_size * pt.issuers > kReplayMaxPackets / 2)
      throw std::invalid_argument(who + ": too many packets for one pass");
    OpenLoopPoint& q = rr.req;
    const SimCfg& c = net.c;
    Rng r{prm.seed * 0x2545f4914f6cdd1dull + 1};
    for (uint32_t k = 0; k < prm.batch_size; ++k)
      for (uint32_t s = 0; s < pt.issuers; ++s) {
        const uint32_t d = M ? N - M + (uint32_t)(r.next() % M)
                             : destination(prm.traffic, s, N, net.anynet ? N : c.topo_k, net.anynet ? 1u : c.topo_n, r);
        if (d == s) continue;  // a fixed point of a permutation sends nothing
        const uint32_t wr = r.uniform() < prm.write_fraction ? 1u : 0u;
        q.src.push_back(s);
        q.dst.push_back(d);
        q.tinj.push_back(0);
        q.nfl.push_back(wr ? prm.write_request_size : prm.read_request_size);
        rr.kind.push_back(wr);
        ++(wr ? rr.writes : rr.reads);
      }
    q.np = (uint32_t)q.src.size();
  }
  pt.req = std::move(rr.req);
  pt.kind = std::move(rr.kind);
  pt.reads = rr.reads;
  pt.writes = rr.writes;
  const uint32_t nq = pt.req.np;
  if (nq > kReplayMaxPackets / 2) throw std::invalid_argument(who + ": too many packets for one pass");
  if (prm.read_occupancy || prm.write_occupancy || prm.write_reply_delay >= 0) {
    const uint64_t wl = prm.write_reply_delay >= 0 ? (uint64_t)prm.write_reply_delay : prm.reply_delay;
    auto fits = [&](uint64_t v, const char* key) {
      if (v > kRtClMemMax)
        throw std::invalid_argument(who + ": " + key + " " + std::to_string(v) + " is above 2^24 (the memory endpoint's limit)");
    };
    fits(prm.read_occupancy, "read_occupancy");
    fits(prm.write_occupancy, "write_occupancy");
    fits(prm.reply_delay, "reply_delay");
    fits(wl, "write_reply_delay");
    pt.mem = CL_MEM_LIST;
    pt.occ.resize(nq);
    pt.lat.resize(nq);
    for (uint32_t i = 0; i < nq; ++i) {
      pt.occ[i] = pt.kind[i] ? prm.write_occupancy : prm.read_occupancy;
      pt.lat[i] = (uint32_t)(pt.kind[i] ? wl : prm.reply_delay);
    }
  }
  pt.src = pt.req.src;
  pt.dst = pt.req.dst;
  pt.nfl = pt.req.nfl;
  pt.src.resize(2 * (size_t)nq);
  pt.dst.resize(2 * (size_t)nq);
  pt.nfl.resize(2 * (size_t)nq);
  uint64_t flits = 0;
  for (uint32_t i = 0; i < nq; ++i) {
    rt_cl_fill_reply(pt.src.data(), pt.dst.data(), pt.nfl.data(), nq, i, N, pt.kind[i], prm.read_reply_size,
                     prm.write_reply_size);
    flits += (uint64_t)pt.nfl[i] + pt.nfl[nq + i];
  }
  if (flits > 0xffffffffull) throw std::invalid_argument(who + ": too many flits for one pass");
  pt.d = list_dims(dbl, 2 * nq, 1);
  pt.d.nf = std::max<uint32_t>(1, (uint32_t)flits);  // exactly the packets' flits
  return pt;
}

ClUnit cl_unit(const ClPoint& pt) {
  ClUnit u;
  u.d = pt.d;
  u.nq = pt.req.np;
  u.window = pt.prm.max_outstanding;
  u.delay = pt.prm.reply_delay;
  u.src = &pt.src;
  u.dst = &pt.dst;
  u.nfl = &pt.nfl;
  u.tinj = &pt.req.tinj;
  u.occ = cl_occ(pt);
  u.lat = cl_lat(pt);
  return u;
}

// the closed-loop pass of one point on the host
ClRaw cl_host(const OpenLoopNet& dbl, const ClPoint& pt, bool par, uint64_t step_cap) {
  ClRaw raw;
  const uint32_t nq = pt.req.np;
  raw.pass.state.assign(rt_state_words(pt.d), 0);
  raw.tiss.assign(nq, 0);
  raw.pass.tarr.assign(2 * (size_t)nq, 0);
  if (!nq) return raw;
  const uint64_t words = rt_carve(pt.d, nullptr, nullptr);
  std::vector<uint32_t> scratch(words + rt_cl_carve(pt.d, nq, nullptr, nullptr), 0);
  RtWork w;
  rt_carve(pt.d, scratch.data(), &w);
  RtClosed cl;
  std::vector<uint32_t> svc;
  cl.window = pt.prm.max_outstanding;
  cl.delay = pt.prm.reply_delay;
  if (pt.mem != CL_MEM_OFF) {
    cl.mem = 1;
    cl.occ_all = pt.occ_all;
    cl.lat_all = pt.lat_all;
    if (pt.mem == CL_MEM_LIST) {  // occupancies, then latencies
      svc = *cl_occ(pt);
      svc.insert(svc.end(), cl_lat(pt)->begin(), cl_lat(pt)->end());
      cl.svc = svc.data();
    }
  }
  rt_cl_carve(pt.d, nq, scratch.data() + words, &cl);
  w.rt_off = dbl.rt_off.data();
  w.rt_links = dbl.rt_links.data();
  w.lat = dbl.lat.empty() ? nullptr : dbl.lat.data();
  w.inj_lat = dbl.inj_lat.empty() ? nullptr : dbl.inj_lat.data();
  std::copy(pt.src.begin(), pt.src.end(), w.src);
  std::copy(pt.dst.begin(), pt.dst.end(), w.dst);
  std::copy(pt.nfl.begin(), pt.nfl.end(), w.nfl);
  std::copy(pt.req.tinj.begin(), pt.req.tinj.end(), w.tinj);
  if (par) {
    const RtHot<uint32_t*> hv{w.vhead, w.vcnt, w.vown, w.vout, w.vocc};
    raw.pass.deadlocked = rt_simulate_par_closed<SeqPar>(dbl.c, pt.d, raw.pass.state.data(), w, hv, cl, raw.pass.act,
                                                         &raw.pass.status, step_cap);
  } else {
    raw.pass.deadlocked =
        rt_simulate_closed(dbl.c, pt.d, raw.pass.state.data(), w, cl, raw.pass.act, &raw.pass.status, step_cap);
  }
  raw.pass.tarr.assign(w.tarr, w.tarr + 2 * (size_t)nq);
  raw.tiss.assign(cl.tiss, cl.tiss + nq);
  if (cl.mem) raw.created.assign(w.tinj + nq, w.tinj + 2 * (size_t)nq);
  return raw;
}

ClosedLoopResult cl_finish(const OpenLoopNet& net, ClPoint& pt, ClRaw& raw, bool arrivals, size_t index,
                           const char* who = "icnt_closed_loop_batch: point ") {
  check_status(raw.pass, index, who);
  const ClosedLoopParams& prm = pt.prm;
  const uint32_t N = net.N, nq = pt.req.np;
  const bool batch = prm.batch_size != 0;
  ClosedLoopResult r;
  r.nodes = N;
  r.issuers = pt.issuers;
  r.requests = nq;
  r.reads = pt.reads;
  r.writes = pt.writes;
  r.deadlocked = raw.pass.deadlocked;
  for (int i = 0; i < RT_ACT_COUNT; ++i) r.activity[i] = raw.pass.act[i];
  const std::vector<uint64_t>&tarr = raw.pass.tarr, &tinj = pt.req.tinj;
  std::vector<uint64_t> finish(N, 0);
  std::vector<char> has(N, 0);
  // the replies' creation times: the pass's with a memory endpoint
  std::vector<uint64_t> created = std::move(raw.created);
  if (pt.mem == CL_MEM_OFF) {
    created.resize(nq);
    for (uint32_t i = 0; i < nq; ++i) created[i] = tarr[i] + prm.reply_delay;
  }
  double lq = 0, lp = 0, lr = 0, stall = 0, flight = 0;
  uint64_t last = 0, ej_req = 0, ej_rep = 0;
  for (uint32_t i = 0; i < nq; ++i) {
    const uint64_t ti = raw.tiss[i], aq = tarr[i], ap = tarr[nq + i];
    last = std::max(last, ap);
    const uint32_t s = pt.req.src[i];
    has[s] = 1;
    finish[s] = std::max(finish[s], ap);
    if (batch || (aq >= prm.warmup && aq < prm.cycles)) ej_req += pt.nfl[i];
    if (batch || (ap >= prm.warmup && ap < prm.cycles)) ej_rep += pt.nfl[nq + i];
    if (ti == ~0ull) continue;  // never issued: a deadlock ended the pass
    flight += (double)(ap - ti);
    if (!batch && tinj[i] < prm.warmup) continue;
    ++r.measured;
    lq += (double)(aq - ti);
    lp += (double)(ap - created[i]);
    lr += (double)(ap - ti);
    stall += (double)(ti - tinj[i]);
    r.max_round_trip_latency = std::max(r.max_round_trip_latency, (double)(ap - ti));
    r.max_issue_stall = std::max(r.max_issue_stall, (double)(ti - tinj[i]));
  }
  if (r.measured) {
    r.request_latency = lq / r.measured;
    r.reply_latency = lp / r.measured;
    r.round_trip_latency = lr / r.measured;
    r.issue_stall = stall / r.measured;
  }
  r.batch_time = batch ? last : 0;
  const double window = (batch ? (double)std::max<uint64_t>(last, 1) : (double)(prm.cycles - prm.warmup)) * N;
  r.accepted_request = (double)ej_req / window;
  r.accepted_reply = (double)ej_rep / window;
  uint32_t active = 0;
  bool first = true;
  for (uint32_t s = 0; s < N; ++s) {
    if (!has[s]) continue;
    ++active;
    r.first_finish = first ? finish[s] : std::min(r.first_finish, finish[s]);
    r.last_finish = std::max(r.last_finish, finish[s]);
    first = false;
  }
  r.avg_outstanding = active && last ? flight / ((double)active * (double)last) : 0;
  {
    // the memory endpoint, node by node in the order of the requests' arrivals
    // (which strictly increase at a node): the server's recurrence once more
    // for the service start and end, the creation times from the pass
    const std::vector<uint32_t>*occ = cl_occ(pt), *lat = cl_lat(pt);
    std::vector<uint32_t> order;
    order.reserve(nq);
    for (uint32_t i = 0; i < nq; ++i)
      if (raw.tiss[i] != ~0ull && created[i] >= tarr[i]) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      const uint32_t na = pt.req.dst[a], nb = pt.req.dst[b];
      return na != nb ? na < nb : tarr[a] != tarr[b] ? tarr[a] < tarr[b] : a < b;
    });
    const double span = batch ? (double)std::max<uint64_t>(last, 1) : (double)(prm.cycles - prm.warmup);
    double mt = 0, wait = 0, hold = 0, usum = 0, served = 0;
    uint64_t busy = 0, count = 0;
    for (size_t k = 0; k < order.size(); ++k) {
      const uint32_t i = order[k], n = pt.req.dst[i];
      if (!k || pt.req.dst[order[k - 1]] != n) {
        busy = 0;
        served = 0;
      }
      const uint64_t oc = pt.mem == CL_MEM_OFF ? 0 : occ ? (*occ)[i] : pt.occ_all;
      const uint64_t la = pt.mem == CL_MEM_OFF ? prm.reply_delay : lat ? (*lat)[i] : pt.lat_all;
      const uint64_t start = std::max(tarr[i], busy);
      busy = start + oc;
      if (batch || tinj[i] >= prm.warmup) {
        ++count;
        mt += (double)(created[i] - tarr[i]);
        r.mem.max_mem_time = std::max(r.mem.max_mem_time, (double)(created[i] - tarr[i]));
        wait += (double)(start - tarr[i]);
        hold += (double)created[i] - (double)(busy + la);
        served += (double)oc;
      }
      if (k + 1 == order.size() || pt.req.dst[order[k + 1]] != n) {
        ++r.mem.mem_nodes_used;
        usum += served / span;
        r.mem.max_mem_utilisation = std::max(r.mem.max_mem_utilisation, served / span);
      }
    }
    if (count) {
      r.mem.mem_time = mt / count;
      r.mem.mem_wait = wait / count;
      r.mem.mem_hold = hold / count;
    }
    if (r.mem.mem_nodes_used) r.mem.mem_utilisation = usum / r.mem.mem_nodes_used;
  }
  const NetEnergy e = net_energy(net, pt.d, raw.pass.act, last);
  r.e_buffer = e.buffer;
  r.e_xbar = e.xbar;
  r.e_link = e.link;
  r.e_alloc = e.alloc;
  r.e_leak = e.leak;
  r.power_w = e.power_w;
  if (arrivals) {
    r.request_arrivals.assign(tarr.begin(), tarr.begin() + nq);
    r.reply_arrivals.assign(tarr.begin() + nq, tarr.end());
    r.tiss = std::move(raw.tiss);
    r.state = std::move(raw.pass.state);
    r.request_src = std::move(pt.req.src);
    r.request_dst = std::move(pt.req.dst);
    r.request_flits = std::move(pt.req.nfl);
    r.request_tinj = std::move(pt.req.tinj);
    r.kind = std::move(pt.kind);
    r.reply_created = std::move(created);
  }
  return r;
}

}  // namespace

std::vector<ClosedLoopResult> icnt_closed_loop_batch(const std::string& icnt_text,
                                                     const std::vector<ClosedLoopParams>& points,
                                                     const std::string& engine, const OpenLoopBatchOpts& opts) {
  check_engine("icnt_closed_loop_batch", engine);
  const OpenLoopNet net = icnt_open_loop_net(icnt_text);
  const OpenLoopNet dbl = doubled_net(net);
  std::vector<ClosedLoopResult> out;
  out.reserve(points.size());
  g_last = OpenLoopBatchStats();
  if (engine != "gpu") {
    for (size_t i = 0; i < points.size(); ++i) {
      ClPoint pt = cl_prepare(net, dbl, points[i], i);
      ClRaw raw = cl_host(dbl, pt, engine == "cpu-par", opts.step_cap);
      out.push_back(cl_finish(net, pt, raw, opts.arrivals, i));
    }
    return out;
  }
  pack_chunks<ClPoint, ClRaw>(
      "icnt_closed_loop_batch: point", opts, icnt_sweep_net_bytes(dbl), points.size(),
      [&](size_t i) { return cl_prepare(net, dbl, points[i], i); },
      [](const ClPoint& pt) { return icnt_cl_unit_bytes(cl_unit(pt)); },
      [&](const std::vector<ClPoint>& chunk, std::vector<ClRaw>& raws) {
        std::vector<ClUnit> units;
        for (const ClPoint& pt : chunk) units.push_back(cl_unit(pt));
        return icnt_cl_run_chunk(dbl, units, opts.step_cap, opts.lds, raws);
      },
      [&](ClPoint& pt, ClRaw& raw) { out.push_back(cl_finish(net, pt, raw, opts.arrivals, out.size())); });
  return out;
}

// ---- one request list, closed loop, over many networks and windows ----

namespace {

const char* const kClnWho = "icnt_closed_loop_networks: network ";

// a network of the call: the .icnt file's, its doubled network, and the list
// as a batch point of it (window and delay are set per unit)
struct ClnNet {
  size_t index = 0;
  OpenLoopNet net, dbl;
  ClPoint pt;
  uint64_t fl_req = 0, fl_rep = 0;
};

ClnNet cln_prepare(const ClosedLoopList& list, const std::string& icnt_text, size_t index, uint64_t delay) {
  const std::string who = kClnWho + std::to_string(index);
  auto bad = [&](const std::string& what) { throw std::invalid_argument(who + ": " + what); };
  const size_t nq = list.src.size();
  if (list.dst.size() != nq || list.req_bytes.size() != nq || list.reply_bytes.size() != nq ||
      list.tcreate.size() != nq)
    bad("src, dst, req_bytes, reply_bytes and tcreate differ in length");
  if (nq > kReplayMaxPackets / 2)
    bad("too many requests for one pass (" + std::to_string(nq) + ", at most " + std::to_string(kReplayMaxPackets / 2) + ")");
  ClnNet cn;
  cn.index = index;
  try {
    cn.net = icnt_open_loop_net(icnt_text);
    cn.dbl = doubled_net(cn.net);
  } catch (const std::invalid_argument& e) {
    bad(e.what());
  }
  const uint32_t N = cn.net.N;
  if (list.nodes && N != list.nodes)
    bad("the network has " + std::to_string(N) + " nodes, the request list is for " + std::to_string(list.nodes));
  if (!cn.net.c.flit_size) bad("flit_size is zero");
  std::vector<char> has(N, 0);
  for (size_t i = 0; i < nq; ++i) {
    const uint32_t s = list.src[i], t = list.dst[i];
    if (s >= N || t >= N)
      bad("request " + std::to_string(i) + " has a node out of range (" + std::to_string(s) + " -> " + std::to_string(t) +
          ", the network has " + std::to_string(N) + " nodes)");
    if (s == t) bad("request " + std::to_string(i) + " has src == dst (" + std::to_string(s) + ")");
    if (i && list.tcreate[i] < list.tcreate[i - 1])
      bad("request " + std::to_string(i) + " has a decreasing tcreate (the list must be in creation order)");
    has[s] = 1;
  }
  ClPoint& pt = cn.pt;
  pt.prm.batch_size = 1;  // a batch point: every request measured, batch_time the last reply's arrival
  pt.prm.reply_delay = delay;
  for (char h : has) pt.issuers += h ? 1 : 0;
  pt.src.assign(2 * nq, 0);
  pt.dst.assign(2 * nq, 0);
  pt.nfl.assign(2 * nq, 0);
  pt.req.tinj.assign(nq, 0);
  // the pass's packets as every engine derives them from the list
  RtWork fw{};
  fw.src = pt.src.data();
  fw.dst = pt.dst.data();
  fw.nfl = pt.nfl.data();
  fw.tinj = pt.req.tinj.data();
  RtClList l;
  l.src = list.src.data();
  l.dst = list.dst.data();
  l.req_bytes = list.req_bytes.data();
  l.reply_bytes = list.reply_bytes.data();
  l.tcreate = list.tcreate.data();
  l.nq = (uint32_t)nq;
  rt_cl_fill_list<SeqPar>(cn.net.c, l, N, fw);
  pt.req.np = (uint32_t)nq;
  pt.req.src.assign(pt.src.begin(), pt.src.begin() + nq);
  pt.req.dst.assign(pt.dst.begin(), pt.dst.begin() + nq);
  pt.req.nfl.assign(pt.nfl.begin(), pt.nfl.begin() + nq);
  for (size_t i = 0; i < nq; ++i) {
    cn.fl_req += pt.nfl[i];
    cn.fl_rep += pt.nfl[nq + i];
  }
  if (cn.fl_req + cn.fl_rep > 0xffffffffull) bad("too many flits for one pass");
  pt.d = list_dims(cn.dbl, 2 * (uint32_t)nq, 1);
  pt.d.nf = std::max<uint32_t>(1, (uint32_t)(cn.fl_req + cn.fl_rep));  // exactly the packets' flits
  return cn;
}

ClnUnit cln_unit(const ClnNet& cn, const ClPoint& pt) {
  ClnUnit u;
  u.dbl = &cn.dbl;
  u.d = pt.d;
  u.nq = pt.req.np;
  u.window = pt.prm.max_outstanding;
  u.delay = pt.prm.reply_delay;
  u.nfl = &pt.nfl;
  u.mem = pt.mem;
  u.occ = pt.occ_all;
  u.lat = pt.lat_all;
  return u;
}

// what the call refuses of the memory endpoint's arguments, naming them
void cln_check_mem(const ClosedLoopList& list, const std::vector<ClosedLoopMemPoint>& mem_points) {
  const std::string who = "icnt_closed_loop_networks: ";
  const size_t nq = list.src.size();
  const bool has = !list.occupancy.empty() || !list.latency.empty();
  if (has && list.occupancy.size() != nq)
    throw std::invalid_argument(who + "occupancy has " + std::to_string(list.occupancy.size()) + " entries, the list " +
                                std::to_string(nq));
  if (has && list.latency.size() != nq)
    throw std::invalid_argument(who + "latency has " + std::to_string(list.latency.size()) + " entries, the list " +
                                std::to_string(nq));
  for (size_t i = 0; has && i < nq; ++i) {
    if (list.occupancy[i] > kRtClMemMax)
      throw std::invalid_argument(who + "occupancy of request " + std::to_string(i) + " is above 2^24");
    if (list.latency[i] > kRtClMemMax)
      throw std::invalid_argument(who + "latency of request " + std::to_string(i) + " is above 2^24");
  }
  for (size_t m = 0; m < mem_points.size(); ++m) {
    const ClosedLoopMemPoint& mp = mem_points[m];
    if (mp.list && !has && nq)
      throw std::invalid_argument(who + "mem_points[" + std::to_string(m) +
                                  "] is `list`, but the list has no occupancy and latency arrays");
    if (!mp.list && (mp.occupancy > kRtClMemMax || mp.latency > kRtClMemMax))
      throw std::invalid_argument(who + "mem_points[" + std::to_string(m) + "] has an occupancy or latency above 2^24");
  }
}

// memory point m of the call (none: rule 2's reply_delay) for a unit's point
void cln_set_mem(ClPoint& pt, const ClosedLoopList& list, const std::vector<ClosedLoopMemPoint>& mem_points, size_t m) {
  if (mem_points.empty()) return;
  const ClosedLoopMemPoint& mp = mem_points[m];
  pt.mem_index = (int32_t)m;
  if (mp.list) {
    pt.mem = CL_MEM_LIST;
    pt.ext_occ = &list.occupancy;
    pt.ext_lat = &list.latency;
  } else {
    pt.mem = CL_MEM_ALL;
    pt.occ_all = mp.occupancy;
    pt.lat_all = mp.latency;
  }
}

ClosedLoopNetResult cln_finish(const ClnNet& cn, ClPoint& pt, ClRaw& raw, bool arrivals) {
  const size_t nq = pt.req.np;
  std::vector<uint32_t> nfl;
  if (arrivals) nfl = pt.nfl;
  ClosedLoopResult c = cl_finish(cn.net, pt, raw, arrivals, cn.index, kClnWho);
  ClosedLoopNetResult r;
  r.network = (uint32_t)cn.index;
  r.window = pt.prm.max_outstanding;
  r.mem_point = pt.mem_index;
  r.mem_list = pt.mem == CL_MEM_LIST;
  r.mem_occupancy = pt.occ_all;
  r.mem_latency = pt.mem == CL_MEM_ALL ? pt.lat_all : 0;
  r.mem = c.mem;
  r.nodes = c.nodes;
  r.issuers = c.issuers;
  r.requests = c.requests;
  r.measured = c.measured;
  r.request_flits = cn.fl_req;
  r.reply_flits = cn.fl_rep;
  r.batch_time = c.batch_time;
  r.request_latency = c.request_latency;
  r.reply_latency = c.reply_latency;
  r.round_trip_latency = c.round_trip_latency;
  r.max_round_trip_latency = c.max_round_trip_latency;
  r.issue_stall = c.issue_stall;
  r.max_issue_stall = c.max_issue_stall;
  r.accepted_request = c.accepted_request;
  r.accepted_reply = c.accepted_reply;
  r.avg_outstanding = c.avg_outstanding;
  r.first_finish = c.first_finish;
  r.last_finish = c.last_finish;
  r.deadlocked = c.deadlocked;
  for (int i = 0; i < 8; ++i) r.activity[i] = c.activity[i];
  r.e_buffer = c.e_buffer;
  r.e_xbar = c.e_xbar;
  r.e_link = c.e_link;
  r.e_alloc = c.e_alloc;
  r.e_leak = c.e_leak;
  r.power_w = c.power_w;
  if (arrivals) {
    r.request_flit_counts.assign(nfl.begin(), nfl.begin() + nq);
    r.reply_flit_counts.assign(nfl.begin() + nq, nfl.end());
    r.tiss = std::move(c.tiss);
    r.request_arrivals = std::move(c.request_arrivals);
    r.reply_arrivals = std::move(c.reply_arrivals);
    r.state = std::move(c.state);
    r.reply_created = std::move(c.reply_created);
  }
  return r;
}

}  // namespace

std::vector<ClosedLoopNetResult> icnt_closed_loop_networks(const ClosedLoopList& list,
                                                           const std::vector<std::string>& icnt_texts,
                                                           const std::vector<uint32_t>& windows, uint64_t reply_delay,
                                                           const std::string& engine, const OpenLoopBatchOpts& opts,
                                                           const std::vector<ClosedLoopMemPoint>& mem_points) {
  check_engine("icnt_closed_loop_networks", engine);
  cln_check_mem(list, mem_points);
  const size_t nw = windows.size(), nm = std::max<size_t>(mem_points.size(), 1);
  std::vector<ClosedLoopNetResult> out;
  out.reserve(icnt_texts.size() * nw * nm);
  g_last = OpenLoopBatchStats();
  if (engine != "gpu") {
    for (size_t i = 0; i < icnt_texts.size(); ++i) {
      const ClnNet cn = cln_prepare(list, icnt_texts[i], i, reply_delay);
      for (uint32_t window : windows)
        for (size_t m = 0; m < nm; ++m) {
          ClPoint pt = cn.pt;
          pt.prm.max_outstanding = window;
          cln_set_mem(pt, list, mem_points, m);
          ClRaw raw = cl_host(cn.dbl, pt, engine == "cpu-par", opts.step_cap);
          out.push_back(cln_finish(cn, pt, raw, opts.arrivals));
        }
    }
    return out;
  }
  // gpu: the (network, window, memory point) units are prepared one after the
  // other, network-major, and packed into chunks under the memory budget (the list's
  // device copy counts once per chunk, a network's tables once per unit); a
  // full chunk is one launch
  struct Item {
    std::shared_ptr<const ClnNet> cn;
    ClPoint pt;
  };
  ClList cl{&list.src, &list.dst, &list.req_bytes, &list.reply_bytes, &list.tcreate};
  for (const ClosedLoopMemPoint& mp : mem_points)
    if (mp.list && !list.occupancy.empty()) {  // uploaded with the list, once per chunk
      cl.occ = &list.occupancy;
      cl.lat = &list.latency;
    }
  std::shared_ptr<const ClnNet> cur;
  pack_chunks<Item, ClRaw>(
      "icnt_closed_loop_networks: unit", opts, icnt_cln_list_bytes(cl), icnt_texts.size() * nw * nm,
      [&](size_t i) {
        const size_t ni = i / (nw * nm);
        if (!cur || cur->index != ni) cur = std::make_shared<const ClnNet>(cln_prepare(list, icnt_texts[ni], ni, reply_delay));
        Item it{cur, cur->pt};
        it.pt.prm.max_outstanding = windows[i / nm % nw];
        cln_set_mem(it.pt, list, mem_points, i % nm);
        return it;
      },
      [](const Item& it) { return icnt_cln_unit_bytes(cln_unit(*it.cn, it.pt)); },
      [&](const std::vector<Item>& chunk, std::vector<ClRaw>& raws) {
        std::vector<ClnUnit> units;
        for (const Item& it : chunk) units.push_back(cln_unit(*it.cn, it.pt));
        return icnt_cln_run_chunk(cl, units, opts.step_cap, opts.lds, raws);
      },
      [&](Item& it, ClRaw& raw) { out.push_back(cln_finish(*it.cn, it.pt, raw, opts.arrivals)); });
  return out;
}

uint64_t icnt_closed_loop_networks_lds_bytes(const std::vector<std::string>& icnt_texts) {
  uint64_t b = 0;
  for (const std::string& t : icnt_texts) b = std::max(b, icnt_hot_bytes(list_dims(doubled_net(icnt_open_loop_net(t)), 1, 1)));
  return b;
}

}  // namespace asim
