// Lane-parallel router pass: the driver of rt_simulate (icnt_router.h) written
// against the lane policy (SeqPar on the host, WavePar on the device: one
// 64-lane wavefront per network).  Same arguments, same scratch layout
// (rt_carve) and same contract as rt_simulate, and bit for bit the same
// results: w.tarr, the return value, act[RT_ACT_*] and the final state words.
//
// The router model itself -- routes, VC rules, the request query, the
// order-sensitive allocators, the commit and traversal of a matched pair, the
// event times -- is RtCtx of icnt_router.h, shared with rt_simulate: a change
// to it is made once.  This file owns how the phases run on lanes: what is
// staged, scanned and synchronised, the separable allocators' lane-parallel
// steps, the two-step commit and the wave-uniform activity counts.
//
// Lanes stride over the units of a phase in steps of 64.  Every list whose
// order the sequential pass depends on -- the source list, the active list,
// the request list and the credit FIFO -- is built with ordered scans
// (P::scan), never with atomics, so the order-sensitive allocators see the
// lists rt_simulate builds.
//
// Lane-parallel phases
//   setup        routes, dateline / Valiant classes and flit tables per packet
//                (flit bases by a scan over the packets' flit counts); the
//                buffer, unit and link tables per element
//   credits      the due prefix of the credit FIFO by ballot (the FIFO is in
//                time order); per 64 credits the ones of the same (unit, VC)
//                are grouped by ballot and vocc is decremented once per group
//                (speedup > 1 returns several credits of one VC in one cycle)
//   injection    per source; the surviving sources and the newly active
//                input units are appended in source-list order by scans
//   requests     per active input unit, the per-output dedup over its VCs
//                inside the lane (the adaptive head choice too: it only
//                reads downstream state that no request changes); the
//                request list is packed in active-list order by a scan
//   commit       per request: matched pairs are disjoint in the input unit
//                and in the link, and downstream unit N + l is written by
//                one pair only.  Two steps with a barrier between them: all
//                pops (and the credit FIFO entries, at scanned positions),
//                then all pushes -- a VC that loses its head flit and takes
//                a new packet's flit in the same pass has its count changed
//                by two pairs
//   matching     iSLIP, separable input first and separable output first: the
//                inputs' choice per input unit over its requests, the
//                outputs' choice as a minimum by key over the requests
//                (P::min32: the keys of one output's contenders are unique,
//                so the minimum does not depend on the order)
//   retire       per active input unit, compacted by a scan
//   next event   per source and per active input unit, min-reduced
//   deadlock     the undelivered packets' arrival per packet
//
// Under P::one (one lane, on the lists built above; exact by construction)
//   source queues   the per-source lists in (injection time, packet) order
//                   and the source list in first-packet order
//   matching        the order-sensitive allocators: wavefront, maximum size
//                   (augmenting paths), PIM (a reservoir over the requesters
//                   in list order) and LOA (RtCtx::allocate_ordered)
//
// Loop guard: rt_step_cap (icnt_router.h); a pass that exceeds it reports
// RT_STATUS_STEP_CAP: a bug ends the pass instead of spinning it.
//
// Closed loop (icnt_closed.h; rt_simulate_par_closed): the same driver with
// the closed-loop rules compiled in.  The issue gate runs a lane per listed
// source at the top of the injection phase; reply creation and release
// queuing run a lane per delivered packet in commit step 1 (two packets
// delivered in one switch pass arrive at different nodes); a reply node's
// first listing is an insertion by key under P::one, at most once per node
// and pass.
//
// Users: the open-loop sweep kernel (engine/icnt_sweep.hip, one wavefront per
// network) and, under -sim_router_pass par, the cycle engines' epoch pass
// (rt_epoch_run_par at the end of this file).
#pragma once
#include "icnt_router.h"

namespace asim {

// status (when given): RT_STATUS_*; step_cap 0: rt_step_cap of the pass
// (Closed: rt_cl_step_cap)
template <class P, class HV, bool Closed>
SIM_HDI uint32_t rt_simulate_par_core(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, const HV& hv,
                                      uint32_t np, uint64_t* act, uint32_t* status, uint64_t step_cap,
                                      const RtClosed& cl) {
  const RtCtx<HV> cx(c, d, st, w, hv);
  const uint32_t V = cx.V, B = cx.B, N = cx.N, L = cx.L, U = cx.U, alloc = cx.alloc;
  uint64_t *const gptr = cx.gptr, *const in_free = cx.in_free, *const aptr = cx.aptr, *const inj_next = cx.inj_next;
  uint64_t ac[RT_ACT_COUNT] = {};  // wave-uniform activity counts, added to act[] at the end
  // ---- setup ----
  P::each((int)N, [&](int s) {
    w.shead[s] = w.stail[s] = kRtNone;
    w.sfl[s] = 0;
    w.svc[s] = kRtNone;
    w.sflag[s] = 0;
  });
  const uint32_t nf = P::scan((int)np, [&](int p) { return w.nfl[p]; }, [&](int p, uint32_t x) { w.fbase[p] = x; });
  P::sync();
  P::each((int)np, [&](int p) { cx.init_packet((uint32_t)p, w.fbase[p]); });
  P::each((int)(U * V), [&](int i) {
    hv.vhead[i] = hv.vcnt[i] = hv.vocc[i] = 0;
    hv.vown[i] = hv.vout[i] = kRtNone;
  });
  P::each((int)U, [&](int u) {
    w.actf[u] = 0;
    w.a_tag[u] = w.m_u[u] = 0;
  });
  P::each((int)L, [&](int l) { w.g_tag[l] = w.m_l[l] = w.vis[l] = 0; });
  P::sync();
  // source queues (injection order: time, then packet)
  uint32_t nsrc = 0;
  P::one([&] {
    if constexpr (Closed) rt_cl_setup(cx, cl, nsrc);
    else
      for (uint32_t p = 0; p < np; ++p) cx.link_source(p, nsrc);
  });
  nsrc = P::uni(nsrc);
  P::sync();
  uint32_t dfs = 0;
  uint32_t nact = 0, tag = 0, rtag = 0, cr_r = 0, cr_w = 0, remaining = np, acc = 0;
  uint64_t now;
  {
    uint64_t m = ~0ull;
    P::lane_loop((int)nsrc, [&](int i) {
      uint64_t t = cx.source_time(w.slist[i]);
      if constexpr (Closed) t = rt_cl_gate_time(cx, cl, w.slist[i]);
      if (t < m) m = t;
    });
    now = P::red_min64(m);
  }
  const uint64_t cap = step_cap ? step_cap : Closed ? rt_cl_step_cap(d, nf, cl.nq) : rt_step_cap(d, nf);
  uint64_t steps = 0;
  uint32_t stat = RT_STATUS_OK;
  // rq_o[j] of a request that was not committed: else RtHop::to of its traversal
  constexpr uint32_t kUnmatched = 0xffffffffu;
  while (remaining > 0) {
    if (++steps > cap) {
      stat = RT_STATUS_STEP_CAP;
      break;
    }
    bool progress = false;
    // ---- credits that reach their upstream this cycle ----
    for (;;) {
      const uint32_t rem = cr_w - cr_r, n = rem < 64u ? rem : 64u;
      if (!n) break;
      const uint32_t base = cr_r;
      const uint64_t due = P::ballot((int)n, [&](int i) { return w.crt[base + i] <= now; });
      const uint32_t cnt = (uint32_t)popc64(due);  // (time order: a prefix)
      if (!cnt) break;
      auto uvs = P::template lanes<uint32_t>((int)cnt, [&](int i) { return w.crv[base + i]; });
      for (uint64_t pend = due; pend;) {
        const uint32_t luv = uvs.at(ffs64(pend));
        const uint64_t same = P::ballot_m(pend, [&](int i) { return uvs.self(i) == luv; });
        P::one([&] { hv.vocc[luv] -= (uint32_t)popc64(same); });
        pend &= ~same;
      }
      ac[RT_ACT_CREDIT] += cnt;
      cr_r += cnt;
      progress = true;
      if (cnt < 64u) break;
    }
    P::sync();
    // ---- injection: one flit per source per cycle ----
    {
      P::each((int)nsrc, [&](int i) {
        const uint32_t s = w.slist[i];
        if constexpr (Closed) rt_cl_gate(cx, cl, s, now);
        const uint32_t p = w.shead[s];
        uint32_t fl = 0;  // 1 stays listed, 2 input unit newly active, 4 injected
        w.st_u[i] = s;
        if (Closed ? !rt_cl_listed(cl, s) : p == kRtNone) {
          w.sflag[s] = 0;
          w.gb[i] = 0;
          return;
        }
        fl = 1;
        w.gb[i] = fl;
        if (Closed && p == kRtNone) return;
        if (now < w.tinj[p] || now < inj_next[s]) return;
        if (w.svc[s] == kRtNone) {
          const uint32_t v = cx.free_vc(s, 2);
          if (v == kRtNone) return;
          w.svc[s] = v;
          hv.vown[s * V + v] = p;
        }
        const uint32_t uv = s * V + w.svc[s];
        if (hv.vocc[uv] >= B) return;
        const uint32_t i_f = w.sfl[s], f = w.fbase[p] + i_f;
        cx.push(uv, f);
        ++hv.vocc[uv];
        w.fhop[f] = 0;
        w.ready[f] = now + (w.inj_lat ? w.inj_lat[s] : cx.chan) + (i_f == 0 ? cx.head_delay : cx.body_delay);
        fl |= 4;
        if (!w.actf[s]) {
          w.actf[s] = 1;
          fl |= 2;
        }
        inj_next[s] = now + 1;
        if (++w.sfl[s] == w.nfl[p]) {
          hv.vown[uv] = kRtNone;
          w.sfl[s] = 0;
          w.svc[s] = kRtNone;
          w.shead[s] = w.next[p];
          if constexpr (Closed) rt_cl_injected(cl, s);
        }
        w.gb[i] = fl;
      });
      P::sync();
      const uint32_t keep = P::scan((int)nsrc, [&](int i) { return w.gb[i] & 1u; },
                                    [&](int i, uint32_t x) { if (w.gb[i] & 1u) w.slist[x] = w.st_u[i]; });
      const uint32_t fresh = P::scan((int)nsrc, [&](int i) { return w.gb[i] >> 1 & 1u; },
                                     [&](int i, uint32_t x) { if (w.gb[i] & 2u) w.act[nact + x] = w.st_u[i]; });
      const uint32_t ninj = P::sum((int)nsrc, [&](int i) { return w.gb[i] >> 2 & 1u; });
      nsrc = keep;
      nact += fresh;
      ac[RT_ACT_BUF_WRITE] += ninj;
      if (ninj) progress = true;
      P::sync();
    }
    // ---- switch passes (internal speedup) ----
    acc += c.rt_speedup_q8 ? c.rt_speedup_q8 : 256u;
    const uint32_t passes = acc >> 8;
    acc &= 255u;
    for (uint32_t pass = 0; pass < passes; ++pass) {
      ++rtag;
      // requests: per input unit, per output the VC with the oldest eligible
      // head flit; staged per active-list slot (rq_k: VC, rq_o: link), then
      // packed in active-list order
      P::each((int)nact, [&](int i) {
        const uint32_t u = w.act[i];
        uint32_t cnt = 0;
        const uint32_t sb = (uint32_t)i * V;
        if (now >= in_free[u]) {
          for (uint32_t v = 0; v < V; ++v) {
            uint32_t f;
            const uint32_t l = cx.request(u, v, now, f);
            if (l == kRtNone) continue;
            uint32_t j = 0;
            while (j < cnt && w.rq_o[sb + j] != l) ++j;
            if (j == cnt) {
              w.rq_k[sb + cnt] = v;
              w.rq_o[sb + cnt] = l;
              ++cnt;
            } else if (cx.older(f, u, w.rq_k[sb + j])) {
              w.rq_k[sb + j] = v;
            }
          }
        }
        w.ge[i] = cnt;
      });
      P::sync();
      const uint32_t nrq = P::scan((int)nact, [&](int i) { return w.ge[i]; }, [&](int i, uint32_t x) { w.gb[i] = x; });
      P::sync();
      P::each((int)nact, [&](int i) {
        const uint32_t u = w.act[i], o = w.gb[i], sb = (uint32_t)i * V;
        for (uint32_t k = 0; k < w.ge[i]; ++k) {
          w.rq_u[o + k] = u;
          w.rq_v[o + k] = w.rq_k[sb + k];
          w.rq_l[o + k] = w.rq_o[sb + k];
        }
      });
      P::sync();
      ++ac[RT_ACT_PASSES];
      ac[RT_ACT_SA_REQ] += nrq;
      if (!nrq) continue;
      const uint32_t nru = nact;  // slot i < nru of the active list holds requests gb[i] .. gb[i] + ge[i]
      // matching
      for (uint32_t it = 0; it < cx.iters; ++it) {
        ++tag;
        if (cx.one_shot_alloc() && it > 0) break;
        if (!cx.ordered_alloc()) {
          // separable allocators, lane-parallel.  The keys (u - gptr[l]) mod U
          // of an output's contenders and (l - aptr[u]) mod L of an input's
          // are unique, so the minimum is the sequential scan's choice.
          // Inputs: a lane per input unit over its requests (contiguous in
          // the request list).  Outputs: a lane per request folds its key
          // into the output's word (P::min32), the request whose key is the
          // minimum takes the output.  `first`: the side that chooses first.
          auto input_step = [&](bool first) {
            P::each((int)nru, [&](int i) {
              const uint32_t u = w.act[i];
              if (first && w.m_u[u] == rtag) return;
              uint32_t bk = ~0u, bl = 0, bv = 0;
              for (uint32_t k = 0; k < w.ge[i]; ++k) {
                const uint32_t j = w.gb[i] + k, l = w.rq_l[j];
                if (first ? w.m_l[l] == rtag : (w.g_tag[l] != tag || w.g_in[l] != u)) continue;
                const uint32_t key = (uint32_t)((l + L - aptr[u] % L) % L);
                if (key < bk) {
                  bk = key;
                  bl = l;
                  bv = w.rq_v[j];
                }
              }
              if (bk != ~0u) {
                w.a_tag[u] = tag;
                w.a_key[u] = bk;
                w.a_l[u] = bl;
                w.a_v[u] = bv;
              }
            });
            P::sync();
          };
          auto output_step = [&](bool first) {
            auto contends = [&](int j, uint32_t& key) -> bool {
              const uint32_t u = w.rq_u[j], l = w.rq_l[j];
              if (first ? (w.m_u[u] == rtag || w.m_l[l] == rtag)
                        : (w.a_tag[u] != tag || w.a_l[u] != l || w.m_l[l] == rtag))
                return false;
              key = (uint32_t)((u + U - gptr[l] % U) % U);
              return true;
            };
            P::each((int)L, [&](int l) { w.g_key[l] = ~0u; });
            P::sync();
            P::each((int)nrq, [&](int j) {
              uint32_t key = 0;
              if (contends(j, key)) P::min32(&w.g_key[w.rq_l[j]], key);
            });
            P::sync();
            P::each((int)nrq, [&](int j) {
              uint32_t key = 0;
              const uint32_t l = w.rq_l[j];
              if (contends(j, key) && w.g_key[l] == key) {
                w.g_tag[l] = tag;
                w.g_in[l] = w.rq_u[j];
              }
            });
            P::sync();
          };
          if (alloc == RT_SEP_INPUT_FIRST) {
            input_step(true);
            output_step(false);
          } else {
            output_step(true);
            input_step(false);
          }
        } else {
          P::one([&] { cx.allocate_ordered(nrq, now, tag, rtag, it, dfs); });
        }
        dfs = P::uni(dfs);
        P::sync();
        // commit the pairs both sides chose, in request order
        P::each((int)nrq, [&](int j) {
          const uint32_t u = w.rq_u[j], l = w.rq_l[j];
          const bool hit = w.a_tag[u] == tag && w.a_l[u] == l && w.g_tag[l] == tag && w.g_in[l] == u &&
                           w.m_u[u] != rtag && w.m_l[l] != rtag;
          w.rq_k[j] = hit ? 1u : 0u;
          w.rq_o[j] = kUnmatched;
        });
        P::sync();
        // step 1: the pops and everything but the downstream push
        const uint32_t nmatch = P::scan((int)nrq, [&](int j) { return w.rq_k[j]; }, [&](int j, uint32_t x) {
          if (!w.rq_k[j]) return;
          const RtHop hop = cx.traverse(w.rq_u[j], w.rq_l[j], rtag, alloc != RT_ISLIP || it == 0, now, cr_w + x);
          w.rq_k[j] = hop.f;
          w.rq_o[j] = hop.to;
          // closed loop: the delivered packet's reply or release; rq_k (which
          // step 2 needs of moved flits only) then names a reply node to list
          if constexpr (Closed)
            if (hop.to == kRtDelivered) w.rq_k[j] = rt_cl_delivered(cx, cl, w.fpk[hop.f]);
        });
        P::sync();
        if constexpr (Closed) {
          auto lists = [&](int j) { return w.rq_o[j] == kRtDelivered && w.rq_k[j] != kRtNone; };
          const uint32_t nnew = P::sum((int)nrq, [&](int j) { return lists(j) ? 1u : 0u; });
          if (nnew) {
            P::one([&] {
              uint32_t ns = nsrc;
              for (uint32_t j = 0; j < nrq; ++j)
                if (lists((int)j)) rt_cl_list_source(cx, cl, w.rq_k[j], ns);
            });
            nsrc += nnew;
            P::sync();
          }
        }
        // step 2: the pushes; newly active downstream units in request order
        P::each((int)nrq, [&](int j) {
          const uint32_t duv = w.rq_o[j];
          if (duv >= kRtDelivered) {
            w.rq_k[j] = 0;
            return;
          }
          cx.push(duv, w.rq_k[j]);
          const uint32_t du = duv / V;
          w.rq_k[j] = w.actf[du] ? 0u : 1u;
          w.actf[du] = 1;
        });
        P::sync();
        const uint32_t fresh = P::scan((int)nrq, [&](int j) { return w.rq_k[j]; },
                                       [&](int j, uint32_t x) { if (w.rq_k[j]) w.act[nact + x] = w.rq_o[j] / V; });
        const uint32_t nlink = P::sum((int)nrq, [&](int j) { return w.rq_o[j] < kRtDelivered ? 1u : 0u; });
        const uint32_t ndone = P::sum((int)nrq, [&](int j) { return w.rq_o[j] == kRtDelivered ? 1u : 0u; });
        P::sync();
        nact += fresh;
        cr_w += nmatch;
        remaining -= ndone;
        ac[RT_ACT_BUF_READ] += nmatch;
        ac[RT_ACT_LINK] += nlink;
        ac[RT_ACT_EJECT] += nmatch - nlink;
        ac[RT_ACT_BUF_WRITE] += nlink;
        if (nmatch) progress = true;
        if (!nmatch) break;
      }
    }
    // ---- retire empty input units ----
    {
      P::each((int)nact, [&](int i) {
        const uint32_t u = w.act[i];
        uint32_t cnt = 0;
        for (uint32_t v = 0; v < V; ++v) cnt += hv.vcnt[u * V + v];
        w.st_u[i] = u;
        w.ge[i] = cnt ? 1u : 0u;
        if (!cnt) w.actf[u] = 0;
      });
      P::sync();
      nact = P::scan((int)nact, [&](int i) { return w.ge[i]; },
                     [&](int i, uint32_t x) { if (w.ge[i]) w.act[x] = w.st_u[i]; });
      P::sync();
    }
    if (!remaining) break;
    // ---- next cycle, or the next time anything can move ----
    uint64_t nxt = ~0ull;
    if (progress) {
      nxt = now + 1;
    } else {
      uint64_t m = ~0ull;
      P::lane_loop((int)nsrc, [&](int i) {
        const uint64_t t = cx.source_time(w.slist[i]);
        if (t > now && t < m) m = t;  // (t <= now: waiting for a credit)
        if constexpr (Closed) {
          const uint64_t g = rt_cl_gate_time(cx, cl, w.slist[i]);
          if (g > now && g < m) m = g;
        }
      });
      P::lane_loop((int)nact, [&](int i) {
        const uint64_t t = cx.unit_time(w.act[i], now);
        if (t < m) m = t;
      });
      nxt = P::red_min64(m);
      if (cr_r < cr_w && w.crt[cr_r] < nxt) nxt = w.crt[cr_r];
    }
    if (nxt == ~0ull) break;  // nothing can ever move: deadlock
    now = nxt;
  }
  if (remaining && stat == RT_STATUS_OK) P::each((int)np, [&](int p) { cx.deadlock_arrival((uint32_t)p, now); });
  P::sync();
  P::one([&] {
    if (act)
      for (int i = 0; i < RT_ACT_COUNT; ++i) act[i] += ac[i];
    if (status) *status = stat;
  });
  P::sync();
  return remaining;
}

template <class P, class HV>
SIM_HDN uint32_t rt_simulate_par_hot(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, const HV& hv,
                                     uint32_t np, uint64_t* act, uint32_t* status, uint64_t step_cap) {
  return rt_simulate_par_core<P, HV, false>(c, d, st, w, hv, np, act, status, step_cap, RtClosed());
}

// the closed-loop pass of icnt_closed.h over the doubled network (2 * cl.nq
// packets); bit for bit rt_simulate_closed
template <class P, class HV>
SIM_HDN uint32_t rt_simulate_par_closed(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, const HV& hv,
                                        const RtClosed& cl, uint64_t* act, uint32_t* status, uint64_t step_cap) {
  return rt_simulate_par_core<P, HV, true>(c, d, st, w, hv, 2 * cl.nq, act, status, step_cap, cl);
}

template <class P>
SIM_HDI uint32_t rt_simulate_par(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, uint32_t np,
                                 uint64_t* act = nullptr, uint32_t* status = nullptr, uint64_t step_cap = 0) {
  const RtHot<uint32_t*> hv{w.vhead, w.vcnt, w.vown, w.vout, w.vocc};
  return rt_simulate_par_hot<P>(c, d, st, w, hv, np, act, status, step_cap);
}

// ---- the cycle engines' epoch pass (-sim_router_pass par) ----
// rt_epoch_run (icnt_router.h) against the lane policy, one subnet or both:
// the same packets in the same order through rt_simulate_par, so the delays,
// the subnets' state words and the statistics are those of rt_epoch_run.
enum RtDir : uint32_t { RT_DIR_REQ = 1, RT_DIR_REP = 2, RT_DIR_BOTH = 3 };

// counters of the lane-parallel epoch pass for the host (outside the state
// image), per direction so that two blocks never write one word
struct RtPassCount {
  uint64_t passes[2];  // subnet passes that had packets {request, reply}
  uint32_t max_np[2];  // the largest packet count of one
};

// `dirs`: RtDir bits; `scratch`: rt_carve(rt_epoch_dims) words of this
// caller's own (two callers running one direction each share only `st`'s
// statistics words, which take P::add64).  Returns RT_STATUS_*: after
// RT_STATUS_STEP_CAP the pass's delays are not applied and the run must end.
template <class P>
SIM_HDN uint32_t rt_epoch_run_par(const SimCfg& c, Pkt* box_req, const uint32_t* cnt_req, uint32_t cap_req,
                                  Pkt* box_rep, const uint32_t* cnt_rep, uint32_t cap_rep, uint64_t* st,
                                  uint32_t* scratch, uint32_t dirs, RtPassCount* pc) {
  const RtDims d = rt_epoch_dims(c, cap_req, cap_rep);
  RtWork w;
  rt_carve(d, scratch, &w);
  uint64_t* stat = st + 2 * rt_state_words(d);
  const uint32_t ncell = c.n_sm * c.n_subpart;
  const uint32_t nfl_max = rt_flits(c, kRtMaxPktBytes);
  for (uint32_t dir = 0; dir < 2; ++dir) {
    if (!(dirs >> dir & 1u)) continue;
    const uint32_t* cnt = dir == 0 ? cnt_req : cnt_rep;
    Pkt* box = dir == 0 ? box_req : box_rep;
    const uint32_t cap = dir == 0 ? cap_req : cap_rep;
    // gather: the packets by cell, then by slot; a cell's first packet index
    // by an ordered scan over the cells' counts (staged in w.roff, which the
    // pass's setup rewrites; ncell <= d.np)
    auto cell_n = [&](int cell) -> uint32_t { return cnt[cell] < cap ? cnt[cell] : cap; };
    const uint32_t np = P::scan((int)ncell, cell_n, [&](int cell, uint32_t x) { w.roff[cell] = x; });
    if (!np) continue;
    P::sync();
    P::each((int)ncell, [&](int ci) {
      const uint32_t cell = (uint32_t)ci, n = cell_n(ci);
      if (!n) return;
      const RtCell ce = rt_cell(c, dir, cell);
      const uint64_t lat = icnt_pkt_lat_fs(c, ce.sm, ce.sub);
      const uint32_t o = w.roff[cell];
      for (uint32_t j = 0; j < n; ++j)
        rt_fill_packet(c, w, o + j, box[(uint64_t)cell * cap + j], ce, lat, nfl_max, cell * cap + j);
    });
    P::sync();
    // the pass; its status comes back through a scratch word every lane can read
    uint32_t* stw = w.ge;
    const uint32_t lost =
        rt_simulate_par<P>(c, d, st + (uint64_t)dir * rt_state_words(d), w, np, nullptr, stw, c.router_step_cap);
    if (P::uni(*stw) != RT_STATUS_OK) return RT_STATUS_STEP_CAP;
    // write-back: a packet's delay into its own mailbox slot
    uint64_t delayed = 0, wait = 0;
    P::lane_loop((int)np, [&](int i) {
      const uint64_t D = rt_packet_delay(c, w, (uint32_t)i);
      if (D) {
        ++delayed;
        wait += D;
        box[w.bidx[i]].t += D * c.per_icnt;
      }
    });
    delayed = P::red_sum64(delayed);
    wait = P::red_sum64(wait);
    if (delayed) P::add64(&stat[0], delayed);
    if (wait) P::add64(&stat[1], wait);
    if (lost) P::add64(&stat[2], lost);  // routing deadlock: those packets kept their uncontended latency
    if (pc) P::one([&] {
      ++pc->passes[dir];
      if (np > pc->max_np[dir]) pc->max_np[dir] = np;
    });
    P::sync();
  }
  return RT_STATUS_OK;
}

}  // namespace asim
