// Lane-parallel router pass: rt_simulate (icnt_router.h) written against the
// lane policy (SeqPar on the host, WavePar on the device: one 64-lane
// wavefront per network).  Same arguments, same scratch layout (rt_carve) and
// same contract as rt_simulate, and bit for bit the same results: w.tarr, the
// return value, act[RT_ACT_*] and the final state words.
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
//                   in list order) and LOA -- the code of rt_simulate,
//                   unchanged
//
// Loop guard: every iteration of the main loop either moves something (a
// credit, an injected flit, a flit hop) or jumps to a later event time, and
// there are at most as many distinct event times as events.  With
// E = flit-hops + credits + injections <= 2 * flits * H + flits, the loop is
// cut off after kRtGuardFactor * E + U + 64 iterations (a factor 2 would do
// for a correct pass; 4 leaves a margin) and the pass reports
// RT_STATUS_STEP_CAP: a bug ends the pass instead of spinning it.
//
// Users: the open-loop sweep kernel (engine/icnt_sweep.hip, one wavefront per
// network) and, under -sim_router_pass par, the cycle engines' epoch pass
// (rt_epoch_run_par at the end of this file).
#pragma once
#include "icnt_router.h"

namespace asim {

enum RtStatus : uint32_t { RT_STATUS_OK = 0, RT_STATUS_STEP_CAP = 1 };
constexpr uint64_t kRtGuardFactor = 4;

SIM_HDI uint64_t rt_step_cap(const RtDims& d, uint64_t flits) {
  return kRtGuardFactor * (2 * flits * d.H + flits) + d.U + 64;
}

// The per-(unit, VC) words of a pass -- head, count, owner, output VC and
// downstream occupancy of every input VC, the words every phase touches --
// behind pointers of their own type: the work arrays' (RtWork, HBM on the
// device) or, in the sweep kernel, LDS-typed pointers (U * V words each).
template <class Ptr>
struct RtHot {
  Ptr vhead, vcnt, vown, vout, vocc;
};

// status (when given): RT_STATUS_*; step_cap 0: rt_step_cap of the pass
template <class P, class HV>
SIM_HDN uint32_t rt_simulate_par_hot(const SimCfg& c, const RtDims& d, uint64_t* st, const RtWork& w, const HV& hv,
                                     uint32_t np, uint64_t* act, uint32_t* status, uint64_t step_cap) {
  uint64_t* link_next = st;
  uint64_t* gptr = st + d.L;
  uint64_t* in_free = st + 2 * d.L;
  uint64_t* aptr = st + 2 * d.L + d.U;
  uint64_t* inj_next = st + 2 * d.L + 2 * d.U;
  const uint32_t V = d.V, B = d.B, N = d.N, L = d.L, U = d.U;
  const uint64_t head_delay = c.hop_icnt > 0 ? c.hop_icnt - 1u : 0u, body_delay = c.rt_sa, chan = c.chan_icnt;
  const uint64_t slack = c.rt_speedup_q8 > 256 ? kRtOutSlack : 0;
  const uint32_t iters = c.rt_iters ? c.rt_iters : 1;
  const bool dateline = c.topo == TOPO_TORUS && V >= 2;
  const uint32_t tk = c.topo_k ? c.topo_k : 2, tn = c.topo_n ? c.topo_n : 1;
  const bool adaptive = c.rt_route == 1 && (c.topo == TOPO_MESH || c.topo == TOPO_CMESH) && V >= 2;
  const uint32_t aconc = c.topo == TOPO_CMESH ? (c.topo_conc ? c.topo_conc : 1) : 1, aP = 2 * tn + aconc;
  const bool valiant = c.rt_route == 2 && (c.topo == TOPO_MESH || c.topo == TOPO_CMESH) && V >= 2;
  const uint32_t alloc = c.rt_alloc;
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
  P::each((int)np, [&](int pi) {
    const uint32_t p = (uint32_t)pi;
    w.roff[p] = p * d.H;
    uint32_t h = 0, dim = ~0u, crossed = 0;
    if (adaptive) {
      h = icnt_routers(c, w.src[p], w.dst[p]);
      for (uint32_t i = 0; i < d.H; ++i) w.route[p * d.H + i] = kRtUnrouted;
      w.pcur[p] = w.src[p] / aconc;
    } else if (valiant) {
      const uint32_t nr = (uint32_t)ipow(tk, tn);
      const uint32_t mid = (uint32_t)(rt_hash(w.tinj[p] * 1000003u + w.src[p], w.dst[p]) % nr);
      const uint32_t mid_node = mid * aconc;
      icnt_route(c, w.src[p], mid_node, [&](uint32_t l) {
        if (h < d.H) w.route[p * d.H + h] = l;
        ++h;
      });
      --h;  // drop the ejection link into the intermediate node
      icnt_route(c, mid_node, w.dst[p], [&](uint32_t l) {
        if (h < d.H) w.route[p * d.H + h] = l | 1u << 31;
        ++h;
      });
    } else if (w.rt_off) {
      const uint64_t pr = (uint64_t)w.src[p] * N + w.dst[p];
      for (uint32_t i = w.rt_off[pr]; i < w.rt_off[pr + 1]; ++i) {
        if (h < d.H) w.route[p * d.H + h] = w.rt_links[i];
        ++h;
      }
    } else icnt_route(c, w.src[p], w.dst[p], [&](uint32_t l) {
      uint32_t cls = 0;
      if (dateline) {
        const uint32_t PP = 2 * tn + 1, port = l % PP, cur = l / PP;
        if (port < 2 * tn) {
          const uint32_t dd = port / 2;
          if (dd != dim) {
            dim = dd;
            crossed = 0;
          }
          const uint32_t x = (uint32_t)((cur / ipow(tk, dd)) % tk);
          if ((port % 2 == 0 && x == tk - 1) || (port % 2 == 1 && x == 0)) crossed = 1;
          cls = crossed;
        }
      }
      if (h < d.H) w.route[p * d.H + h] = l | cls << 31;
      ++h;
    });
    w.nh[p] = h < d.H ? h : d.H;
    const uint32_t fb = w.fbase[p];
    for (uint32_t i = 0; i < w.nfl[p]; ++i) {
      w.fpk[fb + i] = p;
      w.fhop[fb + i] = 0;
    }
    w.tarr[p] = 0;
    w.next[p] = kRtNone;
  });
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
    for (uint32_t p = 0; p < np; ++p) {
      const uint32_t s = w.src[p];
      if (w.shead[s] == kRtNone) {
        w.shead[s] = w.stail[s] = p;
        w.sflag[s] = 1;
        w.slist[nsrc++] = s;
      } else if (w.tinj[w.stail[s]] <= w.tinj[p]) {
        w.next[w.stail[s]] = p;
        w.stail[s] = p;
      } else if (w.tinj[p] < w.tinj[w.shead[s]]) {
        w.next[p] = w.shead[s];
        w.shead[s] = p;
      } else {
        uint32_t q = w.shead[s];
        while (w.next[q] != kRtNone && w.tinj[w.next[q]] <= w.tinj[p]) q = w.next[q];
        w.next[p] = w.next[q];
        w.next[q] = p;
      }
    }
  });
  nsrc = P::uni(nsrc);
  P::sync();
  uint32_t dfs = 0;
  uint32_t nact = 0, tag = 0, rtag = 0, cr_r = 0, cr_w = 0, remaining = np, acc = 0;
  auto push = [&](uint32_t uv, uint32_t f) {
    w.ring[(uint64_t)uv * B + (hv.vhead[uv] + hv.vcnt[uv]) % B] = f;
    ++hv.vcnt[uv];
  };
  auto free_vc = [&](uint32_t du, uint32_t cls) -> uint32_t {
    uint32_t v0 = 0, v1 = V;
    if (cls < 2 && (dateline || valiant)) {
      v0 = cls ? V / 2 : 0;
      v1 = cls ? V : V / 2;
    } else if (cls < 2 && adaptive) {
      v0 = cls ? 1 : 0;
      v1 = cls ? V : 1;
    }
    for (uint32_t v = v0; v < v1; ++v) {
      const uint32_t i = du * V + v;
      if (hv.vown[i] == kRtNone && hv.vocc[i] < B) return v;
    }
    return kRtNone;
  };
  auto adapt_choice = [&](uint32_t p) -> uint32_t {
    const uint32_t cur = w.pcur[p], dst = w.dst[p] / aconc;
    if (cur == dst) return cur * aP + 2 * tn + w.dst[p] % aconc;  // ejection
    uint32_t best = kRtUnrouted, best_free = 0, esc = kRtUnrouted;
    uint64_t pw = 1;
    for (uint32_t dd = 0; dd < tn; ++dd, pw *= tk) {
      const uint32_t x = (uint32_t)((cur / pw) % tk), y = (uint32_t)((dst / pw) % tk);
      if (x == y) continue;
      const uint32_t l = cur * aP + 2 * dd + (y > x ? 0u : 1u), du = N + l;
      if (esc == kRtUnrouted) esc = l;
      for (uint32_t v = 1; v < V; ++v) {
        const uint32_t i = du * V + v;
        if (hv.vown[i] == kRtNone && hv.vocc[i] < B && B - hv.vocc[i] > best_free) {
          best_free = B - hv.vocc[i];
          best = l;
        }
      }
    }
    if (best != kRtUnrouted) return best | 1u << 31;
    if (esc != kRtUnrouted && free_vc(N + esc, 0) != kRtNone) return esc;
    return kRtUnrouted;
  };
  uint64_t now;
  {
    uint64_t m = ~0ull;
    P::lane_loop((int)nsrc, [&](int i) {
      const uint32_t s = w.slist[i];
      const uint64_t t = w.tinj[w.shead[s]] > inj_next[s] ? w.tinj[w.shead[s]] : inj_next[s];
      if (t < m) m = t;
    });
    now = P::red_min64(m);
  }
  const uint64_t cap = step_cap ? step_cap : rt_step_cap(d, nf);
  uint64_t steps = 0;
  uint32_t stat = RT_STATUS_OK;
  // markers of a committed request (rq_o[j]): else the downstream (unit, VC) it pushes into
  constexpr uint32_t kUnmatched = 0xffffffffu, kEject = 0xfffffffeu, kDelivered = 0xfffffffdu;
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
        const uint32_t p = w.shead[s];
        uint32_t fl = 0;  // 1 stays listed, 2 input unit newly active, 4 injected
        w.st_u[i] = s;
        if (p == kRtNone) {
          w.sflag[s] = 0;
          w.gb[i] = 0;
          return;
        }
        fl = 1;
        w.gb[i] = fl;
        if (now < w.tinj[p] || now < inj_next[s]) return;
        if (w.svc[s] == kRtNone) {
          const uint32_t v = free_vc(s, 2);
          if (v == kRtNone) return;
          w.svc[s] = v;
          hv.vown[s * V + v] = p;
        }
        const uint32_t uv = s * V + w.svc[s];
        if (hv.vocc[uv] >= B) return;
        const uint32_t i_f = w.sfl[s], f = w.fbase[p] + i_f;
        push(uv, f);
        ++hv.vocc[uv];
        w.fhop[f] = 0;
        w.ready[f] = now + (w.inj_lat ? w.inj_lat[s] : chan) + (i_f == 0 ? head_delay : body_delay);
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
            const uint32_t uv = u * V + v;
            if (!hv.vcnt[uv]) continue;
            const uint32_t f = w.ring[(uint64_t)uv * B + hv.vhead[uv]];
            if (w.ready[f] > now) continue;
            const uint32_t p = w.fpk[f], h = w.fhop[f];
            if (adaptive && f == w.fbase[p]) {
              const uint32_t ch = adapt_choice(p);
              if (ch == kRtUnrouted) continue;
              w.route[w.roff[p] + h] = ch;
            }
            const uint32_t rl = w.route[w.roff[p] + h], l = rl & 0x7fffffffu;
            const bool last = h + 1 >= w.nh[p];
            if (!last) {
              const uint32_t du = N + l;
              if (f == w.fbase[p]) {
                if (free_vc(du, rl >> 31) == kRtNone) continue;
              } else if (hv.vocc[du * V + hv.vout[uv]] >= B) {
                continue;
              }
            }
            const uint64_t dep = link_next[l] > now + 1 ? link_next[l] : now + 1;
            if (dep > now + 1 + slack) continue;
            uint32_t j = 0;
            while (j < cnt && w.rq_o[sb + j] != l) ++j;
            if (j == cnt) {
              w.rq_k[sb + cnt] = v;
              w.rq_o[sb + cnt] = l;
              ++cnt;
            } else {
              const uint32_t gv = u * V + w.rq_k[sb + j];
              const uint32_t g = w.ring[(uint64_t)gv * B + hv.vhead[gv]];
              if (w.ready[f] < w.ready[g]) w.rq_k[sb + j] = v;
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
      for (uint32_t it = 0; it < iters; ++it) {
        ++tag;
        if ((alloc == RT_WAVEFRONT || alloc == RT_MAX_SIZE) && it > 0) break;
        if (alloc == RT_ISLIP || alloc == RT_SEP_INPUT_FIRST || alloc == RT_SEP_OUTPUT_FIRST) {
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
        } else P::one([&] {
          if (alloc == RT_WAVEFRONT) {
            const uint32_t n = U > L ? U : L, pd = (uint32_t)(now % n);
            for (uint32_t j = 0; j < nrq; ++j) {
              w.rq_k[j] = (w.rq_u[j] + w.rq_l[j] + n - pd) % n;
              uint32_t q = j;  // insertion into the order by (diagonal, request)
              while (q > 0 && w.rq_k[w.rq_o[q - 1]] > w.rq_k[j]) {
                w.rq_o[q] = w.rq_o[q - 1];
                --q;
              }
              w.rq_o[q] = j;
            }
            for (uint32_t q = 0; q < nrq; ++q) {
              const uint32_t j = w.rq_o[q], u = w.rq_u[j], l = w.rq_l[j];
              if (w.a_tag[u] == tag || w.g_tag[l] == tag) continue;
              w.a_tag[u] = w.g_tag[l] = tag;
              w.a_l[u] = l;
              w.a_v[u] = w.rq_v[j];
              w.g_in[l] = u;
            }
          } else if (alloc == RT_MAX_SIZE) {
            for (uint32_t j = 0; j < nrq; ++j) {
              if (j == 0 || w.rq_u[j - 1] != w.rq_u[j]) w.gb[w.rq_u[j]] = j;
              w.ge[w.rq_u[j]] = j + 1;
            }
            for (uint32_t j = 0; j < nrq; j = w.ge[w.rq_u[j]]) {
              ++dfs;
              uint32_t sp = 1;
              w.st_u[0] = w.rq_u[j];
              w.st_e[0] = w.gb[w.rq_u[j]];
              while (sp > 0) {
                const uint32_t u = w.st_u[sp - 1], e = w.st_e[sp - 1];
                if (e >= w.ge[u]) {
                  --sp;
                  continue;
                }
                w.st_e[sp - 1] = e + 1;
                const uint32_t l = w.rq_l[e];
                if (w.vis[l] == dfs) continue;
                w.vis[l] = dfs;
                if (w.g_tag[l] != tag) {
                  for (uint32_t k = sp; k-- > 0;) {
                    const uint32_t uu = w.st_u[k], ee = w.st_e[k] - 1, ll = w.rq_l[ee];
                    w.g_tag[ll] = tag;
                    w.g_in[ll] = uu;
                    w.a_tag[uu] = tag;
                    w.a_l[uu] = ll;
                    w.a_v[uu] = w.rq_v[ee];
                  }
                  break;
                }
                if (sp <= U) {
                  w.st_u[sp] = w.g_in[l];
                  w.st_e[sp] = w.gb[w.g_in[l]];
                  ++sp;
                }
              }
            }
          } else if (alloc == RT_PIM || alloc == RT_LOA) {
            for (uint32_t j = 0; j < nrq; ++j) w.ocnt[w.rq_l[j]] = 0;
            for (uint32_t j = 0; j < nrq; ++j) {
              const uint32_t u = w.rq_u[j], l = w.rq_l[j];
              if (w.m_u[u] == rtag || w.m_l[l] == rtag) continue;
              ++w.ocnt[l];
              if (j == 0 || w.rq_u[j - 1] != u) w.gb[u] = j;
              w.ge[u] = j + 1;
            }
            const uint64_t seed = now * 0x100000001b3ull + (uint64_t)rtag * 131u + it;
            for (uint32_t j = 0; j < nrq; ++j) {
              const uint32_t u = w.rq_u[j], l = w.rq_l[j];
              if (w.m_u[u] == rtag || w.m_l[l] == rtag) continue;
              if (alloc == RT_PIM) {
                const uint32_t n = w.g_tag[l] == tag ? w.g_key[l] + 1 : 1;
                if (n == 1 || rt_hash(seed, (uint64_t)l << 20 | n) % n == 0) w.g_in[l] = u;
                w.g_tag[l] = tag;
                w.g_key[l] = n;
              } else {
                const uint32_t key = (w.ge[u] - w.gb[u]) << 20 | (uint32_t)((u + U - gptr[l] % U) % U);
                if (w.g_tag[l] != tag || key < w.g_key[l]) {
                  w.g_tag[l] = tag;
                  w.g_key[l] = key;
                  w.g_in[l] = u;
                }
              }
            }
            for (uint32_t j = 0; j < nrq; ++j) {
              const uint32_t u = w.rq_u[j], l = w.rq_l[j];
              if (w.g_tag[l] != tag || w.g_in[l] != u) continue;
              if (alloc == RT_PIM) {
                const uint32_t n = w.a_tag[u] == tag ? w.a_key[u] + 1 : 1;
                if (n == 1 || rt_hash(seed + 7, (uint64_t)u << 20 | n) % n == 0) {
                  w.a_l[u] = l;
                  w.a_v[u] = w.rq_v[j];
                }
                w.a_tag[u] = tag;
                w.a_key[u] = n;
              } else {
                const uint32_t key = w.ocnt[l] << 20 | (uint32_t)((l + L - aptr[u] % L) % L);
                if (w.a_tag[u] != tag || key < w.a_key[u]) {
                  w.a_tag[u] = tag;
                  w.a_key[u] = key;
                  w.a_l[u] = l;
                  w.a_v[u] = w.rq_v[j];
                }
              }
            }
          }
        });
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
          const uint32_t u = w.rq_u[j], l = w.rq_l[j];
          w.m_u[u] = rtag;
          w.m_l[l] = rtag;
          // iSLIP moves its pointers on first-iteration matches only
          if (alloc != RT_ISLIP || it == 0) {
            gptr[l] = (u + 1) % U;
            aptr[u] = (l + 1) % L;
          }
          const uint32_t uv = u * V + w.a_v[u];
          const uint32_t f = w.ring[(uint64_t)uv * B + hv.vhead[uv]];
          hv.vhead[uv] = (hv.vhead[uv] + 1) % B;
          --hv.vcnt[uv];
          w.crt[cr_w + x] = now + 1 + c.rt_credit;
          w.crv[cr_w + x] = uv;
          in_free[u] = now;
          const uint32_t p = w.fpk[f], h = w.fhop[f], fi = f - w.fbase[p];
          const bool head = fi == 0, tail = fi + 1 == w.nfl[p];
          const uint64_t dep = link_next[l] > now + 1 ? link_next[l] : now + 1;
          link_next[l] = dep + 1;
          const uint64_t arr = dep + (w.lat ? w.lat[l] : chan);
          w.rq_k[j] = f;
          if (h + 1 < w.nh[p]) {
            const uint32_t du = N + l;
            if (head) {
              const uint32_t dv = free_vc(du, w.route[w.roff[p] + h] >> 31);
              hv.vout[uv] = dv;
              hv.vown[du * V + dv] = p;
            }
            if (adaptive && head) {
              const uint32_t port = l % aP, dd = port / 2;
              const uint32_t pw = (uint32_t)ipow(tk, dd);
              w.pcur[p] = port % 2 == 0 ? w.pcur[p] + pw : w.pcur[p] - pw;
            }
            const uint32_t duv = du * V + hv.vout[uv];
            ++hv.vocc[duv];
            w.fhop[f] = h + 1;
            w.ready[f] = arr + (head ? head_delay : body_delay);
            if (tail) {
              hv.vown[duv] = kRtNone;
              hv.vout[uv] = kRtNone;
            }
            w.rq_o[j] = duv;
          } else if (tail) {
            w.tarr[p] = arr;
            w.rq_o[j] = kDelivered;
          } else {
            w.rq_o[j] = kEject;
          }
        });
        P::sync();
        // step 2: the pushes; newly active downstream units in request order
        P::each((int)nrq, [&](int j) {
          const uint32_t duv = w.rq_o[j];
          if (duv >= kDelivered) {
            w.rq_k[j] = 0;
            return;
          }
          push(duv, w.rq_k[j]);
          const uint32_t du = duv / V;
          w.rq_k[j] = w.actf[du] ? 0u : 1u;
          w.actf[du] = 1;
        });
        P::sync();
        const uint32_t fresh = P::scan((int)nrq, [&](int j) { return w.rq_k[j]; },
                                       [&](int j, uint32_t x) { if (w.rq_k[j]) w.act[nact + x] = w.rq_o[j] / V; });
        const uint32_t nlink = P::sum((int)nrq, [&](int j) { return w.rq_o[j] < kDelivered ? 1u : 0u; });
        const uint32_t ndone = P::sum((int)nrq, [&](int j) { return w.rq_o[j] == kDelivered ? 1u : 0u; });
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
        const uint32_t s = w.slist[i], p = w.shead[s];
        if (p == kRtNone) return;
        const uint64_t t = w.tinj[p] > inj_next[s] ? w.tinj[p] : inj_next[s];
        if (t > now && t < m) m = t;  // (t <= now: waiting for a credit)
      });
      P::lane_loop((int)nact, [&](int i) {
        const uint32_t u = w.act[i];
        for (uint32_t v = 0; v < V; ++v) {
          const uint32_t uv = u * V + v;
          if (!hv.vcnt[uv]) continue;
          const uint32_t f = w.ring[(uint64_t)uv * B + hv.vhead[uv]];
          uint64_t t = w.ready[f] > in_free[u] ? w.ready[f] : in_free[u];
          const uint32_t l = w.route[w.roff[w.fpk[f]] + w.fhop[f]] & 0x7fffffffu;
          if (l < L && link_next[l] > 1 + slack && link_next[l] - 1 - slack > t) t = link_next[l] - 1 - slack;
          if (t > now && t < m) m = t;  // (t <= now: waiting for a VC or a credit)
        }
      });
      nxt = P::red_min64(m);
      if (cr_r < cr_w && w.crt[cr_r] < nxt) nxt = w.crt[cr_r];
    }
    if (nxt == ~0ull) break;  // nothing can ever move: deadlock
    now = nxt;
  }
  if (remaining && stat == RT_STATUS_OK) {
    // deadlocked packets: their uncontended traversal after the last event
    P::each((int)np, [&](int p) {
      if (!w.tarr[p]) w.tarr[p] = (now > w.tinj[p] ? now : w.tinj[p]) + rt_uncontended(c, w.nh[p], w.nfl[p]);
    });
  }
  P::sync();
  P::one([&] {
    if (act)
      for (int i = 0; i < RT_ACT_COUNT; ++i) act[i] += ac[i];
    if (status) *status = stat;
  });
  P::sync();
  return remaining;
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
  const uint32_t cpc = c.cores_per_cluster ? c.cores_per_cluster : 1;
  const uint32_t nfl_max = rt_flits(c, kRtMaxPktBytes);  // the scratch holds nfl_max flits per packet
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
      uint32_t a, b, sm, sub;
      if (dir == 0) {  // request: SM (cell % n_sm) -> sub-partition (cell / n_sm)
        sm = cell % c.n_sm;
        sub = cell / c.n_sm;
        a = sm / cpc;
        b = c.n_clusters + sub;
      } else {  // reply: sub-partition (cell % n_subpart) -> SM (cell / n_subpart)
        sub = cell % c.n_subpart;
        sm = cell / c.n_subpart;
        a = c.n_clusters + sub;
        b = sm / cpc;
      }
      const uint64_t lat = icnt_pkt_lat_fs(c, sm, sub);
      const uint32_t o = w.roff[cell];
      for (uint32_t j = 0; j < n; ++j) {
        const Pkt& p = box[(uint64_t)cell * cap + j];
        const uint64_t t0 = p.t > lat ? p.t - lat : 0;
        const uint32_t nfl = rt_flits(c, p.size ? p.size : 1);
        w.src[o + j] = a;
        w.dst[o + j] = b;
        w.nfl[o + j] = nfl < nfl_max ? nfl : nfl_max;
        w.tinj[o + j] = fdiv(t0, c.dv_icnt);
        w.bidx[o + j] = cell * cap + j;
      }
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
      const uint64_t base = w.tinj[i] + rt_uncontended(c, icnt_routers(c, w.src[i], w.dst[i]), w.nfl[i]);
      const uint64_t D = w.tarr[i] > base ? w.tarr[i] - base : 0;
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
