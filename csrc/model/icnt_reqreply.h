// Request-reply traffic over two subnets: the reply subnet's injection
// schedule from the request subnet's arrivals, written against the lane policy
// (SeqPar on the host, WavePar on the device) like the router pass it sits
// between (icnt_router_par.h).
//
// Request i, delivered (tail) at rq.tarr[i], produces one reply
//   source       rq.dst[i]
//   destination  rq.src[i]
//   flits        fl_write if rq.kind[i] else fl_read
//   injection    rq.tarr[i] + delay
// and the replies are numbered in ascending (injection, i) order: a stable
// sort of the requests by arrival.  reply_of[j] is reply j's request.
//
// No phase walks the packets on one lane:
//   range    the smallest and largest arrival by lane-strided loops and wave
//            reductions (the delay is common to all keys and drops out)
//   sort     least-significant-bit first over the significant bits of
//            (arrival - smallest): per bit a stable split, the zeros' places by
//            an exclusive scan and the ones' behind them (place = zeros +
//            index - zeros before), ping-pong between reply_of and tmp
//   scatter  per reply, its fields from its request
// A split is stable, so equal arrivals stay in request order.
#pragma once
#include "icnt_router.h"

namespace asim {

// significant bits of x (0 for x == 0)
SIM_HDI uint32_t rt_bits64(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

// the requests after their pass (the pass's work arrays, and per request 1
// for a write), and the reply pass's work arrays to fill; np entries each
struct RtReplyIn {
  const uint32_t *src, *dst, *kind;
  const uint64_t* tarr;
};
struct RtReplyOut {
  uint32_t *src, *dst, *nfl;
  uint64_t* tinj;
};

// reply_of, tmp: np words each.  np <= 2^31 - 1.
template <class P>
SIM_HDN void rt_reply_build(uint32_t np, const RtReplyIn& rq, const RtReplyOut& rp, uint32_t fl_read,
                            uint32_t fl_write, uint64_t delay, uint32_t* reply_of, uint32_t* tmp) {
  if (!np) return;
  uint64_t lo = ~0ull, hi = 0;
  P::lane_loop((int)np, [&](int i) {
    const uint64_t a = rq.tarr[i];
    if (a < lo) lo = a;
    if (a > hi) hi = a;
  });
  lo = P::red_min64(lo);
  hi = P::red_max64(hi);
  const uint32_t bits = rt_bits64(hi - lo);
  uint32_t *a = reply_of, *b = tmp;
  P::each((int)np, [&](int i) { a[i] = (uint32_t)i; });
  P::sync();
  for (uint32_t bit = 0; bit < bits; ++bit) {
    auto zero = [&](int j) -> uint32_t { return (uint32_t)(~((rq.tarr[a[j]] - lo) >> bit) & 1ull); };
    const uint32_t zeros = P::sum((int)np, zero);
    (void)P::scan((int)np, zero, [&](int j, uint32_t x) {
      const uint32_t i = a[j];
      b[zero(j) ? x : zeros + ((uint32_t)j - x)] = i;
    });
    P::sync();
    uint32_t* t = a;
    a = b;
    b = t;
  }
  if (a != reply_of) {
    P::each((int)np, [&](int j) { reply_of[j] = a[j]; });
    P::sync();
  }
  P::each((int)np, [&](int j) {
    const uint32_t i = reply_of[j];
    rp.src[j] = rq.dst[i];
    rp.dst[j] = rq.src[i];
    rp.nfl[j] = rq.kind[i] ? fl_write : fl_read;
    rp.tinj[j] = rq.tarr[i] + delay;
  });
  P::sync();
}

}  // namespace asim
