// Exerciser of the lane policy (model/hd.h SeqPar, engine/wave_par.h WavePar)
// and of the GPU engine's register view (engine/sm_view.h), for unit tests
// (tests/test_lane_policy.py).
//
// One single-source function per group of primitives, templated on the policy
// P like the cycle model itself: it runs a named case on plain input arrays
// and writes plain output arrays.  The host instantiates it with SeqPar; a
// one-block, 64-thread kernel (lane_check.hip) instantiates it with WavePar,
// all 64 lanes active and every policy call in wave-uniform control flow (the
// documented contract of WavePar).  lane_plan() validates every length and
// index on the host before anything runs.
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../model/hd.h"
#include "../model/sm.h"
#include "engine.h"

namespace asim {

enum LaneCase : int {
  LC_BALLOT = 0, LC_BALLOT_M, LC_EACH_M, LC_RED_SUM, LC_RED_OR, LC_SUM, LC_VMAX, LC_VOR, LC_RED_SUM64, LC_RED_MIN64,
  LC_RED_MAX64, LC_ARGMIN, LC_FIND_FIRST, LC_SCAN, LC_ORDER16, LC_LANES, LC_UNI, LC_FETCH, LC_REG, LC_SB, LC_STAT,
  LC_VIEW, LC_MIN32
};

constexpr int kLaneScratch = 1024;   // bytes of scratch (LDS and HBM) a case may use
constexpr uint8_t kLaneCanary = 0xEE;
constexpr int kLaneMaxN = 4096;

// what the policy-templated code sees: plain arrays
struct LaneArgs {
  int id, sub, n;
  const uint64_t* val;
  int nval;
  const uint64_t* m;
  int nm;
  uint64_t* out;     // zero-filled, nout words
  uint8_t* scratch;  // kLaneScratch bytes, canary-filled, 16-byte aligned (LDS on the GPU unless the case says HBM)
};

struct LanePlan {
  int id = 0, sub = 0;
  size_t nout = 0;
  bool state = false;        // the case runs on an SMState image (LC_SB / LC_STAT / LC_VIEW)
  bool split = false;        // ... seen through SmSplit on the GPU
  bool scratch_hbm = false;  // the scratch is HBM on the GPU (fetch_copy's plain-copy path)
};

// value of type T made of the low bytes of (v, ~v): the tests' oracle builds the same bytes
template <class T>
SIM_HDI T lane_mk(uint64_t v) {
  const uint64_t w[2] = {v, ~v};
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
template <class T>
SIM_HDI void lane_emit(const T& x, uint64_t* o) {
  uint64_t w[2] = {0, 0};
  __builtin_memcpy(w, &x, sizeof(T));
  o[0] = w[0];
  o[1] = w[1];
}
struct LaneB16 { uint32_t w[4]; };
struct LaneB32 { uint32_t w[8]; };

// A per-warp field as the model sees it through P::view: under SeqPar the
// array itself; lane_check.hip specialises it for WavePar as a WarpReg<T>
// loaded from / stored to the array.
template <class P, class T, int N>
struct LaneReg {
  T (&a)[N];
  SIM_HDI explicit LaneReg(T (&arr)[N]) : a(arr) {}
  SIM_HDI T& operator[](int w) { return a[w]; }
  SIM_HDI void store(T (&)[N]) {}
};

template <class P, class T>
SIM_HD void lane_lanes_case(const LaneArgs& a) {
  auto L = P::template lanes<T>(a.n, [&](int i) { return lane_mk<T>(a.val[i]); });
  uint64_t* o = a.out;
  for (int k = 0; k < a.nm; ++k) {  // wave-uniform reads of one lane's value
    const T x = L.at((int)a.m[k]);
    P::one([&] { lane_emit(x, o + 2 * k); });
  }
  o += 2 * a.nm;
  P::each(a.n, [&](int i) { lane_emit(L.self(i), o + 2 * i); });
}

template <class P, class T>
SIM_HD void lane_uni_case(const LaneArgs& a) {
  const T x = P::uni(lane_mk<T>(a.val[0]));
  P::one([&] { lane_emit(x, a.out); });
}

template <class P, class T>
SIM_HD void lane_fetch_case(const LaneArgs& a) {
  P::fetch_copy(reinterpret_cast<T*>(a.scratch), reinterpret_cast<const T*>(a.val), a.n);
  P::fetch_wait();
  P::sync();
  const uint64_t* s = reinterpret_cast<const uint64_t*>(a.scratch);
  P::each(kLaneScratch / 8, [&](int i) { a.out[i] = s[i]; });
}

// WarpReg<T> over an array of extent N: reads with a wave-uniform index, with
// index == lane, inside each_m with one active lane; put and every Ref
// operator; load / store (the 64 - N slots after the array keep their canary)
template <class P, class T, int N>
SIM_HD void lane_reg_case(const LaneArgs& a) {
  T(&all)[64] = *reinterpret_cast<T(*)[64]>(a.scratch);
  P::each(64, [&](int i) { all[i] = (T)a.val[i]; });
  P::sync();
  T(&arr)[N] = *reinterpret_cast<T(*)[N]>(a.scratch);
  LaneReg<P, T, N> r(arr);
  const uint64_t live = N >= 64 ? ~0ull : ((1ull << (N & 63)) - 1);
  uint64_t* o = a.out;
  for (int k = 0; k < a.nm; ++k) {
    const T x = r[(int)a.m[k]];
    P::one([&] { o[k] = (uint64_t)(int64_t)x; });
  }
  o += a.nm;
  P::each_m(live, [&](int i) { o[i] = (uint64_t)(int64_t)(T)r[i]; });
  o += 64;
  for (int k = 0; k < a.nm; ++k) P::each_m(1ull << a.m[k], [&](int i) { o[k] = (uint64_t)(int64_t)(T)r[i]; });
  o += a.nm;
  for (int k = 0; k < a.nm; ++k) {
    const int j = (int)a.m[k];
    const T x = (T)a.val[64 + k];
    switch (k % 10) {
      case 0: r[j] = x; break;
      case 1: r[j] += x; break;
      case 2: r[j] -= x; break;
      case 3: r[j] |= x; break;
      case 4: r[j] &= x; break;
      case 5: ++r[j]; break;
      case 6: --r[j]; break;
      case 7: {
        const T old = r[j]++;
        P::one([&] { o[k] = (uint64_t)(int64_t)old; });
        break;
      }
      case 8: {
        const T old = r[j]--;
        P::one([&] { o[k] = (uint64_t)(int64_t)old; });
        break;
      }
      default: r[j] = r[(int)a.m[(k + 1) % a.nm]]; break;
    }
  }
  o += a.nm;
  P::each_m(live, [&](int i) { r[i] += (T)(i + 1); });
  r.store(arr);
  P::sync();
  P::each(64, [&](int i) { o[i] = (uint64_t)(int64_t)all[i]; });
}

template <class P, int N>
SIM_HD void lane_reg_types(const LaneArgs& a) {
  switch (a.sub >> 2) {
    case 0: lane_reg_case<P, uint8_t, N>(a); break;
    case 1: lane_reg_case<P, int8_t, N>(a); break;
    case 2: lane_reg_case<P, uint16_t, N>(a); break;
    case 3: lane_reg_case<P, int16_t, N>(a); break;
    case 4: lane_reg_case<P, uint32_t, N>(a); break;
    case 5: lane_reg_case<P, int32_t, N>(a); break;
    case 6: lane_reg_case<P, uint64_t, N>(a); break;
    default: lane_reg_case<P, int64_t, N>(a); break;
  }
}

// every case that needs no SM state
template <class P>
SIM_HD void lane_case_prim(const LaneArgs& a) {
  const uint64_t* v = a.val;
  const int n = a.n;
  switch (a.id) {
    case LC_BALLOT: {
      const uint64_t r = P::ballot(n, [&](int i) { return (v[i] & 1ull) != 0; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_BALLOT_M: {
      const uint64_t r = P::ballot_m(a.m[0], [&](int i) { return (v[i] & 1ull) != 0; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_EACH_M: P::each_m(a.m[0], [&](int i) { a.out[i] = v[i] + 1; }); break;
    case LC_RED_SUM: {
      uint32_t s = 0;
      P::lane_loop(n, [&](int i) { s += (uint32_t)v[i]; });
      const uint32_t r = P::red_sum(s);
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_RED_OR: {
      uint32_t s = 0;
      P::lane_loop(n, [&](int i) { s |= (uint32_t)v[i]; });
      const uint32_t r = P::red_or(s);
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_SUM: {
      const uint32_t r = P::sum(n, [&](int i) { return (uint32_t)v[i]; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_VMAX: {
      const uint32_t r = P::vmax(n, [&](int i) { return (uint32_t)v[i]; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_VOR: {
      const uint64_t r = P::vor(n, [&](int i) { return v[i]; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_RED_SUM64: {
      uint64_t s = 0;
      P::lane_loop(n, [&](int i) { s += v[i]; });
      const uint64_t r = P::red_sum64(s);
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_RED_MIN64: {
      uint64_t s = ~0ull;
      P::lane_loop(n, [&](int i) { s = amin(s, v[i]); });
      const uint64_t r = P::red_min64(s);
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_RED_MAX64: {
      uint64_t s = 0;
      P::lane_loop(n, [&](int i) { s = amax(s, v[i]); });
      const uint64_t r = P::red_max64(s);
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_ARGMIN: {
      const int r = P::argmin(n, [&](int i) { return v[i]; });
      P::one([&] { a.out[0] = (uint64_t)(int64_t)r; });
      break;
    }
    case LC_FIND_FIRST: {
      const int r = P::find_first(n, [&](int i) { return (v[i] & 1ull) != 0; });
      P::one([&] { a.out[0] = (uint64_t)(int64_t)r; });
      break;
    }
    case LC_SCAN: {
      const uint32_t r = P::scan(n, [&](int i) { return (uint32_t)v[i]; }, [&](int i, uint32_t x) { a.out[i] = x; });
      P::one([&] { a.out[n] = r; });
      break;
    }
    case LC_ORDER16: {
      const uint64_t r = P::order16(n, (uint32_t)a.m[0], [&](int i) { return (uint32_t)v[i]; });
      P::one([&] { a.out[0] = r; });
      break;
    }
    case LC_LANES:
      if (a.sub == 4) lane_lanes_case<P, uint32_t>(a);
      else if (a.sub == 8) lane_lanes_case<P, uint64_t>(a);
      else lane_lanes_case<P, LaneB16>(a);
      break;
    case LC_UNI:
      if (a.sub == 1) lane_uni_case<P, uint8_t>(a);
      else if (a.sub == 2) lane_uni_case<P, uint16_t>(a);
      else if (a.sub == 4) lane_uni_case<P, uint32_t>(a);
      else if (a.sub == 8) lane_uni_case<P, uint64_t>(a);
      else lane_uni_case<P, LaneB16>(a);
      break;
    case LC_FETCH:
      if (a.sub == 16) lane_fetch_case<P, LaneB16>(a);
      else lane_fetch_case<P, LaneB32>(a);
      break;
    case LC_MIN32: {
      // value i goes into slot m[i] (64 slots, the low words of out[0..64))
      P::each(64, [&](int i) { a.out[i] = 0xffffffffull; });
      P::sync();
      P::each(n, [&](int i) { P::min32(reinterpret_cast<uint32_t*>(a.out + a.m[i]), (uint32_t)v[i]); });
      P::sync();
      break;
    }
    case LC_REG:
      if ((a.sub & 3) == 0) lane_reg_types<P, 16>(a);
      else if ((a.sub & 3) == 1) lane_reg_types<P, 48>(a);
      else lane_reg_types<P, 64>(a);
      break;
    default: break;
  }
}

// ---- cases on an SM state seen through P::view -----------------------------
// (S is SMState, or SmSplit on the GPU; inside the view the state is SMState&
// under SeqPar and SmView<S>& under WavePar)

constexpr uint32_t kLaneStatLo = 60, kLaneStatHi = 70;  // a counter range spanning two register words
static_assert(kStatWords > 131, "the statistics cases address three register words");

template <class P, class S>
SIM_HD void lane_sb_case(const LaneArgs& a, S& s) {
  uint64_t* o = a.out;
  const uint64_t* v = a.val;
  uint64_t bal = 0;
  P::view(s, [&](auto& vw) {
    for (int k = 0; k < a.nm; ++k) {  // wave-uniform (warp, register)
      const uint32_t op = (uint32_t)(a.m[k] & 0xff), w = (uint32_t)(a.m[k] >> 8 & 0xff);
      const uint8_t r = (uint8_t)(a.m[k] >> 16);
      if (op == 0) sbs(vw.w_sb, w, r);
      else if (op == 1) sbc(vw.w_sb, w, r);
      else if (op == 2) {
        const bool t = sbt(vw.w_sb, w, r);
        P::one([&] { o[k] = t ? 1 : 0; });
      } else sbz(vw.w_sb, w);
    }
    // every warp its own register
    P::each_m(~0ull, [&](int w) { sbs(vw.w_sb, (uint32_t)w, (uint8_t)v[w]); });
    bal = P::ballot_m(~0ull, [&](int w) { return sbt(vw.w_sb, (uint32_t)w, (uint8_t)v[64 + w]); });
    P::each_m(~0ull, [&](int w) { sbc(vw.w_sb, (uint32_t)w, (uint8_t)v[128 + w]); });
  });
  P::one([&] { o[a.nm] = bal; });
  P::each(256, [&](int i) { o[a.nm + 1 + i] = s.w_sb[i >> 2][i & 3]; });
}

template <class P, class S>
SIM_HD void lane_stat_case(const LaneArgs& a, S& s) {
  uint64_t* o = a.out;
  const int nops = a.nm / 2;
  P::view(s, [&](auto& vw) {
    for (int k = 0; k < nops; ++k) {
      const uint32_t op = (uint32_t)(a.m[2 * k] & 0xff), c = (uint32_t)(a.m[2 * k] >> 8);
      const uint64_t d = a.m[2 * k + 1];
      switch (op) {
        case 0: vw.sadd(c, d); break;
        case 1: vw.template sadd_r<0, 64>(c, d); break;
        case 2: vw.template sadd_r<kLaneStatLo, kLaneStatHi>(c, d); break;
        case 3: vw.template sadd_r<0, (uint32_t)kStatWords>(c, d); break;
        case 4: {
          const uint64_t g = vw.sget(c);
          P::one([&] { o[k] = g; });
          break;
        }
        default: vw.sset(c, d); break;
      }
    }
  });
  P::each(kStatWords, [&](int i) { o[nops + i] = s.sget((uint32_t)i); });
}

// the round trip: an empty body must leave every byte, and a fixed list of
// in-range updates made through the view must land where SeqPar's land
template <class P, class S>
SIM_HD void lane_view_case(const LaneArgs& a, S& s) {
  const bool upd = a.val[1] != 0;
  const uint64_t mk = a.m[0];
  P::view(s, [&](auto& v) {
    if (!upd) return;
    // scalars held by value, one of each width, and two held by reference
    v.last_progress = 0x1122334455667788ull;
    v.epoch_end += 3;
    v.age_ctr += 7;
    v.n_cta_active = 5;
    v.live_mask ^= 0x8000000000000001ull;
    v.fetch_rr += 1;
    v.n_pend = 9;
    v.idoc_mask |= 1ull << 40;
    v.oc_mask &= 0x0f0fu;
    v.l1_stamp += 2;
    v.skipped_cycles += 11;
    v.min_emit = ~0ull;
    v.outq_head = 3;
    v.outq_n += 1;
    v.outstanding += 2;
    v.inq_head = 1;
    v.inq_n += 4;
    v.cl_head = 2;
    v.cl_n += 1;
    v.ld_head = 1;
    v.ld_n += 1;
    v.cycle += 1;
    v.arb_next = 3;
    v.used_thr += 64;
    // the LD/ST unit's record (held by value, 16-byte words)
    v.ldst.busy = 1;
    v.ldst.warp = 17;
    v.ldst.start += 5;
    v.ldst.inst.pc = 0x1230;
    v.ldst.inst.mask = 0xf0f0f0f0f0f0f0f0ull;
    // per-warp registers of every element type, first / last entries
    v.w_next[0] = 77;
    v.w_next[63] += 1;
    v.w_end[5] = v.w_next[0];
    v.w_flags[63] |= 0x80;
    v.w_ibuf[1] += 2;
    v.w_cta[62] = 31;
    v.w_inflight[7]++;
    v.w_stores[0] += 3;
    v.w_loads[63] -= 1;
    v.w_slot_used[9] |= 0x11;
    v.idoc_meta[kIdOc - 1] = idoc_pack(3, 2, 1);
    v.oc_info[kMaxOC - 1] += 1ull << 32;
    v.oc_banks[0] = 0xffff0102030405ull;
    v.oc_age[3] = 99;
    v.fu_next[U_COUNT * kMaxSched - 1] += 4;
    v.wb_occ[0] |= 1ull << 63;
    v.hit_occ[0] &= ~1ull;
    v.cta_valid[kMaxCta - 1] = 1;
    v.cta_live[0]--;
    v.cta_bar[5] += 1;
    v.cta_nexit[kMaxCta - 1] = 2;
    v.sched_last[kMaxSched - 1] = 9;
    v.w_iline[17] = 0xabcdef0123456789ull;
    // fields left in memory
    v.w_wait[4] = 0x0102;
    v.cta_id[2] = 1234;
    v.wb_cnt[3] += 1;  // (the split state's HBM tail)
    v.l1[2].lru = 5;
    // lane-parallel updates of the warps in the mask
    P::each_m(mk, [&](int w) {
      v.w_head[w] += (uint32_t)w;
      v.w_age[w] = v.w_next[w];
      v.w_flags[w] &= 0x7f;
    });
    sbs(v.w_sb, 3, 1);
    sbs(v.w_sb, 3, 255);
    sbc(v.w_sb, 9, 64);
    sbz(v.w_sb, 12);
    P::each_m(mk, [&](int w) { sbs(v.w_sb, (uint32_t)w, (uint8_t)(4 * w + 1)); });
    v.sadd(0, 5);
    v.sadd(63, 1);
    v.sadd(64, 1ull << 40);
    v.sadd((uint32_t)kStatWords - 1, 3);
    v.template sadd_r<kLaneStatLo, kLaneStatHi>(64, 2);
    v.sset(130, v.sget(63) + 1);
  });
}

template <class P, class S>
SIM_HD void lane_case_state(const LaneArgs& a, S& s) {
  if (a.id == LC_SB) lane_sb_case<P>(a, s);
  else if (a.id == LC_STAT) lane_stat_case<P>(a, s);
  else lane_view_case<P>(a, s);
}

// ---- host side ---------------------------------------------------------------

// the seeded byte pattern of a state image (splitmix64, little endian words)
inline void lane_fill_pattern(std::vector<uint64_t>& img, uint64_t seed) {
  uint64_t x = seed;
  for (auto& w : img) {
    x += 0x9e3779b97f4a7c15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    w = z ^ (z >> 31);
  }
}

inline LanePlan lane_plan(const std::string& name, int n, const std::vector<uint64_t>& val,
                          const std::vector<uint64_t>& m) {
  auto bad = [&](const char* why) { throw std::invalid_argument("lane_policy_check(" + name + "): " + why); };
  auto need = [&](bool ok, const char* why) {
    if (!ok) bad(why);
  };
  LanePlan p;
  const size_t nv = val.size(), nm = m.size();
  need(nv < (1u << 20) && nm < (1u << 20), "input too long");
  static const char* simple[] = {"ballot", "ballot_m", "each_m", "red_sum", "red_or", "sum", "vmax", "vor",
                                 "red_sum64", "red_min64", "red_max64", "argmin", "find_first", "scan", "order16"};
  for (int i = 0; i < 15; ++i)
    if (name == simple[i]) {
      p.id = i;
      p.nout = 1;
      if (i == LC_BALLOT) need(n >= 0 && n <= 64 && nv >= (size_t)n, "n <= 64 values");
      else if (i == LC_BALLOT_M || i == LC_EACH_M) {
        need(nv >= 64 && nm >= 1, "64 values and a mask");
        if (i == LC_EACH_M) p.nout = 64;
      } else if (i == LC_ORDER16) {
        need(n >= 0 && n <= 16 && nv >= (size_t)n && nm >= 1, "n <= 16 keys and a mask");
        need((m[0] >> n) == 0, "mask bits must be below n");
      } else {
        need(n >= 0 && n <= kLaneMaxN && nv >= (size_t)n, "n values, n <= 4096");
        if (i == LC_SCAN) p.nout = (size_t)n + 1;
      }
      return p;
    }
  if (name == "min32") {
    need(n >= 0 && n <= kLaneMaxN && nv >= (size_t)n && nm >= (size_t)n, "n values and n slots, n <= 4096");
    for (int i = 0; i < n; ++i) need(m[i] < 64, "slot below 64");
    p.id = LC_MIN32;
    p.nout = 64;
    return p;
  }
  auto tail_int = [&](const std::string& prefix) -> int {
    if (name.compare(0, prefix.size(), prefix) != 0) return -1;
    const std::string t = name.substr(prefix.size());
    if (t.empty() || t.size() > 3 || t.find_first_not_of("0123456789") != std::string::npos) return -1;
    return atoi(t.c_str());
  };
  int k;
  if ((k = tail_int("lanes")) >= 0) {
    need(k == 4 || k == 8 || k == 16, "lanes4 / lanes8 / lanes16");
    need(n >= 0 && n <= 64 && nv >= (size_t)n, "n <= 64 values");
    for (uint64_t i : m) need(i < (uint64_t)n, "lane index must be below n");
    p.id = LC_LANES;
    p.sub = k;
    p.nout = 2 * nm + 128;
    return p;
  }
  if ((k = tail_int("uni")) >= 0) {
    need(k == 1 || k == 2 || k == 4 || k == 8 || k == 16, "uni1 / 2 / 4 / 8 / 16");
    need(nv >= 1, "one value");
    p.id = LC_UNI;
    p.sub = k;
    p.nout = 2;
    return p;
  }
  for (const char* pre : {"fetch_lds", "fetch_hbm"})
    if ((k = tail_int(pre)) >= 0) {
      need(k == 16 || k == 32, "16- or 32-byte records");
      need(n >= 1 && n * (k / 16) <= 64, "1 record up to 64 16-byte chunks");
      need(nv >= (size_t)n * (k / 8), "n records of values");
      p.id = LC_FETCH;
      p.sub = k;
      p.scratch_hbm = std::string(pre) == "fetch_hbm";
      p.nout = kLaneScratch / 8;
      return p;
    }
  if (name.compare(0, 4, "reg_") == 0) {
    static const char* types[] = {"u8", "i8", "u16", "i16", "u32", "i32", "u64", "i64"};
    static const int extents[] = {16, 48, 64};
    for (int t = 0; t < 8; ++t)
      for (int e = 0; e < 3; ++e)
        if (name == std::string("reg_") + types[t] + "_" + std::to_string(extents[e])) {
          need(nm >= 1 && nm <= 64 && nv >= 64 + nm, "64 values, then one per index");
          for (uint64_t i : m) need(i < (uint64_t)extents[e], "index must be below the extent");
          p.id = LC_REG;
          p.sub = t << 2 | e;
          p.nout = 3 * nm + 128;
          return p;
        }
    bad("unknown register type / extent");
  }
  if (name == "sb" || name == "stat" || name == "view") {
    p.state = true;
    need(n == 0 || n == 1, "n: 0 = SMState, 1 = SmSplit");
    p.split = n == 1;
    need(nm <= 4096, "at most 4096 operations");
    if (name == "sb") {
      p.id = LC_SB;
      need(nv >= 193, "3 x 64 registers and the state seed");
      for (size_t i = 0; i < 192; ++i) need(val[i] < 256, "register below 256");
      for (uint64_t o : m) need((o & 0xff) < 4 && (o >> 8 & 0xff) < 64 && (o >> 24) == 0, "op < 4, warp < 64, register < 256");
      p.nout = nm + 1 + 256;
    } else if (name == "stat") {
      p.id = LC_STAT;
      need(nv >= 1 && nm % 2 == 0, "the state seed; (op | counter << 8, operand) pairs");
      for (size_t i = 0; i < nm; i += 2) {
        const uint64_t op = m[i] & 0xff, c = m[i] >> 8;
        need(op < 6 && c < (uint64_t)kStatWords, "op < 6, counter below kStatWords");
        if (op == 1) need(c < 64, "sadd_r<0, 64>: counter below 64");
        if (op == 2) need(c >= kLaneStatLo && c < kLaneStatHi, "sadd_r<60, 70>: counter in [60, 70)");
      }
      p.nout = nm / 2 + (size_t)kStatWords;
    } else {
      p.id = LC_VIEW;
      need(nv >= 2 && nm >= 1, "seed, update flag; a warp mask");
      p.nout = 0;
    }
    return p;
  }
  bad("unknown case");
  return p;
}

inline uint64_t lane_state_seed(const LanePlan& p, const std::vector<uint64_t>& val) {
  return val[p.id == LC_SB ? 192 : 0];
}

// the SeqPar half (plain host code)
inline void lane_check_host(const LanePlan& p, int n, const std::vector<uint64_t>& val, const std::vector<uint64_t>& m,
                            LaneCheckResult& r) {
  r.seq.assign(p.nout, 0);
  alignas(16) uint8_t scratch[kLaneScratch];
  memset(scratch, kLaneCanary, sizeof(scratch));
  // values live in a 16-byte aligned copy (fetch_copy's records)
  std::vector<uint64_t> vbuf(val.size() + 2);
  uint64_t* v = vbuf.data();
  if (reinterpret_cast<uintptr_t>(v) % 16) ++v;
  if (!val.empty()) memcpy(v, val.data(), val.size() * 8);
  LaneArgs a{p.id, p.sub, n, v, (int)val.size(), m.data(), (int)m.size(), r.seq.data(), scratch};
  if (!p.state) {
    lane_case_prim<SeqPar>(a);
    return;
  }
  static_assert(sizeof(SMState) % 16 == 0, "SMState is a whole number of 16-byte words");
  const size_t words = sizeof(SMState) / 8;
  r.seq_state.assign(words, 0);
  lane_fill_pattern(r.seq_state, lane_state_seed(p, val));
  // SMState is 16-byte aligned: run on an aligned copy of the image
  std::vector<uint64_t> al(words + 2);
  uint64_t* ap = al.data();
  if (reinterpret_cast<uintptr_t>(ap) % 16) ++ap;
  memcpy(ap, r.seq_state.data(), sizeof(SMState));
  lane_case_state<SeqPar>(a, *reinterpret_cast<SMState*>(ap));
  memcpy(r.seq_state.data(), ap, sizeof(SMState));
}

}  // namespace asim
