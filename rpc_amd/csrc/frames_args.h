// rpc_amd/csrc/frames_args.h -- the frame args: the declared parameters of each
// routed request, decoded into typed 64-bit slots (rpc_frames_args_device;
// DESIGN.md 4.19).  What sits between the route and the handlers: the
// reference's generated rpc_parse_params_<method> functions, for a whole batch.
//
// args_precheck() applies rules 1-5 of include/rpccrc.h before any body byte is
// read.  args_one() applies rules 6-10 to one `params` span: the route's strict
// automaton (its states and byte classes, frames_route.h) walks the span once,
// here over any JSON value and not only an object; at each depth-1 key of a root
// object it compares the key with the method's parameter names, and when the
// value of a matching key ends it converts that value and hands the slot to the
// caller's sink, so that no lane keeps an array of slots.  Numbers are read
// again from the staged bytes once the automaton has accepted them
// (args_number): at most 19 significant digits and a decimal exponent, to a
// double by the exact path or by Eisel-Lemire (args_eisel_lemire) over the
// 128-bit powers of five of pow10_table.h.
//
// Everything here is plain inline code with no HIP types, shared by the kernel
// (frames_args.hip) and the CPU emulator (tests/cpu_emu/args_emu.cpp).
#pragma once
#include <stdint.h>

#include "frames_route.h"
#include "pow10_table.h"

namespace rpccrc {

// RPC_ARGS_* and RPC_ARG_* of include/rpccrc.h (the emulator builds without that header).
constexpr uint8_t kArgsNone = 0, kArgsOk = 1, kArgsInvalid = 2, kArgsDefer = 3, kArgsRange = 4, kArgsBadSchema = 5;
constexpr uint8_t kArgsWalk = 0xFF; // args_precheck: the span is to be walked
constexpr uint8_t kArgI32 = 0, kArgI64 = 1, kArgF64 = 2, kArgBool = 3, kArgStr = 4;
constexpr uint32_t kArgsMaxParams = 8, kArgsMaxSchemaParams = 1024, kArgsMaxNameBytes = 4096;
constexpr int32_t kArgsReplyOk = 0, kArgsReplyInvalid = -32602, kArgsReplyInternal = -32603;

ROUTE_HD int32_t args_reply_status(uint8_t status) {
  return status == kArgsOk ? kArgsReplyOk : status == kArgsInvalid ? kArgsReplyInvalid : kArgsReplyInternal;
}

// Rules 1-5.  Schema: uint32_t first(m), word m of the nmethods + 1; uint32_t
// type(p); uint32_t name_off(p), word p of the nparams + 1; uint32_t name(b),
// byte b of the names.  Only the words of the entry's own method are read, and
// each only after the word before it has been found inside its array.
// Returns the status, or kArgsWalk with the method's parameters [*f0, *f1).
template <class Schema>
ROUTE_HD uint8_t args_precheck(uint8_t kind, uint32_t method, const Schema &sc, uint32_t nmethods, uint32_t nparams,
                               uint32_t name_bytes, uint32_t width, uint64_t body_off, uint32_t body_len,
                               uint32_t p_off, uint32_t p_len, uint64_t bodies_bytes, uint32_t *f0, uint32_t *f1) {
  *f0 = *f1 = 0;
  if (kind != kRouteCall) return kArgsNone;
  if (method >= nmethods) return kArgsBadSchema;
  const uint32_t a = sc.first(method), b = sc.first(method + 1);
  if (a > b || b > nparams || b - a > width) return kArgsBadSchema;
  for (uint32_t p = a; p < b; ++p) {
    const uint32_t x = sc.name_off(p), y = sc.name_off(p + 1);
    if (x > y || y > name_bytes || sc.type(p) > kArgStr) return kArgsBadSchema;
  }
  if (!(body_off <= bodies_bytes && body_len <= bodies_bytes - body_off)) return kArgsRange;
  if (!(p_off <= body_len && p_len <= body_len - p_off)) return kArgsRange;
  *f0 = a, *f1 = b;
  if (a == b) return kArgsOk;            // rule 4: the span is not read
  if (p_len == 0) return kArgsInvalid;   // rule 5
  if (p_len > kRouteMaxBody) return kArgsDefer; // (rule 6: the route's length limit)
  return kArgsWalk;
}

// ---- decimal to double ----------------------------------------------------------
ROUTE_HD void args_mul64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *lo = a * b;
  *hi = __umul64hi(a, b);
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *lo = (uint64_t)p;
  *hi = (uint64_t)(p >> 64);
#endif
}
ROUTE_HD uint64_t args_double_bits(double d) {
  union {
    double d;
    uint64_t u;
  } x;
  x.d = d;
  return x.u;
}
ROUTE_HD double args_bits_double(uint64_t u) {
  union {
    double d;
    uint64_t u;
  } x;
  x.u = u;
  return x.d;
}

// Pow: uint64_t word(uint32_t i), word i of RPCCRC_POW10_WORDS.
// w != 0, kPow10Min <= q <= kPow10Max: the double nearest w * 10^q, ties to
// even (Eisel-Lemire; for a 64-bit w no case needs a fallback, Mushtak & Lemire
// 2023).  False when that double is zero, subnormal or infinite.
template <class Pow> ROUTE_HD bool args_eisel_lemire(uint64_t w, int32_t q, const Pow &pow, uint64_t *bits) {
  const int32_t lz = __builtin_clzll(w);
  w <<= lz;
  const uint32_t idx = 2u * (uint32_t)(q - kPow10Min);
  uint64_t hi, lo;
  args_mul64(w, pow.word(idx), &hi, &lo);
  if ((hi & 0x1FFu) == 0x1FFu) { // the 55 bits kept are not settled by the high word alone
    uint64_t hi2, lo2;
    args_mul64(w, pow.word(idx + 1), &hi2, &lo2);
    lo += hi2;
    if (hi2 > lo) ++hi;
  }
  const int32_t upper = (int32_t)(hi >> 63);
  const int32_t shift = upper + 64 - 52 - 3;
  uint64_t m = hi >> shift;
  // floor(log2(10^q)) + 63, then the biased exponent
  int32_t p2 = (int32_t)(((int64_t)(152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023;
  if (p2 <= 0) { // zero or subnormal, unless the rounding carries into the smallest normal
    if (-p2 + 1 >= 64) return false;
    m >>= -p2 + 1;
    m += m & 1u;
    m >>= 1;
    if (m < (1ull << 52)) return false;
    *bits = 1ull << 52; // (m == 2^52: biased exponent 1, fraction 0)
    return true;
  }
  // the exact tie: round to even, not up
  if (lo <= 1 && q >= -4 && q <= 23 && (m & 3u) == 1u && (m << shift) == hi) m &= ~1ull;
  m += m & 1u;
  m >>= 1;
  if (m >= (2ull << 52)) m = 1ull << 52, ++p2;
  m &= ~(1ull << 52);
  if (p2 >= 0x7FF) return false;
  *bits = ((uint64_t)p2 << 52) | m;
  return true;
}

// The number at bytes [a, b) of the body, which the automaton has accepted, as
// the bits of the double strtod gives.  False (DEFER) with more than 19
// significant digits or when a non-zero number's double is not normal.
template <class Body, class Pow>
ROUTE_HD bool args_number(const Body &body, uint32_t a, uint32_t b, const Pow &pow, uint64_t *bits) {
  const bool neg = body.at(a) == '-';
  uint64_t w = 0;
  uint32_t nd = 0, frac = 0, i = a + (neg ? 1u : 0u);
  bool dot = false, many = false;
  for (; i < b; ++i) {
    const uint32_t c = body.at(i);
    if (c == '.') {
      dot = true;
      continue;
    }
    if (c == 'e' || c == 'E') break;
    if (dot) ++frac;
    const uint32_t v = c - '0';
    if (w == 0 && v == 0) continue; // a leading zero
    if (nd == 19) many = true;
    else w = w * 10u + v, ++nd;
  }
  int32_t ex = 0;
  if (i < b) { // the exponent
    ++i;
    bool eneg = false;
    const uint32_t c = body.at(i);
    if (c == '+' || c == '-') eneg = c == '-', ++i;
    for (; i < b; ++i)
      if (ex < 100000) ex = ex * 10 + (int32_t)(body.at(i) - '0');
    if (eneg) ex = -ex;
  }
  const uint64_t sign = neg ? 1ull << 63 : 0;
  if (w == 0) {
    *bits = sign;
    return true;
  }
  if (many) return false;
  const int32_t q = ex - (int32_t)frac;
  if (q < kPow10Min || q > kPow10Max) return false;
  if (w < (1ull << 53) && q >= -22 && q <= 22) {
    // the exact path: one correctly rounded operation on two exact doubles
    // (5^|q| < 2^53: the table's high word without its shift), then the power
    // of two, which is exact
    const uint32_t aq = (uint32_t)(q < 0 ? -q : q);
    const uint64_t p5w = pow.word(2u * (uint32_t)((int32_t)aq - kPow10Min));
    const double p5 = (double)(p5w >> __builtin_ctzll(p5w)), dw = (double)w;
    const double r = q < 0 ? dw / p5 : dw * p5;
    *bits = (args_double_bits(r) + ((uint64_t)(int64_t)q << 52)) | sign; // (modulo 2^64: q may be negative)
    return true;
  }
  uint64_t u;
  if (!args_eisel_lemire(w, q, pow, &u)) return false;
  *bits = u | sign;
  return true;
}

// trunc(d) of a finite double as sign and magnitude; false at 2^64 and above.
ROUTE_HD bool args_trunc(uint64_t bits, bool *neg, uint64_t *mag) {
  *neg = (bits >> 63) != 0;
  const uint32_t be = (uint32_t)(bits >> 52) & 0x7FFu;
  const uint64_t m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
  *mag = 0;
  if (be < 1023) return true; // |d| < 1
  const uint32_t sh = be - 1023;
  if (sh > 63) return false;
  *mag = sh <= 52 ? m >> (52 - sh) : m << (sh - 52);
  return true;
}
// (int64_t)trunc(d) when it is inside [-2^bits1, 2^bits1), bits1 = 31 or 63.
ROUTE_HD bool args_to_int(uint64_t dbits, uint32_t bits1, uint64_t *slot) {
  bool neg;
  uint64_t mag;
  if (!args_trunc(dbits, &neg, &mag)) return false;
  const uint64_t lim = 1ull << bits1;
  if (neg ? mag > lim : mag >= lim) return false;
  *slot = neg ? 0ull - mag : mag;
  return true;
}

// The string contents at bytes [a, b) as the reference's strtoll reads what its
// client prints: -?[0-9]{1,19} and a value inside int64.
template <class Body> ROUTE_HD bool args_i64_string(const Body &body, uint32_t a, uint32_t b, uint64_t *slot) {
  const bool neg = a < b && body.at(a) == '-';
  if (neg) ++a;
  if (b - a < 1 || b - a > 19) return false;
  uint64_t v = 0; // (19 digits stay below 2^64)
  for (uint32_t i = a; i < b; ++i) {
    const uint32_t d = body.at(i) - '0';
    if (d > 9u) return false;
    v = v * 10u + d;
  }
  if (neg ? v > (1ull << 63) : v >= (1ull << 63)) return false;
  *slot = neg ? 0ull - v : v;
  return true;
}

// ---- rules 6-10 -------------------------------------------------------------------
// Body: the span's bytes (frames_route.h's Body); base: the span's offset in the
// body (a STR slot counts from the body's first byte); [f0, f1): the method's
// parameters, at least one; Sink: put(k, slot) takes parameter f0 + k's slot,
// possibly more than once and also for an entry that ends INVALID or DEFER (the
// caller zeroes those).
template <class Body, class Schema, class Pow, class Sink>
ROUTE_HD uint8_t args_one(Body &body, uint32_t len, uint32_t base, const Schema &sc, uint32_t f0, uint32_t f1,
                          const Pow &pow, Sink &sink) {
  uint32_t state = kRsStart, depth = 0, stack = 0, tokens = 0, lit = 0;
  uint32_t key_at = 0, v_off = 0;
  uint32_t seen = 0; // bit k: parameter f0 + k's name has occurred as a depth-1 key
  uint32_t want = 0; // the parameters that take the depth-1 value to come or under way
  bool root_obj = false, invalid = false, defer = false, v_esc = false;
  const uint32_t np = f1 - f0;
  const auto close = [&]() {
    --depth, stack >>= 1;
    state = depth ? kRsAfter : kRsEnd;
  };
  // A wanted number ended in front of byte `end`.
  const auto number_ends = [&](uint32_t end) {
    uint64_t d = 0;
    const bool ok = args_number(body, v_off, end, pow, &d);
    for (uint32_t k = 0; k < np; ++k) {
      if (!((want >> k) & 1u)) continue;
      const uint32_t t = sc.type(f0 + k);
      uint64_t slot = d;
      if (!ok || (t == kArgI32 && !args_to_int(d, 31, &slot)) || (t == kArgI64 && !args_to_int(d, 63, &slot))) defer = true;
      else sink.put(k, slot);
    }
    want = 0;
  };
  for (uint32_t i = 0; i < len; ++i) {
    if ((state == kRsKeyStr || state == kRsStr) && body.aligned()) {
      while (len - i >= 4 && route_plain4(body.word())) {
        body.skip4();
        i += 4;
      }
      if (i >= len) break;
    }
    const uint32_t c = body.next();
    if (state == kRsKeyStr || state == kRsStr) {
      if (c == '"') {
        if (state == kRsKeyStr) {
          if (depth == 1 && root_obj) { // the first equal key wins, for every parameter of that name
            const uint32_t kl = i - key_at;
            want = 0;
            for (uint32_t k = 0; k < np; ++k) {
              if ((seen >> k) & 1u) continue;
              const uint32_t a = sc.name_off(f0 + k);
              if (sc.name_off(f0 + k + 1) - a != kl) continue;
              uint32_t j = 0;
              while (j < kl && body.at(key_at + j) == sc.name(a + j)) ++j;
              if (j == kl) seen |= 1u << k, want |= 1u << k;
            }
          }
          state = kRsColon;
        } else {
          if (depth == 1 && want) {
            for (uint32_t k = 0; k < np; ++k) {
              if (!((want >> k) & 1u)) continue;
              uint64_t slot = 0;
              if (sc.type(f0 + k) == kArgStr) {
                if (v_esc) defer = true;
                else sink.put(k, (uint64_t)(base + v_off + 1) | ((uint64_t)(i - v_off - 1) << 32));
              } else if (v_esc || !args_i64_string(body, v_off + 1, i, &slot)) {
                defer = true;
              } else {
                sink.put(k, slot);
              }
            }
            want = 0;
          }
          state = depth ? kRsAfter : kRsEnd;
        }
      } else if (c == '\\') {
        if (depth == 1 && root_obj && state == kRsKeyStr) return kArgsDefer; // rule 8
        v_esc = true;
        state = state == kRsKeyStr ? kRsKeyEsc : kRsStrEsc;
      } else if (c < 0x20) {
        return kArgsDefer;
      }
      continue;
    }
    if (state == kRsKeyEsc || state == kRsStrEsc) {
      if (!route_is_escape(c)) return kArgsDefer;
      state = state == kRsKeyEsc ? kRsKeyStr : kRsStr;
      continue;
    }
    if (state == kRsLit) {
      if (c != (lit & 0xFFu)) return kArgsDefer;
      lit >>= 8;
      if (!lit) state = depth ? kRsAfter : kRsEnd;
      continue;
    }
    if (state >= kRsNumMinus) {
      const bool d = route_is_digit(c);
      uint32_t next = kRsAfter;
      bool ok = true;
      switch (state) {
      case kRsNumMinus: ok = d, next = c == '0' ? kRsNumZero : kRsNumInt; break;
      case kRsNumZero:
        if (d) ok = false;
        else if (c == '.') next = kRsNumDot;
        else if (c == 'e' || c == 'E') next = kRsNumE;
        break;
      case kRsNumInt:
        if (d) next = kRsNumInt;
        else if (c == '.') next = kRsNumDot;
        else if (c == 'e' || c == 'E') next = kRsNumE;
        break;
      case kRsNumDot: ok = d, next = kRsNumFrac; break;
      case kRsNumFrac:
        if (d) next = kRsNumFrac;
        else if (c == 'e' || c == 'E') next = kRsNumE;
        break;
      case kRsNumE:
        if (c == '+' || c == '-') next = kRsNumESign;
        else ok = d, next = kRsNumExp;
        break;
      case kRsNumESign: ok = d, next = kRsNumExp; break;
      default:
        if (d) next = kRsNumExp;
        break;
      }
      if (!ok) return kArgsDefer;
      if (next != kRsAfter) {
        state = next;
        continue;
      }
      if (depth == 0) return kArgsDefer; // a byte behind a root number
      if (depth == 1 && want) number_ends(i);
      state = kRsAfter; // and c is looked at as what follows a value
    }
    // -- between tokens: no byte before or after the root value -------------------
    if (state == kRsEnd) return kArgsDefer;
    if (route_is_ws(c)) {
      if (state == kRsStart) return kArgsDefer;
      continue;
    }
    if (++tokens > kRouteMaxTokens) return kArgsDefer;
    switch (state) {
    case kRsObjFirst:
    case kRsObjKey:
      if (c == '"') {
        key_at = i + 1, state = kRsKeyStr;
      } else if (c == '}' && state == kRsObjFirst) {
        close();
      } else {
        return kArgsDefer;
      }
      break;
    case kRsColon:
      if (c != ':') return kArgsDefer;
      state = kRsValue;
      break;
    case kRsStart:
    case kRsValue:
    case kRsArrFirst:
      if (c == ']' && state == kRsArrFirst) {
        close();
        break;
      }
      if (state == kRsStart) root_obj = c == '{';
      if (depth == 1 && want) { // the value of a declared parameter begins: rule 9 on its first byte
        const bool is_num = c == '-' || route_is_digit(c), is_str = c == '"', is_bool = c == 't' || c == 'f';
        for (uint32_t k = 0; k < np; ++k) {
          if (!((want >> k) & 1u)) continue;
          const uint32_t t = sc.type(f0 + k);
          const bool takes = is_num ? t <= kArgF64 : is_str ? (t == kArgStr || t == kArgI64) : is_bool && t == kArgBool;
          if (!takes) invalid = true;
          else if (is_bool) sink.put(k, c == 't' ? 1u : 0u);
          if (!takes || is_bool) want &= ~(1u << k);
        }
        v_off = i, v_esc = false;
      }
      if (c == '{' || c == '[') {
        if (depth == kRouteMaxDepth - 1) return kArgsDefer;
        ++depth, stack = (stack << 1) | (c == '{' ? 1u : 0u);
        state = c == '{' ? kRsObjFirst : kRsArrFirst;
      } else if (c == '"') {
        state = kRsStr;
      } else if (c == '-') {
        state = kRsNumMinus;
      } else if (route_is_digit(c)) {
        state = c == '0' ? kRsNumZero : kRsNumInt;
      } else if (c == 't') {
        lit = 'r' | ('u' << 8) | ('e' << 16), state = kRsLit;
      } else if (c == 'f') {
        lit = 'a' | ('l' << 8) | ('s' << 16) | ((uint32_t)'e' << 24), state = kRsLit;
      } else if (c == 'n') {
        lit = 'u' | ('l' << 8) | ('l' << 16), state = kRsLit;
      } else {
        return kArgsDefer;
      }
      break;
    default: // kRsAfter
      if (c == ',') {
        state = (stack & 1u) ? kRsObjKey : kRsValue;
      } else if (c == ((stack & 1u) ? '}' : ']')) {
        close();
      } else {
        return kArgsDefer;
      }
      break;
    }
  }
  // (a root number ends with the span)
  const bool num_end = state == kRsNumZero || state == kRsNumInt || state == kRsNumFrac || state == kRsNumExp;
  if (!(state == kRsEnd || (depth == 0 && num_end))) return kArgsDefer;
  if (!root_obj) return kArgsInvalid;                      // rule 7
  if (invalid || seen != (1u << np) - 1u) return kArgsInvalid; // rule 9
  return defer ? kArgsDefer : kArgsOk;
}

// ---- the call (frames_args.hip; no workspace) -----------------------------------
struct ArgsArgs {
  const uint8_t *bodies = nullptr;
  uint64_t bodies_bytes = 0;
  const uint64_t *body_off = nullptr;
  const uint32_t *body_len = nullptr;
  const uint8_t *kind = nullptr;
  const uint16_t *method = nullptr;
  const uint32_t *params_off = nullptr, *params_len = nullptr;
  uint64_t n = 0;
  const uint32_t *param_first = nullptr; // nmethods + 1
  uint32_t nmethods = 0;
  const uint8_t *param_types = nullptr;     // nparams
  const uint32_t *param_name_off = nullptr; // nparams + 1
  uint32_t nparams = 0;
  const uint8_t *param_names = nullptr;
  uint32_t name_bytes = 0;
  uint32_t width = 0;
  // outputs (the caller's; all optional)
  uint64_t *slots = nullptr; // width x n, column-major
  uint8_t *status = nullptr;
  int32_t *reply_status = nullptr;
};
#if defined(__HIPCC__)
hipError_t launch_frames_args(const ArgsArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
