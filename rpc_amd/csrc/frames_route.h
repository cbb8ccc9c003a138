// rpc_amd/csrc/frames_route.h -- the frame route: the JSON-RPC envelope of each
// delivered body, without a parse tree (rpc_frames_route_device; DESIGN.md
// 4.15).  What sits between the unpack and the handlers: per body the request's
// id, the index of its method in the server's table and where `params` lies;
// and the entries grouped by method.
//
// route_one() applies rules 3-8 of include/rpccrc.h to one body: a byte
// automaton (a state word, a 32-bit object/array stack, a token counter) walks
// the body once, front to back, records the first depth-1 `id`, `method` and
// `params` on the way and leaves on the first violation of the strict subset;
// route_method() then compares the method's raw bytes with the table.  Nothing
// is converted but a digits-only id.  The caller applies rules 1 and 2
// (route_precheck) before any byte is read.
// Which depth-1 keys the walk records is a key policy (RouteKeys here; the frame
// resolve walks replies with its own, frames_resolve.h).
//
// The grouping is a stable counting sort over buckets: route_bucket() names an
// entry's bucket, route_wave_rank() is the rank inside one wave as the kernel
// takes it from ballots.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_route.hip) and the CPU emulator (tests/cpu_emu/route_emu.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROUTE_HD __host__ __device__ __forceinline__
#else
#define ROUTE_HD inline
#endif

namespace rpccrc {

// RPC_ROUTE_* of include/rpccrc.h (the emulator builds without that header).
constexpr uint8_t kRouteNone = 0, kRouteCall = 1, kRouteNotFound = 2, kRouteInvalid = 3, kRouteDefer = 4,
                  kRouteRange = 5;
constexpr uint16_t kRouteNoMethod = 0xFFFF;
constexpr uint32_t kRouteMaxBody = 1024, kRouteMaxDepth = 32, kRouteMaxTokens = 256;
constexpr uint32_t kRouteMaxMethods = 256, kRouteMaxMethodBytes = 4096;
constexpr uint32_t kRouteTypeData = 0; // RPC_FRAME_TYPE_DATA
// Entries per workgroup (one lane each) and the bytes of bodies a workgroup
// stages in LDS per round.
constexpr uint32_t kRouteEntries = 256;
constexpr uint32_t kRouteStage = 32768;
static_assert(kRouteStage % 16 == 0 && kRouteStage >= kRouteMaxBody + 32, "a round holds any one body at any alignment");

struct RouteOut {
  uint8_t kind;
  uint16_t method;
  uint32_t id, params_off, params_len;
};
ROUTE_HD RouteOut route_plain(uint8_t kind) { return RouteOut{kind, kRouteNoMethod, 0, 0, 0}; }

// Rules 1 and 2: is the body to be read?  (*out is set when it is not.)
ROUTE_HD bool route_precheck(bool has_type, uint32_t type, uint64_t off, uint32_t len, uint64_t bodies_bytes,
                             RouteOut *out) {
  if (has_type && type != kRouteTypeData) {
    *out = route_plain(kRouteNone);
    return false;
  }
  if (!(off <= bodies_bytes && len <= bodies_bytes - off)) {
    *out = route_plain(kRouteRange);
    return false;
  }
  if (len == 0 || len > kRouteMaxBody) { // (rule 3's first line: nothing to walk)
    *out = route_plain(kRouteDefer);
    return false;
  }
  return true;
}

// ---- the strict automaton ---------------------------------------------------
enum RouteState : uint32_t {
  kRsStart,    // before the root '{'
  kRsObjFirst, // after '{': a key or '}'
  kRsObjKey,   // after ',' in an object: a key
  kRsColon,    // after a key
  kRsValue,    // after ':' or after ',' in an array: a value
  kRsArrFirst, // after '[': a value or ']'
  kRsAfter,    // after a value: ',' or the container's closer
  kRsEnd,      // after the root '}'
  kRsKeyStr,   // inside a key
  kRsKeyEsc,
  kRsStr, // inside a string value
  kRsStrEsc,
  kRsLit,     // inside true / false / null
  kRsNumMinus, // after '-': a digit
  kRsNumZero,  // after a leading 0
  kRsNumInt,
  kRsNumDot, // after '.': a digit
  kRsNumFrac,
  kRsNumE,     // after e / E: a sign or a digit
  kRsNumESign, // after the exponent's sign: a digit
  kRsNumExp,
};
ROUTE_HD bool route_is_ws(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
ROUTE_HD bool route_is_digit(uint32_t c) { return c - '0' < 10u; }
ROUTE_HD bool route_is_escape(uint32_t c) {
  return c == '"' || c == '\\' || c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't';
}

// Are the four bytes of x all plain string bytes: >= 0x20, not '"', not a
// backslash?  (The two classic any-byte tests: a borrow can only flag a byte
// above one that is flagged rightly, so as yes / no answers they are exact.)
ROUTE_HD bool route_plain4(uint32_t x) {
  const uint32_t ones = 0x01010101u, high = 0x80808080u;
  const uint32_t q = x ^ (ones * '"'), b = x ^ (ones * '\\');
  const uint32_t below = (x - ones * 0x20u) & ~x & high;
  return ((below | ((q - ones) & ~q & high) | ((b - ones) & ~b & high))) == 0;
}

// What the walk recorded about the first depth-1 members 1, 2 and 3 of its key
// policy (a request's `id`, `method` and `params`: RouteKeys below).
struct RouteScan {
  bool strict;          // rules 3 and 4 hold, and rule 5 does not defer
  bool id_big;          // a digits-only id above 4294967295
  bool has_id;          // the first `id` is a number written as digits only
  bool has_method;      // the first `method` is a string (kSpan2: member 2 is there)
  bool m_esc;           // ... with a backslash in it
  uint32_t id;          // rule 5 (0 when id_big)
  uint32_t m_off, m_len; // the method's raw bytes (kSpan2: member 2's value, as p_off / p_len)
  uint32_t p_off, p_len; // rule 8
};

// The key policy of a walk: key() names a depth-1 key of kl bytes at key_at as
// member 1 (the id), 2, 3 or 0 (none); only the lengths it looks at cost a
// compare.  Member 3's value is recorded as a span.  Member 2 is a string
// whose raw bytes are recorded for a later compare, or with kSpan2 a second
// span.  This one is a request's: `id`, `method`, `params`, compared exactly.
struct RouteKeys {
  static constexpr bool kSpan2 = false;
  template <class Body> ROUTE_HD static uint32_t key(const Body &body, uint32_t key_at, uint32_t kl) {
    if (kl == 2) {
      if (body.at(key_at) == 'i' && body.at(key_at + 1) == 'd') return 1;
    } else if (kl == 6) {
      const uint32_t a = body.at(key_at) | (body.at(key_at + 1) << 8) | (body.at(key_at + 2) << 16) |
                         (body.at(key_at + 3) << 24);
      const uint32_t b = body.at(key_at + 4) | (body.at(key_at + 5) << 8);
      if (a == 0x6874656Du && b == 0x646Fu) return 2; // "meth" "od"
      if (a == 0x61726170u && b == 0x736Du) return 3; // "para" "ms"
    }
    return 0;
  }
};

// Body: uint32_t next(), the body's bytes in order; bool aligned(), does the
// next byte start a word of the staging area; uint32_t word(), that word (asked
// only when aligned() and four bytes of the body are left); skip4(), step over
// it; uint32_t at(uint32_t i), byte i again (i below the bytes handed out; used
// for the few bytes of a depth-1 key of a length the policy looks at and for
// the compare).
template <class Body, class Keys = RouteKeys> ROUTE_HD RouteScan route_scan(Body &body, uint32_t len, Keys = Keys()) {
  RouteScan r{false, false, false, false, false, 0, 0, 0, 0, 0};
  uint32_t state = kRsStart, depth = 0, stack = 0, tokens = 0, lit = 0;
  uint32_t key_at = 0;
  uint32_t seen = 0; // bit 0 member 1, 1 member 2, 2 member 3: the key has occurred at depth 1
  uint32_t want = 0; // the depth-1 value to come or under way: member 1, 2 or 3
  bool id_num = false;
  // A container closes at byte i: back to its parent, and a depth-1 value ends.
  const auto close = [&](uint32_t i) {
    --depth, stack >>= 1;
    if (depth == 1 && want == 3) r.p_len = i + 1 - r.p_off;
    if (Keys::kSpan2 && depth == 1 && want == 2) r.m_len = i + 1 - r.m_off;
    if (depth == 1) want = 0;
    state = depth ? kRsAfter : kRsEnd;
  };
  for (uint32_t i = 0; i < len; ++i) {
    // -- inside a string: plain bytes, four at a time ---------------------------
    // (most bytes of a long body are string contents: a lane whose next byte
    // starts a word steps over whole words of plain bytes in a loop of its own,
    // which costs a fraction of a trip through the automaton below)
    if ((state == kRsKeyStr || state == kRsStr) && body.aligned()) {
      while (len - i >= 4 && route_plain4(body.word())) {
        body.skip4();
        i += 4;
      }
      if (i >= len) break; // the body ends inside the string
    }
    const uint32_t c = body.next();
    // -- inside a token ------------------------------------------------------
    if (state == kRsKeyStr || state == kRsStr) {
      if (c == '"') {
        if (state == kRsKeyStr) {
          if (depth == 1) {
            const uint32_t kl = i - key_at;
            const uint32_t k = Keys::key(body, key_at, kl);
            want = 0;
            if (k && !((seen >> (k - 1)) & 1u)) { // the first wins
              seen |= 1u << (k - 1);
              want = k;
            }
          }
          state = kRsColon;
        } else {
          if (depth == 1) {
            if (want == 2) r.m_len = (Keys::kSpan2 ? i + 1 : i) - r.m_off;
            if (want == 3) r.p_len = i + 1 - r.p_off;
            want = 0;
          }
          state = kRsAfter;
        }
      } else if (c == '\\') {
        if (depth == 1 && state == kRsKeyStr) return r; // rule 4
        // (rule 6 defers a method with a backslash, but after rule 5 has had its say)
        if (!Keys::kSpan2 && depth == 1 && want == 2) r.m_esc = true;
        state = state == kRsKeyStr ? kRsKeyEsc : kRsStrEsc;
      } else if (c < 0x20) {
        return r;
      }
      continue;
    }
    if (state == kRsKeyEsc || state == kRsStrEsc) {
      if (!route_is_escape(c)) return r; // (\u among them)
      state = state == kRsKeyEsc ? kRsKeyStr : kRsStr;
      continue;
    }
    if (state == kRsLit) {
      if (c != (lit & 0xFFu)) return r;
      lit >>= 8;
      if (!lit) {
        if (depth == 1) {
          if (want == 3) r.p_len = i + 1 - r.p_off;
          if (Keys::kSpan2 && want == 2) r.m_len = i + 1 - r.m_off;
          want = 0;
        }
        state = kRsAfter;
      }
      continue;
    }
    if (state >= kRsNumMinus) {
      const bool d = route_is_digit(c);
      uint32_t next = kRsAfter; // the number ends in front of c
      bool ok = true;
      switch (state) {
      case kRsNumMinus: ok = d, next = c == '0' ? kRsNumZero : kRsNumInt; break;
      case kRsNumZero:
        if (d) ok = false; // a leading zero
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
      default: // kRsNumExp
        if (d) next = kRsNumExp;
        break;
      }
      if (!ok) return r;
      if (next != kRsAfter) {
        if (id_num) {
          if (!d) return r; // rule 5: a fraction or an exponent
          const uint32_t v = c - '0';
          if (r.id > 429496729u || (r.id == 429496729u && v > 5u)) r.id_big = true;
          r.id = r.id * 10u + v; // (meaningless once id_big: cleared below)
        }
        state = next;
        continue;
      }
      if (depth == 1) {
        if (want == 3) r.p_len = i - r.p_off;
        if (Keys::kSpan2 && want == 2) r.m_len = i - r.m_off;
        want = 0;
      }
      id_num = false;
      state = kRsAfter; // and c is looked at as what follows a value
    }
    // -- between tokens ------------------------------------------------------
    if (route_is_ws(c)) continue;
    if (++tokens > kRouteMaxTokens) return r;
    switch (state) {
    case kRsStart:
      if (c != '{') return r;
      depth = 1, stack = 1, state = kRsObjFirst;
      break;
    case kRsObjFirst:
    case kRsObjKey:
      if (c == '"') {
        key_at = i + 1, state = kRsKeyStr;
      } else if (c == '}' && state == kRsObjFirst) {
        close(i);
      } else {
        return r;
      }
      break;
    case kRsColon:
      if (c != ':') return r;
      state = kRsValue;
      break;
    case kRsValue:
    case kRsArrFirst:
      if (c == ']' && state == kRsArrFirst) {
        close(i); // (an array is never the root: depth stays >= 1)
        break;
      }
      if (depth == 1) { // the value of a depth-1 key begins
        if (want == 3) r.p_off = i;
        if (want == 2) {
          if (Keys::kSpan2) r.has_method = true, r.m_off = i;
          else if (c == '"') r.has_method = true, r.m_off = i + 1;
          else want = 0;
        }
        if (want == 1) {
          if (c == '-') return r; // rule 5: a sign (a lone '-' is not strict either)
          id_num = r.has_id = route_is_digit(c);
          want = 0;
        }
      }
      if (c == '{' || c == '[') {
        if (depth == kRouteMaxDepth) return r;
        ++depth, stack = (stack << 1) | (c == '{' ? 1u : 0u);
        state = c == '{' ? kRsObjFirst : kRsArrFirst;
      } else if (c == '"') {
        state = kRsStr;
      } else if (c == '-') {
        state = kRsNumMinus;
      } else if (route_is_digit(c)) {
        if (id_num) r.id = c - '0';
        state = c == '0' ? kRsNumZero : kRsNumInt;
      } else if (c == 't') {
        lit = 'r' | ('u' << 8) | ('e' << 16), state = kRsLit;
      } else if (c == 'f') {
        lit = 'a' | ('l' << 8) | ('s' << 16) | ((uint32_t)'e' << 24), state = kRsLit;
      } else if (c == 'n') {
        lit = 'u' | ('l' << 8) | ('l' << 16), state = kRsLit;
      } else {
        return r;
      }
      break;
    case kRsAfter:
      if (c == ',') {
        state = (stack & 1u) ? kRsObjKey : kRsValue;
      } else if (c == ((stack & 1u) ? '}' : ']')) {
        close(i);
      } else {
        return r;
      }
      break;
    default: // kRsEnd: anything but whitespace behind the root
      return r;
    }
  }
  if (state != kRsEnd) return r;
  if (r.id_big) r.id = 0;
  r.strict = true;
  return r;
}

// ---- the method compare (rule 7) ----------------------------------------------
// Tab: uint32_t off(uint32_t m), word m of the nmethods + 1 offsets; uint32_t
// name(uint32_t p), byte p of the names (asked only for p < method_bytes).
// By length first, then by bytes.
template <class Body, class Tab>
ROUTE_HD uint16_t route_method(Body &body, uint32_t m_off, uint32_t m_len, const Tab &tab, uint32_t nmethods,
                               uint32_t method_bytes) {
  for (uint32_t m = 0; m < nmethods; ++m) {
    const uint32_t a = tab.off(m), b = tab.off(m + 1);
    if (a > b || b > method_bytes || b - a != m_len) continue; // (a broken word: the name matches nothing)
    uint32_t j = 0;
    while (j < m_len && body.at(m_off + j) == tab.name(a + j)) ++j;
    if (j == m_len) return (uint16_t)m;
  }
  return kRouteNoMethod;
}

// Rules 3-8 for a body that route_precheck let through.
template <class Body, class Tab>
ROUTE_HD RouteOut route_one(Body &body, uint32_t len, const Tab &tab, uint32_t nmethods, uint32_t method_bytes) {
  const RouteScan s = route_scan(body, len);
  if (!s.strict) return route_plain(kRouteDefer);
  if (s.id_big) return route_plain(kRouteInvalid); // rpc_server_skeleton.c:131-135
  if (!s.has_method) return RouteOut{kRouteInvalid, kRouteNoMethod, s.id, 0, 0};
  if (s.m_esc) return route_plain(kRouteDefer);
  const uint16_t m = route_method(body, s.m_off, s.m_len, tab, nmethods, method_bytes);
  if (m == kRouteNoMethod) return RouteOut{kRouteNotFound, kRouteNoMethod, s.id, 0, 0};
  return RouteOut{kRouteCall, m, s.id, s.p_off, s.p_len};
}

// ---- groups ---------------------------------------------------------------------
// CALL by method index, then NOT_FOUND, INVALID, DEFER; NONE and RANGE are in
// no group.
constexpr uint32_t kRouteNoBucket = 0xFFFFu;
ROUTE_HD uint32_t route_buckets(uint32_t nmethods) { return nmethods + 3; }
ROUTE_HD uint32_t route_bucket(uint8_t kind, uint16_t method, uint32_t nmethods) {
  if (kind == kRouteCall) return method;
  if (kind == kRouteNotFound) return nmethods;
  if (kind == kRouteInvalid) return nmethods + 1;
  if (kind == kRouteDefer) return nmethods + 2;
  return kRouteNoBucket;
}
// A lane's rank among the lanes of its wave with its bucket, and that count,
// from the ballot of those lanes.
ROUTE_HD uint32_t route_popc64(uint64_t x) {
  uint32_t n = 0;
  for (; x; x &= x - 1) ++n;
  return n;
}
ROUTE_HD uint32_t route_wave_rank(uint64_t same, uint32_t lane) { return route_popc64(same & ((1ull << lane) - 1ull)); }

// ---- the call (frames_route.hip) ---------------------------------------------
struct RouteArgs {
  const uint8_t *bodies = nullptr;
  uint64_t bodies_bytes = 0;
  const uint64_t *body_off = nullptr;
  const uint32_t *body_len = nullptr;
  const uint16_t *types = nullptr; // or nullptr: every entry is DATA
  uint64_t n = 0;
  const uint8_t *names = nullptr;
  uint32_t method_bytes = 0;
  const uint32_t *method_off = nullptr; // nmethods + 1
  uint32_t nmethods = 0;
  // outputs (the caller's; all optional)
  uint8_t *kind = nullptr;
  uint16_t *method = nullptr;
  uint32_t *id = nullptr, *params_off = nullptr, *params_len = nullptr;
  uint32_t *order = nullptr, *group_first = nullptr; // both or neither
  // workspace (with order only)
  uint16_t *bucket = nullptr;   // n
  uint64_t *counts = nullptr;   // buckets x workgroups, bucket-major
  uint64_t *offs = nullptr;     // the same + 1: the exclusive scan
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(buckets x workgroups)
};
inline uint64_t route_workgroups(uint64_t n) { return (n + kRouteEntries - 1) / kRouteEntries; }
inline uint64_t route_cells(const RouteArgs &a) { return (uint64_t)route_buckets(a.nmethods) * route_workgroups(a.n); }
// The grouping passes' arrays in pool workspace, over a WsLayout (workspace.h)
// or anything with its take<T>(count); a.n and a.nmethods are set.
template <class Layout> inline void route_ws_layout(Layout &w, RouteArgs &a, size_t tmp_words) {
  a.counts = w.template take<uint64_t>(route_cells(a));
  a.offs = w.template take<uint64_t>(route_cells(a) + 1);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  a.bucket = w.template take<uint16_t>(a.n);
}

#if defined(__HIPCC__)
// The route kernel, then (with a.order) count, exclusive scan, scatter.
hipError_t launch_frames_route(const RouteArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
