// rpc_amd/csrc/frames_resolve.h -- the frame resolve: the JSON-RPC reply
// envelope of each delivered body, matched to the caller's pending ids
// (rpc_frames_resolve_device).  What sits between a client's
// unpack and its completions: per body the reply's id, where `result` and
// `error` lie, and which of the caller's slots it answers.
//
// resolve_one() applies rules 3-7 of include/rpccrc.h to one body: the route's
// automaton (route_scan, frames_route.h) walks it with another key policy,
// ResolveKeys: `id`, `result` and `error` without regard to ASCII letter case,
// the two values as spans.  The caller applies rules 1 and 2 (resolve_precheck)
// before any byte is read.
//
// The join (rule 8) is an open-addressed table of slot indices: resolve_insert()
// puts a slot in with a compare-and-swap per probe, resolve_probe() walks an
// id's run and keeps the lowest slot that holds the id.  Linear probing without
// deletion keeps the slots of equal ids in one run without an empty cell, in
// whatever order they were inserted, so the probe's answer does not depend on
// that order.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_resolve.hip) and the CPU emulator (tests/cpu_emu/resolve_emu.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "frames_route.h"

namespace rpccrc {

// RPC_RESOLVE_* of include/rpccrc.h (the emulator builds without that header).
constexpr uint8_t kResolveNone = 0, kResolveMatched = 1, kResolveUnknown = 2, kResolveDuplicate = 3,
                  kResolveInvalid = 4, kResolveDefer = 5, kResolveRange = 6;
constexpr uint32_t kResolveNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kResolveMaxPending = 1u << 24;

struct ResolveOut {
  uint8_t kind; // from the walk: NONE, RANGE, DEFER, INVALID, or UNKNOWN for a decoded body (the join goes on)
  uint32_t id, result_off, result_len, error_off, error_len;
};
ROUTE_HD ResolveOut resolve_plain(uint8_t kind) { return ResolveOut{kind, 0, 0, 0, 0, 0}; }

// Rules 1 and 2, and rule 3's first line: is the body to be read?
ROUTE_HD bool resolve_precheck(bool has_type, uint32_t type, uint64_t off, uint32_t len, uint64_t bodies_bytes,
                               ResolveOut *out) {
  RouteOut o;
  if (route_precheck(has_type, type, off, len, bodies_bytes, &o)) return true;
  *out = resolve_plain(o.kind == kRouteNone ? kResolveNone : o.kind == kRouteRange ? kResolveRange : kResolveDefer);
  return false;
}

// A reply's keys: `id`, `result` (member 2, a span) and `error` (member 3),
// compared as cJSON_GetObjectItem compares: ASCII letters in either case.
// (c | 0x20 is a lower-case letter only for that letter's two cases.)
struct ResolveKeys {
  static constexpr bool kSpan2 = true;
  template <class Body> ROUTE_HD static uint32_t key(const Body &body, uint32_t key_at, uint32_t kl) {
    const uint32_t fold = 0x20202020u;
    if (kl == 2) {
      if ((body.at(key_at) | 0x20u) == 'i' && (body.at(key_at + 1) | 0x20u) == 'd') return 1;
    } else if (kl == 5 || kl == 6) {
      const uint32_t a = (body.at(key_at) | (body.at(key_at + 1) << 8) | (body.at(key_at + 2) << 16) |
                          (body.at(key_at + 3) << 24)) |
                         fold;
      if (kl == 6) {
        const uint32_t b = (body.at(key_at + 4) | (body.at(key_at + 5) << 8)) | (fold >> 16);
        if (a == 0x75736572u && b == 0x746Cu) return 2; // "resu" "lt"
      } else {
        if (a == 0x6F727265u && (body.at(key_at + 4) | 0x20u) == 'r') return 3; // "erro" "r"
      }
    }
    return 0;
  }
};

// Rules 3-7 for a body that resolve_precheck let through.
template <class Body> ROUTE_HD ResolveOut resolve_one(Body &body, uint32_t len) {
  const RouteScan s = route_scan(body, len, ResolveKeys());
  if (!s.strict) return resolve_plain(kResolveDefer); // (a signed or fractional id among them)
  if (!s.has_id) return resolve_plain(kResolveInvalid);
  if (s.id_big) return resolve_plain(kResolveDefer);
  return ResolveOut{kResolveUnknown, s.id, s.m_off, s.m_len, s.p_off, s.p_len};
}

// ---- the join (rule 8) --------------------------------------------------------
// The table has 2^bits cells, at least two per pending id; a cell holds a slot
// index or kResolveEmpty.
constexpr uint32_t kResolveEmpty = 0xFFFFFFFFu;
constexpr uint32_t kResolveHashMul = 2654435761u; // 2^32 / the golden ratio
ROUTE_HD uint32_t resolve_table_bits(uint32_t npending) {
  uint32_t bits = 1;
  while ((1ull << bits) < 2ull * npending) ++bits;
  return bits;
}
ROUTE_HD uint32_t resolve_hash(uint32_t id, uint32_t bits) { return (id * kResolveHashMul) >> (32u - bits); }

// Cas: uint32_t cas(uint32_t cell, uint32_t expect, uint32_t value), the cell's
// word before the exchange.  (Half of the cells stay empty: the walk ends.)
template <class Cas> ROUTE_HD void resolve_insert(Cas &cas, uint32_t slot, uint32_t id, uint32_t bits) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t h = resolve_hash(id, bits);
  while (cas(h, kResolveEmpty, slot) != kResolveEmpty) h = (h + 1u) & mask;
}
// Cells: uint32_t cell(uint32_t c); Ids: uint32_t id(uint32_t slot).  The
// lowest slot that holds `id`, or kResolveNoSlot.
template <class Cells, class Ids>
ROUTE_HD uint32_t resolve_probe(const Cells &cells, const Ids &ids, uint32_t id, uint32_t bits) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t best = kResolveNoSlot;
  for (uint32_t h = resolve_hash(id, bits);; h = (h + 1u) & mask) {
    const uint32_t s = cells.cell(h);
    if (s == kResolveEmpty) return best;
    if (s < best && ids.id(s) == id) best = s;
  }
}
// The finish pass's word on an entry that named `slot`: whose is the slot?
ROUTE_HD uint8_t resolve_final(uint32_t slot_entry, uint32_t entry) {
  return slot_entry == entry ? kResolveMatched : kResolveDuplicate;
}

// ---- the call (frames_resolve.hip) -------------------------------------------
struct ResolveArgs {
  const uint8_t *bodies = nullptr;
  uint64_t bodies_bytes = 0;
  const uint64_t *body_off = nullptr;
  const uint32_t *body_len = nullptr;
  const uint16_t *types = nullptr; // or nullptr: every entry is DATA
  uint64_t n = 0;
  const uint32_t *pending = nullptr;
  uint32_t npending = 0;
  // outputs (the caller's; all optional)
  uint8_t *kind = nullptr;
  uint32_t *id = nullptr, *result_off = nullptr, *result_len = nullptr, *error_off = nullptr, *error_len = nullptr;
  uint32_t *open = nullptr, *nopen = nullptr; // both or neither
  // the caller's or workspace: with npending > 0 both are there
  uint32_t *slot = nullptr;       // n
  uint32_t *slot_entry = nullptr; // npending
  // workspace
  uint32_t *cells = nullptr; // 2^bits (npending > 0)
  uint32_t bits = 0;
  uint64_t *flags = nullptr;    // npending: the slot is open (with open)
  uint64_t *offs = nullptr;     // npending + 1: the exclusive scan
  uint64_t *scan_tmp = nullptr; // scan_tmp_words(npending)
};
// The join's arrays in pool workspace, over a WsLayout (workspace.h) or anything
// with its take<T>(count), for a call with npending > 0.  Set: a.n, a.npending,
// a.bits, a.open, and a.slot / a.slot_entry where the caller gave them -- where
// it did not, workspace stands in (a measuring pass leaves them nullptr, so the
// carving pass over the same `a` takes the same arrays).
template <class Layout> inline void resolve_ws_layout(Layout &w, ResolveArgs &a, size_t tmp_words) {
  if (a.open) {
    a.flags = w.template take<uint64_t>(a.npending);
    a.offs = w.template take<uint64_t>((uint64_t)a.npending + 1);
    a.scan_tmp = w.template take<uint64_t>(tmp_words);
  }
  a.cells = w.template take<uint32_t>((uint64_t)1 << a.bits);
  if (!a.slot_entry) a.slot_entry = w.template take<uint32_t>(a.npending);
  if (!a.slot && a.n) a.slot = w.template take<uint32_t>(a.n);
}

#if defined(__HIPCC__)
// Table pass, resolve kernel, finish pass [-> exclusive scan -> compaction].
hipError_t launch_frames_resolve(const ResolveArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
