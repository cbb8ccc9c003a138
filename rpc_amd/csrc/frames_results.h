// rpc_amd/csrc/frames_results.h -- the frame results: the `result` and `error`
// members of each matched reply, decoded into one typed 64-bit value per
// pending slot (rpc_frames_results_device).  What sits between
// a client's resolve and its completions: the five result shapes of the
// reference's generated client stubs (client/gen/rpc_client_gen.c), for a whole
// batch, with the type chosen by the method the slot's request was sent with.
//
// results_precheck() applies rules 1-3 of include/rpccrc.h before any body byte
// is read.  results_walk() applies rules 4-7 and the error's rules to one staged
// body: the args' strict automaton (args_one, frames_args.h) walks the `result`
// span with an empty parameter list, which says strict or not strict and
// nothing else, and the `error` span with the fixed schema (code: I32, message:
// STR); the scalar of a strict `result` is then read again from the staged
// bytes with the args' conversions (args_number, args_to_int, args_i64_string).
// The two spans are walked by one loop, so that the automaton is there once.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_results.hip) and the CPU emulator (tests/cpu_emu/results_emu.cpp).
#pragma once
#include <stdint.h>

#include "frames_args.h"
#include "frames_resolve.h"

namespace rpccrc {

// RPC_RESULTS_* of include/rpccrc.h (the emulator builds without that header).
constexpr uint8_t kResultsNone = 0, kResultsOk = 1, kResultsAbsent = 2, kResultsMismatch = 3, kResultsDefer = 4,
                  kResultsRange = 5, kResultsBadSchema = 6;
constexpr uint8_t kResultsWalk = 0xFF; // results_precheck: rules 1-3 passed

// What one entry answers: the value and the error, each with its own status.
struct ResultsOut {
  uint8_t status, error_status;
  uint64_t value;
  int32_t error_code;
  uint64_t error_message;
};
ROUTE_HD ResultsOut results_plain(uint8_t status) { return ResultsOut{status, kResultsAbsent, 0, 0, 0}; }

// Rules 1-3.  Pending: uint32_t method(s), word s of the npending; Types:
// uint32_t type(m), byte m of the nmethods.  Each is read only after its index
// has been found inside its array.  Returns NONE, BAD_SCHEMA or RANGE, or
// kResultsWalk with the slot's declared type.
template <class Pending, class Types>
ROUTE_HD uint8_t results_precheck(uint8_t kind, uint32_t slot, const Pending &pm, uint32_t npending, const Types &ty,
                                  uint32_t nmethods, uint64_t body_off, uint32_t body_len, uint32_t r_off,
                                  uint32_t r_len, uint32_t e_off, uint32_t e_len, uint64_t bodies_bytes,
                                  uint32_t *type) {
  *type = 0;
  if (kind != kResolveMatched) return kResultsNone;
  if (slot >= npending) return kResultsBadSchema;
  const uint32_t m = pm.method(slot);
  if (m >= nmethods) return kResultsBadSchema;
  const uint32_t t = ty.type(m);
  if (t > kArgStr) return kResultsBadSchema;
  if (!(body_off <= bodies_bytes && body_len <= bodies_bytes - body_off)) return kResultsRange;
  if (r_len && !(r_off <= body_len && r_len <= body_len - r_off)) return kResultsRange;
  if (e_len && !(e_off <= body_len && e_len <= body_len - e_off)) return kResultsRange;
  *type = t;
  return kResultsWalk;
}

// What rules 4-7 and the error's rules say without a byte: an absent member, and
// a member of a body too long to stage (rule 5).  True when the body is to be
// staged and walked: at least one member is there.
ROUTE_HD bool results_unread(uint32_t body_len, uint32_t r_len, uint32_t e_len, ResultsOut *out) {
  const bool lng = body_len > kRouteMaxBody;
  *out = ResultsOut{r_len == 0 ? kResultsAbsent : kResultsDefer, e_len == 0 ? kResultsAbsent : kResultsDefer, 0, 0, 0};
  return !lng && (r_len != 0 || e_len != 0);
}

// The error's schema: {"code": I32, "message": STR}, and with no parameters
// (f0 == f1) the schema of the `result` walk.
struct ResultsErrorSchema {
  ROUTE_HD uint32_t type(uint32_t p) const { return p == 0 ? kArgI32 : kArgStr; }
  ROUTE_HD uint32_t name_off(uint32_t p) const { return p == 0 ? 0u : p == 1 ? 4u : 11u; }
  ROUTE_HD uint32_t name(uint32_t b) const { // "codemess" "age", low byte first
    return (uint32_t)((b < 8 ? 0x7373656D65646F63ull >> (8 * b) : 0x656761ull >> (8 * (b - 8))) & 0xFFu);
  }
};
struct ResultsErrorSink {
  uint64_t code = 0, message = 0;
  ROUTE_HD void put(uint32_t k, uint64_t v) {
    if (k == 0) code = v;
    else message = v;
  }
};

// Rules 6 and 7 for a span [0, len) that args_one found strict.  View: the
// span's bytes through at(i); base: the span's offset in the body.
template <class View, class Pow>
ROUTE_HD uint8_t results_convert(const View &v, uint32_t len, uint32_t base, uint32_t type, const Pow &pow,
                                 uint64_t *value) {
  *value = 0;
  const uint32_t c = v.at(0);
  const bool is_num = c == '-' || route_is_digit(c), is_str = c == '"', is_bool = c == 't' || c == 'f';
  const bool takes = is_num ? type <= kArgF64 : is_str ? (type == kArgStr || type == kArgI64) : is_bool && type == kArgBool;
  if (!takes) return kResultsMismatch;
  if (is_bool) {
    *value = c == 't' ? 1u : 0u;
    return kResultsOk;
  }
  uint64_t slot = 0;
  if (is_num) {
    if (!args_number(v, 0, len, pow, &slot)) return kResultsDefer;
    if ((type == kArgI32 && !args_to_int(slot, 31, &slot)) || (type == kArgI64 && !args_to_int(slot, 63, &slot)))
      return kResultsDefer;
  } else { // the bytes between the quotes: [1, len - 1)
    for (uint32_t i = 1; i + 1 < len; ++i)
      if (v.at(i) == '\\') return kResultsDefer;
    if (type == kArgStr) slot = (uint64_t)(base + 1) | ((uint64_t)(len - 2) << 32);
    else if (!args_i64_string(v, 1, len - 1, &slot)) return kResultsDefer;
  }
  *value = slot;
  return kResultsOk;
}

// Rules 4-7 and the error's rules for an entry that results_precheck and
// results_unread let through.  view(off): the staged body from byte `off` on,
// a Body of frames_route.h (next, aligned, word, skip4, at).
template <class MakeView, class Pow>
ROUTE_HD ResultsOut results_walk(const MakeView &view, uint32_t type, uint32_t r_off, uint32_t r_len, uint32_t e_off,
                                 uint32_t e_len, const Pow &pow) {
  ResultsOut o{kResultsAbsent, kResultsAbsent, 0, 0, 0};
  const ResultsErrorSchema sc;
  for (uint32_t pass = 0; pass < 2; ++pass) { // 0: `result`, 1: `error`
    const uint32_t off = pass ? e_off : r_off, len = pass ? e_len : r_len;
    if (len == 0) continue;
    ResultsErrorSink sink;
    auto body = view(off);
    const uint8_t st = args_one(body, len, off, sc, 0u, pass ? 2u : 0u, pow, sink);
    if (pass == 0) {
      // (with no parameters: OK for an object, INVALID for any other strict value)
      o.status = st == kArgsDefer ? kResultsDefer : results_convert(view(off), len, off, type, pow, &o.value);
    } else if (st == kArgsOk) {
      o.error_status = kResultsOk, o.error_code = (int32_t)(uint32_t)sink.code, o.error_message = sink.message;
    } else {
      o.error_status = st == kArgsInvalid ? kResultsMismatch : kResultsDefer;
    }
  }
  return o;
}

// The per-slot part: slot s is completed by entry e = slot_entry[s] if e < n,
// kind[e] is MATCHED and slot[e] == s -- at most one entry per slot, whatever
// the input, so the answer does not depend on any order.  Cols: uint32_t
// kind(e), uint32_t slot(e), read only for e < n.
template <class Cols> ROUTE_HD bool results_completes(uint32_t e, uint64_t n, const Cols &c, uint32_t s) {
  return e < n && c.kind(e) == kResolveMatched && c.slot(e) == s;
}

// ---- the call (frames_results.hip; no workspace) -----------------------------
struct ResultsArgs {
  const uint8_t *bodies = nullptr;
  uint64_t bodies_bytes = 0;
  const uint64_t *body_off = nullptr;
  const uint32_t *body_len = nullptr;
  const uint8_t *kind = nullptr;
  const uint32_t *slot = nullptr;
  const uint32_t *result_off = nullptr, *result_len = nullptr, *error_off = nullptr, *error_len = nullptr;
  const uint32_t *slot_entry = nullptr; // npending (with a per-slot output)
  uint64_t n = 0;
  const uint16_t *pending_method = nullptr; // npending
  uint32_t npending = 0;
  const uint8_t *result_types = nullptr; // nmethods
  uint32_t nmethods = 0;
  // outputs (the caller's; all optional): per entry
  uint8_t *status = nullptr;
  uint64_t *value = nullptr;
  uint8_t *error_status = nullptr;
  int32_t *error_code = nullptr;
  uint64_t *error_message = nullptr;
  // per slot
  uint8_t *slot_status = nullptr;
  uint64_t *slot_value = nullptr;
  uint8_t *slot_error_status = nullptr;
  int32_t *slot_error_code = nullptr;
  uint64_t *slot_str_base = nullptr;
  uint32_t *ndefer = nullptr;
};
#if defined(__HIPCC__)
hipError_t launch_frames_results(const ResultsArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
