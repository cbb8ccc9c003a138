// rpc_amd/csrc/frames_request.h -- the frame request: JSON-RPC request bodies
// built from a method index, the caller's params text and an id
// (rpc_frames_request_device).  The reply's mirror image: what
// sits in front of a client's pack.
//
// Entry i is a method index into the route's table, an id and a value
// [off, off + len) of the params buffer.  request_size_one() applies rules 1-5
// of include/rpccrc.h; the exclusive scan of the sizes is the layout.  Every
// entry is again generated front . copied middle . generated suffix:
//
//   call           {"jsonrpc":"2.0","method":"<name>","params":  . value .  ,"id":<id>}
//   bare call      {"jsonrpc":"2.0","method":"<name>","id":<id>}     (all front)
//   raw            value
//
// (client/rpc_codec.c:6-20 through cJSON_PrintUnformatted).  The name counts as
// generated: its bytes come from the method table (the kernel's copy in LDS), so
// the copied middle stays single and the reply's machinery, the splice
// (frames_splice.h), serves unchanged -- tiles aligned to the output's address,
// whole 16-byte pieces, the value bytes through two aligned blocks and the
// funnel; splice_piece() resolves one piece over RequestSplice, the request's
// policy.
// A front can be 27 + 4096 + 11 bytes, so the per-entry word is 32 bits wide:
// form, the suffix's length (it depends on the id's digits) and the front's.
// The fixed texts are immediates picked by selects and the digits are BCD
// (splice_bcd and its kin).
//
// Plain inline code with no HIP types, shared by the kernels
// (frames_request.hip) and the CPU emulator (tests/cpu_emu/request_emu.cpp).
#pragma once
#include "frames_splice.h"

namespace rpccrc {

// Request states, the method limits and the data type as include/rpccrc.h has them.
constexpr uint8_t kRequestNone = 0, kRequestCall = 1, kRequestRaw = 2, kRequestBadMethod = 3, kRequestRange = 4,
                  kRequestNoRoom = 5;
constexpr uint32_t kRequestNoMethod = 0xFFFFu; // RPC_ROUTE_NO_METHOD
constexpr uint32_t kRequestMaxMethods = 256, kRequestMaxMethodBytes = 4096;
constexpr uint32_t kRequestTypeData = 0; // RPC_FRAME_TYPE_DATA

// ---- forms -------------------------------------------------------------------
constexpr uint32_t kReqFormNone = 0, // size 0
    kReqFormValue = 1,               // front . value . ,"id":<id>}
    kReqFormBare = 2,                // no params: all generated
    kReqFormRaw = 3,                 // value
    kReqFormBad = 4,                 // size 0, RPC_REQUEST_BAD_METHOD
    kReqFormRange = 5;               // size 0, RPC_REQUEST_RANGE

// The fixed texts.  Behind the name both forms go on with `"`; then `,"params":`
// and the value, or at once `,"id":`.
constexpr char kReqHeadText[] = "{\"jsonrpc\":\"2.0\",\"method\":\"";
constexpr char kReqParamsText[] = ",\"params\":";
constexpr char kReqIdText[] = ",\"id\":";
constexpr uint32_t kReqHeadN = sizeof(kReqHeadText) - 1, kReqParamsN = sizeof(kReqParamsText) - 1,
                   kReqIdN = sizeof(kReqIdText) - 1;
static_assert(kReqHeadN == 27 && kReqParamsN == 10 && kReqIdN == 6, "the sizes of include/rpccrc.h: 45 and 35");
constexpr uint64_t kReqHead0 = splice_lit8(kReqHeadText, kReqHeadN, 0),
                   kReqHead1 = splice_lit8(kReqHeadText, kReqHeadN, 1),
                   kReqHead2 = splice_lit8(kReqHeadText, kReqHeadN, 2),
                   kReqHead3 = splice_lit8(kReqHeadText, kReqHeadN, 3);
constexpr uint64_t kReqParams0 = splice_lit8(kReqParamsText, kReqParamsN, 0),
                   kReqParams1 = splice_lit8(kReqParamsText, kReqParamsN, 1);
constexpr uint64_t kReqId0 = splice_lit8(kReqIdText, kReqIdN, 0);
PACK_HD uint32_t request_head_byte(uint32_t i) { // i < 27
  return i < 24 ? splice_text_byte(kReqHead0, kReqHead1, kReqHead2, i)
                : (uint32_t)(kReqHead3 >> (8 * (i & 7u))) & 0xFFu;
}

// ---- the method table (rule 3) --------------------------------------------------
// Tab: uint32_t off(uint32_t m), word m of the nmethods + 1 offsets; uint32_t
// name(uint32_t p), byte p of the names (asked only for p < method_bytes): the
// route's.  What the table pass keeps of name m: its length, or kRequestBadName
// for a word that is not monotone or leaves method_bytes (the route's rule 7:
// such a name matches nothing there) and for a name with a byte the reference
// would print as an escape.
constexpr uint32_t kRequestBadName = 0xFFFFFFFFu;
template <class Tab> PACK_HD uint32_t request_name_word(const Tab &tab, uint32_t m, uint32_t method_bytes) {
  const uint32_t a = tab.off(m), b = tab.off(m + 1);
  if (a > b || b > method_bytes) return kRequestBadName;
  for (uint32_t p = a; p < b; ++p) {
    const uint32_t c = tab.name(p);
    if (c < 0x20u || c == '"' || c == '\\') return kRequestBadName; // (bytes >= 0x80 go out as they are)
  }
  return b - a;
}

// ---- sizing rule -----------------------------------------------------------
// The per-entry word: form, the bytes generated behind the copied ones, the
// bytes generated in front (for the bare form: the whole entry).
constexpr uint32_t kRequestMaxSuf = kReqIdN + 10 + 1;                                // 17
constexpr uint32_t kRequestMaxPre = kReqHeadN + kRequestMaxMethodBytes + 1 + kReqIdN + 10 + 1; // 4141, the bare form
static_assert(kRequestMaxSuf < 32 && kRequestMaxPre < (1u << 24), "five and twenty-four bits of the meta word");
PACK_HD uint32_t request_meta(uint32_t form, uint32_t suf, uint32_t pre) { return form | (suf << 3) | (pre << 8); }
PACK_HD uint32_t request_form(uint32_t m) { return m & 7u; }
PACK_HD uint32_t request_suf(uint32_t m) { return (m >> 3) & 31u; }
PACK_HD uint32_t request_pre(uint32_t m) { return m >> 8; }
PACK_HD uint8_t request_status_of(uint32_t form) {
  return form == kReqFormValue || form == kReqFormBare ? kRequestCall
         : form == kReqFormRaw                         ? kRequestRaw
         : form == kReqFormBad                         ? kRequestBadMethod
         : form == kReqFormRange                       ? kRequestRange
                                                       : kRequestNone;
}

struct RequestSize {
  uint64_t size; // bytes of the output
  uint64_t src;  // params offset of the copied bytes (0 when none)
  uint32_t meta;
};
// Rules 1-5, in that order.  In: the entry's inputs, each asked for only when
// the rules look at it:
//   uint32_t method(), id();  uint64_t poff();  uint32_t plen()
// Names: uint32_t word(uint32_t m), request_name_word of name m < nmethods.
template <class In, class Names>
PACK_HD RequestSize request_size_one(const In &in, const Names &names, bool typed, uint32_t type, uint32_t nmethods,
                                     uint64_t params_bytes) {
  const RequestSize none{0, 0, request_meta(kReqFormNone, 0, 0)};
  if (typed && type != kRequestTypeData) return none;
  const uint32_t m = in.method();
  const bool raw = m == kRequestNoMethod;
  uint32_t nlen = 0;
  if (!raw) { // rule 3
    if (m >= nmethods) return RequestSize{0, 0, request_meta(kReqFormBad, 0, 0)};
    nlen = names.word(m);
    if (nlen == kRequestBadName) return RequestSize{0, 0, request_meta(kReqFormBad, 0, 0)};
  }
  const uint64_t off = in.poff(); // rule 4: the value, before anything is made of it
  const uint32_t len = in.plen();
  if (!(off <= params_bytes && len <= params_bytes - off)) return RequestSize{0, 0, request_meta(kReqFormRange, 0, 0)};
  if (raw) return len ? RequestSize{len, off, request_meta(kReqFormRaw, 0, 0)} : none;
  const uint32_t idn = splice_ndigits(in.id());
  if (len != 0) {
    const uint32_t pre = kReqHeadN + nlen + 1 + kReqParamsN, suf = kReqIdN + idn + 1;
    const uint64_t size = (uint64_t)pre + len + suf;
    if (size > 0xFFFFFFFFull) return RequestSize{0, 0, request_meta(kReqFormRange, 0, 0)}; // (a body length is 32 bits)
    return RequestSize{size, off, request_meta(kReqFormValue, suf, pre)};
  }
  const uint32_t all = kReqHeadN + nlen + 1 + kReqIdN + idn + 1;
  return RequestSize{all, 0, request_meta(kReqFormBare, 0, all)};
}
// An entry that does not end inside out_cap is not written (the pack's rule).
PACK_HD uint8_t request_final_status(uint32_t meta, uint64_t at, uint64_t size, uint64_t out_cap) {
  return (size != 0 && !pack_fits(at, size, out_cap)) ? kRequestNoRoom : request_status_of(request_form(meta));
}
// The pack's `types` entry: what rule 1 passes through, DATA for a written
// entry, NONE for everything else.
PACK_HD uint16_t request_type_out(bool typed, uint32_t type, uint8_t final_status) {
  if (typed && type != kRequestTypeData) return (uint16_t)type;
  return final_status == kRequestCall || final_status == kRequestRaw ? (uint16_t)kRequestTypeData
                                                                     : (uint16_t)kPackTypeNone;
}

// ---- generated bytes -----------------------------------------------------------
struct RequestGen {
  uint32_t noff, nlen; // the name in the table
  bool value;          // `,"params":` follows the name
  uint32_t idn;        // characters of the id
  uint64_t idd;        // splice_bcd of it
};
template <class Tab> PACK_HD RequestGen request_gen(uint32_t meta, uint32_t method, uint32_t id, const Tab &tab) {
  const uint32_t a = tab.off(method);
  return RequestGen{a, tab.off(method + 1) - a, request_form(meta) == kReqFormValue, splice_ndigits(id), splice_bcd(id)};
}
// Generated byte g of a call: the bytes in front of the copied ones and the
// bytes behind them, counted through.
template <class Tab> PACK_HD uint32_t request_gen_byte(const RequestGen &t, const Tab &tab, uint32_t g) {
  if (g < kReqHeadN) return request_head_byte(g);
  g -= kReqHeadN;
  if (g < t.nlen) return tab.name(t.noff + g);
  g -= t.nlen;
  if (g == 0) return '"';
  g -= 1;
  if (t.value) {
    if (g < kReqParamsN) return splice_text_byte(kReqParams0, kReqParams1, 0, g);
    g -= kReqParamsN;
  }
  if (g < kReqIdN) return splice_text_byte(kReqId0, 0, 0, g);
  g -= kReqIdN;
  if (g < t.idn) return splice_digit(t.idd, t.idn, g);
  return '}';
}

// ---- the splice policy -------------------------------------------------------
// The request under splice_piece() (frames_splice.h).  Ent: the entries.
//   uint32_t meta(e), method(e), id(e)   (method and id: asked for only when a byte is generated)
// Tab: the method table, as above; Src: the params.  An entry is written when it
// ends inside out_cap.
template <class Ent, class Tab, class Src> struct RequestSplice {
  const Ent &ent;
  const Tab &tab;
  const Src &params;
  uint64_t out_cap;
  struct Gen {
    RequestGen t;
    const Tab &tab;
    PACK_HD uint32_t byte(uint32_t g) const { return request_gen_byte(t, tab, g); }
  };
  PACK_HD bool written(uint64_t, uint64_t fe) const { return fe <= out_cap; }
  PACK_HD uint32_t meta(uint64_t e) const { return ent.meta(e); }
  PACK_HD uint32_t pre(uint32_t m) const { return request_pre(m); }
  PACK_HD uint32_t suf(uint32_t m) const { return request_suf(m); }
  PACK_HD Gen gen(uint64_t e, uint32_t m) const { return Gen{request_gen(m, ent.method(e), ent.id(e), tab), tab}; }
  PACK_HD const Src &src(uint32_t) const { return params; }
};
// One piece of the request from its readers: splice_piece() over the policy.
// SrcOf, the piece and [lo, hi] as there.
template <class Off, class Ent, class Tab, class SrcOf, class Src>
PACK_HD PackPiece request_piece(const Off &off, const Ent &ent, const Tab &tab, const SrcOf &src_of, const Src &src,
                                uint64_t lo, uint64_t hi, uint64_t x0, uint64_t x1, uint32_t b0, uint64_t out_cap) {
  return splice_piece(RequestSplice<Ent, Tab, Src>{ent, tab, src, out_cap}, off, src_of, lo, hi, x0, x1, b0);
}

// ---- the call (frames_request.hip) ---------------------------------------------
struct RequestArgs {
  const uint16_t *method = nullptr;
  const uint32_t *id = nullptr;
  const uint16_t *types = nullptr; // nullptr: DATA for all
  uint64_t n = 0;
  const uint8_t *names = nullptr;
  uint32_t method_bytes = 0;
  const uint32_t *method_off = nullptr; // nmethods + 1
  uint32_t nmethods = 0;
  const uint8_t *params = nullptr;
  uint64_t params_bytes = 0;
  const uint64_t *params_off = nullptr;
  const uint32_t *params_len = nullptr;
  const uint64_t *conn_first = nullptr; // nconn + 1, or nullptr
  uint64_t nconn = 0;
  // outputs (the caller's; all but out optional)
  uint8_t *out = nullptr;
  uint64_t out_cap = 0;
  uint64_t *body_off = nullptr;
  uint32_t *body_len = nullptr;
  uint16_t *types_out = nullptr; // may be types
  uint8_t *request_status = nullptr;
  uint64_t *conn_bytes_first = nullptr;
  uint64_t *total = nullptr;
  // workspace
  uint64_t *sizes = nullptr;     // n
  uint64_t *offs = nullptr;      // n + 1: the layout
  uint64_t *src_off = nullptr;   // n: where each entry's copied bytes start in the params
  uint32_t *meta = nullptr;      // n
  uint32_t *name_word = nullptr; // kRequestMaxMethods: request_name_word of each name
  uint64_t *scan_tmp = nullptr;  // scan_tmp_words(n)
};
// Its arrays in pool workspace (as pack_ws_layout): the reply's, a 32-bit meta
// word, and one word per table name.  a.n is set.
template <class Layout> inline void request_ws_layout(Layout &w, RequestArgs &a, size_t tmp_words) {
  a.sizes = w.template take<uint64_t>(a.n);
  a.src_off = w.template take<uint64_t>(a.n);
  a.offs = w.template take<uint64_t>(a.n + 1);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  a.meta = w.template take<uint32_t>(a.n);
  a.name_word = w.template take<uint32_t>(kRequestMaxMethods);
}

#if defined(__HIPCC__)
// Table pass, size pass, exclusive scan, request kernel (when a.out is set),
// finish pass.
hipError_t launch_frames_request(const RequestArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
