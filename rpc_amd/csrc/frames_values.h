// rpc_amd/csrc/frames_values.h -- the frame values: typed results and params as
// JSON text (rpc_frames_values_device).  The args' mirror: what
// sits between the handlers' typed columns and the reply, and between a
// client's columns and the request.
//
// Entry i is a mode, the handler's verdict, a method and up to `width` 64-bit
// slots.  values_entry() applies the rules of include/rpccrc.h: the entry's
// status and, per declared parameter (RESULT form: the one result), one item
//
//   generated prefix . copied middle . generated suffix
//
//   lead `{` or `,` . "name": . number text            (all generated)
//   lead . "name": . " . string bytes . " . `}` when it is the last
//   TEXT entry:  the host's bytes                      (all copied)
//
// The exclusive scan of the item sizes is the layout; the output is produced
// with the reply's machinery, the splice (frames_splice.h: splice_piece() over
// ValuesSplice, the values' policy), the item taking the place of the reply's
// entry, so that an entry with several strings still has one copied middle per
// unit.  Numbers are formatted
// once, by values_f64() and its kin, into a 24-byte text record that the write
// pass only reads.
//
// values_f64() gives the bytes of cJSON's print_number (third_party/cJSON.c:
// 591-658): "%.15g", read back, kept when it lies within one epsilon, else
// "%.17g".  The digits are the double's significand times a 128-bit power of
// ten of pow10_table.h, values_scale(): the product's error is bounded by one
// unit of the table's last place, so a rounding is decided unless the
// fraction lies within that bound of one half; where the power is exact (10^0
// .. 10^55) the decision, ties included, is exact; for 10^-1 .. 10^-27 a
// fraction that close to one half is decided by an exact integer compare.
// Every tie that exists for a 53-bit significand lies in those two ranges.
// The read-back is frames_args.h's args_number() on the text itself.
//
// Everything here is plain inline code with no HIP types, shared by the kernels
// (frames_values.hip) and the CPU emulator (tests/cpu_emu/values_emu.cpp).
#pragma once
#include "frames_args.h"
#include "frames_splice.h"

namespace rpccrc {

// RPC_VALUES_* of include/rpccrc.h.
constexpr uint8_t kValuesNone = 0, kValuesOk = 1, kValuesText = 2, kValuesDefer = 3, kValuesRange = 4,
                  kValuesBadSchema = 5, kValuesNoRoom = 6;
constexpr uint8_t kValuesModeNone = 0, kValuesModeEncode = 1, kValuesModeText = 2;
constexpr int kValuesFormResult = 0, kValuesFormParams = 1;
constexpr uint32_t kValuesMaxText = 24; // bytes of a number's text
constexpr int32_t kValuesReplyInternal = -32603;

// ---- the text record ---------------------------------------------------------
// Up to 24 bytes in three little-endian words; bytes are appended through
// selects, so that no lane indexes an array.
struct ValText {
  uint64_t w0, w1, w2;
  uint32_t len;
};
PACK_HD void vt_put(ValText *t, uint32_t c) {
  const uint64_t v = (uint64_t)(c & 0xFFu) << (8 * (t->len & 7u));
  const uint32_t k = t->len >> 3;
  t->w0 |= k == 0 ? v : 0;
  t->w1 |= k == 1 ? v : 0;
  t->w2 |= k == 2 ? v : 0;
  ++t->len;
}
PACK_HD uint32_t vt_byte(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t i) { return splice_text_byte(w0, w1, w2, i); }
PACK_HD void vt_lit(ValText *t, const char *s, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) vt_put(t, (uint8_t)s[i]);
}

// The decimal digits of v, four bits each: digits 0 .. 15 in lo, 16 .. 19 in hi.
struct ValBcd {
  uint64_t lo, hi;
  uint32_t n; // digits without leading zeros, at least 1
};
PACK_HD ValBcd values_bcd(uint64_t v) {
  ValBcd d{0, 0, 1};
  for (uint32_t i = 0; i < 20; ++i) {
    const uint64_t q = v / 10u, r = v - q * 10u;
    if (i < 16) d.lo |= r << (4 * i);
    else d.hi |= r << (4 * (i - 16));
    if (r) d.n = i + 1;
    v = q;
  }
  return d;
}
PACK_HD uint32_t values_digit(const ValBcd &d, uint32_t r) { // digit r, the least significant is 0
  return (uint32_t)(r < 16 ? d.lo >> (4 * r) : d.hi >> (4 * (r - 16))) & 15u;
}
// %d / %lld of a sign and a magnitude.
PACK_HD void vt_int(ValText *t, bool neg, uint64_t mag) {
  const ValBcd d = values_bcd(mag);
  if (neg) vt_put(t, '-');
  for (uint32_t i = d.n; i-- > 0;) vt_put(t, '0' + values_digit(d, i));
}

// ---- significand times a power of ten ---------------------------------------------
constexpr uint64_t kValuesP15 = 1000000000000000ull, kValuesP17 = 100000000000000000ull;

// floor(log2(10^q)) for the table's exponents; floor(log10(2^e)) for a double's.
PACK_HD int32_t values_log2_pow10(int32_t q) { return (int32_t)(((int64_t)217706 * q) >> 16); }
PACK_HD int32_t values_log10_pow2(int32_t e) { return (int32_t)(((int64_t)78913 * e) >> 18); }
// 5^j, j <= 27, from the table's high word (5^j < 2^64: the word is 5^j shifted up).
template <class Pow> PACK_HD uint64_t values_pow5(const Pow &pow, uint32_t j) {
  const uint64_t w = pow.word(2u * (uint32_t)((int32_t)j - kPow10Min));
  return w >> __builtin_ctzll(w);
}

struct ValScaled {
  uint64_t floor; // floor(v) as the arithmetic sees it
  uint64_t near;  // v rounded to the nearest integer, ties to even
  bool decided;   // false: the arithmetic here cannot tell which side of one half v lies on
};
// v = X * 2^xe * 10^q for the 128-bit X = xh:xl with its top bit set,
// kPow10Min <= q <= kPow10Max, 2^40 <= v < 2^62.
template <class Pow> PACK_HD ValScaled values_scale(uint64_t xh, uint64_t xl, int32_t xe, int32_t q, const Pow &pow) {
  const uint32_t idx = 2u * (uint32_t)(q - kPow10Min);
  const uint64_t th = pow.word(idx), tl = pow.word(idx + 1);
  // the 256-bit product w3:w2:w1:w0 = X * T, in [2^254, 2^256)
  uint64_t hh_h, hh_l, hl_h, hl_l, lh_h = 0, lh_l = 0, ll_h = 0, ll_l = 0;
  args_mul64(xh, th, &hh_h, &hh_l);
  args_mul64(xh, tl, &hl_h, &hl_l);
  if (xl) {
    args_mul64(xl, th, &lh_h, &lh_l);
    args_mul64(xl, tl, &ll_h, &ll_l);
  }
  const uint64_t w0 = ll_l;
  uint64_t w1 = ll_h + lh_l, c1 = w1 < lh_l ? 1u : 0u;
  w1 += hl_l, c1 += w1 < hl_l ? 1u : 0u;
  uint64_t w2 = lh_h + hl_h, c2 = w2 < hl_h ? 1u : 0u;
  w2 += hh_l, c2 += w2 < hh_l ? 1u : 0u;
  w2 += c1, c2 += w2 < c1 ? 1u : 0u;
  const uint64_t w3 = hh_h + c2;
  // v = product * 2^-sh: 10^q = T * 2^(log2_pow10(q) - 127)
  const int32_t sh = 127 - xe - values_log2_pow10(q);
  ValScaled r{0, 0, false};
  if (sh < 193 || sh > 254) return r; // (outside what the callers ask for)
  const uint32_t fb = (uint32_t)sh - 192u; // fraction bits of w3: 1 .. 62
  const uint64_t fl = w3 >> fb, fh = w3 & ((1ull << fb) - 1u), hb = 1ull << (fb - 1);
  r.floor = fl;
  const bool low0 = (w2 | w1 | w0) == 0;
  bool up, tie = false;
  if (q >= 0 && q <= 55) { // 5^q < 2^128: the product is exact
    up = fh > hb || (fh == hb && !low0);
    tie = fh == hb && low0;
  } else if (!((fh == hb && w2 == 0) || (fh == hb - 1 && w2 == ~0ull))) {
    up = fh >= hb; // the table's error, under one unit of w2, does not reach one half
  } else if (q < 0 && q >= -27 && xl == 0) {
    // v >= fl + 1/2  <=>  xh * 2^(64 + xe + 1) >= (2 fl + 1) * 10^-q  <=>  xh * 2^s >= (2 fl + 1) * 5^-q
    const uint32_t j = (uint32_t)-q;
    const int32_t s = 64 + xe + 1 + q;
    uint64_t rh, rl, lh2, ll2;
    args_mul64(2 * fl + 1, values_pow5(pow, j), &rh, &rl);
    if (s >= 0) {
      if (s >= 64) return r;
      lh2 = s ? xh >> (64 - s) : 0, ll2 = xh << s;
    } else {
      if (s <= -64 || (rh >> (64 + s)) != 0) return r;
      lh2 = 0, ll2 = xh;
      rh = (rh << -s) | (rl >> (64 + s)), rl <<= -s;
    }
    tie = lh2 == rh && ll2 == rl;
    up = lh2 > rh || (lh2 == rh && ll2 > rl);
  } else {
    return r;
  }
  r.near = tie ? fl + (fl & 1u) : fl + (up ? 1u : 0u);
  r.decided = true;
  return r;
}

// The P significant digits of the normal double m * 2^(e2 - 52) (2^52 <= m <
// 2^53), correctly rounded, ties to even: digits in [10^(P-1), 10^P) and the
// decimal exponent k of the first.  False: undecided.
template <class Pow>
PACK_HD bool values_digits(uint64_t m, int32_t e2, uint32_t P, const Pow &pow, uint64_t *digits, int32_t *k10) {
  const uint64_t top = P == 15 ? kValuesP15 : kValuesP17, bottom = top / 10u;
  int32_t k = values_log10_pow2(e2); // k or k + 1 is the exponent
  for (uint32_t round = 0; round < 4; ++round) {
    int32_t q = (int32_t)P - 1 - k;
    uint64_t xh = m << 11, xl = 0;
    int32_t xe = e2 - 127;
    if (q > kPow10Max) { // the smallest doubles: 10^q = 10^j * 10^kPow10Max, the first factor exact
      const uint32_t j = (uint32_t)(q - kPow10Max); // <= 16
      uint64_t ph, pl;
      args_mul64(m, values_pow5(pow, j), &ph, &pl); // m * 5^j < 2^91: d * 10^j = (ph:pl) * 2^(e2 - 52 + j)
      uint32_t lz;
      if (ph) {
        lz = (uint32_t)__builtin_clzll(ph); // >= 1
        xh = (ph << lz) | (pl >> (64 - lz)), xl = pl << lz;
      } else {
        lz = 64u + (uint32_t)__builtin_clzll(pl);
        xh = pl << (lz - 64u), xl = 0;
      }
      xe = e2 - 52 + (int32_t)j - (int32_t)lz;
      q = kPow10Max;
    }
    const ValScaled s = values_scale(xh, xl, xe, q, pow);
    if (s.floor >= top) {
      ++k;
      continue;
    }
    if (!s.decided) return false;
    if (s.near < bottom) {
      --k;
      continue;
    }
    if (s.near == top) *digits = bottom, *k10 = k + 1; // the rounding carried
    else *digits = s.near, *k10 = k;
    return true;
  }
  return false;
}

// "%.<P>g": the digits and their exponent in C's shape.
PACK_HD void vt_g(ValText *t, bool neg, uint64_t digits, int32_t k, uint32_t P) {
  const ValBcd d = values_bcd(digits); // d.n == P
  uint32_t tz = 0;
  while (tz + 1 < P && values_digit(d, tz) == 0) ++tz;
  const uint32_t nd = P - tz; // significant digits left
  const auto dig = [&](uint32_t j) { return '0' + values_digit(d, P - 1 - j); }; // j < P, from the first
  if (neg) vt_put(t, '-');
  if (k < -4 || k >= (int32_t)P) {
    vt_put(t, dig(0));
    if (nd > 1) {
      vt_put(t, '.');
      for (uint32_t j = 1; j < nd; ++j) vt_put(t, dig(j));
    }
    vt_put(t, 'e');
    vt_put(t, k < 0 ? '-' : '+');
    const uint32_t a = (uint32_t)(k < 0 ? -k : k);
    if (a >= 100) vt_put(t, '0' + a / 100u);
    vt_put(t, '0' + (a / 10u) % 10u);
    vt_put(t, '0' + a % 10u);
  } else if (k >= 0) {
    for (uint32_t j = 0; j <= (uint32_t)k; ++j) vt_put(t, dig(j));
    if (nd > (uint32_t)k + 1) {
      vt_put(t, '.');
      for (uint32_t j = (uint32_t)k + 1; j < nd; ++j) vt_put(t, dig(j));
    }
  } else {
    vt_put(t, '0');
    vt_put(t, '.');
    for (int32_t z = -1; z > k; --z) vt_put(t, '0');
    for (uint32_t j = 0; j < nd; ++j) vt_put(t, dig(j));
  }
}

// The text as args_number() reads it.
struct ValTextBody {
  const ValText *t;
  PACK_HD uint32_t at(uint32_t i) const { return vt_byte(t->w0, t->w1, t->w2, i); }
};

// print_number of the double with these bits.  False: RPC_VALUES_DEFER, one of
//   a subnormal;
//   a rounding the arithmetic of values_scale() cannot decide;
//   a read-back that is neither normal, nor infinite, nor decided among the
//   subnormals next to the smallest normal.
template <class Pow> PACK_HD bool values_f64(uint64_t bits, const Pow &pow, ValText *t) {
  *t = ValText{0, 0, 0, 0};
  const bool neg = (bits >> 63) != 0;
  const uint32_t be = (uint32_t)(bits >> 52) & 0x7FFu;
  const uint64_t frac = bits & ((1ull << 52) - 1);
  if (be == 0x7FF) { // step 1
    vt_lit(t, "null", 4);
    return true;
  }
  if (be == 0 && frac == 0) { // +-0.0 == (double)0
    vt_put(t, '0');
    return true;
  }
  if (be == 0) return false; // step 3
  const uint64_t m = frac | (1ull << 52);
  const int32_t e2 = (int32_t)be - 1023;
  if (e2 >= 0 && e2 <= 31) { // step 2: an integer inside int
    const uint32_t drop = 52u - (uint32_t)e2;
    if ((m & ((1ull << drop) - 1)) == 0) {
      const uint64_t mag = m >> drop;
      if (neg ? mag <= 0x80000000ull : mag <= 0x7FFFFFFFull) {
        vt_int(t, neg, mag);
        return true;
      }
    }
  }
  uint64_t dg;
  int32_t k;
  if (!values_digits(m, e2, 15, pow, &dg, &k)) return false;
  vt_g(t, false, dg, k, 15); // (the magnitude: the sign changes nothing of the test)
  uint64_t rb = 0;
  bool keep;
  const ValTextBody body{t};
  if (args_number(body, 0, t->len, pow, &rb)) {
    const double a = args_bits_double(bits & ~(1ull << 63)), r = args_bits_double(rb);
    const double diff = r > a ? r - a : a - r, mx = r > a ? r : a;
    keep = diff <= mx * 2.220446049250313080847263336181640625e-16; // DBL_EPSILON
  } else if (e2 > 0) {
    keep = true; // above 1.797693134862315e308 the text reads back as infinity, and inf <= inf
  } else {
    // a subnormal read-back: r = R * 2^-1074 beside d = m * 2^-1074 with be == 1;
    // max(r, d) * DBL_EPSILON rounds to 2^-1074
    if (be != 1) return false;
    const uint32_t lz = (uint32_t)__builtin_clzll(dg);
    const ValScaled s = values_scale(dg << lz, 0, 1074 - (int32_t)lz - 64, k - 14, pow);
    if (!s.decided) return false;
    const uint64_t dist = s.near > m ? s.near - m : m - s.near;
    keep = dist <= 1;
  }
  *t = ValText{0, 0, 0, 0};
  if (keep) {
    vt_g(t, neg, dg, k, 15);
    return true;
  }
  if (!values_digits(m, e2, 17, pow, &dg, &k)) return false;
  vt_g(t, neg, dg, k, 17);
  return true;
}

// ---- items -----------------------------------------------------------------------
// What the size pass keeps of an item beside its size and its source offset.
constexpr uint32_t kItemNone = 0, kItemGen = 1, kItemStr = 2, kItemText = 3; // what follows the name
constexpr uint32_t kLeadNone = 0, kLeadOpen = 1, kLeadComma = 2;
PACK_HD uint32_t item_meta(uint32_t pre, uint32_t kind, uint32_t lead, bool named, bool last, uint32_t p) {
  return pre | (kind << 13) | (lead << 15) | ((named ? 1u : 0u) << 17) | ((last ? 1u : 0u) << 18) | (p << 19);
}
PACK_HD uint32_t item_pre(uint32_t m) { return m & 0x1FFFu; } // generated bytes in front of the copied ones
PACK_HD uint32_t item_kind(uint32_t m) { return (m >> 13) & 3u; }
PACK_HD uint32_t item_lead(uint32_t m) { return (m >> 15) & 3u; }
PACK_HD bool item_named(uint32_t m) { return ((m >> 17) & 1u) != 0; }
PACK_HD bool item_last(uint32_t m) { return ((m >> 18) & 1u) != 0; }
PACK_HD uint32_t item_param(uint32_t m) { return m >> 19; }
PACK_HD uint32_t item_suf(uint32_t m) { return (item_kind(m) == kItemStr ? 1u : 0u) + (item_last(m) ? 1u : 0u); }
// pre is at most the lead, "name": and a number's text
static_assert(1 + kArgsMaxNameBytes + 3 + kValuesMaxText < (1u << 13) && kArgsMaxSchemaParams <= (1u << 13),
              "the meta word's fields");

PACK_HD bool values_needs_escape(uint32_t c) { return c < 0x20u || c == '"' || c == '\\'; }

// The items of one entry.  In: the entry's inputs, each asked for only when the
// rules look at it:
//   uint8_t mode()  (ENCODE when the caller gave none), int32_t status() (0 likewise),
//   uint32_t method(), uint64_t slot(k), uint64_t str_base() (0 when none),
//   bool has_text(), uint64_t text_off(), uint32_t text_len()
// Schema: the args' (first, type, name_off, name) and uint32_t result_type(m).
// Str: bool clean(uint64_t off, uint32_t len): no byte of the strings at
// [off, off + len) needs an escape.  Sink: item(k, size, src, meta) and
// text(k, ValText), possibly for an entry that ends non-OK (the caller zeroes those).
// *used: the items an OK / TEXT entry has.
template <class In, class Schema, class Pow, class Str, class Sink>
PACK_HD uint8_t values_entry(const In &in, int form, const Schema &sc, uint32_t nmethods, uint32_t nparams,
                             uint32_t name_bytes, uint32_t width, uint64_t strings_bytes, uint64_t texts_bytes,
                             const Pow &pow, const Str &str, Sink &sink, uint32_t *used) {
  *used = 0;
  if (in.status() != 0) return kValuesNone;
  const uint8_t mode = in.mode();
  if (mode == kValuesModeText) {
    if (!in.has_text()) return kValuesRange;
    const uint64_t off = in.text_off();
    const uint32_t len = in.text_len();
    if (!(off <= texts_bytes && len <= texts_bytes - off)) return kValuesRange;
    sink.item(0, len, off, item_meta(0, kItemText, kLeadNone, false, false, 0));
    *used = 1;
    return kValuesText;
  }
  if (mode != kValuesModeEncode) return kValuesNone;
  const uint32_t method = in.method();
  if (method >= nmethods) return kValuesBadSchema;
  const bool params = form == kValuesFormParams;
  uint32_t f0 = 0, f1 = 1, rtype = 0;
  if (params) {
    f0 = sc.first(method), f1 = sc.first(method + 1);
    if (f0 > f1 || f1 > nparams || f1 - f0 > width) return kValuesBadSchema;
    for (uint32_t p = f0; p < f1; ++p) {
      const uint32_t x = sc.name_off(p), y = sc.name_off(p + 1);
      if (x > y || y > name_bytes || sc.type(p) > kArgStr) return kValuesBadSchema;
      for (uint32_t b = x; b < y; ++b)
        if (values_needs_escape(sc.name(b))) return kValuesBadSchema;
    }
    if (f0 == f1) { // {}
      sink.item(0, 2, 0, item_meta(1, kItemNone, kLeadOpen, false, true, 0));
      *used = 1;
      return kValuesOk;
    }
  } else {
    rtype = sc.result_type(method);
    if (rtype > kArgStr) return kValuesBadSchema;
  }
  const uint32_t np = f1 - f0;
  const uint64_t base = in.str_base();
  for (uint32_t k = 0; k < np; ++k) { // every string span, before any byte is read
    if ((params ? sc.type(f0 + k) : rtype) != kArgStr) continue;
    const uint64_t slot = in.slot(k), at = base + (slot & 0xFFFFFFFFull), len = slot >> 32;
    if (at < base || !(at <= strings_bytes && len <= strings_bytes - at)) return kValuesRange;
  }
  // every item and the entry's size, before any string byte is read (a value
  // that has no text counts no bytes)
  uint64_t total = 0;
  bool defer = false;
  for (uint32_t k = 0; k < np; ++k) {
    const uint32_t p = f0 + k, type = params ? sc.type(p) : rtype;
    const uint64_t slot = in.slot(k);
    const bool last = params && k + 1 == np;
    const uint32_t lead = !params ? kLeadNone : k == 0 ? kLeadOpen : kLeadComma;
    const uint32_t front = params ? 1u + (sc.name_off(p + 1) - sc.name_off(p)) + 3u : 0u;
    uint64_t size, src = 0;
    uint32_t meta;
    if (type == kArgStr) {
      const uint64_t at = base + (slot & 0xFFFFFFFFull);
      const uint32_t len = (uint32_t)(slot >> 32);
      meta = item_meta(front + 1, kItemStr, lead, params, last, params ? p : 0);
      size = (uint64_t)front + 1 + len + 1 + (last ? 1u : 0u);
      src = at;
    } else {
      ValText t{0, 0, 0, 0};
      if (type == kArgI32) {
        const int32_t v = (int32_t)(uint32_t)slot;
        vt_int(&t, v < 0, v < 0 ? 0ull - (uint64_t)(int64_t)v : (uint64_t)v);
      } else if (type == kArgI64) {
        const int64_t v = (int64_t)slot;
        vt_put(&t, '"');
        vt_int(&t, v < 0, v < 0 ? 0ull - slot : slot);
        vt_put(&t, '"');
      } else if (type == kArgBool) {
        if (slot) vt_lit(&t, "true", 4);
        else vt_lit(&t, "false", 5);
      } else if (!values_f64(slot, pow, &t)) {
        defer = true;
        continue;
      }
      meta = item_meta(front + t.len, kItemGen, lead, params, last, params ? p : 0);
      size = (uint64_t)front + t.len + (last ? 1u : 0u);
      sink.text(k, t);
    }
    sink.item(k, size, src, meta);
    total += size;
  }
  if (total > 0xFFFFFFFFull) return kValuesRange; // (a value length is 32 bits)
  if (defer) return kValuesDefer;
  for (uint32_t k = 0; k < np; ++k) { // the strings are read: once each
    if ((params ? sc.type(f0 + k) : rtype) != kArgStr) continue;
    const uint64_t slot = in.slot(k);
    if (!str.clean(base + (slot & 0xFFFFFFFFull), (uint32_t)(slot >> 32))) return kValuesDefer;
  }
  *used = np;
  return kValuesOk;
}
// An entry that does not end inside out_cap is not written (the reply's rule).
PACK_HD uint8_t values_final_status(uint8_t st, uint64_t at, uint64_t size, uint64_t out_cap) {
  return (size != 0 && !pack_fits(at, size, out_cap)) ? kValuesNoRoom : st;
}
PACK_HD int32_t values_reply_status(uint8_t final_status, int32_t status) {
  return final_status == kValuesNone || final_status == kValuesOk || final_status == kValuesText ? status
                                                                                                  : kValuesReplyInternal;
}

// ---- generated bytes --------------------------------------------------------------
// Generated byte g of an item: the bytes in front of the copied ones and the
// bytes behind them, counted through.  Schema: name_off(p), name(b) (asked for
// only under a name); w0 .. w2: the item's text record (a kItemGen item's).
template <class Schema>
PACK_HD uint32_t values_gen_byte(uint32_t meta, uint64_t w0, uint64_t w1, uint64_t w2, const Schema &sc, uint32_t g) {
  const uint32_t lead = item_lead(meta), kind = item_kind(meta);
  uint32_t front = 0;
  if (lead != kLeadNone) {
    if (g == 0) return lead == kLeadOpen ? '{' : ',';
    g -= 1, front = 1;
  }
  if (item_named(meta)) {
    const uint32_t p = item_param(meta), a = sc.name_off(p), nl = sc.name_off(p + 1) - a;
    if (g == 0 || g == nl + 1) return '"';
    if (g <= nl) return sc.name(a + g - 1);
    if (g == nl + 2) return ':';
    g -= nl + 3, front += nl + 3;
  }
  if (kind == kItemGen) {
    const uint32_t tl = item_pre(meta) - front;
    if (g < tl) return vt_byte(w0, w1, w2, g);
    g -= tl;
  } else if (kind == kItemStr) {
    if (g <= 1) return '"'; // the opening quote, then the closing one
    g -= 2;
  }
  return '}';
}

// ---- the splice policy ---------------------------------------------------------------
// The values under splice_piece() (frames_splice.h), the items for its entries.
// Ent: the items.
//   uint32_t meta(u); uint64_t text(u, j), word j of its record (asked for only
//   when a byte of a kItemGen item is generated); bool written(u), the item's
//   entry ends inside out_cap
// Schema: as values_gen_byte()'s.  The copied bytes of a kItemText item come
// from the texts, every other item's from the strings.
template <class Ent, class Schema, class Src> struct ValuesSplice {
  const Ent &ent;
  const Schema &sc;
  const Src &strings, &texts;
  struct Gen {
    uint32_t m;
    uint64_t w0, w1, w2;
    const Schema &sc;
    PACK_HD uint32_t byte(uint32_t g) const { return values_gen_byte(m, w0, w1, w2, sc, g); }
  };
  PACK_HD bool written(uint64_t u, uint64_t) const { return ent.written(u); }
  PACK_HD uint32_t meta(uint64_t u) const { return ent.meta(u); }
  PACK_HD uint32_t pre(uint32_t m) const { return item_pre(m); }
  PACK_HD uint32_t suf(uint32_t m) const { return item_suf(m); }
  PACK_HD Gen gen(uint64_t u, uint32_t m) const {
    const bool gen = item_kind(m) == kItemGen;
    return Gen{m, gen ? ent.text(u, 0) : 0, gen ? ent.text(u, 1) : 0, gen ? ent.text(u, 2) : 0, sc};
  }
  PACK_HD const Src &src(uint32_t m) const { return item_kind(m) == kItemText ? texts : strings; }
};
// One piece of the values from their readers: splice_piece() over the policy.
// SrcOf, the piece and [lo, hi] as there.
template <class Off, class Ent, class SrcOf, class Schema, class Src>
PACK_HD PackPiece values_piece(const Off &off, const Ent &ent, const SrcOf &src_of, const Schema &sc, const Src &strings,
                               const Src &texts, uint64_t lo, uint64_t hi, uint64_t x0, uint64_t x1, uint32_t b0) {
  return splice_piece(ValuesSplice<Ent, Schema, Src>{ent, sc, strings, texts}, off, src_of, lo, hi, x0, x1, b0);
}

// ---- the call (frames_values.hip) ---------------------------------------------------
struct ValuesArgs {
  int form = 0;
  const uint8_t *mode = nullptr;   // nullptr: ENCODE for all
  const int32_t *status = nullptr; // nullptr: 0 for all
  const uint16_t *method = nullptr;
  const uint64_t *slots = nullptr; // width x n, column-major
  uint32_t width = 0;
  uint64_t n = 0;
  const uint8_t *result_types = nullptr; // RESULT form: nmethods
  const uint32_t *param_first = nullptr; // PARAMS form: the args' schema
  uint32_t nmethods = 0;
  const uint8_t *param_types = nullptr;
  const uint32_t *param_name_off = nullptr;
  uint32_t nparams = 0;
  const uint8_t *param_names = nullptr;
  uint32_t name_bytes = 0;
  const uint8_t *strings = nullptr;
  uint64_t strings_bytes = 0;
  const uint64_t *str_base = nullptr; // nullptr: 0 for all
  const uint8_t *texts = nullptr;
  uint64_t texts_bytes = 0;
  const uint64_t *text_off = nullptr;
  const uint32_t *text_len = nullptr;
  // outputs (the caller's; all optional)
  uint8_t *out = nullptr;
  uint64_t out_cap = 0;
  uint64_t *value_off = nullptr;
  uint32_t *value_len = nullptr;
  uint8_t *values_status = nullptr;
  int32_t *reply_status = nullptr;
  uint32_t *ndefer = nullptr;
  uint64_t *total = nullptr;
  // workspace: `unit` items per entry (RESULT: 1; PARAMS: width), items = n * unit
  uint32_t unit = 1;
  uint64_t items = 0;
  uint64_t *sizes = nullptr;              // items
  uint64_t *offs = nullptr;               // items + 1: the layout
  uint64_t *src_off = nullptr;            // items
  uint32_t *meta = nullptr;               // items
  uint64_t *text0 = nullptr, *text1 = nullptr, *text2 = nullptr; // items: the text records
  uint8_t *pre = nullptr;                 // n: provisional statuses
  // the work list of very long strings, one record per STR item at the most
  uint32_t *long_count = nullptr;         // 1
  uint64_t *long_off = nullptr;           // items
  uint32_t *long_len = nullptr, *long_entry = nullptr, *long_bad = nullptr; // items each
  uint64_t *scan_tmp = nullptr;           // scan_tmp_words(items)
};
// Its arrays in pool workspace (as pack_ws_layout); a.n and a.items are set.
template <class Layout> inline void values_ws_layout(Layout &w, ValuesArgs &a, size_t tmp_words) {
  a.sizes = w.template take<uint64_t>(a.items);
  a.src_off = w.template take<uint64_t>(a.items);
  a.offs = w.template take<uint64_t>(a.items + 1);
  a.scan_tmp = w.template take<uint64_t>(tmp_words);
  a.text0 = w.template take<uint64_t>(a.items);
  a.text1 = w.template take<uint64_t>(a.items);
  a.text2 = w.template take<uint64_t>(a.items);
  a.long_off = w.template take<uint64_t>(a.items);
  a.meta = w.template take<uint32_t>(a.items);
  a.long_len = w.template take<uint32_t>(a.items);
  a.long_entry = w.template take<uint32_t>(a.items);
  a.long_bad = w.template take<uint32_t>(a.items);
  a.long_count = w.template take<uint32_t>(1);
  a.pre = w.template take<uint8_t>(a.n);
}

#if defined(__HIPCC__)
// Size pass, the grid's scan of very long strings, exclusive scan, values kernel
// (when a.out is set), finish pass.
hipError_t launch_frames_values(const ValuesArgs &a, hipStream_t s);
#endif

} // namespace rpccrc
