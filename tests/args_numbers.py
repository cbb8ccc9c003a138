"""The number texts the frame args' decimal to double conversion is held against, in one place:
the CPU emulator (tests/test_args_pow10.py) and the device (tests/test_frames_args_numbers.py)
convert the same strings.

Three lists moved here from test_args_pow10.py unchanged (same seeds, same order): `ties`,
`digit_strings` and `integers_and_ties`.  Four lists are chosen to reach each branch of
args_number (rpc_amd/csrc/frames_args.h): `second_product`, `exact_edges`, `normal_edges` and
`int_edges`.

`branch` names the path a text takes, from Python integers over tools/gen_pow10.table().  It
chooses inputs and counts them; no expected value comes from it.  Expected values are float()'s
(args_cases.f64_of, args_cases.convert)."""
import functools
import importlib.util
import math
import os
import random
import re
from fractions import Fraction

import args_fuzz as af

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
MIN_NORMAL = Fraction(1, 2 ** 1022)
MAX_DOUBLE = (2 ** 53 - 1) * 2 ** 971
#: the effective exponents at which a text of at most 19 digits can take the second product and
#: still give a normal double (below -326 no 19-digit significand reaches 2^-1022)
EL2_Q = range(-326, 305)
EXP_FORMS = ("e%d", "E%d", "e%+d", "e%03d")


@functools.lru_cache(maxsize=None)
def gen_pow10():
    spec = importlib.util.spec_from_file_location("gen_pow10", os.path.join(REPO, "tools", "gen_pow10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def table():
    return gen_pow10().table()


# ---- which path a text takes --------------------------------------------------------------
_NUMBER = re.compile(r"-?([0-9]+)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?\Z")


def parts(text):
    """(significant digits without leading zeros, digits behind the point, exponent)."""
    ip, fp, ex = _NUMBER.match(text).groups()
    fp = fp or ""
    return (ip + fp).lstrip("0"), len(fp), int(ex or 0)


def second(w, q):
    """(the second product is taken, it carries into the high word) for w * 10^q."""
    c = table()[q - gen_pow10().E_MIN]
    w <<= 64 - w.bit_length()
    p = w * (c >> 64)
    if (p >> 64) & 0x1FF != 0x1FF:
        return False, False
    return True, (p & M64) + ((w * (c & M64)) >> 64) > M64


def branch(text):
    """(path, q): zero, many (more than 19 digits), range (q outside the table), exact, el, or
    el2 (Eisel-Lemire with the second product); q = exponent - fraction digits."""
    digits, frac, ex = parts(text)
    q = ex - frac
    if not digits:
        return "zero", q
    if len(digits) > 19:
        return "many", q
    if not gen_pow10().E_MIN <= q <= gen_pow10().E_MAX:
        return "range", q
    w = int(digits)
    if w < 2 ** 53 and -22 <= q <= 22:
        return "exact", q
    return ("el2" if second(w, q)[0] else "el"), q


def carries(text):
    """An el2 text whose second product carries into the high word."""
    digits, frac, ex = parts(text)
    return branch(text)[0] == "el2" and second(int(digits), ex - frac)[1]


def decisive(text):
    """An el2 text whose double depends on the carry: the bit the conversion rounds at (bit 10 of
    the high word when its top bit is set, else bit 9) is 0 above the ones."""
    if branch(text)[0] != "el2":
        return False
    digits, frac, ex = parts(text)
    w, c = int(digits), table()[ex - frac - gen_pow10().E_MIN]
    hi = (w << (64 - w.bit_length())) * (c >> 64) >> 64
    return hi & 0x7FF == 0x3FF if hi >> 63 else hi & 0x3FF == 0x1FF


def carry_margin(text):
    """lo + hi2 - 2^64 of an el2 text: not negative when the second product carries."""
    digits, frac, ex = parts(text)
    w, c = int(digits), table()[ex - frac - gen_pow10().E_MIN]
    w <<= 64 - w.bit_length()
    return (w * (c >> 64) & M64) + (w * (c & M64) >> 64) - 2 ** 64


def spell(rng, w, q, plain=False):
    """w * 10^q as text: a sign, a point somewhere (so that the fraction digits and the exponent
    both contribute to q) and one of the exponent forms."""
    d = str(w)
    at = len(d) if plain else rng.randrange(0, len(d) + 1)
    ex = q + len(d) - at
    if at < len(d):
        d = (d[:at] or "0") + "." + d[at:]
    return rng.choice(("", "-")) + d + rng.choice(EXP_FORMS) % ex


def deferral_bounds(texts):
    """(fewest, most) texts that defer, from float() alone: a text whose double is no normal
    double (zero from digits that are not all zero, a subnormal, an infinity) has to defer, and
    one of more than 19 significant digits may."""
    must = may = 0
    for t in texts:
        digits = parts(t)[0]
        f = abs(float(t))
        if digits and (f < 2.0 ** -1022 or math.isinf(f)):
            must += 1
        elif len(digits) > 19:
            may += 1
    return must, must + may


# ---- the lists test_args_pow10.py has always run ------------------------------------------
def ties(rng, count):
    """Integers exactly halfway between two neighbouring doubles above 2^53, below 10^19."""
    out = []
    while len(out) < count:
        s = rng.randrange(1, 11)
        t = (2 * rng.randrange(2**52, 2**53) + 1) << (s - 1)
        if t < 10**19:
            out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def tie_texts():
    return tuple(str(t) for t in ties(random.Random(0x71E5), 5000))


@functools.lru_cache(maxsize=None)
def digit_strings():
    """Fixed-seed strings of 1 to 19 digits with a decimal exponent in [-320, 289], plain and
    with a point, a sign, leading zeros and every exponent form."""
    rng = random.Random(0x9017)
    texts = []
    for k in range(60000):
        digits = str(rng.randrange(1, 10 ** rng.randrange(1, 20)))
        e = rng.randrange(-320, 290)
        if k % 3 == 0:  # a point somewhere: "0.123", "12.3"
            at = rng.randrange(0, len(digits))
            digits = (digits[:at] or "0") + "." + digits[at:]
        text = rng.choice(("", "-")) + digits + rng.choice(("e%d", "E%d", "e%+d", "e%03d")) % e
        texts.append(text)
    texts += ["0", "-0", "0.0", "-0.000", "0e5", "-0E-7", "1", "-1", "0.1", "123456789", "1e22", "1e23", "9007199254740993",
              "1.7976931348623157e308", "2.2250738585072014e-308", "2.225073858507201137e-308", "1e-342", "1e308", "9e-342"]
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def integers_and_ties():
    """(texts, ties): integers in [2^53, 10^19), exact ties between neighbouring doubles above
    2^53, the same with e-1 .. e-25 appended, and the ties that a negative exponent leaves exact.
    The first 40,000 texts are the plain integers and ties."""
    rng = random.Random(0x7135)
    ints = [rng.randrange(2**53, 10**19) for _ in range(20000)]
    tied = ties(rng, 20000)
    texts = [str(v) for v in ints + tied]
    texts += ["%de-%d" % (v, rng.randrange(1, 26)) for v in ints[:10000] + tied]
    for k in range(1, 5):  # m + 1/2 ulp for a double m of [2^(53-k), 2^(54-k)): (2m' + 1) * 5^k e-k
        half = [(2 * rng.randrange(2**52, 2**53) + 1) * 5**k for _ in range(3000)]
        texts += ["%de-%d" % (v, k) for v in half if v < 10**19]
    texts.append("63863781979156355e-1")
    return tuple(texts), tuple(tied)


def plain_integers():
    return integers_and_ties()[0][:40000]


# ---- the second product ---------------------------------------------------------------------
def normal_range(q):
    """[lo, hi): the significands w below 10^19 with 2^-1022 <= w * 10^q <= the largest double;
    on the exact path's exponents only those it does not take."""
    p = Fraction(10) ** q
    lo = max(1, math.ceil(MIN_NORMAL / p))
    hi = min(10 ** 19, math.floor(MAX_DOUBLE / p) + 1)
    if abs(q) <= 22:
        lo = max(lo, 2 ** 53)
    return lo, hi


@functools.lru_cache(maxsize=None)
def second_product():
    """For every effective exponent that has them, texts that take the second product and give
    a normal double, with and without its carry into the high word: a random w in [2^53, 10^19),
    a shorter one where only those stay normal, every w where there are few.  At most 20,000
    tries per exponent.  Then near_carry's two per exponent."""
    rng = random.Random(0x5EC0)
    e_min, e_max = gen_pow10().E_MIN, gen_pow10().E_MAX
    texts = []
    for q in range(e_min, e_max + 1):
        lo, hi = normal_range(q)
        if hi - lo > 20000 and hi > 2 ** 53:
            lo = max(lo, 2 ** 53)
        if lo >= hi:
            continue
        ws = iter(range(lo, hi)) if hi - lo <= 20000 else (rng.randrange(lo, hi) for _ in range(20000))
        c = table()[q - e_min]
        chi, clo = c >> 64, c & M64
        found = [[], []]  # without the carry, with it
        for tries, w in enumerate(ws):
            n = w << (64 - w.bit_length())
            p = n * chi
            if (p >> 64) & 0x1FF != 0x1FF:
                continue
            carry = (p & M64) + ((n * clo) >> 64) > M64
            if len(found[carry]) < 2:
                found[carry].append(w)
            if (found[0] and found[1]) or (len(found[0]) + len(found[1]) >= 2 and tries >= 3000):
                break
        for k, w in enumerate(found[0] + found[1] + near_carry(rng, q, chi, clo)):
            texts.append(spell(rng, w, q, plain=k == 0))
    return tuple(texts)


def near_carry(rng, q, chi, clo, count=256):
    """19-digit w of [2^63, 10^19) that take the second product at q, built and not searched: such
    a w is its own 64-bit form, so for a high word H that ends in nine ones, ceil(H * 2^64 / chi)
    is one, and often the next integer too.  H has a 0 above its ones, in the place the
    conversion rounds at: only then does a carry change the double (an odd significand rounds
    up with and without it).  Of `count` of them the two whose sum lo + hi2 lies nearest to 2^64 from below and
    from above: a wrong high bit in the table's low word moves hi2 across the carry there, which
    it does for few of the texts a random search finds.  None where such a w is no normal double."""
    lo_w, hi_w = normal_range(q)
    lo_w = max(lo_w, 2 ** 63)
    if lo_w >= hi_w:
        return []
    below = above = None  # (margin, w)
    for _ in range(count):
        h = rng.randrange((lo_w * chi >> 75) + 1, hi_w * chi >> 75) << 11 | 0x3FF
        if not h >> 63:
            h ^= rng.choice((0x200, 0x600))  # (one bit fewer is shifted out: the rounding bit is bit 9)
        w = -(-(h << 64) // chi) + rng.randrange(2)  # (one or two w share a high word)
        if not lo_w <= w < hi_w or w * chi >> 64 != h:
            continue
        margin = (w * chi & M64) + (w * clo >> 64) - 2 ** 64
        if margin < 0 and (below is None or margin > below[0]):
            below = margin, w
        if margin >= 0 and (above is None or margin < above[0]):
            above = margin, w
    return [x[1] for x in (below, above) if x]


# ---- the edges of the exact path ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_edges():
    """w around 2^53 and below it against q around +-22 and +-1; 40,000 random w < 2^53 with q in
    [-22, -1] (the divide) and 10,000 with q in [1, 22] (the multiply), every fourth of them
    also with a point and another exponent form."""
    rng = random.Random(0xE8AC7)
    texts = []
    for q in (-23, -22, -1, 1, 22, 23):
        for w in [2**53 - 1, 2**53, 2**53 + 1] + [rng.randrange(1, 2**53) for _ in range(20)]:
            texts.append("%de%d" % (w, q))
            texts.append(spell(rng, w, q))
    for count, qs in ((40000, (-22, 0)), (10000, (1, 23))):
        for k in range(count):
            w = rng.randrange(1, 2 ** rng.randrange(1, 54)) if k % 4 == 3 else rng.randrange(1, 2**53)
            q = rng.randrange(*qs)
            texts.append("%de%d" % (w, q))
            if k % 4 == 0:
                texts.append(spell(rng, w, q))
    return tuple(texts)


# ---- the ends of the normal doubles ---------------------------------------------------------
def cut(x, nd):
    """x cut to nd significant digits: (w, q) with 10^(nd-1) <= w < 10^nd and w * 10^q <= x."""
    q = math.floor(math.log10(x.numerator) - math.log10(x.denominator)) - nd + 1
    while x / Fraction(10) ** q >= 10 ** nd:
        q += 1
    while x / Fraction(10) ** q < 10 ** (nd - 1):
        q -= 1
    return math.floor(x / Fraction(10) ** q), q


def pointed(w, q):
    """d.ddd...e<x>, the way a double is printed."""
    d = str(w)
    return "%s.%se%d" % (d[0], d[1:], q + len(d) - 1)


@functools.lru_cache(maxsize=None)
def normal_edges():
    """17 to 19 digits around 2^-1022 and the double below it (the carry into the smallest
    normal, and DEFER beside it), around the largest double and the halfway point to 2^1024
    behind it; q at both ends of the table and just outside; 20, 25 and 400 digits; exponents of
    six digits and more."""
    texts = []
    below = MIN_NORMAL - Fraction(1, 2 ** 1074)
    half_up = Fraction(MAX_DOUBLE + 2 ** 970)
    for nd in (17, 18, 19):
        for x in (MIN_NORMAL, below, Fraction(MAX_DOUBLE), half_up):
            w, q = cut(x, nd)
            for k in range(-50, 51):
                if 10 ** (nd - 1) <= w + k < 10 ** nd:
                    texts.append("%de%d" % (w + k, q))
                    if k % 5 == 0:
                        texts.append(pointed(w + k, q))
                        texts.append("-" + pointed(w + k, q).replace("e", "E"))
    w, q = cut(Fraction(MAX_DOUBLE), 19)  # every 19-digit text from the largest double to the halfway point
    texts += ["%de%d" % (v, q) for v in range(w, cut(half_up, 19)[0] + 1)]
    texts += ["1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "2.2250738585072014e-308",
              "2.2250738585072011e-308", "4.9e-324"]
    # q = -342, -343, 308, 309, from the exponent alone and with the fraction digits' help
    texts += ["1e-342", "9999999999999999999e-342", "22250738585072014e-342", "1e-343", "9e-343", "1.0e-342", "10e-343",
              "1e308", "1.5e308", "17e307", "2e308", "0.1e309", "0.01e310", "0.17e309", "1e309", "10e308", "0.0e309",
              "1797693134862315708e290", "17976931348623157e292", "179769313486231570e291", "0.000001e314",
              "2225073858507201383e-326", "0.2225073858507201383e-307", "0.000002225073858507201383e-302"]
    # more than 19 significant digits: DEFER whatever the value
    many = ["1" * 20, "1" * 25, "1234567890" * 40, "1.0000000000000000000", "1" + "0" * 19, "1" + "0" * 25, "0." + "1" * 20,
            "12345678901234567890e-10", "9007199254740993.0000", "0.10000000000000000000", "1" + "0" * 399,
            "1." + "0" * 399 + "e5", "123456789012345678905e-400", "0." + "3" * 400, "1" * 25 + "e-30"]
    texts += many + ["-" + t for t in many]
    # ... and long texts that are not: the zeros in front do not count
    texts += ["0." + "0" * 400 + "1", "0." + "0" * 300 + "123e300", "0." + "0" * 300 + "123e301", "0." + "0" * 30 + "5",
              "0." + "0" * 321 + "2225073858507201383e14", "0." + "0" * 400, "-0." + "0" * 400 + "e400",
              "0." + "0" * 19 + "1234567890123456789", "0.00000000000000000001"]
    # exponents of six digits and more: no wrap, and leading zeros are no magnitude
    texts += ["1e999999", "1e-999999", "-1e999999", "0e999999", "-0e-999999", "1e100000", "1e-100000", "1e123456", "1E+999999",
              "5e+000001", "5e-000001", "25e0000000000000000000000001", "1e4294967296", "1e-4294967296", "1e4294967297",
              "1e2147483648", "1e-2147483649", "7e18446744073709551617", "0." + "0" * 400 + "1e000401", "1e000308", "1e000309",
              "1" + "0" * 300 + "e-000300"]
    return tuple(texts)


# ---- number texts for the integer columns ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_edges():
    """The int32 and int64 edges as integers, with fractions, exponents and scaled; what lies
    beside +-2^63 among the doubles and among the 19-digit texts; 5,000 doubles around the int32
    range and 5,000 around the int64 range as %.17g prints them."""
    rng = random.Random(0x10ED6E5)
    texts = []
    for v in af.EDGES:
        texts += [f % v for f in ("%d", "%d.0", "%d.5", "%d.999999999", "%de0", "%d.0e+0")]
        if v:  # (scaled; "00e-1" would be no JSON number)
            texts += [f % v for f in ("%d0e-1", "%d00E-2")]
    texts += ["0.9999", "-0.9999", "-0.0", "1e-300", "-1e-300", "0.5", "-0.5", "1e-320",
              "2147483647.9999999", "2147483647.99999999999", "2147483648.0000001", "-2147483648.9999999",
              "-2147483648.99999999999", "-2147483649.0000001", "21474836470e-1", "21474836480e-1", "-21474836489e-1",
              "-21474836490e-1", "0.2147483647e10", "0.2147483648e10", "-0.2147483649e10", "2147483647e0", "2.147483648e9",
              "-2.147483648e9", "-2.147483649e9"]
    # the doubles beside 2^63 lie 1024 apart below it and 2048 apart above it
    for v in (2**63 - 1024, 2**63 - 1025, 2**63 - 513, 2**63 - 512, 2**63 - 511, 2**63 - 1, 2**63, 2**63 + 1, 2**63 + 1024,
              2**63 + 1025, 2**63 + 2048, 10**19 - 1):
        texts += [str(v), str(-v)]
    texts += ["-9223372036854775808", "-9223372036854775807", "-9223372036854775809", "-9223372036854776832",
              "-9223372036854776833", "-9223372036854777856", "-9.223372036854775808e18", "-9223372036854775808.0",
              "9.223372036854775807e18", "9223372036854774784.0", "922337203685477478e1", "9.2233720368547748e18",
              "-9.2233720368547758e18", "-9.2233720368547778e18", "1e19", "-1e19", "1e300", "-1e300"]
    for k in range(5000):
        d = rng.uniform(-2.0**31 - 2, 2.0**31 + 2) if k % 4 else rng.choice((-1, 1)) * (2.0**31 + rng.uniform(-2, 2))
        texts.append("%.17g" % d)
    for k in range(5000):
        d = rng.uniform(-2.0**63, 2.0**63) if k % 2 else rng.uniform(-1, 1) * 2.0 ** rng.randrange(0, 64)
        texts.append("%.17g" % d)
    return tuple(texts)


def f64_corpus():
    """Every text the F64 column converts, list by list."""
    return (digit_strings() + integers_and_ties()[0] + tie_texts() + second_product() + exact_edges() + normal_edges() +
            int_edges())


def int_corpus():
    """Every text the I32 and I64 columns convert."""
    return int_edges() + tie_texts() + plain_integers()
