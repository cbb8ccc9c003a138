"""The doubles the frame values' number formatting is held against, in one place: the CPU
emulator (tests/test_values_emu.py) and the device (tests/test_frames_values_numbers.py) format
the same bit patterns.  `corpus()` is a dict of labelled lists of 64-bit patterns; expected texts
are values_cases.f64_text's (the plain "%.15g" / float() / "%.17g" rule), never the code's.

Lists on which no entry may defer: ZERO_DEFER.  On every other list but `subnormals` at most one
in 10,000 may (the rules never defer a finite normal double)."""
import functools
import random
import struct

M64 = (1 << 64) - 1
SIGN = 1 << 63
ZERO_DEFER = ("random_bits", "class15", "powers_of_two", "powers_of_ten", "ties15", "ties17")


def bits_of(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def double_of(b):
    return struct.unpack("<d", struct.pack("<Q", b & M64))[0]


def normal(b):
    return 0 < ((b >> 52) & 0x7FF) < 0x7FF


def around(b, span):
    """b and its neighbours up to `span` ulps away that are normal doubles of b's sign."""
    return [b + k for k in range(-span, span + 1) if normal(b + k) and (b + k) >> 63 == b >> 63]


def signed(bs, rng):
    """Every pattern, about a third of them negated."""
    return [b | SIGN if rng.random() < 0.33 else b for b in bs]


def powers_of_two(rng):
    out = []
    for e in range(-1022, 1024):
        out += around(bits_of(2.0 ** e), 1)
    return signed(out, rng)


def powers_of_ten(rng):
    out = []
    for k in range(-307, 309):
        out += around(bits_of(float("1e%d" % k)), 1)
    return signed(out, rng)


def below_powers_of_ten(rng):
    """10^k minus a few ulps for every k: the carry turns 9.99...e22 into 1e+23."""
    out = []
    for k in range(-307, 309):
        b = bits_of(float("1e%d" % k))
        out += [b - j for j in range(1, 6) if normal(b - j)]
    return signed(out, rng)


def shape_switches(rng):
    """Both sides of the 1e-5 / 1e-4, 1e15 and 1e17 switches between fixed and scientific."""
    out = []
    for x in (1e-5, 1e-4, 9.9999999999999e-5, 9.99999999999999954e-5, 1e15, 999999999999999.0, 999999999999999.9,
              1e16, 1e17, 99999999999999984.0, 12345678901234567.0, 1234567890123456.7, 0.00012345678901234567,
              0.000012345678901234567):
        out += around(bits_of(x), 8)
    return signed(out, rng)


def integer_edges(rng):
    out = []
    for x in (2147483647.0, -2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0, 2147483649.0, 2.0 ** 53 - 1,
              2.0 ** 53, 2.0 ** 53 + 2, 1.0, -1.0, 0.5, -0.5):
        out += [bits_of(x), bits_of(x + 0.5), bits_of(x - 0.5)] + around(bits_of(x), 2)
    out += [0, SIGN]
    out += [bits_of(float(rng.randrange(-2 ** 31, 2 ** 31))) for _ in range(2000)]
    out += [bits_of(rng.randrange(-2 ** 33, 2 ** 33) / 2.0) for _ in range(2000)]
    return out


def class15(rng, n):
    """k / 10^j with k < 10^15: the 15-digit class."""
    out = []
    while len(out) < n:
        k, j = rng.randrange(1, 10 ** rng.randrange(1, 16)), rng.randrange(0, 40)
        b = bits_of(float("%de-%d" % (k, j)))
        if normal(b):
            out.append(b)
    return signed(out, rng)


def random_bits(rng, n):
    out = []
    while len(out) < n:
        b = rng.getrandbits(64)
        if normal(b):
            out.append(b)
    return out


def ulps_away(rng, per):
    """By search: doubles whose 15-digit read-back lies exactly 0, 1, 2, 3 and 4 ulps away, on both
    sides of a binade boundary where max * eps changes (1 ulp away keeps 15 digits without
    round-tripping).  A dict distance -> patterns."""
    found = {k: [] for k in range(5)}
    tries = 0
    while min(len(v) for v in found.values()) < per and tries < 400000:
        tries += 1
        e = rng.randrange(-1000, 1000)
        # just above or just below a power of two, or anywhere
        pick = rng.random()
        frac = rng.getrandbits(12) if pick < 0.3 else (1 << 52) - 1 - rng.getrandbits(12) if pick < 0.6 else rng.getrandbits(52)
        b = ((e + 1023) << 52) | frac
        r = bits_of(float("%.15g" % double_of(b)))
        dist = abs(r - b)
        if dist in found and len(found[dist]) < per:
            found[dist].append(b)
    return found


def ties15(rng, n):
    """Exact ties at 15 digits: N + 0.5 for 15-digit N below 2^52, even and odd N."""
    out = []
    for _ in range(n):
        N = rng.randrange(10 ** 14, min(10 ** 15, 2 ** 52))
        out.append(bits_of(N + 0.5))
    out += [bits_of((2 * N + 1) * 5.0) for N in (rng.randrange(10 ** 14, 4 * 10 ** 14) for _ in range(n // 4))]
    return signed(out, rng)


def ties17(rng, n):
    """Exact ties at 17 digits: t / 2^(j+1) with odd t < 2^53 and t * 5^j in the 17-digit window,
    e.g. 1000000000000000.25."""
    out = [bits_of(1000000000000000.25)]
    while len(out) < n:
        j = rng.randrange(1, 12)
        # t * 5^(j+1) is the digit string with a trailing 5: 18 digits, so 17 digits tie
        lo, hi = -(-10 ** 17 // 5 ** (j + 1)), 10 ** 18 // 5 ** (j + 1)
        if lo >= min(hi, 2 ** 53):
            continue
        t = rng.randrange(lo, min(hi, 2 ** 53)) | 1
        x = t / 2.0 ** (j + 1)
        if t < 2 ** 53 and len(("%.25f" % x).rstrip("0").replace(".", "").lstrip("0")) == 18:
            out.append(bits_of(x))
    return signed(out, rng)


def above_max15(rng):
    """The doubles above 1.797693134862315e308, whose t15 reads back as infinity, and the ones
    just below."""
    top = 0x7FEFFFFFFFFFFFFF
    out = [top - k for k in range(0, 16)]
    return out + [b | SIGN for b in out]


def smallest_normals(rng):
    """The smallest normals, whose read-back may be subnormal."""
    out = [(1 << 52) + k for k in range(0, 4096)]
    out += [(1 << 52) + rng.randrange(0, 1 << 20) for _ in range(6000)]
    out += [((rng.randrange(1, 40)) << 52) | rng.getrandbits(52) for _ in range(6000)]
    return signed(out, rng)


def specials():
    return [1, 2, (1 << 52) - 1, SIGN | 1, SIGN | ((1 << 51) + 12345), 1 << 51, 0x7FF0000000000000, 0xFFF0000000000000,
            0x7FF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF] + [random.Random(9).getrandbits(52) | 1
                                                                            for _ in range(50)]


@functools.lru_cache(maxsize=None)
def corpus():
    """label -> tuple of patterns; about 200,000 values in all."""
    rng = random.Random(20)
    c = {
        "powers_of_two": powers_of_two(rng),
        "powers_of_ten": powers_of_ten(rng),
        "below_powers_of_ten": below_powers_of_ten(rng),
        "shape_switches": shape_switches(rng),
        "integer_edges": integer_edges(rng),
        "class15": class15(rng, 60000),
        "random_bits": random_bits(rng, 80000),
        "ties15": ties15(rng, 8000),
        "ties17": ties17(rng, 8000),
        "above_max15": above_max15(rng),
        "smallest_normals": smallest_normals(rng),
        "subnormals": specials(),
    }
    for dist, bs in ulps_away(rng, 1500).items():
        c["ulps_away_%d" % dist] = signed(bs, rng)
    return {k: tuple(v) for k, v in c.items()}


def check_texts(label_texts, want_of):
    """Holds the texts of `label -> [text or None (DEFER)]` against the rules: never a wrong byte,
    DEFER only where the conditions allow.  Returns label -> DEFER count."""
    counts = {}
    for label, bs in corpus().items():
        got = label_texts[label]
        assert len(got) == len(bs), label
        defers = 0
        for b, g in zip(bs, got):
            w = want_of(b)
            if g is None:
                defers += w is not None
                continue
            assert g == w, (label, hex(b), g, w)
        counts[label] = defers
        if label == "subnormals":
            continue
        if label in ZERO_DEFER:
            assert defers == 0, (label, defers)
        assert defers * 10000 <= len(bs), (label, defers, len(bs))
    return counts
