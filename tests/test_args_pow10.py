"""The frame args' decimal to double conversion (rpc_amd/csrc/frames_args.h: args_number, the
exact path and Eisel-Lemire over rpc_amd/csrc/pow10_table.h) against Python's float(), which is
correctly rounded.  The committed table is the generator's output (tools/gen_pow10.py, exact
integer arithmetic); the conversion runs in the CPU emulator (tests/cpu_emu/args_emu.cpp num),
which compiles the kernel's own source.  Every string of at most 19 significant digits gives
float()'s bits; DEFER occurs only where float() gives zero, a subnormal or an infinity."""
import math
import os
import random
import struct
import subprocess
import sys

import args_cases as ac
from test_args_emu import args_emu  # noqa: F401  (a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_table_is_the_generators_output():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_pow10
    finally:
        sys.path.pop(0)
    assert open(gen_pow10.HEADER).read() == gen_pow10.render()
    t = gen_pow10.table()
    assert len(t) == 651 and all(1 << 127 <= c < 1 << 128 for c in t)
    assert t[342] == 1 << 127 and t[342 + 27] == 5**27 << (127 - (5**27).bit_length() + 1)


def convert(args_emu, texts):  # noqa: F811
    exe, d = args_emu
    path = str(d / "numbers.txt")
    open(path, "w").write("".join(t + "\n" for t in texts))
    p = subprocess.run([exe, "num", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split()
    assert len(out) == len(texts)
    return out


def hold(args_emu, texts):  # noqa: F811
    """Every text converts to float()'s bits or, where float() is not a normal double (nor the
    zero of an all-zero text), defers.
    Returns the number of deferred texts."""
    deferred = 0
    for text, got in zip(texts, convert(args_emu, texts)):
        f = float(text)
        zero = not text.lstrip("-").lower().split("e")[0].replace(".", "").strip("0")  # every digit is 0: +-0
        normal = zero or (not math.isinf(f) and abs(f) >= 2.0 ** -1022)
        want = "%016x" % struct.unpack("<Q", struct.pack("<d", f))[0] if normal else "DEFER"
        assert got == want, (text, got, want)
        assert (got == "DEFER") == (ac.f64_of(text.encode()) is None), text  # (the rules agree)
        deferred += not normal
    return deferred


def ties(rng, count):
    """Integers exactly halfway between two neighbouring doubles above 2^53, below 10^19."""
    out = []
    while len(out) < count:
        s = rng.randrange(1, 11)
        t = (2 * rng.randrange(2**52, 2**53) + 1) << (s - 1)
        if t < 10**19:
            out.append(t)
    return out


def test_digit_strings(args_emu):  # noqa: F811
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
    assert 300 < hold(args_emu, texts) < 6000  # (exponents below about -308 leave the normal doubles)


def test_integers_and_ties(args_emu):  # noqa: F811
    """Integers in [2^53, 10^19), exact ties between neighbouring doubles above 2^53, the same
    with e-1 .. e-25 appended, and the ties that a negative exponent leaves exact."""
    rng = random.Random(0x7135)
    ints = [rng.randrange(2**53, 10**19) for _ in range(20000)]
    tied = ties(rng, 20000)
    assert all(float(t - 1) != float(t + 1) for t in tied[:100])
    texts = [str(v) for v in ints + tied]
    texts += ["%de-%d" % (v, rng.randrange(1, 26)) for v in ints[:10000] + tied]
    for k in range(1, 5):  # m + 1/2 ulp for a double m of [2^(53-k), 2^(54-k)): (2m' + 1) * 5^k e-k
        half = [(2 * rng.randrange(2**52, 2**53) + 1) * 5**k for _ in range(3000)]
        texts += ["%de-%d" % (v, k) for v in half if v < 10**19]
    texts.append("63863781979156355e-1")
    assert all(len(t.split("e")[0]) <= 19 for t in texts)
    assert hold(args_emu, texts) == 0
