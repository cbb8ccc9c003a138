"""The frame args' decimal to double conversion (rpc_amd/csrc/frames_args.h: args_number, the
exact path and Eisel-Lemire over rpc_amd/csrc/pow10_table.h) against Python's float(), which is
correctly rounded.  The committed table is the generator's output (tools/gen_pow10.py, exact
integer arithmetic); the conversion runs in the CPU emulator (tests/cpu_emu/args_emu.cpp num),
which compiles the kernel's own source.  Every string of at most 19 significant digits gives
float()'s bits; DEFER occurs only where float() gives zero, a subnormal or an infinity.

The strings come from tests/args_numbers.py; tests/test_frames_args_numbers.py converts the same
ones on the device.  The tests without the emulator hold that module's lists to the conditions
the device test counts on."""
import math
import os
import struct
import subprocess
import sys

import args_cases as ac
import args_fuzz as af
import args_numbers as an
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


def test_digit_strings(args_emu):  # noqa: F811
    """Fixed-seed strings of 1 to 19 digits with a decimal exponent in [-320, 289], plain and
    with a point, a sign, leading zeros and every exponent form."""
    texts = list(an.digit_strings())
    assert 300 < hold(args_emu, texts) < 6000  # (exponents below about -308 leave the normal doubles)


def test_integers_and_ties(args_emu):  # noqa: F811
    """Integers in [2^53, 10^19), exact ties between neighbouring doubles above 2^53, the same
    with e-1 .. e-25 appended, and the ties that a negative exponent leaves exact."""
    texts, tied = an.integers_and_ties()
    assert all(float(t - 1) != float(t + 1) for t in tied[:100])
    assert all(len(t.split("e")[0]) <= 19 for t in texts)
    assert hold(args_emu, list(texts)) == 0


# ---- the lists chosen to reach each branch (tests/args_numbers.py) --------------------------
def test_branch_names_the_path():
    """The integer model that chooses inputs, on texts whose path is known by hand."""
    for text, want in [("0e5", ("zero", 5)), ("-0.000", ("zero", -3)), ("1e22", ("exact", 22)), ("0.001", ("exact", -3)),
                       ("9007199254740991e-22", ("exact", -22)), ("9007199254740992e-22", "el*"), ("1e23", "el*"),
                       ("9007199254740993", "el*"), ("1.5e-23", "el*"), ("1" * 20, ("many", 0)),
                       ("1.0000000000000000000", ("many", -19)), ("0." + "0" * 30 + "5", "el*"), ("1e309", ("range", 309)),
                       ("1e-343", ("range", -343)), ("0.1e309", "el*"), ("1e999999", ("range", 999999))]:
        got = an.branch(text)
        assert got == want or (want == "el*" and got[0] in ("el", "el2")), (text, got)
    assert an.branch("0." + "0" * 30 + "5")[1] == -31 and an.branch("12.5E+3")[1] == 2
    assert an.deferral_bounds(["1", "0e9", "1e400", "1e-400", "4.9e-324", "1" * 20, "1" * 20 + "e400"]) == (4, 5)


def test_second_product_reaches_every_exponent():
    """Every effective exponent of [-326, 304] has a text that takes the second product and
    gives a normal double (for |q| <= 22 with w >= 2^53: below it the exact path converts), and
    at least 100 texts carry from the second product into the high word."""
    texts = an.second_product()
    got = [an.branch(t) for t in texts]
    assert all(b == "el2" for b, _ in got)
    assert all(2.0 ** -1022 <= abs(float(t)) < math.inf for t in texts)
    assert {q for _, q in got} >= set(an.EL2_Q)
    assert all(int(an.parts(t)[0]) >= 2 ** 53 for t, (_, q) in zip(texts, got) if abs(q) <= 22)
    assert sum(map(an.carries, texts)) >= 100
    assert any(an.parts(t)[1] and an.parts(t)[2] for t in texts)  # (fraction digits and an exponent in one text)
    # A wrong low word is noticed: where 19-digit w of [2^63, 10^19) are normal doubles, flipping either of the
    # low word's top two bits changes the carry of some text at that exponent whose double depends on the carry
    # (near_carry puts such texts next to the carry on both sides).  Not claimed for |q| <= 5: 5^|q| has at
    # most 12 bits there, the product's low part takes few values, and at q = 0 no w below 10^19 reaches the
    # carry at all.
    assert all((an.carry_margin(t) >= 0) == an.carries(t) for t in texts[:200])
    by_q = {}
    for t, (_, q) in zip(texts, got):
        w = int(an.parts(t)[0])
        if an.decisive(t):
            by_q.setdefault(q, []).append(w << (64 - w.bit_length()))
    assert sum(1 for t in texts if an.decisive(t) and an.carries(t)) >= 100
    for q in range(-326, 290):
        c = an.table()[q + 342]
        for bit in (63, 62) if abs(q) > 5 else ():
            wrong = (c & an.M64) ^ (1 << bit)
            assert any(((w * (c >> 64) & an.M64) + (w * (c & an.M64) >> 64) > an.M64) !=
                       ((w * (c >> 64) & an.M64) + (w * wrong >> 64) > an.M64) for w in by_q[q]), (q, bit)


def test_corpus_conditions():
    """What the device test counts on the entries it sends, known here from float() and the
    integer model alone: the divides of the exact path, the deferrals, and the integer edges."""
    texts = an.f64_corpus()
    assert len(texts) == len(an.digit_strings()) + len(an.integers_and_ties()[0]) + 5000 + len(an.second_product()) + \
        len(an.exact_edges()) + len(an.normal_edges()) + len(an.int_edges())
    paths = [an.branch(t) for t in texts]
    assert sum(1 for b, q in paths if b == "exact" and q < 0) >= 40000
    assert sum(1 for b, q in paths if b == "exact" and q > 0) >= 10000
    assert {b for b, _ in paths} == {"zero", "exact", "el", "el2", "many", "range"}
    fewest, most = an.deferral_bounds(texts)
    assert 1000 < fewest <= most < len(texts) // 20
    assert fewest <= sum(ac.f64_of(t.encode()) is None for t in texts) <= most
    ints = an.int_corpus()
    for t, inside in ((ac.I32, 31), (ac.I64, 63)):
        slots = [ac.convert(t, "number", x.encode(), False, 0) for x in ints]
        assert sum(s is None for s in slots) > 1000 and sum(s is not None for s in slots) > 1000
        signed = {(s ^ (1 << 63)) - (1 << 63) for s in slots if s is not None}
        assert signed >= {-2 ** inside, 2 ** inside - 1 if t == ac.I32 else 2 ** 63 - 1024}  # (both ends of the type)
    assert set(ints) >= {"2147483647", "2147483648", "-2147483648", "-2147483649", "9223372036854775808",
                         "-9223372036854775808"}
    assert set(ints) >= {str(v) for v in af.EDGES}


def test_second_product(args_emu):  # noqa: F811
    """The second product at every exponent, with and without its carry: all normal doubles."""
    assert hold(args_emu, list(an.second_product())) == 0


def test_exact_edges(args_emu):  # noqa: F811
    """The exact path's divide and multiply on both sides of w = 2^53 and |q| = 22."""
    texts = list(an.exact_edges())
    assert sum(1 for t in texts if an.branch(t)[0] == "exact") >= 50000
    assert hold(args_emu, texts) == 0


def test_normal_edges(args_emu):  # noqa: F811
    """Around the smallest normal and the largest double both outcomes occur, and each text of at
    most 19 digits defers exactly where float() leaves the normal doubles; a text of more
    digits defers whatever its value."""
    texts = an.normal_edges()
    short = [t for t in texts if len(an.parts(t)[0]) <= 19]
    many = [t for t in texts if len(an.parts(t)[0]) > 19]
    fewest, most = an.deferral_bounds(short)
    assert fewest == most and 200 < fewest < len(short) - 200
    assert hold(args_emu, short) == fewest
    assert len(many) >= 20 and all(got == "DEFER" for got in convert(args_emu, many))
    assert all(ac.f64_of(t.encode()) is None for t in many)
    assert "%016x" % (1 << 52) in convert(args_emu, ["2225073858507201383e-326"])  # (the carry into the smallest normal)


def test_int_edges(args_emu):  # noqa: F811
    """The number texts of the integer columns, as doubles."""
    texts = an.int_edges()
    short = [t for t in texts if len(an.parts(t)[0]) <= 19]
    many = [t for t in texts if len(an.parts(t)[0]) > 19]
    assert hold(args_emu, short) == an.deferral_bounds(short)[0]
    assert many and all(got == "DEFER" for got in convert(args_emu, many))
