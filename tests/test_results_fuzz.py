"""The frame results' rules against the live reference: replies from the reference's own
dispatcher (oracle/_ref/ref_dispatch) to tests/test_values_fuzz.py's requests, read by the
reference's decoder and restated generated-client lines (tests/results_ref.py).  CPU only;
skipped where the reference tree is absent.

Two seeds of 12,000 rows, half canonical (the dispatcher's replies as they are) and half mutated
as resolve_cases.mutation_set mutates (one byte replaced, inserted or deleted, or the body cut
short).  Each reply goes through the resolve's rules, then the results' rules with the result
type of the request's method.  Every answer that is not DEFER is what the generated client
returns; MISMATCH and ABSENT are its default.  On the canonical half DEFER appears only in two
named classes, counted from the driver's facts; on the mutated half at most half of the rows may
defer (resolve or results)."""
import math
import random
import struct

import pytest

import args_cases as ac
import resolve_cases as rv
import results_cases as rs
import results_ref
import values_fuzz as vf

SEEDS = [0xC3751, 0xC3752]
ROWS = 12000
#: resolve_cases.mutation_set's four operations, weighted so that at most half of the rows leave
#: the strict subset (a cut always does: one row in ten, not in four; a replaced byte in five;
#: a digit or a letter far more often than a structural byte): with its own pool and even
#: weights 60 % of the rows deferred
POOL = b'{}[]",:\\ \t\n-+.eEtfnIiDdRrEe\x00\x7f\x80' + b"0123456789abcxyz" * 8
HOW = (0, 0, 0, 0, 0, 1, 1, 2, 2, 3)
#: mul_double's (a, b) whose product is subnormal (the last: a small normal, which decodes)
TINY = [(b"1e-200", b"1e-120"), (b"-2.5e-160", b"3e-160"), (b"4.9e-324", b"1"), (b"1e-161", b"-1e-161"),
        (b"2.2250738585072009e-308", b"1"), (b"1.5e-300", b"1e-10"), (b"1e-150", b"1e-150")]


def mutate(rng, body):
    b = bytearray(body)
    how, at = rng.choice(HOW), rng.randrange(len(b))
    if how == 0:
        b[at] = rng.choice(POOL)
    elif how == 1:
        b.insert(at, rng.choice(POOL))
    elif how == 2:
        del b[at]
    else:
        del b[at:]
    return bytes(b) or b"{"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = results_ref.build(tmp_path_factory.mktemp("ref_results"))
    if exe is None:
        pytest.skip("the reference tree is absent")
    return exe


def replies_of(seed):
    from oracle import oracle
    rows, _ = vf.rows(seed, ROWS // 2 - len(TINY))
    # (products below the smallest normal: the one DEFER class a canonical reply of this IDL can
    # reach -- no method returns a string the caller chooses, so none can need an escape)
    tiny = [b'{"jsonrpc":"2.0","method":"mul_double","params":{"a":%s,"b":%s},"id":%d}' % (a, b, 900000 + k)
            for k, (a, b) in enumerate(TINY)]
    got = oracle.ref_dispatch(vf.bodies_of(rows) + tiny)
    if got is None:
        pytest.skip("oracle/_ref/ref_dispatch is not built (needs the reference tree)")
    types = [vf.RESULT_TYPES[r.method] for r in rows] + [rs.F64] * len(tiny)
    replies = [bytes(g) for g in got]
    assert all(replies), "a request of the corpus was not answered"
    return types, replies


def rules(body, t):
    """(resolve kind, results Row or None): the body as the one entry of a call whose only slot
    waits for its id."""
    row = rv.decode_body(body)
    if row[0] != rv.UNKNOWN:
        return row[0], None
    entry = (0, len(body), rv.MATCHED, 0, *row[2:])
    return rv.MATCHED, rs.results_entries(body, [entry], [0], [t])[0]


def not_normal(node):
    d = struct.unpack("<d", struct.pack("<Q", node.bits))[0]
    return d != 0 and (math.isinf(d) or abs(d) < 2.0 ** -1022)


def hold(body, t, r, f):
    """One decoded reply's answers against the driver's facts."""
    assert f.rc == 0, body
    if r.status != rs.DEFER:
        want = results_ref.client_value(t, f.result)
        assert want is not None, (body, r)  # (an undefined cast has to defer)
        if want[0] == "str":
            got = body[r.value & 0xFFFFFFFF:][:r.value >> 32] if r.status == rs.OK else None
            assert got == want[1], (body, r, want)
        else:
            assert r.value == want[1], (body, r, want)
        if r.status in (rs.MISMATCH, rs.ABSENT):
            assert r.value == 0
    if r.error_status == rs.OK:
        assert f.code.is_number and f.message.is_string, body
        d = struct.unpack("<d", struct.pack("<Q", f.code.bits))[0]
        assert r.error_code == int(d), body
        assert body[r.error_message & 0xFFFFFFFF:][:r.error_message >> 32] == f.message.string, body
    elif r.error_status in (rs.MISMATCH, rs.ABSENT):
        assert not (f.code.there and f.code.is_number and f.message.there and f.message.is_string), body


@pytest.mark.parametrize("seed", SEEDS)
def test_rules_hold_against_the_reference(seed, driver):
    types, replies = replies_of(seed)
    rng = random.Random(seed ^ 0x5EED)
    mutated = [mutate(rng, b) for b in replies]
    facts = results_ref.run(driver, replies + mutated)
    # the canonical half
    escaped = subnormal = 0
    for body, t, f in zip(replies, types, facts):
        kind, r = rules(body, t)
        string_escape = f.result.is_string and any(c in b'"\\' or c < 0x20 for c in f.result.string)
        if kind == rv.DEFER:  # the route's strict subset: a \u escape in the reply's string
            assert string_escape, body
            escaped += 1
            continue
        assert kind == rv.MATCHED, body
        hold(body, t, r, f)
        if r.status == rs.DEFER:
            if t in (rs.STR, rs.I64) and string_escape:
                escaped += 1
            else:
                assert t == rs.F64 and f.result.is_number and not_normal(f.result), (body, r)
                subnormal += 1
        assert r.error_status != rs.DEFER, body
    want_escaped = sum(1 for t, f in zip(types, facts) if f.result.is_string and t in (rs.STR, rs.I64) and
                       any(c in b'"\\' or c < 0x20 for c in f.result.string))
    want_subnormal = sum(1 for t, f in zip(types, facts) if t == rs.F64 and f.result.is_number and not_normal(f.result))
    print("canonical DEFER: %d escaped strings, %d doubles outside the normal range, of %d" %
          (escaped, subnormal, len(replies)))
    assert (escaped, subnormal) == (want_escaped, want_subnormal) and subnormal == len(TINY) - 1
    # the mutated half
    deferred = decided = 0
    for body, t, f in zip(mutated, types, facts[len(replies):]):
        kind, r = rules(body, t)
        if kind == rv.DEFER or (r is not None and rs.DEFER in (r.status, r.error_status)):
            deferred += 1
        if r is not None:
            hold(body, t, r, f)
            decided += 1
    print("mutated: %d of %d defer, %d reach the results" % (deferred, len(mutated), decided))
    assert 2 * deferred <= len(mutated)
