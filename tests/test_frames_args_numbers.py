"""The frame args' number conversions on the GPU (rpc_frames_args_device): the
strings the CPU emulator converts (tests/args_numbers.py, tests/test_args_pow10.py) through the
kernel itself -- its 64 x 64 multiply, its table in device memory, the f64 divide and multiply
and the integer conversions the gfx950 back end emits -- against float() for the F64 column and
the plain rules (tests/args_cases.py) for the I32 and I64 columns.

A schema of three methods with one parameter "v" each (F64, I32, I64), width 1; every span is
{"v":T}, or with a second member behind a blank or a comma, so that the number ends on each byte
that can end one.  args_numbers.branch only picks and counts inputs; no expected value is its."""
import functools
import random
from collections import Counter
from typing import NamedTuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
import args_numbers as an  # noqa: E402
import route_cases as rc  # noqa: E402
from test_frames_args import dev_entries, dev_schema, rows_of  # noqa: E402
from test_frames_route import dev_bytes  # noqa: E402

F, I, L = range(3)
METHODS = [(b"f", [(b"v", ac.F64)]), (b"i", [(b"v", ac.I32)]), (b"l", [(b"v", ac.I64)])]
SCHEMA = ac.schema_of(METHODS)
FRAMES = (b'{"v":%s}', b'{"v":%s ,"z":0}', b'{"v":%s,"z":0}')
INTERNAL = -32603


class Item(NamedTuple):
    method: int
    text: str
    frame: int  # (fixed per text: a third of the texts each)


class Batch(NamedTuple):
    items: list
    buf: bytes
    entries: list
    status: np.ndarray  # expected, from float() and the rules per text
    reply: np.ndarray
    slot: np.ndarray


def expected(item):
    """(status, reply status, slot) of one item, from its text alone."""
    t = item.text.encode()
    slot = ac.f64_of(t) if item.method == F else ac.convert(SCHEMA.types[item.method], "number", t, False, 0)
    return (ac.DEFER, INTERNAL, 0) if slot is None else (ac.OK, 0, slot)


def batch(items):
    """The items' spans back to back in the order given, one entry each, and the columns wanted."""
    buf, entries = bytearray(b"###"), []
    for it in items:
        span = FRAMES[it.frame] % it.text.encode()
        entries.append((len(buf), len(span), rc.CALL, it.method, 0, len(span)))
        buf += span + b"\0"
    want = [expected(it) for it in items]
    return Batch(items, bytes(buf), entries, np.array([w[0] for w in want], dtype=np.uint8),
                 np.array([w[1] for w in want], dtype=np.int32), np.array([w[2] for w in want], dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def f64_items():
    return tuple(Item(F, t, k % 3) for k, t in enumerate(an.f64_corpus()))


@functools.lru_cache(maxsize=None)
def int_items():
    return tuple(Item(m, t, (k + m) % 3) for k, t in enumerate(an.int_corpus()) for m in (I, L))


@functools.lru_cache(maxsize=None)
def paths():
    """branch() of every F64 item (to count and to report with; never to expect with)."""
    return {it.text: an.branch(it.text) for it in f64_items()}


@functools.lru_cache(maxsize=None)
def shuffled():
    items = list(f64_items())
    random.Random(0x5A0FF1E).shuffle(items)
    return batch(items)


@functools.lru_cache(maxsize=None)
def uniform():
    return batch(sorted(f64_items(), key=lambda it: paths()[it.text]))


@functools.lru_cache(maxsize=None)
def integers():
    items = list(int_items())
    random.Random(0x1A7E6E5).shuffle(items)
    return batch(items)


def run(b, entries=None, mis=0):
    """(status, reply status, slots) columns of the device for the batch's entries."""
    entries = b.entries if entries is None else entries
    off, ln, route = dev_entries(entries)
    r = rpc_amd.frames_args(dev_bytes(b.buf, mis), off, ln, route, dev_schema(SCHEMA), width=1)
    torch.cuda.synchronize()
    assert tuple(r.slots.shape) == (1, len(entries))
    return r


def hold(b, mis=0):
    """The device's three columns equal the expected ones; the first 20 that do not are printed
    with both bit patterns and the text's path.  Returns the device's status column."""
    r = run(b, mis=mis)
    st = r.status.cpu().numpy().view(np.uint8)
    rs = r.reply_status.cpu().numpy().view(np.int32)
    sl = r.slots.cpu().numpy().view(np.uint64)[0]
    bad = np.flatnonzero((st != b.status) | (rs != b.reply) | (sl != b.slot))
    for k in bad[:20]:
        it = b.items[k]
        print("mismatch: method %d text %s frame %d: got status %d reply %d slot %016x, want %d %d %016x, path %s" %
              (it.method, it.text[:80], it.frame, st[k], rs[k], sl[k], b.status[k], b.reply[k], b.slot[k],
               an.branch(it.text)))
    assert len(bad) == 0, "%d of %d entries differ" % (len(bad), len(b.items))
    return st


def f64_conditions(b, st):
    """The corpus conditions on the entries actually sent and the statuses the device gave."""
    assert 190000 <= len(b.items) <= 260000 and max(e[1] for e in b.entries) > 400
    assert sum(1 for e in b.entries if e[1] < 60) > len(b.entries) * 0.99
    path = [paths()[it.text] for it in b.items]
    ok = st == ac.OK
    el2 = [(it, q) for it, (p, q), good in zip(b.items, path, ok) if p == "el2" and good]
    assert {q for _, q in el2} >= set(an.EL2_Q)
    assert sum(1 for it, _ in el2 if an.carries(it.text) and an.decisive(it.text)) >= 100  # (the carry rounds these)
    assert sum(1 for p, q in path if p == "exact" and q < 0) >= 40000
    fewest, most = an.deferral_bounds([it.text for it in b.items])
    assert fewest <= int((st == ac.DEFER).sum()) <= most and int(ok.sum()) + int((st == ac.DEFER).sum()) == len(st)
    assert Counter(it.frame for it in b.items).keys() == {0, 1, 2}
    return len({q for _, q in el2})


@pytest.mark.parametrize("mis", [0, 5])
def test_doubles_match_float(mis):
    """Every text of the seven lists on the F64 method, shuffled, so that a wave holds lanes on
    the exact path, in Eisel-Lemire, in its second product and deferring side by side: float()'s
    bits, or DEFER where the rules say so.  Among the entries sent, every effective exponent
    of [-326, 304] takes the second product and converts (631 exponents, and 305 beside them), at
    least 100 second products carry where the carry decides the rounding, and at least 40,000
    entries divide on the exact path."""
    b = shuffled()
    waves = [{paths()[it.text][0] for it in b.items[k:k + 64]} for k in range(0, 64 * 200, 64)]
    assert sum(1 for w in waves if w >= {"exact", "el", "el2"}) >= 150  # (the paths do sit side by side)
    st = hold(b, mis)
    assert f64_conditions(b, st) >= len(an.EL2_Q)


def test_same_corpus_in_uniform_waves():
    """The same entries sorted by path, then by effective exponent: neighbouring lanes take the
    same path and read neighbouring words of the table."""
    b = uniform()
    assert sorted(b.items) == sorted(shuffled().items)
    f64_conditions(b, hold(b, 3))


def test_integers_from_number_text():
    """The integer edges, the ties and the integers above 2^53 on the I32 and the I64 method:
    trunc of float()'s double inside the type's range, else DEFER."""
    b = integers()
    texts = {it.text for it in b.items}
    assert texts >= {str(v) for v in (2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**63, -2**63)}
    for m in (I, L):
        mine = np.array([it.method == m for it in b.items])
        assert (b.status[mine] == ac.OK).sum() > 1000 and (b.status[mine] == ac.DEFER).sum() > 1000
    by = {(it.method, it.text): (int(st), int(s)) for it, st, s in zip(b.items, b.status, b.slot)}
    assert by[I, "2147483647.5"] == (ac.OK, 2**31 - 1) and by[I, "-2147483648.5"] == (ac.OK, 2**64 - 2**31)
    assert by[I, "2147483647.999999999"] == (ac.DEFER, 0)  # (the nearest double is 2^31)
    assert by[L, "-9223372036854775808"] == (ac.OK, 2**63) and by[L, "9223372036854774784"] == (ac.OK, 2**63 - 1024)
    assert by[L, "9223372036854775295"] == (ac.OK, 2**63 - 1024) and by[L, "9223372036854775296"] == (ac.DEFER, 0)
    hold(b, 9)


def test_shortcut_is_the_plain_rules():
    """A fixed sample of the entries above, all three methods in all three framings, through the
    full plain rules (args_cases.args_entries): they give what the per-text shortcut expects,
    and the device's rows are theirs field for field."""
    rng = random.Random(0x5A3B1E)
    for b, count in ((shuffled(), 1500), (integers(), 1500)):
        picks = sorted(rng.sample(range(len(b.items)), count))
        longest = max(range(len(b.items)), key=lambda k: b.entries[k][1])
        picks = sorted(set(picks) | {longest})
        entries = [b.entries[k] for k in picks]
        methods = (F,) if b is shuffled() else (I, L)
        assert {(b.items[k].method, b.items[k].frame) for k in picks} == {(m, f) for m in methods for f in range(3)}
        rules = ac.args_entries(b.buf, entries, SCHEMA, 1)
        assert rules == [(int(b.status[k]), int(b.reply[k]), (int(b.slot[k]),)) for k in picks]
        assert rows_of(run(b, entries, mis=1), len(entries)) == rules
        assert {r[0] for r in rules} == {ac.OK, ac.DEFER}
