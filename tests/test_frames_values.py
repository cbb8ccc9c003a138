"""Frame values on the GPU (rpc_frames_values_device): typed results and params
as JSON text, against the plain Python rules of tests/values_cases.py byte for byte and word for
word, and chained: values -> reply against the rules' replies, values -> request."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
import reply_cases as rp  # noqa: E402
import request_cases as rq  # noqa: E402
import route_cases as rc  # noqa: E402
import values_cases as vc  # noqa: E402
from test_frames_args import dev_schema  # noqa: E402
from test_frames_unpack import DEV, GUARD, T, dev_bytes, host, to_dev  # noqa: E402

FILL = 0xA5


def dev_inputs(entries, width, given=(True, True, True)):
    """(method, slots, mode, status, str_base, text_offsets, text_lens) on the device; mode, status
    and str_base are None where `given` says the caller passes none."""
    n = len(entries)
    slots = np.zeros((width, n), dtype=np.uint64)
    for i, e in enumerate(entries):
        for k in range(min(width, len(e.slots))):
            slots[k, i] = e.slots[k] & vc.M64
    col = lambda f, wide, narrow: to_dev(np.array([f(e) for e in entries], dtype=wide).view(narrow))  # noqa: E731
    return (col(lambda e: e.method & 0xFFFF, np.uint16, np.int16), to_dev(slots.view(np.int64)),
            col(lambda e: e.mode, np.uint8, np.uint8) if given[0] else None,
            col(lambda e: e.status, np.int32, np.int32) if given[1] else None,
            col(lambda e: e.str_base & vc.M64, np.uint64, np.int64) if given[2] else None,
            col(lambda e: e.text_off & vc.M64, np.uint64, np.int64), col(lambda e: e.text_len, np.uint32, np.int32))


def dev_form(form, schema, rtypes):
    return dev_schema(schema) if form == vc.FORM_PARAMS else to_dev(np.array(rtypes, dtype=np.uint8))


def placed(strings, texts, mis, place):
    """The two source buffers on the device at their misalignments; with `place` both lie in one
    allocation, "texts_first" or "strings_first" in memory, 48 bytes of 0xEE between them."""
    if place is None:
        return dev_bytes(strings, mis[0]), dev_bytes(texts, mis[1])
    first, second = (texts, strings) if place == "texts_first" else (strings, texts)
    m1, m2 = (mis[1], mis[0]) if place == "texts_first" else (mis[0], mis[1])
    at2 = (m1 + len(first) + 48 + 15) // 16 * 16 + m2
    arena = np.full(at2 + len(second) + 64, 0xEE, dtype=np.uint8)
    arena[m1:m1 + len(first)] = np.frombuffer(first, dtype=np.uint8)
    arena[at2:at2 + len(second)] = np.frombuffer(second, dtype=np.uint8)
    d = to_dev(arena)
    a, b = d[m1:m1 + len(first)], d[at2:at2 + len(second)]
    assert a.data_ptr() % 16 == m1 and b.data_ptr() % 16 == m2 and a.data_ptr() < b.data_ptr()
    return (b, a) if place == "texts_first" else (a, b)


def run_gpu(entries, form, schema, rtypes, width, strings=vc.STRINGS, texts=vc.TEXTS, cap=None, mis=(0, 0, 0),
            have_texts=True, given=(True, True, True), what="", stream=None, place=None):
    """Builds the entries into a slice of a larger 0xA5-filled tensor and checks everything against
    values_cases.values_batch: the output byte for byte (0xA5 outside every written entry), the
    guard bytes on both sides and beyond out_cap, every per-entry word, the total and the count."""
    want_rows, chunks, total, ndefer = vc.values_batch(entries, form, schema, rtypes, width, strings, texts, cap, have_texts)
    nb = total if cap is None else cap
    big = torch.full((GUARD + mis[2] + nb + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = big[GUARD + mis[2]:GUARD + mis[2] + nb]
    assert nb == 0 or out.data_ptr() % 16 == mis[2]
    method, slots, mode, status, base, toff, tlen = dev_inputs(entries, width, given)
    d_strings, d_texts = placed(strings, texts, mis, place)
    r = rpc_amd.frames_values(method, slots, dev_form(form, schema, rtypes), form=form, mode=mode, status=status,
                              strings=d_strings, str_base=base, texts=d_texts if have_texts else None,
                              text_offsets=toff if have_texts else None, text_lens=tlen if have_texts else None, out=out,
                              stream=stream)
    if stream is not None:
        stream.synchronize()
    got = big.cpu().numpy()
    canvas = np.full(len(got), FILL, dtype=np.uint8)
    for at, txt, _ in chunks:
        if txt is not None:
            canvas[GUARD + mis[2] + at:GUARD + mis[2] + at + len(txt)] = np.frombuffer(txt, dtype=np.uint8)
    bad = np.nonzero(got != canvas)[0]
    assert bad.size == 0, (what, "first differing byte", int(bad[0]) - GUARD - mis[2])
    rows = list(zip(host(r.status, np.uint8), host(r.reply_status, np.int32), host(r.value_offsets, np.uint64),
                    host(r.value_lens, np.uint32)))
    for k, (g, w) in enumerate(zip(rows, want_rows)):
        assert g == w, (what, k, entries[k], g, w)
    assert len(rows) == len(want_rows)
    assert int(r.total.cpu()[0]) == total and int(r.ndefer.cpu()[0]) == ndefer, what
    return r, want_rows, chunks


def test_case_table_result():
    """Every rule, status and header example of the RESULT table, one method per case."""
    types, entries = vc.result_entries()
    _, rows, _ = run_gpu(entries, vc.FORM_RESULT, ac.IDL, types, 1, what="result table")
    assert {r[0] for r in rows} == {vc.NONE, vc.OK, vc.TEXT, vc.DEFER, vc.RANGE, vc.BAD_SCHEMA}
    for (name, _, _, st, txt), row in zip(vc.RESULT_CASES, rows):
        assert (row[0], row[3]) == (st, len(txt)), name
    run_gpu(entries, vc.FORM_RESULT, ac.IDL, types, 1, have_texts=False, what="no texts given")
    bare = [e._replace(status=0, str_base=0) for e in entries]
    run_gpu(bare, vc.FORM_RESULT, ac.IDL, types, 1, given=(True, False, False), what="no status, no base")
    run_gpu([e._replace(mode=vc.MODE_ENCODE) for e in bare], vc.FORM_RESULT, ac.IDL, types, 1, given=(False, False, False),
            what="no mode either")


def test_case_table_params():
    """The PARAMS table: the IDL, 0 and 8 parameters, a repeated name, the empty name, names that
    need an escape, each broken schema word, the precedence order; singly and as batches."""
    by = {}
    for what, schema, width, e in vc.params_cases():
        run_gpu([e], vc.FORM_PARAMS, schema, [], width, what=what)
        by.setdefault((id(schema), width), (schema, width, []))[2].append(e)
    for schema, width, es in by.values():
        run_gpu(es * 5, vc.FORM_PARAMS, schema, [], width, what="params batch")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_batch_sizes(n):
    types, entries = vc.result_entries()
    es = [entries[(7 * i) % len(entries)] for i in range(n)]
    run_gpu(es, vc.FORM_RESULT, ac.IDL, types, 1, what=("result", n))
    pe = [c[3] for c in vc.params_cases() if c[1] is vc.EXTRA]
    run_gpu([pe[(3 * i) % len(pe)] for i in range(n)], vc.FORM_PARAMS, vc.EXTRA, [], 8, what=("params", n))


def test_empty_batch():
    e = torch.empty(0, dtype=torch.int16, device=DEV)
    slots = torch.empty((1, 0), dtype=torch.int64, device=DEV)
    r = rpc_amd.frames_values(e, slots, to_dev(np.array([0], dtype=np.uint8)))
    assert r.total == 0 and r.values.numel() == 0 and int(r.ndefer.cpu()[0]) == 0


def test_one_byte_values_and_long_strings():
    """A few thousand one-byte values (a 16 KiB tile holds more entries than the LDS range
    stages), zero-size runs, and strings that cross tiles, scanned by the whole workgroup."""
    rng = random.Random(5)
    long1 = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz \xc3\xa9~") for _ in range(3 * T + 77))
    long2 = long1[:T + 5] + b'"' + long1[T + 6:2 * T]           # an escape deep inside: DEFER
    long3 = long1[100:400]
    strings = b"#" + long1 + long2 + long3 + b"x" * 300 + b"\\"
    a1, a2, a3 = 1, 1 + len(long1), 1 + len(long1) + len(long2)
    a4 = a3 + len(long3)
    types = [vc.I32, vc.STR, vc.BOOL]
    es = [vc.Entry(vc.MODE_ENCODE, 0, 0, (i % 10,)) for i in range(6000)]
    es += [vc.Entry(vc.MODE_NONE, 0, 0, (1,))] * 3000
    es += [vc.Entry(vc.MODE_ENCODE, 0, 1, (a1 | len(long1) << 32,)), vc.Entry(vc.MODE_ENCODE, 0, 1, (a2 | len(long2) << 32,)),
           vc.Entry(vc.MODE_ENCODE, 0, 1, (a3 | len(long3) << 32,)), vc.Entry(vc.MODE_ENCODE, 0, 1, (a4 | 301 << 32,)),
           vc.Entry(vc.MODE_ENCODE, 0, 1, (a4 | 300 << 32,)), vc.Entry(vc.MODE_ENCODE, 0, 2, (1,))]
    es += [vc.Entry(vc.MODE_ENCODE, 0, 1, (rng.randrange(1, len(long1)) | rng.randrange(257, 2000) << 32,)) for _ in range(200)]
    for mis in ((0, 0, 0), (7, 0, 13)):
        _, rows, _ = run_gpu(es, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, mis=mis, what=("long", mis))
        assert [r[0] for r in rows[9000:9005]] == [vc.OK, vc.DEFER, vc.OK, vc.DEFER, vc.OK]
    # several long strings in one entry, one copied middle per item
    sch = ac.schema_of([(b"m", [(b"first", vc.STR), (b"n", vc.I32), (b"second", vc.STR), (b"third", vc.STR)])])
    pe = [vc.Entry(vc.MODE_ENCODE, 0, 0, (a1 | len(long1) << 32, i, a3 | len(long3) << 32, (a1 + i) | (2 * T) << 32))
          for i in range(5)]
    pe.append(vc.Entry(vc.MODE_ENCODE, 0, 0, (a1 | len(long1) << 32, 5, a2 | len(long2) << 32, a3 | 5 << 32)))
    _, rows, _ = run_gpu(pe, vc.FORM_PARAMS, sch, [], 4, strings=strings, mis=(3, 0, 9), what="params long")
    assert [r[0] for r in rows] == [vc.OK] * 5 + [vc.DEFER]


def test_strings_the_whole_grid_scans():
    """Strings over 64 KiB go on the call's work list and are scanned by the whole grid: clean
    ones, one with a quote in its first, a middle and its last byte, two in one entry."""
    rng = random.Random(6)
    big = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz \xc3\xa9~") for _ in range(300000))
    bad = [big[:k] + b'"' + big[k + 1:200001] for k in (0, 131072 + 5, 200000)]
    strings = b"##" + big + b"".join(bad) + b"tail"
    at = [2, 2 + len(big)]
    for b in bad[:-1]:
        at.append(at[-1] + len(b))
    types = [vc.STR, vc.I32]
    es = [vc.Entry(vc.MODE_ENCODE, 0, 1, (7,)), vc.Entry(vc.MODE_ENCODE, 0, 0, (at[0] | len(big) << 32,))]
    es += [vc.Entry(vc.MODE_ENCODE, 0, 0, (a | 200001 << 32,)) for a in at[1:]]
    es += [vc.Entry(vc.MODE_ENCODE, 0, 0, ((at[1] + 1) | 65537 << 32,)), vc.Entry(vc.MODE_ENCODE, 0, 0, ((at[1] + 1) | 65536 << 32,)),
           vc.Entry(vc.MODE_ENCODE, 0, 1, (8,))]
    for mis in ((0, 0, 0), (9, 0, 3)):
        _, rows, _ = run_gpu(es, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, mis=mis, what=("grid scan", mis))
        assert [r[0] for r in rows] == [vc.OK, vc.OK, vc.DEFER, vc.DEFER, vc.DEFER, vc.OK, vc.OK, vc.OK]
    # many strings of two or three chunks each: the work list spreads them over the grid
    many = [vc.Entry(vc.MODE_ENCODE, 0, 0, (rng.randrange(0, len(strings) - 150000) | rng.randrange(65537, 150000) << 32,))
            for _ in range(300)]
    _, rows, _ = run_gpu(many, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, mis=(3, 0, 7), what="many long strings")
    assert min(sum(1 for r in rows if r[0] == st) for st in (vc.OK, vc.DEFER)) >= 30
    sch = ac.schema_of([(b"m", [(b"a", vc.STR), (b"n", vc.I32), (b"b", vc.STR)])])
    pe = [vc.Entry(vc.MODE_ENCODE, 0, 0, (at[0] | 100000 << 32, 1, (at[0] + 7) | 70000 << 32)),
          vc.Entry(vc.MODE_ENCODE, 0, 0, (at[0] | 100000 << 32, 2, at[2] | 200001 << 32)),
          vc.Entry(vc.MODE_ENCODE, 0, 0, (at[3] | 200001 << 32, 3, at[1] | 200001 << 32)),
          vc.Entry(vc.MODE_ENCODE, 0, 0, (at[0] | 5 << 32, 4, at[0] | 66000 << 32))]
    _, rows, _ = run_gpu(pe, vc.FORM_PARAMS, sch, [], 3, strings=strings, mis=(1, 0, 5), what="grid scan, params")
    assert [r[0] for r in rows] == [vc.OK, vc.DEFER, vc.DEFER, vc.OK]


def test_long_texts_and_strings_share_tiles():
    """TEXT entries of a few hundred bytes and some over a tile, beside strings in the same tiles:
    the aligned window into the texts, which the walker reaches through the strings' base
    pointer.  The texts before and behind the strings in memory, in allocations of their own,
    and without any strings buffer; string, text and output misalignments 0-15."""
    types, es, strings, texts = vc.long_text_case(tile=T)
    assert sum(1 for e in es if e.mode == vc.MODE_TEXT and e.text_len > T) >= 3
    for m in range(16):
        mis = ((m * 3 + 2) % 16, m, (m * 5 + 1) % 16)
        place = (None, "texts_first", "strings_first")[m % 3]
        run_gpu(es, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, texts=texts, mis=mis, place=place,
                what=("long texts", mis, place))
    only = [e for e in es if e.mode == vc.MODE_TEXT or e.method != 0]
    for mis in ((0, 0, 0), (0, 9, 3)):
        run_gpu(only, vc.FORM_RESULT, ac.IDL, types, 1, strings=b"", texts=texts, mis=mis, what=("no strings", mis))
    total = vc.values_batch(es, vc.FORM_RESULT, ac.IDL, types, 1, strings, texts)[2]
    for place in ("texts_first", "strings_first"):
        run_gpu(es, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, texts=texts, mis=(1, 2, 3), cap=total // 2,
                place=place, what=("long texts, half the room", place))
    # PARAMS form: TEXT entries beside objects with strings
    sch = ac.schema_of([(b"m", [(b"first", vc.STR), (b"n", vc.I32), (b"second", vc.STR)])])
    pe = [e if e.mode == vc.MODE_TEXT else vc.Entry(vc.MODE_ENCODE, 0, 0, (e.slots[0] if e.method == 0 else 5 << 32, k,
                                                                          (k % 100) | 300 << 32))
          for k, e in enumerate(es)]
    run_gpu(pe, vc.FORM_PARAMS, sch, [], 3, strings=strings, texts=texts, mis=(7, 11, 13), place="texts_first",
            what="long texts, params")


class Unread:
    """A strings buffer of a given length whose bytes the rules must not look at."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        raise AssertionError("a string byte was read")


def test_entry_over_32_bits_is_range_before_any_string_is_read():
    """Four strings of 1.1 GB in one object: over 32 bits, RPC_VALUES_RANGE from the slots alone --
    although the string holds a quote, which would be DEFER, and beside a subnormal, which is."""
    nb = 1100 * 1000 * 1000
    sch = ac.schema_of([(b"m", [(b"a", vc.STR), (b"b", vc.STR), (b"c", vc.STR), (b"d", vc.STR), (b"x", vc.F64)])])
    es = [vc.Entry(vc.MODE_ENCODE, 0, 0, (nb << 32,) * 4 + (vc.bits_of(1.5),)),
          vc.Entry(vc.MODE_ENCODE, 0, 0, (nb << 32,) * 4 + (1,)),                 # (a subnormal beside them)
          vc.Entry(vc.MODE_ENCODE, 0, 0, (5 << 32,) * 4 + (1,)),
          vc.Entry(vc.MODE_ENCODE, 0, 0, (7 | 5 << 32,) * 4 + (vc.bits_of(2.5),))]
    want = [vc.values_entry(e, vc.FORM_PARAMS, sch, [], 5, Unread(nb), b"")[0] for e in es[:3]]
    assert want == [vc.RANGE, vc.RANGE, vc.DEFER]
    strings = torch.full((nb,), ord("a"), dtype=torch.uint8, device=DEV)
    strings[nb // 2] = ord('"')
    method, slots, _, _, _, _, _ = dev_inputs(es, 5)
    out = torch.full((256,), FILL, dtype=torch.uint8, device=DEV)
    r = rpc_amd.frames_values(method, slots, dev_schema(sch), form=vc.FORM_PARAMS, strings=strings, out=out[:128])
    assert host(r.status, np.uint8) == [vc.RANGE, vc.RANGE, vc.DEFER, vc.OK]
    assert host(r.reply_status, np.int32) == [vc.INTERNAL] * 3 + [0] and int(r.ndefer.cpu()[0]) == 1
    text = b'{"a":"aaaaa","b":"aaaaa","c":"aaaaa","d":"aaaaa","x":2.5}'
    assert host(r.value_lens, np.uint32) == [0, 0, 0, len(text)] and int(r.total.cpu()[0]) == len(text)
    got = out.cpu().numpy().tobytes()
    assert got[:len(text)] == text and got[len(text):] == bytes([FILL]) * (256 - len(text))


def test_misalignments():
    """Output, string and text misalignments 0-15."""
    types, entries = vc.result_entries()
    pe = [c[3] for c in vc.params_cases() if c[1] is vc.EXTRA] * 2
    for m in range(16):
        mis = (m, (m * 7 + 3) % 16, (m * 5 + 1) % 16)
        run_gpu(entries, vc.FORM_RESULT, ac.IDL, types, 1, mis=mis, what=("result", mis))
        run_gpu(pe, vc.FORM_PARAMS, vc.EXTRA, [], 8, mis=mis, what=("params", mis))


def test_out_cap_and_canaries():
    """out_cap inside an entry and at its end: the entry that does not end inside it is not
    written, not even in part, and the bytes behind stay as they were."""
    types, entries = vc.result_entries()
    rows, _, total, _ = vc.values_batch(entries, vc.FORM_RESULT, ac.IDL, types, 1, vc.STRINGS, vc.TEXTS)
    ends = sorted({r[2] + r[3] for r in rows if r[3]})
    caps = {0, 1, total - 1, total, total + 9} | {e + d for e in ends[:6] + ends[-3:] for d in (-1, 0, 1)}
    for cap in sorted(c for c in caps if c >= 0):
        _, got, _ = run_gpu(entries, vc.FORM_RESULT, ac.IDL, types, 1, cap=cap, mis=(0, 0, 5), what=("cap", cap))
    assert any(r[0] == vc.NO_ROOM for r in vc.values_batch(entries, vc.FORM_RESULT, ac.IDL, types, 1, vc.STRINGS, vc.TEXTS, 30)[0])
    pe = [c[3] for c in vc.params_cases() if c[1] is vc.EXTRA]
    for cap in (0, 1, 2, 3, 50, 120, 121, 122, 300):
        run_gpu(pe, vc.FORM_PARAMS, vc.EXTRA, [], 8, cap=cap, what=("params cap", cap))


def test_layout_only_and_self_sizing():
    types, entries = vc.result_entries()
    rows, chunks, total, ndefer = vc.values_batch(entries, vc.FORM_RESULT, ac.IDL, types, 1, vc.STRINGS, vc.TEXTS)
    method, slots, mode, status, base, toff, tlen = dev_inputs(entries, 1)
    r = rpc_amd.frames_values(method, slots, dev_form(vc.FORM_RESULT, ac.IDL, types), mode=mode, status=status,
                              strings=dev_bytes(vc.STRINGS), str_base=base, texts=dev_bytes(vc.TEXTS), text_offsets=toff,
                              text_lens=tlen)
    assert r.total == total == r.values.numel()
    out = bytes(r.values.cpu().numpy())
    for at, txt, _ in chunks:
        if txt is not None:
            assert out[at:at + len(txt)] == txt
    assert host(r.status, np.uint8) == [w[0] for w in rows] and int(r.ndefer.cpu()[0]) == ndefer


def test_mutated_mixes():
    """Random mode, status and TEXT mixes over the IDL and the extra schemas, in both forms."""
    from test_values_emu import mutated_rows
    for k, (form, schema, rtypes, width, es) in enumerate(mutated_rows(random.Random(78), 1500)):
        run_gpu(es, form, schema, rtypes, width, mis=(k, 2 * k + 1, 3 * k + 2), what=("mutated", form, width))
        half = sum(r[3] for r in vc.values_batch(es, form, schema, rtypes, width, vc.STRINGS, vc.TEXTS)[0]) // 2
        run_gpu(es, form, schema, rtypes, width, cap=half, what=("mutated, half the room", form, width))


def test_values_then_reply():
    """values -> reply: the handlers' columns in, reply bodies out, against the rules' replies."""
    rng = random.Random(11)
    n = 700
    methods = [rng.randrange(0, 7) for _ in range(n)]
    strings = b"ok then" + bytes(range(0x20, 0x7f)).replace(b'"', b"").replace(b"\\", b"") + b'q"'
    rtypes = list(vc.IDL_RESULTS)
    rtypes[5] = vc.STR  # (a string result beside the IDL's)

    def slot(t):
        if t == vc.STR:
            at = rng.randrange(0, len(strings))
            return at | rng.randrange(0, len(strings) - at + 1) << 32
        if t == vc.F64:
            return vc.bits_of(rng.choice([rng.uniform(-1e9, 1e9), rng.random(), 0.1 + 0.2, 1e22, 5e-324, 3.0]))
        return rng.getrandbits(64)

    status = [rng.choice([0] * 8 + [-32602, -32603]) for _ in range(n)]
    es = [vc.Entry(vc.MODE_ENCODE, status[i], methods[i], (slot(rtypes[methods[i]]),)) for i in range(n)]
    kinds = [rng.choice([rc.CALL] * 8 + [rc.NOT_FOUND, rc.INVALID]) for _ in range(n)]
    ids = [rng.getrandbits(32) for _ in range(n)]
    rows, chunks, total, ndefer = vc.values_batch(es, vc.FORM_RESULT, ac.IDL, rtypes, 1, strings, b"")
    assert ndefer > 0
    method, slots, mode, st, base, _, _ = dev_inputs(es, 1)
    v = rpc_amd.frames_values(method, slots, dev_form(vc.FORM_RESULT, ac.IDL, rtypes), status=st, strings=dev_bytes(strings))
    r = rpc_amd.frames_reply(to_dev(np.array(kinds, dtype=np.uint8)), to_dev(np.array(ids, dtype=np.uint32).view(np.int32)),
                             v.values, v.value_offsets, v.value_lens, status=v.reply_status)
    values = b"".join(c[1] or b"" for c in chunks)
    case = rp.Case("chained", values, [(0, kinds[i], ids[i], rows[i][1], rows[i][2], rows[i][3]) for i in range(n)], None,
                   typed=False)
    want = rp.want_of(case, None)
    assert bytes(r.bodies.cpu().numpy()) == want.out
    assert host(r.status, np.uint8) == want.status and host(r.body_lens, np.uint32) == want.body_lens
    # a DEFER entry answers Internal error, never an empty result
    k = next(i for i in range(n) if rows[i][0] == vc.DEFER and kinds[i] == rc.CALL)
    assert b'"code":-32603' in want.chunks[k]


def test_values_then_request():
    """values -> request: params objects from typed columns, then the request bodies."""
    rng = random.Random(12)
    n = 500
    names = [m for m, _ in ac.IDL_METHODS]
    methods = [rng.randrange(0, 7) for _ in range(n)]
    strings = b"hello world" * 3

    def slot(t):
        if t == vc.STR:
            at = rng.randrange(0, len(strings))
            return at | rng.randrange(0, len(strings) - at + 1) << 32
        return vc.bits_of(rng.uniform(-1e6, 1e6)) if t == vc.F64 else rng.getrandbits(64)

    es = []
    for m in methods:
        ts = [ac.IDL.types[p] for p in range(ac.IDL.first[m], ac.IDL.first[m + 1])]
        es.append(vc.Entry(vc.MODE_ENCODE, 0, m, tuple(slot(t) for t in ts) + (0,) * (3 - len(ts))))
    ids = [rng.getrandbits(32) for _ in range(n)]
    rows, chunks, total, _ = vc.values_batch(es, vc.FORM_PARAMS, ac.IDL, [], 3, strings, b"")
    method, slots, _, _, _, _, _ = dev_inputs(es, 3)
    v = rpc_amd.frames_values(method, slots, dev_schema(ac.IDL), form=vc.FORM_PARAMS, strings=dev_bytes(strings))
    assert bytes(v.values.cpu().numpy()) == b"".join(c[1] for c in chunks)
    table = rpc_amd.route_table(names)
    r = rpc_amd.frames_request(method, to_dev(np.array(ids, dtype=np.uint32).view(np.int32)), v.values, v.value_offsets,
                               v.value_lens, table)
    want = b"".join(rq.call_body(names[methods[i]], chunks[i][1], ids[i]) for i in range(n))
    assert bytes(r.bodies.cpu().numpy()) == want
