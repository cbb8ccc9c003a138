"""The frame resolve on a seeded corpus of reply bodies (tests/resolve_fuzz.py).

The CPU part holds the plain rules and the emulator against the live reference decoder
(rpc_codec_decode_response behind tests/dropin/ref_decode.c, built to a temporary directory; it
skips where the reference tree is absent): a body the reference rejects is never decoded, INVALID
implies a rejection, a decoded body has the reference's id and member presence, and the body
rebuilt from the id and the spans prints the same members as the body itself -- the check of the
spans.  So that deferring cannot hide a failure: no body printed by cJSON (the golden fixture's
class c and the corpus's canonical class) defers, and of the hostile bodies the reference accepts
at least half are decoded.

The gpu part needs no reference: the GPU equals the rules on the same corpus, field for field."""
import json
import os

import numpy as np
import pytest

import resolve_cases as rc
import resolve_fuzz as rz
import resolve_ref
from test_resolve_emu import S_SMALL, resolve_emu, run_emu  # noqa: F401

SEED = 0x5E50
HERE = os.path.dirname(os.path.abspath(__file__))
DECODED = (rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE)


@pytest.fixture(scope="module")
def corpus():
    return rz.corpus(SEED)


@pytest.fixture(scope="module")
def ref_decode(tmp_path_factory):
    exe = resolve_ref.build(tmp_path_factory.mktemp("ref_decode"))
    if exe is None:
        pytest.skip("the reference tree is absent")
    return exe


def test_corpus_covers_its_classes(corpus):
    rows = [rc.decode_body(b) for b in corpus.bodies]
    assert set(corpus.classes) == {name for name, _, _ in rz.SHARES} and len(corpus.bodies) > 5000
    assert {r[0] for r in rows} == {rc.UNKNOWN, rc.INVALID, rc.DEFER}
    assert all(r[0] == rc.UNKNOWN for r, c in zip(rows, corpus.classes) if c == "canonical")
    lim = {(len(b) > rc.MAX_BODY, r[0]) for b, r, c in zip(corpus.bodies, rows, corpus.classes) if c == "limits"}
    assert lim == {(False, rc.UNKNOWN), (False, rc.DEFER), (True, rc.DEFER)}


def hold(bodies, classes, rows, ref, ref_of_rebuilt, what):
    accepted = decoded = 0
    for b, cls, row, g in zip(bodies, classes, rows, ref):
        where = (what, cls, b[:120], row, g)
        hostile = cls != "canonical"
        if g.rc != 0:
            assert row[0] not in DECODED, where  # a -1 is never decoded
        elif hostile:
            accepted += 1
            decoded += row[0] in DECODED
        if row[0] == rc.INVALID:
            assert g.rc == -1, where
        if row[0] in DECODED:
            assert g.rc == 0 and g.id == row[1], where
            assert (g.result is not None) == (row[3] > 0) and (g.error is not None) == (row[5] > 0), where
            again = ref_of_rebuilt[b]
            assert again.rc == 0 and (again.id, again.result, again.error) == (g.id, g.result, g.error), where
        if cls == "canonical":
            assert row[0] in DECODED, where
    return decoded, accepted


def test_rules_and_emulator_against_the_live_reference(corpus, ref_decode, resolve_emu):  # noqa: F811
    golden_c = [e[1].encode("latin-1") for e in
                json.load(open(os.path.join(HERE, "golden", "resolve_golden.json")))["entries"] if e[0] == "c"]
    bodies = corpus.bodies + golden_c
    classes = corpus.classes + ["canonical"] * len(golden_c)
    ref = resolve_ref.run(ref_decode, bodies)
    rows = [rc.decode_body(b) for b in bodies]
    todo = [b for b, r in zip(bodies, rows) if r[0] == rc.UNKNOWN]
    rebuilt = dict(zip(todo, resolve_ref.run(ref_decode, [rz.rebuilt(b, rc.decode_body(b)) for b in todo])))
    decoded, accepted = hold(bodies, classes, rows, ref, rebuilt, "rules")
    print("hostile bodies the reference accepts: %d, decoded: %d (%.1f %%)" % (accepted, decoded, 100.0 * decoded / accepted))
    assert 2 * decoded >= accepted > 1000
    # the emulator: the kernels' own source on the same bodies, against the reference and the rules
    call = rc.Call(*rc.pack_bodies(bodies, nul=1), None, [])
    got = run_emu(resolve_emu, S_SMALL, 7, call, False)
    emu_rows = [(rc.UNKNOWN if k in DECODED else k, *rest) for k, *rest in
                zip(got.kind, got.id, got.result_off, got.result_len, got.error_off, got.error_len)]
    assert emu_rows == rows
    assert hold(bodies, classes, emu_rows, ref, rebuilt, "emulator") == (decoded, accepted)


def test_emulator_joins_the_corpus_as_the_rules_do(corpus, resolve_emu):  # noqa: F811
    call = rz.call_of(corpus)
    want = call.expect()
    assert {rc.MATCHED, rc.UNKNOWN, rc.DUPLICATE, rc.INVALID, rc.DEFER} == set(want.kind) and want.open
    for descending in (False, True):
        assert run_emu(resolve_emu, S_SMALL, 3, call, descending) == want


@pytest.mark.gpu
def test_gpu_equals_the_rules_on_the_corpus(corpus):
    torch = pytest.importorskip("torch")
    import rpc_amd
    call = rz.call_of(corpus)
    mis = 9
    raw = np.zeros(mis + len(call.buf), dtype=np.uint8)
    raw[mis:] = np.frombuffer(call.buf, dtype=np.uint8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    r = rpc_amd.frames_resolve(dev(raw)[mis:], dev(np.array(call.offs, dtype=np.uint64).view(np.int64)),
                               dev(np.array(call.lens, dtype=np.uint32).view(np.int32)),
                               dev(np.array(call.pending, dtype=np.uint32).view(np.int32)))
    torch.cuda.synchronize()
    u32 = lambda x: x.cpu().numpy().view(np.uint32).tolist()  # noqa: E731
    got = rc.Resolved(r.kind.cpu().numpy().tolist(), u32(r.id), u32(r.result_off), u32(r.result_len), u32(r.error_off),
                      u32(r.error_len), u32(r.slot), u32(r.slot_entry), u32(r.open)[:int(r.nopen.cpu()[0])])
    want = call.expect()
    for field in rc.Resolved._fields:
        g, w = getattr(got, field), getattr(want, field)
        bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
        assert not bad and len(g) == len(w), (field, bad[:5], [(g[i], w[i]) for i in bad[:5]])
