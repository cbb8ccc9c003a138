"""The frame request on a seeded corpus of (name, params, id) triples (tests/request_fuzz.py)
against the live reference encoder (rpc_codec_encode_request behind tests/dropin/ref_encode.c,
built to a temporary directory; skipped where the reference tree is absent).  The generator emits
only params that cJSON reprints unchanged, and the test asserts that of every corpus entry -- none
is excluded -- so every body of the plain rules and of the emulator must be the reference's, byte
for byte."""
import pytest

import request_cases as rq
import request_fuzz as rz
import request_ref
from test_request_emu import T_K, request_emu, run_emu  # noqa: F401  (request_emu: a fixture)

SEED = 0x7E57


@pytest.fixture(scope="module")
def corpus():
    return rz.corpus(SEED)


@pytest.fixture(scope="module")
def reference(corpus, tmp_path_factory):
    exe = request_ref.build(tmp_path_factory.mktemp("ref_encode"))
    if exe is None:
        pytest.skip("the reference tree is absent")
    return request_ref.run(exe, [(corpus.names[m], text, rid) for m, text, rid in corpus.triples])


def case_of(corpus):
    params, ents = bytearray(b"#"), []
    for m, text, rid in corpus.triples:
        ents.append((rq.DATA, m, rid, len(params), len(text or b"")))
        params += (text or b"") + b"#"
    return rq.Case("fuzz", bytes(params), rq.make_table(corpus.names), ents, [0, len(ents)], typed=False)


def test_corpus_covers_its_forms(corpus):
    texts = [t for _, t, _ in corpus.triples]
    assert len(texts) >= 3000 and {m for m, _, _ in corpus.triples} == set(range(len(corpus.names)))
    assert sum(t is None for t in texts) > 100
    for mark in (b"[", b"{", b"\\n", b"true", b"null", b".5", b"-", b"[]", b"{}", b'""'):
        assert sum(1 for t in texts if t and mark in t) > 20, mark
    assert max(t.count(b"[") + t.count(b"{") for t in texts if t) >= 8
    assert {rid for _, _, rid in corpus.triples} >= set(rz.IDS)


def hold(corpus, reference, offs, lens, status, out):
    for (m, text, rid), g, at, ln, st in zip(corpus.triples, reference, offs, lens, status):
        assert g.printed == text, (text, g.printed)  # no entry is excluded for non-canonical params
        assert st == rq.Q_CALL and out[at:at + ln] == g.request, (corpus.names[m], text, rid)


def test_rules_against_the_live_reference(corpus, reference):
    want = rq.want_of(case_of(corpus), None)
    hold(corpus, reference, want.body_offsets, want.body_lens, want.status, want.out)


@pytest.mark.parametrize("tile,src_mis,out_mis", [(T_K, 3, 0), (256, 0, 13)])
def test_emulator_against_the_live_reference(corpus, reference, request_emu, tile, src_mis, out_mis):  # noqa: F811
    total, rows, conn, out = run_emu(request_emu, tile, src_mis, out_mis, case_of(corpus), None)
    hold(corpus, reference, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], out)
