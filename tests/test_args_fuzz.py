"""The frame args against the reference's own dispatcher on generated `params` spans
(tests/args_fuzz.py; oracle/_ref/ref_dispatch is rpc_server_dispatch behind a driver of ours).
For every request with the reference's reply R: an OK row's reply, recomputed from the decoded
slots with Python handlers, is R byte for byte; an INVALID row's R is the -32602 form; a DEFER
row claims nothing.  Run on the plain rules (two seeds of 12,000 rows), on the CPU emulator
(6,000) and on the GPU (12,000, with the rows also held against the rules field for field)."""
import numpy as np
import pytest

import args_cases as ac
import args_fuzz as af
from test_args_emu import args_emu, run_emu  # noqa: F401  (args_emu: a fixture)
from test_route_emu import S_K, S_SMALL

SEEDS = [0xA2651, 0xA2652]
N_EMU = 6000


@pytest.mark.parametrize("seed", SEEDS)
def test_corpus_is_canonical_and_decided(seed):
    """args_fuzz.conditions on the plain rules alone: the canonical class has 0 DEFER and 0
    INVALID, and at least half of the hostile class is decided."""
    print(af.conditions(af.corpus(seed), af.ruled(seed)))


@pytest.mark.parametrize("seed", SEEDS)
def test_rules_hold_against_the_reference(seed):
    n = af.hold(af.corpus(seed), af.answers(seed), af.ruled(seed))
    assert n[ac.OK] >= 8000 and n[ac.INVALID] >= 500, n


@pytest.mark.parametrize("stage,mis,nul", [(S_K, 0, 1), (S_SMALL, 11, 0)])
def test_emulator_holds_against_the_reference(args_emu, stage, mis, nul):  # noqa: F811
    seed = SEEDS[0]
    rows = af.corpus(seed)[:N_EMU]
    buf, entries = af.entries_of(rows, nul=nul)
    layer = run_emu(args_emu, stage, mis, buf, entries)
    assert layer == ac.args_entries(buf, entries)
    af.hold(rows, af.answers(seed)[:N_EMU], layer)


@pytest.mark.gpu
@pytest.mark.parametrize("nul,mis", [(1, 0), (0, 5)])
def test_gpu_holds_against_the_reference(nul, mis):
    """rpc_amd.frames_args on the whole corpus, with and without the 0 byte between the bodies,
    the buffer at a 16-byte boundary and 5 bytes past one: the rows are the plain rules' and the
    three claims hold."""
    import torch
    import rpc_amd
    from test_frames_args import dev_entries, dev_schema, rows_of
    from test_frames_route import dev_bytes
    seed = SEEDS[0]
    rows = af.corpus(seed)
    buf, entries = af.entries_of(rows, nul=nul)
    off, ln, route = dev_entries(entries)
    r = rpc_amd.frames_args(dev_bytes(buf, mis), off, ln, route, dev_schema(ac.IDL), width=3)
    torch.cuda.synchronize()
    layer = rows_of(r, len(entries))
    want = ac.args_entries(buf, entries, ac.IDL, 3)
    for row, g, w in zip(rows, layer, want):
        assert g == w, (row, g, w)
    assert np.count_nonzero(r.status.cpu().numpy() == ac.OK) >= 8000
    af.hold(rows, af.answers(seed), layer)
