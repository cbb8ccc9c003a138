"""The frame values against the live reference (tests/values_fuzz.py): RESULT form through the
reference's own dispatcher (oracle/_ref/ref_dispatch), PARAMS form through the reference
client's encoder (tests/request_ref.py).  CPU only for the rules and the emulator, and on the GPU
with the same rows; skipped where the reference tree is absent.

Sizes: 2 seeds of 12,000 RESULT rows on the rules, 6,000 on the emulator, 12,000 on the GPU;
6,000 PARAMS objects on the rules and the emulator."""
import pytest

import args_cases as ac
import request_ref
import values_cases as vc
import values_fuzz as vf
from test_values_emu import run_emu, values_emu  # noqa: F401  (values_emu: a fixture)

SEEDS = [0xB2651, 0xB2652]
N_EMU = 6000


def reference(rs):
    from oracle import oracle
    got = oracle.ref_dispatch(vf.bodies_of(rs))
    if got is None:
        pytest.skip("oracle/_ref/ref_dispatch is not built (needs the reference tree)")
    return got


def rules_layer(rs, strings):
    types, entries = vf.entries_of(rs)
    return [vc.values_entry(e, vc.FORM_RESULT, ac.IDL, types, 1, strings, b"") for e in entries]


@pytest.mark.parametrize("seed", SEEDS)
def test_rules_hold_against_the_reference(seed):
    rs, strings = vf.rows(seed, 12000)
    n = vf.hold(rs, reference(rs), rules_layer(rs, strings), strings)
    print("RESULT rows per status:", n)
    assert n[vc.OK] >= 11000


def test_emulator_holds_against_the_reference(values_emu):  # noqa: F811
    rs, strings = vf.rows(SEEDS[0], N_EMU)
    types, entries = vf.entries_of(rs)
    rows, out, _, _ = run_emu(values_emu, entries, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, texts=b"", tile=4096,
                              mis=(3, 0, 9))
    layer = [(r[0], out[r[2]:r[2] + r[3]]) for r in rows]
    assert layer == rules_layer(rs, strings)
    vf.hold(rs, reference(rs), layer, strings)


@pytest.mark.gpu
def test_gpu_holds_against_the_reference():
    from test_frames_values import run_gpu
    rs, strings = vf.rows(SEEDS[0], 12000)
    types, entries = vf.entries_of(rs)
    _, rows, chunks = run_gpu(entries, vc.FORM_RESULT, ac.IDL, types, 1, strings=strings, texts=b"", mis=(5, 0, 3))
    # (run_gpu has held the device's bytes to the rules'; the rules' bytes to the reference)
    vf.hold(rs, reference(rs), [(r[0], c[1] or b"") for r, c in zip(rows, chunks)], strings)


def test_params_objects_are_the_encoders_print(tmp_path, values_emu):  # noqa: F811
    exe = request_ref.build(tmp_path)
    if exe is None:
        pytest.skip("the reference tree is absent")
    es, strings = vf.params_rows(0xB2660, 6000)
    layer = [vc.values_entry(e, vc.FORM_PARAMS, ac.IDL, [], 3, strings, b"") for e in es]
    n = {s: sum(1 for st, _ in layer if st == s) for s in (vc.OK, vc.DEFER)}
    print("PARAMS rows per status:", n)
    # (one method in seven takes a string, and 3 of its 23 picks need an escape: about 110 of 6,000)
    assert n[vc.OK] >= 4500 and n[vc.DEFER] >= 50 and n[vc.OK] + n[vc.DEFER] == len(es)
    ok = [(e, text) for e, (st, text) in zip(es, layer) if st == vc.OK]
    enc = request_ref.run(exe, [(ac.IDL_METHODS[e.method][0], text, k + 1) for k, (e, text) in enumerate(ok)])
    for (e, text), got in zip(ok, enc):
        assert got.printed == text, (e, text, got.printed)
    # every DEFER there is a string that needs an escape (no subnormal is in these rows)
    for e, (st, _) in zip(es, layer):
        if st == vc.DEFER:
            assert e.method == ac.S and vc.needs_escape(strings[e.slots[0] & 0xFFFFFFFF:][:e.slots[0] >> 32])
    rows, out, _, _ = run_emu(values_emu, es, vc.FORM_PARAMS, ac.IDL, [], 3, strings=strings, texts=b"", tile=1024, mis=(1, 0, 7))
    assert [(r[0], out[r[2]:r[2] + r[3]]) for r in rows] == layer
