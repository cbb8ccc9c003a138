"""The frame values' number formatting on the GPU (rpc_frames_values_device): the
bit patterns the CPU emulator formats (tests/values_numbers.py, tests/test_values_emu.py) through
the kernel itself -- its 64 x 64 multiplies, its table in device memory, the f64 subtract,
multiply and compare and the divide of the read-back that the gfx950 back end emits -- against
the plain rule ("%.15g", float(), "%.17g": values_cases.f64_text) byte for byte.

One method of result type F64, width 1; the corpus shuffled, so that a wave holds 15-digit,
17-digit, integer and deferring lanes side by side, and sorted by list, so that neighbouring
lanes take the same path."""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import values_cases as vc  # noqa: E402
import values_numbers as vn  # noqa: E402
from test_frames_unpack import DEV, to_dev  # noqa: E402


@functools.lru_cache(maxsize=None)
def labelled():
    return tuple((label, b) for label, bs in vn.corpus().items() for b in bs)


@functools.lru_cache(maxsize=None)
def wanted():
    return {b: vc.f64_text(b) for _, b in labelled()}


def device_texts(patterns, mis=0):
    """The device's text (None: DEFER) for each pattern, and its columns checked for consistency."""
    n = len(patterns)
    slots = to_dev(np.array(patterns, dtype=np.uint64).view(np.int64).reshape(1, n))
    method = torch.zeros(n, dtype=torch.int16, device=DEV)
    big = torch.full((mis + 25 * n + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    r = rpc_amd.frames_values(method, slots, to_dev(np.array([vc.F64], dtype=np.uint8)), out=big[mis:mis + 25 * n])
    torch.cuda.synchronize()
    st = r.status.cpu().numpy().view(np.uint8)
    off = r.value_offsets.cpu().numpy().view(np.uint64)
    ln = r.value_lens.cpu().numpy().view(np.uint32)
    rs = r.reply_status.cpu().numpy().view(np.int32)
    out = big.cpu().numpy()[mis:].tobytes()
    assert set(st.tolist()) <= {vc.OK, vc.DEFER}
    assert ((st == vc.DEFER) == (ln == 0)).all() and ((st == vc.DEFER) == (rs == vc.INTERNAL)).all()
    assert int(r.ndefer.cpu()[0]) == int((st == vc.DEFER).sum()) and int(r.total.cpu()[0]) == int(ln.sum())
    assert (off == np.concatenate(([0], np.cumsum(ln.astype(np.uint64))[:-1]))).all() and ln.max() <= 24
    assert out[int(ln.sum()):int(ln.sum()) + 16] == b"\xa5" * 16
    return [None if s == vc.DEFER else out[int(o):int(o) + int(k)] for s, o, k in zip(st, off, ln)]


def hold(pairs, mis):
    """Every text the rule's; the conditions per list; returns the DEFER count per list."""
    texts = device_texts([b for _, b in pairs], mis)
    by = {}
    for (label, _), t in zip(pairs, texts):
        by.setdefault(label, []).append(t)
    order = {label: [b for lb, b in pairs if lb == label] for label in by}
    for label, bs in vn.corpus().items():
        assert sorted(order[label]) == sorted(bs), label
    # (check_texts walks each list in the corpus's order: line the texts up with it)
    lined = {}
    for label, bs in vn.corpus().items():
        text_of = {}
        for b, t in zip(order[label], by[label]):
            assert text_of.setdefault(b, t) == t, (label, hex(b))  # (the same pattern, the same answer)
        lined[label] = [text_of[b] for b in bs]
    counts = vn.check_texts(lined, wanted().__getitem__)
    print("F64 DEFER per list on the device:", counts)
    return counts


@pytest.mark.parametrize("mis", [0, 5])
def test_corpus_shuffled(mis):
    pairs = list(labelled())
    random.Random(0xF64).shuffle(pairs)
    assert 190000 <= len(pairs) <= 260000
    hold(pairs, mis)


def test_corpus_sorted_by_list():
    counts = hold(list(labelled()), 3)
    assert counts["subnormals"] == 0  # (NaN and the infinities print null; every subnormal defers by rule)


def test_defers_are_the_rules():
    """The device defers exactly where the rules do: on this corpus, the subnormals and nothing
    else.  tests/test_values_emu.py::test_corpus holds the emulator to the same entries, so a DEFER
    is the same entry in the emulator and on the device."""
    texts = device_texts([b for _, b in labelled()])
    for (label, b), t in zip(labelled(), texts):
        assert (t is None) == (wanted()[b] is None), (label, hex(b))
