"""The frame values on a stream of their own, in the manner of tests/test_frames_streams.py: the
inputs arrive late behind a long kernel on the side stream, and the wrapper's three stream forms.
A launch, a memset or a wrapper fill on another stream is a wrong answer here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
import args_cases as ac  # noqa: E402
import values_cases as vc  # noqa: E402
from test_frames_streams import Job, form_c, guarded, host, run_late, same_bytes, side_streams, total_of  # noqa: E402
from test_frames_unpack import dev_bytes  # noqa: E402
from test_frames_values import dev_form, dev_inputs  # noqa: E402


def values_job(form, mis, sized=False):
    if form == vc.FORM_RESULT:
        rtypes, entries = vc.result_entries()
        schema, width = ac.IDL, 1
        entries = entries * 40  # (more than one workgroup of the size pass, more than one tile of texts)
    else:
        rtypes, schema, width = [], vc.EXTRA, 8
        entries = [c[3] for c in vc.params_cases() if c[1] is vc.EXTRA] * 60
    rows, chunks, total, ndefer = vc.values_batch(entries, form, schema, rtypes, width, vc.STRINGS, vc.TEXTS)
    want = bytearray(b"\xa5" * total)
    for at, txt, _ in chunks:
        if txt is not None:
            want[at:at + len(txt)] = txt
    big, out = guarded(total, mis)
    method, slots, mode, status, base, toff, tlen = dev_inputs(entries, width)
    strings, texts = dev_bytes(vc.STRINGS, 5 if mis else 0), dev_bytes(vc.TEXTS, 3 if mis else 0)
    sch = dev_form(form, schema, rtypes)

    def call(stream):
        return rpc_amd.frames_values(method, slots, sch, form=form, mode=mode, status=status, strings=strings,
                                     str_base=base, texts=texts, text_offsets=toff, text_lens=tlen,
                                     out=None if sized else out, stream=stream)

    def check(r):
        what = ("values", form, mis, sized)
        assert total_of(r) == total and int(r.ndefer.cpu()[0]) == ndefer > 0, what
        if sized:
            got = r.values.cpu().numpy().tobytes()
            for at, txt, _ in chunks:
                assert txt is None or got[at:at + len(txt)] == txt, what
        else:
            same_bytes(big, mis, bytes(want), what)
        got_rows = list(zip(host(r.status, np.uint8), host(r.reply_status, np.int32), host(r.value_offsets, np.uint64),
                            host(r.value_lens, np.uint32)))
        assert got_rows == rows, what

    late = [method, slots, mode, status, base, toff, tlen, strings, texts]
    late += [sch] if form == vc.FORM_RESULT else [sch.first, sch.types, sch.name_off, sch.names]
    return Job(f"values {form} {mis}", late, call, check)


@pytest.mark.parametrize("form", [vc.FORM_RESULT, vc.FORM_PARAMS])
@pytest.mark.parametrize("mis", [0, 5])
def test_values_behind_late_inputs(form, mis):
    run_late(values_job(form, mis))


@pytest.mark.parametrize("how", ["a", "b", "c"])
@pytest.mark.parametrize("sized", [False, True])
def test_wrapper_stream_forms(how, sized):
    job = values_job(vc.FORM_RESULT if sized else vc.FORM_PARAMS, 0 if sized else 5, sized=sized)
    s = side_streams()[0]
    torch.cuda.synchronize()
    if how == "c":
        r = form_c(s, lambda: job.call(s))
    else:
        with torch.cuda.stream(s):
            r = job.call(s if how == "a" else None)
        s.synchronize()
    job.check(r)
