"""The staging rounds of the frame route, resolve and args on the GPU (stage_rounds,
rpc_amd/csrc/frames_stage.h) held to any placement of the bodies.  The three
contracts judge entry i by the bytes at its (offset, length) wherever those lie; the rounds are
where the placement matters.  tests/stage_cases.py places the bodies: memory order reversed and
shuffled, fixed slots, all lanes on one span and on two spans far apart, every prefix and suffix
of one text, bodies that end on a window's last byte and one byte behind it, bodies on the
buffer's first and last byte at every address.  Every input is legal and lies inside its buffer.
Each test first asserts, by stage_cases.rounds, that its input has the property it was built for,
then compares one call with the plain rules, as the three kernels' own tests do."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import args_cases as ac  # noqa: E402
import resolve_cases as rsc  # noqa: E402
import route_cases as rc  # noqa: E402
import stage_cases as sc  # noqa: E402
import test_frames_args as fa  # noqa: E402
import test_frames_resolve as fres  # noqa: E402
import test_frames_route as fr  # noqa: E402

KERNELS = ["route", "resolve", "args"]
#: ids the resolve's edge bodies are waited for under (stage_cases.reply(k) has id 4000000001 + k);
#: nobody waits for bodies 11 and 20
EDGE_IDS = [4000000001 + k for k in (3, 1, 30, 2, 21, 10, 0, 12)]
MAKE = {"route": sc.request, "resolve": sc.reply, "args": sc.params}


def run(kernel, buf, spans, mis, what, methods=None, strangers=(), schema=ac.IDL, width=ac.MAX_PARAMS, holds=None):
    """``holds`` (a placement's property) asserted for the entries that reach the rounds, then one
    call per kernel variant over entries on ``spans``, compared with the plain rules by the
    kernel's own check.  Returns those entries and what the rules give (the args: for the span as
    a body of its own, and inside a body that starts up to 40 bytes earlier)."""
    if kernel == "args":
        variants = [sc.args_entries(spans, methods or [ac.N] * len(spans), lead, strangers) for lead in (False, True)]
        pending = sc.args_walked(buf, variants[0], schema)
        assert pending == sc.args_walked(buf, variants[1], schema)
    else:
        pending = sc.walked(buf, spans)
    if holds:
        holds(pending, mis)
    if kernel == "route":
        return pending, [fr.check(buf, spans, None, rc.IDL, mis, what)]
    if kernel == "resolve":
        waited = sc.resolve_set()[1] + EDGE_IDS + [7]
        call = rsc.Call(buf, [s[0] for s in spans], [s[1] for s in spans], None, waited)
        return pending, [fres.check(call, mis, what)]
    wants = [fa.check(buf, entries, schema, width, mis, (what, k)) for k, entries in enumerate(variants)]
    assert all(want[t][0] == ac.NONE for want in wants for t in strangers)
    return pending, wants


def placed(kernel, name):
    """(Placed, methods, strangers) of a batch placement for a kernel."""
    if kernel == "args":
        p, methods = sc.args_batch(name)
        return p, methods, sc.STRANGERS if len(p.spans) == len(sc.args_set()) else ()
    bodies = sc.route_set() if kernel == "route" else sc.resolve_set()[0]
    return sc.batch(name, bodies, MAKE[kernel]), None, ()


def specific(kernel, want):
    """The number each entry's answer carries: the request's or reply's id, is_even's n."""
    if kernel == "route":
        return [w[2] for w in want]
    return want.id if kernel == "resolve" else [w[2][0] for w in want]


def number(kernel, k):
    return (2000000001 if kernel == "args" else 4000000001) + k


@pytest.mark.parametrize("mis", [0, 5, 15])
@pytest.mark.parametrize("name", sc.BATCH)
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_placements_match_plain_rules(kernel, name, mis):
    """700 bodies over three workgroups in reversed and shuffled memory order and in slots of
    1,040 and 4,099 bytes (the args: with entries of other kinds and garbage offsets on four
    lanes, two of them lane 0); 256 lanes on one span; lanes alternating between two spans more
    than a window apart; every prefix and suffix of one text.  The route's groups are checked on
    every placement."""
    p, methods, strangers = placed(kernel, name)
    _, wants = run(kernel, p.buf, p.spans, mis, (name, mis), methods, strangers, holds=p.holds)
    if name == "nested":  # each span has its own answer: only the two whole texts carry the number
        for want in wants:
            assert sorted(set(specific(kernel, want))) == [0, number(kernel, 30)]


@pytest.mark.parametrize("name", ["reversed", "shuffled", "slots"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_rows_do_not_depend_on_the_placement(kernel, name):
    """Entry i is body i in every placement, so the outputs of a placed batch equal the outputs
    of the same bodies back to back, entry for entry: the route's rows and groups, the resolve's
    rows and join, the args' slots (offsets in them are relative to the body, so equal too)."""
    base, methods, strangers = placed(kernel, "back to back")
    _, plain = run(kernel, base.buf, base.spans, 5, "back to back", methods, strangers)
    for n in ([name] if name != "slots" else ["slots of 1040", "slots of 4099"]):
        p, methods, strangers = placed(kernel, n)
        assert [s[1] for s in p.spans] == [s[1] for s in base.spans]
        _, wants = run(kernel, p.buf, p.spans, 5, n, methods, strangers)
        if kernel == "args":  # (how far a body reaches in front of its span depends on the span's offset,
            # and a string slot counts from the body's start: compare its length alone there)
            strip = lambda want: [(w[0], w[1], (w[2][0] >> 32,) + w[2][1:]) if m == ac.S else w  # noqa: E731
                                  for w, m in zip(want, methods)]
            assert wants[0] == plain[0] and strip(wants[1]) == strip(plain[1])
        else:
            assert wants == plain


@pytest.mark.parametrize("mis", [0, 1, 15])
@pytest.mark.parametrize("kernel", KERNELS)
def test_window_edges(kernel, mis):
    """Lane 0's body at low address bits 0, 1 and 15 opens the window; lanes 1 and 2 hold a body,
    the shortest and one of kRouteMaxBody bytes, that ends on the window's last byte (one round
    takes all three) and one byte behind it (it waits for round two)."""
    edges = sc.window_edges(MAKE[kernel], mis)
    assert len(edges) == 12
    for p in edges:
        _, wants = run(kernel, p.buf, p.spans, mis, (p.name, mis), holds=p.holds)
        for want in wants:
            assert specific(kernel, want) == [number(kernel, 0), number(kernel, 1), number(kernel, 1)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_buffer_ends(kernel):
    """A body at offset 0 and a body that ends on the buffer's last byte, at every address mod 16:
    both edge blocks are partial whenever the address is not a multiple of 16; and a whole buffer of 8 bytes whose
    only block is both the first and the last, or that straddles a 16-byte step."""
    for mis in range(16):
        p = sc.buffer_ends(MAKE[kernel], mis)
        _, wants = run(kernel, p.buf, p.spans, mis, p.name, holds=p.holds)
        for want in wants:
            assert specific(kernel, want) == [number(kernel, 2), number(kernel, 3)]
    for mis in sc.WHOLE_MIS:
        p = sc.whole_buffer(sc.WHOLE, mis)
        _, wants = run(kernel, p.buf, p.spans, mis, p.name, [0], (), sc.ID_SCHEMA, 1, holds=p.holds)
        for want in wants:
            assert specific(kernel, want) == [7]


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_placement_in_one_call(kernel):
    """One buffer, 1,166 entries: a workgroup with a round per lane beside one with a single
    round, one with two, and the other placements behind them."""
    mis = 5
    if kernel == "args":
        buf, spans, methods = sc.args_mixture(mis)
        pending, _ = run(kernel, buf, spans, mis, "mixture", methods, sc.STRANGERS)
    else:
        bodies = sc.route_set() if kernel == "route" else sc.resolve_set()[0]
        buf, spans, bodies_placed = sc.mixture(bodies, MAKE[kernel], mis)
        pending, (want,) = run(kernel, buf, spans, mis, "mixture")
        if kernel == "route":
            assert want == [rc.route_body(b) for b in bodies_placed]
        else:
            assert list(zip(want.id, want.result_off, want.result_len, want.error_off, want.error_len)) == \
                [rsc.decode_body(b)[1:] for b in bodies_placed]
    assert len(spans) >= 3 * sc.LANES + 1
    counts = [len(g) for g in sc.rounds(spans, pending, mis)]
    assert counts[0] >= 128 and counts[1] == 1 and counts[2] == 2 and len(counts) >= 4
