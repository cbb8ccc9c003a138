"""The frame results' plain rules (tests/results_cases.py) against the answers written by hand
beside each case of its table: a check of the rules themselves, which the emulator and the
device are then held to (tests/test_results_emu.py, tests/test_frames_results.py)."""
import args_cases as ac
import results_cases as rs


def test_rules_on_the_stated_cases():
    """The plain rules give each case of the table the answers written beside it, every status
    occurs for every type, and the limit cases sit exactly on their limits."""
    buf, entries, pm, se = rs.back_to_back([(t, r, e) for _, t, r, e, *_ in rs.CASES])
    got = rs.results_entries(buf, entries, pm)
    for (name, t, result, error, status, value, estatus, ecode), row, e in zip(rs.CASES, got, entries):
        assert (row.status, row.error_status, row.error_code) == (status, estatus, ecode), (name, row)
        if value is not None:
            assert row.value == value, (name, row)
        elif status == rs.OK:  # a STR value is the bytes between the quotes
            at, ln = row.value & 0xFFFFFFFF, row.value >> 32
            assert b'"' + buf[e[0] + at:e[0] + at + ln] + b'"' == result, name
        if estatus == rs.OK:  # and so is the message
            at, ln = row.error_message & 0xFFFFFFFF, row.error_message >> 32
            assert b'"message":"' + buf[e[0] + at:e[0] + at + ln] + b'"' in error, name
        else:
            assert row.error_message == 0, name
    seen = {(t, row.status) for (_, t, *_), row in zip(rs.CASES, got)}
    assert seen >= {(t, s) for t in range(5) for s in (rs.OK, rs.MISMATCH, rs.DEFER)}, sorted(seen)
    assert {rs.ABSENT} <= {row.status for row in got} and {r.error_status for r in got} == {rs.OK, rs.ABSENT, rs.MISMATCH,
                                                                                         rs.DEFER}
    by_name = {c[0]: c[2] for c in rs.CASES}
    assert [ac.Span(by_name["tokens 256"]).tokens] == [256] and len(by_name["tokens 257"].split(b",")) == 128
    assert [len(s) for _, s, _ in rs.BARE[:3]] == [1024, 1025, 1024]
    buf, entries, pm, se = rs.case_entries()
    want = rs.results_entries(buf, entries, pm)
    assert {r.status for r in want} == set(range(7))
    nb = len(rs.CASES)
    assert [r.status for r in want[nb:nb + len(rs.BARE)]] == [s for _, _, s in rs.BARE]
    assert want[nb].value == 1 | 1022 << 32
    tail = [r.status for r in want[nb + len(rs.BARE):]]
    assert tail == [rs.NONE] * 9 + [rs.OK] + [rs.BAD_SCHEMA] * 7 + [rs.RANGE] * 7 + [rs.ABSENT, rs.DEFER, rs.OK]  # ("}" alone is no value)
    assert want[-2].error_status == rs.OK and want[-3].error_status == rs.ABSENT and want[-1].error_status == rs.ABSENT
    # the per-slot cases
    buf, entries, pm, se = rs.slot_cases()
    rows = rs.results_entries(buf, entries, pm)
    slots = rs.results_slots(entries, rows, se)
    assert [s[0] for s in slots] == [rs.OK, 0, rs.OK, rs.OK, 0, 0, 0, 0]
    assert slots[3] == (rs.OK, 104, rs.ABSENT, 0, entries[4][0]) and slots[0][1] == 100
