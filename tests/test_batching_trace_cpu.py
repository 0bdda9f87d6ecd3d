"""CPU: the continuous-batching scheduler (fq3hip/batching.py) makes exactly the recorded sequence of calls on its engines and its
batch object and yields exactly the recorded events -- tools/scheduler_trace.py drives it over scripted fakes through admission,
staging, packed groups, chunked streaming, errors, a short KV pool, seeded lanes, text lanes and an abandoned run, and
tests/golden/scheduler_trace.json holds what it did.  A change that is meant to leave the scheduler's behaviour alone leaves this
file alone; one that is not re-records it with ``python tools/scheduler_trace.py --write`` and says what moved."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def trace():
    import scheduler_trace as T
    return T, T.scenarios()


def test_the_scheduler_makes_the_recorded_calls(trace):
    T, got = trace
    want = json.load(open(T.GOLDEN))
    assert list(got) == list(want)
    for name in want:
        rec = json.loads(json.dumps(got[name]))
        first = next((i for i, (a, b) in enumerate(zip(rec, want[name])) if a != b), min(len(rec), len(want[name])))
        assert rec == want[name], f"{name}: differs from entry {first}: got {rec[first:first + 3]}, recorded {want[name][first:first + 3]}"
    assert T.render(got) == open(T.GOLDEN).read()


def test_the_scenarios_reach_the_paths_they_are_meant_for(trace):
    """The trace is only as good as its coverage: every scenario must really take the branch it was written for."""
    _T, got = trace
    kinds = lambda name: [e[0] for e in got[name]]
    events = lambda name: [e for e in got[name] if e[0] == "event"]
    for batch in ("sync", "lookahead"):
        assert sorted(e[1] for e in events(f"mixed_{batch}")) == list(range(7))
        assert [e[2] for e in sorted(events(f"mixed_{batch}"), key=lambda e: e[1])] == [20, 13, 70, 8, 16, 33, 5]
        assert ["refill", 2, 64] in got[f"mixed_{batch}"] or any(e[0] == "refill" and e[2] == 64 for e in got[f"mixed_{batch}"])
        assert "prefill_first_tokens_packed" in kinds(f"staged_{batch}") and "kv_adopt" in kinds(f"staged_{batch}")
        ch = events(f"chunked_{batch}")
        assert [e[2:5] for e in ch if e[1] == 0] == [[4, False, 4], [4, False, 8], [4, True, 12]]       # a multiple of the chunk
        assert [e[2:5] for e in ch if e[1] == 1] == [[None, True, 0]]                                   # no frame at all
        assert any(e[7] > 0 for e in ch)                                                                # events that share a poll
        tx = got[f"text_{batch}"]
        appends = [e[1] for e in tx if e[0] == "text_append"]
        assert any(len(a) == 2 for a in appends)                                                        # ONE append for two lanes
        assert sum(len(i[1]) for a in appends for i in a if i[0] == 0) == 81                            # the capacity clamp
        assert any(i[1][-1:] == [999] and i[2] for a in appends for i in a)                             # a feeder closed early
        assert [e[2] for e in sorted(events(f"text_{batch}"), key=lambda e: e[1])] == [80, 30, 70, 12]
        ab = got[f"abandoned_{batch}"]
        cut = kinds(f"abandoned_{batch}").index("abandoned")
        assert "decode_cancel" in [e[0] for e in ab[cut:]] and [e[2] for e in events(f"abandoned_{batch}")][2:] == [8, 8, 4]
    assert any(e[0] == "prefill_first_token" for e in got["staged_split_rows"]) and \
        all(len(e[1]) == 2 for e in got["staged_split_rows"] if e[0] == "prefill_first_tokens_packed")
    assert "prefill_first_tokens_packed" not in kinds("staged_unpacked")
    assert any(e[0] == "prefill_first_tokens_packed" and e[3] is not None and None in e[3] and e[4] for e in got["staged_seeded_cache"])
    # the packed group with the bad request is tried, fails as a whole, and only the culprit is reported
    pk = got["error_in_packed_group"]
    assert any(e[0] == "prefill_first_tokens_packed" and 1 in e[2] for e in pk) and any(e[0] == "prefill_first_token" and e[2] == 0 for e in pk)
    assert sorted((e[1], e[6] is not None) for e in events("error_in_packed_group")) == [(0, False), (1, True), (2, False), (3, False), (4, True), (5, False)]
    for name in ("error_at_arming_direct", "error_at_arming_staged"):
        assert "decode_cancel" in kinds(name) and "raised" in kinds(name) and any(e[6] for e in events(name))
    # postponement keeps the order: the helpers see the requests 0, 1, 2(, 3) for the first time in that order, all finish
    for name, n in (("enomem_first_wave", 3), ("enomem_while_active", 4)):
        assert sorted(e[1] for e in events(name)) == list(range(n)) and all(e[6] is None for e in events(name))
        armed = [e[2] for e in got[name] if e[0] == "arm_decode"]
        assert armed == list(range(n))
    assert [e[6] is not None for e in sorted(events("enomem_nothing_active_yield"), key=lambda e: e[1])] == [False, True]
    assert "raised" in kinds("enomem_nothing_active_raise")
    fills = [e[1] for e in got["seeded_ring"] if e[0] == "noise_fill_many"]
    assert fills[0] == [[0, 100, 0], [2, 7, 0]] and [[0, 100, 64], [2, 7, 64]] in fills
    assert [e[1:] for e in got["seeded_ring"] if e[0] == "refill"] == [[1, 0], [1, 64]]
