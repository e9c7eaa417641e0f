"""Calls on one handle are ordered against the CALLER's stream, on a stream that is busy (-m gpu).

Every case (tests/handle_cases.py: STREAM_CASES) runs on a torch.cuda.Stream of its own, all enqueued without a host wait:
a delay, the copy of the true scene into persistent input tensors that held a decoy scene, the library call, an in-stream clone of
every output tensor, the copy of the decoy back.  After one synchronise the call's results and the clones must equal, byte for
byte, what the case gives on idle streams with the true scene -- and differ from what it gives with the decoy.  An input read on
an internal stream that was never joined sees the decoy (before or after); an output written after the caller's stream moved on
misses the clone.  Both scenes are valid frames: a mis-ordered read gives a wrong answer, never a bad address.

The delay (torch.cuda._sleep) is 20 x the slowest quiescent call of the file, between 10 and 200 ms.  Each case proves the
stream was busy: an entry that does not wait returns while an event behind the delay is pending, an entry that waits keeps the
host at least half the delay.  A case that cannot show it doubles the delay once, then fails.

The list runs twice: here with the hardware queues the process has, and in ONE child process with GPU_MAX_HW_QUEUES=16 (streams
that share a queue hide a missing wait).  The child also runs the control: the waiting cases with the library call on a second
stream that nothing orders behind the producer -- legal input, mis-ordered by the caller -- must answer the true scene or the
decoy (a case of several library calls: each call's part one of the two); how many saw the decoy is printed
(profiles/NOTES_handle_sequences.md), it is no pass condition.  A control call that the hardware held behind the producer all
the same (it spent half the delay or more in the call: two streams on one hardware queue) ran beside the producer's copies, on
a mask of one scene and a depth of the other for all the library can know: it is counted, its answer is not judged."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import handle_cases as HC  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 40   # 3 x the measured run of the child, 12 s (profiles/NOTES_handle_sequences.md)


@pytest.fixture(scope="module")
def cal():
    assert torch.cuda.is_available()
    cpm = HC.sleep_cycles_per_ms()
    refs = {n: HC.stream_reference(n) for n in HC.STREAM_CASES}
    delay = HC.calibrate_delay(refs)
    print(f"delay {delay:.1f} ms ({cpm:.0f} cycles per ms); quiescent ms:", {n: round(r[2], 2) for n, r in refs.items()})
    return cpm, refs, delay


@pytest.mark.parametrize("name", list(HC.STREAM_CASES))
def test_case_on_a_busy_stream(cal, name):
    cpm, refs, delay = cal
    r = HC.check_stream_case(name, refs[name], delay, cpm)
    print(r)
    assert r["decoy_differs"], "the decoy must have another answer, or the case cannot fail"
    assert r["busy"], f"the stream was not shown busy at {r['delay_ms']} ms (call {r['call_ms']} ms)"
    assert r["ok"], f"{name}: not the true scene's answer" + (" -- the DECOY's" if r["saw_decoy"] else "")


def test_every_case_again_with_sixteen_hardware_queues():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "tests.handle_cases", "--streams"], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=CHILD_LIMIT_S)
    took = time.perf_counter() - t0
    print(p.stdout[-6000:], p.stderr[-3000:], f"child: {took:.1f} s")
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    head = [x for x in lines if x.get("calibration")]
    assert len(head) == 1 and head[0]["queues"] == "16" and 10.0 <= head[0]["delay_ms"] <= 200.0
    cases = {x["case"]: x for x in lines if "case" in x}
    assert set(cases) == set(HC.STREAM_CASES)
    for name, r in cases.items():
        assert r["decoy_differs"] and r["busy"], (name, r)
        assert r["ok"], f"{name}: not the true scene's answer" + (" -- the DECOY's" if r["saw_decoy"] else "")
    ctl = [x for x in lines if x.get("control")]
    assert len(ctl) == 1 and ctl[0]["cases"] == sum(1 for p_, _ in HC.STREAM_CASES.values() if p_ == "host")
    for name, v in ctl[0]["answers"].items():
        if not v["held"]:   # the call returned before the delay ended: it ran on inputs nobody was writing
            assert v["answer"] in ("true", "decoy", "mixed"), (name, v)
    print("control: cases that saw the decoy:", ctl[0]["saw_decoy"], "of", ctl[0]["cases"], "-- held by the producer:", ctl[0]["held"])
