"""The measurement protocol of scripts/benchkit.py on the device: units, the division by reps, warm-up counts, the memory peak, the order
of alternated routes and the record keys.  Tiny tensors only."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

import benchkit as BK  # noqa: E402


def test_timed_is_per_call_in_ms_after_the_warmup_calls():
    from gnn_pretraining_amd import _lib as L
    st = torch.cuda.current_stream()
    calls = []

    def fn():
        calls.append(1)
        L.check(L.lib().gmp_spin_us(2000, st.cuda_stream), "spin")

    t = BK.timed(fn, reps=3, warmup=2)
    assert len(calls) == 5
    assert isinstance(t, BK.Timing) and t == (t.host_ms, t.event_ms)
    assert 1.5 <= t.event_ms <= 4.0                             # a 2000 us spin per call (test_gpu_streams.py holds the spin to this): ms, over reps
    assert t.host_ms >= 1.5                                     # the host clock stops after the synchronise (no upper bound: the host is shared)


def test_peak_counts_above_what_was_allocated_before_the_call():
    alive = torch.empty(4 << 20, dtype=torch.uint8, device=BK.DEV)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    p = BK.peak(lambda: torch.empty(8 << 20, dtype=torch.uint8, device=BK.DEV))
    assert isinstance(p, BK.Peak)
    assert p.above_bytes == 8 << 20
    assert p.total_bytes - p.above_bytes == before and before >= alive.numel()
    assert isinstance(p.out, torch.Tensor) and p.out.numel() == 8 << 20 and p.out.is_cuda


def test_attempt_records_the_first_line_of_the_error():
    assert BK.attempt(lambda: 7) == (7, None)

    def fails(msg):
        def fn():
            raise RuntimeError(msg)
        return fn

    assert BK.attempt(fails("first\nsecond")) == (None, "RuntimeError: first")
    out, err = BK.attempt(fails("x" * 300))
    assert out is None and err == "RuntimeError: " + "x" * 160


def test_alternate_warms_every_route_then_times_each_once_per_round():
    order = []
    routes = {"a": lambda: order.append("a"), "b": lambda: order.append("b")}
    times = BK.alternate(routes, reps={"a": 2, "b": 1}, rounds=3, warmup=1)
    assert "".join(order) == "ab" + "aab" * 3
    assert list(times) == ["a", "b"] and all(len(ts) == 3 and all(isinstance(t, BK.Timing) for t in ts) for ts in times.values())
    order.clear()
    BK.alternate(routes, reps=1, rounds=2, route_warmup=2)      # the same reps for every route; warm-up calls before each timed run
    assert "".join(order) == "aaabbb" * 2


def test_record_min_writes_the_three_keys_with_the_digits_asked_for():
    times = {"kernel": [BK.Timing(1.23456, 0.98765), BK.Timing(1.11111, 1.00009), BK.Timing(2.0, 0.5)], "torch": [BK.Timing(3.14159, 2.71828)]}
    res = {"n": 1}
    BK.record_min(res, times, 3)
    assert res == {"n": 1, "kernel_ms": 1.111, "kernel_event_ms": 0.5, "kernel_ms_runs": [1.235, 1.111, 2.0],
                   "torch_ms": 3.142, "torch_event_ms": 2.718, "torch_ms_runs": [3.142]}
    assert list(res) == ["n", "kernel_ms", "kernel_event_ms", "kernel_ms_runs", "torch_ms", "torch_event_ms", "torch_ms_runs"]
    four = {}
    BK.record_min(four, times, 4)
    assert four["kernel_ms"] == 1.1111 and four["kernel_ms_runs"] == [1.2346, 1.1111, 2.0] and four["torch_event_ms"] == 2.7183


def test_emit_prints_one_line_and_writes_the_line_or_the_indented_form(tmp_path, capsys):
    res = {"what": "x", "rows": [{"a": 1, "b": [1.5, 2.5]}], "ok": True}
    line_file, indented_file = tmp_path / "deep" / "line.json", tmp_path / "indented.json"
    BK.emit(res, str(line_file))
    BK.emit(res, str(indented_file), indent=1)
    BK.emit(res, None)
    assert capsys.readouterr().out == (json.dumps(res) + "\n") * 3
    assert line_file.read_text() == json.dumps(res) + "\n"
    assert indented_file.read_text() == json.dumps(res, indent=1) + "\n"
    assert json.loads(line_file.read_text()) == json.loads(indented_file.read_text()) == res
