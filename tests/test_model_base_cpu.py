"""The host-side pieces every model plugin shares (scl_amd.model_base, encoder.shape_entry), without a GPU or a library call: run_plan
records a forward / backward on its first run and replays it afterwards — driven here by ops.host_callback, which records a Python
callback — and the rule that sends a batch shape's state to the kept, the least-recently-used or the kept-for-training store."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scl_amd import ops  # noqa: E402
from scl_amd.encoder import FIXED, VARLEN_SETS, RowLayout, VarlenSets, shape_entry  # noqa: E402
from scl_amd.model_base import run_plan  # noqa: E402


class Step:
    """A stand-in for the kernels of a step: one recorded callback that logs its (patchable) argument."""

    def __init__(self):
        self.log, self.builds, self.patched = [], 0, []

    def build(self):
        self.builds += 1
        ops.host_callback(self.log.append, "first")
        return dict(drop_descs=["d"], saved={"T": 3})

    def patch(self, plan):
        assert ops._rec() is None
        self.patched.append(plan)
        plan["calls"][0][1][0] = "patched %d" % len(self.patched)      # as a seed goes into a recorded entry


def test_first_call_records_and_later_calls_patch_then_replay():
    s, plans = Step(), {}
    got, replayed = run_plan(plans, ("fwd", True), True, s.patch, s.build)
    assert not replayed and s.builds == 1 and s.log == ["first"] and s.patched == [] and ops._rec() is None
    assert list(plans) == [("fwd", True)] and got is plans[("fwd", True)]
    assert set(got) == {"calls", "drop_descs", "saved"} and got["drop_descs"] == ["d"] and got["saved"] == {"T": 3} and len(got["calls"]) == 1
    again = run_plan(plans, ("fwd", True), True, s.patch, s.build)
    assert again == (got, True) and again[0] is got and s.builds == 1 and s.patched == [got] and s.log == ["first", "patched 1"]      # patched before the replay
    run_plan(plans, ("fwd", True), True, s.patch, s.build)
    assert s.builds == 1 and s.log == ["first", "patched 1", "patched 2"]
    run_plan(plans, ("fwd", False), True, s.patch, s.build)      # another plan key: recorded on its own
    assert s.builds == 2 and len(plans) == 2 and len(s.patched) == 2


def test_planning_off_stores_nothing():
    s, plans = Step(), {"k": "kept as it is"}
    for _ in range(2):
        got = run_plan(plans, "k", False, s.patch, s.build)
        assert got == (dict(drop_descs=["d"], saved={"T": 3}), False) and ops._rec() is None
    assert s.builds == 2 and s.log == ["first", "first"] and s.patched == [] and plans == {"k": "kept as it is"}


def test_a_build_that_raises_stops_the_recording():
    plans, log = {}, []

    def build():
        ops.host_callback(log.append, 1)
        raise ZeroDivisionError("in the kernels")
    with pytest.raises(ZeroDivisionError, match="in the kernels"):
        run_plan(plans, "k", True, None, build)
    assert ops._rec() is None and plans == {} and log == [1]
    s = Step()
    run_plan(plans, "k", True, s.patch, s.build)      # the next step records a plan of its own, one call long
    assert len(plans["k"]["calls"]) == 1


def test_shape_entry_sends_each_kind_of_batch_to_its_store():
    evicted, made = [], []
    kept, lru, kept_train = {}, VarlenSets(on_evict=evicted.append), {}
    padded, packed = RowLayout(frames="frames"), RowLayout("frames", "row0", 64)

    def entry(key, layout, train):
        return shape_entry(key, lambda: made.append(key) or {"key": key}, layout, train, kept, lru, kept_train)
    a = entry((2, 400), FIXED, False)
    assert entry((2, 400), FIXED, True) is a and list(kept) == [(2, 400)] and not lru and not kept_train      # a fixed shape: kept, train or not
    b = entry(padded.key(2, 400), padded, False)
    c = entry(packed.key(2, 400), packed, False)
    assert list(lru) == [(2, 400), (2, 400, "packed")] and b is not a and c is not b and not kept_train
    t = entry(padded.key(2, 400), padded, True)
    assert list(kept_train) == [(2, 400)] and t is not b and entry((2, 400), padded, True) is t
    assert made == [(2, 400), (2, 400), (2, 400, "packed"), (2, 400)] and list(kept) == [(2, 400)]
    # the least recently used of VARLEN_SETS scoring shapes goes when one more arrives
    assert entry((2, 400), padded, False) is b      # (2, 400) is now the most recent
    for L in range(VARLEN_SETS - 2):
        entry((2, 500 + L), padded, False)
    assert len(lru) == VARLEN_SETS and evicted == []
    entry((2, 999), padded, False)
    assert evicted == [(2, 400, "packed")] and len(lru) == VARLEN_SETS and (2, 400) in lru
    assert len(kept) == 1 and len(kept_train) == 1
