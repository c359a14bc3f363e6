"""scl_amd.plan_pool.PlanPool, the pool resstack.py and graph.py keep their per-shape plans in: hand-out, the busy flag, the generation
stamp, the cap per shape, eviction and the finaliser — on a stand-in plan class, plain objects as autograd contexts, no GPU."""
import gc
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scl_amd.plan_pool import PlanPool, _release, _storages  # noqa: E402


class Plan:
    def __init__(self, key, dev="gpu0"):
        self.key, self.dev, self.busy = key, dev, False


class Ctx:
    pass


def acquire(pool, key, hold, dev="gpu0"):
    return pool.acquire(key, dev, hold, lambda: Plan(key, dev))


def test_an_idle_plan_is_handed_out_again_and_a_busy_one_is_not():
    pool = PlanPool()
    a = acquire(pool, (2, 3), hold=False)
    assert (a.gen, a.busy, pool.plans) == (1, False, [a])
    b = acquire(pool, (2, 3), hold=True)
    assert b is a and (a.gen, a.busy) == (2, True)
    c = acquire(pool, (2, 3), hold=True)      # a's backward is pending: a second plan
    assert c is not a and c.gen == 1 and pool.plans == [a, c]
    assert acquire(pool, (2, 3), hold=False, dev="gpu1") not in (a, c)      # the same shape on another device
    a.busy = False
    assert acquire(pool, (2, 3), hold=False) is a and a.gen == 3


def test_the_cap_of_live_plans_per_shape():
    pool = PlanPool()
    assert PlanPool.MAX_LIVE_PLANS == 16
    held = [acquire(pool, "k", hold=True) for _ in range(PlanPool.MAX_LIVE_PLANS)]
    assert len({id(p) for p in held}) == 16
    with pytest.raises(RuntimeError, match="16 forward passes of shape 'k' are waiting for their backward"):
        acquire(pool, "k", hold=True)
    assert acquire(pool, "other", hold=True).key == "other"      # the cap is per shape
    held[3].busy = False
    assert acquire(pool, "k", hold=True) is held[3]


def test_a_new_key_evicts_the_oldest_idle_plan_of_a_full_pool():
    pool = PlanPool()
    plans = [acquire(pool, i, hold=True) for i in range(8)]
    plans[5].busy = plans[2].busy = False
    new = acquire(pool, "new", hold=True)
    assert plans[2] not in pool.plans and plans[5] in pool.plans and pool.plans[-1] is new and len(pool.plans) == 8
    for p in pool.plans:
        p.busy = True
    acquire(pool, "more", hold=True)      # nothing idle: the pool grows
    assert len(pool.plans) == 9
    small = PlanPool()
    idle = [acquire(small, i, hold=False) for i in range(7)]
    acquire(small, "eighth", hold=False)      # below 8 plans nothing is evicted
    assert small.plans[:7] == idle and len(small.plans) == 8


def test_the_generation_stamp_guards_backward_and_release():
    pool = PlanPool()
    pl = acquire(pool, "k", hold=True)
    ctx = Ctx()
    pool.hold(ctx, pl)
    assert ctx.pl is pl and ctx.gen == 1 and pool.owned(ctx) is pl
    pl.busy = False
    assert acquire(pool, "k", hold=True) is pl and pl.gen == 2      # handed out again: the first node no longer owns it
    with pytest.raises(RuntimeError, match=r"re-used by a later forward \(generation 2, node holds 1\)"):
        pool.owned(ctx)
    _release(pl, 1)      # the first node's late release
    assert pl.busy is True
    _release(pl, 2)
    assert pl.busy is False


def test_a_dropped_context_frees_its_plan_and_an_unheld_one_gets_no_finaliser():
    pool = PlanPool()
    pl = acquire(pool, "k", hold=True)
    ctx = Ctx()
    pool.hold(ctx, pl)
    del ctx
    gc.collect()
    assert pl.busy is False
    free = acquire(pool, "k", hold=False)
    assert free is pl and pl.gen == 2
    ctx = Ctx()
    pool.hold(ctx, free)
    pl.busy = True      # as a later grad-mode forward of generation 2 would: a finaliser of this context would clear it
    del ctx
    gc.collect()
    assert pl.busy is True


def test_storages_keeps_storages_not_tensors():
    a, b, c = torch.zeros(3), torch.zeros(2, 2), torch.zeros(1)
    got = _storages(a, (b, [c, None]), None, 7)
    ptr = lambda s: s.data_ptr()
    assert ptr(got[0]) == a.untyped_storage().data_ptr() and not torch.is_tensor(got[0])
    assert isinstance(got[1], tuple) and ptr(got[1][0]) == b.untyped_storage().data_ptr()
    assert ptr(got[1][1][0]) == c.untyped_storage().data_ptr() and got[1][1][1] is None
    assert got[2] is None and got[3] == 7 and len(got) == 4
