"""The pool of per-shape plans (buffers + recorded launch sequences) of a back-end that is one autograd node: resstack.py and graph.py keep
one PlanPool each.  A plan is any object with `.key`, `.dev` and `.busy`; the pool stamps `.gen`.

A plan is busy from a grad-mode forward until its backward.  A busy plan is never handed out (its saved maps, statistics, dropout seeds and
recorded pointers belong to the waiting node): a further forward of the same shape gets a fresh plan, up to MAX_LIVE_PLANS per shape.  A
node freed without a backward gives its plan back through the finaliser hold() attaches; the generation stamp keeps a late finaliser, or
a backward of a node whose plan was handed out again, from touching a plan that is no longer its own.
"""
import weakref

import torch


def _storages(*ts):
    """What a plan keeps of the tensors its in-flight kernels read / write: the STORAGE (the memory stays allocated), never the tensor
    object — an output tensor carries its grad_fn, and a plan that held it would keep its own autograd node (and through ctx.pl itself)
    alive until the next forward of the shape, so a graph dropped without a backward could never hand its plan back."""
    out = []
    for t in ts:
        if isinstance(t, (tuple, list)):
            out.append(_storages(*t))
        elif torch.is_tensor(t):
            out.append(t.untyped_storage())
        else:
            out.append(t)
    return tuple(out)


def _release(pl, gen):
    if pl.gen == gen:
        pl.busy = False


class PlanPool:
    MAX_LIVE_PLANS = 16      # plans of one (key, device), busy or not
    MAX_POOL = 8             # from this many plans on, a new plan evicts the oldest idle one

    def __init__(self):
        self.plans = []

    def acquire(self, key, dev, hold, make):
        """An idle plan of (key, dev), or `make()`'s new one; busy from now on when `hold`."""
        for pl in self.plans:
            if pl.key == key and pl.dev == dev and not pl.busy:
                pl.busy = hold
                pl.gen = getattr(pl, "gen", 0) + 1
                return pl
        same = [pl for pl in self.plans if pl.key == key and pl.dev == dev]
        if len(same) >= self.MAX_LIVE_PLANS:
            raise RuntimeError("%d forward passes of shape %r are waiting for their backward; run the backwards (or drop the graphs) "
                               "before another forward of this shape" % (len(same), key))
        idle = [pl for pl in self.plans if not pl.busy]
        if len(self.plans) >= self.MAX_POOL and idle:
            self.plans.remove(idle[0])
        pl = make()
        pl.busy = hold
        pl.gen = 1
        self.plans.append(pl)
        return pl

    @staticmethod
    def hold(ctx, pl):
        """Ties the plan to the autograd node: generation stamp for the backward's ownership check, release when the node dies unused."""
        ctx.pl, ctx.gen = pl, pl.gen
        if pl.busy:
            weakref.finalize(ctx, _release, pl, pl.gen)

    @staticmethod
    def owned(ctx):
        pl = ctx.pl
        if pl.gen != ctx.gen:
            raise RuntimeError("this node's plan was re-used by a later forward (generation %d, node holds %d): its saved activations are gone" % (pl.gen, ctx.gen))
        return pl
