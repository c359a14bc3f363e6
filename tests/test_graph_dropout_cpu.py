"""The reference of tests/test_graph_dropout_gpu.py on its own (no GPU): the fp64 graph module of oracle/aasist_head.py with the 19 dropout
masks of scl_amd/graph.py rebuilt on the host (tests/graph_dropout_cases.py).  With p = 0 it is the oracle's graph part bit for bit; it is
a function of the seeds; every mask keeps its share; a backward that hashes another seed than its forward at ANY ONE of the 19 sites
moves a compared gradient by at least 100 times the GPU test's bar; and the GraphPool scores of every case the GPU test runs are at least
2e-6 apart at the top-k cut, so that fp32 and fp64 select the same nodes."""
import functools
import math

import pytest
import torch

from oracle import aasist_head as OH
from scl_amd.graph import _SEED_NAMES
from tests import graph_dropout_cases as C


def test_seed_names_map_to_the_sites_of_the_reference():
    table = {"in_S": ("GAT_layer_S.input_drop", 0), "in_T": ("GAT_layer_T.input_drop", 0), "in_11": ("HtrgGAT_layer_ST11.input_drop", 0),
             "in_21": ("HtrgGAT_layer_ST21.input_drop", 0), "in_12": ("HtrgGAT_layer_ST12.input_drop", 0), "in_22": ("HtrgGAT_layer_ST22.input_drop", 0),
             "pool_S": ("pool_S.drop", 0), "pool_T": ("pool_T.drop", 0), "pool_S1": ("pool_hS1.drop", 0), "pool_T1": ("pool_hT1.drop", 0),
             "pool_S2": ("pool_hS2.drop", 0), "pool_T2": ("pool_hT2.drop", 0), "way_T0": ("drop_way", 0), "way_T1": ("drop_way", 1),
             "way_S0": ("drop_way", 2), "way_S1": ("drop_way", 3), "way_M0": ("drop_way", 4), "way_M1": ("drop_way", 5), "drop": ("drop", 0)}
    assert sorted(table) == sorted(_SEED_NAMES) and len(set(_SEED_NAMES)) == 19
    assert {n: C.site_of(n) for n in _SEED_NAMES} == table
    ref = C.masked_reference(C.head_state(C.HEAD_SEED[(2, 33)]))
    probs = {n: s.p for s in ref.mask_sites for n in s.names}
    assert all(probs[n] == (0.3 if n.startswith("pool") else 0.5 if n == "drop" else 0.2) for n in _SEED_NAMES), probs


def test_step_seeds_mirror_the_modules_generator():
    from scl_amd import graph
    old = graph._SEED[0]
    try:
        graph.seed(2 ** 31 + 12345)
        want = [{n: graph._next_seed() for n in _SEED_NAMES} for _ in range(3)]
    finally:
        graph._SEED[0] = old
    got = C.step_seeds(2 ** 31 + 12345, 3)
    assert got == want
    flat = [v for s in got for v in s.values()]
    assert len(set(flat)) == 57 and all(0 <= v < 2 ** 31 for v in flat)      # no two sites and no two steps share a seed


@functools.lru_cache(maxsize=None)
def _run(shape):
    """The reference's STEPS training steps and the eval call of one GPU case, BatchNorm buffers carried along."""
    B, nT = shape
    ref = C.masked_reference(C.head_state(C.HEAD_SEED[shape]))
    probs = {n: s.p for s in ref.mask_sites for n in s.names}
    seeds = C.step_seeds(C.STREAM_SEED[shape], C.STEPS)
    steps = [C.ref_step(ref, seeds[i], *C.step_inputs(B, nT, i)) for i in range(C.STEPS)]
    ref.eval()
    with torch.no_grad():
        ev = C.ref_step(ref, seeds[-1], *C.step_inputs(B, nT, C.STEPS))
    return steps, ev, probs


@pytest.mark.parametrize("shape", C.SHAPES)
def test_with_p_zero_the_masked_reference_is_the_oracles_graph_part(shape):
    B, nT = shape
    sd = C.head_state(C.HEAD_SEED[shape])
    ref = C.masked_reference(sd, p=0.0)
    plain = OH.AasistHead().double()
    plain.load_state_dict({k: v.to(plain.state_dict()[k].dtype) for k, v in sd.items()})
    plain.train()
    for m in plain.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    e_S, e_T, wl, wh = C.step_inputs(B, nT, 0)
    got = C.ref_step(ref, C.step_seeds(5, 1)[0], e_S, e_T, wl, wh)
    assert sorted(got["masks"]) == sorted(_SEED_NAMES) and all(bool((m == 1).all()) for m in got["masks"].values())
    xs, xt = e_S.double().requires_grad_(True), e_T.double().requires_grad_(True)
    logits, hidden = plain.graph(xs, xt)
    ((logits * wl.double()).sum() + (hidden * wh.double()).sum()).backward()
    assert torch.equal(got["logits"], logits) and torch.equal(got["hidden"], hidden)
    assert torch.equal(got["deS"], xs.grad) and torch.equal(got["deT"], xt.grad)
    want = {n: p.grad for n, p in plain.named_parameters() if p.grad is not None}
    assert sorted(want) == sorted(got["grads"]) and len(want) == 122 and all(torch.equal(got["grads"][n], g) for n, g in want.items())
    bufs = dict(plain.named_buffers())
    assert all(torch.equal(b, bufs[n]) for n, b in ref.named_buffers())


def test_the_reference_is_a_function_of_the_seeds():
    shape = (2, 33)
    sd = C.head_state(C.HEAD_SEED[shape])
    inputs = C.step_inputs(*shape, 0)
    s1, s2 = C.step_seeds(7, 1)[0], C.step_seeds(8, 1)[0]
    a, b, c = (C.ref_step(C.masked_reference(sd), s, *inputs) for s in (s1, s1, s2))
    for k in ("logits", "hidden", "deS", "deT"):
        assert torch.equal(a[k], b[k]) and not torch.equal(a[k], c[k]), k
    assert all(torch.equal(a["masks"][n], b["masks"][n]) and not torch.equal(a["masks"][n], c["masks"][n]) for n in _SEED_NAMES)
    # a mask follows its own site's seed alone, and no two sites of a step share a mask
    one = dict(s1, in_12=s2["in_12"])
    d = C.ref_step(C.masked_reference(sd), one, *inputs)
    assert all(torch.equal(a["masks"][n], d["masks"][n]) == (n != "in_12") for n in ("in_S", "in_T", "in_11", "in_21", "in_12", "pool_S", "pool_T"))
    assert not torch.equal(a["masks"]["in_11"], a["masks"]["in_21"]) and not torch.equal(a["masks"]["way_M0"], a["masks"]["way_M1"])


@pytest.mark.parametrize("shape", C.SHAPES)
def test_every_mask_keeps_its_share(shape):
    """The zero share of each of the 19 masks of each step is within 4 binomial standard deviations of the site's p, and the kept
    elements carry 1 / (1 - p) in fp32."""
    B, nT = shape
    steps, _, probs = _run(shape)
    kT, kS = max(int(nT * 0.5), 1), 21
    numel = {"in_S": B * 42 * 64, "in_T": B * nT * 64, "in_11": B * (kT + kS) * 64, "in_21": B * (kT + kS) * 64, "in_12": B * (kT // 2 + 10) * 32,
             "in_22": B * (kT // 2 + 10) * 32, "pool_S": B * 42 * 64, "pool_T": B * nT * 64, "pool_S1": B * kS * 32, "pool_S2": B * kS * 32,
             "pool_T1": B * kT * 32, "pool_T2": B * kT * 32, "way_T0": B * (kT // 2) * 32, "way_T1": B * (kT // 2) * 32, "way_S0": B * 10 * 32,
             "way_S1": B * 10 * 32, "way_M0": B * 32, "way_M1": B * 32, "drop": B * 160}
    for i, st in enumerate(steps):
        assert sorted(st["masks"]) == sorted(_SEED_NAMES)
        for n, m in st["masks"].items():
            p, cnt = probs[n], m.numel()
            assert cnt == numel[n], (n, cnt, numel[n])
            share = float((m == 0).double().mean())
            assert abs(share - p) <= 4 * math.sqrt(p * (1 - p) / cnt), (shape, i, n, share, p, cnt)
            kept = m[m != 0]
            assert bool((kept == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)))).all()), n


@pytest.mark.parametrize("shape", C.SHAPES)
def test_a_backward_with_another_seed_at_any_one_site_moves_a_gradient_by_100_bars(shape):
    """Sensitivity of the GPU comparison: at each of the 19 sites in turn the backward gets another seed than the forward; the largest
    deviation over d e_S, d e_T (bar 2e-4) and the parameter gradients (bar 5e-4), each in units of its bar, is at least 100.  Smallest
    ratio reached over the sites, per shape: (2, 33) 5.7e2 (pool_S2); (3, 67) 3.3e2 (way_S0); (5, 66) 2.0e3 (pool_T); (2, 80) 1.0e3
    (pool_S)."""
    B, nT = shape
    ref = C.masked_reference(C.head_state(C.HEAD_SEED[shape]))
    seeds = C.step_seeds(C.STREAM_SEED[shape], 1)[0]
    base = C.ref_step(ref, seeds, *C.step_inputs(B, nT, 0), retain=True)
    names = sorted(base["grads"])
    params = dict(ref.named_parameters())

    def grads_with(bwd):
        for site in ref.mask_sites:
            site.bwd = {n: bwd[n] for n in site.names}
        gs = torch.autograd.grad(base["loss"], list(base["leaves"]) + [params[n] for n in names], retain_graph=True)
        return gs[0], gs[1], dict(zip(names, gs[2:]))

    deS, deT, grads = grads_with(seeds)
    assert torch.equal(deS, base["deS"]) and torch.equal(deT, base["deT"]) and all(torch.equal(grads[n], base["grads"][n]) for n in names)
    ratios = {}
    for site in _SEED_NAMES:
        bS, bT, bg = grads_with(dict(seeds, **{site: seeds[site] ^ 0x2545F491}))
        r = max(C.relerr(bS, deS), C.relerr(bT, deT)) / C.BARS["din"]
        for n in names:
            if not n.endswith(C.BN_BIASES):
                r = max(r, C.relerr(bg[n], grads[n]) / C.BARS["param"])
        ratios[site] = r
    worst = min(ratios, key=ratios.get)
    print("sensitivity %s: smallest ratio %.3e at %s" % (shape, ratios[worst], worst))
    assert ratios[worst] >= 100, ratios


@pytest.mark.parametrize("shape", C.SHAPES)
def test_topk_scores_of_every_gpu_case_are_apart(shape):
    """Precondition of the GPU comparison (it rests on the reference alone): over the six GraphPools and all utterances of every step
    and of the eval call, the fp64 scores at the top-k cut are at least 2e-6 apart behind the masks.  Smallest gaps met: (2, 33) 4.0e-4;
    (3, 67) 1.2e-5 (its eval call); (5, 66) 6.2e-5; (2, 80) 2.1e-5."""
    steps, ev, _ = _run(shape)
    gaps = [st["gap"] for st in steps] + [ev["gap"]]
    print("top-k gaps %s: %s" % (shape, " ".join("%.3e" % g for g in gaps)))
    assert min(gaps) >= C.MIN_GAP, gaps


def test_topk_scores_of_the_whole_back_end_case_are_apart():
    """The same precondition for the whole back-end case.  Gap met: 1.5e-3."""
    c = C.BACKEND
    ref = C.masked_reference(C.head_state(c["head_seed"]))
    out = C.backend_step(ref, C.step_seeds(c["stream_seed"], 1)[0], *C.backend_inputs())
    print("top-k gap of the back-end case: %.3e" % out["gap"])
    assert out["gap"] >= C.MIN_GAP
    assert out["masks"]["in_T"].shape == (c["B"], c["frames"] // 3, 64) and out["dfeats"].abs().max() > 0
