"""Conv layers 1..6 of the feature extractor as the encoder composes them, layer by layer against fp64 (tests/conv_stack_cases.py).

One real training step of the linear model (forward, seeded Gaussian cotangents on its three outputs, backward), then a second one on
another input: after each, every stage i = 6..1 is compared with stage_reference fed that stage's own stored inputs (z[i - 1], dz[i], the
master weight at its bf16 rounding, the fp32 vectors) — the forward GEMM over overlapping rows, LayerNorm + GELU, the LayerNorm backward
into the zero-padded dyp rows, the split-K weight gradient with conv_weight_unpack_grad, the phase-split transposed convolution, and the
Q / Qe / Rp / Up geometry of Encoder._make_bufs.  Before each step the frame region of every z, y and dz is NaN, so a row the step does
not write shows; dyp's padding rows (zeroed once, by design) and dz's left-over rows must be exactly 0 after both steps.

Bars: tests/conv_stack_cases.py::BARS.  bf16-limited tensors: twice what the fp64 reference with the encoder's permitted roundings gives
on the CPU (EMU; tests/test_conv_stack_cases_cpu.py asserts it).  Nothing is excluded from any comparison.

Worst values measured on the MI355X over the four cases and both steps, as "measured / emulated / bar":
    z    rel-L2 1.690e-3 / 1.72e-3 / 3.44e-3   max 3.548e-3 / 3.2e-3 / 6.4e-3    boundary rows 2.784e-3 / 2.9e-3 / 5.8e-3
    dyp  rel-L2 1.755e-3 / 1.68e-3 / 3.36e-3   max 3.387e-3 / 2.65e-3 / 5.3e-3   boundary rows 2.841e-3 / 2.75e-3 / 5.5e-3
    dz   rel-L2 2.473e-3 / 2.37e-3 / 4.74e-3   max 4.680e-3 / 4.2e-3 / 8.4e-3    boundary rows 3.795e-3 / 3.4e-3 / 6.8e-3
    dW   rel-L2 2.048e-3 / 1.68e-3 / 3.36e-3   max 2.399e-3 / 2.35e-3 / 4.7e-3
    y 1.5e-2 of its per-element bound; mean 4.5e-7 (bar 1e-5), rstd 1.3e-7 (2e-5), dgamma 3.8e-7 (5e-5), dbeta 2.5e-7 (5e-5),
    conv bias gradient 4.0e-7 (2e-4).  Every padding row of dyp and every left-over row of dz was exactly 0 after both steps.
All four cases passed on first contact with the kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import conv_stack_cases as CS  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
PRE = "ssl_model.model."
FE = PRE + "feature_extractor.conv_layers.%d."


class Report:
    """Collects every metric against its bar; the test fails once, listing everything over its bar."""

    def __init__(self, tag, bars):
        self.tag, self.bars, self.worst, self.fails, self.step = tag, bars, {}, [], 0

    def check(self, kind, name, value):
        bar = self.bars[kind]
        name = "step %d %s" % (self.step, name)
        if not (value == value) or value > bar:
            self.fails.append("%s %s: %.3e > %.3e" % (kind, name, value, bar))
        w = self.worst.get(kind)
        if w is None or not value <= w[0]:
            self.worst[kind] = (value, name)

    def require(self, ok, what):
        if not ok:
            self.fails.append("step %d %s" % (self.step, what))

    def done(self):
        print("\n[%s] worst:" % self.tag, ", ".join("%s %.3e (%s)" % (k, v, n) for k, (v, n) in sorted(self.worst.items())))
        assert not self.fails, "%s: %d over the bar:\n  %s" % (self.tag, len(self.fails), "\n  ".join(self.fails))


def build(dev, width):
    kw = CS.config_kwargs(width)
    ocfg = W.W2VConfig(**kw)
    ssl, head = W.init_state(ocfg, seed=31), OH.init_head(ocfg.embed, seed=32)
    m = Model(ARGS, dev, w2v_cfg=W2VConfig(**kw))      # every encoder dropout is 0 in W2VConfig's defaults
    sd = {PRE + k: v for k, v in ssl.items()}
    sd.update(head)
    _, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.eval()      # the head's dropout off
    return m


def poison(d, Bn, C):
    """NaN over the frame region [0, B t C) of every z, y and dz; the slack tails and dyp stay as they are."""
    for i, t in enumerate(d["Ts"]):
        n = Bn * t * C
        d["z"][i][:n].fill_(float("nan"))
        d["dz"][i][:n].fill_(float("nan"))
        if d["y"][i] is not None:
            d["y"][i][:n].fill_(float("nan"))


def step(m, x, cot):
    out, feats, emb = m(x)
    for p in m.parameters():
        p.grad = None
    ((out * cot[0]).sum() + (feats * cot[1]).sum() + (emb * cot[2]).sum()).backward()
    torch.cuda.synchronize()


def check_stages(rep, m, d, Bn):
    cfg, P = m.cfg, m.P
    C, Ts = cfg.conv_dim, d["Ts"]
    frames = lambda buf, t: buf[: Bn * t * C].view(Bn, t, C).cpu()
    for i, t in enumerate(Ts):      # precondition: a real gradient reached every layer
        g = frames(d["dz"][i], t).float()
        rep.require(bool(torch.isfinite(g).all()) and bool(g.any()), "dz[%d] is not finite and non-zero" % i)
    for i in reversed(range(1, len(Ts))):
        k, s, Tin, Tout = cfg.conv_kernels[i], cfg.conv_strides[i], Ts[i - 1], Ts[i]
        Q, Rp = d["dyp_geom"][i]
        vec = lambda name: P.f32(FE % i + name).float().cpu()
        w = P.f32(FE % i + "0.weight").to(torch.bfloat16).float().cpu().view(C, C, k)
        ref = CS.stage_reference(frames(d["z"][i - 1], Tin), w, vec("0.bias"), vec("2.1.weight"), vec("2.1.bias"), frames(d["dz"][i], Tout), s)
        dyp = d["dyp"][i].cpu()
        got = dict(y=d["y"][i].view(Bn, Tout, C).cpu(), mean=d["cmean"][i].view(Bn, Tout).cpu(), rstd=d["crstd"][i].view(Bn, Tout).cpu(),
                   z=frames(d["z"][i], Tout), dy=CS.dyp_frames(dyp, Bn, C, Q, Rp, Tout), dz_prev=frames(d["dz"][i - 1], Tin),
                   dw=P.g(FE % i + "0.weight").view(C, C, k).cpu(), db=P.g(FE % i + "0.bias").cpu(),
                   dgamma=P.g(FE % i + "2.1.weight").cpu(), dbeta=P.g(FE % i + "2.1.bias").cpu())
        tag = "layer %d (Tin %d%s)" % (i, Tin, ", left-over" if CS.leftover(Tin, k, s) else "")
        for kind, v in CS.stage_metrics(got, ref).items():
            rep.check(kind, tag, v)
        pad = CS.dyp_padding(dyp, Bn, C, Q, Rp, Tout)
        rep.require(Rp >= Q + Tout and bool((pad == 0).all()), "%s: a padding row of dyp is not 0" % tag)
        rows = list(CS.unreached_rows(Tin, k, s))
        rep.require(len(rows) == CS.leftover(Tin, k, s) and bool((got["dz_prev"][:, rows] == 0).all()),
                    "%s: a left-over row of dz[%d] is not 0" % (tag, i - 1))


@pytest.mark.parametrize("width,L", CS.CASES, ids=["%s-%d" % c for c in CS.CASES])
def test_conv_stack_layers_against_fp64(dev, width, L):
    m = build(dev, width)
    Bn, C = CS.B, m.cfg.conv_dim
    d = m.encoder.bufs(Bn, L, train=True)
    assert d["Ts"] == W2VConfig().conv_lens(L)
    T = d["T"]
    g = torch.Generator().manual_seed(7)
    cot = [torch.randn(Bn, 2, generator=g).to(dev), torch.randn(Bn, T, 128, generator=g).to(dev), torch.randn(Bn, 128, generator=g).to(dev)]
    rep = Report("conv stack %s L=%d" % (width, L), CS.BARS)
    for n in range(2):      # the second step replays the recorded plans on another input: stale state, dirty slabs, overwritten padding
        rep.step = n + 1
        x = (0.1 * torch.randn(Bn, L, generator=torch.Generator().manual_seed(1000 * n + L))).to(dev)
        poison(d, Bn, C)
        step(m, x, cot)
        assert m.encoder.bufs(Bn, L, train=True) is d
        check_stages(rep, m, d, Bn)
    rep.done()
