"""The learned weighted sum over the encoder's hidden states (YAML `ssl_layer_mix`): its definition in torch, composed from the oracle,
and the shapes and bars of the tests that hold the HIP path to it (test_layer_mix_cpu.py, test_layer_mix_kernels_gpu.py,
test_layer_mix_model_gpu.py).

Definition (the convention of transformers' `output_hidden_states` for stable-layer-norm wav2vec2): h_0 is the input of layer 0 (the
positional-conv residual after its dropout, inter["pos"]), h_l for l = 1 .. L-1 the raw output of layer l-1, h_L the final LayerNorm
of the last layer's output; mix = sum_l softmax(a)_l h_l.  A layer skipped by LayerDrop hands its input on: h_{n+1} = h_n.
"""
import torch
import torch.nn.functional as F

from oracle import head as OH
from oracle import wav2vec2 as W

MIX_KEY = "layer_mix.weight"

# (Mt, E, states) of the kernel tests: ragged tail at the narrowest row; XLS-R 300M; XLS-R 2B; the cap at a packed row count
KERNEL_SHAPES = [(37, 64, 3), (222, 1024, 25), (64, 1920, 49), (512, 64, 64)]

# Bars of the kernel tests, derived from the arithmetic (nothing measured):
#   fwd      |y - y64| <= 2^-8 |y64| + 64 * 2^-24 * sum_l |s_l h_l|   one bf16 rounding + f32 accumulation of at most 64 terms
#   acc_f32, the f32 side of inject, s_L g:  2 * 2^-24 * sum |terms|   one product, one sum
#   bwd_w    1e-6 of the largest |da|: fp64 accumulation, what is left is the f32 soft-max and the f32 store
BF16_EPS, F32_EPS = 2.0 ** -8, 2.0 ** -24
BWD_W_REL = 1e-6


def hidden_states(ssl_sd, cfg, x, masks=None, skip_last=False):
    """[h_0 .. h_L], each [B, T, E], in the dtype of the state dict.  skip_last: the last layer is skipped (LayerDrop), so its raw output is
    its input and h_L the final LayerNorm of that."""
    h, inter = W.forward(ssl_sd, cfg, x, return_all=True, masks=masks)
    raw = [inter["pos"]] + list(inter["layers"])
    if skip_last:
        raw[-1] = raw[-2]
        h = F.layer_norm(raw[-1], (cfg.embed,), ssl_sd["encoder.layer_norm.weight"], ssl_sd["encoder.layer_norm.bias"], 1e-5)
    return raw[:-1] + [h]


def mix_of(states, logits=None, weights=None):
    s = torch.softmax(logits, dim=0) if weights is None else weights
    return sum(s[l] * h for l, h in enumerate(states))


def full_forward(ssl_sd, head_sd, cfg, x, logits, skip_last=False, dropout_masks=None, enc_masks=None):
    """(log-probs, feats, emb) of the linear plugin with the mix in front of LL."""
    return OH.head_forward(head_sd, mix_of(hidden_states(ssl_sd, cfg, x, enc_masks, skip_last), logits), dropout_masks)


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def reference_grads(ssl_sd, head_sd, cfg, x, y, logits, skip_last=False, loss_type=1):
    """fp64 autograd through the definition, the head and the loss: ((out, feats, emb), {state-dict name: gradient}).  A parameter the
    graph does not reach (a skipped layer's) has gradient zero."""
    ssl, head, a = to64(ssl_sd), to64(head_sd), logits.double().clone()
    names = [n for n, _, tr in W.param_shapes(cfg) if tr]
    leaves = {"ssl_model.model." + n: ssl[n] for n in names}
    leaves.update(head)
    leaves[MIX_KEY] = a
    for p in leaves.values():
        p.requires_grad_(True)
    out, feats, emb = full_forward(ssl, head, cfg, x.double(), a, skip_last)
    total = sum(OH.model_loss(out, feats, emb, y, loss_type).values())
    gs = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {k: (torch.zeros_like(p) if g is None else g).detach() for (k, p), g in zip(leaves.items(), gs)}
    return (out.detach(), feats.detach(), emb.detach()), grads
