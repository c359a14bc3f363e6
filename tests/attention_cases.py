"""Shared pieces of the attention tests (CPU only, no scl_amd import): the numpy port of the kernels' dropout hash, error measures, the
fp64 reference of  softmax((q scale) k^T) o mask . v  with its autograd gradients, and a ROUNDING MODEL of the materialised-score bf16
chain (scl_amd/encoder.py: QK^T GEMM -> scl_softmax_fwd -> scl_dropout_rows -> PV GEMM, and its backward): the same computation in fp64
with a rounding wherever the shipped chain stores a value.  The model's distance to fp64 is the floor the GPU tests' bars are multiples
of; it is computed from the reference alone."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def hash_u32(seed, idx):
    """csrc/common.h::hash_u32, bit for bit (idx: uint64 array)."""
    idx = idx.astype(np.uint64)
    seed = np.uint64(seed)
    x = ((idx & M32) * np.uint64(0x9E3779B1) & M32) ^ (((idx >> np.uint64(32)) * np.uint64(0x85EBCA77)) & M32) ^ seed
    x ^= x >> np.uint64(16); x = x * np.uint64(0x7feb352d) & M32
    x ^= x >> np.uint64(15); x = x * np.uint64(0x846ca68b) & M32
    x ^= x >> np.uint64(16)
    x = (x + (seed * np.uint64(0xC2B2AE3D) & M32)) & M32
    x ^= x >> np.uint64(15); x = x * np.uint64(0x2c1b3c6d) & M32
    x ^= x >> np.uint64(12); x = x * np.uint64(0x297a2d39) & M32
    x ^= x >> np.uint64(15)
    return x


def keep_scale_range(seed, start, n, p):
    """csrc/common.h::dropout_scale over element indices start .. start + n - 1 -> float32 factors (0 or 1 / (1 - p))."""
    u = (hash_u32(seed, np.arange(start, start + n, dtype=np.uint64)) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32))


def keep_scale(seed, n, p):
    """csrc/common.h::dropout_scale over element indices 0 .. n-1 -> float32 factors (0 or 1 / (1 - p))."""
    return keep_scale_range(seed, 0, n, p)


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def cosine(a, b):
    a = torch.as_tensor(a).double().cpu().flatten(); b = torch.as_tensor(b).double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()


def enc_masks_for(step_seed, cfg, B, T, probs):
    """The encoder's element-dropout masks of one step, as oracle.wav2vec2.forward(masks=...) takes them."""
    from scl_amd.encoder import Encoder
    p_res, p_attn, p_act, p_in = probs
    E, H, Fd = cfg.embed, cfg.heads, cfg.ffn
    ss = lambda layer, site: Encoder.site_seed(step_seed, layer, site)
    masks = {}
    if p_in > 0:
        masks["in"] = keep_scale(ss(-1, Encoder.SITE_IN), B * T * E, p_in).view(B, T, E)
    if p_res > 0:
        masks["enc"] = keep_scale(ss(-1, Encoder.SITE_ENC), B * T * E, p_res).view(B, T, E)
    for n in range(cfg.layers):
        m = {}
        if p_attn > 0:
            m["attn"] = keep_scale(ss(n, Encoder.SITE_ATTN), B * H * T * T, p_attn).view(B, H, T, T)
        if p_res > 0:
            m["d1"] = keep_scale(ss(n, Encoder.SITE_1), B * T * E, p_res).view(B, T, E)
            m["d3"] = keep_scale(ss(n, Encoder.SITE_3), B * T * E, p_res).view(B, T, E)
        if p_act > 0:
            m["d2"] = keep_scale(ss(n, Encoder.SITE_2), B * T * Fd, p_act).view(B, T, Fd)
        masks[n] = m
    return masks


# ---- fp64 attention and the rounding model of the bf16 chain ------------------------------------------------------------------------
def r32(x):
    """Round an fp64 tensor to f32 (what an f32 store keeps)."""
    return x.float().double()


def rbf(x):
    """Round an fp64 tensor to bf16 the way the kernels do: the f32 value, then round-to-nearest-even to bf16."""
    return x.float().to(torch.bfloat16).double()


def _heads(qkv):
    """qkv [B, T, 3, H, D] (any dtype) -> q, k, v fp64 [B, H, T, D]."""
    return tuple(qkv[:, :, i].double().cpu().permute(0, 2, 1, 3).contiguous() for i in range(3))


def _merge(x):
    """[B, H, T, D] -> [B, T, H * D]."""
    B, H, T, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, H * D)


def attention_fp64(qkv, dctx=None, keep=None):
    """fp64 softmax((q scale) k^T) o keep . v on the given qkv [B, T, 3, H, D] (scale = D^-1/2; keep: [B, H, T, T] factors or None).
    Returns ctx [B, T, E] and, with dctx [B, T, E], (dq, dk, dv) [B, T, H, D] each by autograd."""
    D = qkv.shape[-1]
    q, k, v = (t.requires_grad_(dctx is not None) for t in _heads(qkv))
    pr = torch.softmax((q * D ** -0.5) @ k.transpose(-1, -2), -1)
    if keep is not None:
        pr = pr * keep.double()
    ctx = _merge(pr @ v)
    if dctx is None:
        return ctx, None
    ctx.backward(dctx.double().cpu())
    return ctx.detach(), tuple(t.grad.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))


def attention_rounding_model(qkv, dctx=None, keep=None):
    """The bf16 chain of scl_amd/encoder.py in fp64 with the chain's stores rounded: S and dP to f32; P, the dropped P, dS, ctx, dQ, dK
    and dV to bf16.  Accumulation order, `__expf` and the f32 arithmetic inside a kernel are NOT modelled (exact here).  Same returns
    as attention_fp64."""
    D = qkv.shape[-1]
    sc = D ** -0.5
    q, k, v = _heads(qkv)
    S = r32((q @ k.transpose(-1, -2)) * sc)                 # QK^T GEMM, alpha = scale, f32 C
    P = rbf(torch.softmax(S, -1))                           # scl_softmax_fwd
    Pd = P if keep is None else rbf(P * keep.double())      # scl_dropout_rows (bf16 in, bf16 out)
    ctx = _merge(rbf(Pd @ v))                               # PV GEMM, bf16 C
    if dctx is None:
        return ctx, None
    B, H, T, _ = q.shape
    do = dctx.double().cpu().view(B, T, H, D).permute(0, 2, 1, 3)
    dV = rbf(Pd.transpose(-1, -2) @ do)
    dP = r32(do @ v.transpose(-1, -2))                      # f32 C
    if keep is not None:
        dP = r32(dP * keep.double())                        # scl_dropout_rows in place on the f32 buffer
    dS = rbf(P * (dP - (P * dP).sum(-1, keepdim=True)))     # scl_softmax_bwd
    dQ = rbf((dS @ k) * sc)
    dK = rbf((dS.transpose(-1, -2) @ q) * sc)
    return ctx, tuple(t.permute(0, 2, 1, 3).contiguous() for t in (dQ, dK, dV))
