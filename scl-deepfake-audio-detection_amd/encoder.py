"""wav2vec2 / XLS-R encoder: forward and hand-scheduled backward over the HIP kernels.

What the reference gets from `fairseq Wav2Vec2Model.forward(src, mask=False, features_only=True)['x']`
(model/xlsr.py:41) and from autograd's backward through it (main.py:79).
Layout decisions (MI355X-first, not fairseq's):
  * activations are channels-last [B, T, C] everywhere, so every Conv1d of the feature extractor is
    a plain GEMM whose A rows overlap (ld = stride*C) — no im2col buffer, no transposes;
  * GEMM operands are bf16, accumulation fp32; the residual stream, LayerNorm statistics, softmax
    and all gradients of parameters are fp32;
  * q/k/v projections are one [3E, E] GEMM; attention scores are materialised per layer as bf16
    P[B,H,T,Tp] (41 MB at B=32) and reused by the backward — HBM is 288 GB, recompute buys nothing here;
  * every buffer is allocated once per (B, L) and reused across steps (no allocator traffic).
"""
import collections
import collections.abc
import contextlib
import os

import torch

from . import ops
from .lib import ACT_GELU, ACT_GELU_DC2, FLAT, RACT_STORED, SclError
from .ops import Op

# the four weight gradients of a transformer layer as ONE grouped launch at the end of the layer's backward (ops.gemm_group: 16 + 48 + 64 + 64
# tiles of 256 x 256, every block walks the whole reduction, finished tiles go straight into the flat gradient buffer): no split-K slabs, no
# slab reduction, 5 launches -> 1.  SCL_WGRAD_GROUP=0: one split-K launch per gradient + the layer's slab combine, as rounds 2-4 ran.
# Engaged when the group covers at least 3/8 of the CUs and the reduction has at least WGRAD_GROUP_MIN_KSTEPS steps of 64 rows.
WGRAD_GROUP = os.environ.get("SCL_WGRAD_GROUP", "1") != "0"
WGRAD_CARRY = os.environ.get("SCL_WGRAD_CARRY", "1") != "0"      # carry a layer's tile remainder into the next layer's launch (whole rounds of 256 tiles)
WGRAD_GROUP_MIN_KSTEPS = 16      # from 1024 rows on (measured: 11 x 199 rows 16.2 -> 14.2 ms per step, 16 x 199 20.8 -> 17.6, 32 x 199 29.1 -> 26.1, 64 x 199 44.1 -> 42.5)
# BASELINE.json configs[4] names fp8 attention: csrc/attention_fp8.hip (e4m3 operands, fp32 accumulation) for the no-grad bf16 forward.  Opt-in:
# the reference is fp32 and the fused forward is bound by its soft-max VALU work, not by the matrix pipe (profiles/r4_attn_fp8_probe.txt).
ATTN_FP8 = os.environ.get("SCL_ATTN_FP8", "0") == "1"
# Attention above 512 frames: the streaming kernels of csrc/attention_long.hip (64-wide heads) and csrc/attention_wide.hip (72- to
# 128-wide heads), no T x T buffer.  SCL_ATTN_LONG=1 sends 225-512 frames there too (same-box A/B against the materialised-score path,
# which stays the default there).
ATTN_LONG = os.environ.get("SCL_ATTN_LONG", "0") == "1"
MAT_ATTN_MAX_T = 512      # the materialised path's soft-max keeps a whole score row in registers (csrc/attention.hip)
# fp32 scoring path above 512 frames: utterances per chunk of the materialised f32 attention such that S (and Pm) stay within this many bytes
F32_ATTN_CHUNK_BYTES = 1 << 30
SCORE_X3PLANES = os.environ.get("SCL_SCORE_X3PLANES", "1") != "0"      # fp32 scoring path: plain linears as one bf16 GEMM over [hi | hi | lo] x [hi | lo | hi] (forward_f32)


# Variable-length batches on the bf16 path (training, and scoring with SCL_SCORE_FP32=0): run the transformer layers on the valid frames
# only, packed back to back (csrc/attention_packed.hip).  Opt-in (SCL_VARLEN_PACK=1); the callers read the attribute at call time.
VARLEN_PACK = os.environ.get("SCL_VARLEN_PACK", "0") == "1"
# The packed row count of a step is rounded up to a multiple of PACK_ROWS (ops.packed_rows): launch plans are recorded per row count, so
# the bucket width trades rows wasted per step (< PACK_ROWS) against the number of plans (at most roundup(B * T, 64) / PACK_ROWS + 1 per
# direction: 25 at 64 x 199 frames).  A multiple of 64: the weight-gradient reductions walk 64 rows per K step.
PACK_ROWS = 512
# The same layout for the fp32 scoring path (forward_f32 with packed=(row0, Mq)): its attention is then the streaming pair-form kernel of
# csrc/attention_f32.hip — no T x T score buffers, no chunk loop, no padded rows in the layers.  Opt-in (SCL_SCORE_PACK=1), read at call
# time; SCL_VARLEN_PACK does not reach the fp32 path.  The head dims of the streaming family (stream_attn_takes): 72..128 run
# csrc/attention_f32_wide.hip behind the same entry.
SCORE_PACK = os.environ.get("SCL_SCORE_PACK", "0") == "1"


def stream_attn_takes(head_dim):
    """Whether the streaming attention kernels (fixed, zero-padded and packed rows in bf16, packed rows in fp32) take this head dim: 64,
    or 72..128 in steps of 8 (XLS-R 300M: 64, 1B: 80, 2B: 120).  The fused on-chip kernels take 64 only."""
    return head_dim == 64 or (64 < head_dim <= 128 and head_dim % 8 == 0)


STREAM_ATTN_HEAD_DIMS = "head dim 64, or 72..128 in steps of 8"

VARLEN_SETS = 4      # buffer sets kept per path for variable-length scoring batches (every distinct padded shape is a set of its own)


class VarlenSets(collections.OrderedDict):
    """Least-recently-used store of the buffer sets of variable-length batches: at most VARLEN_SETS entries; an evicted set is dropped
    (its device memory returns to the allocator once no launch plan refers to it).  `on_evict(key)` lets the owner drop what it keeps
    per key besides."""

    def __init__(self, on_evict=None):
        super().__init__()
        self.on_evict = on_evict

    def get_or_make(self, key, make):
        if key in self:
            self.move_to_end(key)
            return self[key]
        while len(self) >= VARLEN_SETS:
            old, _ = self.popitem(last=False)
            if self.on_evict is not None:
                self.on_evict(old)
        self[key] = make()
        return self[key]


def shape_entry(key, make, layout, train, kept, lru, kept_train):
    """What is kept per batch shape (an encoder buffer set, a model's boundary state) under `key`, made on first use, in the store of its
    kind: a fixed shape's is kept for ever (`kept`); a variable-length scoring batch's lives in a VarlenSets (`lru`: every padded length is a
    shape of its own); a variable-length training batch's (train: what it saved waits for the backward) is kept (`kept_train`)."""
    if not layout.fixed and not train:
        return lru.get_or_make(key, make)
    store = kept if layout.fixed else kept_train
    if key not in store:
        store[key] = make()
    return store[key]


class RowLayout(collections.namedtuple("RowLayout", "frames row0 Mq", defaults=(None, None, None))):
    """How the rows of a [B, T] batch are laid out, the host-side twin of `enum class Rows` (csrc/attn_stream_body.h): fixed (every frame of
    every utterance counts), padded (frames: int32 [B] on the device, the valid frames of each zero-padded utterance) or packed (row0 besides:
    int32 [B + 1] on the device, the row offsets of the valid frames back to back; Mq rows per launch, a multiple of 64, ops.packed_rows)."""
    __slots__ = ()
    BAD_MQ = "encoder: packed row count %d: need a multiple of 64"

    def __new__(cls, frames=None, row0=None, Mq=None):
        if (row0 is not None or Mq is not None) and frames is None:
            raise ValueError("encoder: packed=(row0, Mq) needs the frame counts of the batch (frames)")
        if Mq is not None and int(Mq) % 64:
            raise ValueError(cls.BAD_MQ % Mq)
        return super().__new__(cls, frames, row0, None if Mq is None else int(Mq))

    @classmethod
    def of(cls, frames, packed):
        """From the arguments of Encoder.forward / forward_f32: frames, packed=(row0, Mq)."""
        return cls(frames, *(packed if packed is not None else ()))

    fixed = property(lambda self: self.frames is None)
    padded = property(lambda self: self.frames is not None and self.Mq is None)
    packed = property(lambda self: self.Mq is not None)

    @property
    def args(self):
        """The layout as Encoder.forward / forward_f32 take it."""
        return dict(frames=self.frames, packed=(self.row0, self.Mq) if self.packed else None)

    def check(self, B, T):
        """The packed row count against the shape of the batch: B <= Mq <= roundup(B * T, 64)."""
        cap = (B * T + 63) // 64 * 64
        if self.packed and not B <= self.Mq <= cap:
            raise ValueError((self.BAD_MQ + " in %d..%d") % (self.Mq, B, cap))

    def rows(self, M):
        """The rows the transformer layers run over, of the M = B * T of the padded rectangle."""
        return self.Mq if self.packed else M

    def key(self, B, L):
        """Of the buffer set / state of a [B, L] batch: the packed layout has a set of its own."""
        return (B, L, "packed") if self.packed else (B, L)

    def plan_key(self, *base):
        """Of a recorded launch plan: one plan per packed row count."""
        return base + (self.Mq,) if self.packed else base


FIXED = RowLayout()


def row_layout(cfg, lengths, B, L, *, min_samples, refuse_short, score_f32, device):
    """Sample counts of a zero-padded [B, L] batch -> (frame counts, a list of ints validated on the host; the RowLayout with the counts
    uploaded to `device`).  A row below min_samples: counted as min_samples (refuse_short=False: its zero padding is part of the signal, as
    for a file padded on disk) or an error (refuse_short=True: a back-end that would have to take the padding as signal throughout).
    Packed when the switch of the precision is on, read at call time: SCORE_PACK for fp32 scoring (score_f32), else VARLEN_PACK."""
    lengths = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    need = "lengths: need one sample count in 1..%d per row of the [%d, %d] batch" % (L, B, L)
    bad = len(lengths) != B or any(n < 1 or n > L for n in lengths)
    if refuse_short:
        if bad:
            raise ValueError("%s, got %r" % (need, lengths))
        if any(n < min_samples for n in lengths):
            raise ValueError("lengths: this back-end needs at least %d samples (%d frames) per row, got %r; zero-pad shorter utterances "
                             "to %d samples" % (min_samples, cfg.conv_lens(min_samples)[-1], lengths, min_samples))
    elif bad or L < min_samples:
        raise ValueError("%s (at least %d samples per row), got %r" % (need, min_samples, lengths))
    T = cfg.conv_lens(L)[-1]
    counts = ops.check_lengths([cfg.conv_lens(max(n, min_samples))[-1] for n in lengths], T)
    device = torch.device(device)

    def upload(values):
        host = torch.tensor(values, dtype=torch.int32)
        return (host.pin_memory() if device.type == "cuda" else host).to(device, non_blocking=True)
    frames, row0, Mq = upload(counts), None, None
    if SCORE_PACK if score_f32 else VARLEN_PACK:
        row0, Mq = ops.packed_rows(counts, T, PACK_ROWS)
        row0 = upload(row0)
    return counts, RowLayout(frames, row0, Mq)


class W2VConfig:
    def __init__(self, conv_dim=512, conv_kernels=(10, 3, 3, 3, 3, 2, 2), conv_strides=(5, 2, 2, 2, 2, 2, 2), embed=1024,
                 layers=24, heads=16, ffn=4096, pos_k=128, pos_groups=16, final_dim=768, latent_vars=320, latent_groups=2,
                 encoder_layerdrop=0.0, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, dropout_input=0.0, layer_mix=False):
        # element-dropout probabilities of fairseq's Wav2Vec2Config (read from the checkpoint's cfg by scl_amd.checkpoint; the
        # reference runs the encoder in train mode, model/xlsr.py:33-41): `dropout` after the positional conv and on the outputs of
        # out_proj / fc2, `attention_dropout` on the attention probabilities, `activation_dropout` after the FFN's GELU, `dropout_input`
        # on the projected features
        self.dropout, self.attention_dropout, self.activation_dropout, self.dropout_input = dropout, attention_dropout, activation_dropout, dropout_input
        self.conv_dim, self.conv_kernels, self.conv_strides = conv_dim, tuple(conv_kernels), tuple(conv_strides)
        self.embed, self.layers, self.heads, self.ffn = embed, layers, heads, ffn
        self.pos_k, self.pos_groups = pos_k, pos_groups
        self.final_dim, self.latent_vars, self.latent_groups = final_dim, latent_vars, latent_groups
        self.encoder_layerdrop = encoder_layerdrop
        # YAML `ssl_layer_mix`: the encoder hands on the learned soft-max-weighted sum over all layers + 1 hidden states (csrc/layer_mix.hip)
        # instead of the last layer's alone; one more parameter, `layer_mix.weight` [layers + 1], beside the LL projection (mix_specs)
        self.layer_mix = bool(layer_mix)
        if self.layer_mix and layers + 1 > ops.LAYER_MIX_MAX_STATES:
            raise SclError("ssl_layer_mix: %d layers give %d hidden states; the mix kernels take at most %d"
                           % (layers, layers + 1, ops.LAYER_MIX_MAX_STATES))
        assert embed % heads == 0 and (embed // heads) % 8 == 0 and conv_dim % 8 == 0 and pos_k % 2 == 0
        assert (embed // pos_groups) % 8 == 0

    @staticmethod
    def tiny():
        return W2VConfig(conv_dim=32, embed=64, layers=2, heads=4, ffn=128, pos_k=16, pos_groups=4, final_dim=16,
                         latent_vars=8, latent_groups=2)

    @staticmethod
    def xlsr_1b(**kw):
        """XLS-R 1B as fairseq publishes its config (80-wide heads); the conv stack and the positional convolution of the 300M model."""
        return W2VConfig(embed=1280, layers=48, heads=16, ffn=5120, final_dim=1024, **kw)

    @staticmethod
    def xlsr_2b(**kw):
        """XLS-R 2B as fairseq publishes its config (120-wide heads); the conv stack and the positional convolution of the 300M model."""
        return W2VConfig(embed=1920, layers=48, heads=16, ffn=7680, final_dim=1024, **kw)

    def with_layer_mix(self, on=True):
        """A copy of this config with the layer mix switched (the cap on the number of hidden states is checked as at construction)."""
        fields = {k: getattr(self, k) for k in ("conv_dim", "conv_kernels", "conv_strides", "embed", "layers", "heads", "ffn", "pos_k", "pos_groups",
                                                "final_dim", "latent_vars", "latent_groups", "encoder_layerdrop", "dropout", "attention_dropout",
                                                "activation_dropout", "dropout_input")}
        return W2VConfig(layer_mix=on, **fields)

    def conv_lens(self, L):
        out = []
        for k, s in zip(self.conv_kernels, self.conv_strides):
            L = (L - k) // s + 1
            out.append(L)
        return out

    def samples_for(self, frames):
        """The shortest clip that yields `frames` frames (400 + 320 (frames - 1) samples for the XLS-R stack)."""
        L = int(frames)
        for k, s in zip(reversed(self.conv_kernels), reversed(self.conv_strides)):
            L = (L - 1) * s + k
        return L

    def min_samples(self):
        """The shortest clip that yields one frame (400 samples for the XLS-R stack)."""
        return self.samples_for(1)


W2V_ARCHS = {"xlsr_300m": W2VConfig, "xlsr_1b": W2VConfig.xlsr_1b, "xlsr_2b": W2VConfig.xlsr_2b, "tiny": lambda **kw: W2VConfig.tiny()}


def w2v_config_from(args):
    """The encoder a YAML names (needs no GPU).  `w2v_arch`: one of W2V_ARCHS ("xlsr_300m" when absent: the reference's only encoder;
    "tiny" for tests and plumbing), or a mapping of W2VConfig fields such as {embed: 1280, layers: 48, heads: 16, ffn: 5120, final_dim: 1024}
    (fields left out keep the 300M model's values).  `encoder_layerdrop` of the YAML applies to every arch but "tiny".
    `ssl_layer_mix: true` (or `layer_mix` inside a mapping): W2VConfig.layer_mix, every arch."""
    arch = args.get("w2v_arch", "xlsr_300m")
    layerdrop = float(args.get("encoder_layerdrop", 0.0))
    mix = bool(args.get("ssl_layer_mix", False))
    if isinstance(arch, collections.abc.Mapping):
        fields = dict(arch)
        fields.setdefault("encoder_layerdrop", layerdrop)
        fields.setdefault("layer_mix", mix)
        try:
            return W2VConfig(**fields)
        except TypeError as e:
            raise ValueError("w2v_arch: %s; the fields are those of W2VConfig" % e) from None
    if arch not in W2V_ARCHS:
        raise ValueError("w2v_arch: unknown encoder %r; the names are %s, or give a mapping of W2VConfig fields"
                         % (arch, ", ".join(sorted(W2V_ARCHS))))
    cfg = W2V_ARCHS[arch](encoder_layerdrop=layerdrop)
    if mix:      # after construction: "tiny" takes no fields, and the switch-off path stays the call it was
        cfg = cfg.with_layer_mix()
    return cfg


def param_specs(cfg, prefix="ssl_model.model."):
    """(name, shape, trainable) in MEMORY order (q,k,v adjacent); names are fairseq's."""
    C, E = cfg.conv_dim, cfg.embed
    sp = []
    cin = 1
    for i, k in enumerate(cfg.conv_kernels):
        p = prefix + "feature_extractor.conv_layers.%d." % i
        sp += [(p + "0.weight", (C, cin, k), True), (p + "0.bias", (C,), True),
               (p + "2.1.weight", (C,), True), (p + "2.1.bias", (C,), True)]
        cin = C
    sp += [(prefix + "layer_norm.weight", (C,), True), (prefix + "layer_norm.bias", (C,), True),
           (prefix + "post_extract_proj.weight", (E, C), True), (prefix + "post_extract_proj.bias", (E,), True),
           (prefix + "encoder.pos_conv.0.bias", (E,), True), (prefix + "encoder.pos_conv.0.weight_g", (1, 1, cfg.pos_k), True),
           (prefix + "encoder.pos_conv.0.weight_v", (E, E // cfg.pos_groups, cfg.pos_k), True)]
    for n in range(cfg.layers):
        p = prefix + "encoder.layers.%d." % n
        sp += [(p + "self_attn_layer_norm.weight", (E,), True), (p + "self_attn_layer_norm.bias", (E,), True)]
        for proj in ("q_proj", "k_proj", "v_proj"):
            sp.append((p + "self_attn.%s.weight" % proj, (E, E), True))
        for proj in ("q_proj", "k_proj", "v_proj"):
            sp.append((p + "self_attn.%s.bias" % proj, (E,), True))
        sp += [(p + "self_attn.out_proj.weight", (E, E), True), (p + "self_attn.out_proj.bias", (E,), True),
               (p + "final_layer_norm.weight", (E,), True), (p + "final_layer_norm.bias", (E,), True),
               (p + "fc1.weight", (cfg.ffn, E), True), (p + "fc1.bias", (cfg.ffn,), True),
               (p + "fc2.weight", (E, cfg.ffn), True), (p + "fc2.bias", (E,), True)]
    sp += [(prefix + "encoder.layer_norm.weight", (E,), True), (prefix + "encoder.layer_norm.bias", (E,), True)]
    vd = cfg.final_dim // cfg.latent_groups
    nv = cfg.latent_vars * cfg.latent_groups
    sp += [(prefix + "mask_emb", (E,), False), (prefix + "quantizer.vars", (1, nv, vd), False),
           (prefix + "quantizer.weight_proj.weight", (nv, C), False), (prefix + "quantizer.weight_proj.bias", (nv,), False),
           (prefix + "project_q.weight", (cfg.final_dim, cfg.final_dim), False), (prefix + "project_q.bias", (cfg.final_dim,), False),
           (prefix + "final_proj.weight", (cfg.final_dim, E), False), (prefix + "final_proj.bias", (cfg.final_dim,), False)]
    return sp


MIX_WEIGHT = "layer_mix.weight"


def mix_specs(cfg):
    """The layer mix's one parameter (cfg.layer_mix; nothing without it): the f32 logits of the soft-max over the layers + 1 hidden states,
    zeros at initialisation (a uniform average).  A model puts it directly behind LL.bias, at the module root of its state dict: inside
    trainable_range() with and without a frozen encoder, and no offset in front of it moves."""
    return [(MIX_WEIGHT, (cfg.layers + 1,), True)] if cfg.layer_mix else []


def plan_group_launches(pend, final, carry=True, round_tiles=256, max_members=8):
    """Pending tile work -> launches.  pend: list of [problem, tiles, next tile, age in layers] (oldest first; consumed in place).
    Returns a list of launches, each a list of (problem, first tile, count).  Rules: while at least `round_tiles` tiles are pending, launch
    exactly that many (a whole round of the CUs), oldest first, splitting a problem where the cut falls; then, if anything older than the
    current layer is left (its operands are about to be re-used), or `final`, or carrying is off, launch the rest; otherwise keep it for
    the next call.  Every tile of every problem is launched exactly once."""
    launches = []
    while pend:
        total = sum(it[1] - it[2] for it in pend)
        if total >= round_tiles and carry:
            take = round_tiles
        elif final or not carry or any(it[3] >= 1 for it in pend):
            take = total
        else:
            break
        parts = []
        while take > 0 and pend and len(parts) < max_members:
            it = pend[0]
            c = min(take, it[1] - it[2])
            parts.append((it[0], it[2], c))
            it[2] += c
            take -= c
            if it[2] == it[1]:
                pend.pop(0)
        launches.append(parts)
    return launches


def _splitk(tiles, ksteps, target=512, cap=32):
    s = max(1, min(cap, target // max(tiles, 1), ksteps))
    return s


class Encoder:
    """Forward / backward of the SSL encoder on one GPU.  `P` is a FlatParams holding (at least)
    the parameters named by param_specs(cfg, prefix)."""

    def __init__(self, cfg, P, prefix="ssl_model.model."):
        self.cfg, self.P, self.pre = cfg, P, prefix
        self.dev = P.device
        self._bufs = {}
        # variable-length scoring batches (forward / forward_f32 with `frames`): every padded shape is a buffer set of its own, so these
        # live in two small LRUs (bf16 path, fp32 path) instead of the keep-forever table of the fixed shapes.  Variable-length TRAINING
        # batches share one padded shape (the data path pads every pack to trim_length): their sets are kept like the fixed shapes'
        self._vbufs, self._vbufs_f32 = VarlenSets(), VarlenSets()
        self._vbufs_train = {}
        C, E, K, G = cfg.conv_dim, cfg.embed, cfg.pos_k, cfg.pos_groups
        Cg = E // G
        bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=self.dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        # derived bf16 weights that are not plain casts
        self.wk = [None] + [bf(C, cfg.conv_kernels[i] * C) for i in range(1, len(cfg.conv_kernels))]
        # backward-data operands of the phase-split transposed convolution ([k tap blocks][C][C], see scl_conv_weight_pack)
        self.wd = [None] + [bf(cfg.conv_kernels[i] * C, C) for i in range(1, len(cfg.conv_kernels))]
        self.pos_wf, self.pos_wd, self.pos_norm = bf(G, Cg, K * Cg), bf(G, Cg, K * Cg), f32(K)
        self.ws_small = f32(K + E * K)      # weight-norm backward: per-tap sums + per-output-channel partials
        self.on_grads_ready = None   # callback(lo_offset): every gradient at flat offset >= lo_offset is final (DP overlap)
        # Backward, optional (SCL_WGRAD_STREAM=1): the weight-gradient GEMMs and bias column sums are leaves of the graph — nothing in
        # the layer's data-gradient chain reads them — so they can run on a second stream beside the chain's bandwidth-bound kernels
        # (LayerNorm / attention backward).  Measured: 54.35 -> 53.6 ms/step at batch 64, 32.75 -> 32.25 at batch 32, same loss to the
        # last bit.  The gain is small because a wide GEMM block owns all 160 KiB of its CU's LDS, so the chain's kernels (48-116 KiB
        # of LDS each) cannot co-reside with it and only interleave at block granularity; and with two GEMMs in flight the
        # event-bracketed per-launch durations that bench.py's roofline is built from overlap (their sum over-counts).  Off by default.
        self.wstream = torch.cuda.Stream(device=self.dev) if (os.environ.get("SCL_WGRAD_STREAM", "0") == "1" and self.dev.type == "cuda") else None

    # ---- weights ---------------------------------------------------------------------------------
    def n(self, name):
        return self.pre + name

    def refresh_weights(self):
        """Rebuild the bf16 working set after the fp32 masters changed (the flat cast is fused into
        the AdamW kernel; this covers load_state_dict / first use and the re-laid-out weights)."""
        P, cfg = self.P, self.cfg
        if P.bf16_version != P.version:
            ops.cast_bf16(P.flat, P.bf16, P.n_train)
            P.bf16_version = P.version
        if getattr(self, "_derived_version", -1) == P.version:
            return
        C, E, K, G = cfg.conv_dim, cfg.embed, cfg.pos_k, cfg.pos_groups
        for i in range(1, len(cfg.conv_kernels)):
            ops.conv_weight_pack(P.f32(self.n("feature_extractor.conv_layers.%d.0.weight" % i)), self.wk[i], C, C, cfg.conv_kernels[i],
                                 wd=self.wd[i], stride=cfg.conv_strides[i])
        ops.posconv_weight_pack(P.f32(self.n("encoder.pos_conv.0.weight_v")), P.f32(self.n("encoder.pos_conv.0.weight_g")),
                                self.pos_norm, self.pos_wf, self.pos_wd, E, E // G, K)
        self._derived_version = P.version

    def W(self, name, ld):
        """bf16 GEMM operand view of a plain (cast-only) weight."""
        return Op(self.P.bf16, ld, offset=self.P.off(self.n(name)))

    def b(self, name):
        return self.P.f32(self.n(name))

    # ---- buffers ---------------------------------------------------------------------------------
    def _set(self, key, make, layout, train=False, f32=False):
        """The buffer set under `key` in the store of its kind (shape_entry); the LRU of a scoring batch is the one of its precision."""
        return shape_entry(key, make, layout, train, self._bufs, self._vbufs_f32 if f32 else self._vbufs, self._vbufs_train)

    def bufs(self, B, L, layout=FIXED, train=False):
        """The buffer set of a [B, L] batch on the bf16 path.  A variable-length batch's runs the streaming attention whatever T is (lse,
        attn_ws, no T x T buffers); the packed layout's is a set of its own (layout.key) — one per padded shape, sized for roundup(B * T, 64)
        rows whatever the step's lengths are."""
        return self._set(layout.key(B, L), lambda: self._make_bufs(B, L, layout), layout, train)

    def _make_bufs(self, B, L, layout):
        varlen, packed = not layout.fixed, layout.packed
        cfg, dev = self.cfg, self.dev
        C, E, H, Fd, K = cfg.conv_dim, cfg.embed, cfg.heads, cfg.ffn, cfg.pos_k
        Ts = cfg.conv_lens(L)
        T = Ts[-1]
        M = B * T
        Tp = (T + 7) // 8 * 8
        bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        # The operands of a layer's weight gradients (reduction over the M rows) carry zero rows up to the next multiple of 64: no kernel
        # ever writes past row M (tile rows beyond it are masked), so the rows stay zero and the gradient GEMMs may walk Mp rows — which
        # puts them on the wide tiles / the grouped launch (K % 64 == 0) at batch sizes like 32 x 199 = 6368 rows too.
        Mp = (M + 63) // 64 * 64
        d = {"Ts": Ts, "T": T, "M": M, "Tp": Tp, "Mp": Mp}
        # packed layout: the transformer layers run over up to Mp rows (every frame valid: roundup(B * T, 64)), so their buffers hold Mp rows
        Mr = Mp if packed else M
        bfz = lambda rows, width, extra=0: torch.zeros(rows * width + extra, dtype=torch.bfloat16, device=dev)
        slack = 128 * max(C, E)  # tail slack: tile rows past the last frame are clamped/masked, never dereferenced past this
        d["z"] = [bf(B * t * C + slack) for t in Ts]
        d["y"] = [None] + [f32(B * t * C) for t in Ts[1:]]   # pre-LayerNorm conv outputs stay fp32 (fairseq's Fp32LayerNorm input)
        d["cmean"] = [None] + [f32(B * t) for t in Ts[1:]]
        d["crstd"] = [None] + [f32(B * t) for t in Ts[1:]]
        d["h0"], d["fmean"], d["frstd"] = bf(M * C), f32(M), f32(M)
        d["x0"] = f32(M * E)
        d["xpad"] = bf(B * (T + K) * E + slack)
        d["pc_pre"] = bf(M * E)
        d["xin"] = [f32(Mr * E) for _ in range(cfg.layers + 1)]
        d["h1"] = [bfz(Mp, E) for _ in range(cfg.layers)]
        d["m1"], d["r1"] = [f32(Mr) for _ in range(cfg.layers)], [f32(Mr) for _ in range(cfg.layers)]
        d["qkv"] = [bf(Mr * 3 * E + slack) for _ in range(cfg.layers)]
        d["fused_attn"] = (E // H == 64) and T <= 224      # scores stay on chip (csrc/attention.hip); else materialised path
        # streaming attention (csrc/attention_long.hip, csrc/attention_wide.hip): above 512 frames, or from 225 frames with SCL_ATTN_LONG=1
        d["long_attn"] = stream_attn_takes(E // H) and not d["fused_attn"] and (T > MAT_ATTN_MAX_T or ATTN_LONG)
        if varlen:
            if not stream_attn_takes(E // H):
                raise SclError("encoder: variable-length batches on the bf16 path run the streaming attention, which takes %s "
                               "(got %d); the fp32 scoring path takes any head dim" % (STREAM_ATTN_HEAD_DIMS, E // H))
            d["fused_attn"], d["long_attn"] = False, True
        if T > MAT_ATTN_MAX_T and not d["long_attn"]:
            raise SclError("encoder: %d frames need the streaming attention, which takes %s (got %d); other head dims are limited "
                           "to %d frames (%d samples)" % (T, STREAM_ATTN_HEAD_DIMS, E // H, MAT_ATTN_MAX_T, L))
        if d["fused_attn"] or d["long_attn"]:
            d["lse"] = [f32(B * H * T) for _ in range(cfg.layers)]
        if d["long_attn"]:
            d["attn_ws"] = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
        elif not d["fused_attn"]:
            d["S"] = f32(B * H * T * Tp)   # row stride Tp keeps the 4-wide epilogue stores aligned
            d["P"] = [bf(B * H * T * Tp + 1024) for _ in range(cfg.layers)]
        d["ctx"] = [bfz(Mp, E) for _ in range(cfg.layers)]
        d["x1"] = [f32(Mr * E) for _ in range(cfg.layers)]
        d["m2"], d["r2"] = [f32(Mr) for _ in range(cfg.layers)], [f32(Mr) for _ in range(cfg.layers)]
        d["h2"] = [bfz(Mp, E) for _ in range(cfg.layers)]
        d["f"] = [bf(Mr * Fd) for _ in range(cfg.layers)]
        d["a"] = [bfz(Mp, Fd) for _ in range(cfg.layers)]
        d["out"], d["omean"], d["orstd"] = bf(Mr * E), f32(Mr), f32(Mr)
        if cfg.layer_mix:
            # the final LayerNorm's output as the f32 hidden state h_L (the one new activation; xin[0 .. L-1] are the others and `out` holds
            # the mix); for the backward s_L d(mix), which that LayerNorm's backward takes, and the fp64 block partials of d(logits)
            d["hL"], d["mix_gL"] = f32(Mr * E), f32(Mr * E)
            d["mix_ws"] = torch.empty(ops.layer_mix_bwd_w_ws_bytes(Mr * E, cfg.layers + 1), dtype=torch.uint8, device=dev)
            d["mix_a"] = torch.zeros(ops.LAYER_MIX_MAX_STATES, dtype=torch.float32, device=dev)      # the backward's own copy of the logits
        if packed:      # the padded ends of the packed stretch: xin[0] before the pack, the output behind the unpack, d(xin[0]) behind its unpack
            d["xin_pad"], d["out_pad"], d["dxin_pad"] = f32(M * E), bf(M * E), f32(M * E)
        # backward scratch (shared by all layers)
        # residual-gradient pairs (f32, bf16) rotate over FIVE buffers and d_f / dqkv alternate between TWO: the weight gradients of a layer may
        # be carried over into the grouped launch at the end of the NEXT layer (see _flush_slabs), so their operands outlive their layer by one
        d["dx_rot"] = [(f32(Mr * E), bfz(Mp, E, slack)) for _ in range(5)]
        if packed:      # d(x0) behind the positional convolution is padded again: a pair of its own, the rotating ones stay packed
            d["dx0_pad"] = (f32(M * E), bfz(Mp, E, slack))
        d["d_f"] = [bfz(Mp, Fd, slack), bfz(Mp, Fd, slack)]
        d["d_h"] = bf(Mr * E + slack)
        d["d_ctx"] = bf(Mr * E + slack)
        d["dqkv"] = [bfz(Mp, 3 * E, slack), bfz(Mp, 3 * E, slack)]
        d["dS"] = None if (d["fused_attn"] or d["long_attn"]) else bf(B * H * T * Tp + 1024)
        d["dcpad"] = bf(B * (T + K) * E + slack)
        d["dz"] = [bf(B * t * C + slack) for t in Ts]
        # conv-stack backward: LayerNorm-backward output of layer i with per-utterance zero rows (Q in front, Qe behind) so that
        # the transposed convolution reads [dy[u-1], dy[u]] as one overlapping GEMM row; zeroed once, only frame rows are rewritten
        d["dyp"], d["dyp_geom"] = [None], [None]
        for i in range(1, len(Ts)):
            k, s, Tin, Tout = cfg.conv_kernels[i], cfg.conv_strides[i], Ts[i - 1], Ts[i]
            Q = (k - 1) // s
            Qe = max(0, max((Tin - 1 - p) // s for p in range(s)) - (Tout - 1))
            Rp = Q + Tout + Qe
            d["dyp"].append(torch.zeros(B * Rp * C + slack, dtype=torch.bfloat16, device=dev))
            d["dyp_geom"].append((Q, Rp))
        nln = max(ops.layernorm_bwd_nparts(B * t) for t in Ts)
        d["ln_part"] = f32(nln * 3 * max(C, E))
        d["ln_part2"] = f32(nln * 3 * E)      # the layer's second LayerNorm backward: both reductions wait for the layer's one closing launch
        ncs = max(ops.colsum_nparts(B * (max(Ts[1:] + [T + K]) + 4)), 1) + 1      # conv bias sums run over the zero-padded dyp rows
        d["cs_part"] = f32(ncs * max(3 * E, Fd, C))
        d["qkv_bias_part"] = f32(B * 3 * E)
        d["cs_fused"] = f32(4 * (Mr // 200 + 2) * Fd)      # per-tile column sums written by the fc2 data-gradient GEMM (main stream only)
        d["conv0_ws"] = f32(ops.conv0_bwd_nparts(B, L, cfg.conv_kernels[0], cfg.conv_strides[0]) * C * (cfg.conv_kernels[0] + 3))
        d["conv0_stats"] = f32(B * Ts[0] * 2)   # per-frame (mean, rstd) of layer 0's LayerNorm
        # the weight-gradient queue (_wgrad fills it, _flush_slabs drains it at the end of a layer's backward):
        d["wgrad_group"] = []       # this layer's gradients waiting for the grouped launch: (A, B, out, Mo, No, Kr, slot)
        d["wgrad_pending"] = []     # tile work carried between layers: [problem, tiles, next tile, age in layers]
        d["slab_slots"] = {}        # split-K slab buffer per slot (0..3; None = the shared one of unslotted gradients), sized on first use
        d["slab_jobs"] = []         # slab combines of the slotted gradients waiting for the layer's one combine launch
        d["slabs_keep"] = []        # outgrown slab buffers: recorded launch plans may still point into them
        kmax = max(cfg.conv_kernels[1:]) if len(cfg.conv_kernels) > 1 else 1
        d["dwk"] = f32(C * kmax * C)
        d["dwf"] = f32(E * (E // cfg.pos_groups) * K)
        return d

    # ---- element dropout: seeds --------------------------------------------------------------------
    # Every site draws its keep-mask from hash(site seed, element index) in the kernel that applies it (GEMM epilogue, attention,
    # LayerNorm backward, scl_dropout_f32); the backward recomputes the mask from the same seed.  A site seed mixes the step's seed
    # with (layer, site).  Launch plans replay recorded argument lists, so every call that carries a seed leaves a "slot" behind
    # (the descriptor or the argument list + position) and apply_seeds() re-seeds the slots before a replay.
    SITE_IN, SITE_ENC, SITE_ATTN, SITE_1, SITE_2, SITE_3 = 1, 2, 3, 4, 5, 6

    @staticmethod
    def site_seed(step_seed, layer, site):
        x = (int(step_seed) * 0x9E3779B1 + (layer + 1) * 0x85EBCA77 + site * 0xC2B2AE3D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
        x ^= x >> 12
        return x & 0x7FFFFFFF

    def drop_probs(self, training):
        c = self.cfg
        if not training:
            return 0.0, 0.0, 0.0, 0.0
        return float(c.dropout), float(c.attention_dropout), float(c.activation_dropout), float(c.dropout_input)

    @staticmethod
    def _slot(slots, handle, pos, layer, site):
        """handle: a GEMM descriptor (pos None) or a recorded call entry (argument position pos); None when nothing was recorded."""
        if handle is not None:
            slots.append((handle, pos, layer, site))

    def apply_seeds(self, slots, step_seed):
        for handle, pos, layer, site in slots:
            sd = self.site_seed(step_seed, layer, site)
            if pos is None:
                handle.drop_seed = sd
            else:
                handle[1][pos] = sd

    # ---- helpers ---------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _side(self):
        """Leaf work of the backward (weight / bias gradients): ordered behind the main stream's work so far, issued on the second
        stream.  With SCL_WGRAD_STREAM=0 it simply runs in place."""
        if self.wstream is None:
            yield
            return
        ops.stream_wait(self.wstream, torch.cuda.current_stream())
        with torch.cuda.stream(self.wstream):
            yield

    def _join_side(self):
        """The main stream goes on only when the second stream has drained: its inputs may be overwritten, its gradients read."""
        if self.wstream is not None:
            ops.stream_wait(torch.cuda.current_stream(), self.wstream)

    def _mix_states(self, d):
        """The hidden states of the layer mix in a bf16-path buffer set, in index order: the residual stream entering each layer
        (xin[0]: behind the positional convolution and its dropout; a skipped layer copies its input on) and the final LayerNorm's output."""
        return d["xin"][: self.cfg.layers] + [d["hL"]]

    def _mix_bwd_w(self, d, g, Mt):
        """d(logits) into the flat gradient buffer (overwritten) and s_L g into d["mix_gL"], from g = d(mix) over Mt rows.  Returns the
        logits the whole backward reads: a copy taken here, because an optimizer that steps underneath the backward (optim._StepOverlap)
        updates the tail of the flat buffer, the logits with it, as soon as this gradient is announced."""
        S, o = self.cfg.layers + 1, self.P.off(MIX_WEIGHT)
        n4 = (S + 3) // 4 * 4      # inside the parameter's slot: FlatParams aligns every tensor to 8 elements
        ops.axpby(self.P.flat[o:o + n4], None, 1.0, 0.0, d["mix_a"], n4)
        logits = d["mix_a"][:S]
        ops.layer_mix_bwd_w(g, self._mix_states(d), logits, d["mix_gL"], d["mix_ws"], self.P.g(MIX_WEIGHT), Mt * self.cfg.embed)
        return logits

    def _slab(self, d, slot, numel):
        """The split-K slab buffer of `slot` with room for `numel` floats.  A buffer only grows; the outgrown one is kept alive because
        recorded launch plans may still point into it."""
        bufs = d["slab_slots"]
        if slot not in bufs or bufs[slot].numel() < numel:
            if slot in bufs:
                d["slabs_keep"].append(bufs[slot])
            bufs[slot] = torch.empty(numel, dtype=torch.float32, device=self.dev)
        return bufs[slot]

    def _wgrad(self, d, A, B_, out, Mo, No, Kr, slot=None, queue=True, **kw):
        """out[Mo, No] (f32, contiguous) = A^T B over the Kr reduction rows; split-K when the output is small.
        slot (0..3: the four weight gradients of a transformer layer): the gradient is queued for the layer's grouped launch, or (queue=False,
        short reductions, SCL_WGRAD_GROUP=0) its slabs stay in the slot's own buffer and the combine is queued; _flush_slabs launches both."""
        ksteps = (Kr + 63) // 64
        if queue and WGRAD_GROUP and slot is not None and not kw and Kr % 64 == 0 and ksteps >= WGRAD_GROUP_MIN_KSTEPS:
            d["wgrad_group"].append((A, B_, out, Mo, No, Kr, slot))      # launched by _flush_slabs at the end of the layer
            return
        tiles = ((Mo + 127) // 128) * ((No + 127) // 128) * kw.get("nb2", 1)
        sk = _splitk(tiles, ksteps)
        # wide tiles (gemm_w8.hip: 256 x 256 output tiles, one 8-wave block per CU): size the split for one round of the 256 CUs
        t256 = ((Mo + 255) // 256) * ((No + 255) // 256) * kw.get("nb2", 1)
        if t256 >= 12:
            # slabs: one round of the 256 CUs; at most 8 (>= 32 tiles) / 16 (12-31 tiles; out-proj: 16 tiles, where the 128 x 128 sizing left
            # 160 blocks of 25 K steps.  Measured in one call, three pairs, ms per step: 47.78 / 47.59 / 47.66 on the 128 x 128 sizing, 47.76 /
            # 47.29 / 47.26 with 16 slabs; launch + slab reduction 61.4 -> 53.8 us) / 21 (12 tiles and >= 700 K steps: the conv layers, utterance-
            # batched K rows; tools/_wg probe, us incl. the slab reduction, 16 -> 21 slabs: 766 -> 677, 400 -> 358, 207 -> 184, 116 -> 102)
            skw = max(1, min(8 if t256 >= 32 else (21 if ksteps >= 700 else 16), (256 + t256 // 2) // t256, ksteps // 8))
            if ops.gemm_wide_kind(A, B_, out, Mo, No, Kr, a_t=True, b_t=True, splitk=skw, c_split_stride=out.numel() if skw > 1 else 0, **kw):
                sk = skw
        if sk == 1:
            ops.gemm(A, B_, out, Mo, No, Kr, a_t=True, b_t=True, **kw)
            return
        n = out.numel()
        slab = self._slab(d, slot, sk * n)
        ops.gemm(A, B_, slab, Mo, No, Kr, a_t=True, b_t=True, splitk=sk, c_split_stride=n, **kw)
        if slot is not None:      # one combine launch per layer instead of one behind every gradient: 72 kernel boundaries per step less
            d["slab_jobs"].append((slab, out, n, sk, n))
        else:
            ops.reduce_slabs(slab, out, n, sk, n)

    def _flush_slabs(self, d, final=True):
        """End of a layer's backward: its queued weight gradients join the pending tile work and whole rounds of 256 tiles are launched
        (ops.gemm_group_part: a launch takes tile RANGES of up to 8 problems, oldest first).  A layer's 192 tiles do not fill the 256 CUs and a
        grouped launch takes about as long with 192 tiles as with 256 (336 vs 348 us, tools/group_fill_probe.py), so the remainder is carried
        into the NEXT layer's launch: 3 launches per 4 layers.  Everything of the previous layer is flushed here (its operands are re-used
        by the layer after this one); `final` flushes all.  SCL_WGRAD_CARRY=0: one launch of a layer's own tiles per layer.  If the list
        does not qualify the gradients run one by one on the split-K path.  Then the queued split-K combines, one launch."""
        group, d["wgrad_group"] = d["wgrad_group"], []
        pend = d["wgrad_pending"]
        for it in pend:
            it[3] += 1
        if group:
            counts = [ops.gemm_group_tiles(*g[:6]) for g in group]
            if min(counts) > 0 and sum(counts) >= 96:
                pend.extend([g[:6], c, 0, 0] for g, c in zip(group, counts))
            else:
                with self._side():
                    for A, B_, out, Mo, No, Kr, slot in group:
                        self._wgrad(d, A, B_, out, Mo, No, Kr, slot=slot, queue=False)
        for parts in plan_group_launches(pend, final, WGRAD_CARRY):
            with self._side():
                ops.gemm_group_part(parts)
        if d["slab_jobs"]:
            with self._side():
                ops.reduce_slabs_multi(d["slab_jobs"])
            d["slab_jobs"] = []

    def _bias_grad(self, d, dy, Mrows, N, gname):
        ops.colsum_reduce(dy, d["cs_part"], self.P.g(self.n(gname)), Mrows, N)

    def _ln_job(self, part, nparts, C, wname, bname, resid_bias=None):
        """weight and bias of a LayerNorm are adjacent in the flat buffer: one reduction over the (dgamma | dbeta) partials, as a job
        tuple for ops.colreduce_multi; with resid_bias also the third partial row, colsum(dres) = the bias gradient of the linear that
        feeds the residual."""
        ow, ob = self.P.off(self.n(wname)), self.P.off(self.n(bname))
        assert ob == ow + C
        if resid_bias is None:
            return (part, self.P.grad[ow:ow + 2 * C], nparts, 2 * C)
        return (part, self.P.grad[ow:ow + 2 * C], nparts, 3 * C, self.P.g(self.n(resid_bias)), 2 * C)

    def _ln_grads(self, d, nparts, C, wname, bname, resid_bias=None):
        """The reduction of _ln_job over d["ln_part"] in a launch of its own (ops.colreduce_seg)."""
        part, out, nparts, width, out2, split = (self._ln_job(d["ln_part"], nparts, C, wname, bname, resid_bias) + (None, 0))[:6]
        ops.colreduce_seg(part, out, nparts, width, out2=out2, split=split)

    # ---- attention: the path of a layer, by row layout and buffer set ---------------------------------
    def _attn_fwd(self, d, n, layout, B, training, p_attn, seed, slots):
        """qkv[n] -> ctx[n] (and lse[n], or P[n]).  With attention dropout the launch that carries `seed` leaves its slot in `slots`."""
        E, H = self.cfg.embed, self.cfg.heads
        D, T, Tp = E // H, d["T"], d["Tp"]
        qkv, ctx, sc = d["qkv"][n], d["ctx"][n], (E // H) ** -0.5
        e = pos = None
        if layout.packed and p_attn > 0:
            e = ops.attn_fwd_packed_drop(qkv, ctx, d["lse"][n], layout.row0, B, T, H, D, layout.Mq, sc, drop_p=p_attn, drop_seed=seed)
            pos = ops.ATTN_FWD_PACKED_SEED
        elif layout.packed:
            ops.attn_fwd_packed(qkv, ctx, d["lse"][n], layout.row0, B, T, H, D, layout.Mq, sc)
        elif layout.padded and p_attn > 0:
            e = ops.attn_fwd_varlen_drop(qkv, ctx, d["lse"][n], layout.frames, B, T, H, D, sc, drop_p=p_attn, drop_seed=seed)
            pos = ops.ATTN_FWD_VARLEN_SEED
        elif layout.padded:
            ops.attn_fwd_varlen(qkv, ctx, d["lse"][n], layout.frames, B, T, H, D, sc)
        elif d["fused_attn"] and ATTN_FP8 and not training and T <= 256:
            ops.attn_fwd_fp8(qkv, ctx, d["lse"][n], B, T, H, D, sc)      # configs[4]'s fp8 attention (opt-in, no-grad forward)
        elif d["fused_attn"]:
            e, pos = ops.attn_fwd(qkv, ctx, d["lse"][n], B, T, H, D, sc, drop_p=p_attn, drop_seed=seed), ops.ATTN_FWD_SEED
        elif d["long_attn"]:
            e, pos = ops.attn_fwd_long(qkv, ctx, d["lse"][n], B, T, H, D, sc, drop_p=p_attn, drop_seed=seed), ops.ATTN_FWD_LONG_SEED
        else:
            ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), d["S"], T, T, D,
                     nb1=B, nb2=H, alpha=sc, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
            ops.softmax_fwd(d["S"], d["P"][n], B * H * T, T, Tp, Tp)
            Pv = d["P"][n]
            if p_attn > 0:      # attention dropout: the dropped copy feeds P V (the backward rebuilds it from P and the seed)
                Pv = d["dS"]
                e, pos = ops.dropout_rows(d["P"][n], Pv, B * H * T, T, Tp, seed, p_attn), ops.DROPOUT_ROWS_SEED
            ops.gemm(Op(Pv, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E),
                     ctx, T, D, T, b_t=True, nb1=B, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D)
        if p_attn > 0:
            self._slot(slots, e, pos, n, self.SITE_ATTN)

    def _attn_bwd(self, d, n, layout, B, dqkv, p_attn, seed, slots, jobs):
        """d_ctx -> dqkv, every row of it written (beyond an utterance's frames, and in the packed tail [row0[B], Mq), as 0).  Seed slots as in
        _attn_fwd.  The fused kernel leaves per-utterance column sums for the q/k/v bias gradients: their reduction joins `jobs`; on the other
        paths the caller's colsum_reduce over dqkv gives them."""
        E, H = self.cfg.embed, self.cfg.heads
        D, T, Tp = E // H, d["T"], d["Tp"]
        qkv, sc = d["qkv"][n], (E // H) ** -0.5
        drop = dict(drop_p=p_attn, drop_seed=seed)
        if layout.packed:
            e = ops.attn_bwd_packed(qkv, d["ctx"][n], d["d_ctx"], d["lse"][n], layout.row0, dqkv, d["attn_ws"], B, T, H, D, layout.Mq, sc, **drop)
            pos = ops.ATTN_BWD_PACKED_SEED
        elif layout.padded:
            e = ops.attn_bwd_varlen(qkv, d["ctx"][n], d["d_ctx"], d["lse"][n], layout.frames, dqkv, d["attn_ws"], B, T, H, D, sc, **drop)
            pos = ops.ATTN_BWD_VARLEN_SEED
        elif d["fused_attn"]:
            e = ops.attn_bwd(qkv, d["ctx"][n], d["d_ctx"], d["lse"][n], dqkv, B, T, H, D, sc, bias_part=d["qkv_bias_part"], **drop)
            pos = ops.ATTN_BWD_SEED
            jobs.append((d["qkv_bias_part"], self._qkv_view("encoder.layers.%d." % n, "bias"), B, 3 * E))
        elif d["long_attn"]:
            e, pos = ops.attn_bwd_long(qkv, d["ctx"][n], d["d_ctx"], d["lse"][n], dqkv, d["attn_ws"], B, T, H, D, sc, **drop), ops.ATTN_BWD_LONG_SEED
        else:
            Pn = Pv = d["P"][n]
            bq = dict(nb1=B, nb2=H)
            if p_attn > 0:      # the dropped probabilities, rebuilt from P with the forward's seed
                Pv = d["dS"]
                self._slot(slots, ops.dropout_rows(Pn, Pv, B * H * T, T, Tp, seed, p_attn), ops.DROPOUT_ROWS_SEED, n, self.SITE_ATTN)
            # dV[j] = sum_i (P o mask)[i][j] dctx[i]
            ops.gemm(Op(Pv, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(d["d_ctx"], E, bs1=T * E, bs2=D), dqkv, T, D, T, a_t=True, b_t=True,
                     ldc=3 * E, c_bs1=T * 3 * E, c_bs2=D, c_offset=2 * E, **bq)
            # dP = (dctx V^T) o mask
            ops.gemm(Op(d["d_ctx"], E, bs1=T * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E), d["S"], T, T, D,
                     ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp, **bq)
            e, pos = None, ops.DROPOUT_ROWS_SEED
            if p_attn > 0:
                e = ops.dropout_rows(d["S"], d["S"], B * H * T, T, Tp, seed, p_attn)
            ops.softmax_bwd(Pn, d["S"], d["dS"], B * H * T, T, Tp, Tp)
            dS = Op(d["dS"], Tp, bs1=H * T * Tp, bs2=T * Tp)
            ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), dqkv, T, D, T, b_t=True, alpha=sc, ldc=3 * E,
                     c_bs1=T * 3 * E, c_bs2=D, c_offset=0, **bq)                                   # dQ = s dS K
            ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=0), dqkv, T, D, T, a_t=True, b_t=True, alpha=sc, ldc=3 * E,
                     c_bs1=T * 3 * E, c_bs2=D, c_offset=E, **bq)                                   # dK = s dS^T Q
        if p_attn > 0:
            self._slot(slots, e, pos, n, self.SITE_ATTN)

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, x, training=True, refresh=True, step_seed=0, frames=None, grad=None, packed=None):
        """x [B, L] fp32 contiguous on the GPU -> (enc_out bf16 [B*T, E], ctx).  step_seed: seed of this step's element-dropout masks.
        frames: int32 [B] on the GPU, the valid frames of each zero-padded utterance — rows beyond them are zeroed before the positional
        convolution and take no part in any soft-max (scl_attn_fwd_varlen / _drop in every layer); output rows beyond them are finite
        and meaningless.  A recorded plan keeps the tensor's address: overwrite it in place before a replay.
        grad: a backward(ctx, ...) will follow (default: autograd is on; a caller inside an autograd.Function, where it is off, says so).
        With frames, a forward that a backward follows takes the shape's training buffer set and the backward masks the same rows;
        without one it is the scoring mode (training=False), whose sets live in the small LRU.
        packed: (row0, Mq) with frames — the transformer layers and the final LayerNorm run on the valid frames only, packed back to back
        (ops.packed_rows: row0 int32 [B + 1] on the GPU, a fixed address like frames; Mq rows per launch, a multiple of 64).  The conv
        stack, zero_tail_rows(x0), the positional convolution and its dropout stay padded (the convolution needs the utterance's slab);
        then xin[0] is packed, the layers run over Mq rows with the packed attention, and the output is unpacked into the padded
        [B*T, E] buffer with zero rows beyond each utterance.  The rows [row0[B], Mq) belong to no utterance: they start as zeros (the
        pack writes them), every kernel but the attention works row by row and keeps them finite, and the attention writes zeros there.
        cfg.layer_mix: enc_out is the soft-max-weighted sum over the layers + 1 hidden states (scl_layer_mix_fwd over the rows of the
        transformer layers, ahead of the unpack) instead of the final LayerNorm's output, which is then kept in f32 as the last state."""
        cfg, P = self.cfg, self.P
        B, L = x.shape
        layout = RowLayout.of(frames, packed)
        grad = torch.is_grad_enabled() if grad is None else bool(grad)
        if not layout.fixed and training and not grad:
            raise NotImplementedError("encoder: per-utterance frame counts without a backward are a scoring mode (training=False, "
                                      "torch.no_grad()); with training=True they need autograd on")
        p_res, p_attn, p_act, p_in = self.drop_probs(training)
        slots = []
        sseed = lambda layer, site: self.site_seed(step_seed, layer, site)
        recording = ops._rec() is not None
        if refresh:
            self.refresh_weights()
        d = self.bufs(B, L, layout, train=grad)
        C, E, H, Fd, K, G = cfg.conv_dim, cfg.embed, cfg.heads, cfg.ffn, cfg.pos_k, cfg.pos_groups
        D, Cg = E // H, E // G
        Ts, T, M, Tp = d["Ts"], d["T"], d["M"], d["Tp"]
        layout.check(B, T)
        Mt = layout.rows(M)      # rows of the transformer layers
        xin0 = d["xin_pad"] if layout.packed else d["xin"][0]      # the positional convolution's (padded) output
        fe = "feature_extractor.conv_layers.%d."
        # -- conv stack (M1)
        ops.conv0_fwd(x, self.b(fe % 0 + "0.weight"), self.b(fe % 0 + "0.bias"), self.b(fe % 0 + "2.1.weight"),
                      self.b(fe % 0 + "2.1.bias"), d["z"][0], B, L, C, cfg.conv_kernels[0], cfg.conv_strides[0], stats=d["conv0_stats"])
        for i in range(1, len(Ts)):
            k, s, Tin, Tout = cfg.conv_kernels[i], cfg.conv_strides[i], Ts[i - 1], Ts[i]
            ops.gemm(Op(d["z"][i - 1], s * C, rpb=Tout, rbstride=Tin * C), Op(self.wk[i], k * C), d["y"][i], B * Tout, C, k * C,
                     bias=self.b(fe % i + "0.bias"))
            ops.layernorm_fwd(d["y"][i], self.b(fe % i + "2.1.weight"), self.b(fe % i + "2.1.bias"), d["z"][i], None,
                              d["cmean"][i], d["crstd"][i], B * Tout, C, act=1)
        ops.layernorm_fwd(d["z"][-1], self.b("layer_norm.weight"), self.b("layer_norm.bias"), d["h0"], None, d["fmean"],
                          d["frstd"], M, C)
        dsc = ops.gemm(Op(d["h0"], C), self.W("post_extract_proj.weight", C), d["x0"], M, E, C, bias=self.b("post_extract_proj.bias"),
                       drop_p=p_in, drop_seed=sseed(-1, self.SITE_IN))        # dropout_input
        if p_in > 0 and recording:
            self._slot(slots, dsc, None, -1, self.SITE_IN)
        # -- positional conv (grouped, weight-normed), GELU, residual (M2 head)
        if not layout.fixed:
            ops.zero_tail_rows(d["x0"], layout.frames, B, T, E)      # fairseq: features[padding_mask] = 0
        ops.pad_rows(d["x0"], d["xpad"], B, T, E, T + K, K // 2)
        if ops.posconv_supported(T, K, G, Cg):      # utterance slab resident in LDS, weights streamed (csrc/posconv.hip); else the grouped GEMM
            ops.posconv_mfma(d["xpad"], self.pos_wf, xin0, d["x0"], B, T, K, G, Cg, bias=self.b("encoder.pos_conv.0.bias"), c2=d["pc_pre"])
        else:
            ops.gemm(Op(d["xpad"], E, rpb=T, rbstride=(T + K) * E, cin=Cg, cout=E, bs2=Cg), Op(self.pos_wf, K * Cg, bs2=Cg * K * Cg),
                     xin0, M, Cg, K * Cg, nb2=G, ldc=E, c_bs2=Cg, bias=self.b("encoder.pos_conv.0.bias"), bias_bs2=Cg,
                     act=ACT_GELU, c2=d["pc_pre"], R=d["x0"], rmode=1)
        if p_res > 0:      # F.dropout(x + pos_conv(x), p = cfg.dropout): after the residual add, so not a GEMM epilogue
            self._slot(slots, ops.dropout(xin0, xin0, None, M * E, sseed(-1, self.SITE_ENC), p_res), ops.DROPOUT_SEED, -1, self.SITE_ENC)
        if layout.packed:      # valid frames back to back, rows [row0[B], Mt) zero
            ops.pack_rows(xin0, d["xin"][0], layout.row0, B, T, E, Mt)
        # -- transformer layers
        skipped = []
        for n in range(cfg.layers):
            pn = "encoder.layers.%d." % n
            xin, xout = d["xin"][n], d["xin"][n + 1]
            if training and cfg.encoder_layerdrop > 0 and float(torch.rand(())) < cfg.encoder_layerdrop:
                xout.copy_(xin)  # fairseq LayerDrop: the whole layer is skipped
                skipped.append(n)
                continue
            ops.layernorm_fwd(xin, self.b(pn + "self_attn_layer_norm.weight"), self.b(pn + "self_attn_layer_norm.bias"),
                              d["h1"][n], None, d["m1"][n], d["r1"][n], Mt, E)
            ops.gemm(Op(d["h1"][n], E), self.W(pn + "self_attn.q_proj.weight", E), d["qkv"][n], Mt, 3 * E, E,
                     bias=self.b(pn + "self_attn.q_proj.bias"))  # q,k,v biases are adjacent in the flat buffer
            self._attn_fwd(d, n, layout, B, training, p_attn, sseed(n, self.SITE_ATTN), slots)
            dsc = ops.gemm(Op(d["ctx"][n], E), self.W(pn + "self_attn.out_proj.weight", E), d["x1"][n], Mt, E, E,
                           bias=self.b(pn + "self_attn.out_proj.bias"), R=xin, rmode=1, drop_p=p_res, drop_seed=sseed(n, self.SITE_1))    # dropout1
            if p_res > 0 and recording:
                self._slot(slots, dsc, None, n, self.SITE_1)
            ops.layernorm_fwd(d["x1"][n], self.b(pn + "final_layer_norm.weight"), self.b(pn + "final_layer_norm.bias"),
                              d["h2"][n], None, d["m2"][n], d["r2"][n], Mt, E)
            # fc1's epilogue stores gelu'(pre-activation) as its second output (one erf / exp evaluation serves gelu and its derivative);
            # fc2's data-gradient epilogue multiplies by the stored number
            dsc = ops.gemm(Op(d["h2"][n], E), self.W(pn + "fc1.weight", E), d["a"][n], Mt, Fd, E, bias=self.b(pn + "fc1.bias"),
                           act=ACT_GELU_DC2, c2=d["f"][n], drop_p=p_act, drop_seed=sseed(n, self.SITE_2))                         # dropout2 (activation)
            if p_act > 0 and recording:
                self._slot(slots, dsc, None, n, self.SITE_2)
            dsc = ops.gemm(Op(d["a"][n], Fd), self.W(pn + "fc2.weight", Fd), xout, Mt, E, Fd, bias=self.b(pn + "fc2.bias"),
                           R=d["x1"][n], rmode=1, drop_p=p_res, drop_seed=sseed(n, self.SITE_3))                                # dropout3
            if p_res > 0 and recording:
                self._slot(slots, dsc, None, n, self.SITE_3)
        if cfg.layer_mix:      # h_L in f32, then the mix of the layers + 1 states over the Mt rows (packed rows in a packed layout)
            ops.layernorm_fwd(d["xin"][cfg.layers], self.b("encoder.layer_norm.weight"), self.b("encoder.layer_norm.bias"),
                              None, d["hL"], d["omean"], d["orstd"], Mt, E)
            ops.layer_mix_fwd(self._mix_states(d), self.P.f32(MIX_WEIGHT), d["out"], Mt * E)
        else:
            ops.layernorm_fwd(d["xin"][cfg.layers], self.b("encoder.layer_norm.weight"), self.b("encoder.layer_norm.bias"),
                              d["out"], None, d["omean"], d["orstd"], Mt, E)
        out = d["out"]
        if layout.packed:      # back to the padded [B*T, E] rectangle, zero rows beyond each utterance
            out = d["out_pad"]
            ops.unpack_rows(d["out"], out, layout.row0, B, T, E, Mt)
        return out, {"d": d, "x": x, "B": B, "L": L, "skipped": skipped, "drop": (p_res, p_attn, p_act, p_in), "step_seed": step_seed,
                     "drop_slots": slots, "layout": layout}

    # ---- fp32 scoring forward ----------------------------------------------------------------------
    def _f32_weights(self):
        """fp32 re-layouts of the weights that are not plain views of the flat buffer (conv stack [C][k*C], weight-normed grouped
        positional conv [G][Cg][K*Cg]); rebuilt when the masters change.  A handful of small torch copies, scoring path only."""
        P, cfg = self.P, self.cfg
        if getattr(self, "_f32w_version", -1) == P.version:
            return self._f32w
        C, E, K, G = cfg.conv_dim, cfg.embed, cfg.pos_k, cfg.pos_groups
        Cg = E // G
        wk = [None] + [P.f32(self.n("feature_extractor.conv_layers.%d.0.weight" % i)).permute(0, 2, 1).reshape(C, -1).contiguous()
                       for i in range(1, len(cfg.conv_kernels))]
        v, g = P.f32(self.n("encoder.pos_conv.0.weight_v")), P.f32(self.n("encoder.pos_conv.0.weight_g"))
        w = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())                              # weight_norm(dim=2)
        pos = w.view(G, Cg, Cg, K).permute(0, 1, 3, 2).reshape(G, Cg, K * Cg).contiguous()       # k index = (tap, channel in group)
        self._f32w, self._f32w_version = {"wk": wk, "pos": pos, "w3": {}}, P.version
        return self._f32w

    def _w3(self, fw, name, N, K):
        """[N, 3 K] bf16 image [hi | lo | hi] of a Linear's fp32 master weight (ops.split3, order 1): the right operand of the scoring
        path's triple-plane GEMMs; built on first use, dropped with the rest of the fp32 re-layouts when the masters change."""
        w3 = fw["w3"].get(name)
        if w3 is None:
            w3 = torch.empty(N * 3 * K, dtype=torch.bfloat16, device=self.dev)
            ops.split3(self.P.flat, N, K, w3, 1, x_offset=self.P.off(self.n(name)))
            fw["w3"][name] = w3
        return w3

    def forward_f32(self, x, frames=None, packed=None):
        """The encoder forward with fp32 activations and the fp32 master weights, every contraction on the exact-fp32 matrix-core
        kernel (csrc/gemm_f32.hip) — what main.py --eval / --predict / --emb score with: the reference runs fp32 end to end
        (main.py:161-214, no autocast) and north_star asks for scores within 1e-3 of it, which bf16 operands cannot give.
        Forward only, one layer's activations live at a time.  x [B, L] fp32 on the GPU -> enc_out f32 [B*T, E].
        frames: as in forward() — int32 [B] on the GPU, valid frames per zero-padded utterance (any head dim).
        packed: (row0, Mq) with frames, as in forward() — the conv stack, zero_tail_rows(x0) and the positional convolution stay padded;
        its f32 result is packed into the other ping-pong buffer, the layers and the final LayerNorm run over Mq rows with the streaming
        fp32 attention of csrc/attention_f32.hip (no S / Pm buffers, no chunk loop above 512 frames), and the output is unpacked into
        the padded [B*T, E] buffer with zero rows beyond each utterance.  The head dims of stream_attn_takes (72..128:
        csrc/attention_f32_wide.hip); any other raises NotImplementedError.
        cfg.layer_mix: the f32 weighted sum over the hidden states is returned instead; one layer is alive at a time here (xa / xb), so
        scl_layer_mix_acc_f32 adds each state as it appears: behind the positional convolution (and the pack), behind every layer but
        the last, and behind the final LayerNorm."""
        cfg, P = self.cfg, self.P
        B, L = x.shape
        C, E, H, Fd, K, G = cfg.conv_dim, cfg.embed, cfg.heads, cfg.ffn, cfg.pos_k, cfg.pos_groups
        D, Cg = E // H, E // G
        Ts = cfg.conv_lens(L)
        T = Ts[-1]
        M, Tp = B * T, (T + 7) // 8 * 8
        layout = RowLayout.of(frames, packed)
        layout.check(B, T)
        Mt, Mp = layout.rows(M), (M + 63) // 64 * 64      # rows of the transformer layers; the packed set's capacity
        # above 512 frames the materialised attention runs in chunks of `bc` utterances (S / Pm sized per chunk, <= F32_ATTN_CHUNK_BYTES)
        long_attn = T > MAT_ATTN_MAX_T and not layout.packed
        bc = max(1, min(B, F32_ATTN_CHUNK_BYTES // (4 * H * T * Tp))) if long_attn else B
        if layout.packed and not stream_attn_takes(D):
            raise NotImplementedError("encoder: SCL_SCORE_PACK=1 needs 64-wide attention heads, or 72..128 in steps of 8 (this encoder's "
                                      "are %d wide): the packed fp32 attention kernels take %s" % (D, STREAM_ATTN_HEAD_DIMS))
        R = Mp if layout.packed else M      # row capacity of the layer buffers: every packed row count of the shape
        nstat = max(B * Ts[1], R)      # LayerNorm statistics: the widest row count of the path

        def make():
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
            slack = 128 * max(C, E)
            d = dict(z=[f32(B * t * C + slack) for t in Ts], y=f32(B * Ts[1] * C), stat=f32(2 * nstat), h=f32(R * max(C, E) + slack),
                     x0=f32(M * E), xpad=torch.zeros(B * (T + K) * E + slack, device=self.dev), xa=f32(R * E), xb=f32(R * E),
                     x1=f32(R * E), qkv=f32(R * 3 * E + slack))
            if not layout.packed:      # the score buffers of the materialised attention
                d.update(S=f32(bc * H * T * Tp), Pm=torch.zeros(bc * H * T * Tp + 1024, device=self.dev))
            d.update(ctx=f32(R * E + slack), a=f32(R * Fd + slack), out=f32(R * E),
                     a3=torch.empty(R * 3 * max(C, E, Fd) + 2 * slack, dtype=torch.bfloat16, device=self.dev),
                     a3b=torch.empty(R * 3 * Fd + 2 * slack, dtype=torch.bfloat16, device=self.dev))
            if layout.packed:      # the padded rectangle behind the unpack
                d["out_pad"] = f32(M * E)
            if cfg.layer_mix:      # the running weighted sum: one layer is alive at a time here, so every state is added as it appears
                d["mix"] = f32(R * E)
            return d
        mix_a = P.f32(MIX_WEIGHT) if cfg.layer_mix else None

        def mix_add(h, index):
            if mix_a is not None:
                ops.layer_mix_acc_f32(h, mix_a, index, d["mix"], Mt * E, accumulate=index > 0)
        d = self._set(("f32",) + layout.key(B, L) + ((bc,) if long_attn else ()), make, layout, f32=True)
        fw = self._f32_weights()
        Wf = lambda name, ld: Op(P.flat, ld, offset=P.off(self.n(name)))
        # Round 6: the plain linears (flat K) as ONE bf16 GEMM over 3 K on the wide-tile kernel — left operand [hi | hi | lo] written by a
        # streaming split pass, right operand [hi | lo | hi] cached per weight: hi.hi + hi.lo + lo.hi with f32 accumulation, the same three
        # products the f32-pair kernel forms inside its K loop (4 - 6e-6 of float64), at the bf16 kernel's operand feed (LDS-DMA, no
        # conversion in the loop).  SCL_SCORE_X3PLANES=0 / shapes with K % 64 != 0: the f32-operand kernel as before.
        use3 = SCORE_X3PLANES and ops.F32X3
        # fc1 -> fc2 without an f32 activation: needs the wide-tile kernel for fc1 (it alone writes the triple-plane image), i.e. K, N
        # multiples of 64 / 8 and enough tiles — asked of the library once per shape
        ffn3 = bool(use3 and E % 64 == 0 and Fd % 64 == 0 and
                    ops.gemm_wide_kind(Op(d["a3"], 3 * E), Op(d["a3"], 3 * E), d["a3b"], Mt, Fd, 3 * E, ldc=3 * Fd))

        LN3 = 0x100      # scl_layernorm_fwd: write [hi | hi | lo] rows straight into a3 (no f32 copy, no split pass)

        def ln_then_lin(xsrc, lnw, lnb, Kin, wname, N, out, rows=None, **epi):
            """LayerNorm(xsrc) -> Linear: the LayerNorm kernel writes the triple-plane operand itself when that path is on.
            rows: the row count (default: the transformer layers', Mt)."""
            R_ = Mt if rows is None else rows
            if use3 and Kin % 64 == 0 and N % 8 == 0:
                ops.layernorm_fwd(xsrc, self.b(lnw), self.b(lnb), d["a3"], None, mean, rstd, R_, Kin, act=LN3)
                ops.gemm(Op(d["a3"], 3 * Kin), Op(self._w3(fw, wname, N, Kin), 3 * Kin), out, R_, N, 3 * Kin, **epi)
            else:
                ops.layernorm_fwd(xsrc, self.b(lnw), self.b(lnb), None, d["h"], mean, rstd, R_, Kin)
                ops.gemm(Op(d["h"], Kin), Wf(wname, Kin), out, R_, N, Kin, **epi)

        def lin(A, Kin, wname, N, out, **epi):
            if use3 and Kin % 64 == 0 and N % 8 == 0:
                ops.split3(A, Mt, Kin, d["a3"], 0)
                ops.gemm(Op(d["a3"], 3 * Kin), Op(self._w3(fw, wname, N, Kin), 3 * Kin), out, Mt, N, 3 * Kin, **epi)
            else:
                ops.gemm(Op(A, Kin), Wf(wname, Kin), out, Mt, N, Kin, **epi)
        fe = "feature_extractor.conv_layers.%d."
        mean, rstd = d["stat"][:nstat], d["stat"][nstat:]
        ops.conv0_fwd_f32(x, self.b(fe % 0 + "0.weight"), self.b(fe % 0 + "0.bias"), self.b(fe % 0 + "2.1.weight"), self.b(fe % 0 + "2.1.bias"),
                          d["z"][0], B, L, C, cfg.conv_kernels[0], cfg.conv_strides[0])
        for i in range(1, len(Ts)):
            k, s, Tin, Tout = cfg.conv_kernels[i], cfg.conv_strides[i], Ts[i - 1], Ts[i]
            ops.gemm(Op(d["z"][i - 1], s * C, rpb=Tout, rbstride=Tin * C), Op(fw["wk"][i], k * C), d["y"], B * Tout, C, k * C, bias=self.b(fe % i + "0.bias"))
            ops.layernorm_fwd(d["y"], self.b(fe % i + "2.1.weight"), self.b(fe % i + "2.1.bias"), None, d["z"][i], mean, rstd, B * Tout, C, act=1)
        ln_then_lin(d["z"][-1], "layer_norm.weight", "layer_norm.bias", C, "post_extract_proj.weight", E, d["x0"], rows=M,
                    bias=self.b("post_extract_proj.bias"))
        # positional conv: zero-padded rows (the pad rows of xpad are never written), GELU, residual
        if not layout.fixed:
            ops.zero_tail_rows(d["x0"], layout.frames, B, T, E)      # fairseq: features[padding_mask] = 0
        d["xpad"][: B * (T + K) * E].view(B, T + K, E)[:, K // 2: K // 2 + T].copy_(d["x0"].view(B, T, E))
        xin, xout = d["xa"], d["xb"]
        ops.gemm(Op(d["xpad"], E, rpb=T, rbstride=(T + K) * E, cin=Cg, cout=E, bs2=Cg), Op(fw["pos"], K * Cg, bs2=Cg * K * Cg), xin, M, Cg, K * Cg,
                 nb2=G, ldc=E, c_bs2=Cg, bias=self.b("encoder.pos_conv.0.bias"), bias_bs2=Cg, act=ACT_GELU, R=d["x0"], rmode=1)
        if layout.packed:      # valid frames back to back into the other ping-pong buffer, rows [row0[B], Mt) zero
            ops.pack_rows(xin, xout, layout.row0, B, T, E, Mt)
            xin, xout = xout, xin
        mix_add(xin, 0)
        qkv = d["qkv"]
        if not layout.packed:
            S, Pm = d["S"], d["Pm"]
            # fp32 soft-max, as fairseq: one wave per row with the row in registers up to 512 frames, the looped kernel for longer rows
            softmax = ops.softmax_fwd_f32_long if long_attn else ops.softmax_fwd_f32
        for n in range(cfg.layers):
            pn = "encoder.layers.%d." % n
            ln_then_lin(xin, pn + "self_attn_layer_norm.weight", pn + "self_attn_layer_norm.bias", E, pn + "self_attn.q_proj.weight", 3 * E, qkv,
                        bias=self.b(pn + "self_attn.q_proj.bias"))
            if layout.packed:      # streaming fp32 attention over the packed rows: one launch, nothing of size T^2
                ops.attn_fwd_packed_f32(qkv, d["ctx"], layout.row0, B, T, H, D, Mt, D ** -0.5)
            else:
                for c0 in range(0, B, bc):      # scores, soft-max, P V per chunk of utterances (up to 512 frames: one chunk of all B)
                    nb, o3 = min(bc, B - c0), c0 * T * 3 * E
                    ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + E), S, T, T, D, nb1=nb, nb2=H,
                             alpha=D ** -0.5, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
                    if layout.padded:      # keys beyond the utterance's frames take no part (any T: one entry point)
                        ops.softmax_fwd_f32_varlen(S, Pm, layout.frames, nb * H * T, H * T, T, Tp, Tp, klen_offset=c0)
                    else:
                        softmax(S, Pm, nb * H * T, T, Tp, Tp)
                    ops.gemm(Op(Pm, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + 2 * E), d["ctx"], T, D, T, b_t=True,
                             nb1=nb, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D, c_offset=c0 * T * E)
            lin(d["ctx"], E, pn + "self_attn.out_proj.weight", E, d["x1"], bias=self.b(pn + "self_attn.out_proj.bias"), R=xin, rmode=1)
            if use3 and ffn3:
                # fc1 writes gelu(.) as the triple-plane image itself (SCL_GEMM_C_SPLIT3: no f32 activation, no split pass) and fc2 reads it
                ln_then_lin(d["x1"], pn + "final_layer_norm.weight", pn + "final_layer_norm.bias", E, pn + "fc1.weight", Fd, d["a3b"],
                            bias=self.b(pn + "fc1.bias"), act=ACT_GELU, ldc=3 * Fd, split3=True)
                ops.gemm(Op(d["a3b"], 3 * Fd), Op(self._w3(fw, pn + "fc2.weight", E, Fd), 3 * Fd), xout, Mt, E, 3 * Fd, bias=self.b(pn + "fc2.bias"),
                         R=d["x1"], rmode=1)
            else:
                ln_then_lin(d["x1"], pn + "final_layer_norm.weight", pn + "final_layer_norm.bias", E, pn + "fc1.weight", Fd, d["a"],
                            bias=self.b(pn + "fc1.bias"), act=ACT_GELU)
                lin(d["a"], Fd, pn + "fc2.weight", E, xout, bias=self.b(pn + "fc2.bias"), R=d["x1"], rmode=1)
            xin, xout = xout, xin
            if n + 1 < cfg.layers:      # the last layer's raw output is no state of the mix: its LayerNorm below is
                mix_add(xin, n + 1)
        ops.layernorm_fwd(xin, self.b("encoder.layer_norm.weight"), self.b("encoder.layer_norm.bias"), None, d["out"], mean, rstd, Mt, E)
        mix_add(d["out"], cfg.layers)
        out = d["mix"] if cfg.layer_mix else d["out"]
        if layout.packed:      # back to the padded [B*T, E] rectangle, zero rows beyond each utterance
            ops.unpack_rows(out, d["out_pad"], layout.row0, B, T, E, Mt)
            return d["out_pad"], T
        return out, T

    # ---- backward --------------------------------------------------------------------------------
    def backward(self, ctx, d_out, mix_only=False, after_mix=None):
        """d_out: bf16 or f32 [M, E] gradient w.r.t. forward()'s output.  Writes every parameter
        gradient of the encoder into the flat gradient buffer (overwrite semantics).
        With cfg.layer_mix, d_out = g = d(mix).  First of all, since it needs nothing the chain produces, scl_layer_mix_bwd_w writes
        d(logits) and s_L g, and after_mix() is called: the logits sit beside LL at the tail of the flat buffer, whose gradients a
        data-parallel caller announces as final before the chain starts.  mix_only (a frozen encoder): that is all.  Otherwise the final
        LayerNorm's backward takes s_L g; at the top of layer n's backward (n <= L - 2, a skipped layer included) s_{n+1} g is added to the
        pair (d(xin[n+1]) f32, its bf16 companion under the dropout3 mask of the next active layer at or below n, as the LayerNorm
        backward above wrote it) before anything reads it; behind the loop s_0 g goes into d(xin[0]), f32 only.  Nothing else moves: the
        residual column sums riding on the LayerNorm backwards then sum the complete d(xout) / d(x1), and every weight-gradient launch, carried
        or on the side stream, is issued behind the injection into the pair it reads.
        A forward with `frames` (ctx["layout"] padded or packed): d_out's rows beyond an utterance's frames must be 0 (the head's masked mean pool and feats
        give that).  Two kernels then carry the mask: scl_attn_bwd_varlen writes zero dqkv rows there, and the rows of d(x0) are zeroed
        behind the positional convolution's data gradient (the backward of the forward's zero_tail_rows(x0)).  Every other kernel of the
        chain works row by row, so the gradient of a padded row is exactly 0 from the head down to the conv stack, and padded rows add
        nothing to any weight, bias or LayerNorm gradient.
        A packed forward (row0, Mq): d_out is packed, the layers run over M = Mp = Mq rows with scl_attn_bwd_packed,
        and d(xin[0]) is unpacked into the padded buffer; everything behind it runs as above.  Inside the packed stretch there are no padded
        rows, only the tail [row0[B], Mq) that belongs to no utterance.  Going forward those rows start as zeros and stay finite through the
        row-wise kernels.  Going backward they start as exact zeros — the pack of d_out writes zeros there, scl_attn_bwd_packed writes zero
        dqkv rows there — and a row-wise kernel turns a zero gradient row into a zero gradient row (finite activations, masks only scale),
        so every gradient buffer is exactly 0 there.  The weight, bias and LayerNorm reductions run over the Mq rows only (Mq is a multiple
        of 64: no K step reaches a stale row), and a zero gradient row times a finite activation row adds nothing to them."""
        cfg, P = self.cfg, self.P
        d, x, B, L = ctx["d"], ctx["x"], ctx["B"], ctx["L"]
        layout = ctx["layout"]
        C, E, H, Fd, K, G = cfg.conv_dim, cfg.embed, cfg.heads, cfg.ffn, cfg.pos_k, cfg.pos_groups
        D, Cg = E // H, E // G
        Ts, T, M, Tp, Mp = d["Ts"], d["T"], d["M"], d["Tp"], d["Mp"]
        Mt = layout.rows(M)      # rows of the transformer layers
        if layout.packed:
            Mp = Mt      # a multiple of 64
            key = "d_out_pk_f32" if d_out.dtype == torch.float32 else "d_out_pk"
            if key not in d:
                d[key] = torch.empty(d["Mp"] * E, dtype=d_out.dtype, device=self.dev)
            ops.pack_rows(d_out, d[key], layout.row0, B, T, E, Mt)      # rows [row0[B], Mt): zeros
            d_out = d[key]
        elif not (WGRAD_GROUP and Mp // 64 >= WGRAD_GROUP_MIN_KSTEPS):
            Mp = M      # short reductions stay on the split-K path, which is faster on the exact row count (pack of 11: 16.2 vs 17.6 ms per step)
        mix_g = mix_a = None
        if cfg.layer_mix:
            mix_g = d_out
            mix_a = self._mix_bwd_w(d, mix_g, Mt)
            if after_mix is not None:
                after_mix()
            if mix_only:
                return []
            d_out = d["mix_gL"]
        nlnM = ops.layernorm_bwd_nparts(Mt)
        p_res, p_attn, p_act, p_in = ctx.get("drop", (0.0, 0.0, 0.0, 0.0))
        step_seed = ctx.get("step_seed", 0)
        slots = []
        sseed = lambda layer, site: self.site_seed(step_seed, layer, site)
        recording = ops._rec() is not None
        active = [n for n in range(cfg.layers) if n not in ctx["skipped"]]
        def mask3_of(layer_list):      # dropout3 mask of the topmost active layer of the list: the bf16 gradient handed down to it carries it
            return ((sseed(layer_list[-1], self.SITE_3), p_res), layer_list[-1]) if (p_res > 0 and layer_list) else ((0, 0.0), None)
        # final LayerNorm
        # residual-gradient buffers rotate over five (f32, bf16) pairs (see bufs(): a weight gradient carried into the next layer's grouped
        # launch reads its operands one layer late): a LayerNorm backward never writes a pair a weight-gradient GEMM may still be reading
        rot = d["dx_rot"]
        NR = len(rot)
        cur = 0
        dx, dxb = rot[cur]
        dout, lyr = mask3_of(active)
        e = ops.layernorm_bwd(d_out, d["xin"][cfg.layers], d["omean"], d["orstd"], self.b("encoder.layer_norm.weight"), None, None,
                              dx, dxb, d["ln_part"], Mt, E, dout=dout)
        if lyr is not None:
            self._slot(slots, e, ops.LN_BWD_DOUT_SEED, lyr, self.SITE_3)
        self._ln_grads(d, nlnM, E, "encoder.layer_norm.weight", "encoder.layer_norm.bias")
        other, otherb = rot[(cur + 1) % NR]
        li, prev_off = 0, None
        d["wgrad_group"], d["wgrad_pending"] = [], []      # nothing is carried across backward passes (an interrupted one may have left work)
        for n in reversed(range(cfg.layers)):
            pn = "encoder.layers.%d." % n
            if mix_g is not None and n <= cfg.layers - 2:      # d(xin[n+1]) += s_{n+1} g, the bf16 companion under the mask it was written with
                (sd, p_), lyr = mask3_of([m_ for m_ in active if m_ <= n])
                e = ops.layer_mix_bwd_inject(mix_g, mix_a, n + 1, dx, dxb, Mt * E, seed=sd, p=p_)
                if lyr is not None:
                    self._slot(slots, e, ops.LAYER_MIX_INJECT_SEED, lyr, self.SITE_3)
            if n in ctx["skipped"]:
                for nm in ("self_attn_layer_norm.weight", "self_attn_layer_norm.bias", "self_attn.q_proj.weight",
                           "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.bias",
                           "self_attn.v_proj.bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "final_layer_norm.weight",
                           "final_layer_norm.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
                    P.g(self.n(pn + nm)).zero_()
                continue
            xin = d["xin"][n]
            d_f, li = d["d_f"][li & 1], li + 1      # li: layers processed so far (the parity picks this layer's d_f / dqkv)
            # ---- FFN:  xout = x1 + gelu(h2 W1^T + b1) W2^T + b2
            with self._side():
                self._wgrad(d, Op(dxb, E), Op(d["a"][n], Fd), P.g(self.n(pn + "fc2.weight")), E, Fd, Mp, slot=0)
            # fc1.bias.grad = colsum(d_f): summed per tile by the GEMM that writes d_f (wide tiles), else by a pass over d_f
            fc2_dgrad = dict(b_t=True, R=d["f"][n], rmode=2, ract=RACT_STORED, drop_p=p_act, drop_seed=sseed(n, self.SITE_2))
            nrows = ops.gemm_colsum_rows(Op(dxb, E), self.W(pn + "fc2.weight", Fd), d_f, Mt, Fd, E, **fc2_dgrad)
            if nrows * Fd > d["cs_fused"].numel():
                nrows = 0
            dsc = ops.gemm(Op(dxb, E), self.W(pn + "fc2.weight", Fd), d_f, Mt, Fd, E, colsum_part=d["cs_fused"] if nrows else None, **fc2_dgrad)
            if p_act > 0 and recording:
                self._slot(slots, dsc, None, n, self.SITE_2)
            jobs = []      # the (up to) four small column reductions that close this layer's backward: one launch at the end of the layer
            if nrows:
                jobs.append((d["cs_fused"], P.g(self.n(pn + "fc1.bias")), nrows, Fd))
            with self._side():
                if not nrows:
                    self._bias_grad(d, d_f, Mt, Fd, pn + "fc1.bias")
                self._wgrad(d, Op(d_f, Fd), Op(d["h2"][n], E), P.g(self.n(pn + "fc1.weight")), Fd, E, Mp, slot=1)
            ops.gemm(Op(d_f, Fd), self.W(pn + "fc1.weight", E), d["d_h"], Mt, E, Fd, b_t=True)
            # dx (= d xout) is the gradient of fc2's output: its column sum (fc2.bias.grad) rides on this LayerNorm backward
            # dres = d(xout): fc2.bias.grad = colsum(dres x dropout3 mask); the bf16 output d(x1) feeds out_proj's gradients: dropout1 mask
            e = ops.layernorm_bwd(d["d_h"], d["x1"][n], d["m2"][n], d["r2"][n], self.b(pn + "final_layer_norm.weight"), None, dx,
                                  other, otherb, d["ln_part"], Mt, E, sum_dres=True,
                                  din=(sseed(n, self.SITE_3), p_res), dout=(sseed(n, self.SITE_1), p_res))
            if p_res > 0:
                self._slot(slots, e, ops.LN_BWD_DIN_SEED, n, self.SITE_3)
                self._slot(slots, e, ops.LN_BWD_DOUT_SEED, n, self.SITE_1)
            jobs.append(self._ln_job(d["ln_part"], nlnM, E, pn + "final_layer_norm.weight", pn + "final_layer_norm.bias", resid_bias=pn + "fc2.bias"))
            cur = (cur + 1) % NR
            (dx, dxb), (other, otherb) = rot[cur], rot[(cur + 1) % NR]      # dx = d x1
            # ---- attention:  x1 = xin + ctx Wo^T + bo
            with self._side():
                self._wgrad(d, Op(dxb, E), Op(d["ctx"][n], E), P.g(self.n(pn + "self_attn.out_proj.weight")), E, E, Mp, slot=2)
            ops.gemm(Op(dxb, E), self.W(pn + "self_attn.out_proj.weight", E), d["d_ctx"], Mt, E, E, b_t=True)
            dqkv = d["dqkv"][li & 1]
            self._attn_bwd(d, n, layout, B, dqkv, p_attn, sseed(n, self.SITE_ATTN), slots, jobs)
            with self._side():
                if not d["fused_attn"]:
                    ops.colsum_reduce(dqkv, d["cs_part"], self._qkv_view(pn, "bias"), Mt, 3 * E)
                self._wgrad(d, Op(dqkv, 3 * E), Op(d["h1"][n], E), self._qkv_view(pn, "weight"), 3 * E, E, Mp, slot=3)
            ops.gemm(Op(dqkv, 3 * E), self.W(pn + "self_attn.q_proj.weight", E), d["d_h"], Mt, E, 3 * E, b_t=True)
            # dx (= d x1) is the gradient of out_proj's output: out_proj.bias.grad rides on this LayerNorm backward
            # dres = d(x1): out_proj.bias.grad = colsum(dres x dropout1 mask); the bf16 output d(xin) feeds the fc2 gradients of the next
            # active layer below: its dropout3 mask
            dout, lyr = mask3_of([m_ for m_ in active if m_ < n])
            e = ops.layernorm_bwd(d["d_h"], xin, d["m1"][n], d["r1"][n], self.b(pn + "self_attn_layer_norm.weight"), None, dx,
                                  other, otherb, d["ln_part2"], Mt, E, sum_dres=True,
                                  din=(sseed(n, self.SITE_1), p_res), dout=dout)
            if p_res > 0:
                self._slot(slots, e, ops.LN_BWD_DIN_SEED, n, self.SITE_1)
                if lyr is not None:
                    self._slot(slots, e, ops.LN_BWD_DOUT_SEED, lyr, self.SITE_3)
            jobs.append(self._ln_job(d["ln_part2"], nlnM, E, pn + "self_attn_layer_norm.weight", pn + "self_attn_layer_norm.bias",
                                     resid_bias=pn + "self_attn.out_proj.bias"))
            ops.colreduce_multi(jobs)
            cur = (cur + 1) % NR
            (dx, dxb), (other, otherb) = rot[cur], rot[(cur + 1) % NR]      # dx = d xin
            self._flush_slabs(d, final=(n == active[0]))
            self._join_side()
            # gradients that are final now: this layer's if nothing of it is still pending in the carried-over tile work, else the previous
            # processed layer's (everything older than one layer has been flushed)
            this_off = P.off(self.n(pn + "self_attn_layer_norm.weight"))
            ready_off = this_off if not d["wgrad_pending"] else prev_off
            prev_off = this_off
            if self.on_grads_ready is not None and ready_off is not None:
                ops.host_callback(self.on_grads_ready, ready_off)
        if mix_g is not None:      # d(xin[0]) += s_0 g: only the f32 side is read from here on
            ops.layer_mix_bwd_inject(mix_g, mix_a, 0, dx, None, Mt * E)
        if layout.packed:      # d(xin[0]) back to the padded rectangle (zero rows beyond each utterance): the convolution needs the slab
            ops.unpack_rows(dx, d["dxin_pad"], layout.row0, B, T, E, Mt)
            dx, (other, otherb) = d["dxin_pad"], d["dx0_pad"]
        # ---- positional conv:  xin0 = x0 + gelu(conv(x0) + b)
        pb = K // 2 - 1
        if p_res > 0:      # backward of F.dropout(x0 + pos_conv(x0)): dx = d(xin[0]) x mask, in place (nothing reads the unmasked value again)
            self._slot(slots, ops.dropout(dx, dx, None, M * E, sseed(-1, self.SITE_ENC), p_res), ops.DROPOUT_SEED, -1, self.SITE_ENC)
        ops.pad_rows(dx, d["dcpad"], B, T, E, T + K, pb, pre=d["pc_pre"], ract=ACT_GELU)
        ops.colsum_reduce(d["dcpad"], d["cs_part"], P.g(self.n("encoder.pos_conv.0.bias")), B * (T + K), E)
        dwf = d["dwf"]
        if ops.posconv_wgrad_supported(T, K, G, Cg):      # accumulators resident over the utterances, one wave per tap
            ops.posconv_wgrad(d["dcpad"], pb, d["xpad"], dwf, B, T, K, G, Cg)
        else:
            self._wgrad(d, Op(d["dcpad"], E, rpb=T, rbstride=(T + K) * E, bs2=Cg, offset=pb * E),
                        Op(d["xpad"], E, rpb=T, rbstride=(T + K) * E, cin=Cg, cout=E, bs2=Cg), dwf, Cg, K * Cg, M,
                        nb2=G, c_bs2=Cg * K * Cg, ldc=K * Cg)
        ops.posconv_weight_bwd(dwf, self.b("encoder.pos_conv.0.weight_v"), self.b("encoder.pos_conv.0.weight_g"), self.pos_norm,
                               self.ws_small, P.g(self.n("encoder.pos_conv.0.weight_v")), P.g(self.n("encoder.pos_conv.0.weight_g")),
                               E, Cg, K)
        if ops.posconv_supported(T, K, G, Cg):
            ops.posconv_mfma(d["dcpad"], self.pos_wd, other, dx, B, T, K, G, Cg)
        else:
            ops.gemm(Op(d["dcpad"], E, rpb=T, rbstride=(T + K) * E, cin=Cg, cout=E, bs2=Cg), Op(self.pos_wd, K * Cg, bs2=Cg * K * Cg),
                     other, M, Cg, K * Cg, nb2=G, ldc=E, c_bs2=Cg, R=dx, rmode=1)
        dx0 = other
        if not layout.fixed:      # the forward zeroed x0's padded rows: no gradient flows into them (the convolution's reaches them)
            ops.zero_tail_rows(dx0, layout.frames, B, T, E)
        if p_in > 0:       # backward of dropout_input: d(post_extract_proj output) = dx0 x mask (f32 for the bias sum, bf16 for the GEMMs)
            self._slot(slots, ops.dropout(dx0, dx0, otherb, M * E, sseed(-1, self.SITE_IN), p_in), ops.DROPOUT_SEED, -1, self.SITE_IN)
        else:
            ops.cast_bf16(dx0, otherb, M * E)
        # ---- post_extract_proj + feature LayerNorm
        self._bias_grad(d, dx0, M, E, "post_extract_proj.bias")
        self._wgrad(d, Op(otherb, E), Op(d["h0"], C), P.g(self.n("post_extract_proj.weight")), E, C, M)
        ops.gemm(Op(otherb, E), self.W("post_extract_proj.weight", C), d["d_h"], M, C, E, b_t=True)
        ops.layernorm_bwd(d["d_h"], d["z"][-1], d["fmean"], d["frstd"], self.b("layer_norm.weight"), None, None, None, d["dz"][-1],
                          d["ln_part"], M, C)
        self._ln_grads(d, ops.layernorm_bwd_nparts(M), C, "layer_norm.weight", "layer_norm.bias")      # the padded rows again (nlnM: the layers')
        # ---- conv stack, layers 6..1
        fe = "feature_extractor.conv_layers.%d."
        for i in reversed(range(1, len(Ts))):
            k, s, Tin, Tout = cfg.conv_kernels[i], cfg.conv_strides[i], Ts[i - 1], Ts[i]
            Mi = B * Tout
            Q, Rp = d["dyp_geom"][i]
            dyp = d["dyp"][i]
            ops.layernorm_bwd(d["dz"][i], d["y"][i], d["cmean"][i], d["crstd"][i], self.b(fe % i + "2.1.weight"),
                              self.b(fe % i + "2.1.bias"), None, None, dyp, d["ln_part"], Mi, C, act=1,
                              out_rpb=Tout, out_rbstride=Rp * C, out_off=Q * C, sum_dres=2)
            # third partial row = colsum of this LayerNorm backward's output = the Conv1d bias gradient
            self._ln_grads(d, ops.layernorm_bwd_nparts(Mi), C, fe % i + "2.1.weight", fe % i + "2.1.bias", resid_bias=fe % i + "0.bias")
            dwk = d["dwk"][: C * k * C].view(C, k * C)
            self._wgrad(d, Op(dyp, C, rpb=Tout, rbstride=Rp * C, offset=Q * C), Op(d["z"][i - 1], s * C, rpb=Tout, rbstride=Tin * C), dwk,
                        C, k * C, Mi)
            ops.conv_weight_unpack_grad(dwk, P.g(self.n(fe % i + "0.weight")), C, C, k)
            # backward-data, one GEMM per output phase p: dz[s*u + p] = sum_q dy[u - q] W[p + s*q]  (K = nq*C, overlapping A rows)
            blk = 0
            for p in range(s):
                nq = len(range(p, k, s))
                Up = (Tin - 1 - p) // s
                if nq == 0:
                    raise NotImplementedError("conv layer with kernel < stride")
                ops.gemm(Op(dyp, C, rpb=Up + 1, rbstride=Rp * C, offset=(Q - (nq - 1)) * C), Op(self.wd[i], C, offset=blk * C * C),
                         d["dz"][i - 1], B * (Up + 1), C, nq * C, b_t=True, ldc=s * C, c_rpb=Up + 1, c_rbstride=Tin * C, c_offset=p * C)
                blk += nq
        ops.conv0_bwd(x, self.b(fe % 0 + "0.weight"), self.b(fe % 0 + "0.bias"), self.b(fe % 0 + "2.1.weight"),
                      self.b(fe % 0 + "2.1.bias"), d["dz"][0], d["conv0_ws"], P.g(self.n(fe % 0 + "0.weight")),
                      P.g(self.n(fe % 0 + "0.bias")), P.g(self.n(fe % 0 + "2.1.weight")), P.g(self.n(fe % 0 + "2.1.bias")),
                      B, L, C, cfg.conv_kernels[0], cfg.conv_strides[0], stats=d["conv0_stats"])
        # names for d(xin[0]) and d(x0) (references to the f32 buffers the backward ended in: nothing behind the positional conv writes them)
        d["dxin0"], d["dx0"] = dx, dx0
        return slots

    def _qkv_view(self, pn, kind):
        """q/k/v gradients are adjacent in the flat buffer: one [3E, E] wgrad / [3E] bias-grad output."""
        E = self.cfg.embed
        o = self.P.off(self.n(pn + "self_attn.q_proj." + kind))
        n = 3 * E * E if kind == "weight" else 3 * E
        v = self.P.grad[o:o + n]
        return v.view(3 * E, E) if kind == "weight" else v
