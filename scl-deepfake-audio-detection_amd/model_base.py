"""What every model plugin shares: `FlatModel`, an nn.Module over one FlatParams buffer and one Encoder, under `model_linear.Model` and
`model_front.FrontHeadModel`; the seeded initialisation, the pretrained-checkpoint hook and `run_plan`, the one place where the launches
of a forward or a backward are recorded into a plan or a recorded plan is replayed.
"""
import math
import os

import torch
from torch import nn

from . import ops
from .encoder import MIX_WEIGHT, Encoder, RowLayout, VarlenSets, shape_entry, w2v_config_from
from .params import FlatParams

HEAD_DIM = 128


def init_parameters_(P, cfg, seed=0):
    """Seeded random init at the right shapes (no checkpoint ships with the repo): kaiming-normal convs
    and N(0, 0.02) linears for the encoder, torch's default uniform for the head."""
    g = torch.Generator().manual_seed(seed)
    for name, (o, n, shape, tr) in P.index.items():
        short = name.split("ssl_model.model.")[-1]
        if short.endswith("2.1.weight") or "layer_norm.weight" in short:
            t = torch.ones(shape)
        elif short.endswith("2.1.bias") or "layer_norm.bias" in short:
            t = torch.zeros(shape)
        elif "conv_layers" in short and short.endswith("0.weight"):
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2]))
        elif short == "encoder.pos_conv.0.weight_v":
            t = torch.randn(shape, generator=g) * math.sqrt(4.0 / (cfg.pos_k * cfg.embed))
        elif short == "encoder.pos_conv.0.weight_g":
            continue
        elif name == MIX_WEIGHT:      # a uniform average of the hidden states; draws nothing, so every other tensor starts as without it
            t = torch.zeros(shape)
        elif name.startswith("LL.") or name.startswith("backend."):
            fan_in = shape[-1] if len(shape) > 1 else HEAD_DIM
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        elif short.endswith(".bias"):
            t = torch.zeros(shape)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        P.f32(name).copy_(t.to(P.device))
    v = P.f32("ssl_model.model.encoder.pos_conv.0.weight_v")
    P.f32("ssl_model.model.encoder.pos_conv.0.weight_g").copy_(v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    P.mark_dirty()


def dropout_stream_seed(seed, rank):
    return (int(seed) * 2654435761 + int(rank) * 40503 + 12345) & 0x7FFFFFFF


def maybe_load_pretrained(model, args):
    """The reference's SSLModel loads pretrained/xlsr2_300m.pt at construction (model/xlsr.py:14-16).  Do the same when the file
    (or the YAML's optional `pretrained:` path) exists; take encoder_layerdrop from its cfg unless the YAML overrides it."""
    from . import checkpoint
    explicit = hasattr(args, "get") and args.get("pretrained")
    path = explicit or checkpoint.DEFAULT_PRETRAINED
    if not os.path.exists(path) or (not explicit and model.cfg.layers != 24):     # toy encoders never pick up the default file
        return False
    probs = checkpoint.load_pretrained_into(model, path)
    if "encoder_layerdrop" in probs and "encoder_layerdrop" not in args:
        model.cfg.encoder_layerdrop = probs["encoder_layerdrop"]
    print("[scl] XLS-R weights loaded from %s (encoder_layerdrop %.3f)" % (path, model.cfg.encoder_layerdrop))
    return True


def run_plan(plans, key, use_plan, patch, build):
    """One forward or backward of a shape's state, recorded on its first run and replayed afterwards.  `plans`: the state's plan dict;
    `patch(plan)` puts this step's seeds into the recorded entries before a replay; `build()` runs the kernels and returns what the plan
    keeps besides its "calls" (a dict).  Returns (the plan, whether it was replayed) — with planning off (use_plan False: the launches
    differ from step to step) build()'s dict in the plan's place, and nothing is stored.  A build() that raises stops the recording, stores
    nothing and raises on."""
    plan = plans.get(key) if use_plan else None
    if plan is not None:
        patch(plan)
        ops.replay(plan["calls"])
        return plan, True
    if not use_plan:
        return build(), False
    ops.start_recording()
    try:
        extras = build()
    finally:
        calls = ops.stop_recording()
    plans[key] = dict(calls=calls, **extras)
    return plans[key], False


class FlatModel(nn.Module):
    """All parameters in one flat fp32 device buffer (self.P), the SSL encoder on it (self.ssl), and per batch shape a state of static
    buffers with the launch plans recorded on them (self._states, self._vstates, self._vstates_train: encoder.shape_entry)."""

    def __init__(self, args, device, is_train=True, w2v_cfg=None):
        super().__init__()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("scl_amd.Model needs an MI355X device: the product path has no CPU fallback")
        self.is_train = is_train
        # optional YAML key `w2v_arch`: a name ("xlsr_300m", the default and the reference's only encoder; "xlsr_1b", "xlsr_2b"; "tiny") or
        # a mapping of W2VConfig fields (encoder.w2v_config_from)
        self.cfg = w2v_config_from(args) if w2v_cfg is None else w2v_cfg

    def _make_params(self, specs):
        """Once the parameter specs are known: the flat buffer.  The sub-class then registers its views under the reference's names and puts
        the initial values in, and calls _finish_build: device allocations keep this order (it decides which freed block a later temporary gets)."""
        self.P = FlatParams(specs, self.device)

    def _finish_build(self, args):
        """The encoder on the filled flat buffer and the per-shape stores; then the pretrained checkpoint, if there is one."""
        self.ssl = Encoder(self.cfg, self.P)      # not `encoder`: that is a child module of the AASIST back-end, grafted at the root
        self._anchor = torch.zeros((), device=self.device, requires_grad=True)
        self._states = {}
        # variable-length scoring batches (forward(x, lengths)): state and launch plans per padded shape, least recently used of at most
        # encoder.VARLEN_SETS; an evicted shape takes its encoder buffer set with it.  Training ones share one padded shape per run: kept
        self._vstates = VarlenSets(on_evict=lambda key: self.ssl._vbufs.pop(key, None))
        self._vstates_train = {}
        self.out_dim = self.cfg.embed
        self.grad_sync = None   # scl_amd.parallel.GradSync when data-parallel (set by FusedAdamW)
        self.pretrained_loaded = maybe_load_pretrained(self, args)

    def layer_mix_weights(self):
        """softmax(layer_mix.weight) on the host: the share of each of the layers + 1 hidden states in what the encoder hands on (YAML
        `ssl_layer_mix`; index 0 the positional-conv residual, index `layers` the final LayerNorm's output).  None with the switch off."""
        if not self.cfg.layer_mix:
            return None
        return torch.softmax(self.P.f32(MIX_WEIGHT).detach().float().cpu(), dim=0)

    # nn.Module plumbing ----------------------------------------------------------------------------
    def _apply(self, fn, recurse=True):
        # .to(device) / .cuda() on an already-placed model must not break the flat-buffer views
        probe = fn(torch.zeros(1, device=self.device))
        if probe.device != self.device or probe.dtype != torch.float32:
            raise RuntimeError("scl_amd.Model lives in one flat fp32 device buffer; construct it on the target device")
        return self

    def _weights_changed(self):
        """The fp32 masters changed behind the views (checkpoint load, optimizer step): what a sub-class derives from them besides."""

    def load_state_dict(self, state_dict, strict=True):
        r = super().load_state_dict(state_dict, strict=strict)
        self._weights_changed()
        self.P.mark_dirty()
        return r

    def optimizer_stepped(self, bf16_fresh):
        self._weights_changed()
        self.P.mark_dirty()
        if bf16_fresh:
            self.P.bf16_version = self.P.version

    # per-shape state -------------------------------------------------------------------------------
    def _shape_state(self, key, make, layout, train=False):
        return shape_entry(key, make, layout, train, self._states, self._vstates, self._vstates_train)

    @staticmethod
    def _bind_layout(st, layout):
        """The frame counts and, packed, the row offsets of this step into the state's buffers, which the recorded plans read."""
        st["frames"].copy_(layout.frames)
        if layout.packed:
            st["row0"].copy_(layout.row0)
        return RowLayout(st["frames"], st["row0"], layout.Mq)
