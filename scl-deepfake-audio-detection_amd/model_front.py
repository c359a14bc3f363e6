"""HIP front end (XLS-R encoder + LL projection, losses) in front of a back-end module: the shared machinery of the
`wav2vec2_aasist`, `wav2vec2_resnet_nll` and `wav2vec2_btse` plugins.

What runs where: the encoder, the LL projection and the three loss terms are the HIP kernels of the wav2vec2_linear_nll
path (one autograd boundary around encoder + LL, launch plans recorded per (B, L)).  The back-end on the [bz, T, 128]
features is an nn.Module (a parameter container whose forward is hand-written HIP behind its own autograd Function: resstack.py +
graph.py, resnet_head.py, btse_head.py) whose parameters are views into the same flat fp32 buffer, so the fused AdamW kernel and the
data-parallel gradient buckets cover them too.  SCL_HEAD_GRAPH=1 replays a back-end as two captured hipGraphs per feature shape (off by
default: the HIP back-ends are a few dozen launches).
Variable-length scoring batches (forward(x, lengths), eval mode under torch.no_grad()) for a back-end that declares `head_takes_frames`
and whose `_head_forward(mod, feats, frames)` masks the padding itself (resnet_head.py; btse_head.py; aasist_head.py behind SCL_AASIST_LENGTHS=1, whose
fused kernels also bound an utterance's frames from above: head_max_frames / max_samples): the encoder runs with its padding mask on either
scoring precision and either row layout, feats rows beyond an utterance's frames are zeroed, and the back-end gets the host-side frame counts.
Variable-length TRAINING batches (train mode, autograd on) for a back-end that declares `head_trains_frames` besides: the autograd boundary
carries the row layout, the encoder trains under its padding mask or on packed rows (SCL_VARLEN_PACK=1; the back-end stays padded), and the
rows of d(feats) beyond an utterance's frames are zeroed before LL's gradients and the encoder backward; the back-end runs eagerly.
`head_takes_frames` / `head_trains_frames` may be properties read at call time: the AASIST plugin declares the training mode only behind
SCL_AASIST_TRAIN_LENGTHS=1 (AasistHead.forward_frames_train) and the scoring mode only behind SCL_AASIST_LENGTHS.
Sub-classes supply `_build_head(args)` (an nn.Module whose children / parameters are grafted at the root under the
reference's state-dict names) and `_head_forward(mod, feats) -> (output, emb)`.
"""
import os

import torch
from torch import nn

from . import encoder as ENC
from . import hipnn
from . import ops
from .encoder import FIXED, param_specs
from .model_base import FlatModel, dropout_stream_seed, init_parameters_, run_plan
from .ops import Op
from .params import register_by_name

FEAT_DIM = 128
SCORE_FP32 = os.environ.get("SCL_SCORE_FP32", "1") != "0"      # scoring runs fp32 end to end unless SCL_SCORE_FP32=0 (the linear plugin keeps a switch of its own)


class _FrontFn(torch.autograd.Function):
    """Autograd boundary around encoder + LL: waveform -> feats [bz, T, 128] fp32."""

    @staticmethod
    def forward(ctx, model, x, anchor, layout=FIXED):
        feats, saved = model._front_forward(x, layout, train=True)      # layout: the rows of a variable-length training batch
        ctx.model, ctx.saved = model, saved
        return feats.clone()

    @staticmethod
    def backward(ctx, d_feats):
        ctx.model._front_backward(ctx.saved, d_feats)
        return None, None, None, None


class _HeadRunner(nn.Module):
    """The graph back-end's sub-modules and parameters (shared objects, not copies) under one nn.Module: the unit that
    torch.cuda.make_graphed_callables captures into a forward and a backward hipGraph."""

    def __init__(self, owner):
        super().__init__()
        for n in owner._head_children:
            self.add_module(n, owner._modules[n])
        for n in owner._head_root_params:
            self.register_parameter(n, owner._parameters[n])
        self.__dict__["_fwd"] = owner._head_forward

    def forward(self, feats):
        return self._fwd(self, feats)


class FrontHeadModel(FlatModel):
    flag_fix_ssl = False
    head_takes_frames = False      # the back-end masks the padding of a variable-length batch: _head_forward(mod, feats, frames)
    head_trains_frames = False     # ... in train mode with autograd on too (masked batch statistics and a masked backward)
    front_prefix = ""        # module path of `ssl_model` / `LL` in the state dict ("backend." for wav2vec2_btse, backend.py:31-33)

    def _build_head(self, args):
        raise NotImplementedError

    @staticmethod
    def _head_forward(mod, feats):
        raise NotImplementedError

    def _ssl_train(self):
        return bool(self.training)

    def head_min_frames(self):
        """The fewest frames per utterance the back-end takes (a head_takes_frames plugin overrides it)."""
        return 1

    def min_samples(self):
        """The shortest row forward(x, lengths) takes: main.py --padding_type none zero-pads shorter files to it."""
        return self.cfg.samples_for(self.head_min_frames())

    def head_max_frames(self):
        """The most frames per utterance the back-end takes with lengths, or None: no limit of its own (a head_takes_frames plugin overrides it)."""
        return None

    def max_samples(self):
        """The longest row forward(x, lengths) takes: main.py --padding_type none cuts longer files to it.  pack.VARLEN_MAX_SAMPLES unless the
        back-end has a limit of its own: then the most samples that still give head_max_frames() frames."""
        from .pack import VARLEN_MAX_SAMPLES
        hi = self.head_max_frames()
        if hi is None:
            return VARLEN_MAX_SAMPLES
        return min(VARLEN_MAX_SAMPLES, self.cfg.samples_for(hi + 1) - 1)

    def __init__(self, args, device, is_train=True, w2v_cfg=None, seed=0, rank=0):
        super().__init__(args, device, is_train, w2v_cfg)
        self.contra_mode = args.get("contra_mode", "all")
        self.loss_type = args.get("loss_type", 1)
        rng_state = torch.get_rng_state()          # seeded head init without disturbing the caller's RNG stream
        torch.manual_seed(seed + 1)
        head = self._build_head(args)
        torch.set_rng_state(rng_state)
        head_params = list(head.named_parameters())
        frozen = getattr(head, "frozen_names", ())      # no gradient in the reference
        specs = param_specs(self.cfg) + [("LL.weight", (FEAT_DIM, self.cfg.embed), True), ("LL.bias", (FEAT_DIM,), True)] + \
            ENC.mix_specs(self.cfg) + [(n, tuple(p.shape), n not in frozen) for n, p in head_params]
        self._make_params(specs)
        self._head_lo = self.P.off(next(n for n, _ in head_params if n not in frozen))
        init_parameters_(self.P, self.cfg, seed)
        for n, p in head_params:
            self.P.f32(n).copy_(p.detach().to(self.device))
        # graft the head's sub-modules at the root (reference state-dict names: encoder.0.0.conv1.weight, GAT_layer_S.…) and
        # swap every head parameter for its flat-buffer view
        head.to(self.device)
        self._head_children = [n for n, _ in head.named_children()]
        self._head_root_params = list(head._parameters.keys())
        for n, child in head.named_children():
            self.add_module(n, child)
        for name, p in self.P.params.items():
            if name.startswith("ssl_model.") or name.startswith("LL.") or name == ENC.MIX_WEIGHT:
                register_by_name(self, self.front_prefix + name, p)
            else:
                mod = self
                parts = name.split(".")
                for part in parts[:-1]:
                    mod = mod._modules[part]
                mod._parameters[parts[-1]] = p
        self.P.mark_dirty()
        self._drop_step = dropout_stream_seed(seed, rank)      # encoder element-dropout masks differ per --seed and per data-parallel rank
        # Optional (SCL_HEAD_GRAPH=1): replay the back-end's training forward / backward as two captured hipGraphs per feature
        # shape.  Both HIP back-ends capture and replay correctly (tests/test_aasist_gpu.py), but the step is kernel-bound: AASIST
        # 45.9 -> 45.5 ms/step at batch 32, ResNet +-0.  Off by default.
        self.use_graphs = os.environ.get("SCL_HEAD_GRAPH", "0") == "1"
        self.__dict__["_graphed"] = {}
        self._finish_build(args)      # the fp32 scoring path keeps no state in the stores (Encoder.forward_f32's own LRU)
        if rank:      # torch dropout in the back-end: decorrelate the data-parallel ranks' masks
            torch.cuda.manual_seed(int(seed) * 1000003 + int(rank))

    def trainable_range(self):
        return 0, self.P.n_train

    def _weights_changed(self):
        hipnn.weights_changed()      # the back-end's re-laid-out convolution weights are rebuilt on next use

    def zero_torch_grads(self):
        """The head's gradients are ACCUMULATED by torch autograd into the flat gradient buffer (the HIP backward
        overwrites its part), so FusedAdamW.zero_grad clears that 0.4 M-element tail."""
        self.P.rebind_grads()
        self.P.grad[self._head_lo:].zero_()

    # encoder + LL ----------------------------------------------------------------------------------
    def _state(self, B, L, layout=FIXED, train=False):
        """Boundary buffers and launch plans of a [B, L] batch.  A variable-length batch: the frame counts and, packed, the row offsets
        besides — device buffers of fixed address, overwritten before every replay; a state of its own per layout.  Forward-only for a
        scoring batch (least recently used of a few); with the backward's buffers for a training one (train: kept)."""
        def make():
            T = self.cfg.conv_lens(L)[-1]
            M, E, dev = B * T, self.cfg.embed, self.device
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            st = dict(T=T, x=f32(B, L), feats=f32(B, T, FEAT_DIM), dfe_bf=bf(M * FEAT_DIM + 1024), plans={})
            if layout.fixed or train:
                st.update(d_feats=f32(B, T, FEAT_DIM), denc=bf(M * E), cs=f32(ops.colsum_reduce_nparts(M, 8) * FEAT_DIM))
            if not layout.fixed:
                st.update(frames=torch.ones(B, **i32), row0=torch.arange(B + 1, **i32) if layout.packed else None)
            return st
        return self._shape_state(layout.key(B, L), make, layout, train)

    def _front_forward(self, x, layout=FIXED, train=False):
        """Encoder (bf16 kernels) + LL on the shape's state, recorded once per plan key and replayed.  A variable-length batch: padding mask
        (or packed rows) in the encoder, feats rows beyond an utterance's frames zeroed.  train: a backward follows (_FrontFn) — a
        variable-length batch then takes the shape's training state and the encoder its dropout seeds, as a fixed-length one; without it
        a variable-length batch is scored (no dropout mask drawn)."""
        B, L = x.shape
        ssl_train = (layout.fixed or train) and self._ssl_train()
        st = self._state(B, L, layout, train)
        st["x"].copy_(x)
        seed = 0
        if layout.fixed or train:
            self._drop_step = seed = (self._drop_step * 1664525 + 1013904223) & 0x7FFFFFFF
        if not layout.fixed:
            layout = self._bind_layout(st, layout)
        self.ssl.refresh_weights()
        use_plan = self.cfg.encoder_layerdrop == 0 or not ssl_train
        pk = layout.plan_key("fwd", ssl_train)

        def build():
            P, E = self.P, self.cfg.embed
            enc_out, ectx = self.ssl.forward(st["x"], training=ssl_train, refresh=False, step_seed=seed,
                                             grad=None if layout.fixed else train, **layout.args)
            M = B * st["T"]
            # the bf16 primary output of the GEMM is not needed here: it lands in dfe_bf, which the backward overwrites
            ops.gemm(Op(enc_out, E), Op(P.bf16, E, offset=P.off("LL.weight")), st["dfe_bf"], M, FEAT_DIM, E, bias=P.f32("LL.bias"),
                     c2=st["feats"])
            if not layout.fixed:
                ops.zero_tail_rows(st["feats"], layout.frames, B, st["T"], FEAT_DIM)
            return dict(saved=dict(ectx=ectx, st=st, enc_out=enc_out, B=B))
        # replay: the encoder's element-dropout sites (none at p = 0) take this step's seed
        plan, replayed = run_plan(st["plans"], pk, use_plan, lambda plan: self.ssl.apply_seeds(plan["saved"]["ectx"]["drop_slots"], seed), build)
        saved = plan["saved"]
        if replayed:
            saved = dict(saved, ectx=dict(saved["ectx"], step_seed=seed))
        return st["feats"], saved

    def _front_f32(self, x, layout=FIXED):
        """Scoring: fp32 activations / master weights / exact-fp32 GEMMs through the encoder and LL (the back-end is fp32 anyway)."""
        B, E = x.shape[0], self.cfg.embed
        enc, T = self.ssl.forward_f32(x, **layout.args)
        feats = torch.empty(B, T, FEAT_DIM, device=self.device)
        ops.gemm(Op(enc, E), Op(self.P.flat, E, offset=self.P.off("LL.weight")), feats, B * T, FEAT_DIM, E, bias=self.P.f32("LL.bias"))
        if not layout.fixed:
            ops.zero_tail_rows(feats, layout.frames, B, T, FEAT_DIM)
        return feats

    def _front_backward(self, sv, d_feats):
        P, E = self.P, self.cfg.embed
        P.rebind_grads()
        st = sv["st"]
        st["d_feats"].copy_(d_feats)
        if self.grad_sync is not None:
            self.ssl.on_grads_ready = self.grad_sync.ready_above
        use_plan = not sv["ectx"]["skipped"] and self.cfg.encoder_layerdrop == 0
        layout = sv["ectx"]["layout"]      # the row offsets and frame counts are the state's, already in place
        pk = layout.plan_key("bwd", self.grad_sync is not None)

        def build():
            enc_slots = []
            M = sv["B"] * st["T"]
            if layout.frames is not None:
                # the forward zeroed feats beyond the frames (zero_tail_rows), so whatever the loss hands back there (SupCon's gradient is
                # not 0) stops here, before LL's gradients and the encoder backward
                ops.zero_tail_rows(st["d_feats"], layout.frames, sv["B"], st["T"], FEAT_DIM)
            ops.cast_bf16(st["d_feats"], st["dfe_bf"], M * FEAT_DIM)
            ops.colsum_reduce(st["d_feats"], st["cs"], P.g("LL.bias"), M, FEAT_DIM)
            self.ssl._wgrad(sv["ectx"]["d"], Op(st["dfe_bf"], FEAT_DIM), Op(sv["enc_out"], E), P.g("LL.weight"), FEAT_DIM, E, M)
            if self.cfg.layer_mix:
                # the mix's logits lie between LL and the torch head: final once the encoder backward's first launch has run (after_mix);
                # a frozen encoder still forms d(mix) for them alone (mix_only) and announces nothing, as without the mix
                ops.gemm(Op(st["dfe_bf"], FEAT_DIM), Op(P.bf16, E, offset=P.off("LL.weight")), st["denc"], M, E, FEAT_DIM, b_t=True)
                ready = None
                if self.grad_sync is not None and not self.flag_fix_ssl:
                    ready = lambda: ops.host_callback(self.grad_sync.ready_above, P.off("LL.weight"))
                enc_slots = self.ssl.backward(sv["ectx"], st["denc"], mix_only=self.flag_fix_ssl, after_mix=ready)
            elif not self.flag_fix_ssl:
                ops.gemm(Op(st["dfe_bf"], FEAT_DIM), Op(P.bf16, E, offset=P.off("LL.weight")), st["denc"], M, E, FEAT_DIM, b_t=True)
                if self.grad_sync is not None:     # LL and the torch head's gradients (the END of the flat buffer) are final here
                    ops.host_callback(self.grad_sync.ready_above, P.off("LL.weight"))
                enc_slots = self.ssl.backward(sv["ectx"], st["denc"])
            return dict(enc_slots=enc_slots)
        run_plan(st["plans"], pk, use_plan, lambda plan: self.ssl.apply_seeds(plan["enc_slots"], sv["ectx"]["step_seed"]), build)

    # forward / loss --------------------------------------------------------------------------------
    VARLEN_REFUSAL = ("variable-length batches (forward(x, lengths), main.py --padding_type none, --padding_type zero --batch_size k) "
                      "are implemented for the wav2vec2_linear_nll and wav2vec2_resnet_nll plugins: this back-end has no padding mask; "
                      "use fixed-length clips (--padding_type zero / repeat at --batch_size 1) or one utterance per call")
    LENGTHS_SWITCH = None      # a plugin whose scoring mode with lengths is opt-in names its environment switch here

    def forward(self, x, lengths=None):
        if lengths is not None and not self.head_takes_frames:
            hint = "" if self.LENGTHS_SWITCH is None else ".  %s=1 turns on this plugin's scoring mode with lengths (eval mode under torch.no_grad())" % self.LENGTHS_SWITCH
            raise NotImplementedError("%s: %s%s" % (type(self).__module__.split(".")[-1], self.VARLEN_REFUSAL, hint))
        if x.dim() == 3:
            x = x[:, :, 0]
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        counts, layout = None, FIXED
        if lengths is not None:
            train = bool(self.training) and torch.is_grad_enabled() and self.head_trains_frames
            if not train and (self.training or torch.is_grad_enabled()):
                raise NotImplementedError("%s: forward(x, lengths) is a scoring mode on model.eval() under torch.no_grad()%s; eval with "
                                          "autograd on, or train mode under torch.no_grad(), is neither"
                                          % (type(self).__module__.split(".")[-1],
                                             " and a training mode on model.train() with autograd on" if self.head_trains_frames else
                                             " (training on zero-padded batches: wav2vec2_linear_nll and wav2vec2_resnet_nll)"))
            # the packed layout: encoder.VARLEN_PACK serves the bf16 encoder path (training, bf16 scoring), encoder.SCORE_PACK fp32 scoring
            if self.head_max_frames() is not None and max(int(n) for n in lengths) > self.max_samples():
                raise ValueError("%s: forward(x, lengths) takes at most %d samples (%d frames) per utterance — the back-end's fused kernels keep "
                                 "an utterance's temporal nodes in LDS — got %d" % (type(self).__module__.split(".")[-1], self.max_samples(),
                                                                                   self.head_max_frames(), max(int(n) for n in lengths)))
            counts, layout = ENC.row_layout(self.cfg, lengths, *x.shape, min_samples=self.min_samples(), refuse_short=True,
                                            score_f32=not train and SCORE_FP32, device=self.device)
        if torch.is_grad_enabled():
            feats = _FrontFn.apply(self, x, self._anchor, layout)
        elif not self.training and SCORE_FP32:
            feats = self._front_f32(x, layout)
        else:
            feats = self._front_forward(x, layout)[0].clone()
        # a variable-length batch: the back-end masks the padding itself, from the host-side frame counts
        output, last_hidden = self._head(feats) if counts is None else self._head_forward(self, feats, counts)
        if self.is_train:
            return output, feats, last_hidden
        return output

    def _head(self, feats):
        if not (self.use_graphs and self.training and torch.is_grad_enabled() and feats.requires_grad):
            return self._head_forward(self, feats)
        key = tuple(feats.shape)
        runner = self._graphed.get(key)
        if runner is None:
            runner = self._capture_head(feats)
            self._graphed[key] = runner
        if runner is False:          # capture failed once for this shape: stay eager
            return self._head_forward(self, feats)
        out, hid = runner(feats)          # static graph outputs: hand out copies, successive calls must not alias
        return out.clone(), hid.clone()

    def _capture_head(self, feats):
        """Warm-up + capture (torch runs the callable a few times on a side stream): BatchNorm running statistics and the RNG
        offset it consumes are put back afterwards, so capturing is invisible to the training trajectory."""
        runner = _HeadRunner(self)
        runner.train()
        saved = [b.detach().clone() for b in runner.buffers()]
        rng = torch.cuda.get_rng_state(self.device)
        try:
            sample = feats.detach().clone().requires_grad_(True)
            runner = torch.cuda.make_graphed_callables(runner, (sample,), allow_unused_input=True)   # e.g. AASIST's bn1 of Residual_block is unused
        except Exception as e:   # noqa: BLE001 - any capture problem degrades to the eager path, loudly
            print("[scl_amd] torch back-end: hipGraph capture failed (%s: %s); running it eagerly" % (type(e).__name__, e))
            runner = False
        finally:
            with torch.no_grad():
                for b, v in zip(_HeadRunner(self).buffers(), saved):
                    b.copy_(v)
            torch.cuda.set_rng_state(rng, self.device)
        return runner
