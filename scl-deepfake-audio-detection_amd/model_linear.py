"""`wav2vec2_linear_nll` model plugin — host-side mirror of the reference's
model/wav2vec2_linear_nll.py::Model (ctor, `is_train`, forward, loss), with every
numeric step executed by the HIP kernels behind the C ABI.

    Model(args: dict, device, is_train=True)
    forward(x [bz, L] fp32) -> (log_probs [bz,2], feats [bz,T,128], emb [bz,128])   (or log_probs when not is_train)
    forward(x, lengths=[n_0, ...])   row b holds n_b samples followed by padding and gets the result it gets alone at its own length; feats
                                     rows beyond its frames are 0.  Scoring (eval, no_grad) or training (train mode, autograd on: the
                                     backward carries the same mask, padded frames add nothing to any gradient)
    loss(output, feats, emb, labels, config, info=None) -> dict of 0-d tensors, summed and .backward()-ed by the caller

State-dict keys equal the reference's (ssl_model.model.<fairseq keys>, LL.*, first_bn.*, first_bn1.*,
backend.m_frame_level.{0,3,6}.*, backend.m_utt_level.*), so its checkpoints load unchanged.  The YAML key `ssl_layer_mix: true` (not in
the reference) adds one, `layer_mix.weight`: LL then reads the learned weighted sum over all hidden states of the encoder (encoder.py).
`train_loss.backward()` reaches the hand-written backward through two torch.autograd.Function
boundaries (model, loss); parameter gradients are written straight into the flat gradient buffer.
"""
import os

import torch
from torch import nn

from . import encoder as ENC
from . import ops
from .encoder import FIXED, param_specs
from .lib import ACT_LEAKY, ACT_RELU
from .model_base import HEAD_DIM, FlatModel, dropout_stream_seed, init_parameters_, maybe_load_pretrained, run_plan  # noqa: F401
from .ops import Op
from .params import register_by_name

N_CLASS = 2
# scoring (model.eval() under torch.no_grad(): main.py --eval / --predict / --emb, the validation pass) runs fp32 end to end unless
# SCL_SCORE_FP32=0 asks for the bf16-operand training kernels (about 8x faster forward, scores to ~1e-2)
SCORE_FP32 = os.environ.get("SCL_SCORE_FP32", "1") != "0"
# the 128-wide frame-level head in f32 on the exact-fp32 GEMM (SCL_HEAD_F32=0: bf16 operands, the A/B switch of tests / probes)
HEAD_F32 = os.environ.get("SCL_HEAD_F32", "1") != "0"
X3_OFF = {"x3": False} if HEAD_F32 else {}      # the training head's f32 GEMMs stay on the exact kernel (its backward is checked at 4e-6)
DROP_P = 0.5  # BackEnd(128, 128, 2, 0.5, False): torch.nn.Dropout(0.5) after each frame-level layer


def head_specs(embed, mix=()):
    """mix: encoder.mix_specs(cfg) — the layer mix's logits directly behind LL.bias (nothing with the switch off)."""
    return [("LL.weight", (HEAD_DIM, embed), True), ("LL.bias", (HEAD_DIM,), True)] + list(mix) + [
            ("backend.m_frame_level.0.weight", (HEAD_DIM, HEAD_DIM), True), ("backend.m_frame_level.0.bias", (HEAD_DIM,), True),
            ("backend.m_frame_level.3.weight", (HEAD_DIM, HEAD_DIM), True), ("backend.m_frame_level.3.bias", (HEAD_DIM,), True),
            ("backend.m_frame_level.6.weight", (HEAD_DIM, HEAD_DIM), True), ("backend.m_frame_level.6.bias", (HEAD_DIM,), True),
            ("backend.m_utt_level.weight", (N_CLASS, HEAD_DIM), True), ("backend.m_utt_level.bias", (N_CLASS,), True)]


class _ModelFn(torch.autograd.Function):
    """Autograd boundary around the whole network: forward runs the kernels and keeps the activation
    buffers; backward consumes (d_logp, d_feats, d_emb) and fills the flat gradient buffer."""

    @staticmethod
    def forward(ctx, model, x, anchor, layout=FIXED):
        out, feats, emb, saved = model._run_forward(x, layout, train=not layout.fixed)
        ctx.model, ctx.saved = model, saved
        # the outputs live in static per-(B, L) buffers (launch plans point at them): hand out copies, so results
        # of successive forward calls do not alias (3 small device copies)
        return out.clone(), feats.clone(), emb.clone()

    @staticmethod
    def backward(ctx, d_out, d_feats, d_emb):
        ctx.model._run_backward(ctx.saved, d_out, d_feats, d_emb)
        return None, None, None, None


class Model(FlatModel):
    def __init__(self, args, device, is_train=True, w2v_cfg=None, seed=0, rank=0):
        super().__init__(args, device, is_train, w2v_cfg)
        self.flag_fix_ssl = args["flag_fix_ssl"]
        self.contra_mode = args["contra_mode"]
        self.loss_type = args["loss_type"]
        if self.contra_mode not in ("all", "one"):
            raise ValueError("Unknown mode: {}".format(self.contra_mode))     # loss_metrics.py:161
        # memory order: trainable encoder, head, then the checkpoint-only tensors (FlatParams puts those last)
        self._make_params(param_specs(self.cfg) + head_specs(self.cfg.embed, ENC.mix_specs(self.cfg)))
        for name, p in self.P.params.items():
            register_by_name(self, name, p)
        # defined-but-unused modules of the reference (linear_nll:108-109) — state-dict compatibility only
        self.first_bn = nn.BatchNorm2d(num_features=1).to(self.device)
        self.first_bn1 = nn.BatchNorm2d(num_features=64).to(self.device)
        init_parameters_(self.P, self.cfg, seed)
        self._hbufs = {}
        self._step_seed = dropout_stream_seed(seed, rank)   # head dropout masks differ per --seed and per data-parallel rank
        self._finish_build(args)

    encoder = property(lambda self: self.ssl)      # read-only alias of FlatModel.ssl: there is no setter, `m.encoder = ...` raises

    def trainable_range(self):
        """[lo, hi) of the flat buffer that receives gradients: with flag_fix_ssl the encoder backward is skipped, and
        torch.optim.AdamW in the reference leaves parameters whose .grad is None untouched (no weight decay, no all-reduce)."""
        return (self.P.off("LL.weight") if self.flag_fix_ssl else 0), self.P.n_train

    # forward ---------------------------------------------------------------------------------------
    def _head_bufs(self, B, T, keep=True):
        key = (B, T)
        if not keep:      # a variable-length state owns its head buffers (freed with it)
            return self._make_head_bufs(B, T)
        if key not in self._hbufs:
            self._hbufs[key] = self._make_head_bufs(B, T)
        return self._hbufs[key]

    def _make_head_bufs(self, B, T):
        M, dev = B * T, self.device
        bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        # the frame-level head (three 128 x 128 linears) runs in f32 on the exact-fp32 GEMM with the fp32 master weights, forward and
        # backward: 3.8 GFLOP per step at batch 64, and its gradients then meet the same bound as every other tensor (the
        # mean-pool backward hands every frame of an utterance the SAME row — rounded to bf16 its error is systematic over T)
        hd = f32 if HEAD_F32 else bf
        return dict(r0=hd(M * HEAD_DIM + 1024), pre=[hd(M * HEAD_DIM) for _ in range(3)],
                    h=[hd(M * HEAD_DIM + 1024) for _ in range(3)], dpre=[hd(M * HEAD_DIM + 1024) for _ in range(3)],
                    dfe=f32(M * HEAD_DIM), dfe_bf=bf(M * HEAD_DIM + 1024), denc=bf(M * self.cfg.embed),
                    demb=f32(B * HEAD_DIM), ws=f32(B * N_CLASS + 16),
                    cs=f32(ops.colsum_reduce_nparts(M, 8) * max(HEAD_DIM, 8)), dW=f32(HEAD_DIM * max(HEAD_DIM, self.cfg.embed)))

    def _state(self, B, L, layout=FIXED, train=False):
        """Static buffers of a [B, L] batch at the autograd boundary, so recorded launch plans stay valid.  A variable-length batch (a state
        of its own per row layout, keyed like the encoder's buffer set): the frame counts and, packed, the row offsets besides — device
        buffers of fixed address, overwritten before every replay of the shape's plans, which are kept per packed row count — and the shape's
        own head buffers; forward-only for a scoring batch (least recently used of a few), both directions for a training one (kept)."""
        def make():
            T = self.cfg.conv_lens(L)[-1]
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
            i32 = dict(dtype=torch.int32, device=self.device)
            st = dict(T=T, x=f32(B, L), feats=f32(B, T, HEAD_DIM), emb=f32(B, HEAD_DIM), logp=f32(B, N_CLASS), train=train, plans={})
            if layout.fixed or train:
                st.update(d_logp=f32(B, N_CLASS), d_feats=f32(B, T, HEAD_DIM), d_emb=f32(B, HEAD_DIM))
            if not layout.fixed:
                st.update(frames=torch.ones(B, **i32), row0=torch.arange(B + 1, **i32) if layout.packed else None,
                          hb=self._head_bufs(B, T, keep=False))
            return st
        return self._shape_state(layout.key(B, L), make, layout, train)

    def min_samples(self):
        """The shortest row forward(x, lengths) takes (main.py --padding_type none pads shorter files to it): one frame."""
        return self.cfg.min_samples()

    def _run_forward(self, x, layout=FIXED, train=False):
        """layout: the rows of the batch (encoder.row_layout); train: a backward follows a variable-length batch."""
        B, L = x.shape
        training = bool(self.training)
        ssl_train = False if self.flag_fix_ssl else bool(self.is_train and training)
        st = self._state(B, L, layout, train)
        if not layout.fixed:
            layout = self._bind_layout(st, layout)
        st["x"].copy_(x)
        drop = DROP_P if training else 0.0
        self._step_seed = (self._step_seed * 1664525 + 1013904223) & 0x7FFFFFFF
        seeds = [(self._step_seed + 7919 * j) & 0x7FFFFFFF for j in range(3)]
        self.encoder.refresh_weights()
        use_plan = self.cfg.encoder_layerdrop == 0 or not ssl_train
        pk = layout.plan_key("fwd", training, ssl_train)

        def patch(plan):
            for dsc, sd in zip(plan["drop_descs"], seeds):
                dsc.drop_seed = sd
            self.encoder.apply_seeds(plan["saved"]["ectx"]["drop_slots"], self._step_seed)      # the encoder's element-dropout sites (none at p = 0)

        def build():
            saved, drop_descs = self._forward_kernels(st, B, L, ssl_train, drop, seeds, layout)
            return dict(drop_descs=drop_descs, saved=saved)
        plan, replayed = run_plan(st["plans"], pk, use_plan, patch, build)
        saved = plan["saved"]
        if replayed:      # the recorded step's context with this step's seed; a first run hands on the encoder's own
            saved = dict(saved, ectx=dict(saved["ectx"], step_seed=self._step_seed))
        return st["logp"], st["feats"], st["emb"], dict(saved, seeds=seeds)

    def _forward_kernels(self, st, B, L, ssl_train, drop, seeds, layout):
        P, E = self.P, self.cfg.embed
        enc_out, ectx = self.encoder.forward(st["x"], training=ssl_train, refresh=False, step_seed=self._step_seed,
                                             grad=None if layout.fixed else st["train"], **layout.args)
        T = ectx["d"]["T"]
        M = B * T
        hb = self._head_bufs(B, T) if layout.fixed else st["hb"]
        feats, emb, logp = st["feats"], st["emb"], st["logp"]
        W = lambda name, ld: Op(P.bf16, ld, offset=P.off(name))
        # feats = LL(x) (pre-ReLU tensor is what SupCon sees, linear_nll:127-129), r0 = relu(feats)
        ops.gemm(Op(enc_out, E), W("LL.weight", E), hb["r0"], M, HEAD_DIM, E, bias=P.f32("LL.bias"), act=ACT_RELU, c2=feats)
        Wf = (lambda name, ld: Op(P.flat, ld, offset=P.off(name))) if HEAD_F32 else W
        prev, drop_descs = hb["r0"], []
        for j, idx in enumerate((0, 3, 6)):
            dsc = ops.gemm(Op(prev, HEAD_DIM), Wf("backend.m_frame_level.%d.weight" % idx, HEAD_DIM), hb["h"][j], M, HEAD_DIM, HEAD_DIM,
                           bias=P.f32("backend.m_frame_level.%d.bias" % idx), act=ACT_LEAKY, c2=hb["pre"][j], drop_p=drop,
                           drop_seed=seeds[j], x3=False)
            drop_descs.append(dsc)
            prev = hb["h"][j]
        if not layout.fixed:
            ops.zero_tail_rows(feats, layout.frames, B, T, HEAD_DIM)
            ops.meanpool_fwd_varlen(prev, emb, layout.frames, B, T, HEAD_DIM)
        else:
            ops.meanpool_fwd(prev, emb, B, T, HEAD_DIM)
        ops.utt_head_fwd(emb, P.f32("backend.m_utt_level.weight"), P.f32("backend.m_utt_level.bias"), logp, B, HEAD_DIM, N_CLASS)
        saved = dict(ectx=ectx, hb=hb, B=B, L=L, T=T, drop=drop, feats=feats, emb=emb, logp=logp, enc_out=enc_out, st=st)
        return saved, drop_descs

    def _run_backward(self, sv, d_logp, d_feats, d_emb):
        P = self.P
        P.rebind_grads()
        st, seeds = sv["st"], sv["seeds"]
        for name, g in (("d_logp", d_logp), ("d_feats", d_feats), ("d_emb", d_emb)):
            if g is None:
                st[name].zero_()
            else:
                st[name].copy_(g)
        if self.grad_sync is not None:
            self.encoder.on_grads_ready = self.grad_sync.ready_above
        use_plan = not sv["ectx"]["skipped"] and self.cfg.encoder_layerdrop == 0
        pk = sv["ectx"]["layout"].plan_key("bwd", sv["drop"] > 0, self.grad_sync is not None)      # the row offsets are the state's, already in place

        def patch(plan):
            plan["drop_descs"][0].drop_seed = seeds[1]
            plan["drop_descs"][1].drop_seed = seeds[0]
            plan["meanpool_entry"][1][plan["meanpool_seed_pos"]] = seeds[2]
            self.encoder.apply_seeds(plan["enc_slots"], sv["ectx"]["step_seed"])
        run_plan(st["plans"], pk, use_plan, patch, lambda: self._backward_kernels(sv, st, seeds))

    def _backward_kernels(self, sv, st, seeds):
        P, E = self.P, self.cfg.embed
        B, T, hb = sv["B"], sv["T"], sv["hb"]
        M = B * T
        W = lambda name, ld: Op(P.bf16, ld, offset=P.off(name))
        ops.utt_head_bwd(st["d_logp"], sv["logp"], sv["emb"], P.f32("backend.m_utt_level.weight"), st["d_emb"], hb["demb"],
                         P.g("backend.m_utt_level.weight"), P.g("backend.m_utt_level.bias"), hb["ws"], B, HEAD_DIM, N_CLASS)
        frames = sv["ectx"]["layout"].frames      # a variable-length training batch: the mean ran over each utterance's own frames
        if frames is not None:
            # the forward zeroed feats beyond them, so whatever the loss hands back there (SupCon's gradient is not 0) stops here
            ops.zero_tail_rows(st["d_feats"], frames, B, T, HEAD_DIM)
            mp_entry = ops.meanpool_bwd_varlen(hb["demb"], hb["pre"][2], hb["dpre"][2], frames, B, T, HEAD_DIM, ACT_LEAKY, sv["drop"], seeds[2])
            mp_pos = ops.MEANPOOL_BWD_VARLEN_SEED
        else:
            mp_entry = ops.meanpool_bwd(hb["demb"], hb["pre"][2], hb["dpre"][2], B, T, HEAD_DIM, ACT_LEAKY, sv["drop"], seeds[2])
            mp_pos = ops.MEANPOOL_BWD_SEED
        drop_descs, enc_slots = [], []
        for j, idx in reversed(list(enumerate((0, 3, 6)))):
            dpre = hb["dpre"][j]
            inp = hb["h"][j - 1] if j > 0 else hb["r0"]
            ops.colsum_reduce(dpre, hb["cs"], P.g("backend.m_frame_level.%d.bias" % idx), M, HEAD_DIM)
            self.encoder._wgrad(sv["ectx"]["d"], Op(dpre, HEAD_DIM), Op(inp, HEAD_DIM), P.g("backend.m_frame_level.%d.weight" % idx),
                                HEAD_DIM, HEAD_DIM, M, **X3_OFF)
            # fp32 master weights on the exact-fp32 GEMM (bf16 working copy when SCL_HEAD_F32=0)
            wj = Op(P.flat if HEAD_F32 else P.bf16, HEAD_DIM, offset=P.off("backend.m_frame_level.%d.weight" % idx))
            if j > 0:
                drop_descs.append(ops.gemm(Op(dpre, HEAD_DIM), wj, hb["dpre"][j - 1], M, HEAD_DIM, HEAD_DIM, b_t=True, R=hb["pre"][j - 1],
                                           rmode=2, ract=ACT_LEAKY, drop_p=sv["drop"], drop_seed=seeds[j - 1], x3=False))
            else:
                ops.gemm(Op(dpre, HEAD_DIM), wj, hb["dfe"], M, HEAD_DIM, HEAD_DIM, b_t=True, R=sv["feats"], rmode=2, ract=ACT_RELU, x3=False)
        # total gradient at feats = ReLU path + SupCon path
        ops.add_f32(hb["dfe"], st["d_feats"], hb["dfe"], hb["dfe_bf"], M * HEAD_DIM)
        ops.colsum_reduce(hb["dfe"], hb["cs"], P.g("LL.bias"), M, HEAD_DIM)
        self.encoder._wgrad(sv["ectx"]["d"], Op(hb["dfe_bf"], HEAD_DIM), Op(sv["enc_out"], E), P.g("LL.weight"), HEAD_DIM, E, M)
        if self.cfg.layer_mix:
            # the mix's logits lie among the head's gradients: final once the encoder backward's first launch has run (after_mix), and a
            # frozen encoder still forms d(mix) for them alone (mix_only); the frozen case announces nothing, as without the mix
            ops.gemm(Op(hb["dfe_bf"], HEAD_DIM), W("LL.weight", E), hb["denc"], M, E, HEAD_DIM, b_t=True)
            ready = None
            if self.grad_sync is not None and not self.flag_fix_ssl:
                ready = lambda: ops.host_callback(self.grad_sync.ready_above, P.off("LL.weight"))
            enc_slots = self.encoder.backward(sv["ectx"], hb["denc"], mix_only=self.flag_fix_ssl, after_mix=ready)
        elif not self.flag_fix_ssl:
            ops.gemm(Op(hb["dfe_bf"], HEAD_DIM), W("LL.weight", E), hb["denc"], M, E, HEAD_DIM, b_t=True)
            if self.grad_sync is not None:      # head gradients (the END of the flat buffer) are final: start their all-reduce
                ops.host_callback(self.grad_sync.ready_above, P.off("LL.weight"))
            enc_slots = self.encoder.backward(sv["ectx"], hb["denc"])
        return dict(drop_descs=drop_descs, meanpool_entry=mp_entry, meanpool_seed_pos=mp_pos, enc_slots=enc_slots)

    def _score_fp32(self, x, layout=FIXED):
        """Scoring forward (no grad, eval mode): fp32 activations, fp32 master weights, exact-fp32 GEMMs end to end — the
        reference's precision (main.py:161-214), for scores / embeddings within 1e-3 of it.
        A packed layout (encoder.SCORE_PACK): the encoder's transformer layers run on the packed valid frames and it hands back the padded
        rectangle, so the head below is the same either way."""
        P, E = self.P, self.cfg.embed
        B = x.shape[0]
        enc, T = self.encoder.forward_f32(x, **layout.args)
        frames = layout.frames
        M = B * T
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
        Wf = lambda name, ld: Op(P.flat, ld, offset=P.off(name))
        feats, h0, h1 = f32(B, T, HEAD_DIM), f32(M, HEAD_DIM), f32(M, HEAD_DIM)
        ops.gemm(Op(enc, E), Wf("LL.weight", E), h0, M, HEAD_DIM, E, bias=P.f32("LL.bias"), act=ACT_RELU, c2=feats)
        for idx in (0, 3, 6):
            ops.gemm(Op(h0, HEAD_DIM), Wf("backend.m_frame_level.%d.weight" % idx, HEAD_DIM), h1, M, HEAD_DIM, HEAD_DIM,
                     bias=P.f32("backend.m_frame_level.%d.bias" % idx), act=ACT_LEAKY)
            h0, h1 = h1, h0
        if frames is not None:      # the utterance's own frames: feats rows beyond them are 0, the mean runs over them alone
            ops.zero_tail_rows(feats, frames, B, T, HEAD_DIM)
            emb = f32(B, HEAD_DIM)
            ops.meanpool_fwd_varlen(h0, emb, frames, B, T, HEAD_DIM)
        else:
            emb = h0.view(B, T, HEAD_DIM).mean(dim=1)
        logp = f32(B, N_CLASS)
        ops.utt_head_fwd(emb.contiguous(), P.f32("backend.m_utt_level.weight"), P.f32("backend.m_utt_level.bias"), logp, B, HEAD_DIM, N_CLASS)
        return logp, feats, emb

    def _forward(self, x, lengths=None):
        if x.dim() == 3:
            x = x[:, :, 0]
        x = x.to(device=self.device, dtype=torch.float32).contiguous()   # main.py:60 hands over a transposed view
        layout = FIXED
        if lengths is not None:
            if torch.is_grad_enabled() != bool(self.training):
                raise NotImplementedError("forward(x, lengths) is a scoring mode on model.eval() under torch.no_grad() and a training "
                                          "mode on model.train() with autograd on; eval with autograd, or train under no_grad, is neither")
            # the packed layout: encoder.VARLEN_PACK serves the bf16 encoder path, encoder.SCORE_PACK the fp32 scoring path (whose
            # materialised-score attention is strided per utterance: packed, it runs the streaming kernel of csrc/attention_f32.hip)
            _, layout = ENC.row_layout(self.cfg, lengths, *x.shape, min_samples=self.min_samples(), refuse_short=False,
                                       score_f32=not self.training and SCORE_FP32, device=self.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in (self._anchor,)):
            out, feats, emb = _ModelFn.apply(self, x, self._anchor, layout)
        elif not self.training and SCORE_FP32:
            out, feats, emb = self._score_fp32(x, layout)
        else:
            out, feats, emb, _ = self._run_forward(x, layout)
            out, feats, emb = out.clone(), feats.clone(), emb.clone()
        if self.is_train:
            return out, feats, emb
        return out

    def forward(self, x_big, lengths=None):
        if not self.is_train:
            print("Inference mode")  # linear_nll:152
        return self._forward(x_big, lengths)

    # loss ------------------------------------------------------------------------------------------
    def loss(self, output, feats, emb, labels, config, info=None):
        return loss_custom(output, feats, emb, labels, config)


_LOSS_SCALE = {}


def _loss_scale(bz, dev):
    """[1, 1/bz, 1/bz] on the device, built once per (batch, device): torch.tensor(..., device=) is a blocking host-to-device copy, and
    one per step in the middle of the forward -> backward hand-over stalled the launch thread until the GPU had caught up."""
    key = (bz, dev.type, dev.index)
    if key not in _LOSS_SCALE:
        _LOSS_SCALE[key] = torch.tensor([1.0, 1.0 / bz, 1.0 / bz], device=dev)
    return _LOSS_SCALE[key]


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, feats, emb, labels):
        dev = output.device
        bz = output.shape[0]
        Tq, dq = feats.shape[1], feats.shape[2]
        res = torch.empty(3, device=dev)
        coef = torch.empty(bz, output.shape[1], device=dev)
        labels = labels.to(torch.int64).contiguous()
        outc, F1, F2 = output.contiguous(), feats.contiguous().view(bz, -1), emb.contiguous()
        ops.nll_fwd(outc, labels, bz, output.shape[1], res[0:1], coef)
        K1, K2 = Tq * dq, emb.shape[1]
        ws = torch.empty(max(ops.supcon_ws_floats(bz, K1), ops.supcon_ws_floats(bz, K2)), device=dev)
        G1, G2 = torch.empty(2 * bz * bz, device=dev), torch.empty(2 * bz * bz, device=dev)      # dL/dS + the backward's scratch
        ops.supcon_fwd(F1, labels, bz, K1, K1, Tq, 0.07, ws, G1, res[1:2])
        ops.supcon_fwd(F2, labels, bz, K2, K2, K2, 0.07, ws, G2, res[2:3])   # emb as [bz,1,128,1]: T' = 128, d = 1
        ctx.save_for_backward(coef, G1, G2, F1, F2)
        ctx.dims = (bz, Tq, dq, K1, K2)
        scale = _loss_scale(bz, dev)   # Model.loss multiplies the SupCon terms by 1/bz
        out = res * scale
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_ce, g_cf1, g_cf2):
        coef, G1, G2, F1, F2 = ctx.saved_tensors
        bz, Tq, dq, K1, K2 = ctx.dims
        dev = coef.device
        d_out = coef * g_ce
        dF1 = torch.empty(bz, K1, device=dev)
        dF2 = torch.empty(bz, K2, device=dev)
        ops.supcon_bwd(F1, G1, g_cf1.contiguous().view(1), 1.0 / bz, bz, K1, K1, Tq, 0.07, dF1)
        ops.supcon_bwd(F2, G2, g_cf2.contiguous().view(1), 1.0 / bz, bz, K2, K2, K2, 0.07, dF2)
        return d_out, dF1.view(bz, Tq, dq), dF2, None


GLOBAL_SUPCON = os.environ.get("SCL_GLOBAL_SUPCON", "0") == "1"


def loss_custom(output, feats, emb, labels, config):
    """model/loss_metrics.py:498-532 / Model.loss: dict of loss terms selected by loss_type.
    SCL_GLOBAL_SUPCON=1 under data parallelism (optional): the loss nn.DataParallel computes (main.py:62-66: Model.loss on
    the outputs of ALL GPUs) — the two SupCon terms see the batch of all ranks (features and labels all-gathered, positives / negatives
    across ranks, 1/bz with the global bz), and the NLL term, a sum over utterances, is the rank's own share of CE_global / bz_global
    (= its local term / world size: averaged over the ranks by the gradient exchange it is the global term).  Default: every term
    rank-local, the reference's semantics at --batch_size 1."""
    L_CE, L_CF1, L_CF2 = _LossFn.apply(output, feats, emb, labels)
    if GLOBAL_SUPCON and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        from .parallel import gather_for_global_loss as gather
        _, L_CF1, L_CF2 = _LossFn.apply(gather(output.detach()), gather(feats), gather(emb), gather(labels))
        L_CE = L_CE / torch.distributed.get_world_size()
    lt = config["model"]["loss_type"]
    # contra_mode 'one' anchors only the first VIEW (loss_metrics.py:155-157); Model.loss hands supcon_loss exactly one view per
    # utterance (feats.unsqueeze(1), wav2vec2_linear_nll.py:176-180), so anchor_feature == contrast_feature and anchor_count == nv == 1:
    # both modes are the same computation here
    if config["model"].get("contra_mode", "all") not in ("all", "one"):
        raise ValueError("Unknown mode: {}".format(config["model"]["contra_mode"]))
    if lt == 1:
        return {"L_CE": L_CE, "L_CF1": L_CF1, "L_CF2": L_CF2}
    if lt == 2:
        return {"L_CE": L_CE, "L_CF1": L_CF1}
    if lt == 3:
        return {"L_CE": L_CE, "L_CF2": L_CF2}
    if lt == 4:
        return {"L_CE": L_CE}
    if lt == 5:
        return {"L_CF1": L_CF1, "L_CF2": L_CF2}
    return None
