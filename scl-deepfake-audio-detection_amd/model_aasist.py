"""`wav2vec2_aasist` model plugin — host-side mirror of model/wav2vec2_aasist.py::Model.

    Model(args: dict with an `aasist` section, device, is_train=True)
    forward(x [bz, L]) -> (logits [bz, 2], feats [bz, T, 128], last_hidden [bz, 160])   (logits only when not is_train)
    forward(x, lengths=[n_0, ...])   SCL_AASIST_LENGTHS=1 (read at call time; without it the call is refused as before): scoring mode (eval, no
                                     grad): row b holds n_b samples (min_samples() .. max_samples()) followed by padding and gets the result it
                                     gets alone at its own length; feats rows beyond an utterance's frames are 0
    forward(x, lengths=[n_0, ...])   SCL_AASIST_TRAIN_LENGTHS=1 (read at call time), model.train() with autograd on: training on a zero-padded
                                     batch - AasistHead.forward_frames_train, the per-layer composition with batch statistics over the
                                     batch's own positions, at every length up to aasist_long.MAX_FRAMES frames and eagerly even under
                                     SCL_HEAD_GRAPH=1.  Batch statistics couple the rows: a row is what the utterance gets in this batch.
                                     Without the switch every call behaves as before, the scoring-mode refusals included
    loss(output, feats, emb, labels, config, info=None) -> dict of 0-d tensors

Encoder + LL + losses: HIP kernels; graph back-end: `aasist_head.AasistHead` on flat-buffer parameter views, replayed as
hipGraphs in training (scl_amd/model_front.py).

The reference's train-mode forward returns a 2-tuple while main.py:63 unpacks three values: this plugin
returns the triple main.py and Model.loss need — feats is the LL output, exactly what the linear plugin hands to SupCon.
"""
import os

import torch

from . import aasist_head
from .aasist_head import UPSTREAM_AASIST, AasistHead
from .model_front import FrontHeadModel
from .model_linear import dropout_stream_seed, loss_custom


class Model(FrontHeadModel):
    def __init__(self, args, device, is_train=True, w2v_cfg=None, seed=0, rank=0):
        super().__init__(args, device, is_train=is_train, w2v_cfg=w2v_cfg, seed=seed, rank=rank)
        # the fused graph module draws its dropout masks (input_drop, GraphPool, drop_way, read-out) from a counter-hash stream:
        # start it from --seed and the data-parallel rank, like the encoder's (model_front.py)
        from . import graph
        graph.seed(dropout_stream_seed(seed, rank) ^ 0x3C6EF372)

    def _build_head(self, args):
        head = AasistHead(args.get("aasist") or UPSTREAM_AASIST)
        self.__dict__["pool_cfg"] = head.pool_cfg
        return head

    LENGTHS_SWITCH = "SCL_AASIST_LENGTHS"

    @staticmethod
    def _lengths_mode():
        """SCL_AASIST_LENGTHS, read at call time: "1" (the fused kernels, up to 242 frames), "long" (beyond them the per-layer composition
        with count tables, up to 3074 frames) or off."""
        v = os.environ.get(Model.LENGTHS_SWITCH, "0")
        return v if v in ("1", "long") else "0"

    TRAIN_LENGTHS_SWITCH = "SCL_AASIST_TRAIN_LENGTHS"

    @staticmethod
    def _train_lengths():
        """SCL_AASIST_TRAIN_LENGTHS=1, read at call time: forward(x, lengths) in train mode with autograd on."""
        return os.environ.get(Model.TRAIN_LENGTHS_SWITCH, "0") == "1"

    @staticmethod
    def _head_forward(mod, feats, frames=None):
        if frames is None:
            return AasistHead.forward(mod, feats)
        if mod.training and torch.is_grad_enabled() and Model._train_lengths():
            return AasistHead.forward_frames_train(mod, feats, frames)
        # long: a batch whose longest utterance fits the fused kernels takes them (the bits of SCL_AASIST_LENGTHS=1); any longer one goes whole
        if Model._lengths_mode() == "long" and max(int(t) for t in frames) > aasist_head.max_frames(mod.pool_cfg):
            return AasistHead.forward_frames_long(mod, feats, frames)
        return AasistHead.forward_frames(mod, feats, frames)

    @property
    def head_takes_frames(self):
        """forward(x, lengths) is opt-in for this plugin: SCL_AASIST_LENGTHS=1 or =long, read at call time."""
        return self._lengths_mode() != "0" or self._training_with_lengths()

    @property
    def head_trains_frames(self):
        """... and in train mode with autograd on behind SCL_AASIST_TRAIN_LENGTHS=1."""
        return self._train_lengths()

    def _training_with_lengths(self):
        return self._train_lengths() and torch.is_grad_enabled() and bool(self.training)      # the switch first: off, nothing else is read

    def head_min_frames(self):
        return aasist_head.min_frames()

    def head_max_frames(self):
        if self._lengths_mode() == "long" or self._training_with_lengths():
            from . import aasist_long
            return aasist_long.MAX_FRAMES
        return aasist_head.max_frames(self.pool_cfg)

    def forward(self, x, lengths=None):
        if lengths is not None and self._training_with_lengths():
            from . import aasist_long
            if not aasist_long.widths_supported(self):      # the training path is the per-layer composition at every length
                raise NotImplementedError("wav2vec2_aasist: training with lengths needs graph-attention widths among %r" % (aasist_long.GAT_WIDTHS,))
        elif lengths is not None and self._lengths_mode() == "long" and max(int(n) for n in lengths) > self.cfg.samples_for(aasist_head.max_frames(self.pool_cfg) + 1) - 1:
            from . import aasist_long
            if not aasist_long.widths_supported(self):      # the long path does not depend on SCL_AASIST_FUSED / SCL_AASIST_FUSED_GRAPH
                raise NotImplementedError("wav2vec2_aasist: forward(x, lengths) beyond %d frames needs graph-attention widths among %r"
                                          % (aasist_head.max_frames(self.pool_cfg), aasist_long.GAT_WIDTHS))
        elif lengths is not None and self.head_takes_frames and not AasistHead.frames_supported(self):
            raise NotImplementedError("wav2vec2_aasist: forward(x, lengths) runs on the fused stack and graph kernels only: this configuration's "
                                      "shapes are not theirs, or SCL_AASIST_FUSED=0 is set")
        return super().forward(x, lengths)

    # aasist.py:33-52: the SSL model simply follows the parent's train / eval mode (FrontHeadModel._ssl_train default)

    def loss(self, output, feats, emb, labels, config, info=None):
        # aasist.py:607-640: unweighted CrossEntropy on raw logits (the NLL kernel folds the log-softmax), SupCon over the
        # frame features and over last_hidden viewed as [bz, 1, 160, 1]
        return loss_custom(output, feats, emb, labels, config)
