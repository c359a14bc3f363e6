"""`wav2vec2_btse` model plugin — host-side mirror of model/wav2vec2_btse/model.py::Model (BASELINE.json configs[4]).

    Model(args: the YAML `model:` block of conf-5-btse-trans64.yaml, device, is_train=True)
    forward(x [bz, L], bio=None, bio_lengths=None, y=None, lengths=None) -> (log_probs [bz, 2], ssl_feat [bz, T, 128], b [bz, 128 + bio_out])
                                                              (log_probs only when not is_train)          (model.py:321-343)
    loss(output, feats, emb, labels, config, info=None) -> dict of 0-d tensors

What the plugin IS in the reference (not a Conformer): XLS-R -> LL 1024 -> 128 -> a 3-layer MLP, mean over time (backend.py:17-47,
linear.py:5-67) joined with a 3-layer relative-position transformer over "bio" tokens (model.py:210-238, transformer.py) -> fc2 ->
log_softmax.  State-dict keys equal the reference's: backend.ssl_model.model.<fairseq keys>, backend.LL.*, backend.mlp.m_frame_level.linear_{0,1,2}.*,
backend.mlp.m_utt_level.*, bioScoring.bio_embedding.weight, bioScoring.encoder.{attn_layers,norm_layers_1,ffn_layers,norm_layers_2}.<i>.*,
bioScoring.bio_scoring.*, [fc1.*,] fc2.*  (tests/test_btse_gpu.py compares them with the key list of the reference's own Model).

Two things the reference does not hold, and what this plugin does about them:
  * the TOKENISER.  model.py:306-319 calls `Wav2bioCNN.wav2bio` from a `biosegment` package that is a dangling symlink in the reference;
    `forward` takes the bio tokens as an argument (model.py:321), and that is the supported way in.  Without them, a tokeniser named by
    the optional YAML key `bio_tokenizer: "<module>:<callable>"` (signature (waveforms [bz, L] numpy, sample_rate) -> list of equal-length
    int sequences, as get_Bio expects) is called; with neither, forward raises.
  * `loss`.  model.py:345-375 reads self.loss_CE / self.contra_mode / self.sim_metric_seq, none of which is ever set: it cannot run.  This
    plugin uses the linear plugin's loss (model/wav2vec2_linear_nll.py:158-192), which is what that code was copied from.
The MLP's own logits (m_utt_level) are computed and dropped by the reference (model.py:324): here they are not computed, and the two
tensors sit behind the trainable range so that AdamW leaves them untouched exactly as torch.optim.AdamW skips a parameter without .grad.
The SSL encoder always runs in train mode (backend.py:29,39: the back-end's own `is_train` stays True whatever the outer flag says).

Variable-length batches: forward(x, lengths=[n_b]) takes whole utterances of different lengths, zero-padded to [bz, L] — scoring (eval mode
under torch.no_grad(), either scoring precision) and training (train mode with autograd on).  Row b's outputs and its share of every
gradient are what the plugin computes for that utterance alone at its own length with its own tokens: the encoder runs under its padding
mask (or on packed rows), the mean over time of the frame-level MLP runs over its T_b frames, rows of feats and d(feats) beyond T_b are zero,
and the bio score is read at its OWN last token k_b - 1 — not, as model.py:234-236 has it for fixed-length batches and as this plugin keeps
it without `lengths`, at the last padded position, which would leave every row shorter than the longest with a zero bio score
(btse_head.py).  Tokens: bio [bz, Lt] padded with any valid id and bio_lengths = the own counts k_b (1..Lt on the host); without explicit
tokens the tokeniser is called once per utterance on x[b:b+1, :n_b] and the rows are padded with token 0 to the longest.  Limits: 400
samples at least (one frame), 1..512 tokens per utterance (the fused bio kernel).  main.py routes --eval --padding_type none here;
main.py training with --padding_type zero --batch_size k is not routed (forward(x, lengths=...) in train mode is the training interface).
"""
import importlib

import numpy as np
import torch

from .btse_head import BtseHead
from .model_front import FrontHeadModel
from .model_linear import dropout_stream_seed, loss_custom


def pad_token_rows(rows):
    """Ragged token rows (one sequence per utterance) -> (bio [bz, longest] int32 with token 0 as filler, the own counts [bz] int32)."""
    lens = [len(r) for r in rows]
    bio = np.zeros((len(rows), max(lens + [1])), dtype=np.int32)
    for b, r in enumerate(rows):
        bio[b, :lens[b]] = np.asarray(r, dtype=np.int32)
    return torch.from_numpy(bio), torch.tensor(lens, dtype=torch.int32)


class Model(FrontHeadModel):
    front_prefix = "backend."
    head_takes_frames = True       # BtseHead masks the mean over time and reads the bio score at the utterance's own last token
    head_trains_frames = True      # ... with a masked backward

    def __init__(self, args, device, is_train=True, w2v_cfg=None, seed=0, rank=0):
        super().__init__(args, device, is_train=is_train, w2v_cfg=w2v_cfg, seed=seed, rank=rank)
        self.is_add = bool(self.btse_args["is_add"])
        self.use_graphs = False          # the head is one hand-scheduled autograd node already
        BtseHead.reseed(self, dropout_stream_seed(seed, rank) ^ 0x2B7E15)      # MLP dropout masks follow --seed and the data-parallel rank
        self.bio_tokenizer = None
        spec = args.get("bio_tokenizer") if hasattr(args, "get") else None
        if spec:
            mod, fn = spec.split(":")
            self.bio_tokenizer = getattr(importlib.import_module(mod), fn)

    def _build_head(self, args):
        head = BtseHead(args)
        self.btse_args = head.btse_args
        return head

    @staticmethod
    def _head_forward(mod, feats, frames=None):
        return BtseHead.forward(mod, feats, frames=frames)

    def _ssl_train(self):
        return True      # backend.py:29,39 -> xlsr.py:30-31: self.model.train() on every call

    def get_Bio(self, X_pad, fs):
        """model.py:306-319, with the absent Wav2bioCNN replaced by the configured callable."""
        if self.bio_tokenizer is None:
            raise RuntimeError("wav2vec2_btse: forward() needs bio tokens (bio, bio_lengths): the reference's tokeniser package "
                               "`model/wav2vec2_btse/biosegment` is absent from the reference itself; pass the tokens, or name a "
                               "tokeniser with the YAML key model.bio_tokenizer = '<module>:<callable>'")
        toks = self.bio_tokenizer(X_pad.detach().cpu().numpy(), fs)
        lens = torch.tensor([len(t) for t in toks], dtype=torch.int32)
        return torch.from_numpy(np.asarray(toks, dtype=np.int32)), lens          # ragged lists fail here, as torch.IntTensor(bio) does

    def get_bio_own(self, X_pad, lengths, fs):
        """The tokens of a variable-length batch: the tokeniser runs once per utterance on its own samples x[b:b+1, :n_b]; the rows may
        differ in length and are padded with token 0, bio_lengths are the own counts."""
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lengths) != X_pad.shape[0] or any(n < 1 or n > X_pad.shape[1] for n in lengths):
            raise ValueError("lengths: need one sample count in 1..%d per row of the %r batch, got %r" % (X_pad.shape[1], tuple(X_pad.shape), lengths))
        rows = []
        for b, n in enumerate(lengths):
            toks, _ = self.get_Bio(X_pad[b:b + 1, :n], fs)
            rows.append(toks[0].tolist())
        return pad_token_rows(rows)

    def forward(self, x, bio=None, bio_lengths=None, y=None, lengths=None):
        if bio is None:
            xs = x if x.dim() == 2 else x[:, :, 0]
            bio, bio_lengths = self.get_Bio(xs, 16000) if lengths is None else self.get_bio_own(xs, lengths, 16000)
        self.__dict__["_bio"] = (bio, bio_lengths)
        try:
            return super().forward(x, lengths)
        finally:
            self.__dict__["_bio"] = None

    def loss(self, output, feats, emb, labels, config, info=None):
        return loss_custom(output, feats, emb, labels, config)
