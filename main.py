#!/usr/bin/env python
"""Training / scoring driver on the MI355X hot path — drop-in for the reference's main.py
(same flags main.py:217-298, same plugin resolution :325-333, same score-file formats :178/:212,
same checkpoint naming :310-318,44-45), so `02_train.sh` / `03_eval.sh` keep working.

What is different underneath:
  * model, losses, backward and AdamW run in the HIP kernels of libscl_hip.so; augmentation runs on the
    GPU inside the dataset, so the loaders use no worker processes;
  * loss terms are accumulated on the device and read back once per epoch instead of 3-4 `.item()`
    host syncs per step (main.py:71,73,76) — the epoch sums are the same numbers;
  * multi-GPU = one process per GPU (`python -m torch.distributed.run --nproc-per-node N main.py ...`):
    packs are sharded rank-strided, gradients all-reduced over RCCL/xGMI overlapped with backward
    (the reference's nn.DataParallel training path cannot run).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import yaml
from torch.utils.data import DataLoader, Subset

from model.wav2vec2_aasist import Model as wav2vec2_aasist
from model.wav2vec2_linear_nll import Model as wav2vec2_linear_nll
from model.wav2vec2_resnet_nll import Model as wav2vec2_resnet_nll
from model.wav2vec2_btse import wav2vec2_btse

MODEL_REGISTRY = {"wav2vec2_linear_nll": wav2vec2_linear_nll, "wav2vec2_aasist": wav2vec2_aasist, "wav2vec2_resnet_nll": wav2vec2_resnet_nll,
                  "wav2vec2_btse": wav2vec2_btse}
VARLEN_MODELS = ("wav2vec2_linear_nll", "wav2vec2_resnet_nll")      # --padding_type none / zero with --batch_size k: the plugins whose forward takes `lengths`
# --padding_type none alone (scoring, never --padding_type zero --batch_size k training): plugin -> the environment switch that turns its
# scoring mode with lengths on, read when main() runs
VARLEN_SCORING_OPT_IN = {"wav2vec2_aasist": "SCL_AASIST_LENGTHS"}
# --padding_type none with no switch, and likewise never routed into --padding_type zero --batch_size k training: the plugin's own
# forward(x, lengths=...) in train mode is its training interface (the tokeniser runs per utterance)
VARLEN_SCORING_MODELS = ("wav2vec2_btse",)
# --padding_type zero --batch_size k TRAINING by opt-in: plugin -> the environment switch that turns its training mode with lengths on.  The
# packs are zero-padded and masked only when that switch AND the plugin's scoring switch (VARLEN_SCORING_OPT_IN: validation scores under the
# mask) are set, read when main() runs; with neither the plugin keeps its behaviour, with only one main() exits at start-up naming both
VARLEN_TRAIN_OPT_IN = {"wav2vec2_aasist": "SCL_AASIST_TRAIN_LENGTHS"}


def _scores_varlen(name):
    return name in VARLEN_MODELS or name in VARLEN_SCORING_MODELS or os.environ.get(VARLEN_SCORING_OPT_IN.get(name, ""), "0") in ("1", "long")


def _train_opt_in(name):
    """(training switch set, scoring switch set) of a VARLEN_TRAIN_OPT_IN plugin; (False, False) for every other model."""
    if name not in VARLEN_TRAIN_OPT_IN:
        return False, False
    return os.environ.get(VARLEN_TRAIN_OPT_IN[name], "0") == "1", os.environ.get(VARLEN_SCORING_OPT_IN[name], "0") in ("1", "long")


def _trains_varlen(name):
    return name in VARLEN_MODELS or all(_train_opt_in(name))


class EarlyStop:
    """Patience on validation accuracy; saves state_dict when it improves (reference main.py:23-45)."""

    def __init__(self, patience=5, delta=0, init_best=60, save_dir="", is_main=True):
        self.patience, self.delta, self.best_score, self.save_dir = patience, delta, init_best, save_dir
        self.counter, self.early_stop, self.is_main = 0, False, is_main

    def __call__(self, score, model, epoch):
        if self.best_score is None:
            self.best_score = score
        elif score < self.best_score + self.delta:
            self.counter += 1
            self.early_stop = self.counter >= self.patience
        else:
            print("Best epoch: {}".format(epoch))
            self.best_score, self.counter = score, 0
            if self.is_main:
                torch.save(model.state_dict(), os.path.join(self.save_dir, "epoch_{}.pth".format(epoch)))


class ScalarLog:
    """tensorboardX.SummaryWriter when installed, else one JSON line per scalar under logs/<tag>/scalars.jsonl."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        try:
            from tensorboardX import SummaryWriter
            self.tb, self.f = SummaryWriter(logdir), None
        except ImportError:
            self.tb, self.f = None, open(os.path.join(logdir, "scalars.jsonl"), "a")

    def add_scalar(self, name, value, step):
        if self.tb is not None:
            self.tb.add_scalar(name, value, step)
        else:
            self.f.write(json.dumps({"tag": name, "value": float(value), "step": int(step)}) + "\n")
            self.f.flush()


def _as_model_input(batch_x, device):
    """[1, L, V] pack -> [V, L]; [bz, L] batch stays (reference main.py:57-63).  Returns (x, n_utts, n_packs).
    Extension over the reference (whose reshape only works for --batch_size 1): [k, L, V] with k > 1 packs becomes [k*V, L] —
    the encoder sees one k*V batch (k = 3 packs of 11 views run at 935 instead of 507 utterances/s on one MI355X), the loss is
    still computed pack by pack and summed, i.e. one optimizer step on the summed gradient of k packs."""
    batch_x = batch_x.to(device)
    if batch_x.dim() == 3:
        k, L, V = batch_x.shape
        return batch_x.permute(0, 2, 1).reshape(k * V, L), k * V, k
    return batch_x, batch_x.shape[0], 1


def run_epoch(loader, model, optimizer, device, config, train):
    model.train(train)
    sums, total_sum, correct, n_total = {}, torch.zeros((), device=device), torch.zeros((), device=device), 0.0
    ctx = torch.enable_grad() if train else torch.no_grad()
    with ctx:
        for batch in loader:
            info, batch_x, batch_y = batch[:3]
            x, n, n_packs = _as_model_input(batch_x, device)
            n_total += n
            y = batch_y.view(-1).type(torch.int64).to(device)
            if len(batch) > 3:      # zero-padded packs (PackDataset pad_to_trim): [k, V] sample counts -> one per row of the [k*V, L] batch
                out, feat, emb = model(x, lengths=batch[3].reshape(-1).tolist())
            else:
                out, feat, emb = model(x)
            step_loss = None
            V = n // n_packs
            for pk in range(n_packs):        # SupCon positives / negatives stay inside a pack, as with --batch_size 1
                sl = slice(pk * V, (pk + 1) * V)
                losses = model.loss(out[sl], feat[sl], emb[sl], y[sl], config, info) if n_packs > 1 else \
                    model.loss(out, feat, emb, y, config, info)
                for k, v in losses.items():
                    step_loss = v if step_loss is None else step_loss + v
                    sums[k] = sums.get(k, 0) + v.detach()
            total_sum += step_loss.detach()
            correct += (out.argmax(dim=1) == y).sum()
            if train:
                optimizer.zero_grad()
                if getattr(optimizer, "grad_sync", None) is not None:
                    optimizer.grad_sync.begin()
                step_loss.backward()
                optimizer.step()
    # one host sync per epoch.  Data-parallel validation: the shards differ in size (drop_last=False), so the sums — not the per-rank
    # ratios — are all-reduced: accuracy and losses are the same global numbers a single-GPU run logs
    if not train and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        keys = sorted(sums)
        t = torch.stack([total_sum, correct, torch.tensor(float(n_total), device=device)] + [sums[k].float() for k in keys])
        torch.distributed.all_reduce(t)
        total_sum, correct, n_total = t[0], t[1], float(t[2])
        sums = {k: t[3 + i] for i, k in enumerate(keys)}
    detail = {k: float(v) for k, v in sums.items()}
    return float(total_sum), float(correct) / max(n_total, 1.0) * 100.0, detail


def _score_loop(dataset, model, device, batch_size, fn, workers=None):
    """Scoring loop of produce_evaluation_file / _prediction_file / _emb_file (reference main.py:120-214: a DataLoader over Dataset_for_eval).
    Round 6: the reference decodes on DataLoader workers; here a thread pool decodes and pads the files (the FLAC decoder is C behind ctypes:
    no GIL), batches are assembled in pinned memory and uploaded asynchronously, and `fn` — which reads results back to the host — runs for
    batch i - 1 AFTER batch i has been launched, so the GPU never waits for a file or for the host's result formatting.
    Order of `fn` calls and of the lines they write = protocol order, as before.  SCL_EVAL_THREADS=1: the plain loop."""
    from concurrent.futures import ThreadPoolExecutor
    from collections import deque
    if workers is None:
        workers = max(1, int(os.environ.get("SCL_EVAL_THREADS", "8")))
    model.eval()
    if getattr(getattr(dataset, "dataset", dataset), "padding_type", None) == "none":      # the dataset itself, or the Subset of a rank
        return _score_loop_varlen(dataset, model, device, batch_size, fn, workers)
    n = len(dataset)
    if workers <= 1 or n == 0:
        loader = DataLoader(dataset, batch_size, shuffle=False, drop_last=False)
        with torch.no_grad():
            for batch_x, utt_id in loader:
                fn(model(batch_x.to(device)), list(utt_id))
        return
    use_gpu = torch.device(device).type == "cuda"
    ahead = max(4 * batch_size, 4 * workers)            # items decoded or being decoded beyond the batch in flight
    old_switch = sys.getswitchinterval()
    sys.setswitchinterval(min(old_switch, 5e-4))        # the launch thread shares the interpreter lock with the decoders (scl_amd/prefetch.py)
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="scl-eval") as pool, torch.no_grad():
        futs = deque()
        nxt = 0

        def top_up():
            nonlocal nxt
            while nxt < n and len(futs) < ahead:
                futs.append(pool.submit(dataset.__getitem__, nxt))
                nxt += 1
        direct = hasattr(dataset, "load_into") and hasattr(dataset, "cut")      # scl_amd.pack.EvalDataset: decode straight into the batch's pinned rows
        if not direct:
            top_up()
        pending = None                                   # (host copies of the previous batch's results, their event, its ids)

        def to_host(res):
            # results -> pinned host tensors by an ASYNCHRONOUS copy queued right behind the batch's own kernels.  (A `.cpu()` inside
            # `fn` is a blocking copy that is ordered behind everything queued so far — i.e. behind the NEXT batch's forward: the
            # host then sat out every forward and assembled the following batch with the GPU idle: 70 instead of 44 ms per batch.)
            def one(t):
                if not (torch.is_tensor(t) and t.is_cuda):
                    return t
                h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
                return h
            out = tuple(one(t) for t in res) if isinstance(res, (tuple, list)) else one(res)
            ev = torch.cuda.Event() if use_gpu else None
            if ev is not None:
                ev.record()
            return out, ev
        if direct:
            batches = deque()

            def submit_batch():
                nonlocal nxt
                cnt = min(batch_size, n - nxt)
                host = torch.empty((cnt, dataset.cut), dtype=torch.float32, pin_memory=use_gpu)
                hv = host.numpy()
                fs = [pool.submit(dataset.load_into, nxt + j, hv[j]) for j in range(cnt)]
                nxt += cnt
                batches.append((host, fs))
            while nxt < n and len(batches) < 4:          # three batches being decoded beyond the one in flight
                submit_batch()
        while (batches if direct else futs):
            if direct:
                host, fs = batches.popleft()
                ids = [f.result() for f in fs]
                if nxt < n:
                    submit_batch()
            else:
                items = [futs.popleft().result() for _ in range(min(batch_size, len(futs)))]
                top_up()
                xs, ids = [it[0] for it in items], [it[1] for it in items]
                host = torch.empty((len(xs),) + tuple(xs[0].shape), dtype=xs[0].dtype, pin_memory=use_gpu)
                torch.stack(xs, out=host)
            res, ev = to_host(model(host.to(device, non_blocking=True)))
            if pending is not None:
                if pending[1] is not None:
                    pending[1].synchronize()             # batch i - 1's copy: done long ago, batch i is what the GPU works on now
                fn(pending[0], pending[2])
            pending = (res, ev, ids)
        if pending is not None:
            if pending[1] is not None:
                pending[1].synchronize()
            fn(pending[0], pending[2])
    sys.setswitchinterval(old_switch)


def _score_loop_varlen(dataset, model, device, batch_size, fn, workers):
    """--padding_type none: every utterance at its own length.  The list is walked in windows of VARLEN_WINDOW * batch_size utterances; the
    thread pool decodes window i + 1 while window i is scored.  A decoded window is cut into length-sorted batches
    (scl_amd.pack.plan_varlen_batches), each batch goes to the model as a zero-padded pinned [count, Lpad] tensor plus its sample
    counts, results come back by asynchronous copies, and once a window is complete its rows are handed to `fn` in protocol order — after
    the NEXT window's batches have been launched, so the GPU does not wait for the host's formatting.  `fn` receives what the model
    returns with rows for the whole window: the log-probs, or (log-probs, None, emb) (no emitter reads feats)."""
    from concurrent.futures import ThreadPoolExecutor
    from scl_amd.pack import VARLEN_MAX_SAMPLES, VARLEN_WINDOW, plan_varlen_batches
    inner = getattr(dataset, "dataset", dataset)
    n = len(dataset)
    use_gpu = torch.device(device).type == "cuda"
    win = VARLEN_WINDOW * max(1, batch_size)
    starts = list(range(0, n, win))
    pending = None      # the previous window: ([(indices, results on the host)] per batch, last copy's event, ids, first index)

    def emit(batches, ev, ids, w0):
        if ev is not None:
            ev.synchronize()
        cnt = len(ids)
        tup = isinstance(batches[0][1], tuple)
        logp = torch.empty(cnt, batches[0][1][0].shape[1] if tup else batches[0][1].shape[1])
        emb = torch.empty(cnt, batches[0][1][2].shape[1]) if tup else None
        for idx, res in batches:
            rows = torch.tensor([i - w0 for i in idx])
            logp[rows] = res[0] if tup else res
            if tup:
                emb[rows] = res[2]
        fn((logp, None, emb) if tup else logp, ids)

    with ThreadPoolExecutor(max_workers=max(1, workers), thread_name_prefix="scl-eval") as pool, torch.no_grad():
        submit = lambda w0: [pool.submit(dataset.__getitem__, i) for i in range(w0, min(w0 + win, n))]
        futs = submit(starts[0]) if starts else []
        for wi, w0 in enumerate(starts):
            items = [f.result() for f in futs]
            futs = submit(starts[wi + 1]) if wi + 1 < len(starts) else []
            xs, ids = [it[0] for it in items], [it[1] for it in items]
            done, ev = [], None
            for idx, lpad in plan_varlen_batches([int(x.shape[0]) for x in xs], batch_size):
                host = torch.zeros((len(idx), lpad), dtype=torch.float32, pin_memory=use_gpu)
                lens = []
                for r, i in enumerate(idx):
                    host[r, : xs[i].shape[0]] = xs[i]
                    lens.append(int(xs[i].shape[0]))
                res = model(host.to(device, non_blocking=True), lengths=lens)
                keep = lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=use_gpu).copy_(t, non_blocking=True)
                res = (keep(res[0]), None, keep(res[2])) if isinstance(res, (tuple, list)) else keep(res)
                if use_gpu:
                    ev = torch.cuda.Event()
                    ev.record()
                done.append(([w0 + i for i in idx], res))
            if pending is not None:
                emit(*pending)
            pending = (done, ev, ids, w0)
        if pending is not None:
            emit(*pending)
    print("variable-length scoring: %d utterances, %d cut to %d samples"
          % (n, getattr(inner, "n_cut", 0), getattr(inner, "max_samples", VARLEN_MAX_SAMPLES)))


def produce_evaluation_file(dataset, model, device, save_path, batch_size=10):
    """'<utt> <logp0> <logp1>' per line (reference main.py:161-180)."""
    def emit(res, ids):
        scores = res[0].cpu().numpy().tolist()
        with open(save_path, "a+") as fh:
            for f, cm in zip(ids, scores):
                fh.write("{} {} {}\n".format(f, cm[0], cm[1]))
    _score_loop(dataset, model, device, batch_size, emit)
    print("Scores saved to {}".format(save_path))


def produce_prediction_file(dataset, model, device, save_path, batch_size=10):
    """'<utt> <logp1> <argmax>' per line, model.is_train = False (reference main.py:182-214)."""
    model.is_train = False

    def emit(out, ids):
        score = out[:, 1].cpu().numpy().ravel().tolist()
        pred = out.argmax(dim=1).tolist()
        with open(save_path, "a+") as fh:
            for f, cm, p in zip(ids, score, pred):
                fh.write("{} {} {}\n".format(f, cm, p))
    _score_loop(dataset, model, device, batch_size, emit)
    print("Scores saved to {}".format(save_path))


def produce_emb_file(dataset, model, device, save_path, batch_size=10, scores_name="scores.txt"):
    """<save_path>/<utt>.npy embeddings + scores.txt (reference main.py:120-159)."""
    model.is_train = True
    os.makedirs(save_path, exist_ok=True)

    def emit(res, ids):
        out, _, emb = res
        for f, e in zip(ids, emb):
            np.save(os.path.join(save_path, f.split("/")[-1].split(".")[0]), e.cpu().numpy())
        with open(os.path.join(save_path, scores_name), "a+") as fh:
            for f, cm in zip(ids, out.cpu().numpy().tolist()):
                fh.write("{} {} {}\n".format(f, cm[0], cm[1]))
    _score_loop(dataset, model, device, batch_size, emit)
    print("Scores saved to {}".format(save_path))


def merge_rank_outputs(path, world, n_items):
    """Rank r scored items r, r + world, ...: interleave the shards back into protocol order and drop them."""
    shards = []
    for r in range(world):
        with open("%s.rank%d" % (path, r)) as fh:
            shards.append(fh.read().splitlines())
        want = len(range(r, n_items, world))
        if len(shards[r]) != want:      # a shard of an aborted run that was appended to, or a rank that died: never merge it silently
            raise RuntimeError("%s.rank%d holds %d lines, expected %d" % (path, r, len(shards[r]), want))
    with open(path, "a+") as out:
        for i in range(n_items):
            out.write(shards[i % world][i // world] + "\n")
    for r in range(world):
        os.remove("%s.rank%d" % (path, r))
    print("Scores of %d ranks merged into %s" % (world, path))


def build_parser():
    p = argparse.ArgumentParser(description="SCL deepfake-audio detection on MI355X")
    p.add_argument("--database_path", type=str, default="/your/path/to/data/")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--num_epochs", type=int, default=100)
    p.add_argument("--start_epoch", type=int, default=0)
    p.add_argument("--min_lr", type=float, default=0.00000001)
    p.add_argument("--max_lr", type=float, default=0.00001)
    p.add_argument("--weight_decay", type=float, default=0.0001)
    p.add_argument("--loss", type=str, default="weighted_CCE")
    p.add_argument("--config", type=str, default="configs/config.yaml")
    p.add_argument("--padding_type", type=str, default="zero",
                   help="zero or repeat: cut / pad every clip to its fixed length; none (--eval only): score every utterance at its own length")
    p.add_argument("--is_train", type=bool, default=True)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--model_path", type=str, default=None)
    p.add_argument("--comment", type=str, default=None)
    p.add_argument("--eval_output", type=str, default=None)
    p.add_argument("--eval", action="store_true", default=False)
    p.add_argument("--predict", action="store_true", default=False)
    p.add_argument("--emb", action="store_true", default=False)
    # RawBoost hyper-parameters (names and defaults of the reference CLI)
    p.add_argument("--algo", type=int, default=5)
    for name, default in (("nBands", 5), ("minF", 20), ("maxF", 8000), ("minBW", 100), ("maxBW", 1000), ("minCoeff", 10),
                          ("maxCoeff", 100), ("minG", 0), ("maxG", 0), ("minBiasLinNonLin", 5), ("maxBiasLinNonLin", 20),
                          ("N_f", 5), ("P", 10), ("g_sd", 2), ("SNRmin", 10), ("SNRmax", 40)):
        p.add_argument("--" + name, type=int, default=default)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.padding_type == "none" and not args.eval:
        sys.exit("main.py: --padding_type none scores whole utterances and needs --eval (alone or with --predict / --emb); "
                 "training packs clips of one fixed length: use zero or repeat")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("SCL_RCCL_CHANNELS"):      # opt-in cap on RCCL's persistent blocks (no multi-GPU A/B backs a default)
            os.environ.setdefault("NCCL_MAX_NCHANNELS", os.environ["SCL_RCCL_CHANNELS"])
        torch.distributed.init_process_group("nccl")
    os.makedirs("out", exist_ok=True)
    torch.manual_seed(args.seed)
    model_tag = "model_{}_{}_{}_{}".format(args.loss, args.num_epochs, args.batch_size, args.min_lr)
    if args.comment:
        model_tag += "_{}".format(args.comment)
    model_save_path = os.path.join("out", model_tag)
    os.makedirs(model_save_path, exist_ok=True)
    if not torch.cuda.is_available():
        sys.exit("main.py needs an MI355X: the product path has no CPU fallback (use the oracle/ for CPU experiments)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    args.device = str(device)
    print("Number of GPUs available: ", torch.cuda.device_count(), "| processes:", world)

    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    data_mod = importlib.import_module("datautils." + config["data"]["name"])
    genList, Dataset_for, Dataset_for_eval = data_mod.genList, data_mod.Dataset_for, data_mod.Dataset_for_eval
    # --seed initialises the weights (02_train.sh: "random seed to initialize the weight") and, with the rank, the dropout stream
    if config["model"]["name"] == "wav2vec2_btse" and not config["model"].get("bio_tokenizer"):
        # run_epoch / the scoring loops call model(x) as the reference's train_epoch does (main.py:60): the plugin then needs its tokeniser,
        # and the reference's own (model/wav2vec2_btse/biosegment) is a dangling symlink.  Say so now, not at the first forward.
        sys.exit("main.py: model wav2vec2_btse needs the YAML key model.bio_tokenizer = '<module>:<callable>' (waveforms [bz, L] numpy, "
                 "sample_rate) -> equal-length token rows; the reference's biosegment package does not exist, so %s cannot run as shipped "
                 "(scl_amd/model_btse.py; bench.py --model wav2vec2_btse feeds synthetic tokens)" % args.config)
    if args.padding_type == "none" and not _scores_varlen(config["model"]["name"]):
        switch = VARLEN_SCORING_OPT_IN.get(config["model"]["name"])
        sys.exit("main.py: --padding_type none needs a model that takes per-utterance lengths: wav2vec2_linear_nll only, or the scoring mode "
                 "of wav2vec2_resnet_nll (%s has no padding mask in its back-end); use --padding_type zero or repeat" % config["model"]["name"]
                 + ("" if switch is None else ".  %s=1 turns on this plugin's scoring mode with lengths" % switch))
    if args.padding_type == "zero" and args.batch_size > 1 and len(set(_train_opt_in(config["model"]["name"]))) == 2:
        name = config["model"]["name"]
        sys.exit("main.py: --padding_type zero --batch_size %d trains %s on zero-padded packs only with BOTH %s=1 (training with lengths) and "
                 "%s=1 or =long (validation scores under the mask) set; only one of them is.  Set both, or neither to keep the fixed-length "
                 "behaviour" % (args.batch_size, name, VARLEN_TRAIN_OPT_IN[name], VARLEN_SCORING_OPT_IN[name]))
    model = MODEL_REGISTRY[config["model"]["name"]](config["model"], device, seed=args.seed, rank=rank)
    print("nb_params:", sum(p.numel() for p in model.parameters()))

    from scl_amd.optim import FusedAdamW
    from scl_amd.parallel import GradSync, shard_indices
    from scl_amd.prefetch import Prefetcher
    g_lo, g_hi = model.trainable_range()
    # SCL_DP_MODE=shard: reduce-scatter + AdamW on the rank's shards + all-gather of the parameters instead of all-reduce + replicated AdamW
    sync = GradSync(model.P.grad[g_lo:g_hi], base=g_lo, mode=os.environ.get("SCL_DP_MODE", "allreduce")) if world > 1 else None
    optimizer = FusedAdamW(model, lr=args.max_lr, weight_decay=args.weight_decay, grad_sync=sync)
    scheduler = torch.optim.lr_scheduler.CyclicLR(optimizer, base_lr=args.min_lr, max_lr=args.max_lr, step_size_up=3,
                                                  mode="exp_range", gamma=0.85, cycle_momentum=False)
    if args.model_path:
        sd = torch.load(args.model_path, map_location=device)
        sd = {k.replace("module.", "").replace("_orig_mod.", ""): v for k, v in sd.items()}
        model.load_state_dict(sd)
        print("Model loaded")
    else:
        print("Model initialized")
        if not getattr(model, "pretrained_loaded", False):
            msg = ("no --model_path and no pre-trained XLS-R checkpoint (pretrained/xlsr2_300m.pt, model/xlsr.py:14): the 300 M-parameter "
                   "encoder starts from seeded random noise")
            if args.eval:
                sys.exit("main.py --eval: " + msg + "; refusing to score with it")
            print("WARNING: " + msg + " — the reference fine-tunes the pre-trained encoder")

    proto = os.path.join(args.database_path, "protocol.txt")
    if args.eval:
        if not args.eval_output:
            sys.exit("main.py --eval needs --eval_output")
        _, file_eval = genList(dir_meta=proto, is_train=False, is_eval=True)
        print("no. of eval trials", len(file_eval))
        eval_set = Dataset_for_eval(list_IDs=file_eval, base_dir=os.path.join(args.database_path + "/"), padding_type=args.padding_type)
        if args.padding_type == "none":      # shorter files are zero-padded to what the model takes (400 samples; 17,680 for the ResNet back-end)
            eval_set.min_samples = model.min_samples()
            eval_set.max_samples = model.max_samples() if hasattr(model, "max_samples") else eval_set.max_samples      # longer files are cut (77,839 for the AASIST back-end)
        final_output = args.eval_output
        if world > 1:
            eval_set = Subset(eval_set, list(range(rank, len(eval_set), world)))
            # per-rank score shards, merged below in protocol order (embeddings are one file per utterance; their scores.txt is a shard too)
            shard = "%s.rank%d" % (os.path.join(final_output, "scores.txt") if args.emb else final_output, rank)
            if os.path.exists(shard):       # left behind by an aborted run: the writers append
                os.remove(shard)
            if not args.emb:
                args.eval_output = shard
        if args.predict:
            produce_prediction_file(eval_set, model, device, args.eval_output, batch_size=args.batch_size)
        elif args.emb:
            produce_emb_file(eval_set, model, device, args.eval_output, batch_size=args.batch_size,
                             scores_name="scores.txt.rank%d" % rank if world > 1 else "scores.txt")
        else:
            produce_evaluation_file(eval_set, model, device, args.eval_output, batch_size=args.batch_size)
        if world > 1:
            torch.distributed.barrier()
            if rank == 0:
                merge_rank_outputs(os.path.join(final_output, "scores.txt") if args.emb else final_output, world, len(file_eval))
        return 0

    repeat = args.padding_type == "repeat"
    # --padding_type zero with several packs per step: the default collate cannot stack packs of different lengths, so every pack is
    # zero-padded to trim_length and comes with per-view sample counts; run_epoch hands them to the model, which masks the padding in the
    # forward and the backward (training) or scores under the mask (validation).  The linear and the ResNet plugin (VARLEN_MODELS; the
    # latter's clips are padded to the 17,680 samples its back-end needs): the others take no lengths and keep their behaviour.  One pack
    # per step needs no mask (a pack at its own length), --padding_type repeat has no padding.
    pad_kw = {}
    if args.padding_type == "zero" and args.batch_size > 1 and _trains_varlen(config["model"]["name"]):
        if model.cfg.embed // model.cfg.heads != 64:
            sys.exit("main.py: --padding_type zero with --batch_size %d masks the padding in the streaming attention, which takes 64-wide "
                     "heads (this encoder's are %d wide); use --padding_type repeat or --batch_size 1"
                     % (args.batch_size, model.cfg.embed // model.cfg.heads))
        pad_kw = dict(pad_to_trim=True, min_samples=model.min_samples())
    # RawBoost parameter draws of the pack builder: "fast" = every builder thread's own numpy Generator, batched closed-form filter design,
    # ISD positions without a 64000-element permutation per clip (same distributions; scl_amd/augment.py); SCL_PACK_SAMPLER=reference =
    # the reference's draw-for-draw order on the global np.random stream (what the pack goldens pin; 0.5 ms more host time per clip), i.e.
    # SCL_PACK_SAMPLER=reference restores the reference's global-stream draws.  The fast sampler is seeded with [--seed, rank]: each rank
    # and each --seed draws its own notch filters, ISD positions, SNRs and noise (unseeded, every rank drew the same ones)
    args.rawboost_sampler = os.environ.get("SCL_PACK_SAMPLER", "fast")
    from scl_amd import augment
    augment.seed_fast_sampler([args.seed, rank])
    d_label_trn, file_train = genList(dir_meta=proto, is_train=True, is_eval=False, is_dev=False)
    print("no. of training trials", len(file_train))
    train_set = Dataset_for(args, list_IDs=file_train, labels=d_label_trn, base_dir=args.database_path + "/", algo=args.algo,
                            repeat_pad=repeat, **pad_kw, **config["data"]["kwargs"])
    d_label_dev, file_dev = genList(dir_meta=proto, is_train=False, is_eval=False, is_dev=True)
    print("no. of validation trials", len(file_dev))
    args.is_train = False
    dev_set = Dataset_for(args, list_IDs=file_dev, labels=d_label_dev, base_dir=args.database_path + "/", algo=args.algo,
                          repeat_pad=repeat, **pad_kw, **config["data"]["kwargs"])
    if world > 1:
        dev_set = Subset(dev_set, shard_indices(len(dev_set), rank, world, drop_last=False))
    dev_loader = DataLoader(dev_set, batch_size=args.batch_size, num_workers=0, shuffle=False)

    writer = ScalarLog("logs/{}".format(model_tag)) if rank == 0 else None
    early = EarlyStop(patience=10, delta=0.01, init_best=90.0, save_dir=model_save_path, is_main=rank == 0)
    t_start = time.time()
    for epoch in range(args.start_epoch, args.start_epoch + args.num_epochs):
        print("Epoch {}/{}. Current LR: {}".format(epoch, args.num_epochs - 1, optimizer.param_groups[0]["lr"]))
        if world > 1:   # same permutation on every rank, rank-strided shards, equal step counts
            epoch_set = Subset(train_set, shard_indices(len(train_set), rank, world, epoch_seed=args.seed + epoch))
            train_loader = DataLoader(epoch_set, batch_size=args.batch_size, num_workers=0, shuffle=False, drop_last=True)
        else:
            train_loader = DataLoader(train_set, batch_size=args.batch_size, num_workers=0, shuffle=True, drop_last=True)
        # pack i+1 is decoded / sampled / augmented by a prefetch thread on its own HIP stream while pack i trains (SCL_PREFETCH=0: inline)
        wrap = (lambda ld: Prefetcher(ld, depth=2, device=device)) if os.environ.get("SCL_PREFETCH", "1") != "0" else (lambda ld: ld)
        running_loss, train_acc, train_detail = run_epoch(wrap(train_loader), model, optimizer, device, config, train=True)
        val_loss, val_acc, val_detail = run_epoch(wrap(dev_loader), model, None, device, config, train=False)
        if writer is not None:
            for k, v in (("train_accuracy", train_acc), ("val_accuracy", val_acc), ("val_loss", val_loss), ("loss", running_loss)):
                writer.add_scalar(k, v, epoch)
            for k, v in train_detail.items():
                writer.add_scalar("train_{}".format(k), v, epoch)
            for k, v in val_detail.items():
                writer.add_scalar("val_{}".format(k), v, epoch)
        print("\n{} - {} - {} ".format(epoch, running_loss, val_loss))
        mix = model.layer_mix_weights() if hasattr(model, "layer_mix_weights") else None
        if mix is not None:      # ssl_layer_mix: the share of each hidden state (0: positional-conv residual ... last: final LayerNorm)
            print("layer mix: " + " ".join("%.4f" % v for v in mix.tolist()))
        scheduler.step()
        early(val_acc, model, epoch)
        if early.early_stop:
            print("Early stopping activated.")
            break
    print("Total training time: {}s".format(time.time() - t_start))
    return 0


if __name__ == "__main__":
    sys.exit(main())
