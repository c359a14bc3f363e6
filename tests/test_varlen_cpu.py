"""Host side of variable-length scoring (main.py --eval --padding_type none), no GPU: the batch planner of scl_amd/pack.py, the
own-length mode of EvalDataset, the command line, and the unchanged items of the zero / repeat modes."""
import os
import wave

import numpy as np
import pytest

from scl_amd import pack
from scl_amd.pack import EvalDataset, pad_eval, plan_varlen_batches


def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _check_plan(lengths, batch_size, budget=None, quantum=16000):
    plan = plan_varlen_batches(lengths, batch_size, budget, quantum) if budget is not None else plan_varlen_batches(lengths, batch_size)
    budget = batch_size * 64600 if budget is None else budget
    seen = []
    for idx, lpad in plan:
        assert 1 <= len(idx) <= batch_size
        assert lpad % quantum == 0 and lpad >= max(lengths[i] for i in idx)
        assert lpad - max(lengths[i] for i in idx) < quantum                  # rounded up to the NEXT multiple, not further
        assert len(idx) * lpad <= budget or len(idx) == 1
        seen += idx
    assert sorted(seen) == list(range(len(lengths)))                          # every index exactly once
    # inverting the permutation restores protocol order
    inv = np.empty(len(seen), dtype=np.int64)
    inv[np.asarray(seen, dtype=np.int64)] = np.arange(len(seen))
    assert [seen[j] for j in inv] == list(range(len(lengths)))
    # sorting never crosses a window of 16 * batch_size consecutive utterances
    win = pack.VARLEN_WINDOW * batch_size
    for idx, _ in plan:
        assert len({i // win for i in idx}) == 1
    return plan


@pytest.mark.parametrize("seed,n,batch_size", [(0, 1, 1), (1, 37, 1), (2, 500, 4), (3, 129, 8), (4, 2048, 10)])
def test_plan_on_seeded_random_lengths(seed, n, batch_size):
    rs = np.random.RandomState(seed)
    lengths = np.exp(rs.uniform(np.log(400), np.log(960000), n)).astype(np.int64).tolist()
    _check_plan(lengths, batch_size)


def test_plan_edge_cases():
    assert plan_varlen_batches([], 4) == []
    assert plan_varlen_batches([400], 4) == [([0], 16000)]
    assert plan_varlen_batches([16000, 16001], 2) == [([0, 1], 32000)]
    # an utterance beyond the budget is a batch of one; the rest still packs
    plan = _check_plan([960000, 400, 500, 129201], 2)
    assert ([0], 960000) in plan and ([3], 144000) in plan and ([1, 2], 16000) in plan
    # equal lengths keep protocol order (stable sort), batches are cut at batch_size
    assert [idx for idx, _ in plan_varlen_batches([5000] * 5, 2)] == [[0, 1], [2, 3], [4]]
    # the budget cuts a batch before batch_size does: 3 x 48000 > 2 x 64600
    assert [idx for idx, _ in plan_varlen_batches([40000, 40000, 40000], 3, budget=2 * 64600)] == [[0, 1], [2]]
    # windows: with batch_size 1 a window is 16 utterances; the 17th starts a new one although it is the shortest
    lengths = list(range(17000, 1000, -1000)) + [400]
    plan = _check_plan(lengths, 1)
    assert [idx for idx, _ in plan][-1] == [16] and [idx for idx, _ in plan][0] == [15]


def test_eval_dataset_none_returns_own_length_pads_to_400_and_cuts_at_960000(tmp_path):
    rs = np.random.RandomState(5)
    sizes = {"a.wav": 100, "b.wav": 400, "c.wav": 70001, "d.wav": 960123}
    for name, n in sizes.items():
        _write_wav(str(tmp_path / name), 0.1 * rs.randn(n))
    ds = EvalDataset(list(sizes), str(tmp_path), "none", subdir="")
    got = {name: ds[i] for i, name in enumerate(sizes)}
    assert [got[n][1] for n in sizes] == list(sizes)
    assert [got[n][0].shape[0] for n in sizes] == [400, 400, 70001, 960000]
    a = got["a.wav"][0].numpy()
    ref = pack.load_audio(str(tmp_path / "a.wav"), 16000)
    assert a.dtype == np.float32 and np.array_equal(a[:100], ref) and not a[100:].any() and np.abs(a[:100]).max() > 0
    assert np.array_equal(got["c.wav"][0].numpy(), pack.load_audio(str(tmp_path / "c.wav"), 16000))
    assert np.array_equal(got["d.wav"][0].numpy(), pack.load_audio(str(tmp_path / "d.wav"), 16000)[:960000])
    assert ds.n_cut == 1


@pytest.mark.parametrize("padding_type", ["zero", "repeat"])
def test_zero_and_repeat_items_are_pad_eval_of_the_decoded_file(tmp_path, padding_type):
    rs = np.random.RandomState(6)
    sizes = {"s.wav": 3000, "e.wav": 64600, "l.wav": 70000}
    for name, n in sizes.items():
        _write_wav(str(tmp_path / name), 0.1 * rs.randn(n))
    ds = EvalDataset(list(sizes), str(tmp_path), padding_type, subdir="")
    assert ds.cut == 64600
    for i, name in enumerate(sizes):
        x, uid = ds[i]
        ref = np.ascontiguousarray(pad_eval(pack.load_audio(str(tmp_path / name), 16000), padding_type, 64600), dtype=np.float32)
        assert uid == name and x.numpy().tobytes() == ref.tobytes()
        row = np.full(64600, np.nan, dtype=np.float32)
        assert ds.load_into(i, row) == name and row.tobytes() == ref.tobytes()


def test_parser_accepts_none_and_training_with_none_exits_with_the_message(tmp_path, monkeypatch):
    import main as M
    assert M.build_parser().parse_args(["--padding_type", "none", "--eval"]).padding_type == "none"
    assert M.build_parser().parse_args([]).padding_type == "zero"
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        M.main(["--padding_type", "none", "--config", "missing.yaml"])
    assert "--padding_type none" in str(e.value) and "--eval" in str(e.value)
    assert not os.path.exists(tmp_path / "out")      # refused before anything was created


def test_scoring_loop_hands_rows_over_in_protocol_order_across_windows_and_through_a_subset(tmp_path):
    """main.py's three writers over 63 files (two windows of 16 batches of 2) with a stand-in model on the CPU: every batch is a
    zero-padded [count <= 2, multiple of 16000] tensor with its sample counts, every utterance is written once, in protocol order, for
    the dataset itself and for the Subset a rank of a multi-rank run gets."""
    import torch
    from torch.utils.data import Subset
    import main as M
    rs = np.random.RandomState(0)
    sizes = [3000, 9000, 30000, 70000, 24000, 100, 50000] * 9
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(tmp_path / "data" / u), 0.1 * rs.randn(n))

    class StandIn(torch.nn.Module):
        is_train = True

        def forward(self, x, lengths=None):
            assert lengths is not None and x.shape[1] % 16000 == 0 and x.shape[0] == len(lengths) <= 2
            assert all(not x[b, n:].any() for b, n in enumerate(lengths))
            s = torch.stack([x[b, :n].sum() for b, n in enumerate(lengths)])
            logp = torch.stack([s, torch.tensor([float(n) for n in lengths])], 1)
            return (logp, torch.zeros(len(lengths), 3, 128), s[:, None].repeat(1, 128)) if self.is_train else logp

    ds = EvalDataset(ids, str(tmp_path / "data"), "none", subdir="")
    for tag, dset, want in (("all", ds, list(range(len(ids)))), ("rank1", Subset(ds, list(range(1, len(ids), 2))), list(range(1, len(ids), 2)))):
        out = str(tmp_path / ("scores_%s.txt" % tag))
        M.produce_evaluation_file(dset, StandIn(), "cpu", out, batch_size=2)
        lines = open(out).read().strip().split("\n")
        assert [l.split()[0] for l in lines] == [ids[i] for i in want]
        for l, i in zip(lines, want):
            assert abs(float(l.split()[1]) - float(ds[i][0].sum())) < 1e-3 and float(l.split()[2]) == max(sizes[i], 400)
        pred = str(tmp_path / ("pred_%s.txt" % tag))
        M.produce_prediction_file(dset, StandIn(), "cpu", pred, batch_size=2)
        assert [l.split()[0] for l in open(pred).read().strip().split("\n")] == [ids[i] for i in want]
        emb = str(tmp_path / ("emb_%s" % tag))
        M.produce_emb_file(dset, StandIn(), "cpu", emb, batch_size=2)
        assert sorted(f for f in os.listdir(emb) if f.endswith(".npy")) == sorted("u%d.npy" % i for i in want)
        assert [l.split()[0] for l in open(os.path.join(emb, "scores.txt")).read().strip().split("\n")] == [ids[i] for i in want]
