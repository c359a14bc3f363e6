"""Host side of training on zero-padded packs (main.py --padding_type zero --batch_size k > 1), no GPU: the crop window and per-view
sample counts of scl_amd/augment.py against a numpy restatement of the crop kernel, the padded item of PackDataset, and the way the
counts travel through the default collate, a data-parallel Subset, the Prefetcher and main.run_epoch to the model."""
import argparse
import os
import wave

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Subset

from scl_amd import augment, pack
from scl_amd.prefetch import Prefetcher

TRIM, LO = 6000, 400


def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def crop_numpy(views, firstlen, start, out_len, repeat_pad):
    """csrc/augment.hip::multiview_crop_kernel, element for element."""
    out = np.zeros((len(views), out_len), dtype=np.float32)
    for v, sv in enumerate(views):
        lv = len(sv)
        for n in range(out_len):
            m = start + n
            if repeat_pad and firstlen > 0:
                m %= firstlen
            if m < firstlen:
                if m < lv:
                    out[v, n] = sv[m]
                elif repeat_pad:
                    out[v, n] = sv[m % lv]
    return out


@pytest.mark.parametrize("lens,length,u", [
    ([50, 50, 80, 20, 1], 64, 0.0),          # anchor shorter than the window: padded to it; a longer view is cut at the anchor's length
    ([64, 64, 10], 64, 0.0),                 # anchor exactly the window
    ([200, 200, 150, 90, 300], 64, 0.75),    # anchor longer: start = 102 — one view ends inside the window, one before it starts
    ([200, 120], 64, 0.5),                   # start = 68: 52 of the view's samples left
])
def test_crop_plan_counts_are_the_samples_the_kernel_copies(monkeypatch, lens, length, u):
    monkeypatch.setattr(np.random, "rand", lambda: u)
    start, out_len, counts = augment.crop_plan(lens, length, False, random_trim=True, pad=True)
    assert out_len == length and start == (int(u * (lens[0] - length)) if lens[0] >= length else 0)
    views = [np.arange(1, n + 1, dtype=np.float32) for n in lens]      # no sample is 0
    out = crop_numpy(views, lens[0], start, out_len, 0)
    for v, c in enumerate(counts):
        assert 0 <= c <= length and (out[v, :c] != 0).all() and not out[v, c:].any(), (v, c)
        assert np.array_equal(out[v, :c], views[v][start:start + c])
    # without pad: the window of the reference (an anchor shorter than the window gives a pack at its own length), no counts
    s2, o2, c2 = augment.crop_plan(lens, length, False, random_trim=True, pad=False)
    assert (s2, o2, c2) == (start, min(lens[0], length) if lens[0] < length else length, None)
    assert augment.crop_plan(lens, length, True, random_trim=True, pad=False)[:2] == (start, length)


@pytest.fixture
def host_pack(monkeypatch, tmp_path):
    """A PackDataset whose device work runs on the host: the crop kernel restated in numpy, an identity augmenter, plain tensors."""
    def crop_stub(src, off, lens, V, firstlen, start, out_len, repeat_pad, out, ldo):
        views = [src[int(off[v]):int(off[v]) + int(lens[v])].numpy() for v in range(V)]
        out.copy_(torch.from_numpy(crop_numpy(views, firstlen, start, out_len, 1 if repeat_pad else 0)))
    monkeypatch.setattr(augment.ops, "multiview_crop", crop_stub)
    monkeypatch.setattr(augment, "_h2d_pack", lambda arrays, dev: [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays])
    monkeypatch.setitem(pack.AUGMENTERS, "identity", lambda x, args, sr, audio_path=None: x)
    rs = np.random.RandomState(3)
    sizes = [2500, 9000, 4100, 6000, 300, 7000]      # shorter, longer, equal to TRIM, shorter than the shortest clip with a frame
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(tmp_path / "bonafide" / u), 0.1 + 0.05 * rs.rand(n))      # no sample is 0
        _write_wav(str(tmp_path / "vocoded" / ("hifigan_" + u)), 0.1 + 0.05 * rs.rand(max(n - 2200, 100)))

    def make(**kw):
        args = argparse.Namespace(device="cpu")
        return pack.PackDataset("augall_3", args, ids, {}, str(tmp_path), vocoders=["hifigan"], augmentation_methods=["identity"],
                                num_additional_real=1, trim_length=TRIM, **kw)
    return make, ids, sizes


def test_padded_pack_and_its_counts(host_pack):
    make, ids, sizes = host_pack
    ds = make(repeat_pad=False, pad_to_trim=True, min_samples=LO)
    np.random.seed(0)
    for i, n in enumerate(sizes):
        uid, x, lab, counts = ds[i]
        V = x.shape[1]
        assert uid == ids[i] and x.shape == (TRIM, 5) and lab.shape == (V,) and counts.shape == (V,) and counts.dtype == torch.int32
        assert not counts.is_cuda
        xv = x.t().numpy()
        for v in range(V):
            filled = int((xv[v] != 0).sum())      # the view's own samples in the window, then zeros
            assert (xv[v, :filled] != 0).all() and not xv[v, filled:].any()
            assert int(counts[v]) == min(max(filled, LO), TRIM), (i, v, filled, int(counts[v]))
        assert int(counts[0]) == min(max(n, LO), TRIM)      # the anchor
        if n > TRIM + 2200:      # its vocoded view is 2200 samples shorter: it may end inside the window
            assert int(counts[3]) <= TRIM


def test_one_pack_per_step_and_repeat_padding_keep_their_items(host_pack):
    make, ids, sizes = host_pack
    np.random.seed(0)
    own = make(repeat_pad=False)      # --batch_size 1: the pack at the anchor's own length, three items
    rep = make(repeat_pad=True, pad_to_trim=True)      # repeat padding wins: no padding to mask, three items
    for i, n in enumerate(sizes):
        item = own[i]
        assert len(item) == 3 and item[1].shape == (min(n, TRIM), 5)
        item = rep[i]
        assert len(item) == 3 and item[1].shape == (TRIM, 5) and (item[1] != 0).all()


class StandIn(torch.nn.Module):
    """Records what main.run_epoch hands over; the zeros beyond every row's count are checked on the way."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, lengths=None):
        assert lengths is not None and len(lengths) == x.shape[0] and all(isinstance(n, int) for n in lengths)
        assert all(not x[b, n:].any() for b, n in enumerate(lengths))
        self.calls.append((tuple(x.shape), list(lengths), x[:, 0].clone()))
        s = x.sum(1)
        return torch.stack([s, -s], 1), torch.zeros(x.shape[0], 3, 128), s[:, None].repeat(1, 128)

    def loss(self, out, feats, emb, y, config, info=None):
        return {"L_CE": out.sum() * 0.0 + 1.0}


@pytest.mark.parametrize("prefetch", [False, True])
def test_counts_travel_through_collate_subset_prefetcher_and_run_epoch(host_pack, prefetch):
    import main as M
    make, ids, sizes = host_pack
    ds = make(repeat_pad=False, pad_to_trim=True, min_samples=LO)
    sub = Subset(ds, [4, 1, 0, 3, 2])      # a rank's shard
    loader = DataLoader(sub, batch_size=2, num_workers=0, shuffle=False)
    model = StandIn()
    np.random.seed(1)
    total, acc, detail = M.run_epoch(Prefetcher(loader, depth=2, device=None) if prefetch else loader, model, None, "cpu", {}, train=False)
    assert total == 5.0 and detail == {"L_CE": 5.0}      # three steps of 2 + 2 + 1 packs, the loss computed pack by pack and summed
    assert [c[0] for c in model.calls] == [(10, TRIM), (10, TRIM), (5, TRIM)]
    anchors = [sizes[i] for i in (4, 1, 0, 3, 2)]
    got = [c[1][v] for c in model.calls for v in range(0, len(c[1]), 5)]      # row k*V of the [k*V, L] batch is pack k's anchor
    assert got == [min(max(n, LO), TRIM) for n in anchors]
    for shape, lengths, _ in model.calls:
        assert all(LO <= n <= TRIM for n in lengths)
