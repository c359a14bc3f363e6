"""Host side of the packed variable-length layout (csrc/attention_packed.hip), no GPU: the row offsets and the row count of a step
(ops.packed_rows: the bucket rule and its cap), the validation of the offsets, and the entry points refusing null or bad arguments with an
error code and a message before anything is launched.  The header / ctypes agreement is tests/test_abi.py's."""
import ctypes

import pytest
import torch

from scl_amd import encoder, lib, ops
from scl_amd.lib import SclError


def test_row_offsets_and_row_count():
    # the frames of tests/test_varlen_pack_gpu.py: B * T = 390 -> cap 448
    row0, Mq = ops.packed_rows([65, 1, 64, 24, 37, 12], 65, 64)
    assert row0 == [0, 65, 66, 130, 154, 191, 203] and Mq == 256
    assert ops.packed_rows([65, 1, 64, 24, 37, 12], 65, 512)[1] == 448      # one bucket wider than the padded batch: the cap
    assert ops.packed_rows([65] * 6, 65, 64) == ([65 * b for b in range(7)], 448)      # every frame valid: roundup(B * T, 64)
    assert ops.packed_rows([1] * 6, 65, 64)[1] == 64 and ops.packed_rows([64], 199, 64)[1] == 64 and ops.packed_rows([65], 199, 64)[1] == 128


def test_the_bucket_rule():
    """Mq is the smallest multiple of PACK_ROWS that holds the valid rows, capped at roundup(B * T, 64); always a multiple of 64, never
    below the valid rows, less than PACK_ROWS above them; 64 x 199 frames give at most 25 row counts."""
    assert encoder.PACK_ROWS == 512 and encoder.PACK_ROWS % 64 == 0 and encoder.VARLEN_PACK is False
    B, T = 64, 199
    cap = (B * T + 63) // 64 * 64
    seen = set()
    for n in list(range(1, T + 1)):
        for frames in ([n] * B, [n] + [T] * (B - 1), [n] + [1] * (B - 1)):
            row0, Mq = ops.packed_rows(frames, T, encoder.PACK_ROWS)
            Mv = sum(frames)
            assert row0[-1] == Mv and Mq % 64 == 0 and Mv <= Mq <= cap and Mq - Mv < encoder.PACK_ROWS
            assert Mq == min((Mv + 511) // 512 * 512, cap)
            seen.add(Mq)
    assert len(seen) <= 25 and max(seen) == cap == 12736
    for bad in (0, 32, 100, -64):
        with pytest.raises(ValueError, match="multiple of 64"):
            ops.packed_rows([3, 4], 8, bad)


def test_offsets_are_validated_on_the_host():
    assert ops.check_packed_rows([0, 3, 4], 8, 64) == [0, 3, 4]
    for row0, T, Mq, what in (([0, 5, 3], 8, 64, "outside 1..8"),            # not monotone
                              ([0, 4, 4], 8, 64, "outside 1..8"),            # an utterance without a frame
                              ([0, 9, 12], 8, 64, "outside 1..8"),           # longer than the padded length
                              ([1, 3, 4], 8, 64, r"row0\[0\]"),
                              ([0, 60, 120, 180], 64, 128, "do not fit")):   # row0[B] > Mq
        with pytest.raises(SclError, match=what):
            ops.check_packed_rows(row0, T, Mq)
    with pytest.raises(SclError):
        ops.packed_rows([3, 0, 4], 8, 64)
    with pytest.raises(SclError):
        ops.packed_rows([3, 9], 8, 64)


def test_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    L = lib.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)      # a host address: a refused call never dereferences it
    assert L.scl_packed_check_rows(None, 2, 8, 64) == -1 and b"packed_check_rows" in L.scl_last_error()
    assert L.scl_packed_check_rows(buf, 0, 8, 64) == -1 and L.scl_packed_check_rows(buf, 4, 8, 3) == -1
    assert L.scl_attn_fwd_packed(None, p, p, p, 2, 8, 2, 64, 64, 0.125, None) == -1 and b"attn_fwd_packed" in L.scl_last_error()
    assert L.scl_attn_fwd_packed(p, p, p, None, 2, 8, 2, 64, 64, 0.125, None) == -1
    assert L.scl_attn_fwd_packed(p, p, p, p, 2, 8, 2, 32, 64, 0.125, None) == -1 and b"head dim 64" in L.scl_last_error()
    assert L.scl_attn_fwd_packed(p, p, p, p, 2, 8, 2, 64, 128, 0.125, None) == -1 and b"Mq" in L.scl_last_error()      # above roundup(B * T, 64)
    assert L.scl_attn_fwd_packed(p, p, p, p, 2, 8, 2, 64, 1, 0.125, None) == -1      # fewer rows than utterances
    assert L.scl_attn_fwd_packed_drop(p, p, p, p, 2, 8, 2, 64, 64, 0.125, 1.0, 1, None) == -1 and b"attn_fwd_packed_drop" in L.scl_last_error()
    assert L.scl_attn_fwd_packed_drop(p, p, p, p, 2, 8, 2, 32, 64, 0.125, 0.1, 1, None) == -1 and b"head dim 64" in L.scl_last_error()
    assert L.scl_attn_bwd_packed(p, p, p, p, p, p, None, 2, 8, 2, 64, 64, 0.125, 0.0, 0, None) == -1 and b"attn_bwd_packed" in L.scl_last_error()
    assert L.scl_attn_bwd_packed(p, p, p, p, p, p, p, 2, 8, 2, 32, 64, 0.125, 0.0, 0, None) == -1 and b"head dim 64" in L.scl_last_error()
    assert L.scl_attn_bwd_packed(p, p, p, p, p, p, p, 2, 8, 2, 64, 64, 0.125, -0.5, 0, None) == -1
    for fn, name in ((L.scl_pack_rows, b"pack_rows"), (L.scl_unpack_rows, b"unpack_rows")):
        assert fn(None, p, 1, p, 2, 8, 128, 64, None) == -1 and name in L.scl_last_error()
        assert fn(p, p, 1, None, 2, 8, 128, 64, None) == -1
        assert fn(p, p, 0, p, 2, 8, 12, 64, None) == -1 and b"C % 8" in L.scl_last_error()
        assert fn(p, p, 0, p, 2, 8, 128, 128, None) == -1 and b"Mq" in L.scl_last_error()


def test_sample_counts_to_a_row_layout(monkeypatch):
    """encoder.row_layout on the host (device="cpu"): frame counts from the conv stack's own arithmetic, the two rules for a row below the
    minimum clip, the pack switch of each precision read at call time, and the refusals of RowLayout itself."""
    cfg = encoder.W2VConfig.tiny()
    B, L, lengths, lo = 4, 4000, [4000, 1000, 399, 1], cfg.min_samples()
    assert cfg.conv_lens(L)[-1] == 12 and cfg.conv_lens(lo)[-1] == 1 and lo > 399
    want = [cfg.conv_lens(max(n, lo))[-1] for n in lengths]
    assert want[2:] == [1, 1]      # the last two rows count as the minimum clip: one frame
    monkeypatch.setattr(encoder, "PACK_ROWS", 64)
    for score_f32, switch, other in ((True, "SCORE_PACK", "VARLEN_PACK"), (False, "VARLEN_PACK", "SCORE_PACK")):
        kw = dict(min_samples=lo, refuse_short=False, score_f32=score_f32, device="cpu")
        monkeypatch.setattr(encoder, switch, True)
        monkeypatch.setattr(encoder, other, False)
        counts, lay = encoder.row_layout(cfg, lengths, B, L, **kw)
        assert counts == want and lay.frames.tolist() == want and lay.frames.dtype == torch.int32
        assert lay.packed and not lay.padded and not lay.fixed and lay.Mq == 64
        assert lay.row0.tolist() == [sum(want[:b]) for b in range(B + 1)] and lay.row0.dtype == torch.int32
        assert lay.rows(B * 12) == 64 and lay.key(B, L) == (B, L, "packed") and lay.plan_key("fwd", True) == ("fwd", True, 64)
        lay.check(B, 12)
        monkeypatch.setattr(encoder, switch, False)
        monkeypatch.setattr(encoder, other, True)      # the other precision's switch has no effect
        counts, lay = encoder.row_layout(cfg, torch.tensor(lengths), B, L, **kw)
        assert counts == want and lay.frames.tolist() == want and lay.row0 is None and lay.Mq is None
        assert lay.padded and not lay.packed and not lay.fixed
        assert lay.rows(B * 12) == B * 12 and lay.key(B, L) == (B, L) and lay.plan_key("fwd", True) == ("fwd", True)
        with pytest.raises(ValueError, match="at least"):
            encoder.row_layout(cfg, lengths, B, L, **dict(kw, refuse_short=True))
        for refuse in (False, True):
            with pytest.raises(ValueError, match="lengths"):
                encoder.row_layout(cfg, [4000, 4001], 2, L, **dict(kw, refuse_short=refuse))
    fixed = encoder.RowLayout()
    assert fixed.fixed and not fixed.padded and not fixed.packed and fixed.rows(48) == 48 and fixed.key(B, L) == (B, L)
    frames = torch.tensor(want, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"packed=\(row0, Mq\) needs the frame counts of the batch"):
        encoder.RowLayout(None, torch.tensor([0, 12, 14, 15, 16], dtype=torch.int32), 64)
    with pytest.raises(ValueError, match="packed row count 100: need a multiple of 64"):
        encoder.RowLayout(frames, torch.tensor([0, 12, 14, 15, 16], dtype=torch.int32), 100)
    with pytest.raises(ValueError, match=r"packed row count 128: need a multiple of 64 in 4\.\.64"):      # above roundup(B * T, 64)
        encoder.RowLayout(frames, torch.tensor([0, 12, 14, 15, 16], dtype=torch.int32), 128).check(B, 12)
    with pytest.raises(AttributeError):      # immutable
        fixed.Mq = 64
