"""What the packed fp32 scoring path says about head dims, without a GPU: encoder.stream_attn_takes is the one gate (unchanged: 64, or
72..128 in steps of 8), the docstrings of the gate, of Encoder.forward_f32 and of ops.attn_fwd_packed_f32 name the wide kernels instead of
"64 only", and the C entry's refusal is the streaming family's."""
import os
import re

from scl_amd import encoder as ENC
from scl_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scl-deepfake-audio-detection_amd", "csrc")


def test_the_gate_is_unchanged():
    assert [d for d in range(0, 160) if ENC.stream_attn_takes(d)] == [64, 72, 80, 88, 96, 104, 112, 120, 128]
    assert ENC.STREAM_ATTN_HEAD_DIMS == "head dim 64, or 72..128 in steps of 8"


def test_the_docstrings_name_the_head_dims_of_the_streaming_family():
    for doc in (ENC.Encoder.forward_f32.__doc__, ops.attn_fwd_packed_f32.__doc__, ops.attn_fwd_long.__doc__):
        assert "64 only" not in doc and "64-wide heads only" not in doc
    assert "packed rows in fp32" in ENC.stream_attn_takes.__doc__ and "packed fp32 kernel" not in ENC.stream_attn_takes.__doc__
    assert "attention_f32_wide.hip" in ENC.Encoder.forward_f32.__doc__ and "attention_f32_wide.hip" in ops.attn_fwd_packed_f32.__doc__


def test_forward_f32_refuses_by_the_gate_and_names_the_switch():
    src = open(os.path.join(ROOT, "scl-deepfake-audio-detection_amd", "encoder.py")).read()
    assert "if layout.packed and not stream_attn_takes(D):" in src and "layout.packed and D != 64" not in src
    m = re.search(r"if layout\.packed and not stream_attn_takes\(D\):\n\s+raise NotImplementedError\((.*?)\)\n", src, re.S)
    assert m and "SCL_SCORE_PACK" in m.group(1) and "STREAM_ATTN_HEAD_DIMS" in m.group(1)


def test_the_c_entry_refuses_with_the_streaming_familys_text():
    entry = open(os.path.join(CSRC, "attention_f32.hip")).read()
    assert 'SCL_REQUIRE(D == LD || scl_attn_wide_takes(D), "attn_fwd_packed_f32: " SCL_ATTN_HEAD_DIMS " (got D=%d)", D);' in entry
    assert "needs head dim 64 (got" not in entry
    hdr = open(os.path.join(ROOT, "include", "scl_hip.h")).read()
    assert "Head dim 64 only" not in hdr and "scl_attn_fwd_packed_f32 takes 64 only" not in hdr
