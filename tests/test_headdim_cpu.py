"""Head dims beyond 64 without a GPU: the `w2v_arch` choice of a YAML (encoder.w2v_config_from: names, the mapping form, the presets of
XLS-R 1B / 2B), the head dims the streaming attention takes, and static checks on the gfx950 assembly of csrc/attention_wide.hip
(hipcc cross-compiles): no kernel has a private segment or spills, and tools/isa_hazard_audit.py finds no use of a register with an
LDS read in flight — tests/test_attention_long_isa.py's two checks on the new file."""
import importlib.util
import os
import re
import subprocess

import pytest

from scl_amd.encoder import W2V_ARCHS, W2VConfig, stream_attn_takes, w2v_config_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scl-deepfake-audio-detection_amd", "csrc", "attention_wide.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("conv_dim", "conv_kernels", "conv_strides", "embed", "layers", "heads", "ffn", "pos_k", "pos_groups", "final_dim", "latent_vars",
          "latent_groups", "encoder_layerdrop")


def fields(cfg):
    return {k: getattr(cfg, k) for k in FIELDS}


def test_the_four_names():
    assert sorted(W2V_ARCHS) == ["tiny", "xlsr_1b", "xlsr_2b", "xlsr_300m"]
    assert fields(w2v_config_from({})) == fields(W2VConfig())      # the default: the reference's only encoder
    assert fields(w2v_config_from({"w2v_arch": "xlsr_300m", "encoder_layerdrop": 0.05})) == fields(W2VConfig(encoder_layerdrop=0.05))
    assert fields(w2v_config_from({"w2v_arch": "tiny"})) == fields(W2VConfig.tiny())
    base = fields(W2VConfig())
    b1 = w2v_config_from({"w2v_arch": "xlsr_1b", "encoder_layerdrop": 0.1})
    assert fields(b1) == dict(base, embed=1280, layers=48, heads=16, ffn=5120, final_dim=1024, encoder_layerdrop=0.1)
    b2 = w2v_config_from({"w2v_arch": "xlsr_2b"})
    assert fields(b2) == dict(base, embed=1920, layers=48, heads=16, ffn=7680, final_dim=1024)
    # the 300M model's conv stack and positional convolution, and the head dims the streaming attention was widened for
    assert (b1.embed // b1.heads, b2.embed // b2.heads) == (80, 120)
    assert stream_attn_takes(80) and stream_attn_takes(120)


def test_the_mapping_form():
    cfg = w2v_config_from({"w2v_arch": {"embed": 1280, "layers": 48, "heads": 16, "ffn": 5120, "final_dim": 1024}})
    assert fields(cfg) == fields(W2VConfig.xlsr_1b())
    small = dict(conv_dim=32, embed=160, layers=2, heads=2, ffn=320, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)
    cfg = w2v_config_from({"w2v_arch": small, "encoder_layerdrop": 0.2})
    assert fields(cfg) == dict(fields(W2VConfig()), encoder_layerdrop=0.2, **small)
    assert w2v_config_from({"w2v_arch": dict(small, encoder_layerdrop=0.0), "encoder_layerdrop": 0.2}).encoder_layerdrop == 0.0
    with pytest.raises(ValueError, match="W2VConfig"):
        w2v_config_from({"w2v_arch": {"embed": 1280, "width": 3}})


def test_an_unknown_name_lists_the_names():
    with pytest.raises(ValueError) as e:
        w2v_config_from({"w2v_arch": "xlsr_3b"})
    assert all(name in str(e.value) for name in W2V_ARCHS) and "xlsr_3b" in str(e.value)


def test_the_head_dims_the_streaming_attention_takes():
    assert [d for d in range(0, 200) if stream_attn_takes(d)] == [64, 72, 80, 88, 96, 104, 112, 120, 128]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "attention_wide.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", out, SRC],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_every_wide_kernel_has_no_private_segment_and_no_spills(asm):
    meta = re.findall(r"- \.agpr_count.*?\.wavefront_size: 64", asm, re.S)
    names = []
    for blk in meta:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        names.append(name)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    # forward, dK / dV and dQ: 3 layouts x 2 padded head dims x with / without dropout each; the delta pass: one per layout
    assert len(names) == 3 * (3 * 2 * 2) + 3, names
    for part in ("attn_fwd_wide_kernel", "attn_bwd_dkdv_wide_kernel", "attn_bwd_dq_wide_kernel", "attn_delta_wide_kernel"):
        assert any(part in n for n in names), part


def test_no_use_of_a_register_with_an_lds_read_in_flight(asm):
    spec = importlib.util.spec_from_file_location("isa_hazard_audit", os.path.join(ROOT, "tools", "isa_hazard_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.audit(asm) == 0
