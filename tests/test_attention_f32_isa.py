"""Static checks on the gfx950 assembly of the fp32 streaming attention over packed rows (csrc/attention_f32.hip; no GPU needed: hipcc
cross-compiles), as tests/test_attention_packed_isa.py for the bf16 kernels: the kernel has no private segment — no scratch, no VGPR or
SGPR spills —, it is the only kernel of the file, its LDS is the four double-buffered images (64 KiB: two workgroups per CU), and no
vector instruction touches the destination of an LDS read that may still be in flight (tools/isa_hazard_audit.py)."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scl-deepfake-audio-detection_amd", "csrc", "attention_f32.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "attention_f32.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", out, SRC],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernels(asm):
    return re.findall(r"- \.agpr_count.*?\.wavefront_size: 64", asm, re.S)


def test_every_kernel_has_no_private_segment_and_no_spills(asm):
    names = []
    for blk in _kernels(asm):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        names.append(name)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    assert len(names) == 1, names      # the forward: no dropout variant, no backward
    assert "attn_fwd_packed_f32_kernel" in names[0]


def test_two_workgroups_fit_a_compute_unit(asm):
    (blk,) = _kernels(asm)
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
    agpr = int(re.search(r"\.agpr_count:\s+(\d+)", blk).group(1))
    print("attn_fwd_packed_f32_kernel: %d VGPRs (%d of them AGPRs), %d bytes of LDS" % (vgpr, agpr, lds))
    assert lds == 2 * 4 * 64 * 128      # K hi / lo rows, V hi / lo transposed, two buffers
    assert 2 * lds <= 160 * 1024        # the CU's LDS
    assert vgpr <= 256                  # 8 waves per CU = 2 per SIMD of 512 registers


def test_the_products_are_bf16_pairs_not_the_f32_matrix_form(asm):
    body = asm[asm.index("attn_fwd_packed_f32_kernel"):]
    assert "v_mfma_f32_16x16x32_bf16" in body
    assert "v_mfma_f32_16x16x4_f32" not in asm and "v_mfma_f32_32x32x2_f32" not in asm


def test_no_use_of_a_register_with_an_lds_read_in_flight(asm):
    spec = importlib.util.spec_from_file_location("isa_hazard_audit", os.path.join(ROOT, "tools", "isa_hazard_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.audit(asm) == 0
