"""Static checks on the gfx950 assembly of the packed variable-length attention kernels (csrc/attention_packed.hip; no GPU needed: hipcc
cross-compiles), as tests/test_attention_varlen_isa.py for the padded ones: no kernel has a private segment — no scratch, no VGPR or SGPR
spills — and no vector instruction touches the destination of an LDS read that may still be in flight (tools/isa_hazard_audit.py)."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "scl-deepfake-audio-detection_amd", "csrc", "attention_packed.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "attention_packed.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", out, SRC],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_every_kernel_has_no_private_segment_and_no_spills(asm):
    meta = re.findall(r"- \.agpr_count.*?\.wavefront_size: 64", asm, re.S)
    names = []
    for blk in meta:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        names.append(name)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name
    # forward, dK / dV and dQ with and without dropout (6), the delta pass, pack and unpack
    assert len(names) == 9, names
    for part in ("attn_fwd_packed_kernel", "attn_bwd_dkdv_packed_kernel", "attn_bwd_dq_packed_kernel", "attn_delta_packed_kernel",
                 "pack_rows_kernel", "unpack_rows_kernel"):
        assert any(part in n for n in names), part


def test_no_use_of_a_register_with_an_lds_read_in_flight(asm):
    spec = importlib.util.spec_from_file_location("isa_hazard_audit", os.path.join(ROOT, "tools", "isa_hazard_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.audit(asm) == 0
