"""tests/conv_stack_cases.py on the CPU: the fp64 stage reference is pinned to the oracle, the reference with the encoder's permitted
roundings (stage_emulation) stays under the bars the GPU test applies, every boundary mistake the bars are meant to catch is over them,
and the case list reaches the exact-fit and the left-over geometry in every layer."""
import pytest
import torch

from oracle import wav2vec2 as W
from scl_amd.encoder import W2VConfig
from tests import conv_stack_cases as CS

# (C, k, s, Tin): exact fit and one left-over input frame, for both kernel widths of the stack
EMU_SHAPES = [(C, k, s, Tin) for C in (512, 32) for (k, s, Tin) in ((3, 2, 399), (3, 2, 400), (2, 2, 99), (2, 2, 98))]


@pytest.fixture(scope="module")
def emulated():
    """{shape: (inputs, reference, emulation)}, computed once."""
    out = {}
    for i, (C, k, s, Tin) in enumerate(EMU_SHAPES):
        inp = CS.gaussian_stage(C, k, s, Tin, seed=100 + i)
        out[(C, k, s, Tin)] = (inp, CS.stage_reference(*inp, s), CS.stage_emulation(*inp, s))
    return out


def test_case_list_reaches_both_geometries_in_every_layer():
    cfg = W2VConfig()
    seen = {i: set() for i in range(1, len(cfg.conv_kernels))}
    for L in CS.CLIPS:
        Ts = cfg.conv_lens(L)
        for i in seen:
            seen[i].add(CS.leftover(Ts[i - 1], cfg.conv_kernels[i], cfg.conv_strides[i]) > 0)
    assert all(v == {False, True} for v in seen.values()), seen
    assert cfg.conv_lens(4000) == [799, 399, 199, 99, 49, 24, 12] and cfg.conv_lens(6075) == [1214, 606, 302, 150, 74, 37, 18]
    for width in CS.WIDTHS:      # both widths run the production kernel / stride list
        c = W2VConfig(**CS.config_kwargs(width))
        assert (c.conv_kernels, c.conv_strides) == (cfg.conv_kernels, cfg.conv_strides)
    assert W2VConfig(**CS.config_kwargs("c512")).conv_dim == 512 and len(CS.CASES) == 4


def test_reference_chain_equals_the_oracle_conv_stack():
    cfg = W.W2VConfig.tiny()
    sd = W.init_state(cfg, seed=5, dtype=torch.float64)
    for L in CS.CLIPS:
        x = 0.1 * torch.randn(CS.B, L, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
        outs = W.conv_stack(sd, cfg, x)
        z = outs[0]
        for i in range(1, len(cfg.conv_kernels)):
            p = "feature_extractor.conv_layers.%d." % i
            z = CS.stage_reference(z, sd[p + "0.weight"], sd[p + "0.bias"], sd[p + "2.1.weight"], sd[p + "2.1.bias"], None, cfg.conv_strides[i])["z"]
            assert z.shape == outs[i].shape
            assert CS.rel_max(z, outs[i]) <= 1e-12, (L, i, CS.rel_max(z, outs[i]))


def test_phase_dgrad_over_wd_blocks_is_the_transposed_convolution():
    g = torch.Generator().manual_seed(3)
    for (Co, Ci, k, s, Tin) in ((16, 8, 3, 2, 41), (16, 8, 3, 2, 42), (16, 8, 2, 2, 41), (8, 8, 10, 5, 64), (8, 16, 3, 1, 9), (8, 8, 4, 3, 20)):
        Tout = (Tin - k) // s + 1
        w = torch.randn(Co, Ci, k, generator=g, dtype=torch.float64)
        dy = torch.randn(2, Tout, Co, generator=g, dtype=torch.float64)
        got = CS.phase_dgrad(dy, CS.wd_reference(w, s), k, s, Tin)
        ref = torch.nn.functional.conv_transpose1d(dy.transpose(1, 2), w, stride=s).transpose(1, 2)
        ref = torch.cat([ref, torch.zeros(2, Tin - ref.shape[1], Ci, dtype=torch.float64)], dim=1)
        assert CS.rel_max(got, ref) <= 1e-14, (Co, Ci, k, s, Tin)
        assert all(not got[:, r].any() for r in CS.unreached_rows(Tin, k, s))


def test_emulation_stays_under_the_bars(emulated):
    """The reference with the permitted roundings passes: every metric of the emulation is at most EMU (half the bar of a bf16-limited
    tensor) and under the bar of every fp32-limited quantity."""
    worst, over = {}, []
    for shape, (inp, ref, emu) in emulated.items():
        for kind, v in CS.stage_metrics(emu, ref).items():
            worst[kind] = max(worst.get(kind, 0.0), v)
            lim = CS.EMU.get(kind, CS.BARS[kind])
            if not v <= lim:
                over.append("%s %s: %.3e > %.3e" % (shape, kind, v, lim))
    print("\nemulation, worst per kind:", ", ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    assert not over, "\n".join(over)
    # the constants are the measured worst rounded up, not a loose cover: within 15 % of what the emulation gives
    for kind, v in CS.EMU.items():
        assert worst[kind] > 0.85 * v, (kind, worst[kind], v)


MUTATIONS = [("dgrad_last_frame", ("dz",)), ("wgrad_last_frame", ("dw",)), ("wd_swap", ("dz",)), ("stale_leftover", ("dz",))]


@pytest.mark.parametrize("mutation,kinds", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_bars_reject_boundary_mistakes(emulated, mutation, kinds):
    """Each mutated gradient is over its bar on the whole tensor (rel-L2 and max) and, for a tensor with frames, on the boundary-row
    metric; the weight gradient has no rows per frame, so there the whole-tensor metrics stand alone."""
    n = 0
    for (C, k, s, Tin), (inp, ref, _) in emulated.items():
        if mutation == "wd_swap" and len(range(0, k, s)) != 2:
            continue
        if mutation == "stale_leftover" and not CS.leftover(Tin, k, s):
            continue
        m = CS.stage_metrics(CS.stage_emulation(*inp, s, mutate=mutation), ref, vectors=False)
        for kind in kinds:
            for suffix in ("_l2", "_max") + (("_rows",) if kind != "dw" else ()):
                print("%s %s %s%s: %.3e (bar %.3e)" % (mutation, (C, k, s, Tin), kind, suffix, m[kind + suffix], CS.BARS[kind + suffix]))
                assert m[kind + suffix] > CS.BARS[kind + suffix], (mutation, (C, k, s, Tin), kind + suffix, m[kind + suffix])
        n += 1
    assert n >= 2
