"""tests/posconv_cases.py on the CPU: the fp64 stages are pinned to the oracle, the references with the encoder's permitted roundings
(stage_emulation_p / _f) stay under the bars the GPU test applies, every composition mistake the bars are meant to catch is over them
(and the one a short clip cannot see is shown to be invisible there), and the case list reaches every kernel path of the stage."""
import pytest
import torch

from oracle import wav2vec2 as W
from scl_amd.encoder import W2VConfig
from tests import posconv_cases as PC

E = PC.BASE["embed"]
VL_K128 = (199, 66, 18, 1)      # the frame counts of VARLEN_LENGTHS
VL_CG32 = (37, 12, 24, 1)
# (G, K, T, frames): the geometry of every GPU case
EMU_SHAPES = [(2, 128, 18, None), (2, 128, 199, None), (2, 128, 208, None), (2, 128, 209, None), (2, 128, 225, None), (2, 16, 18, None),
              (4, 16, 18, None), (2, 128, 199, VL_K128), (4, 16, 37, VL_CG32)]


@pytest.fixture(scope="module")
def emulated():
    """{shape: (inputs, reference P, emulation P, reference F, emulation F)}, computed once."""
    out = {}
    for i, (G, K, T, frames) in enumerate(EMU_SHAPES):
        s = PC.gaussian_stage(E, G, K, T, seed=200 + i, Bn=PC.B_FIXED if frames is None else len(frames), frames=frames)
        emu_f = PC.stage_emulation_f(*PC.f_args(s))
        ref_f = PC.stage_reference_f(*PC.f_args(s), h0_stored=emu_f["h0"], dh_stored=emu_f["d_h"])
        out[(G, K, T, frames)] = (s, PC.stage_reference_p(*PC.p_args(s)), PC.stage_emulation_p(*PC.p_args(s)), ref_f, emu_f)
    return out


def test_case_list_reaches_every_path_of_the_stage():
    frames_of = lambda cfg, lengths: [cfg.conv_lens(n)[-1] for n in lengths]
    cfgs = {name: W2VConfig(**PC.config_kwargs(name)) for name in PC.CONFIGS}
    per = {name: cfgs[name].embed // cfgs[name].pos_groups for name in cfgs}
    assert per == {"k128": 64, "k16": 64, "cg32": 32}
    assert (cfgs["k128"].pos_k, cfgs["k16"].pos_k, cfgs["cg32"].pos_k) == (128, 16, 16)
    fixed = {name: set() for name in cfgs}
    for name, layout, lengths in PC.CASES:
        T = frames_of(cfgs[name], lengths)
        if layout == "fixed":
            assert len(set(T)) == 1 and len(lengths) == 3 and (T[0], lengths[0]) in PC.FIXED_CLIPS[name]
            assert lengths[0] == 64000 or lengths[0] == PC.samples_for(T[0]) == cfgs[name].samples_for(T[0])
            fixed[name].add(T[0])
    assert fixed["k128"] >= {208, 209, 225} and any(t >= 65 for t in fixed["k128"]) and min(fixed["k128"]) < 65      # every tap; a clip that cannot
    assert fixed["k16"] == {18} and fixed["cg32"] == {18}
    varlen = {(name, layout): frames_of(cfgs[name], lengths) for name, layout, lengths in PC.CASES if layout != "fixed"}
    assert set(varlen) == {("k128", "padded"), ("k128", "packed"), ("cg32", "padded"), ("cg32", "packed")}
    for layout in ("padded", "packed"):
        fr = varlen[("k128", layout)]
        assert tuple(fr) == VL_K128 and len(fr) == 4
        assert 1 in fr and any(65 <= n < max(fr) for n in fr)      # a single frame; every tap reached inside a slab it does not fill
        assert tuple(varlen[("cg32", layout)]) == VL_CG32
    for name, second in PC.VARLEN_SECOND.items():      # the second step: same padded shape, other rows valid
        first = PC.VARLEN_LENGTHS[name]
        assert max(second) == max(first) and len(second) == len(first) and list(second) != list(first)
        assert frames_of(cfgs[name], second) != frames_of(cfgs[name], first)
    assert len(PC.CASES) == 11


def test_reference_stages_equal_the_oracle():
    for name, T, B in (("k16", 18, 2), ("cg32", 37, 2), ("k128", 70, 1)):
        cfg = W.W2VConfig(**PC.config_kwargs(name))
        sd = W.init_state(cfg, seed=5, dtype=torch.float64)
        x = 0.1 * torch.randn(B, PC.samples_for(T), generator=torch.Generator().manual_seed(T), dtype=torch.float64)
        _, inter = W.forward(sd, cfg, x, return_all=True)
        f = PC.stage_reference_f(inter["conv"][-1], sd["layer_norm.weight"], sd["layer_norm.bias"], sd["post_extract_proj.weight"],
                                 sd["post_extract_proj.bias"], None)
        assert f["proj"].shape == inter["proj"].shape == (B, T, cfg.embed)
        assert PC.rel_max(f["proj"], inter["proj"]) <= 1e-12
        p = PC.stage_reference_p(inter["proj"], sd["encoder.pos_conv.0.weight_v"], sd["encoder.pos_conv.0.weight_g"],
                                 sd["encoder.pos_conv.0.bias"], None, cfg.pos_groups)
        assert PC.rel_max(p["xin0"], inter["pos"]) <= 1e-12, (name, PC.rel_max(p["xin0"], inter["pos"]))
        assert PC.rel_max(p["w"], W.pos_conv_weight(sd)) <= 1e-14


def test_masked_reference_is_each_utterance_alone():
    """With frames, the valid rows of the stage are those of the utterance alone at its own length (the gradient of the weights is the
    sum), and the padded rows of dx0 are 0: fairseq's features[padding_mask] = 0."""
    s = PC.gaussian_stage(E, 4, 16, 37, seed=9, Bn=4, frames=VL_CG32)
    ref = PC.stage_reference_p(*PC.p_args(s))
    dw = torch.zeros_like(ref["dw"])
    for b, n in enumerate(VL_CG32):
        one = PC.stage_reference_p(s["x0"][b: b + 1, :n], s["v"], s["g"], s["b"], s["dxin0"][b: b + 1, :n], s["G"])
        for key in ("pre", "xin0", "dc", "dx0"):
            assert PC.rel_max(ref[key][b: b + 1, :n], one[key]) <= 1e-12, (b, key)
        assert not ref["dx0"][b, n:].any()
        dw += one["dw"]
    assert PC.rel_max(ref["dw"], dw) <= 1e-12


def test_slab_products_over_the_packed_layouts_are_the_convolution():
    """The index-built operands and the two zero-padded images (K // 2 rows in front of x0, K // 2 - 1 in front of dc) in fp64 give the
    convolution, its transpose and its weight gradient: the composition of Encoder.forward / backward, without any rounding."""
    for (G, K, T) in ((2, 16, 18), (1, 2, 5), (3, 8, 1), (2, 128, 70)):
        Cg = 8
        En = G * Cg
        gen = torch.Generator().manual_seed(K)
        x, dxin = torch.randn(2, T, En, generator=gen, dtype=torch.float64), torch.randn(2, T, En, generator=gen, dtype=torch.float64)
        v = torch.randn(En, Cg, K, generator=gen, dtype=torch.float64)
        g, b = 1 + 0.1 * torch.randn(1, 1, K, generator=gen, dtype=torch.float64), torch.randn(En, generator=gen, dtype=torch.float64)
        ref = PC.stage_reference_p(x, v, g, b, dxin, G)
        xpad, dcpad = PC.pad_image(x, K, K // 2), PC.pad_image(ref["dc"], K, K // 2 - 1)
        assert PC.rel_max(PC.slab_product(xpad, PC.wf_layout(ref["w"], G), T, G) + b, ref["pre"]) <= 1e-13
        assert PC.rel_max(PC.slab_product(dcpad, PC.wd_layout(ref["w"], G), T, G), ref["dbranch"]) <= 1e-13
        dwf = PC.wgrad_product(dcpad, K // 2 - 1, xpad, T, G)
        assert PC.rel_max(PC.dwf_to_conv(dwf, En, Cg, K), ref["dw"]) <= 1e-13
        dv, dg = PC.weight_norm_backward(dwf, v, g, G)
        assert PC.rel_max(dv, ref["dv"]) <= 1e-12 and PC.rel_max(dg, ref["dg"]) <= 1e-12


def test_emulation_stays_under_the_bars(emulated):
    """The references with the permitted roundings pass: every metric of the emulations is at most EMU (half the bar of a bf16-limited
    tensor) and under the bar of every fp32-limited quantity."""
    worst, over = {}, []
    for shape, (s, ref_p, emu_p, ref_f, emu_f) in emulated.items():
        m = PC.stage_metrics_p(emu_p, ref_p, s["frames"])
        m.update(PC.stage_metrics_f(emu_f, ref_f, s["frames"]))
        dv, dg = PC.weight_norm_backward(emu_p["dwf"], s["v"], s["g"], s["G"])
        m["dv_wn"], m["dg_wn"] = PC.rel_max(emu_p["dv"], dv), PC.rel_max(emu_p["dg"], dg)
        m["dbp_sum"] = PC.rel_max(emu_p["db"], emu_p["dcpad"].double().sum((0, 1)))
        m["wpack"] = max(PC.wpack_ratio(emu_p["wf"], PC.wf_layout(ref_p["w"], s["G"])), PC.wpack_ratio(emu_p["wd"], PC.wd_layout(ref_p["w"], s["G"])))
        for kind, val in m.items():
            worst[kind] = max(worst.get(kind, 0.0), val)
            lim = PC.EMU.get(kind, PC.BARS[kind])
            if not val <= lim:
                over.append("%s %s: %.3e > %.3e" % (shape, kind, val, lim))
    print("\nemulation, worst per kind:", ", ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    assert not over, "\n".join(over)
    # the constants are the measured worst rounded up, not a loose cover: within 15 % of what the emulation gives
    for kind, val in PC.EMU.items():
        assert worst[kind] > 0.85 * val, (kind, worst[kind], val)


# mutation -> the tensor kinds it must push over their bars
TOUCHES = {"drop_last_tap": ("pre", "br", "dxb", "dwf"), "trim_first": ("pre", "br", "dxb", "dwf"), "pb_off": ("dxb", "dwf"),
           "no_flip": ("dxb",), "tail_leak": ("pre", "br"), "tail_grad": ("dxb",), "wgrad_last_frame": ("dwf",)}


def _mutated(emulated, shape, mutation):
    s, ref_p = emulated[shape][0], emulated[shape][1]
    return PC.stage_metrics_p(PC.stage_emulation_p(*PC.p_args(s), mutate=mutation), ref_p, s["frames"])


@pytest.mark.parametrize("mutation", PC.MUTATIONS_P)
def test_bars_reject_composition_mistakes(emulated, mutation):
    """Each mutated stage is over the bar (rel-L2 and max) on every tensor the mistake touches.  The tap mistake is asserted at T = 199 with
    K = 128 and at K = 16; the two tail mistakes need padded rows, so they are asserted on the variable-length shapes."""
    assert set(TOUCHES) == set(PC.MUTATIONS_P)
    if mutation in ("tail_leak", "tail_grad"):
        shapes = [sh for sh in EMU_SHAPES if sh[3] is not None]
    elif mutation == "drop_last_tap":
        shapes = [(2, 128, 199, None), (2, 16, 18, None), (4, 16, 18, None), (2, 128, 199, VL_K128)]
    else:
        shapes = [(2, 128, 18, None), (2, 128, 199, None), (2, 16, 18, None), (4, 16, 18, None), (2, 128, 199, VL_K128)]
    assert len(shapes) >= 2
    for shape in shapes:
        m = _mutated(emulated, shape, mutation)
        for kind in TOUCHES[mutation]:
            for suffix in ("_l2", "_max"):
                print("%s %s %s%s: %.3e (bar %.3e)" % (mutation, shape, kind, suffix, m[kind + suffix], PC.BARS[kind + suffix]))
                assert m[kind + suffix] > PC.BARS[kind + suffix], (mutation, shape, kind + suffix, m[kind + suffix])


def test_a_short_clip_cannot_see_the_outer_taps(emulated):
    """Output frame t reads input t + j - K // 2, so tap K - 1 = 127 needs T >= 65: at T = 18 the stage without it is the same stage, to
    the last bit of every metric.  Why the k128 cases carry clips of 199 frames and more."""
    shape = (2, 128, 18, None)
    s, ref_p, emu_p = emulated[shape][:3]
    base = PC.stage_metrics_p(emu_p, ref_p, s["frames"])
    assert _mutated(emulated, shape, "drop_last_tap") == base
    long = _mutated(emulated, (2, 128, 199, None), "drop_last_tap")
    assert long["pre_l2"] > 10 * PC.BARS["pre_l2"]
