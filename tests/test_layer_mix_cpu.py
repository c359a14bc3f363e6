"""The layer mix without a GPU: the YAML switch, the parameter layout, the cap on the number of hidden states, and the definition of
tests/layer_mix_cases.py against transformers' `output_hidden_states` and against the oracle's encoder output."""
import pytest
import torch

from scl_amd.encoder import MIX_WEIGHT, W2VConfig, mix_specs, param_specs, w2v_config_from
from scl_amd.lib import SclError
from scl_amd.model_linear import head_specs
from scl_amd.params import FlatParams
from oracle import wav2vec2 as W
from tests import layer_mix_cases as LM


def test_yaml_key_and_mapping_form_switch_the_mix():
    assert W2VConfig().layer_mix is False and w2v_config_from({}).layer_mix is False
    assert w2v_config_from({"ssl_layer_mix": False}).layer_mix is False
    for arch in ("xlsr_300m", "xlsr_1b", "tiny"):
        off, on = w2v_config_from({"w2v_arch": arch}), w2v_config_from({"w2v_arch": arch, "ssl_layer_mix": True, "encoder_layerdrop": 0.1})
        assert on.layer_mix is True and off.layer_mix is False
        assert (on.embed, on.layers, on.heads, on.ffn, on.pos_k) == (off.embed, off.layers, off.heads, off.ffn, off.pos_k)
    assert w2v_config_from({"w2v_arch": "xlsr_1b", "ssl_layer_mix": True, "encoder_layerdrop": 0.1}).encoder_layerdrop == 0.1
    small = {"embed": 128, "layers": 3, "heads": 2, "ffn": 256}
    assert w2v_config_from({"w2v_arch": small}).layer_mix is False
    assert w2v_config_from({"w2v_arch": small, "ssl_layer_mix": True}).layer_mix is True
    assert w2v_config_from({"w2v_arch": dict(small, layer_mix=True)}).layer_mix is True
    assert w2v_config_from({"w2v_arch": dict(small, layer_mix=False), "ssl_layer_mix": True}).layer_mix is False      # the mapping's own field wins


def test_parameter_sits_behind_LL_bias_and_moves_no_earlier_offset():
    off_cfg = W2VConfig.tiny()
    on_cfg = off_cfg.with_layer_mix()
    assert mix_specs(off_cfg) == [] and mix_specs(on_cfg) == [(MIX_WEIGHT, (off_cfg.layers + 1,), True)]
    assert param_specs(on_cfg) == param_specs(off_cfg)      # not an encoder tensor: checkpoints of the encoder stay complete
    off = FlatParams(param_specs(off_cfg) + head_specs(off_cfg.embed, mix_specs(off_cfg)), "cpu")
    on = FlatParams(param_specs(on_cfg) + head_specs(on_cfg.embed, mix_specs(on_cfg)), "cpu")
    assert MIX_WEIGHT not in off.index and on.index[MIX_WEIGHT][2] == (3,) and on.index[MIX_WEIGHT][3]
    assert [n for n in on.index if n != MIX_WEIGHT] == list(off.index)
    names = list(on.index)
    assert names[names.index(MIX_WEIGHT) - 1] == "LL.bias" and on.off(MIX_WEIGHT) == on.off("LL.bias") + 128
    assert on.off(MIX_WEIGHT) < on.n_train and on.off(MIX_WEIGHT) > on.off("LL.weight")      # in the trainable range, frozen encoder or not
    shift = on.off("backend.m_frame_level.0.weight") - off.off("backend.m_frame_level.0.weight")
    assert shift == 8      # 3 logits in a slot aligned to 8 elements
    for n, (o, cnt, shape, tr) in off.index.items():
        later = o >= off.off("backend.m_frame_level.0.weight")
        assert on.index[n] == (o + (shift if later else 0), cnt, shape, tr), n
    assert head_specs(off_cfg.embed) == head_specs(off_cfg.embed, mix_specs(off_cfg))


def test_more_than_64_hidden_states_are_refused_at_construction():
    assert W2VConfig(layers=63, layer_mix=True).layers == 63
    assert W2VConfig(layers=64).layers == 64      # without the mix there is no cap
    with pytest.raises((SclError, ValueError), match="64"):
        W2VConfig(layers=64, layer_mix=True)
    with pytest.raises((SclError, ValueError), match="64"):
        w2v_config_from({"w2v_arch": {"layers": 70}, "ssl_layer_mix": True})
    with pytest.raises((SclError, ValueError), match="64"):
        W2VConfig(layers=64).with_layer_mix()


def test_definition_states_equal_transformers_hidden_states():
    transformers = pytest.importorskip("transformers")
    cfg = W.W2VConfig.tiny()
    sd = W.init_state(cfg, seed=5)
    hf_cfg = transformers.Wav2Vec2Config(
        hidden_size=cfg.embed, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, intermediate_size=cfg.ffn,
        conv_dim=[cfg.conv_dim] * len(cfg.conv_kernels), conv_kernel=list(cfg.conv_kernels), conv_stride=list(cfg.conv_strides),
        conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True, num_conv_pos_embeddings=cfg.pos_k,
        num_conv_pos_embedding_groups=cfg.pos_groups, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
        feat_proj_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0, hidden_act="gelu", layer_norm_eps=1e-5)
    hf = transformers.Wav2Vec2Model(hf_cfg).eval()
    missing, unexpected = hf.load_state_dict(W.to_hf_state(sd, cfg), strict=False)
    assert not missing and set(unexpected) <= {"masked_spec_embed"}, (missing, unexpected)      # no masking configured: no mask embedding
    x = 0.1 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ours = LM.hidden_states(sd, cfg, x)
        theirs = hf(x, output_hidden_states=True).hidden_states
    assert len(ours) == len(theirs) == cfg.layers + 1
    for l, (a, b) in enumerate(zip(ours, theirs)):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item(), l      # fp32 round-off of two implementations of the same graph


def test_one_hot_on_the_last_state_is_the_encoder_output():
    cfg = W.W2VConfig.tiny()
    sd = W.init_state(cfg, seed=6)
    x = 0.1 * torch.randn(3, 2500, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        states = LM.hidden_states(sd, cfg, x)
        onehot = torch.zeros(cfg.layers + 1)
        onehot[-1] = 1.0
        assert torch.equal(LM.mix_of(states, weights=onehot), W.forward(sd, cfg, x))
        # the logits the model test uses give exactly that soft-max in f32
        logits = torch.full((cfg.layers + 1,), -1e4)
        logits[-1] = 0.0
        assert torch.equal(torch.softmax(logits, 0), onehot)
        # a skipped last layer: its input is handed on
        skipped = LM.hidden_states(sd, cfg, x, skip_last=True)
        assert torch.equal(skipped[-2], states[-2]) and not torch.equal(skipped[-1], states[-1])
