"""Variable-length scoring batches on the AASIST back-end, the parts that need no GPU: the host-side node counts against the shapes the
oracle's own layers produce; the frame limits against the oracle and the kernels' constants; the DEFINITION of the masked forward — an fp64
restatement written here on the oracle's state-dict names (every convolution input zeroed by selection at and beyond an utterance's
columns, the attention pooling and the graph module on the utterance's own columns / nodes) against oracle/aasist_head.AasistHead on each
utterance alone, and the same with the masks removed to show the comparison can fail; the refusals with the switch off and on; the data
path's cut at the model's maximum; the new entry points refusing bad arguments.  The header / ctypes agreement is tests/test_abi.py's."""
import ctypes
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import aasist_head as OH
from oracle.aasist import fill_state
from scl_amd import aasist_head as AH
from scl_amd import graph, lib, pack, resstack

FRAMES = [3, 5, 6, 61, 199, 200, 201, 242, 100, 8]      # both T = 3 W + 2 cases, one and two temporal nodes, the limit
TEMPS = OH.UPSTREAM_AASIST["temperatures"]


# ---- counts and limits ----------------------------------------------------------------------------------------------------------------
def test_node_counts_are_the_shapes_the_oracle_layers_produce():
    pr = OH.UPSTREAM_AASIST["pool_ratios"]
    kept = lambda n, k: OH.GraphPool(k, 4, 0.3).eval()(torch.zeros(1, n, 4)).shape[1]
    with torch.no_grad():
        nS = F.max_pool2d(torch.zeros(1, 1, 128, 3), (3, 3)).shape[2]
        kS = kept(nS, pr[0])
        kS2 = kept(kS, pr[2])
        for T in range(3, 243):
            c = AH.node_counts([T])
            W = F.max_pool2d(torch.zeros(1, 1, 128, T), (3, 3)).shape[3]
            kT = kept(W, pr[1])
            kT2 = kept(kT, pr[2])
            assert (c["W"], c["kT"], c["kT2"], c["N1"], c["N2"]) == ([W], [kT], [kT2], [kT + kS], [kT2 + kS2]), T
            assert (c["nS"], c["kS"], c["kS2"]) == (nS, kS, kS2) == (42, 21, 10)
    batch = AH.node_counts(FRAMES)
    assert batch["W"] == [1, 1, 2, 20, 66, 66, 67, 80, 33, 2] and batch["kT"] == [1, 1, 1, 10, 33, 33, 33, 40, 16, 1]
    assert batch["kT2"] == [1, 1, 1, 5, 16, 16, 16, 20, 8, 1]


def _oracle(dtype=torch.float64, seed=3):
    ref = OH.AasistHead().to(dtype).eval()
    sd = fill_state({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k: torch.from_numpy(v).to(ref.state_dict()[k].dtype) for k, v in sd.items()})
    return ref


def test_min_frames_is_the_smallest_the_oracle_runs_and_the_limits_follow_the_kernels():
    ref = _oracle(torch.float32)

    def runs(T):
        try:
            with torch.no_grad():
                return bool(torch.isfinite(ref(torch.zeros(1, T, 128))[0]).all())
        except RuntimeError:
            return False
    assert AH.min_frames() == 3 and runs(3) and not runs(2) and not runs(1)
    # the limits come from the kernels' constants: 80 nodes in a homogeneous layer, kS + kT <= 64, maps up to resstack.MAX_W wide
    assert (graph.MAX_NODES, graph.MAX_HTRG_NODES, resstack.MAX_W) == (80, 64, 93)
    assert AH.max_nodes() == 80 and AH.max_frames() == 242
    assert AH.node_counts([AH.max_frames()])["N1"][0] <= graph.MAX_HTRG_NODES
    assert AH.max_nodes({"pool_ratios": [0.5, 0.8, 0.5, 0.5]}) == 54      # 21 + int(54 * 0.8) = 64
    assert AH.max_nodes({"pool_ratios": [1.0, 0.5, 0.5, 0.5]}) == 45      # 42 + int(45 * 0.5) = 64


def test_max_samples_follows_head_max_frames_through_samples_for():
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_aasist import Model
    from scl_amd.model_front import FrontHeadModel
    m = Model.__new__(Model)      # the limits read the configuration alone: no device, no parameters
    m.__dict__.update(cfg=W2VConfig(), pool_cfg={"pool_ratios": [0.5, 0.5, 0.5, 0.5]})
    assert m.head_min_frames() == 3 and m.head_max_frames() == 242
    assert FrontHeadModel.min_samples(m) == W2VConfig().samples_for(3) == 1040
    assert FrontHeadModel.max_samples(m) == W2VConfig().samples_for(243) - 1 == 77839
    assert W2VConfig().conv_lens(77839)[-1] == 242 and W2VConfig().conv_lens(77840)[-1] == 243
    plain = FrontHeadModel.__new__(FrontHeadModel)
    plain.__dict__.update(cfg=W2VConfig())
    assert plain.head_max_frames() is None and FrontHeadModel.max_samples(plain) == pack.VARLEN_MAX_SAMPLES


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def _bn(t, name, x):
    return F.batch_norm(x, t[name + ".running_mean"], t[name + ".running_var"], t[name + ".weight"], t[name + ".bias"], False, 0.1, 1e-5)


def _lin(t, name, x):
    return F.linear(x, t[name + ".weight"], t[name + ".bias"])


def _bn_nodes(t, name, y):
    return _bn(t, name, y.reshape(-1, y.shape[-1])).view_as(y)


def _gat(t, p, x, temp):
    att = torch.tanh(_lin(t, p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1))) @ t[p + "att_weight"]
    att = F.softmax(att / temp, dim=-2).squeeze(-1)
    return F.selu(_bn_nodes(t, p + "bn", _lin(t, p + "proj_with_att", att @ x) + _lin(t, p + "proj_without_att", x)))


def _htrg(t, p, x1, x2, master, temp):
    n1 = x1.shape[1]
    x = torch.cat([_lin(t, p + "proj_type1", x1), _lin(t, p + "proj_type2", x2)], dim=1)
    h = torch.tanh(_lin(t, p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1)))
    first = torch.arange(x.shape[1]) < n1
    same = first[:, None] == first[None, :]
    a = torch.where(same[..., None], torch.where(first[:, None, None], t[p + "att_weight11"][:, 0], t[p + "att_weight22"][:, 0]), t[p + "att_weight12"][:, 0])
    att = F.softmax((h * a).sum(-1) / temp, dim=-1)      # the board is symmetric in its type pattern: soft-max over the second node index
    am = F.softmax(torch.tanh(_lin(t, p + "att_projM", x * master)) @ t[p + "att_weightM"] / temp, dim=-2)
    m_out = _lin(t, p + "proj_with_attM", am.transpose(1, 2) @ x) + _lin(t, p + "proj_without_attM", master)
    y = F.selu(_bn_nodes(t, p + "bn", _lin(t, p + "proj_with_att", att @ x) + _lin(t, p + "proj_without_att", x)))
    return y[:, :n1], y[:, n1:], m_out


def _pool(t, p, h, keep):
    s = torch.sigmoid(_lin(t, p + "proj", h))
    idx = torch.topk(s, keep, dim=1)[1].expand(-1, -1, h.shape[2])
    return torch.gather(h * s, 1, idx)


def _graph(t, e_S, e_T, kS, kT, kS2, kT2):
    out_S = _pool(t, "pool_S.", _gat(t, "GAT_layer_S.", e_S, TEMPS[0]), kS)
    out_T = _pool(t, "pool_T.", _gat(t, "GAT_layer_T.", e_T, TEMPS[1]), kT)
    res = []
    for l1, l2, pS, pT, m in (("HtrgGAT_layer_ST11.", "HtrgGAT_layer_ST12.", "pool_hS1.", "pool_hT1.", "master1"),
                              ("HtrgGAT_layer_ST21.", "HtrgGAT_layer_ST22.", "pool_hS2.", "pool_hT2.", "master2")):
        tt, ss, mm = _htrg(t, l1, out_T, out_S, t[m], TEMPS[2])
        ss, tt = _pool(t, pS, ss, kS2), _pool(t, pT, tt, kT2)
        ta, sa, ma = _htrg(t, l2, tt, ss, mm, TEMPS[2])
        res.append((tt + ta, ss + sa, mm + ma))
    T_, S_, M_ = (torch.max(res[0][i], res[1][i]) for i in range(3))
    hid = torch.cat([T_.abs().max(dim=1)[0], T_.mean(dim=1), S_.abs().max(dim=1)[0], S_.mean(dim=1), M_.squeeze(1)], dim=1)
    return _lin(t, "out_layer", hid), hid


def _masked_forward(t, feats, frames, masks=True):
    """The definition: the oracle head in eval mode on the zero-padded batch with (a) every convolution input — the stack input behind first_bn +
    SELU, every selu(bn2(conv1(x))), every block output — set to zero by selection at the map columns >= W_b, (b) the attention pooling's
    soft-max over time and both sums over the columns < W_b, (c) the graph module on the first W_b temporal nodes with the utterance's own
    GraphPool counts.  masks=False: the same code without (a), (b), (c) — the padded batch as the fixed-length forward would take it."""
    cnt = AH.node_counts(frames)
    Wmax = max(cnt["W"])
    W = torch.tensor(cnt["W"])

    def mask(x):
        if not masks:
            return x
        keep = torch.arange(x.shape[3])[None, :] < W[:, None]
        return torch.where(keep[:, None, None, :], x, torch.zeros((), dtype=x.dtype))
    conv = lambda x, p, pad: F.conv2d(x, t[p + ".weight"], t[p + ".bias"], padding=pad)
    x = feats[:, :3 * Wmax].transpose(1, 2).unsqueeze(1)
    x = mask(F.selu(_bn(t, "first_bn", F.max_pool2d(x, (3, 3)))))
    for i in range(6):
        p = "encoder.%d.0." % i
        a = mask(F.selu(_bn(t, p + "bn2", conv(x, p + "conv1", (1, 1)))))
        idn = conv(x, p + "conv_downsample", (0, 1)) if (p + "conv_downsample.weight") in t else x
        x = mask(conv(a, p + "conv2", (0, 1)) + idn)
    x = F.selu(_bn(t, "first_bn1", x))
    w = conv(_bn(t, "attention.2", F.selu(conv(x, "attention.0", 0))), "attention.3", 0)
    outs = []
    for b in range(len(frames)):
        n = cnt["W"][b] if masks else Wmax
        xb, wb = x[b:b + 1, :, :, :n], w[b:b + 1, :, :, :n]
        e_S = (xb * F.softmax(wb, dim=-1)).sum(-1).transpose(1, 2) + t["pos_S"]
        e_T = (xb * F.softmax(wb, dim=-2)).sum(-2).transpose(1, 2)
        one = cnt if masks else AH.node_counts([3 * Wmax] * len(frames))
        outs.append(_graph(t, e_S, e_T, cnt["kS"], one["kT"][b], cnt["kS2"], one["kT2"][b]) + (e_S, e_T))
    return outs


@pytest.fixture(scope="module")
def definition_case():
    ref = _oracle()
    t = {k: v for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(100)
    T = max(FRAMES) + 9      # the padded length does not size anything
    feats = torch.zeros(len(FRAMES), T, 128, dtype=torch.float64)
    for b, n in enumerate(FRAMES):
        feats[b, :n] = torch.randn(n, 128, generator=g, dtype=torch.float64)
    with torch.no_grad():
        alone = [ref(feats[b:b + 1, :n]) for b, n in enumerate(FRAMES)]
    return t, feats, alone


def _worst(outs, alone):
    worst = 0.0
    for (lo, hid, _, _), (rl, rh) in zip(outs, alone):
        worst = max(worst, (lo - rl).abs().max().item(), (hid - rh).abs().max().item())
    return worst


def test_the_masked_definition_equals_the_oracle_on_each_utterance_alone(definition_case):
    t, feats, alone = definition_case
    junk = feats.clone()
    for b, n in enumerate(FRAMES):
        junk[b, n:] = 1e3 * torch.randn(junk.shape[1] - n, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(b))
    with torch.no_grad():
        worst = _worst(_masked_forward(t, junk, FRAMES), alone)
    print("masked definition against the oracle alone: %.2e" % worst)
    assert worst < 1e-10


def test_without_the_masks_the_comparison_fails(definition_case):
    t, feats, alone = definition_case
    with torch.no_grad():
        worst = _worst(_masked_forward(t, feats, FRAMES, masks=False), alone)      # zero padding, as a fixed-length forward takes the batch
    print("without the masks: %.2e" % worst)
    assert worst > 1e-3


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _main_args(tmp_path, monkeypatch):
    import yaml
    cfg = {"model": {"name": "wav2vec2_aasist", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "eval_only", "kwargs": {}}}
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # the refusal comes before anything touches a device
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    return ["--config", str(tmp_path / "conf.yaml"), "--database_path", str(tmp_path), "--eval", "--padding_type", "none",
            "--eval_output", str(tmp_path / "x.txt")]


def test_switch_off_main_and_the_plugin_refuse_as_before(tmp_path, monkeypatch):
    import main as M
    from scl_amd.model_aasist import Model
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    assert M.VARLEN_MODELS == ("wav2vec2_linear_nll", "wav2vec2_resnet_nll") and "wav2vec2_aasist" in M.VARLEN_SCORING_OPT_IN
    with pytest.raises(SystemExit) as e:
        M.main(_main_args(tmp_path, monkeypatch))
    msg = str(e.value)
    assert "wav2vec2_linear_nll only" in msg and "wav2vec2_resnet_nll" in msg and "wav2vec2_aasist" in msg and "SCL_AASIST_LENGTHS=1" in msg
    m = Model.__new__(Model)
    assert m.head_takes_frames is False
    with pytest.raises(NotImplementedError) as e:
        m.forward(torch.zeros(1, 4000), lengths=[4000])
    msg = str(e.value)
    assert "wav2vec2_linear_nll" in msg and "wav2vec2_resnet_nll" in msg and "no padding mask" in msg and "SCL_AASIST_LENGTHS=1" in msg
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "0")
    assert m.head_takes_frames is False


def test_switch_on_main_passes_its_start_up_check(tmp_path, monkeypatch):
    import main as M

    class Reached(Exception):
        pass

    def build(*a, **k):
        raise Reached()
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    monkeypatch.setitem(M.MODEL_REGISTRY, "wav2vec2_aasist", build)      # the model is the first thing behind the start-up checks
    with pytest.raises(Reached):
        M.main(_main_args(tmp_path, monkeypatch))
    from scl_amd.model_aasist import Model
    assert Model.__new__(Model).head_takes_frames is True
    # the switch never routes this plugin into --padding_type zero --batch_size k training
    assert "wav2vec2_aasist" not in M.VARLEN_MODELS


def test_forward_frames_refuses_train_mode_autograd_and_frames_outside_the_limits():
    head = AH.AasistHead()
    feats = torch.zeros(2, 250, 128)
    head.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        head.forward_frames(feats, [100, 100])
    head.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):      # autograd on
        head.forward_frames(feats, [100, 100])
    with torch.no_grad():
        with pytest.raises(ValueError, match="3..250"):
            head.forward_frames(feats, [100, 2])
        with pytest.raises(ValueError, match="exceeds the 242 frames"):
            head.forward_frames(feats, [243, 100])
        with pytest.raises(ValueError):
            head.forward_frames(feats, [100])                    # one count per row
        with pytest.raises(ValueError):
            head.forward_frames(feats[:, :90], [100, 50])        # more frames than the batch has
        small = AH.AasistHead(dict(AH.UPSTREAM_AASIST, gat_dims=[48, 32]))      # shapes the fused graph module does not take
        small.eval()
        assert not small.frames_supported() and head.frames_supported()
        with pytest.raises(NotImplementedError, match="fused"):
            small.forward_frames(feats, [100, 100])


def test_fused_switch_off_refuses_lengths(monkeypatch):
    head = AH.AasistHead().eval()
    monkeypatch.setattr(AH, "FUSED_STACK", False)      # what SCL_AASIST_FUSED=0 sets at import
    with torch.no_grad(), pytest.raises(NotImplementedError, match="SCL_AASIST_FUSED=0"):
        head.forward_frames(torch.zeros(1, 30, 128), [30])


def test_eval_dataset_cuts_a_long_file_to_max_samples_and_counts_it(tmp_path):
    path = tmp_path / "long.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(0.1 * np.random.RandomState(0).randn(3000), -1, 1) * 32767).astype("<i2").tobytes())
    ds = pack.EvalDataset(["long.wav"], str(tmp_path), padding_type="none", subdir="")
    assert ds.max_samples == pack.VARLEN_MAX_SAMPLES and ds.n_cut == 0
    x, _ = ds[0]
    assert x.shape == (3000,) and ds.n_cut == 0
    ds.max_samples = 2000
    x2, _ = ds[0]
    assert x2.shape == (2000,) and torch.equal(x2, x[:2000]) and ds.n_cut == 1


# ---- entry points -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # a 16-byte aligned host address: a refused call never dereferences it
    odd = ctypes.c_void_p(p.value + 4)
    err = lambda: L.scl_last_error()
    geom = lambda **kw: lib.SclRsGeom(kw.get("B", 2), kw.get("H", 42), kw.get("W", 16), kw.get("r_lo", 1), kw.get("r_hi", 42), 0)
    bad_geoms = [dict(B=0), dict(H=0), dict(W=0), dict(r_lo=-1), dict(r_hi=44), dict(r_lo=5, r_hi=4), dict(B=1 << 20, W=80)]

    def conv(widths=p, g=None, **kw):
        d = lib.SclRsConv()
        d.inp, d.wpk, d.out = kw.get("inp", p.value), kw.get("wpk", p.value), kw.get("out", p.value)
        d.geom = g or geom()
        d.cin, d.cout, d.ntaps, d.stat_mode = kw.get("cin", 32), kw.get("cout", 64), kw.get("ntaps", 6), kw.get("stat_mode", 0)
        return L.scl_rs_conv_w(ctypes.byref(d), widths, None)
    for rc in [conv(widths=None), conv(inp=None), conv(wpk=None), conv(out=None), conv(stat_mode=1), conv(ntaps=4), conv(cin=64, cout=32), conv(cin=48),
               conv(inp=odd.value), conv(g=geom(W=94))] + [conv(g=geom(**kw)) for kw in bad_geoms]:
        assert rc == -1 and b"scl_rs_conv_w" in err(), err()
    assert L.scl_rs_conv_w(None, p, None) == -1 and b"scl_rs_conv_w" in err()

    bn = lambda y=p, stats=p, a=p, C=64, act=1, g=None, widths=p: L.scl_rs_bn_act_w(y, stats, a, C, act, ctypes.byref(g or geom()), widths, None)
    for rc in [bn(y=None), bn(stats=None), bn(a=None), bn(widths=None), bn(C=0), bn(C=6), bn(act=2), bn(y=odd)] + [bn(g=geom(**kw)) for kw in bad_geoms]:
        assert rc == -1 and b"scl_rs_bn_act_w" in err(), err()
    assert L.scl_rs_bn_act_w(p, p, p, 64, 1, None, p, None) == -1 and b"scl_rs_bn_act_w" in err()

    cp = lambda src=p, dst=p, Cs=1, Cd=16, sw=16, g=None, widths=p: L.scl_rs_copy_w(src, dst, Cs, Cd, sw, ctypes.byref(g or geom()), widths, None)
    for rc in [cp(src=None), cp(dst=None), cp(widths=None), cp(Cs=0), cp(Cs=32), cp(sw=0), cp(sw=17)] + [cp(g=geom(**kw)) for kw in bad_geoms]:
        assert rc == -1 and b"scl_rs_copy_w" in err(), err()

    ap = lambda x=p, l=p, pos=p, eS=p, eT=p, C=64, g=None, widths=p: L.scl_rs_attn_pool_fwd_w(x, l, pos, eS, eT, C, ctypes.byref(g or geom()), widths, None)
    for rc in [ap(x=None), ap(l=None), ap(eS=None), ap(eT=None), ap(widths=None), ap(C=0), ap(C=6), ap(x=odd), ap(g=geom(H=200, W=90, r_hi=200))] + \
              [ap(g=geom(**kw)) for kw in bad_geoms]:
        assert rc == -1 and b"scl_rs_attn_pool_fwd_w" in err(), err()

    sc = lambda x=p, W=p, bias=p, a=p, s=p, nodes=p, n1=None, B=2, N=80, D=64, Do=64: L.scl_gat_score_fwd_var(x, W, bias, a, s, nodes, n1, B, N, D, Do, None)
    for rc in (sc(x=None), sc(W=None), sc(bias=None), sc(a=None), sc(s=None), sc(nodes=None), sc(B=0), sc(N=0), sc(N=129), sc(D=48), sc(D=32, Do=64), sc(Do=16)):
        assert rc == -1 and b"scl_gat_score_fwd_var" in err(), err()

    lay = (lib.SclGraphLayer * 2)()
    for i in range(2):
        lay[i].N, lay[i].D, lay[i].Do = 80, 64, 64
        for f in ("xd", "S", "g", "y", "Wa", "ba", "Wb", "bb"):
            setattr(lay[i], f, p.value)
        lay[i].bn.stats = p.value
    post = lambda layers=lay, n=2, t0=p, t1=p, B=2: L.scl_graph_post_fwd_var(layers, n, t0, t1, B, None)
    assert post(layers=None) == -1 and b"scl_graph_post_fwd_var" in err()
    for rc in (post(n=0), post(n=3), post(B=0), post(t0=None, t1=None)):
        assert rc == -1 and b"scl_graph_post_fwd_var" in err(), err()
    for field, value in (("N", 0), ("N", 97), ("D", 48), ("Do", 16), ("xd", None), ("S", None)):
        keep = getattr(lay[1], field)
        setattr(lay[1], field, value)
        assert post() == -1 and b"scl_graph_post_fwd_var" in err(), field
        setattr(lay[1], field, keep)
    lay[0].bn.training = 1
    assert post() == -1 and b"scoring" in err() and b"scl_graph_post_fwd_var" in err()
    lay[0].bn.training = 0
    lay[0].has_master = 1      # a heterogeneous layer holds at most 64 nodes
    assert post() == -1 and b"scl_graph_post_fwd_var" in err()

    pre = (lib.SclGraphPre * 2)()
    for i in range(2):
        pre[i].Dp, pre[i].N = 64, 61
        pre[i].u[0].n_in, pre[i].u[0].K, pre[i].u[0].row_out = 80, 40, 0
        pre[i].u[1].n_in, pre[i].u[1].K, pre[i].u[1].row_out = 42, 21, 40
    prf = lambda inst=pre, t_in=p, t_keep=p, B=2: L.scl_graph_pre_fwd_var(inst, 1, t_in, t_keep, B, None)
    for rc in (prf(inst=None), prf(t_in=None), prf(t_keep=None), prf(B=0)):
        assert rc == -1 and b"scl_graph_pre_fwd_var" in err(), err()
    for unit, field, value in ((0, "n_in", 97), (0, "K", 0), (1, "K", 43), (1, "row_out", 39)):
        keep = getattr(pre[0].u[unit], field)
        setattr(pre[0].u[unit], field, value)
        assert prf() == -1 and b"scl_graph_pre_fwd_var" in err(), field
        setattr(pre[0].u[unit], field, keep)
    pre[1].in_p = 0.2
    assert prf() == -1 and b"no dropout" in err() and b"scl_graph_pre_fwd_var" in err()

    fin = lib.SclGraphFinal()
    fin.KT, fin.KS, fin.D, fin.NC = 20, 10, 32, 2
    ff = lambda f=fin, kt=p, B=2: L.scl_graph_final_fwd_var(None if f is None else ctypes.byref(f), kt, B, None)
    for rc in (ff(f=None), ff(kt=None), ff(B=0)):
        assert rc == -1 and b"scl_graph_final_fwd_var" in err(), err()
    for field, value in (("KT", 0), ("KS", 0), ("D", 0), ("D", 64), ("NC", 0), ("NC", 9), ("way_p", 0.2), ("drop_p", 0.5)):
        keep = getattr(fin, field)
        setattr(fin, field, value)
        assert ff() == -1 and b"scl_graph_final_fwd_var" in err(), field
        setattr(fin, field, keep)
