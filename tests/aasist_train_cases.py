"""float64 references and case tables for the train-mode BatchNorm with the mask on the COLUMNS of a zero-padded batch [B, H, W, C] (utterance
b owns the columns w < widths[b] of every row: the AASIST stack's ragged axis), scl_bn_fwd_cols / scl_bn_bwd_cols.
tests/test_aasist_varlen_train_cpu.py pins the reference against torch autograd on the compact tensor, tests/test_aasist_train_kernels_gpu.py
compares the kernels with it.  Further down: the node lists and float64 references of the node-side backward kernels
(scl_gat_score_bwd_var, scl_gat_softmax_agg_var_bwd).  Nothing here imports product code.

The column mask of x is the row mask of x.transpose(1, 2) ([B, W, H, C], utterance b owns its first widths[b] rows), and a BatchNorm does not
care in which order it meets its positions: the reference is tests/masked_train_cases.masked_bn_reference on the transposed map, transposed back."""
import torch

from tests import masked_train_cases as MC
from tests import nn_cases as NC

ACTS = (NC.ACT_NONE, NC.ACT_SELU)

# (B, H, W, C, widths): C = 1 scalar path (first_bn's single-channel map) / C % 4 == 0 16-byte path; an utterance without a column, with one,
# with all; 42 x 70 and 42 x 33 own positions are several 128-position slabs per utterance, both ending inside one; C = 128 (attention.2)
COLS_BN_CASES = [
    (3, 5, 9, 1, [9, 1, 4]),
    (4, 42, 12, 32, [12, 1, 7, 0]),
    (2, 42, 70, 64, [70, 33]),
    (2, 3, 8, 128, [8, 5]),
]


def case_id(c):
    return "B%d-H%d-W%d-C%d" % c[:4]


def keep_cols(widths, W):
    """bool [B, W]: column w belongs to utterance b."""
    return torch.arange(W)[None, :] < torch.as_tensor(widths)[:, None]


def keep_map(widths, H, W):
    """bool [B, H, W]."""
    return keep_cols(widths, W)[:, None, :].expand(len(widths), H, W)


def cols_bn_reference(x, gamma, beta, running_mean, running_var, widths, momentum, eps, act, dy):
    """-> MC.MaskedBNRef on the [B, H, W, C] layout: statistics over the N_v = H * sum(widths) own positions, y and dx exactly 0 at and beyond
    widths[b].  x / dy may hold anything (NaN included) there."""
    r = MC.masked_bn_reference(x.transpose(1, 2), gamma, beta, running_mean, running_var, widths, momentum, eps, act, dy.transpose(1, 2))
    return r._replace(y=r.y.transpose(1, 2).contiguous(), dx=r.dx.transpose(1, 2).contiguous())


def cols_bn_inputs(B, H, W, C, widths, act, fill=float("nan")):
    """NC.bn_inputs on the N_v own positions, scattered into the padded map in (b, h, w) order; x and dy hold `fill` at and beyond widths[b].
    -> MC.MaskedBNInputs (compact: the BNInputs the own positions came from)."""
    n = H * sum(widths)
    inp = NC.bn_inputs(C, n, act)
    x, dy = torch.full((B, H, W, C), fill), torch.full((B, H, W, C), fill)
    o = 0
    for b, w in enumerate(widths):
        x[b, :, :w] = inp.x[o:o + H * w].view(H, w, C)
        dy[b, :, :w] = inp.dy[o:o + H * w].view(H, w, C)
        o += H * w
    return MC.MaskedBNInputs(x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, inp.nbt.clone(), dy, inp.prior_dgamma, inp.prior_dbeta, inp)


# ---- the node side: pair-score backward and soft-max + aggregation backward on graphs of different sizes -------------------------------
# nodes per utterance: both sides of the 128-node change of kernel form and of a 128-row j tile, a 16-pair block with one pair, one node
NODES_TILED, N1_TILED = [257, 130, 129, 128, 17, 1], [128, 130, 0, 100, 5, 1]
NODES_WHOLE, N1_WHOLE = [128, 100, 17, 1], [100, 100, 5, 0]
GAT_WIDTHS = ((64, 64), (64, 32), (32, 32))
GRAD_BAR = 1e-4          # of the tensor's maximum; else 4 x what the fp32 torch formulation loses on the same inputs (tests/test_gat_long_gpu.py)


def ref_score(x, W, bias, a, n1):
    """tests/test_gat_gpu.py::ref_score on one utterance x [N, D]: s [N, N]."""
    pair = x.unsqueeze(1) * x.unsqueeze(0)
    h = torch.tanh(torch.nn.functional.linear(pair, W, bias))
    if a.shape[0] == 1:
        return h @ a[0]
    first = torch.arange(x.shape[0], device=x.device) < n1
    same = first[:, None] == first[None, :]
    pick = torch.where(same, torch.where(first[:, None], 0, 1), 2)          # [N, N]: 0 both first, 1 both second, 2 mixed
    return (h * a[pick]).sum(-1)


def agg_reference(s, x, dout, temp):
    """Closed form in float64 on one utterance: s [N, N] (or [1, N]), x [N, D], dout [N, D] (or [1, D]) -> (out, ds, dx) of
    out = softmax(s / temp, -1) @ x."""
    s, x, dout = s.double(), x.double(), dout.double()
    p = torch.exp(s / temp - (s / temp).max(-1, keepdim=True)[0])
    p = p / p.sum(-1, keepdim=True)
    dp = dout @ x.t()
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) / temp
    return p @ x, ds, p.t() @ dout


# ---- the DEFINITION of the train-mode AASIST back-end on a zero-padded batch ---------------------------------------------------------------
# Every utterance goes through every layer on its OWN compact tensors (map [1, C, 42, W_b], graphs of its own node counts): a convolution's
# zero border is then what "every convolution input is zero at and beyond W_b" means, and soft-maxes, GraphPool and the read-out see the own
# columns and nodes only.  What couples the utterances is each BatchNorm: mean and biased variance over the CONCATENATION of all utterances'
# own positions, running statistics moved with the unbiased N_v / (N_v - 1), num_batches_tracked + 1.  Dropout is p = 0.
TEMPS = (2.0, 2.0, 100.0, 100.0)
TOPK_MARGIN = 1e-5


def masked_train_forward(t, feats, frames, record=None):
    """t: {oracle state-dict name: tensor} (parameters may require grad; the running statistics are updated in place), feats [B, T, 128],
    frames: ints.  Rows of feats at and beyond 3 * (frames[b] // 3) are never read.  record: a dict that receives, per BatchNorm name,
    (mean, biased variance, N_v, the concatenated input [N_v, C]) and under "margins" every GraphPool's top-k gap per utterance.
    -> (logits [B, 2], last_hidden [B, 160])."""
    import torch.nn.functional as F
    from scl_amd.aasist_head import node_counts
    cnt = node_counts(frames)
    B = len(frames)
    if record is not None:
        record["margins"] = []

    def bn(name, xs, cdim, apply=True):
        C = xs[0].shape[cdim]
        flat = torch.cat([x.movedim(cdim, -1).reshape(-1, C) for x in xs])
        n = flat.shape[0]
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        with torch.no_grad():
            t[name + ".running_mean"].mul_(0.9).add_(0.1 * mean)
            t[name + ".running_var"].mul_(0.9).add_(0.1 * (var * n / (n - 1) if n > 1 else var))
            t[name + ".num_batches_tracked"] += 1
        if record is not None:
            record[name] = (mean.detach(), var.detach(), n, flat.detach())
        if not apply:
            return None
        shape = [1] * xs[0].dim()
        shape[cdim] = C
        v = lambda p: p.view(shape)          # noqa: E731
        return [(x - v(mean)) * v((var + 1e-5) ** -0.5) * v(t[name + ".weight"]) + v(t[name + ".bias"]) for x in xs]

    lin = lambda name, x: F.linear(x, t[name + ".weight"], t[name + ".bias"])          # noqa: E731
    conv = lambda x, p, pad: F.conv2d(x, t[p + ".weight"], t[p + ".bias"], padding=pad)          # noqa: E731
    selu = lambda xs: [F.selu(x) for x in xs]          # noqa: E731

    xs = [F.max_pool2d(feats[b:b + 1, :3 * w].transpose(1, 2).unsqueeze(1), (3, 3)) for b, w in enumerate(cnt["W"])]
    xs = selu(bn("first_bn", xs, 1))
    for i in range(6):
        p = "encoder.%d.0." % i
        if i > 0:
            bn(p + "bn1", [x.detach() for x in xs], 1, apply=False)          # the reference discards its output: running statistics only
        a = selu(bn(p + "bn2", [conv(x, p + "conv1", (1, 1)) for x in xs], 1))
        idn = [conv(x, p + "conv_downsample", (0, 1)) for x in xs] if (p + "conv_downsample.weight") in t else xs
        xs = [conv(ab, p + "conv2", (0, 1)) + ib for ab, ib in zip(a, idn)]
    xs = selu(bn("first_bn1", xs, 1))
    ws = bn("attention.2", selu([conv(x, "attention.0", 0) for x in xs]), 1)
    ws = [conv(w, "attention.3", 0) for w in ws]
    e_S = [(x * F.softmax(w, dim=-1)).sum(-1).transpose(1, 2) + t["pos_S"] for x, w in zip(xs, ws)]
    e_T = [(x * F.softmax(w, dim=-2)).sum(-2).transpose(1, 2) for x, w in zip(xs, ws)]

    def gat(p, xs, temp):
        ys = []
        for x in xs:
            att = torch.tanh(lin(p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1))) @ t[p + "att_weight"]
            att = F.softmax(att / temp, dim=-2).squeeze(-1)
            ys.append(lin(p + "proj_with_att", att @ x) + lin(p + "proj_without_att", x))
        return selu(bn(p + "bn", ys, 2))

    def htrg(p, x1s, x2s, masters, temp):
        ys, ms = [], []
        for x1, x2, master in zip(x1s, x2s, masters):
            n1 = x1.shape[1]
            x = torch.cat([lin(p + "proj_type1", x1), lin(p + "proj_type2", x2)], dim=1)
            h = torch.tanh(lin(p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1)))
            first = torch.arange(x.shape[1]) < n1
            same = first[:, None] == first[None, :]
            a = torch.where(same[..., None], torch.where(first[:, None, None], t[p + "att_weight11"][:, 0], t[p + "att_weight22"][:, 0]),
                            t[p + "att_weight12"][:, 0])
            att = F.softmax((h * a).sum(-1) / temp, dim=-1)
            am = F.softmax(torch.tanh(lin(p + "att_projM", x * master)) @ t[p + "att_weightM"] / temp, dim=-2)
            ms.append(lin(p + "proj_with_attM", am.transpose(1, 2) @ x) + lin(p + "proj_without_attM", master))
            ys.append(lin(p + "proj_with_att", att @ x) + lin(p + "proj_without_att", x))
        ys = selu(bn(p + "bn", ys, 2))          # temporal and spectral nodes together, as the reference's BatchNorm1d sees them
        return [y[:, :x1.shape[1]] for y, x1 in zip(ys, x1s)], [y[:, x1.shape[1]:] for y, x1 in zip(ys, x1s)], ms

    def pool(p, hs, keeps):
        out = []
        for h, keep in zip(hs, keeps):
            s = torch.sigmoid(lin(p + "proj", h))
            if record is not None and h.shape[1] > keep:
                top = torch.topk(s.detach().squeeze(-1), keep + 1, dim=1).values
                record["margins"].append((top[:, keep - 1] - top[:, keep]).min().item())
            idx = torch.topk(s, keep, dim=1)[1].expand(-1, -1, h.shape[2])
            out.append(torch.gather(h * s, 1, idx))
        return out

    out_S = pool("pool_S.", gat("GAT_layer_S.", e_S, TEMPS[0]), [cnt["kS"]] * B)
    out_T = pool("pool_T.", gat("GAT_layer_T.", e_T, TEMPS[1]), cnt["kT"])
    res = []
    for l1, l2, pS, pT, m in (("HtrgGAT_layer_ST11.", "HtrgGAT_layer_ST12.", "pool_hS1.", "pool_hT1.", "master1"),
                              ("HtrgGAT_layer_ST21.", "HtrgGAT_layer_ST22.", "pool_hS2.", "pool_hT2.", "master2")):
        tt, ss, mm = htrg(l1, out_T, out_S, [t[m]] * B, TEMPS[2])
        ss, tt = pool(pS, ss, [cnt["kS2"]] * B), pool(pT, tt, cnt["kT2"])
        ta, sa, ma = htrg(l2, tt, ss, mm, TEMPS[2])
        res.append(([a_ + b_ for a_, b_ in zip(tt, ta)], [a_ + b_ for a_, b_ in zip(ss, sa)], [a_ + b_ for a_, b_ in zip(mm, ma)]))
    hid = []
    for b in range(B):
        T_, S_, M_ = (torch.max(res[0][i][b], res[1][i][b]) for i in range(3))
        hid.append(torch.cat([T_.abs().max(dim=1)[0], T_.mean(dim=1), S_.abs().max(dim=1)[0], S_.mean(dim=1), M_.squeeze(1)], dim=1))
    hid = torch.cat(hid)
    return lin("out_layer", hid), hid


def oracle_state(seed, dtype=torch.float64):
    """(oracle head filled from `seed` in `dtype`, {state-dict name: tensor} of a copy of it; float parameters require grad)."""
    from oracle.aasist import fill_state
    from oracle.aasist_head import AasistHead as OracleAasist
    from scl_amd.aasist_head import UPSTREAM_AASIST
    ref = OracleAasist(UPSTREAM_AASIST).to(dtype)
    filled = fill_state({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    params = {k for k, _ in ref.named_parameters()}
    t = {k: (v.detach().clone().requires_grad_(True) if k in params else v.detach().clone()) for k, v in ref.state_dict().items()}
    return ref, t


# the GPU head tests' cases: frames and the seed of the weights (tests/test_aasist_varlen_train_cpu.py asserts the top-k margins in float64)
HEAD_EQUAL = {"equal": (2, 121, 199, 1004), "alone": (1, 199, 199, 1004)}
HEAD_RAGGED = {"199": ([30, 199, 121, 202, 64], 1004), "780": ([780, 513, 45], 1004)}


def head_input(step, B, T):
    return torch.randn(B, T, 128, generator=torch.Generator().manual_seed(7919 * step + B + T))


def head_cotangents(step, B):
    g = torch.Generator().manual_seed(17 + step)
    return torch.randn(B, 2, generator=g, dtype=torch.float64), torch.randn(B, 160, generator=g, dtype=torch.float64) / 16
