"""The toy Qwen3 of the training-step tests (tests/test_gpu_qwen3_step.py) and its torch fp64 restatement: B 2, T 64, dim 128, 4 / 2 heads of 64, ffn 256, 2 layers, V 250
padded to 256, 4-bit layers -- the shape of tests/test_gpu_train_step.py::test_qwen3_toy_training_step_vs_autograd.  Not a test module: no test_ functions."""
import numpy as np
import torch

from koifish_amd import lib as L
from koifish_amd.train_step import Q3_MATS, Qwen3Step
from oracle import oracle as O
from tests.conftest import u16

CFG = dict(dim=128, n_layer=2, n_head=4, n_kv=2, head_dim=64, ffn=256, vocab=250, theta=10000.0, rms_eps=1e-6)
Bn, T, V, Vp = 2, 64, 250, 256
N = Bn * T
HP = dict(lr=2e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=99)
F64 = lambda a_u16: torch.tensor(O.bf16_to_f32(a_u16).astype(np.float64))


def make(ctx, seed=91, tied=True, **kw):
    """(Qwen3Step on host-made masters, ids, tgt): the fp64 side sees the same numbers"""
    rng = np.random.default_rng(seed)
    bf = lambda a: torch.from_numpy(O.f32_to_bf16(a.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    mk = lambda *s, std=0.08: bf(rng.normal(0, std, size=s))
    nw = lambda n: bf(1 + rng.normal(0, 0.1, n))
    dim, H, KV, hd, ffn = (CFG[k] for k in ("dim", "n_head", "n_kv", "head_dim", "ffn"))
    shapes = dict(q=(H * hd, dim), k=(KV * hd, dim), v=(KV * hd, dim), o=(dim, H * hd), gate=(ffn, dim), up=(ffn, dim), down=(dim, ffn))
    masters = dict(wte=mk(V, dim, std=0.2), nf=nw(dim),
                   layers=[dict({k: mk(*shapes[k]) for k in Q3_MATS}, n1=nw(dim), n2=nw(dim), qn=nw(hd), kn=nw(hd)) for _ in range(CFG["n_layer"])])
    if not tied:
        masters["head"] = mk(V, dim, std=0.2)
    ids, tgt = rng.integers(0, V, N).astype(np.int32), rng.integers(0, V, N).astype(np.int32)
    return Qwen3Step(ctx, CFG, Bn, T, tied=tied, masters=masters, **kw), ids, tgt


def key_of(name):
    """'l0.q.w' -> '0.q', 'l1.n2' -> '1.n2', 'wte' -> 'wte'"""
    if name[0] == "l" and name[1].isdigit():
        name = name[1:]
        return name[:-2] if name.endswith(".w") else name
    return name


def torch_params(ctx, st):
    """the fp64 model's parameters as the step's forward reads them (dequantised blobs, bf16 tensors), and the leaves whose .grad the device's gradients are compared
    with; for a gama entry the leaves are (zero, step) and the weight is W_deq.detach() + (step Q - zero) - (step Q - zero).detach() (tests/test_gpu_gama_step.py)"""
    P, leaves = {}, {}
    for e in st.params:
        k = key_of(e["name"])
        if e.get("gama"):
            b = e["blob"]
            Q = torch.tensor((O.unpack(b.blob[:b.szData].cpu().numpy(), L.BITS[b.type]).astype(np.float64) - b.qBias).reshape(b.nGroup, 128))
            zs = F64(u16(e["p"]))
            zero, step = zs[:b.nGroup].clone().requires_grad_(True), zs[b.nGroup:].clone().requires_grad_(True)
            lin = (step[:, None] * Q - zero[:, None]).reshape(b.ne0, b.ne1)
            P[k] = F64(u16(ctx.dequant(b))).reshape(b.ne0, b.ne1) + lin - lin.detach()
            leaves[e["name"]] = (zero, step)
        elif e["type"] is not None and e["type"] != L.BF16:
            P[k] = F64(u16(ctx.dequant(e["blob"]))).reshape(tuple(e["p"].shape)).requires_grad_(True)   # kf_dequant is bit-exact against the oracle (tests/test_gpu_ops.py)
            leaves[e["name"]] = P[k]
        else:
            P[k] = F64(u16(e["p"])).reshape(tuple(e["p"].shape)).requires_grad_(True)
            leaves[e["name"]] = P[k]
    return P, leaves


def ref_logits(P, ids, n_seq, n_tok):
    """the toy in torch fp64 on given parameters -> logits [n_seq * n_tok, V]; every sequence at positions 0 .. n_tok - 1"""
    F = torch.nn.functional
    dim, H, KV, hd, NL, theta, eps = (CFG[k] for k in ("dim", "n_head", "n_kv", "head_dim", "n_layer", "theta", "rms_eps"))
    rmsn = lambda t_, w_: t_ * torch.rsqrt((t_ * t_).mean(-1, keepdim=True) + eps) * w_
    ang = torch.arange(n_tok, dtype=torch.float64)[:, None] * (1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd)))[None, :]
    cs, sn = torch.cos(ang)[None, :, None, :], torch.sin(ang)[None, :, None, :]

    def rope(t_):   # [n_seq, n_tok, heads, hd], rotate-half
        a, b = t_[..., :hd // 2], t_[..., hd // 2:]
        return torch.cat([a * cs - b * sn, a * sn + b * cs], dim=-1)
    xt = P["wte"][torch.from_numpy(np.asarray(ids)).long()]
    for li in range(NL):
        g_ = lambda nm: P["%d.%s" % (li, nm)]
        h1 = rmsn(xt, g_("n1"))
        q = rope(rmsn((h1 @ g_("q").T).reshape(n_seq, n_tok, H, hd), g_("qn"))).transpose(1, 2)
        k = rope(rmsn((h1 @ g_("k").T).reshape(n_seq, n_tok, KV, hd), g_("kn"))).transpose(1, 2)
        v = (h1 @ g_("v").T).reshape(n_seq, n_tok, KV, hd).transpose(1, 2)
        k, v = k.repeat_interleave(H // KV, dim=1), v.repeat_interleave(H // KV, dim=1)
        at = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(n_seq * n_tok, H * hd)
        x2 = xt + at @ g_("o").T
        h2 = rmsn(x2, g_("n2"))
        xt = x2 + (F.silu(h2 @ g_("gate").T) * (h2 @ g_("up").T)) @ g_("down").T
    return (rmsn(xt, P["nf"]) @ P["head" if "head" in P else "wte"].T)[:, :V]


def ref_loss(P, ids, tgt):
    return torch.nn.functional.cross_entropy(ref_logits(P, ids, Bn, T), torch.from_numpy(tgt).long())


def grad_deviation(got_bf16, ref):
    """(max, rms) deviation of a device gradient from the fp64 one, as fractions of the reference's largest magnitude"""
    got = O.bf16_to_f32(u16(got_bf16)).astype(np.float64).reshape(ref.shape)
    sc_ = np.abs(ref).max()
    return float(np.abs(got - ref).max() / sc_), float(np.sqrt(((got - ref) ** 2).mean()) / sc_)
