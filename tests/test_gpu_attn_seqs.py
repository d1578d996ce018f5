"""kf_attn_block_seqs on the GPU, all equalities (include/kf_abi.h): n_seq independent sequences in one launch against (a) kf_attn_block called per sequence on that
sequence's rows and (b) the oracle's fp64 canonical attention on the same rows -- the output rows, the K and V rows written, every other cache row and the row padding
unchanged, a parked sequence's rows and output untouched, the arrival counters back at zero -- at the slice rule's edges (one slice up to 192 keys, four at 193, five
at 301, 32 at 2048), in both settings of kf_set_canonical (ONE arithmetic), twice on a scratch zeroed once per head geometry.  The regions adjoin, so a read or write past
a position would show.  A parked sequence is parked in the DEVICE table only: the host's mirror still lists it.  Then every refusal: its status, nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import a8_restate as R
import exact_inputs as E
from conftest import bf16_t, u16
from oracle import oracle as O

pytestmark = pytest.mark.gpu
THETA, EPS = 1e6, 1e-6
POSITIONS = [0, 1, 63, 64, 191, 192, 193, 300, 2047]   # the slice-rule edges of tests/test_gpu_kv8.py
T_MAX, PAD, S_MAX = 2048, 8, 32                        # PAD: elements behind every cache row
FILL = 0x3FC0                                          # 1.5 in the padding, in the rows to be written and in the output before the launch
INVALID_ARGS, UNALIGN = -20, -2000
_BASE, _REF, _WS = {}, {}, {}
to_bf = lambda a: R.to_bf(np.asarray(a, dtype=np.float32))


def base(nh, nkv, hd):
    """drawn once per shape: T_MAX K / V rows every sequence's region starts from, S_MAX raw q / k / v rows (one per sequence), the norm weights"""
    key = (nh, nkv, hd)
    if key not in _BASE:
        rng = np.random.default_rng(nh * 1000 + nkv * 10 + hd)
        kvd = nkv * hd
        draw = lambda *s: to_bf(rng.standard_normal(s))
        k = to_bf(rng.standard_normal((T_MAX, kvd)) * rng.uniform(0.25, 4.0, (T_MAX, 1)))
        wq, wk = to_bf(rng.uniform(0.5, 1.5, hd)), to_bf(rng.uniform(0.5, 1.5, hd))
        _BASE[key] = (k, draw(T_MAX, kvd), to_bf(3 * rng.standard_normal((S_MAX, nh * hd))), draw(S_MAX, kvd), draw(S_MAX, kvd), wq, wk)
    return _BASE[key]


def oracle_ref(nh, nkv, hd, s, pos):
    """the oracle's (output row, prepared K row) of sequence s at pos: computed once, shared by every mix and order"""
    key = (nh, nkv, hd, s, pos)
    if key not in _REF:
        k, v, q, kr, vr, wq, wk = base(nh, nkv, hd)
        qp = O.rope(O.headnorm(q[s], wq, nh, hd, EPS), nh, hd, pos, THETA)
        kp = O.rope(O.headnorm(kr[s], wk, nkv, hd, EPS), nkv, hd, pos, THETA)
        kc, vc = k[:pos + 1].copy(), v[:pos + 1].copy()
        kc[pos], vc[pos] = kp, vr[s]
        _REF[key] = (O.attn_decode(qp, kc, vc, pos, nh, nkv, hd, mode=O.ATTN_CANON), kp)
    return _REF[key]


def shared(ctx, nh, hd):
    """ONE scratch per (n_head, hd) -- the sequences' counters lie a decode scratch of that shape apart -- zeroed when it is made and never again, and the rope tables"""
    _WS.setdefault("tab", {}) or _WS["tab"].update({d: ctx.rope_table(T_MAX, d, THETA) for d in E.HEAD_DIMS})
    if (nh, hd) not in _WS:
        _WS[nh, hd] = torch.zeros(ctx.hip.kf_attn_seqs_scratch_bytes(nh, hd, S_MAX), dtype=torch.uint8, device=ctx.device)
    return _WS[nh, hd], _WS["tab"]


def mixes(n_seq):
    equal = [193] * n_seq
    differ = [POSITIONS[(2 * s + s // 9 + n_seq) % 9] for s in range(n_seq)]   # all different up to 9 sequences, every edge met at 32
    parked = list(differ)
    parked[n_seq // 2] = -1                                                    # parked on the device, listed at 2047 by the host: its workgroups leave at once
    return [equal, differ, parked]


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
@pytest.mark.parametrize("n_seq", [1, 3, 8, 32])
def test_seqs_equal_block_and_oracle(ctx, n_seq, nh, nkv, hd):
    k, v, q, kr, vr, wq, wk = base(nh, nkv, hd)
    kvd = nkv * hd
    ws, tabs = shared(ctx, nh, hd)
    qd, krd, vrd, wqd, wkd = (bf16_t(a, ctx.device) for a in (q[:n_seq], kr[:n_seq], vr[:n_seq], wq, wk))
    for pos in mixes(n_seq):
        live = [s for s in range(n_seq) if pos[s] >= 0]
        row0 = np.concatenate([[1], 1 + np.cumsum([max(p, 0) + 1 for p in pos])]).astype(int)   # row 0 and the last row belong to nobody
        rows = int(row0[-1]) + 1
        hk, hv = np.full((rows, kvd + PAD), FILL, dtype=np.uint16), np.full((rows, kvd + PAD), FILL, dtype=np.uint16)
        for s in range(n_seq):                       # a parked sequence owns one row, which nobody may touch
            n = max(pos[s], 0)
            hk[row0[s]:row0[s] + n, :kvd], hv[row0[s]:row0[s] + n, :kvd] = k[:n], v[:n]
        # (a) kf_attn_block per sequence on its own rows, the V row in place, in the canonical order
        kc_ref, vc_ref = bf16_t(hk, ctx.device), bf16_t(hv, ctx.device)
        want = torch.from_numpy(np.full((n_seq, nh * hd), FILL, dtype=np.uint16).view(np.int16)).to(ctx.device).view(torch.bfloat16)
        ctx.set_canonical(True)
        for s in live:
            vc_ref[row0[s] + pos[s], :kvd] = vrd[s]
            want[s] = ctx.attn_block(qd[s], krd[s], kc_ref[row0[s]:], vc_ref[row0[s]:], wqd, wkd, tabs[hd], pos[s], nh, nkv, hd, EPS, kv_stride=kvd + PAD)
        # (b) the oracle on the same rows
        for s in live:
            o_out, o_k = oracle_ref(nh, nkv, hd, s, pos[s])
            assert np.array_equal(u16(want[s]), o_out) and np.array_equal(u16(kc_ref[row0[s] + pos[s], :kvd]), o_k), "kf_attn_block left the oracle: sequence %d" % s
        per = ctx.hip.kf_attn_scratch_bytes(nh, hd)
        for canon in (True, False):
            ctx.set_canonical(canon)
            kc, vc = bf16_t(hk, ctx.device), bf16_t(hv, ctx.device)
            out = want.clone().fill_(1.5)
            for run in range(2):
                mirror = [2047 if p < 0 else p for p in pos]    # the host's mirror only bounds the device table: a sequence the device parked is still listed
                ctx.attn_block_seqs(qd, krd, vrd, kc, vc, wqd, wkd, tabs[hd], mirror, row0[:n_seq], nh, nkv, hd, EPS, kv_stride=kvd + PAD, out=out, scratch=ws,
                                    d_pos=torch.tensor(pos, dtype=torch.int32, device=ctx.device))
                what = "n_seq %d pos %s canon %d run %d" % (n_seq, pos, canon, run)
                assert torch.equal(out.view(torch.int16), want.view(torch.int16)), "output rows: " + what
                assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16)), "K cache: " + what
                assert torch.equal(vc.view(torch.int16), vc_ref.view(torch.int16)), "V cache: " + what
                assert not ws[:n_seq * per].view(n_seq, per)[:, :16384].any(), "arrival counters: " + what
    ctx.set_canonical(True)


def test_refusals_launch_nothing(ctx):
    nh, nkv, hd, S = 4, 2, 128, 3
    kvd, dev = nkv * hd, ctx.device
    ws, tabs = shared(ctx, nh, hd)
    mk = lambda *s: torch.full(s, 1.5, dtype=torch.bfloat16, device=dev)
    q, kr, vr, kc, vc, out, wn = mk(S, nh * hd + 8), mk(S, kvd + 8), mk(S, kvd + 8), mk(64, kvd + 8), mk(64, kvd + 8), mk(S, nh * hd + 8), mk(hd)
    tables = torch.tensor([3, 5, 7, 0, 10, 20], dtype=torch.int32, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    # the arguments of kf_attn_block_seqs in order (ctx and eps apart), then what each refused call changes
    good = dict(q=p(q), qs=q.stride(0), k=p(kr), ks=kr.stride(0), v=p(vr), vs=vr.stride(0), kc=p(kc), vc=p(vc), out=p(out), os=out.stride(0), wq=p(wn), wk=p(wn),
                tab=p(tabs[hd]), dp=p(tables), dr=p(tables, 12), hp=(C.c_int32 * 3)(3, 5, 7), S=S, nh=nh, nkv=nkv, hd=hd, kvs=kvd + 8)
    cases = [({n: None}, INVALID_ARGS) for n in ("q", "k", "v", "kc", "vc", "out", "tab", "dp", "dr", "hp", "ws")]
    cases += [(c, INVALID_ARGS) for c in (dict(S=0), dict(S=33), dict(hd=96), dict(nh=6, nkv=4), dict(nh=32, nkv=2), dict(qs=nh * hd - 8), dict(ks=kvd - 8), dict(vs=kvd - 8),
                                          dict(os=nh * hd - 8), dict(kvs=kvd - 8))]
    cases += [(c, UNALIGN) for c in (dict(kvs=kvd + 4), dict(qs=nh * hd + 4), dict(vs=kvd + 4), dict(os=nh * hd + 4), dict(kc=p(kc, 2)), dict(vc=p(vc, 2)), dict(v=p(vr, 2)),
                                     dict(ws=p(ws, 8)))]
    for change, status in cases:
        a = dict(good, ws=p(ws))
        a.update(change)
        assert ctx.hip.kf_attn_block_seqs(ctx.h, *[a[n] for n in good], EPS, a["ws"]) == status, change
    assert ctx.hip.kf_attn_block_seqs(ctx.h, *[dict(good, hp=(C.c_int32 * 3)(-1, -1, -1))[n] for n in good], EPS, p(ws)) == 0   # every sequence parked: KF_OK, no launch
    ctx.sync()
    assert all(bool((t == 1.5).all()) for t in (kc, vc, out)), "a refused call wrote"
