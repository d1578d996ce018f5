"""Python plumbing over the C ABI: device memory comes from torch tensors, every computation is a kf_* / kfh_* call.

Nothing here computes on the CPU and nothing imports oracle/.  bf16 tensors are torch.bfloat16 on the GPU;
packed weights are torch.uint8 blobs laid out `data || gama` exactly as the reference allocates them
(GTensor.cpp:456-510).
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L

SLOTS = ("q", "k", "v", "o", "gate", "up", "down")
NORMS = ("norm_in", "norm_post", "qn", "kn")


def quant_range(type_, symmetric=False):
    """qMin, qMax, qBias as the GeQuant ctor sets them (GeQuant.cpp:107-124)."""
    if type_ == L.T_SIGN:
        return -1, 1, 1
    if type_ in (L.BOOL1, L.T_BINARY):
        return 0, 1, 0
    if type_ == L.Q4:
        return (-8, 7, 8) if symmetric else (0, 15, 0)
    return 0, 0, 0


def perplexity_from_logprobs(logprobs):
    """The reference's perplexity figures (Fish::Eval_ppl, Evaluate.cpp:64-80) from per-token log-probabilities, in fp64, no device needed:
    sum = sum(lp), ss = sum(lp^2), nz = their number; ppl = exp(-sum / nz), pplerr = ppl * sqrt((ss - sum * sum / nz) / nz / nz).  Returns (ppl, pplerr, nz)."""
    lp = np.asarray(logprobs, dtype=np.float64).reshape(-1)
    nz = int(lp.size)
    if nz < 1:
        raise ValueError("perplexity_from_logprobs: no log-probabilities")
    s, ss = float(lp.sum()), float((lp * lp).sum())
    ppl = float(np.exp(-s / nz))
    return ppl, ppl * float(np.sqrt(max(ss - s * s / nz, 0.0) / nz / nz)), nz


class DevWeight:
    """A weight resident in HBM: blob = torch.uint8 [szData + szGama]."""

    def __init__(self, type_, ne0, ne1, blob, lGroup=128, symmetric=False):
        self.type, self.ne0, self.ne1, self.blob, self.lGroup = type_, ne0, ne1, blob, lGroup
        bits = L.BITS[type_]
        self.szData = ne0 * ne1 * bits // 8
        self.quantised = bits < 8
        self.nGroup = ne0 * ne1 // lGroup if self.quantised else 0
        self.szGama = (ne0 + ne1 + 2 * self.nGroup) * 2 if self.quantised else 0
        assert blob.numel() == self.szData + self.szGama, (blob.numel(), self.szData, self.szGama)
        self.qMin, self.qMax, self.qBias = quant_range(type_, symmetric)

    @staticmethod
    def blob_bytes(type_, ne0, ne1, lGroup=128):
        bits = L.BITS[type_]
        n = ne0 * ne1 * bits // 8
        if bits < 8:
            n += (ne0 + ne1 + 2 * (ne0 * ne1 // lGroup)) * 2
        return n

    def desc(self):
        p = self.blob.data_ptr()
        return L.Weight(p, (p + self.szData) if self.quantised else None, self.type, self.ne0, self.ne1, self.nGroup, self.lGroup, self.qMin, self.qMax,
                        self.qBias, None, None)

    def algorithmic_bytes(self):
        """what a mat-vec has to read: packed data + zero/step"""
        return self.szData + 4 * self.nGroup

    def zero_step(self):
        g = self.blob[self.szData:].view(torch.bfloat16)
        z0 = self.ne0 + self.ne1
        return g[z0:z0 + self.nGroup], g[z0 + self.nGroup:z0 + 2 * self.nGroup]


    def gama_slice(self):
        """the blob's [ZERO nGroup][STEP nGroup] region as a bf16 view, 2 nGroup long (element offset ne0 + ne1 of gama): the parameter of "train_target": "gama"
        (GTensor::InitGamaParam) -- what kf_adamw is pointed at, in place inside the blob"""
        if not self.quantised:
            raise L.KFError("gama_slice: type %d has no (zero, step) groups" % self.type)
        g = self.blob[self.szData:].view(torch.bfloat16)
        z0 = self.ne0 + self.ne1
        return g[z0:z0 + 2 * self.nGroup]


class LutDevWeight:
    """Row-codebook weight in HBM (KF_QUANT_ROW_LUT; GeQuant::RT_NormalF): blob = MSB-first `bits`-wide stream [ne0*ne1*bits/8] ‖ bf16 gama
    [ne0 + ne1 + (2^bits)*ne0]; bits 4 (the mat-vec format), 3 or 2 (dequantised in front of a product, or multiplied from the stream with Context.set_row_unpack); rtn=True (bits 2): (zero, step) per row, KF_QUANT_ROW_RTN."""

    def __init__(self, ne0, ne1, blob, bits=4, rtn=False):
        self.type, self.ne0, self.ne1, self.blob, self.lGroup = {4: L.Q4, 3: L.Q3, 2: L.Q2}[bits], ne0, ne1, blob, 0
        self.bits, self.rtn = bits, rtn
        self.szData = ne0 * ne1 * bits // 8
        self.szGama = (ne0 + ne1 + (2 if rtn else 1 << bits) * ne0) * 2
        assert blob.numel() == self.szData + self.szGama, (blob.numel(), self.szData, self.szGama)

    @staticmethod
    def blob_bytes(ne0, ne1, bits=4):
        return ne0 * ne1 * bits // 8 + (ne0 + ne1 + (1 << bits) * ne0) * 2

    def desc(self):
        p = self.blob.data_ptr()
        return L.Weight(p, p + self.szData, self.type, self.ne0, self.ne1, 0, 0, 0, (1 << self.bits) - 1, 0, None, None,
                        L.QUANT_ROW_RTN if self.rtn else L.QUANT_ROW_LUT, 0)

    def algorithmic_bytes(self):
        """what a mat-vec has to read: the nibble stream + the rows' tables"""
        return self.szData + 32 * self.ne0

    def lut(self):
        g = self.blob[self.szData:].view(torch.bfloat16)
        return g[self.ne0 + self.ne1:].view(self.ne0, -1)


class AWQDevWeight:
    """Vendor AutoAWQ tensors in HBM: qweight int32 [in, out/8], qzeros int32 [in/128, out/8], scales fp16 [in/128, out]."""

    def __init__(self, n_out, n_in, qweight, qzeros, scales):
        self.type, self.ne0, self.ne1, self.lGroup = L.Q4, n_out, n_in, 128
        self.qweight, self.qzeros, self.scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()

    def desc(self):
        return L.Weight(self.qweight.data_ptr(), None, L.Q4, self.ne0, self.ne1, self.ne0 * self.ne1 // 128, 128, 0, 15, 0, self.qzeros.data_ptr(),
                        self.scales.data_ptr())

    def algorithmic_bytes(self):
        return self.qweight.numel() * 4 + self.qzeros.numel() * 4 + self.scales.numel() * 2


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_STREAM = {}


def stream(device=0):
    """One dedicated (non-default) HIP stream per device, made torch's current stream, so that torch's allocations /
    copies and the kf_* launches are ordered on the same queue and the queue can be captured into a hipGraph
    (the legacy default stream cannot)."""
    if device not in _STREAM:
        torch.cuda.set_device(device)
        _STREAM[device] = torch.cuda.Stream(device=device)
        torch.cuda.set_stream(_STREAM[device])
    return _STREAM[device]


# Test hook (Python side only; the library reads no environment): the summation order every Context / Qwen3 created from here on is switched to right after its
# creation.  None = the library's own default (canonical, kf_abi.h).  tests/conftest.py sets False: the tolerance tests were written against the v_dot2c order and keep
# covering it, the canonical order is asserted bit for bit by the tests that switch it on themselves.
DEFAULT_CANONICAL = None


class Context:
    """kf_ctx bound to torch's current stream on `device`."""

    def __init__(self, device=0):
        self.hip, self.host = L.load()
        if not torch.cuda.is_available():
            raise L.KFError("no GPU visible: koifish_amd runs on MI355X only (no CPU fallback)")
        torch.cuda.set_device(device)
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        L.check(self.hip.kf_init(device, C.c_void_p(stream(device).cuda_stream), C.byref(self.h)), "kf_init")
        self._attn_ws = None
        self._head_ws = torch.empty(self.hip.kf_head_scratch_bytes(), dtype=torch.uint8, device=self.device)
        self._lin_ws = None
        if DEFAULT_CANONICAL is not None:
            self.set_canonical(DEFAULT_CANONICAL)

    def close(self):
        if self.h:
            self.hip.kf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        L.check(self.hip.kf_sync(self.h), "kf_sync")

    def set_canonical(self, on):
        """1 (the library default): the decode kernels sum in the canonical order the CPU oracle shares (bit-exact); 0: the v_dot2c / fp32 forms"""
        L.check(self.hip.kf_set_canonical(self.h, int(bool(on))), "kf_set_canonical")

    def set_row_unpack(self, on):
        """1: the 3- / 2-bit row forms are multiplied from the packed stream (kf_set_row_unpack: one token, the fused decode entries, token batches -- the bits of the
        4-bit row codebook holding the same values); 0 (the library default): dequantise + bf16 product, and the fused entries refuse them"""
        L.check(self.hip.kf_set_row_unpack(self.h, int(bool(on))), "kf_set_row_unpack")

    # ---- weights
    def upload_blob(self, type_, ne0, ne1, blob_np, lGroup=128, symmetric=False):
        t = torch.from_numpy(np.ascontiguousarray(blob_np).view(np.uint8).reshape(-1).copy()).to(self.device)
        return DevWeight(type_, ne0, ne1, t, lGroup, symmetric)

    def quantize(self, w_bf16, type_, lGroup=128, symmetric=False):
        """w_bf16: torch.bfloat16 [ne0, ne1] on the GPU -> DevWeight (kf_quantize: GeQuant::RTN_x / YinYang on device)."""
        if type_ == L.NF4:
            return self.quantize_nf4(w_bf16)
        if type_ == L.NF3:
            return self.quantize_nf4(w_bf16, bits=3)
        ne0, ne1 = w_bf16.shape
        w_bf16 = w_bf16.contiguous()
        if type_ == L.BF16:
            return DevWeight(L.BF16, ne0, ne1, w_bf16.view(torch.uint8).reshape(-1))
        if type_ == L.F8E5M2:
            # Float2T<f8e5> (g_float.hpp:433-443): float -> half (RNE) -> keep the high byte
            h = w_bf16.to(torch.float32).to(torch.float16).view(torch.int16)
            b = ((h.to(torch.int32) >> 8) & 0xFF).to(torch.uint8)
            return DevWeight(L.F8E5M2, ne0, ne1, b.reshape(-1).contiguous())
        blob = torch.zeros(DevWeight.blob_bytes(type_, ne0, ne1, lGroup), dtype=torch.uint8, device=self.device)
        dw = DevWeight(type_, ne0, ne1, blob, lGroup, symmetric)
        g = blob[dw.szData:].view(torch.bfloat16)
        g[:ne0 + ne1] = 1.0  # R_SCALE / C_SCALE (unused: rc_normal = 0)
        d = dw.desc()
        L.check(self.hip.kf_quantize(self.h, C.byref(d), _ptr(w_bf16), int(symmetric)), "kf_quantize")
        return dw

    def upload_lut_blob(self, ne0, ne1, blob_np, bits=4, rtn=False):
        t = torch.from_numpy(np.ascontiguousarray(blob_np).view(np.uint8).reshape(-1).copy()).to(self.device)
        return LutDevWeight(ne0, ne1, t, bits, rtn)

    def quantize_nf4(self, w_bf16, bits=4):
        """w_bf16: torch.bfloat16 [ne0, ne1] on the GPU -> LutDevWeight (kf_quantize in KF_QUANT_ROW_LUT mode: GeQuant::RT_NormalF on device; bits 4 or 3)."""
        ne0, ne1 = w_bf16.shape
        w_bf16 = w_bf16.contiguous()
        blob = torch.zeros(LutDevWeight.blob_bytes(ne0, ne1, bits), dtype=torch.uint8, device=self.device)
        dw = LutDevWeight(ne0, ne1, blob, bits)
        blob[dw.szData:].view(torch.bfloat16)[:ne0 + ne1] = 1.0  # R_SCALE / C_SCALE (unused: rc_normal = 0)
        d = dw.desc()
        L.check(self.hip.kf_quantize(self.h, C.byref(d), _ptr(w_bf16), 0), "kf_quantize")
        return dw

    # ---- operators (each one ABI call)
    def dequant(self, w):
        shape = (w.ne1, w.ne0) if isinstance(w, AWQDevWeight) else (w.ne0, w.ne1)   # AWQ: [in, out] (TransA = 0)
        out = torch.empty(*shape, dtype=torch.bfloat16, device=self.device)
        d = w.desc()
        L.check(self.hip.kf_dequant(self.h, C.byref(d), _ptr(out)), "kf_dequant")
        return out

    def linear_scratch(self, w, n_tok=1):
        """kernels never allocate: storages served by dequantise-then-multiply (AWQ, 3- / 2-bit row forms unless set_row_unpack serves them from the stream, row-codebook
        batches) get their workspace here"""
        d = w.desc() if not isinstance(w, L.Weight) else w
        need = self.hip.kf_linear_scratch_bytes(C.byref(d), int(n_tok))
        if need and (self._lin_ws is None or self._lin_ws.numel() < need):
            self.sync()   # earlier launches may still read the old buffer
            self._lin_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            L.check(self.hip.kf_set_scratch(self.h, C.c_void_p(self._lin_ws.data_ptr()), C.c_size_t(need)), "kf_set_scratch")
        return need

    def linear(self, w, x, bias=None, alpha=1.0, beta=0.0, residual=None, y=None):
        y = torch.zeros(w.ne0, dtype=torch.bfloat16, device=self.device) if y is None else y
        self.linear_scratch(w)
        d = w.desc()
        epi = L.KF_EPI_RESIDUAL if residual is not None else 0
        L.check(self.hip.kf_linear(self.h, C.byref(d), _ptr(x), _ptr(y), _ptr(bias), 1, alpha, beta, epi, _ptr(residual)), "kf_linear")
        return y

    def gama_backward(self, w, dIn, inp, g, scale=1.0):
        """kf_gama_backward: g [2 nGroup] bf16 (zero gradients, then step gradients) += scale x the (zero, step) gradients of the group-quantised w [OC, IC] from
        dIn [n, OC] and inp [n, IC].  Owns the scratch (kernels never allocate) and sizes it with kf_gama_backward_scratch_bytes: the entry itself is not told the size."""
        n = dIn.shape[0]
        need = self.hip.kf_gama_backward_scratch_bytes(w.ne0, w.ne1, n)
        if dIn.shape != (n, w.ne0) or inp.shape != (n, w.ne1) or g.numel() != 2 * w.nGroup:
            raise L.KFError("gama_backward: dIn %s, inp %s, g %d for a [%d, %d] weight of %d groups" % (tuple(dIn.shape), tuple(inp.shape), g.numel(), w.ne0, w.ne1, w.nGroup))
        ws = getattr(self, "_gama_ws", None)
        if ws is None or ws.numel() < need + 256:
            self.sync()   # earlier launches may still read the old buffer
            ws = self._gama_ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        d = w.desc()
        L.check(self.hip.kf_gama_backward(self.h, C.byref(d), _ptr(dIn), _ptr(inp), _ptr(g), n, scale, C.c_void_p((ws.data_ptr() + 255) & ~255)), "kf_gama_backward")
        return g

    def lora_forward(self, a, b, x, y, s=1.0):
        """kf_lora_forward beside a frozen matrix: a [r, IC], b [OC, r], x [n, IC] bf16; y [n, OC] bf16 already holds the base product and becomes
        bf16(y + s ax b^T) in place, with ax = bf16(s x a^T) [n, r], which is returned for the backward.  s multiplies BOTH products (the reference's sAB): the adapter's
        effective weight is s^2 b a."""
        (r, IC), (OC, n) = a.shape, (b.shape[0], x.shape[0])
        if b.shape != (OC, r) or x.shape != (n, IC) or y.shape != (n, OC):
            raise L.KFError("lora_forward: a %s, b %s, x %s, y %s" % (tuple(a.shape), tuple(b.shape), tuple(x.shape), tuple(y.shape)))
        ax = torch.empty(n, r, dtype=torch.bfloat16, device=self.device)
        L.check(self.hip.kf_lora_forward(self.h, _ptr(a), _ptr(b), r, OC, IC, _ptr(x), _ptr(y), _ptr(ax), n, s), "kf_lora_forward")
        return ax

    def lora_apply(self, a, b, x, y, s=1.0, keep_ax=False):
        """kf_lora_apply, the adapter at inference.  One adapter: a [r, IC], b [OC, r], x [n, IC] (or [IC]), y [n, OC] (or [OC]) bf16, any n >= 1; y becomes
        bf16(y + s ax b^T) in place; keep_ax (n >= 2 only): ax [n, r] is kept and returned.  Up to three adapters that share ONE input row (n == 1, the vector form, one
        launch): a, b and y are tuples of tensors, the y's separate and of their own lengths."""
        many = isinstance(a, (tuple, list))
        a_, b_, y_ = (list(a), list(b), list(y)) if many else ([a], [b], [y])
        n_w, (r, IC) = len(a_), a_[0].shape
        n = 1 if x.dim() == 1 else x.shape[0]
        OC = [t.shape[0] for t in b_]
        if len(b_) != n_w or len(y_) != n_w or x.numel() != n * IC or any(tuple(a_[i].shape) != (r, IC) or tuple(b_[i].shape) != (OC[i], r) or y_[i].numel() != n * OC[i]
                                                                            for i in range(n_w)):
            raise L.KFError("lora_apply: a %s, b %s, x %s, y %s" % ([tuple(t.shape) for t in a_], [tuple(t.shape) for t in b_], tuple(x.shape), [tuple(t.shape) for t in y_]))
        ax = torch.empty(n, r, dtype=torch.bfloat16, device=self.device) if keep_ax and n > 1 else None
        ptrs = lambda ts: (C.c_void_p * n_w)(*[t.data_ptr() for t in ts])
        L.check(self.hip.kf_lora_apply(self.h, n_w, ptrs(a_), ptrs(b_), r, (C.c_int * n_w)(*OC), IC, _ptr(x), ptrs(y_), _ptr(ax), n, s),
                "kf_lora_apply")
        return ax

    def lora_backward(self, a, b, dIn, inp, ax, delta, g, s=1.0):
        """kf_lora_backward: delta [n, IC] bf16 (what the base's kf_linear_backward left) += s adelta a with adelta = bf16(s dIn b); g = [gA (r IC) | gB (OC r)] bf16 +=
        s adelta^T inp | s dIn^T ax.  Owns the scratch (kernels never allocate), sized with kf_lora_backward_scratch_bytes; returns adelta [n, r], a view of its head."""
        (r, IC), (OC, n) = a.shape, (b.shape[0], dIn.shape[0])
        need = self.hip.kf_lora_backward_scratch_bytes(r, OC, IC, n)
        if b.shape != (OC, r) or dIn.shape != (n, OC) or inp.shape != (n, IC) or ax.shape != (n, r) or delta.shape != (n, IC) or g.numel() != r * (IC + OC) or not need:
            raise L.KFError("lora_backward: a %s, b %s, dIn %s, inp %s, ax %s, delta %s, g %d" % (tuple(a.shape), tuple(b.shape), tuple(dIn.shape), tuple(inp.shape),
                                                                                                 tuple(ax.shape), tuple(delta.shape), g.numel()))
        ws = getattr(self, "_lora_ws", None)
        if ws is None or ws.numel() < need + 256:
            self.sync()   # earlier launches may still read the old buffer
            ws = self._lora_ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        off = ((ws.data_ptr() + 255) & ~255) - ws.data_ptr()
        L.check(self.hip.kf_lora_backward(self.h, _ptr(a), _ptr(b), r, OC, IC, _ptr(dIn), _ptr(inp), _ptr(ax), _ptr(delta), _ptr(g), n, s, C.c_void_p(ws.data_ptr() + off)),
                "kf_lora_backward")
        return ws[off:off + n * r * 2].view(torch.bfloat16).view(n, r)

    def evolve(self, x, head, algorithm, alpha=0.9, social=2.0, t_crossover=0.6, seed=0):
        """kf_evolve (Fuyou::Exploitation): the follower matrix x [ne0, ne1] bf16 moves towards head [ne0, ne1] bf16, in place; algorithm "pso" | "pso_ga" | "mix"
        (Fuyou_params::Algo2Name) or a kf_evo_algorithm value; the defaults are Fuyou_params' (alpha 0.9, social 2, T_crossover 0.6).  Returns x."""
        if isinstance(algorithm, str):
            if algorithm not in L.EVO_ALGORITHMS:
                raise ValueError("evolve algorithm %r: one of %s" % (algorithm, sorted(L.EVO_ALGORITHMS)))
            algorithm = L.EVO_ALGORITHMS[algorithm]
        if x.dtype != torch.bfloat16 or head.dtype != torch.bfloat16 or x.dim() != 2 or x.shape != head.shape or not x.is_contiguous() or not head.is_contiguous():
            raise L.KFError("evolve: x %s %s and head %s %s must be contiguous bf16 matrices of one shape" % (tuple(x.shape), x.dtype, tuple(head.shape), head.dtype))
        L.check(self.hip.kf_evolve(self.h, _ptr(x), _ptr(head), x.shape[0], x.shape[1], int(algorithm), alpha, social, t_crossover, seed & 0xFFFFFFFF), "kf_evolve")
        return x

    def grad_norms_plan(self, grads, no_clip=None):
        """kf_grad_norms_plan over a list of bf16 device tensors (each 16-byte aligned, a positive multiple of 8 elements; they must stay alive and in place): returns
        the plan -- a dict that owns the scratch and the three device outputs `sumsq` fp64 [n + 1], `gnorm` fp32 [n + 1], `scale` fp32 [n] -- for grad_norms().
        no_clip: optional list of flags, one per tensor: its scale is 1.0 in every mode."""
        nt = len(grads)
        n = (C.c_longlong * max(nt, 1))(*[g.numel() for g in grads])
        ptrs = (C.c_void_p * max(nt, 1))(*[g.data_ptr() for g in grads])
        mask = None if no_clip is None else (C.c_uint8 * max(nt, 1))(*[int(bool(f)) for f in no_clip])
        need = self.hip.kf_grad_norms_scratch_bytes(nt, n)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        sp = (ws.data_ptr() + 255) & ~255
        L.check(self.hip.kf_grad_norms_plan(self.h, nt, ptrs, n, mask, C.c_void_p(sp), need), "kf_grad_norms_plan")
        # (the plan dict keeps ws alive; a caller that drops a plan it will not use again may call kf_grad_norms_forget(ctx, scratch) first)
        return dict(n=nt, ws=ws, scratch=sp, grads=list(grads), sumsq=torch.zeros(nt + 1, dtype=torch.float64, device=self.device),
                    gnorm=torch.zeros(nt + 1, dtype=torch.float32, device=self.device), scale=torch.zeros(nt, dtype=torch.float32, device=self.device))

    def grad_norms(self, plan, mode="report", gclip=1.0):
        """kf_grad_norms: every tensor's sum of squares in one launch, fixed summation order, nothing read back.  mode "report" | "tensor" | "global" (or a kf_clip_mode
        value).  Returns the plan's device tensors (sumsq, gnorm, scale); the last entry of sumsq / gnorm is the whole list's."""
        if isinstance(mode, str):
            if mode not in L.CLIP_MODES:
                raise ValueError("grad_norms mode %r: 'report', 'tensor' or 'global'" % (mode,))
            mode = L.CLIP_MODES[mode]
        L.check(self.hip.kf_grad_norms(self.h, C.c_void_p(plan["scratch"]), plan["n"], int(mode), gclip, _ptr(plan["sumsq"]), _ptr(plan["gnorm"]), _ptr(plan["scale"])),
                "kf_grad_norms")
        return plan["sumsq"], plan["gnorm"], plan["scale"]

    def loss_mean(self, members):
        """kf_loss_mean over a list of fp32 [n] device tensors: ((m0 + m1) + m2 ...) / len(members) in fp32, one launch per member"""
        out = torch.empty_like(members[0])
        for k, m in enumerate(members):
            L.check(self.hip.kf_loss_mean(self.h, _ptr(out), _ptr(m), out.numel(), k, len(members)), "kf_loss_mean")
        return out

    def act_quant_i8(self, x, norm_w=None, eps=1e-6):
        """kf_act_quant_i8: x bf16 [dim] or [rows, dim] (a row stride larger than dim is honoured) -> (q int8 of x's shape, step fp32 [rows]); with norm_w the rows are
        first RMS-normed and rounded to bf16 as kf_rmsnorm stores them"""
        rows, dim = (1, x.shape[0]) if x.dim() == 1 else x.shape
        ldx = dim if x.dim() == 1 else x.stride(0)
        assert x.stride(-1) == 1 and x.dtype == torch.bfloat16
        q = torch.empty((rows, dim) if x.dim() == 2 else (dim,), dtype=torch.int8, device=self.device)
        step = torch.empty(rows, dtype=torch.float32, device=self.device)
        L.check(self.hip.kf_act_quant_i8(self.h, _ptr(x), ldx, _ptr(norm_w), eps, rows, dim, _ptr(q), _ptr(step)), "kf_act_quant_i8")
        return q, step

    def kv8_quant_rows(self, k, v, k8, v8, ks, vs, pos0, n_kv, hd):
        """kf_kv8_quant_rows: k, v bf16 [n, n_kv * hd] (a row stride larger than that is honoured) -> rows pos0 .. pos0 + n - 1 of k8 / v8 int8 [n_ctx, kv_stride] and of
        ks / vs fp32 [n_ctx, n_kv], in place"""
        assert k.dim() == 2 and k.stride(1) == 1 and k.stride() == v.stride() and k.dtype == v.dtype == torch.bfloat16
        L.check(self.hip.kf_kv8_quant_rows(self.h, _ptr(k), _ptr(v), k.stride(0), k.shape[0], n_kv, hd, _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), pos0, k8.stride(0)),
                "kf_kv8_quant_rows")

    def kv8_dequant_rows(self, k8, v8, ks, vs, n, n_kv, hd, kout, vout):
        """kf_kv8_dequant_rows: rows 0 .. n - 1 of the int8 pair -> kout, vout bf16 [n, n_kv * hd] (their row stride is honoured), in place"""
        assert kout.stride() == vout.stride() and kout.stride(1) == 1
        L.check(self.hip.kf_kv8_dequant_rows(self.h, _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), n, n_kv, hd, k8.stride(0), _ptr(kout), _ptr(vout), kout.stride(0)),
                "kf_kv8_dequant_rows")

    def attn_prefill_kv8(self, q, k8, v8, ks, vs, pos0, n_head, n_kv, hd, out=None):
        """kf_attn_prefill_kv8: kf_attn_prefill's contract on the int8 cache -- q the prepared bf16 queries [n, n_head * hd] (a larger row stride is honoured, out's must
        equal it), rows pos0 .. pos0 + n - 1 of k8 / v8 / ks / vs already written (kv8_quant_rows) -> out [n, n_head * hd]"""
        if out is None:   # rows as far apart as q's: the entry has one row stride for both
            out = torch.empty((q.shape[0], q.stride(0)), dtype=q.dtype, device=q.device)[:, :q.shape[1]]
        assert out.stride(0) == q.stride(0) and q.stride(1) == 1 and out.stride(1) == 1
        L.check(self.hip.kf_attn_prefill_kv8(self.h, _ptr(q), _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(out), pos0, q.shape[0], q.stride(0), n_head, n_kv, hd,
                                             k8.stride(0)), "kf_attn_prefill_kv8")
        return out

    def attn_block_kv8(self, q_raw, k_raw, v_raw, k8, v8, ks, vs, wq, wk, table, pos, n_head, n_kv, hd, eps=1e-6, d_pos=None, ws=None):
        """kf_attn_block_kv8: kf_attn_block's contract on the int8 cache -- the new K / V rows are quantised and written (with their steps) at the position; pos is the
        launch bound when d_pos (an int32 device tensor holding the position) is given"""
        out = torch.empty(n_head * hd, dtype=torch.bfloat16, device=self.device)
        L.check(self.hip.kf_attn_block_kv8(self.h, _ptr(q_raw), _ptr(k_raw), _ptr(v_raw), _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(out), _ptr(wq), _ptr(wk), _ptr(table),
                                           pos, _ptr(d_pos), n_head, n_kv, hd, k8.stride(0), eps, _ptr(ws if ws is not None else self._ws(n_head, hd))), "kf_attn_block_kv8")
        return out

    def _linear_a8(self, entry, w, q, step, bias, residual, y):
        """the four int8-activation products share one calling convention: entry is the ABI function's name"""
        n = 1 if q.dim() == 1 else q.shape[0]
        if y is None:
            y = torch.zeros((n, w.ne0) if q.dim() == 2 else (w.ne0,), dtype=torch.bfloat16, device=self.device)
        d = w.desc()
        L.check(getattr(self.hip, entry)(self.h, C.byref(d), _ptr(q), _ptr(step), _ptr(y), _ptr(bias), _ptr(residual), n), entry)
        return y

    def linear_a8(self, w, q, step, bias=None, residual=None, y=None):
        """kf_linear_a8: a ternary / 1-bit weight times int8 activations q [ne1] or [nTok, ne1] with their steps [nTok] -> y bf16 [ne0] or [nTok, ne0]"""
        return self._linear_a8("kf_linear_a8", w, q, step, bias, residual, y)

    def linear_a8_tiles(self, w, q, step, bias=None, residual=None, y=None):
        """kf_linear_a8_tiles: linear_a8's contract and bits on int8 MFMA tiles, for token batches (any nTok >= 1 is served); residual may be y"""
        return self._linear_a8("kf_linear_a8_tiles", w, q, step, bias, residual, y)

    def linear_w4a8(self, w, q, step, bias=None, residual=None, y=None):
        """kf_linear_w4a8: a 4-bit group weight times int8 activations q [ne1] or [nTok, ne1] with their steps [nTok] -> y bf16 [ne0] or [nTok, ne0]"""
        return self._linear_a8("kf_linear_w4a8", w, q, step, bias, residual, y)

    def linear_w4a8_tiles(self, w, q, step, bias=None, residual=None, y=None):
        """kf_linear_w4a8_tiles: linear_w4a8's contract and bits on int8 MFMA tiles, for token batches (any nTok >= 1 is served); residual may be y"""
        return self._linear_a8("kf_linear_w4a8_tiles", w, q, step, bias, residual, y)

    def rmsnorm(self, x, w, eps=1e-6):
        y = torch.empty_like(x)
        rows = 1 if x.dim() == 1 else x.shape[0]
        L.check(self.hip.kf_rmsnorm(self.h, _ptr(x), _ptr(w), _ptr(y), rows, x.shape[-1], eps, None), "kf_rmsnorm")
        return y

    def rope_table(self, n_pos, hd, theta):
        t = np.zeros((n_pos, hd // 2, 2), dtype=np.float32)
        L.check(self.hip.kf_rope_table_host(t.ctypes.data_as(C.c_void_p), n_pos, hd, theta), "kf_rope_table_host")
        return torch.from_numpy(t).to(self.device)

    def qknorm_rope(self, q, k, wq, wk, table, pos, n_head, n_kv, hd, eps=1e-6):
        """in place on q and k"""
        L.check(self.hip.kf_qknorm_rope(self.h, _ptr(q), _ptr(k), _ptr(wq), _ptr(wk), _ptr(table), pos, None, n_head, n_kv, hd, eps), "kf_qknorm_rope")

    def _ws(self, n_head, hd):
        n = self.hip.kf_attn_scratch_bytes(n_head, hd)
        if self._attn_ws is None or self._attn_ws.numel() < n:
            self._attn_ws = torch.zeros(n, dtype=torch.uint8, device=self.device)  # arrival counters start at zero
        return self._attn_ws

    def attn_decode(self, q, kc, vc, pos, n_head, n_kv, hd, kv_stride=None):
        out = torch.empty(n_head * hd, dtype=torch.bfloat16, device=self.device)
        L.check(self.hip.kf_attn_decode(self.h, _ptr(q), _ptr(kc), _ptr(vc), _ptr(out), pos, None, n_head, n_kv, hd, kv_stride or n_kv * hd,
                                        _ptr(self._ws(n_head, hd))), "kf_attn_decode")
        return out

    def attn_block(self, q_raw, k_raw, kc, vc, wq, wk, table, pos, n_head, n_kv, hd, eps=1e-6, kv_stride=None):
        out = torch.empty(n_head * hd, dtype=torch.bfloat16, device=self.device)
        L.check(self.hip.kf_attn_block(self.h, _ptr(q_raw), _ptr(k_raw), _ptr(kc), _ptr(vc), _ptr(out), _ptr(wq), _ptr(wk), _ptr(table), pos, None, n_head,
                                       n_kv, hd, kv_stride or n_kv * hd, eps, _ptr(self._ws(n_head, hd))), "kf_attn_block")
        return out

    def swiglu(self, gate, up):
        out = torch.empty_like(gate)
        L.check(self.hip.kf_swiglu(self.h, _ptr(gate), _ptr(up), _ptr(out), gate.numel()), "kf_swiglu")
        return out

    def add(self, a, b):
        out = torch.empty_like(a)
        L.check(self.hip.kf_add(self.h, _ptr(a), _ptr(b), _ptr(out), a.numel()), "kf_add")
        return out

    def embed(self, w, token):
        out = torch.empty(w.ne1, dtype=torch.bfloat16, device=self.device)
        d = w.desc()
        L.check(self.hip.kf_embed(self.h, C.byref(d), int(token), None, _ptr(out)), "kf_embed")
        return out

    def lm_head(self, w, x):
        logits = torch.empty(w.ne0, dtype=torch.bfloat16, device=self.device)
        am = torch.zeros(1, dtype=torch.int32, device=self.device)
        d = w.desc()
        L.check(self.hip.kf_lm_head(self.h, C.byref(d), _ptr(x), _ptr(logits), _ptr(am), _ptr(self._head_ws)), "kf_lm_head")
        return logits, int(am.item())

    def norm_linear(self, x, norm_w, ws, eps=1e-6):
        ys = [torch.zeros(w.ne0, dtype=torch.bfloat16, device=self.device) for w in ws]
        descs = [w.desc() for w in ws]
        wp = (C.c_void_p * len(ws))(*[C.addressof(d) for d in descs])
        yp = (C.c_void_p * len(ws))(*[y.data_ptr() for y in ys])
        L.check(self.hip.kf_norm_linear(self.h, _ptr(x), _ptr(norm_w), eps, len(ws), wp, yp, None, 0, None), "kf_norm_linear")
        return ys

    def norm_gateup_swiglu(self, x, norm_w, gate, up, eps=1e-6):
        act = torch.zeros(gate.ne0, dtype=torch.bfloat16, device=self.device)
        dg, du = gate.desc(), up.desc()
        L.check(self.hip.kf_norm_gateup_swiglu(self.h, _ptr(x), _ptr(norm_w), eps, C.byref(dg), C.byref(du), _ptr(act)), "kf_norm_gateup_swiglu")
        return act

    # ---- the row siblings: x [R, ne1] (R = 1 .. 8 consecutive positions of one sequence) against one pass over the weights; thin mirrors for the op tests
    def linear_rows(self, w, x, residual=None, y=None):
        """kf_linear_rows: y [R, ne0] = x . W^T (+ residual); y may be the residual tensor itself (the in-place form)"""
        R = x.shape[0]
        y = torch.zeros(R, w.ne0, dtype=torch.bfloat16, device=self.device) if y is None else y
        d = w.desc()
        epi = L.KF_EPI_RESIDUAL if residual is not None else 0
        L.check(self.hip.kf_linear_rows(self.h, C.byref(d), _ptr(x), x.stride(0), _ptr(y), y.stride(0), R, epi, _ptr(residual),
                                        residual.stride(0) if residual is not None else 0), "kf_linear_rows")
        return y

    def norm_linear_rows(self, x, norm_w, ws, eps=1e-6, ys=None, y_row_stride=None, y_pos_stride=None, pos0=0):
        """kf_norm_linear_rows: row r of projection i at ys[i] + r * y_row_stride[i] + (pos0 + r) * y_pos_stride[i] (default: fresh [R, ne0] tensors)"""
        R = x.shape[0]
        if ys is None:
            ys = [torch.zeros(R, w.ne0, dtype=torch.bfloat16, device=self.device) for w in ws]
            y_row_stride, y_pos_stride = [y.stride(0) for y in ys], [0] * len(ws)
        descs = [w.desc() for w in ws]
        wp = (C.c_void_p * len(ws))(*[C.addressof(d) for d in descs])
        yp = (C.c_void_p * len(ws))(*[y.data_ptr() for y in ys])
        rs, ps = (C.c_int64 * len(ws))(*y_row_stride), (C.c_int64 * len(ws))(*y_pos_stride)
        L.check(self.hip.kf_norm_linear_rows(self.h, _ptr(x), x.stride(0), _ptr(norm_w), eps, len(ws), wp, yp, rs, ps, int(pos0), R), "kf_norm_linear_rows")
        return ys

    def norm_gateup_swiglu_rows(self, x, norm_w, gate, up, eps=1e-6):
        R = x.shape[0]
        act = torch.zeros(R, gate.ne0, dtype=torch.bfloat16, device=self.device)
        dg, du = gate.desc(), up.desc()
        L.check(self.hip.kf_norm_gateup_swiglu_rows(self.h, _ptr(x), x.stride(0), _ptr(norm_w), eps, C.byref(dg), C.byref(du), _ptr(act), act.stride(0), R),
                "kf_norm_gateup_swiglu_rows")
        return act

    def norm_lm_head_rows(self, w, x, norm_w=None, eps=1e-6, want_logits=True):
        """kf_norm_lm_head_rows -> (logits [R, ne0] or None, top1 [R] as a list of ints)"""
        R = x.shape[0]
        d = w.desc()
        ws = torch.empty(self.hip.kf_head_rows_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=self.device)
        logits = torch.zeros(R, w.ne0, dtype=torch.bfloat16, device=self.device) if want_logits else None
        top1 = torch.full((R,), -1, dtype=torch.int32, device=self.device)
        L.check(self.hip.kf_norm_lm_head_rows(self.h, _ptr(x), x.stride(0), _ptr(norm_w), eps, C.byref(d), _ptr(logits), w.ne0 if want_logits else 0, _ptr(top1), R,
                                              _ptr(ws)), "kf_norm_lm_head_rows")
        self.sync()   # ws is this call's own
        return logits, top1.tolist()

    def attn_decode_rows(self, q, kc, vc, pos0, n_head, n_kv, hd, kv_stride=None, scratch=None):
        """kf_attn_decode_rows: q [R, n_head * hd] prepared queries at positions pos0 .. pos0 + R - 1 -> out [R, n_head * hd]; scratch: a zero-filled uint8 tensor
        of kf_attn_rows_scratch_bytes the caller keeps between calls (default: a fresh one)"""
        q = q.contiguous()   # q and out rows lie one stride apart
        R = q.shape[0]
        out = torch.empty(R, n_head * hd, dtype=torch.bfloat16, device=self.device)
        if scratch is None:
            scratch = torch.zeros(self.hip.kf_attn_rows_scratch_bytes(n_head, hd, R), dtype=torch.uint8, device=self.device)
        L.check(self.hip.kf_attn_decode_rows(self.h, _ptr(q), q.stride(0), _ptr(kc), _ptr(vc), _ptr(out), int(pos0), R, n_head, n_kv, hd, kv_stride or n_kv * hd,
                                             _ptr(scratch)), "kf_attn_decode_rows")
        return out

    def rows_route_counts(self):
        """(activation rows served with the shared unpack, rows served by one-token launches) by the *_rows entries of this context"""
        out = (C.c_int64 * 2)()
        L.check(self.hip.kf_rows_route_counts(self.h, out), "kf_rows_route_counts")
        return int(out[0]), int(out[1])

    # ---- HIP events on the ctx stream
    def event(self):
        e = C.c_void_p()
        L.check(self.hip.kf_event_create(C.byref(e)), "kf_event_create")
        return e

    def record(self, e):
        L.check(self.hip.kf_event_record(self.h, e), "kf_event_record")

    def elapsed_ms(self, a, b):
        ms = C.c_float()
        L.check(self.hip.kf_event_elapsed_ms(a, b, C.byref(ms)), "kf_event_elapsed_ms")
        return ms.value


class Qwen3:
    """The host-side Fish (koifish_amd/host/kf_host.cpp) for a Qwen3-shaped decoder."""

    def __init__(self, cfg, device=0, own_stream=False):
        """own_stream: this decoder launches on a HIP stream of its own (several decoders then overlap on the GPU); otherwise on the
        device's shared stream."""
        self.hip, self.host = L.load()
        if not torch.cuda.is_available():
            raise L.KFError("no GPU visible: koifish_amd runs on MI355X only (no CPU fallback)")
        torch.cuda.set_device(device)
        self.cfg, self.device = dict(cfg), torch.device("cuda", device)
        rc = C.c_int(0)
        shared = stream(device)
        self._stream = torch.cuda.Stream(device=device) if own_stream else shared
        self.h = self.host.kfh_create(device, C.c_void_p(self._stream.cuda_stream), cfg["dim"], cfg["n_layer"], cfg["n_head"], cfg["n_kv"],
                                      cfg["head_dim"], cfg["ffn"], cfg["vocab"], cfg["max_seq"], cfg.get("rms_eps", 1e-6), cfg.get("qk_eps", 1e-6),
                                      cfg.get("theta", 1e6), C.byref(rc))
        if not self.h:
            why = self.host.kfh_host_error().decode()
            if why:
                raise L.KFError("kfh_create failed with %d: %s" % (rc.value, why))
            L.check(rc.value or -1, "kfh_create")
        self.h = C.c_void_p(self.h)
        if DEFAULT_CANONICAL is not None:
            L.check(self.host.kfh_set_canonical(self.h, int(bool(DEFAULT_CANONICAL))), "kfh_set_canonical")
        self._keep = []
        self.weights = {}
        self._norms = {}

    @classmethod
    def from_hf(cls, path, layer_type=L.Q4, head_type=L.BF16, device=0, lGroup=128, max_seq=0):
        """Hugging Face directory (config.json + model.safetensors[.index.json]; dense BF16/F16/F32 tensors are quantised on the GPU to
        `layer_type` / `head_type`, AutoAWQ qweight/qzeros/scales triples are taken as they are) -> a ready model.  The C++ loader is
        koifish_amd/host/kf_safetensors.cpp (K_SafeTensors, Serialize.cpp:849-976 read side)."""
        self = cls.__new__(cls)
        self.hip, self.host = L.load()
        if not torch.cuda.is_available():
            raise L.KFError("no GPU visible: koifish_amd runs on MI355X only (no CPU fallback)")
        torch.cuda.set_device(device)
        rc = C.c_int(0)
        self.device = torch.device("cuda", device)
        self.h = self.host.kfh_load_hf(str(path).encode(), device, C.c_void_p(stream(device).cuda_stream), int(layer_type), int(head_type), int(lGroup), int(max_seq),
                                       C.byref(rc))
        if not self.h:
            raise L.KFError("kfh_load_hf(%s) failed with %d: %s" % (path, rc.value, self.host.kfh_last_error().decode()))
        self.h = C.c_void_p(self.h)
        if DEFAULT_CANONICAL is not None:
            L.check(self.host.kfh_set_canonical(self.h, int(bool(DEFAULT_CANONICAL))), "kfh_set_canonical")
        self._read_config()
        return self

    @classmethod
    def from_kun(cls, path, device=0, max_seq=0):
        """A `.kun` checkpoint (the reference's container: safetensors header, `data||gama` blobs, msgpack config tensor; Serialize.cpp:849-976)
        -> a ready model.  The blobs go to HBM as stored: nothing is re-quantised."""
        self = cls.__new__(cls)
        self.hip, self.host = L.load()
        if not torch.cuda.is_available():
            raise L.KFError("no GPU visible: koifish_amd runs on MI355X only (no CPU fallback)")
        torch.cuda.set_device(device)
        rc = C.c_int(0)
        self.device = torch.device("cuda", device)
        self.h = self.host.kfh_load_kun(str(path).encode(), device, C.c_void_p(stream(device).cuda_stream), int(max_seq), C.byref(rc))
        if not self.h:
            raise L.KFError("kfh_load_kun(%s) failed with %d: %s" % (path, rc.value, self.host.kfh_last_error().decode()))
        self.h = C.c_void_p(self.h)
        if DEFAULT_CANONICAL is not None:
            L.check(self.host.kfh_set_canonical(self.h, int(bool(DEFAULT_CANONICAL))), "kfh_set_canonical")
        self._read_config()
        return self

    def _read_config(self):
        iv = (C.c_int * 10)()
        fv = (C.c_float * 2)()
        L.check(self.host.kfh_get_config(self.h, iv, fv), "kfh_get_config")
        self.cfg = dict(dim=iv[0], n_layer=iv[1], n_head=iv[2], n_kv=iv[3], head_dim=iv[4], ffn=iv[5], vocab=iv[6], max_seq=iv[7], tied=bool(iv[8]),
                        theta=float(fv[1]))
        self.fuse_level = iv[9]
        self._keep, self.weights, self._norms = [], {}, {}
        self._ctx = None

    def save_kun(self, path):
        """Write every parameter of the model as its `data||gama` blob plus the config tensor (Fish::SAFETENSOR_Serialize, save branch)."""
        rc = self.host.kfh_save_kun(self.h, str(path).encode())
        if rc != 0:
            raise L.KFError("kfh_save_kun(%s) failed with %d: %s" % (path, rc, self.host.kfh_last_error().decode()))

    def close(self):
        """the objects built on this model (XcdReplicas / XcdTP: they read its context and weights when they go) are closed first"""
        for d in list(getattr(self, "_dependents", ())):
            try:
                d.close()
            except Exception:
                pass
        if getattr(self, "h", None):
            self.host.kfh_destroy(self.h)
            self.h = None

    def _depends(self, obj):
        import weakref
        if not hasattr(self, "_dependents"):
            self._dependents = weakref.WeakSet()
        self._dependents.add(obj)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weight(self, layer, slot, w):
        """w: DevWeight (already in HBM)."""
        self._keep.append(w)
        self.weights[(layer, slot)] = w
        if isinstance(w, LutDevWeight) and w.bits != 4:   # NF3 layer matrices (the host refuses other widths, the embedding and the head, with a reason)
            if w.rtn:
                raise L.KFError("set_weight: the 2-bit row forms are operator-level storage (the reference has no quantiser for them)")
            rc = self.host.kfh_set_weight_lut_bits(self.h, layer, slot, w.bits, w.ne0, w.ne1, C.c_void_p(w.blob.data_ptr()), C.c_size_t(w.blob.numel()), C.c_size_t(w.szData), 1)
            if rc != 0:
                raise L.KFError("kfh_set_weight_lut_bits failed: code %d: %s" % (rc, self.host.kfh_host_error().decode()))
            return
        if isinstance(w, LutDevWeight):
            L.check(self.host.kfh_set_weight_lut(self.h, layer, slot, w.ne0, w.ne1, C.c_void_p(w.blob.data_ptr()), C.c_size_t(w.blob.numel()), C.c_size_t(w.szData), 1),
                    "kfh_set_weight_lut")
            return
        L.check(self.host.kfh_set_weight(self.h, layer, slot, w.type, w.ne0, w.ne1, C.c_void_p(w.blob.data_ptr()), w.blob.numel(), w.szData, 1, w.lGroup,
                                         w.qMin, w.qMax, w.qBias), "kfh_set_weight")

    def tie_head(self):
        L.check(self.host.kfh_tie_head(self.h), "kfh_tie_head")
        self.weights[(-1, 1)] = self.weights[(-1, 0)]

    def set_norm(self, layer, slot, w_bf16):
        w_bf16 = w_bf16.contiguous()
        self._keep.append(w_bf16)
        self._norms[(layer, slot)] = w_bf16
        L.check(self.host.kfh_set_norm(self.h, layer, slot, C.c_void_p(w_bf16.data_ptr()), w_bf16.numel(), 1), "kfh_set_norm")

    def set_fuse_level(self, lvl):
        rc = self.host.kfh_set_fuse_level(self.h, lvl)
        if rc != 0:   # refused only while the int8 KV cache is on
            raise L.KFError("set_fuse_level failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))

    def set_hot(self, layer, hot):
        """sparse forward (D_matmul_sparse / CS_Picker::hot): hot[ffn] int32 host array, 1 = the FFN row of gate / up is computed; None = dense"""
        if hot is None:
            L.check(self.host.kfh_set_hot(self.h, int(layer), None, 0), "kfh_set_hot")
            self._hot.pop(layer, None) if hasattr(self, "_hot") else None
            return
        a = np.ascontiguousarray(hot, dtype=np.int32)
        rc = self.host.kfh_set_hot(self.h, int(layer), a.ctypes.data_as(C.c_void_p), a.size)
        if rc != 0 and (getattr(self, "_act_int8", False) or getattr(self, "_act_int8_q4", False) or getattr(self, "_adapters", None) or self.kv_int8()):   # the refusals the host explains: a mask while int8 activations are on or adapters are attached (the text is set on those paths only)
            raise L.KFError("kfh_set_hot failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))
        L.check(rc, "kfh_set_hot")
        if not hasattr(self, "_hot"):
            self._hot = {}
        self._hot[layer] = int(self.host.kfh_n_hot(self.h, int(layer)))

    def set_engine(self, on):
        """The persistent decode engine (kf_engine_*: all layers of a step in one launch) on / off; off = the five launches per layer.
        Same arithmetic either way, bit for bit, in the canonical order (the default); in the v_dot2c order the engine's fp32 attention sums are its own (tolerances)."""
        L.check(self.host.kfh_set_engine(self.h, int(bool(on))), "kfh_set_engine")

    def set_act_int8(self, on):
        """int8 activations for every ternary / 1-bit layer matrix (kf_act_quant_i8 + kf_linear_a8; embedding, final norm and head untouched), in forward, run_steps,
        generate, prefill, score and perplexity, on per-layer launches (engine_why() then says so).  Raises with the reason when no layer matrix is ternary / 1-bit, a group
        zero is not 0 or a hot-row mask is set.  step_bytes is unchanged: the weights read are the same."""
        rc = self.host.kfh_set_act_int8(self.h, int(bool(on)))
        if rc != 0:
            raise L.KFError("set_act_int8 failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))
        self._act_int8 = bool(on)

    def set_act_int8_q4(self, on):
        """int8 activations for every 4-bit (KF_Q4 group storage) layer matrix (kf_act_quant_i8 + kf_linear_w4a8 / kf_linear_w4a8_tiles; include/kf_abi.h "int8 activations
        for 4-bit layers"), in forward, run_steps, generate, prefill, score and perplexity, on per-layer launches.  A second switch, independent of set_act_int8: a mixed
        model with both on sends its ternary / 1-bit matrices to kf_linear_a8 and its 4-bit ones to kf_linear_w4a8.  Raises with the reason when no layer matrix is
        served or a hot-row mask is set."""
        rc = self.host.kfh_set_act_int8_q4(self.h, int(bool(on)))
        if rc != 0:
            raise L.KFError("set_act_int8_q4 failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))
        self._act_int8_q4 = bool(on)

    def set_kv_int8(self, on):
        """The int8 KV cache (include/kf_abi.h "int8 KV cache"): K / V rows as int8 codes with one fp32 step per row and kv-head, decode attention on exact integer scores
        (kf_attn_block_kv8), token batches on the dequantised rows (or, with set_kv_int8_prefill, on the int8 rows); forward, run_steps, generate (graphs included), prefill, score and perplexity, on per-layer launches
        (engine_why() says so).  The two caches are independent: switching converts nothing, prefill again.  Raises with the reason on a TP rank, with int8 activations,
        adapters, a hot-row mask or fuse_level 0."""
        rc = self.host.kfh_set_kv_int8(self.h, int(bool(on)))
        if rc != 0:
            raise L.KFError("set_kv_int8 failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))

    def kv_int8(self):
        return bool(self.host.kfh_kv_int8(self.h))

    def set_kv_int8_prefill(self, on):
        """The int8 prompt attention, a sub-setting of the int8 KV cache (include/kf_abi.h "int8 KV cache, the prompt form"): prefill, score, perplexity and every
        chunk of them attend to the int8 rows themselves (kf_attn_prefill_kv8: integer scores, the decode kernel's score and weight arithmetic) instead of the
        dequantised staging pair.  Off by default; off: the dequantise route, bit for bit.  Raises with the reason unless set_kv_int8(True) came first;
        set_kv_int8(False) switches it off too.  Captured graphs are dropped at the switch."""
        rc = self.host.kfh_set_kv_int8_prefill(self.h, int(bool(on)))
        if rc != 0:
            raise L.KFError("set_kv_int8_prefill failed with %d: %s" % (rc, self.host.kfh_host_error().decode()))

    def kv_int8_prefill(self):
        return bool(self.host.kfh_kv_int8_prefill(self.h))

    def kv8_route_counts(self, reset=False):
        """prompt-attention launches of the token batches on the int8 cache since the last reset: {"prefill_int8": kf_attn_prefill_kv8, "prefill_dequant": the
        dequantise route}; reset=True zeroes them after the read"""
        out = (C.c_int64 * 2)()
        L.check(self.host.kfh_kv8_route_counts(self.h, out, int(bool(reset))), "kfh_kv8_route_counts")
        return {"prefill_int8": int(out[0]), "prefill_dequant": int(out[1])}

    def kv8_to_host(self):
        """the int8 cache copied to the host: (k8 int8 [n_layer, max_seq, kv_dim], ks fp32 [n_layer, max_seq, n_kv], v8, vs); allocated by the first set_kv_int8(True)"""
        c = self.cfg
        kvd, rows = c["n_kv"] * c["head_dim"], c["n_layer"] * c["max_seq"]
        ctx = C.c_void_p(self.host.kfh_ctx(self.h))
        out = []
        for val in (0, 1):
            codes, steps = np.zeros(rows * kvd, dtype=np.int8), np.zeros(rows * c["n_kv"], dtype=np.float32)
            for a, p in ((codes, self.host.kfh_kv8_codes(self.h, val)), (steps, self.host.kfh_kv8_steps(self.h, val))):
                if not p:
                    raise L.KFError("kv8_to_host: the int8 cache is allocated by the first set_kv_int8(True)")
                L.check(self.hip.kf_d2h(ctx, a.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(a.nbytes)), "kf_d2h")
            out += [codes.reshape(c["n_layer"], c["max_seq"], kvd), steps.reshape(c["n_layer"], c["max_seq"], c["n_kv"])]
        return tuple(out)

    @classmethod
    def check_adapters(cls, cfg, adapters, lora_s):
        """every argument error of set_adapters as a ValueError, without a device: names "l<layer>.<target>.w" with target out of q k v o gate up down, (a [r, in],
        b [out, r]) bf16 tensors of ONE rank 16 / 32 / 64, a finite lora_s.  Returns [(layer, slot, a, b)] and the rank."""
        if not (isinstance(lora_s, (int, float)) and lora_s == lora_s and abs(lora_s) != float("inf")):
            raise ValueError("lora_s %r: a finite number" % (lora_s,))
        if not adapters:
            raise ValueError("adapters: an empty dict (clear_adapters() detaches)")
        dim, H, KV, hd, ffn = (cfg[k] for k in ("dim", "n_head", "n_kv", "head_dim", "ffn"))
        shapes = dict(q=(H * hd, dim), k=(KV * hd, dim), v=(KV * hd, dim), o=(dim, H * hd), gate=(ffn, dim), up=(ffn, dim), down=(dim, ffn))
        out, rank = [], None
        for name, ab in adapters.items():
            l, _, k = name[1:].partition(".")
            if not (name[:1] == "l" and l.isdigit() and int(l) < cfg["n_layer"] and k.endswith(".w") and k[:-2] in SLOTS):
                raise ValueError("adapters: %r is no layer matrix (names are l<layer>.<target>.w, target out of %s)" % (name, SLOTS))
            OC, IC = shapes[k[:-2]]
            if len(ab) != 2 or any(not torch.is_tensor(t) or t.dim() != 2 for t in ab):
                raise ValueError("adapters[%r]: a pair of 2-D tensors (a [r, %d], b [%d, r])" % (name, IC, OC))
            a, b = ab
            if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
                raise ValueError("adapters[%r]: bf16 tensors (got %s, %s)" % (name, a.dtype, b.dtype))
            r = a.shape[0]
            if r not in (16, 32, 64) or tuple(a.shape) != (r, IC) or tuple(b.shape) != (OC, r):
                raise ValueError("adapters[%r]: a [r, %d], b [%d, r] with r 16, 32 or 64 (got %s, %s)" % (name, IC, OC, tuple(a.shape), tuple(b.shape)))
            if rank is not None and r != rank:
                raise ValueError("adapters[%r]: rank %d beside rank %d -- one rank per model" % (name, r, rank))
            rank = r
            out.append((int(l), SLOTS.index(k[:-2]), a, b))
        return out, rank

    def set_adapters(self, adapters, lora_s=1.0):
        """Attach trained low-rank pairs (Qwen3Step.lora_state()'s layout): {"l<layer>.<target>.w": (a [r, in], b [out, r])} of bf16 DEVICE tensors, any subset of the
        layers' seven matrices, one rank; lora_s multiplies both products (effective weight lora_s^2 b a).  No copy: the model keeps the tensors alive and reads them at
        every launch, so an in-place update is seen.  forward, run_steps, generate, prefill, score and perplexity then apply them (kf_lora_apply after each base product)
        on per-layer launches -- engine_why() says so; the packed base stays byte for byte.  Replaces whatever was attached.  ValueError for a bad argument (before
        anything touches the device); KFError when the model refuses: a TP rank, int8 activations on, a hot-row mask set, a shape kf_lora_apply does not serve."""
        items, rank = self.check_adapters(self.cfg, adapters, lora_s)
        for _, _, a, b in items:
            if a.device != self.device or b.device != self.device or not a.is_contiguous() or not b.is_contiguous():
                raise ValueError("adapters: contiguous tensors on %s" % (self.device,))
        self.clear_adapters()
        for layer, slot, a, b in items:
            rc = self.host.kfh_set_adapter(self.h, layer, slot, _ptr(a), _ptr(b), rank, float(lora_s))
            if rc != 0:
                why = self.host.kfh_host_error().decode()
                self.clear_adapters()
                raise L.KFError("set_adapters failed with %d: %s" % (rc, why))
        self._adapters, self._lora_s = {name: tuple(ab) for name, ab in adapters.items()}, float(lora_s)

    def clear_adapters(self):
        """detach every adapter: the fused launches, the engines and the captured graphs serve the model again, bit for bit as before set_adapters"""
        L.check(self.host.kfh_clear_adapters(self.h), "kfh_clear_adapters")
        self._adapters = {}

    def adapters(self):
        """{name: (a, b)} of what is attached (the tensors themselves)"""
        return dict(getattr(self, "_adapters", {}))

    def set_a8_tile_min(self, n):
        """token batches of at least n rows send their ternary / 1-bit matrices to the int8 MFMA tiles (kf_linear_a8_tiles) while int8 activations are on, smaller ones and
        single tokens to the mat-vec (kf_linear_a8): n >= 2 sets the threshold (1 is treated as 2), 0 restores the default (32), n < 0 = never.  The bits are the same."""
        L.check(self.host.kfh_set_a8_tile_min(self.h, int(n)), "kfh_set_a8_tile_min")

    def a8_route_counts(self):
        """(tile launches, mat-vec launches) of both integer families (kf_linear_a8*, kf_linear_w4a8*) since the last set_act_int8(True) / set_act_int8_q4(True)"""
        out = (C.c_int64 * 2)()
        L.check(self.host.kfh_a8_route_counts(self.h, out), "kfh_a8_route_counts")
        return int(out[0]), int(out[1])

    def set_canonical(self, on):
        """1 (the library default): the decode kernels sum in the canonical order the CPU oracle shares (bit-exact logits, ids and KV rows); 0: the v_dot2c_f32_bf16 / fp32 forms"""
        L.check(self.host.kfh_set_canonical(self.h, int(bool(on))), "kfh_set_canonical")

    def engine_why(self):
        """why the persistent engine does not serve this model ("" when it does)"""
        self.host.kfh_engine_why.restype = C.c_char_p
        return self.host.kfh_engine_why(self.h).decode()

    def engine_tune(self, passes=2):
        """kf_engine_tune at the position the decode state holds: (mean launch us before, after)"""
        us = (C.c_float * 2)()
        L.check(self.host.kfh_engine_tune(self.h, int(passes), us), "kfh_engine_tune")
        return float(us[0]), float(us[1])

    def set_engine_autotune(self, passes):
        """> 0: the hand-off delays are measured once per position bucket, at the first multi-step launch inside it (passes of kf_engine_tune)"""
        L.check(self.host.kfh_set_engine_autotune(self.h, int(passes)), "kfh_set_engine_autotune")

    def weights_changed(self):
        """after an IN-PLACE update of weight data handed over as device pointers: drops the resident bf16 copies, the engine's tables and the captured graphs"""
        L.check(self.host.kfh_weights_changed(self.h), "kfh_weights_changed")

    def set_prefill_resident(self, on, max_bytes=0):
        """bf16 copies of the layers' quantised matrices kept in HBM for long prompts (kf_set_dequant_arena): takes effect at the next prefill.  OFF by default; turning it
        on is the caller's promise that weight data given as device pointers is not changed in place afterwards (or that weights_changed() is called when it is): the
        copies are keyed by the blobs' addresses.  max_bytes: budget (default 16 GiB; Qwen3-32B needs 62 GB)."""
        L.check(self.host.kfh_set_prefill_resident(self.h, int(bool(on)), int(max_bytes)), "kfh_set_prefill_resident")

    def resident_bytes(self):
        """bytes of resident dequantised copies the prefill has filled so far"""
        return int(self.host.kfh_resident_bytes(self.h))

    def engine_stats(self, pos):
        """kf_engine_stats: {'sweeps_per_poll': [6], 'polls', 'delay': [6], 'tuned'} for the hand-offs x, q|k|v, slice partials, ao, xB, act"""
        w = (C.c_int32 * 14)()
        L.check(self.host.kfh_engine_stats(self.h, int(pos), w), "kfh_engine_stats")
        polls = max(int(w[6]), 1)
        return {"sweeps_per_poll": [round(int(w[i]) / polls, 3) for i in range(6)], "polls": int(w[6]), "delay": [int(w[7 + i]) for i in range(6)], "tuned": int(w[13])}

    def engine_screen_stats(self):
        """kf_engine_screen_stats: the head screen's counters since the engine was built or reset (zeros when there is none)"""
        w = (C.c_int64 * 3)()
        L.check(self.host.kfh_engine_screen_stats(self.h, w), "kfh_engine_screen_stats")
        return {"screened_steps": int(w[0]), "rows_reranked": int(w[1]), "wg_fallbacks": int(w[2])}

    def engine_steps(self):
        """steps enqueued or captured through the engine so far (-1: the engine does not serve this model's shapes / storage)"""
        return int(self.host.kfh_engine_steps(self.h))

    def engine_only(self, n):
        """n launches of the engine kernel alone at the position the device state holds (timing); returns False when the engine does not serve the model"""
        rc = self.host.kfh_engine_only(self.h, int(n))
        if rc == 1:
            return False
        L.check(rc, "kfh_engine_only")
        return True

    def engine_check(self):
        """synchronises; raises when one of the engine's hand-off polls timed out (the launch was not fully resident)"""
        L.check(self.host.kfh_engine_check(self.h), "kfh_engine_check")

    def forward(self, token, pos, want_logits=True):
        logits = np.zeros(self.cfg["vocab"], dtype=np.uint16) if want_logits else None
        r = self.host.kfh_forward(self.h, int(token), int(pos), None if logits is None else logits.ctypes.data_as(C.c_void_p))
        if r < 0:
            L.check(r, "kfh_forward")
        return r, logits

    def generate(self, prompt, n_new, use_graph=True):
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        out = np.zeros(n_new, dtype=np.int32)
        L.check(self.host.kfh_generate(self.h, p.ctypes.data_as(C.c_void_p), p.size, n_new, out.ctypes.data_as(C.c_void_p), int(use_graph)), "kfh_generate")
        return out.tolist()

    # ---- speculative decoding (host/kf_spec.hpp, Fish::Verify, koifish::SpecDecoder)
    def _host_check(self, rc, what):
        if rc != 0:
            why = self.host.kfh_host_error().decode()
            raise L.KFError("%s failed with %d: %s" % (what, rc, why or self.hip.kf_last_error().decode()))

    def verify(self, tokens, pos0, want_logits=False):
        """The verify pass: R = len(tokens) <= 8 tokens at positions pos0 .. pos0 + R - 1 -- a token and its drafted continuations -- through every layer with ONE pass
        over the weights.  Returns top1 [R] (the greedy id behind each row), and with want_logits the rows' logits as uint16 [R, vocab].  In the canonical order row i
        carries every bit (id, logits, K / V rows pos0 + i) of forward(tokens[i], pos0 + i) called one after the other.  The decode state is not touched.  Raises with
        the reason while a mode is on (TP, int8 activations, adapters, int8 KV cache, hot-row masks, fuse_level 0) or a sampler is set."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        top1 = np.zeros(t.size, dtype=np.int32)
        logits = np.zeros((t.size, self.cfg["vocab"]), dtype=np.uint16) if want_logits else None
        self._host_check(self.host.kfh_verify(self.h, t.ctypes.data_as(C.c_void_p), t.size, int(pos0), top1.ctypes.data_as(C.c_void_p),
                                              None if logits is None else logits.ctypes.data_as(C.c_void_p)), "kfh_verify")
        return (top1, logits) if want_logits else top1

    def generate_speculative(self, prompt, n_new, draft="lookup", k=4, ngram=3):
        """generate()'s ids -- id for id -- by rounds of "propose k ids, verify them in one pass over the weights, keep the longest prefix the model agrees with".
        draft: another Qwen3 on this device with this vocabulary (its greedy steps, the engine included), "lookup" (the longest suffix of the context, up to `ngram`
        ids, found earlier in the context proposes what followed it: no model), or a callable (ids, k) -> up to k proposed ids.  k = 1 .. 7.  spec_stats() counts."""
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        out = np.zeros(n_new, dtype=np.int32)
        s = self.host.kfh_spec_create(self.h, int(k))
        if not s:
            raise L.KFError("kfh_spec_create: %s" % self.host.kfh_host_error().decode())
        keep = None
        try:
            if isinstance(draft, Qwen3):
                L.check(self.host.kfh_spec_set_draft_model(s, draft.h), "kfh_spec_set_draft_model")
            elif draft == "lookup":
                L.check(self.host.kfh_spec_set_lookup(s, int(ngram)), "kfh_spec_set_lookup")
            elif callable(draft):
                def cb(ids, n, kk, outp, _user):
                    got = list(draft([ids[i] for i in range(n)], kk))[:kk]
                    for i, g in enumerate(got):
                        outp[i] = int(g)
                    return len(got)
                keep = L.SPEC_DRAFT_FN(cb)
                L.check(self.host.kfh_spec_set_callback(s, keep, None), "kfh_spec_set_callback")
            else:
                raise L.KFError("generate_speculative: draft is a Qwen3, \"lookup\" or a callable")
            rc = self.host.kfh_spec_generate(s, p.ctypes.data_as(C.c_void_p), p.size, int(n_new), out.ctypes.data_as(C.c_void_p))
            st = (C.c_int64 * 5)()
            self.host.kfh_spec_stats(s, st)
            self._spec = {"rounds": int(st[0]), "proposed": int(st[1]), "accepted": int(st[2]), "rows_shared": int(st[3]), "rows_row_by_row": int(st[4])}
            self._host_check(rc, "kfh_spec_generate")
        finally:
            self.host.kfh_spec_destroy(s)
        return out.tolist()

    def spec_stats(self):
        """the last generate_speculative: rounds, ids proposed, ids accepted, and the activation rows its verify passes' mat-vec entries served with the shared unpack
        (rows_shared) and with one-token launches (rows_row_by_row: the v_dot2c order, storages the row kernel does not take, one-row rounds)"""
        return dict(getattr(self, "_spec", {"rounds": 0, "proposed": 0, "accepted": 0, "rows_shared": 0, "rows_row_by_row": 0}))

    def set_sampler(self, temperature=0.0, top_p=0.95, top_k=50, seed=42, true_topk=False):
        """CHAT_SAMPLER: temperature 0 (or top_k 1) = greedy; otherwise GeneratOnPrompt::Sample on the device, rng reseeded here.
        true_topk: candidates = the k largest logits (kf_sample_topk) instead of the set the reference's heap keeps (kf_sample)."""
        L.check(self.host.kfh_set_sampler(self.h, float(temperature), float(top_p), int(top_k) | (0x10000 if true_topk else 0), int(seed)), "kfh_set_sampler")

    def set_prefill_mode(self, mode, chunk=0):
        """generate(): 0 = token-serial prefill through the decode path (like the reference), 1 = token batches on the MFMA kernels"""
        L.check(self.host.kfh_set_prefill_mode(self.h, int(mode), int(chunk)), "kfh_set_prefill_mode")

    def prefill(self, tokens, pos0=0, want_logits=True):
        """Batched prefill of `tokens` at positions pos0..; returns (greedy next id, logits of the last token as uint16 or None)."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        L.check(self.host.kfh_prefill(self.h, t.ctypes.data_as(C.c_void_p), t.size, int(pos0)), "kfh_prefill")
        nxt = int(self.tokens_out(pos0 + t.size)[pos0 + t.size - 1])
        logits = None
        if want_logits:
            logits = np.zeros(self.cfg["vocab"], dtype=np.uint16)
            ctx = C.c_void_p(self.host.kfh_ctx(self.h))
            L.check(self.hip.kf_d2h(ctx, logits.ctypes.data_as(C.c_void_p), C.c_void_p(self.host.kfh_logits(self.h)), C.c_size_t(logits.size * 2)), "kf_d2h")
        return nxt, logits

    def score(self, tokens, pos0=0, want_top1=False):
        """log P(tokens[i + 1] | tokens[.. i]) for every i < n - 1 as np.float32 [n - 1] (and, with want_top1, the greedy id after each of those tokens as
        np.int32 [n - 1]): the prompt through the batched prefill and the LM head with the log-softmax in its epilogue (Fish::Score).  K / V rows, logits,
        next id and decode state are left as prefill(tokens, pos0) leaves them."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        lp = np.zeros(max(t.size - 1, 0), dtype=np.float32)
        top1 = np.zeros(max(t.size - 1, 0), dtype=np.int32) if want_top1 else None
        L.check(self.host.kfh_score(self.h, t.ctypes.data_as(C.c_void_p), t.size, int(pos0), lp.ctypes.data_as(C.c_void_p),
                                    None if top1 is None else top1.ctypes.data_as(C.c_void_p)), "kfh_score")
        return (lp, top1) if want_top1 else lp

    def perplexity(self, tokens, window=None):
        """(ppl, pplerr, n_scored) of a token sequence as Fish::Eval_ppl reports them: windows of at most `window` tokens (default: the context), each scored
        from position 0; the sums in fp64 on the host (Fish::EvalPPL).  perplexity_from_logprobs is the same arithmetic on given log-probs."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        ppl, err, nz = C.c_double(0.0), C.c_double(0.0), C.c_longlong(0)
        L.check(self.host.kfh_eval_ppl(self.h, t.ctypes.data_as(C.c_void_p), t.size, int(window or 0), C.byref(ppl), C.byref(err), C.byref(nz)), "kfh_eval_ppl")
        return ppl.value, err.value, int(nz.value)

    def logits(self):
        """the last step's logits (bf16 bit patterns as uint16 [vocab])"""
        out = np.zeros(self.cfg["vocab"], dtype=np.uint16)
        ctx = C.c_void_p(self.host.kfh_ctx(self.h))
        L.check(self.hip.kf_d2h(ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.host.kfh_logits(self.h)), C.c_size_t(out.size * 2)), "kf_d2h")
        return out

    def set_forced(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        L.check(self.host.kfh_set_forced(self.h, a.ctypes.data_as(C.c_void_p), a.size), "kfh_set_forced")

    def set_state(self, token, pos):
        L.check(self.host.kfh_set_state(self.h, int(token), int(pos)), "kfh_set_state")

    def run_steps(self, pos, n, use_graph=True):
        L.check(self.host.kfh_run_steps(self.h, int(pos), int(n), int(use_graph)), "kfh_run_steps")

    def sync(self):
        L.check(self.host.kfh_sync(self.h), "kfh_sync")

    def tokens_out(self, n):
        out = np.zeros(n, dtype=np.int32)
        L.check(self.host.kfh_get_tokens(self.h, out.ctypes.data_as(C.c_void_p), n), "kfh_get_tokens")
        return out

    def kv_to_host(self):
        """KV cache copied to host as uint16 arrays [n_layer, max_seq, kv_dim]."""
        c = self.cfg
        kvd = c["n_kv"] * c["head_dim"]
        n = c["n_layer"] * c["max_seq"] * kvd
        k = np.zeros(n, dtype=np.uint16)
        v = np.zeros(n, dtype=np.uint16)
        ctx = C.c_void_p(self.host.kfh_ctx(self.h))
        L.check(self.hip.kf_d2h(ctx, k.ctypes.data_as(C.c_void_p), C.c_void_p(self.host.kfh_kcache(self.h)), C.c_size_t(n * 2)), "kf_d2h")
        L.check(self.hip.kf_d2h(ctx, v.ctypes.data_as(C.c_void_p), C.c_void_p(self.host.kfh_vcache(self.h)), C.c_size_t(n * 2)), "kf_d2h")
        shp = (c["n_layer"], c["max_seq"], kvd)
        return k.reshape(shp), v.reshape(shp)

    def num_graphs(self):
        return self.host.kfh_num_graphs(self.h)

    def step_bytes(self, pos):
        """Algorithmic HBM bytes of one decode step at position `pos`: every weight's packed data +
        zero/step once, the norm vectors, and the KV rows 0..pos read once plus the new row written."""
        c = self.cfg
        kvd = c["n_kv"] * c["head_dim"]
        wb = 0
        hot = getattr(self, "_hot", {})
        for (layer, slot), w in self.weights.items():
            if layer == -1 and slot == 0:
                continue  # embedding: one row
            if layer in hot and slot in (4, 5):   # sparse forward: only the hot rows of gate / up are read
                wb += w.algorithmic_bytes() * hot[layer] // w.ne0
                continue
            wb += w.algorithmic_bytes()
        emb = self.weights[(-1, 0)]
        wb += emb.algorithmic_bytes() // emb.ne0
        norms = (c["n_layer"] * (2 * c["dim"] + 2 * c["head_dim"]) + c["dim"]) * 2
        kv = 2 * c["n_layer"] * (pos + 1) * kvd * 2 + 2 * c["n_layer"] * kvd * 2
        return wb + norms + kv


class XcdReplicas:
    """Up to eight independent decoders of ONE model on one GPU, one per XCD (koifish::XcdReplicas over kf_xengine_*): the sequences share the model's weights; each has its
    own KV cache, decode state, forced ids, ids out and logits.  Every sequence's results are bit for bit those of `model.run_steps` for it alone (canonical order)."""

    def __init__(self, model, n_seq=8):
        self.m, self.n_seq = model, int(n_seq)
        self.host, self.hip = model.host, model.hip
        rc = C.c_int(0)
        h = self.host.kfh_xr_create(model.h, self.n_seq, C.byref(rc))
        if not h:
            raise L.KFError("kfh_xr_create failed with %d: %s" % (rc.value, self.host.kfh_host_error().decode() or self.hip.kf_last_error().decode()))
        self.h = C.c_void_p(h)
        model._depends(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.m, "h", None):   # a garbage cycle (a failed test's frame) finalises in any order: a model that went first took the context with it
                self.host.kfh_xr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_forced(self, seq, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        L.check(self.host.kfh_xr_set_forced(self.h, int(seq), a.ctypes.data_as(C.c_void_p), a.size), "kfh_xr_set_forced")

    def set_state(self, seq, token, pos):
        L.check(self.host.kfh_xr_set_state(self.h, int(seq), int(token), int(pos)), "kfh_xr_set_state")

    def prefill(self, seq, tokens):
        """the sequence's prompt through the model's batched prefill; its K / V rows into the sequence's cache; the sequence then stands behind the prompt (state = {first generated id, len(tokens)})"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        L.check(self.host.kfh_xr_prefill(self.h, int(seq), t.ctypes.data_as(C.c_void_p), t.size), "kfh_xr_prefill")

    def run_steps(self, n):
        """n greedy steps of EVERY sequence from wherever each stands; no host sync"""
        L.check(self.host.kfh_xr_run_steps(self.h, int(n)), "kfh_xr_run_steps")

    def set_steps_per_launch(self, n):
        L.check(self.host.kfh_xr_set_steps_per_launch(self.h, int(n)), "kfh_xr_set_steps_per_launch")

    def check(self):
        L.check(self.host.kfh_xr_check(self.h), "kfh_xr_check")

    @property
    def batch(self):
        """sequences per decoder of the form the engine launches: 1 (<= 8 sequences), 2 (<= 16) or 4 (<= 32): every unpacked block is multiplied against that many sequences' activations"""
        return 1 if self.n_seq <= 8 else (2 if self.n_seq <= 16 else 4)

    decoders_per_xcd = 1

    def park(self, seq, on=True):
        """a parked sequence is skipped by the launches; the others decode on"""
        L.check(self.host.kfh_xr_park(self.h, int(seq), int(bool(on))), "kfh_xr_park")

    def prefill_batch(self, slots, prompts):
        """several prompts at once (one token batch of len(prompts) x longest rows through the tile kernels; a prompt's rows attend to that prompt only): every prompt's
        K / V rows into its slot's cache, the slot stands behind its prompt, the last prompt token's logits in the slot's logits"""
        n = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        stride = int(lens.max())
        flat = np.zeros((n, stride), dtype=np.int32)
        for i, p in enumerate(prompts):
            flat[i, :len(p)] = p
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        L.check(self.host.kfh_xr_prefill_batch(self.h, sl.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, stride), "kfh_xr_prefill_batch")

    def set_prefill_batch(self, n):
        """chat(): up to n waiting prompts are prefilled together when as many slots are free (1, the default: one by one -- the bits of the model's own prefill)"""
        L.check(self.host.kfh_xr_set_prefill_batch(self.h, int(n)), "kfh_xr_set_prefill_batch")

    def set_sampler(self, temperature=0.0, top_p=0.95, top_k=50, seed=42, true_topk=False):
        """chat()'s sampler (CHAT_SAMPLER; greedy by default).  Non-greedy: one launch per token leaves every slot's logits, kf_sample draws each slot's id with the slot's own
        rng, seeded with seed + the request's index at the request's start -- answer r == the model alone on prompt r under set_sampler(seed=seed + r)."""
        L.check(self.host.kfh_xr_set_sampler(self.h, float(temperature), float(top_p), int(top_k) | (0x10000 if true_topk else 0), int(seed)), "kfh_xr_set_sampler")

    def chat(self, prompts, max_new, eos=-1, max_new_each=None):
        """a queue of prompts answered through the sequences' slots (Fish::Chat's rounds over its prompt list, GoPT.cpp:1111-1180, n_seq rounds in flight): a free slot
        prefills the next prompt, the launches decode every occupied slot, an answer ends at `eos`, at max_new ids or at the last cache row.
        max_new_each: a limit of its own per request (each <= max_new).
        Returns (list of id lists in the prompts' order, {launches, steps, prefills, dropped})."""
        n = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        stride = int(lens.max())
        flat = np.zeros((n, stride), dtype=np.int32)
        for i, p in enumerate(prompts):
            flat[i, :len(p)] = p
        out = np.zeros((n, int(max_new)), dtype=np.int32)
        out_len = np.zeros(n, dtype=np.int32)
        stats = np.zeros(4, dtype=np.int64)
        each = None if max_new_each is None else np.ascontiguousarray(max_new_each, dtype=np.int32)
        assert each is None or each.size == n
        L.check(self.host.kfh_xr_chat_each(self.h, flat.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, stride, int(max_new), int(eos),
                                           out.ctypes.data_as(C.c_void_p), out_len.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p),
                                           None if each is None else each.ctypes.data_as(C.c_void_p)), "kfh_xr_chat_each")
        return [out[i, :out_len[i]].tolist() for i in range(n)], dict(zip(("launches", "steps", "prefills", "dropped"), (int(v) for v in stats)))

    def status(self, seq):
        """{token, pos, parked, status} of the sequence (status 64: the last launch would have left its cache rows and skipped it)"""
        out = np.zeros(4, dtype=np.int32)
        L.check(self.host.kfh_xr_status(self.h, int(seq), out.ctypes.data_as(C.c_void_p)), "kfh_xr_status")
        return [int(v) for v in out]

    def state(self, seq):
        out = np.zeros(2, dtype=np.int32)
        L.check(self.host.kfh_xr_get_state(self.h, int(seq), out.ctypes.data_as(C.c_void_p)), "kfh_xr_get_state")
        return int(out[0]), int(out[1])

    def tokens_out(self, seq, n):
        out = np.zeros(n, dtype=np.int32)
        L.check(self.host.kfh_xr_get_tokens(self.h, int(seq), out.ctypes.data_as(C.c_void_p), n), "kfh_xr_get_tokens")
        return out

    def _d2h(self, ptr, n_u16):
        out = np.zeros(n_u16, dtype=np.uint16)
        ctx = C.c_void_p(self.host.kfh_ctx(self.m.h))
        L.check(self.hip.kf_d2h(ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.size * 2)), "kf_d2h")
        return out

    def logits(self, seq):
        """the sequence's last logits (bf16 bit patterns as uint16 [vocab])"""
        return self._d2h(self.host.kfh_xr_logits(self.h, int(seq)), self.m.cfg["vocab"])

    def hidden(self, seq):
        return self._d2h(self.host.kfh_xr_hidden(self.h, int(seq)), self.m.cfg["dim"])

    def kv_to_host(self, seq):
        c = self.m.cfg
        kvd = c["n_kv"] * c["head_dim"]
        n = c["n_layer"] * c["max_seq"] * kvd
        shp = (c["n_layer"], c["max_seq"], kvd)
        return self._d2h(self.host.kfh_xr_kcache(self.h, int(seq)), n).reshape(shp), self._d2h(self.host.kfh_xr_vcache(self.h, int(seq)), n).reshape(shp)

    def variant(self, nwv, depth):
        """A/B hook of the next launches: variant(-2, 1) runs 9 .. 16 sequences through the round-5 form (two decoders per XCD), variant(-2, 0) back; other codes are refused"""
        if self.host.kfh_xr_variant(self.h, int(nwv), int(depth)) != 0:
            raise ValueError("xengine variant (%d, %d): only (-2, 0 | 1) is served" % (nwv, depth))

    def stamps(self, seq, wg, steps, n_layer):
        """enable (steps > 0) / read the per-phase wall-clock stamps [step][layer][64] of one workgroup of one decoder (diagnostic instantiation)"""
        if steps > 0:
            L.check(self.host.kfh_xr_stamps_enable(self.h, int(seq), int(wg), int(steps)), "kfh_xr_stamps_enable")
            return None
        out = np.zeros((-steps) * n_layer * 64, dtype=np.uint64)
        self.host.kfh_xr_stamps(self.h, out.ctypes.data_as(C.c_void_p), out.size)
        return out.reshape(-steps, n_layer, 64)


class XcdTP:
    """ONE sequence of a model split over eight tensor-parallel ranks, the ranks as the eight XCDs of ONE launch (koifish::XcdTP over kf_xengine_create_tp).  `native_tp`: a
    koifish_amd.tp.NativeTP -- its ranks hold the shards (and stay usable: the per-launch rank step and this engine give the same bits).  K / V rows, state, forced ids, ids
    out and the full logits vector live in this object."""

    def __init__(self, native_tp):
        self.nt = native_tp
        r0 = native_tp.ranks[0]
        self.host, self.hip = r0.host, r0.hip
        self._hs = (C.c_void_p * len(native_tp.ranks))(*[m.h for m in native_tp.ranks])
        rc = C.c_int(0)
        h = self.host.kfh_xtp_create(self._hs, len(native_tp.ranks), C.byref(rc))
        if not h:
            raise L.KFError("kfh_xtp_create failed with %d: %s" % (rc.value, self.host.kfh_host_error().decode() or self.hip.kf_last_error().decode()))
        self.h = C.c_void_p(h)
        for m in native_tp.ranks:
            m._depends(self)

    def close(self):
        if getattr(self, "h", None):
            if all(getattr(m, "h", None) for m in self.nt.ranks):   # (as XcdReplicas.close)
                self.host.kfh_xtp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_forced(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        L.check(self.host.kfh_xtp_set_forced(self.h, a.ctypes.data_as(C.c_void_p), a.size), "kfh_xtp_set_forced")

    def set_state(self, token, pos):
        L.check(self.host.kfh_xtp_set_state(self.h, int(token), int(pos)), "kfh_xtp_set_state")

    def run_steps(self, n):
        L.check(self.host.kfh_xtp_run_steps(self.h, int(n)), "kfh_xtp_run_steps")

    def set_steps_per_launch(self, n):
        L.check(self.host.kfh_xtp_set_steps_per_launch(self.h, int(n)), "kfh_xtp_set_steps_per_launch")

    def check(self):
        L.check(self.host.kfh_xtp_check(self.h), "kfh_xtp_check")

    def tokens_out(self, n):
        out = np.zeros(n, dtype=np.int32)
        L.check(self.host.kfh_xtp_get_tokens(self.h, out.ctypes.data_as(C.c_void_p), n), "kfh_xtp_get_tokens")
        return out

    def _d2h(self, ptr, n_u16):
        out = np.zeros(n_u16, dtype=np.uint16)
        ctx = C.c_void_p(self.host.kfh_ctx(self.nt.ranks[0].h))
        L.check(self.hip.kf_d2h(ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.size * 2)), "kf_d2h")
        return out

    def logits(self):
        """the last step's logits of the FULL vocabulary (the ranks' shards in rank order), bf16 bit patterns"""
        return self._d2h(self.host.kfh_xtp_logits(self.h), int(self.host.kfh_xtp_vocab(self.h)))

    def hidden(self):
        return self._d2h(self.host.kfh_xtp_hidden(self.h), self.nt.cfg["dim"])

    def kv_to_host(self):
        """[rank][layer][max_seq][head_dim]: rank r = kv-head r's rows"""
        c = self.nt.cfg
        kvd = (c["n_kv"] // len(self.nt.ranks)) * c["head_dim"]
        n = len(self.nt.ranks) * c["n_layer"] * c["max_seq"] * kvd
        shp = (len(self.nt.ranks), c["n_layer"], c["max_seq"], kvd)
        return self._d2h(self.host.kfh_xtp_kcache(self.h), n).reshape(shp), self._d2h(self.host.kfh_xtp_vcache(self.h), n).reshape(shp)

    def stamps(self, rank, wg, steps, n_layer):
        """enable (steps > 0) / read the per-phase wall-clock stamps [step][layer][64] of one workgroup of one rank (diagnostic instantiation)"""
        if steps > 0:
            L.check(self.host.kfh_xtp_stamps_enable(self.h, int(rank), int(wg), int(steps)), "kfh_xtp_stamps_enable")
            return None
        n = -steps * n_layer * 64
        out = np.zeros(n, dtype=np.uint64)
        self.host.kfh_xtp_stamps(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out.reshape(-steps, n_layer, 64)
