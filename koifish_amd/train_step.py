"""One WHOLE training step of the hybrid-precision GPT-2 of BASELINE config 3, every operator through the C ABI -- the host-side order of the reference's step:

  forward  (TokenEmbed, 48 x [LayerNorm, SLP qkv, causal attention, SLP proj + residual, LayerNorm, SLP fc, GELU, SLP proj2 + residual], LayerNorm, tied head)
           on the QUANTISED blobs (attention matrices f8e5m2, MLP matrices 4-bit PackedQ): SLP::Forw, NeuronFuse.cu:305-381
  loss     fused classifier (cross entropy + logit gradient in place), NeuronFuse.cu / kf_loss.hip
  backward SLP::Back (NeuronFuse.cu:495-563), LayerNormal / GELU / attention / embedding backward -- weight gradients into PER-TENSOR buffers
  update   CU_adamw_ (Optimizer.cu:135-160: seeded stochastic rounding) on the model's OWN bf16 master weights and bf16 moments
  requant  CU_XtoQ128_ / Float2T<f8e5> (T.cu:105-175) of every updated matrix back into its blob, which the next forward reads

train_target="gama" is the reference's other way to train a quantised layer ("train_target": "gama"; SLP::Back's gama branch, GTensor::InitGamaParam): a block matrix stored
as a PackedQ group type keeps its packed integers frozen and trains each group's (zero, step) pair in place inside the blob -- no bf16 master, no [OC, IC] gradient, no
moments of that size, no re-quantisation: per 128 weights two bf16 parameters, two gradients, four moments (kf_gama_backward + kf_adamw on the blob's gama slice).

train_target="lora" (Qwen3Step only) is the third way, the LORA branch of SLP::Forw / SLP::Back: the quantised matrix stays frozen as it is and a low-rank pair a [r, IN],
b [OUT, r] trains beside it (kf_lora_forward after the base product, kf_lora_backward after kf_linear_backward(gW = NULL)): no master, no [OUT, IN] gradient or moments,
no weight-gradient GEMM and no re-quantisation.  [a | b] is ONE trained vector per matrix.

layers_in_branch is the reference's EOE, "Evolutionary Optimization of Experts" (Fuyou_params::nLayerInBranch; RLSchedule::InitBranch, Fuyou::UpdateFollower,
Fish::ForwardOnRLS): the NL layers are cut into NL / layers_in_branch sections; a section plus the shared embedding, final norm and head is a shallow model of its own
(a "Fuyou").  set_branch(b) picks the one that forward / backward / update / step run; evolve(head) pulls the weight matrices of every other branch towards the head
branch's (kf_evolve: particle swarm, particle swarm + genetic crossover, or a fixed mix) and re-quantises them; eval_loss scores one branch or the mean of all.  The
schedule -- which branch trains when, which one is the head -- is the caller's loop over set_branch / step / evolve.

set_distill(teacher, kd_weight, ce_weight, temperature) on either class turns the objective into ce_weight CE + kd_weight temperature^2 KL(teacher || student) on the
logits (kf_distill_classifier in the fused classifier's place); the teacher is another trainer, whose forward_logits then runs first in every forward / step, or a
tensor of logits the caller refills.

The step keeps every activation (no recomputation).  Python here OWNS the device buffers (torch tensors: setup, outside any timed region) and registers them with
koifish::GPT2Trainer (koifish_amd/host/kf_train.cpp, libkf_host.so), which sequences the step: forward / backward / update are one C call each, step() is ONE call,
and nothing in them is a torch op (the embedding gather + add is kf_embed_pos, the attention reads q out of the fused rows, the zero fills are kf_memset / kf_memset2d).
Used by tests/test_gpu_train_step.py (a 2-layer toy, two consecutive steps against the oracle) and by bench.py's config3 leg (full size).

Qwen3Step, further down, is the same for the Qwen3 family (koifish::Qwen3Trainer, koifish_amd/host/kf_train_qwen3.cpp); the two trainers share the tensor table, SLP::Back,
the optimiser switch, the update loop and the step around them (koifish_amd/host/kf_train_common.hpp), and the two classes here share _TrainStep: the registration of
tensors and buffers with the trainer and every method that is one call into it."""
import ctypes as C

import torch

from . import lib as L

MATS = ("qkv", "proj", "fc", "proj2")
GAMA_TYPES = (L.Q4, L.T_SIGN, L.BOOL1)   # the PackedQ group storages kf_gama_backward serves


def _align256(ptr):
    """a scratch the ABI wants 256-byte aligned is allocated 256 bytes longer and handed over from here"""
    return (ptr + 255) & ~255


class _TrainStep:
    """What GPT2Step and Qwen3Step share.  A subclass's constructor draws or takes the tensors in its trainer's order (_reg / _reg_matrix), allocates the activations
    (self.A) and buffers, creates its trainer (self.h) and hands everything over with _attach; the step itself is the entries kfh_<_family>_* of libkf_host.so."""
    _family = None         # "gpt2" / "qwen3t": the entries are kfh_<_family>_<name>
    _acts_entry = None     # the entry that takes one layer's kept activations, and the keys of a self.A dict in the order it takes them
    _act_keys = ()
    _layer_prefix = None   # what the name of a layer's tensor starts with ("h3.fc.w", "l3.gate.w")
    _layer_noun = None     # what set_optimizer's refusal calls a layer matrix
    _reason_codes = None   # the return codes whose reason is in kfh_<_family>_last_error; None: every code
    _targets = ("weights", "gama")   # the train_target values the family offers
    optimizer = "adamw"
    _clip = None           # (gclip, mode) of set_grad_clip, None: off
    _distill = None        # (teacher, "trainer" | "tensor") of set_distill, None: off
    _kd = None             # the KL rows kf_distill_classifier writes, fp32 [B * T]
    _n_sections = 1        # EOE layer sections (GPT2Step's layers_in_branch)

    def _begin(self, ctx, train_target, seed):
        """checks train_target before anything touches ctx; returns the device generator of the initial draws"""
        if train_target not in self._targets:
            raise ValueError("train_target %r: one of %s" % (train_target, ", ".join(repr(t_) for t_ in self._targets)))
        self.train_target, self.ctx = train_target, ctx
        self.params = []   # every trained tensor: dict(name, p (bf16 master), g (bf16 gradient), m, v (bf16 moments), wd (bool), blob (DevWeight or None), type)
        g = torch.Generator(device=ctx.device)
        g.manual_seed(seed)
        return g

    def _entry(self, name):
        return getattr(self.ctx.host, "kfh_%s_%s" % (self._family, name))

    def _call(self, name, *args, check=L.check):
        """kfh_<family>_<name>(self.h, ...), its return code through check"""
        check(self._entry(name)(self.h, *args), "kfh_%s_%s" % (self._family, name))

    def _check_host(self, rc, what):
        """a refusal of the trainer itself carries its reason in kfh_<family>_last_error; one of a kf_* entry underneath in kf_last_error"""
        if rc != 0:
            own = self._reason_codes is None or rc in self._reason_codes
            why = self._entry("last_error")().decode() if own else ""
            raise L.KFError("%s failed: code %d: %s" % (what, rc, why or self.ctx.hip.kf_last_error().decode()))

    def _check_arena(self):
        """train_target="gama" changes the (zero, step) a resident dequantised copy was made from: refused while the context holds a dequant arena"""
        if self.train_target == "gama" and self.ctx.hip.kf_dequant_arena_bytes(self.ctx.h):
            raise L.KFError("train_target='gama' on a context with a dequant arena (kf_set_dequant_arena): the resident bf16 copies of the trained matrices would go stale "
                            "with every update -- switch the arena off (kf_set_dequant_arena(ctx, NULL, 0)) for training")

    # ---- the tensors, appended to self.params in the trainer's order
    def _reg(self, name, p, wd, type_=None):
        e = dict(name=name, p=p.contiguous(), g=torch.zeros_like(p), m=torch.zeros_like(p), v=torch.zeros_like(p), wd=wd, blob=None, type=type_)
        if type_ is not None:
            e["blob"] = self.ctx.quantize(e["p"], type_)
            if type_ == L.BF16:
                e["p"] = e["blob"].blob.view(torch.bfloat16).view(p.shape)   # a bf16 "blob" IS the master (the tied head): updated in place, nothing to re-quantise
        self.params.append(e)
        return e

    def _reg_gama(self, name, W, type_):
        blob = self.ctx.quantize(W.contiguous(), type_)   # the draw is dropped: the packed integers are the weight from here on
        p = blob.gama_slice()
        e = dict(name=name, p=p, g=torch.zeros_like(p), m=torch.zeros_like(p), v=torch.zeros_like(p), wd=False, blob=blob, type=type_, gama=True)
        self.params.append(e)
        return e

    def _reg_lora(self, name, W, type_, a, b):
        """one of a layer's weight matrices with an adapter: the blob is quantised once from W, which is then dropped; the trained tensor is the vector [a | b]"""
        blob = self.ctx.quantize(W.contiguous(), type_)
        p = torch.cat([a.reshape(-1), b.reshape(-1)]).contiguous()
        e = dict(name=name, p=p, g=torch.zeros_like(p), m=torch.zeros_like(p), v=torch.zeros_like(p), wd=True, blob=blob, type=type_, lora=True, rank=a.shape[0],
                 s=self.lora_s, ax=torch.zeros(self.N, a.shape[0], dtype=torch.bfloat16, device=self.ctx.device))
        self.params.append(e)
        return e

    def _reg_matrix(self, name, W, type_):
        """one of a layer's weight matrices: its (zero, step) pairs under train_target="gama" when its storage is a PackedQ group type, its weights (decayed) otherwise"""
        if self.train_target == "gama" and type_ in GAMA_TYPES:
            return self._reg_gama(name, W, type_)
        return self._reg(name, W, True, type_)

    def _alloc_linear_scratch(self, layer, shapes, dim):
        """kf_linear's scratch for one layer's matrices (the context's), kf_linear_backward's for the largest of the matrix shapes and the [Vp, dim] head"""
        for k in shapes:
            self.ctx.linear_scratch(layer[k]["blob"], self.N)
        nb = max(self.ctx.hip.kf_linear_backward_scratch_bytes(oc, ic, self.N) for oc, ic in list(shapes.values()) + [(self.Vp, dim)])
        self._sc_lin = torch.empty(nb + 256, dtype=torch.uint8, device=self.ctx.device)
        self._sp_lin = _align256(self._sc_lin.data_ptr())

    def _attach(self, bufs, scratch):
        """every tensor registered once with the trainer just created: self.params in order, the activations of every layer (self.A), then the buffer table: bufs (torch
        tensors, in the order kfh_<family>_set_buffers takes them), kf_linear_backward's scratch, the other scratch tensors"""
        hip, N = self.ctx.hip, self.N
        assert self._entry("n_params")(self.h) == len(self.params)
        gama = [e for e in self.params if e.get("gama")]
        if gama:
            self._check_arena()
            need = [hip.kf_gama_backward_scratch_bytes(e["blob"].ne0, e["blob"].ne1, N) for e in gama]
            if not all(need):
                bad = gama[need.index(0)]
                raise L.KFError("train_target='gama': kf_gama_backward does not take %s [%d, %d] at %d rows (in-features a multiple of 128, out-features and rows multiples of 64)"
                                % (bad["name"], bad["blob"].ne0, bad["blob"].ne1, N))
            self._sc_gama = torch.empty(max(need) + 256, dtype=torch.uint8, device=self.ctx.device)
            self._call("set_gama_scratch", _align256(self._sc_gama.data_ptr()), max(need))
        lora = [e for e in self.params if e.get("lora")]
        if lora:
            need = max(hip.kf_lora_backward_scratch_bytes(e["rank"], e["blob"].ne0, e["blob"].ne1, N) for e in lora)
            self._sc_lora = torch.empty(need + 256, dtype=torch.uint8, device=self.ctx.device)
            self._call("set_lora_scratch", _align256(self._sc_lora.data_ptr()), need, check=self._check_host)
        for i, e in enumerate(self.params):
            d = e["blob"].desc() if e["blob"] is not None else None
            if e.get("lora"):
                self._call("set_param_lora", i, e["p"].data_ptr(), e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), e["rank"], e["s"], e["ax"].data_ptr(), C.byref(d),
                           check=self._check_host)
                continue
            if e.get("gama"):
                self._call("set_param_gama", i, e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), C.byref(d), check=self._check_host)
                continue
            self._call("set_param", i, e["p"].data_ptr(), e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), e["p"].numel(), int(e["wd"]),
                       C.byref(d) if d is not None else None, int(e["type"] is not None and e["type"] != L.BF16))
        for l, a in enumerate(self.A):
            self._call(self._acts_entry, l, (C.c_void_p * len(self._act_keys))(*[a[k].data_ptr() for k in self._act_keys]))
        ptrs = [t_.data_ptr() for t_ in bufs] + [self._sp_lin] + [t_.data_ptr() for t_ in scratch]
        self._call("set_buffers", (C.c_void_p * len(ptrs))(*ptrs))

    def set_optimizer(self, method="adamw", lr_scale=50.0, mui=0.95, eps=1e-7, tp_decay=1):
        """"adamw" (the default: every tensor) or "muon" (OPT_Muon, the reference's default): a layer's weight matrices with ne0 >= ne1 and a bf16 master (GPT-2: qkv, proj,
        fc; Qwen3 at its shapes: q, k, v, gate, up) take SGD-momentum + five Newton-Schulz steps (kf_muon: lr x lr_scale, weight decay by tp_decay as Pipe.cpp:23-37, mG =
        the tensor's m buffer); the other matrices (proj2; o, down), the embeddings, the head, biases and norms keep kf_adamw -- and so does every gama-trained tensor
        (train_target="gama"): its parameter is a [2 nGroup] slice, never a matrix for kf_muon -- and every adapter (train_target="lora"): its parameter is the vector
        [a | b].  Owns the scratch, sized for the largest Muon tensor."""
        if method not in ("adamw", "muon"):
            raise ValueError("optimizer %r: 'adamw' or 'muon'" % (method,))
        sp, nb = None, 0
        if method == "muon":
            shapes = [tuple(e["p"].shape) for e in self.params if e["blob"] is not None and not e.get("gama") and not e.get("lora") and e["name"].startswith(self._layer_prefix)
                      and e["p"].dim() == 2 and e["p"].shape[0] >= e["p"].shape[1]]
            nb = max([self.ctx.hip.kf_muon_scratch_bytes(a, b) for a, b in shapes], default=256)   # no Muon tensor at all (every matrix gama-trained): a token scratch
            if nb == 0:
                raise L.KFError("muon: a %s matrix has a dimension that is no multiple of 64" % self._layer_noun)
            self._sc_muon = torch.empty(nb + 256, dtype=torch.uint8, device=self.ctx.device)
            sp = _align256(self._sc_muon.data_ptr())
        self._call("set_optimizer", int(method == "muon"), lr_scale, mui, eps, tp_decay, sp, nb)
        self.optimizer = method
        if self._clip is not None:
            self.set_grad_clip(*self._clip)   # the clip table masks the Muon tensors: written again for the new switch

    def set_grad_clip(self, gclip=1.0, mode="tensor"):
        """Gradient norms and clipping at the head of every update, on the device (kf_grad_norms: every tensor in one launch, a fixed summation order, no host read).
        mode "tensor": each AdamW tensor's gradient is scaled by gclip / |g_i| where |g_i| > gclip (adam.gclip, the reference's per-tensor rule, Optimizer.cu:756-774);
        "global": all by gclip / |g| of the whole gradient (Optimizer::gClip); "report": norms only, the update's bits are those of clipping off; None: off (the
        default: nothing is launched).  Gama tensors are AdamW tensors; Muon tensors are never scaled (the reference's Muon path reads the raw gradient) and still
        count in |g|.  Owns the scratch."""
        if mode not in L.CLIP_MODES:
            raise ValueError("grad clip mode %r: None, 'report', 'tensor' or 'global'" % (mode,))
        sc, sp, nb = None, None, 0
        if mode is not None:
            nb = int(self._entry("grad_clip_scratch_bytes")(self.h))
            sc = torch.empty(nb + 256, dtype=torch.uint8, device=self.ctx.device)
            sp = _align256(sc.data_ptr())
        self._call("set_grad_clip", L.CLIP_MODES[mode], gclip, sp, nb, check=self._check_host)
        # only now: a refusal changes nothing in the trainer, which then still reads the scratch it had
        self._sc_clip, self._clip = sc, (None if mode is None else (gclip, mode))

    def grad_norms(self):
        """|g_i| of every tensor at the last update, float32 numpy array in the order of self.params -- the one host read, made here and never inside update()"""
        import numpy as np
        out = np.empty(len(self.params) + 1, dtype=np.float32)
        self._call("grad_norms", out.ctypes.data_as(C.c_void_p), out.size, check=self._check_host)
        self._gnorm = float(out[-1])
        return out[:-1]

    def grad_norm(self):
        """|g| of the whole gradient at the last update (the reference's g_step), Muon tensors included"""
        self.grad_norms()
        return self._gnorm

    # ---- distillation: the objective of every forward becomes ce_weight CE + kd_weight temperature^2 KL(teacher || student) (kf_distill_classifier)
    @classmethod
    def check_distill(cls, student, teacher, kd_weight=0.5, ce_weight=0.5, temperature=1.0):
        """every argument error of set_distill as a ValueError, without a device.  student: the trainer (anything with ctx, B, T, N, V, Vp); teacher: another trainer of
        any family on the same Context with equal B, T, V, Vp, or a bf16 tensor [B * T, >= V] on the student's device whose rows are 16-byte aligned (row stride a
        multiple of 8, unit column stride).  Returns ("trainer" | "tensor", the teacher's row stride in elements)."""
        for name, w in (("kd_weight", kd_weight), ("ce_weight", ce_weight), ("temperature", temperature)):
            if isinstance(w, bool) or not isinstance(w, (int, float)) or w != w or abs(w) == float("inf"):
                raise ValueError("%s %r: a finite number" % (name, w))
        if kd_weight < 0 or ce_weight < 0 or (kd_weight == 0 and ce_weight == 0):
            raise ValueError("kd_weight %r, ce_weight %r: both >= 0 and not both zero" % (kd_weight, ce_weight))
        if temperature <= 0:
            raise ValueError("temperature %r: > 0" % (temperature,))
        if teacher is student:
            raise ValueError("set_distill: a trainer cannot be its own teacher (its logits buffer is where the gradient is written)")
        if getattr(student, "_n_sections", 1) > 1:
            raise ValueError("set_distill: a trainer with EOE layer sections (layers_in_branch) is not distilled: eval_loss shares the step's loss buffer")
        if isinstance(teacher, _TrainStep):
            if teacher.ctx is not student.ctx:
                raise ValueError("set_distill: the teacher lives on another Context: both must share one (one device, one stream)")
            for k in ("B", "T", "V", "Vp"):
                if getattr(teacher, k) != getattr(student, k):
                    raise ValueError("set_distill: the teacher's %s = %d, the student's %d" % (k, getattr(teacher, k), getattr(student, k)))
            return "trainer", teacher.Vp
        if not torch.is_tensor(teacher):
            raise ValueError("set_distill: teacher %r is neither a trainer nor a tensor (None switches distillation off)" % (type(teacher).__name__,))
        if teacher.dtype != torch.bfloat16 or teacher.dim() != 2:
            raise ValueError("set_distill: teacher logits must be a 2-D bf16 tensor (got %s, %d-D)" % (teacher.dtype, teacher.dim()))
        if teacher.shape[0] != student.N or teacher.shape[1] < student.V:
            raise ValueError("set_distill: teacher logits %s: [%d, >= %d] wanted" % (tuple(teacher.shape), student.N, student.V))
        if teacher.device != student.ctx.device:
            raise ValueError("set_distill: teacher logits on %s, the trainer on %s" % (teacher.device, student.ctx.device))
        ld = teacher.stride(0) if teacher.shape[0] > 1 else teacher.shape[1]
        if teacher.stride(1) != 1 or ld < teacher.shape[1] or ld % 8 or teacher.data_ptr() % 16:
            raise ValueError("set_distill: teacher rows must be 16-byte aligned: unit column stride, a row stride that is a multiple of 8 (got strides %s)" % (tuple(teacher.stride()),))
        return "tensor", ld

    def set_distill(self, teacher, kd_weight=0.5, ce_weight=0.5, temperature=1.0):
        """Distil from a teacher's logits: every forward / step from here on ends in kf_distill_classifier, losses = ce_weight CE + kd_weight temperature^2
        KL(softmax(teacher / temperature) || softmax(student / temperature)) per row, and the backward starts from that sum's gradient.  teacher: another trainer of
        either family on the same Context with equal B, T, V, Vp -- its forward_logits(ids) then runs first in every forward / step, on the same stream; it is never
        updated, and the gradient and moment buffers it carries are simply unused (an accepted cost: build the teacher with the cheapest storage that holds its weights)
        -- or a bf16 device tensor [B * T, ld >= V] that the caller refills before every forward.  None switches distillation off: the plain path, bit for bit.
        eval_loss is not offered under distillation, and a trainer with EOE layer sections is refused."""
        if teacher is None:
            self._call("set_distill", None, 0, 1.0, 0.0, 1.0, None, check=self._check_host)
            self._distill = self._kd = None
            return
        kind, ld = self.check_distill(self, teacher, kd_weight, ce_weight, temperature)
        rows = teacher.logits if kind == "trainer" else teacher
        kd = torch.zeros(self.N, dtype=torch.float32, device=self.ctx.device)
        self._call("set_distill", rows.data_ptr(), ld, ce_weight, kd_weight, temperature, kd.data_ptr(), check=self._check_host)
        # only now: a refusal changes nothing in the trainer
        self._distill, self._kd = (teacher, kind), kd

    def forward_logits(self, ids):
        """the forward through the head product only: raw bf16 logits in self.logits ([B * T, Vp]; the columns from V on are the padded vocabulary rows' products), no
        loss, no gradient.  A backward after it is refused: it needs a forward."""
        self._check_arena()
        self._call("forward_logits", ids.data_ptr(), check=self._check_host)

    def _teach(self, ids):
        """a trainer as teacher: its logits of this batch, on the same stream, before the student's forward reads them"""
        if self._distill is not None and self._distill[1] == "trainer":
            self._distill[0].forward_logits(ids)

    def kd_losses(self):
        """KL(teacher || student) at the temperature of set_distill, per row of the last forward: fp32 [B * T] device tensor (a copy)"""
        if self._distill is None:
            raise L.KFError("kd_losses: no teacher is set (set_distill)")
        return self._kd.clone()

    def kd_loss(self):
        """the mean of kd_losses() -- the one host read, made here and never inside forward / step"""
        return float(self.kd_losses().mean())

    def close(self):
        if getattr(self, "h", None):
            if self._clip is not None and getattr(self.ctx, "h", None):
                self._entry("set_grad_clip")(self.h, L.CLIP_OFF, 1.0, None, 0)   # the context forgets the scratch before it is freed
                self._clip = None
            self._entry("destroy")(self.h)
            self.h = None

    __del__ = close

    @property
    def t(self):
        """optimizer steps taken"""
        return int(self._entry("steps_taken")(self.h))

    # ---- the step: sequenced by the host library; Python passes two device pointers and the hyper-parameters
    def forward(self, ids, tgt):
        """ids, tgt: int32 [B * T] on the device.  Leaves the per-row losses in self.losses and the logit gradients (of the MEAN loss) in self.logits."""
        self._ids = ids   # kept alive: the backward reads them
        self._check_arena()
        self._teach(ids)
        self._call("forward", ids.data_ptr(), tgt.data_ptr())

    def backward(self):
        self._call("backward")

    def _after_update(self):
        """what a subclass does once the weights have changed"""

    def update(self, lr=3e-4, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=1234):
        """AdamW on every tensor (its own master, moments and gradient; seeded stochastic rounding: seed + 7919 t + the tensor's index, as one seed per launch in the
        reference), then the re-quantisation of every quantised matrix from its updated master.  kf_adamw zeroes the gradients it has consumed."""
        self._call("update", lr, beta1, beta2, eps, wd, seed & 0xFFFFFFFF)
        self._after_update()

    def step(self, ids, tgt, lr=3e-4, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=1234):
        """forward + loss, backward, update + re-quantisation: ONE call into the host library"""
        self._ids = ids
        self._check_arena()
        self._teach(ids)
        self._call("step", ids.data_ptr(), tgt.data_ptr(), lr, beta1, beta2, eps, wd, seed & 0xFFFFFFFF)
        self._after_update()

    def n_params(self):
        return sum(e["p"].numel() for e in self.params)


class GPT2Step(_TrainStep):
    _family, _acts_entry, _layer_prefix, _layer_noun = "gpt2", "set_block_acts", "h", "hidden"
    _act_keys = ("x", "h1", "m1", "r1", "qkv", "att", "x2", "h2", "m2", "r2", "f", "g")
    _reason_codes = (-20, -1000)   # kfh_gpt2_last_error is cleared by the EOE entries only: for any other code it could hold a stale reason

    def __init__(self, ctx, C_, H, NL, V, Vp, B, T, types=None, seed=0, w_std=0.02, masters=None, train_target="weights", layers_in_branch=None):
        """masters: optional dict of host-provided bf16 torch tensors (tests hand the same numbers to the reference): 'wte' [Vp, C], 'wpe' [T, C], 'lnf' (w, b), 'blocks':
        list of dicts {mat: (W [out, in], b [out])} + 'ln' (w1, b1, w2, b2).  Otherwise N(0, w_std) draws on the device.
        train_target: "weights" (the default: bf16 masters, re-quantised after every update) or "gama": every block matrix whose storage is a PackedQ group type (GAMA_TYPES)
        is quantised once from its initial draw, which is then dropped; its entry of self.params has p = the blob's [ZERO][STEP] slice and g, m, v of 2 nGroup elements, no
        weight decay.  f8e5m2 / bf16 matrices, biases, norms and embeddings train as under "weights".  Refused with a reason: a matrix kf_gama_backward does not take
        (in-features no multiple of 128), and a context that holds a dequant arena (kf_set_dequant_arena: its resident copies would go stale with every update).
        layers_in_branch: None, 0 or NL: one branch, the whole depth (the default); otherwise a divisor of NL: NL / layers_in_branch branches, branch 0 active."""
        g = self._begin(ctx, train_target, seed)
        self.C, self.H, self.NL, self.V, self.Vp, self.B, self.T = C_, H, NL, V, Vp, B, T
        self.hd, self.N = C_ // H, B * T
        self.types = dict(qkv=L.F8E5M2, proj=L.F8E5M2, fc=L.Q4, proj2=L.Q4) if types is None else dict(types)
        dev, bf = ctx.device, torch.bfloat16
        z = lambda *s, dt=bf: torch.zeros(*s, device=dev, dtype=dt)
        rnd = lambda *s, std=w_std: (torch.randn(*s, device=dev, generator=g) * std).to(bf)
        shapes = dict(qkv=(3 * C_, C_), proj=(C_, C_), fc=(4 * C_, C_), proj2=(C_, 4 * C_))
        self.blocks = []
        for l in range(NL):
            mb = masters["blocks"][l] if masters else None
            blk = {}
            for k in MATS:
                W = mb[k][0].to(dev) if mb else rnd(*shapes[k])
                b = mb[k][1].to(dev) if mb else z(shapes[k][0])
                blk[k] = self._reg_matrix("h%d.%s.w" % (l, k), W, self.types[k])
                blk[k + "_b"] = self._reg("h%d.%s.b" % (l, k), b, False)
            ln = [t.to(dev) for t in mb["ln"]] if mb else [torch.ones(C_, device=dev, dtype=bf), z(C_), torch.ones(C_, device=dev, dtype=bf), z(C_)]
            for i, nm in enumerate(("ln1.w", "ln1.b", "ln2.w", "ln2.b")):
                blk[nm] = self._reg("h%d.%s" % (l, nm), ln[i], False)
            self.blocks.append(blk)
        wte = masters["wte"].to(dev) if masters else torch.cat([rnd(V, C_), z(Vp - V, C_)])
        self.wte = self._reg("wte", wte, True, L.BF16)
        self.wpe = self._reg("wpe", masters["wpe"].to(dev) if masters else rnd(T, C_, std=w_std / 2), False)
        lnf = [t.to(dev) for t in masters["lnf"]] if masters else [torch.ones(C_, device=dev, dtype=bf), z(C_)]
        self.lnf_w, self.lnf_b = self._reg("lnf.w", lnf[0], False), self._reg("lnf.b", lnf[1], False)
        # activations of one step, all kept
        N = self.N
        self.A = [dict(x=z(N, C_), h1=z(N, C_), m1=z(N, dt=torch.float32), r1=z(N, dt=torch.float32), qkv=z(N, 3 * C_), att=z(N, C_), x2=z(N, C_), h2=z(N, C_),
                       m2=z(N, dt=torch.float32), r2=z(N, dt=torch.float32), f=z(N, 4 * C_), g=z(N, 4 * C_)) for _ in range(NL)]
        self.xf, self.hf, self.mf, self.rf = z(N, C_), z(N, C_), z(N, dt=torch.float32), z(N, dt=torch.float32)
        self.qc, self.logits, self.losses = z(N, C_), z(N, Vp), z(N, dt=torch.float32)
        self.dx, self.dh, self.dqkv, self.datt, self.d4 = z(N, C_), z(N, C_), z(N, 3 * C_), z(N, C_), z(N, 4 * C_)
        hip = ctx.hip
        self._alloc_linear_scratch(self.blocks[0], shapes, C_)
        self._sc_ln = torch.empty(hip.kf_norm_backward_scratch_bytes(N, C_, 1) // 8 + 1, dtype=torch.float64, device=dev)
        self._sc_at = torch.empty(hip.kf_attn_backward_scratch_bytes(T, H, B) // 4 + 1, dtype=torch.float32, device=dev)

        # the step's sequencer: koifish::GPT2Trainer of libkf_host.so (koifish_amd/host/kf_train.cpp) over the buffers above -- every tensor registered once
        self.h = ctx.host.kfh_gpt2_create(ctx.h, C_, H, NL, V, Vp, B, T)
        if not self.h:
            raise RuntimeError("kfh_gpt2_create refused the shape")
        self._attach((self.xf, self.hf, self.mf, self.rf, self.logits, self.losses, self.dx, self.dh, self.dqkv, self.datt, self.d4), (self._sc_ln, self._sc_at))
        if layers_in_branch:
            self._check_host(ctx.host.kfh_gpt2_set_branches(self.h, int(layers_in_branch)), "kfh_gpt2_set_branches")
            self._n_sections = NL // int(layers_in_branch)

    # ---- EOE: layer-section branches
    @property
    def n_branches(self):
        return int(self.ctx.host.kfh_gpt2_n_branches(self.h))

    @property
    def branch(self):
        """the active branch"""
        return int(self.ctx.host.kfh_gpt2_active_branch(self.h))

    def set_branch(self, b):
        """forward / backward / update / step from here on run embed -> the layers of branch b -> lnf -> tied head, and update the shared tensors and that section's only"""
        self._check_host(self.ctx.host.kfh_gpt2_set_active_branch(self.h, int(b)), "kfh_gpt2_set_active_branch")

    def evolve(self, head, algorithm="pso_ga", alpha=0.9, social=2.0, t_crossover=0.6, seed=0):
        """Fuyou::UpdateFollower over the swarm: every branch but `head` has its qkv / proj / fc / proj2 masters moved towards the head branch's (kf_evolve, seed + the
        follower tensor's index in self.params) and its blobs re-quantised; biases, norms, embeddings and the head branch are not touched.  Refused, with nothing
        changed, while any block matrix is gama-trained.  One branch: nothing to do."""
        if algorithm not in L.EVO_ALGORITHMS:
            raise ValueError("evolve algorithm %r: one of %s" % (algorithm, sorted(L.EVO_ALGORITHMS)))
        self._check_host(self.ctx.host.kfh_gpt2_evolve(self.h, int(head), L.EVO_ALGORITHMS[algorithm], alpha, social, t_crossover, seed & 0xFFFFFFFF), "kfh_gpt2_evolve")

    def eval_loss(self, ids, tgt, ensemble="aggregation", branch=None):
        """per-row losses fp32 [B * T] without a backward or an update: "aggregation": the mean over all branches (Fuyou_params::AGGREGATION); "branch": of the given branch
        (FUYOU_BEST / RANDOM_1: the choice is the caller's; None: the active one).  The active branch is the same afterwards; a backward needs a new forward."""
        if ensemble not in ("aggregation", "branch"):
            raise ValueError("ensemble %r: 'aggregation' or 'branch'" % (ensemble,))
        self._check_arena()
        out = torch.empty(self.N, dtype=torch.float32, device=self.ctx.device)
        b = self.branch if branch is None else int(branch)
        self._check_host(self.ctx.host.kfh_gpt2_eval(self.h, ids.data_ptr(), tgt.data_ptr(), L.ENSEMBLE_BRANCH if ensemble == "branch" else L.ENSEMBLE_AGGREGATION, b,
                                                     out.data_ptr()), "kfh_gpt2_eval")
        return out


Q3_MATS = ("q", "k", "v", "o", "gate", "up", "down")   # the slot order of Qwen3.set_weight
Q3_NORMS = ("n1", "n2", "qn", "kn")                    # the slot order of Qwen3.set_norm


class Qwen3Step(_TrainStep):
    """One WHOLE training step of the Qwen3 family, GPT2Step's counterpart: the model everything else in this package serves (decode engines, prefill, score, .kun), and
    the one the reference's own training goldens run (cases/test_lite.py, tutorial_qwen3.md: Qwen3-596M plain and 4-bit with "train_target": "gama").

      forward  kf_embed_batch, n_layer x [RMSNorm, q / k / v, per-head q/k RMSNorm + RoPE (kf_qknorm_rope_train), GQA causal attention, o_proj + residual, RMSNorm,
               gate / up / SwiGLU / down + residual], RMSNorm, head, fused classifier -- on the QUANTISED blobs
      backward the reverse; dq | dk | dv of the attention backward through ONE kf_qknorm_rope_backward; weight gradients into per-tensor buffers
      update   kf_adamw (or kf_muon under set_optimizer("muon"): q, k, v, gate, up at the Qwen3 shapes) on the bf16 masters, every blob re-quantised

    Python owns the torch buffers and registers them once with koifish::Qwen3Trainer (host/kf_train_qwen3.cpp); forward / backward / update are one C call each, step()
    is ONE call, and nothing in them is a torch op.  self.params holds the same dicts as GPT2Step.params, in the trainer's order: per layer q.w k.w v.w o.w gate.w up.w
    down.w n1 n2 qn kn, then wte, nf, and head when untied.

    as_model(max_seq) hands out a Qwen3 decoder built ON these blobs and norm tensors (no copy): score, perplexity, generate, save_kun and the engines then work on the
    trained weights; every update() calls weights_changed() on each model still alive.

    train_target="lora": every matrix named in lora_targets is quantised once and frozen, and a rank-r pair trains beside it (the LORA branch of SLP::Forw / SLP::Back):
    lora_state() hands out the trained pairs, merged_masters() the masters of an equivalent plain model, as_model(max_seq, adapters=True) a decoder on the packed base
    with the pairs attached (kf_lora_apply); plain as_model(max_seq) refuses.

    set_documents(doc_lens, doc_rows, loss_mask): supervised fine-tuning on packed documents -- any number of documents share the B * T rows, each at its own positions
    and attending to itself only, the loss over the rows that count (sft_loss()); the attention and the q/k-norm + RoPE, forward and backward, then run their _docs /
    _pos entries, everything else is row-wise and unchanged.

    Not offered on this trainer: EOE layer-section branches (GPT2Step's layers_in_branch)."""

    _targets = ("weights", "gama", "lora")
    _family, _acts_entry, _layer_prefix, _layer_noun = "qwen3t", "set_layer_acts", "l", "layer"
    _act_keys = ("x", "h1", "r1", "qraw", "kraw", "qkv", "rq", "rk", "att", "x2", "h2", "r2", "gate", "up", "act")

    @staticmethod
    def _mat_shapes(cfg):
        dim, H, KV, hd, ffn = (cfg[k] for k in ("dim", "n_head", "n_kv", "head_dim", "ffn"))
        return dict(q=(H * hd, dim), k=(KV * hd, dim), v=(KV * hd, dim), o=(dim, H * hd), gate=(ffn, dim), up=(ffn, dim), down=(dim, ffn))

    @classmethod
    def _check_lora_args(cls, cfg, B, T, lora_rank, lora_s, lora_targets, adapters):
        """every argument error of train_target="lora", before anything touches a context"""
        if lora_rank not in (16, 32, 64):
            raise ValueError("lora_rank %r: 16, 32 or 64" % (lora_rank,))
        if 2 * lora_rank >= cfg["dim"]:
            raise ValueError("lora_rank %d: 2 x rank must stay below dim %d" % (lora_rank, cfg["dim"]))   # the reference's assertion (SparseNeuron.cpp)
        if not (isinstance(lora_s, (int, float)) and lora_s == lora_s and abs(lora_s) != float("inf")):
            raise ValueError("lora_s %r: a finite number" % (lora_s,))
        targets = tuple(lora_targets)
        bad = [k for k in targets if k not in Q3_MATS]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError("lora_targets %r: distinct names out of %s" % (lora_targets, Q3_MATS))
        shapes, sb = cls._mat_shapes(cfg), L.load()[0].kf_lora_backward_scratch_bytes
        for k in targets:
            if not sb(lora_rank, shapes[k][0], shapes[k][1], B * T):
                raise ValueError("train_target='lora': kf_lora_backward does not take %s [%d, %d] at %d rows (out- and in-features multiples of 64 and >= 128, rows a "
                                 "multiple of 64)" % (k, shapes[k][0], shapes[k][1], B * T))
        for name, ab in (adapters or {}).items():
            l, _, k = name[1:].partition(".")
            if not (name[:1] == "l" and l.isdigit() and int(l) < cfg["n_layer"] and k.endswith(".w") and k[:-2] in targets):
                raise ValueError("adapters: %r is no adapted matrix (names are l<layer>.<target>.w)" % (name,))
            OC, IC = shapes[k[:-2]]
            if len(ab) != 2 or tuple(ab[0].shape) != (lora_rank, IC) or tuple(ab[1].shape) != (OC, lora_rank) or ab[0].dtype != torch.bfloat16 or ab[1].dtype != torch.bfloat16:
                raise ValueError("adapters[%r]: (a [%d, %d], b [%d, %d]) bf16" % (name, lora_rank, IC, OC, lora_rank))
        return targets

    def __init__(self, ctx, cfg, B, T, types=None, tied=True, seed=0, w_std=0.02, masters=None, train_target="weights", lora_rank=16, lora_s=1.0, lora_targets=Q3_MATS,
                 adapters=None):
        """cfg: the dict Qwen3 takes (dim, n_layer, n_head, n_kv, head_dim, ffn, vocab, theta, rms_eps).  types: storage per matrix name of Q3_MATS (default: 4-bit for
        all seven); the embedding / head are bf16.  The vocabulary is padded to a multiple of 64 rows (kf_linear_backward); the padded rows stay zero.
        masters: optional dict of host-provided bf16 torch tensors: 'wte' [V or Vp, dim], 'nf' [dim], 'head' [V or Vp, dim] (untied), 'layers': list of dicts
        {q .. down: W [out, in], n1, n2: [dim], qn, kn: [head_dim]}.  Otherwise N(0, w_std) draws on the device and unit norms.
        train_target: "weights" or "gama" (every layer matrix stored as a PackedQ group type trains its (zero, step) pairs in place, as GPT2Step); a context that holds a
        dequant arena is refused; or "lora": every matrix named in lora_targets is quantised once from its master, which is then dropped, and gets an adapter a [lora_rank,
        in] ~ N(0, w_std), b [out, lora_rank] = 0 (the reference's isBZero), or the pair adapters[name] = (a, b) of bf16 host tensors (name "l<layer>.<target>.w").  lora_s is
        the reference's sAB: it multiplies BOTH products of a direction, the adapter's effective weight is lora_s^2 b a.  [a | b] is one entry of self.params
        (e["lora"] = True, decayed like any 2-D tensor, AdamW under every optimiser switch); everything else -- the matrices not named, norms, embedding, head -- trains as
        under "weights".  Raised before anything touches ctx: a rank outside {16, 32, 64} or with 2 rank >= dim (the reference's assertion), an unknown target, a matrix
        or row count kf_lora_backward does not take, a badly shaped adapter.  A dequant arena is accepted: the base never changes."""
        self._lora_targets = self._check_lora_args(cfg, B, T, lora_rank, lora_s, lora_targets, adapters) if train_target == "lora" else ()
        self.lora_rank, self.lora_s = int(lora_rank), float(lora_s)
        g = self._begin(ctx, train_target, seed)
        self.tied, self.cfg, self.B, self.T, self.N = bool(tied), dict(cfg), B, T, B * T
        dim, NL, H, KV, hd, ffn, V = (cfg[k] for k in ("dim", "n_layer", "n_head", "n_kv", "head_dim", "ffn", "vocab"))
        self.V, self.Vp = V, (V + 63) // 64 * 64
        self.eps, self.theta = float(cfg.get("rms_eps", 1e-6)), float(cfg.get("theta", 1e6))
        Vp, N, Cq, Ck = self.Vp, self.N, H * hd, KV * hd
        W_ = Cq + 2 * Ck
        self.types = dict({k: L.Q4 for k in Q3_MATS}, **(types or {}))
        dev, bf, f32 = ctx.device, torch.bfloat16, torch.float32
        z = lambda *s, dt=bf: torch.zeros(*s, device=dev, dtype=dt)
        rnd = lambda *s: (torch.randn(*s, device=dev, generator=g) * w_std).to(bf)
        ones = lambda n: torch.ones(n, device=dev, dtype=bf)
        self.shapes = self._mat_shapes(cfg)
        self.layers, self._models = [], []
        self._check_arena()

        def vocab_rows(t_):
            t_ = t_.to(dev)
            return t_ if t_.shape[0] == Vp else torch.cat([t_, z(Vp - t_.shape[0], dim)])
        for l in range(NL):
            ml = masters["layers"][l] if masters else None
            ly = {}
            for k in Q3_MATS:
                Wm = ml[k].to(dev) if ml else rnd(*self.shapes[k])
                name = "l%d.%s.w" % (l, k)
                if k in self._lora_targets:
                    ab = adapters.get(name) if adapters else None
                    a_ = ab[0].to(dev) if ab else rnd(self.lora_rank, self.shapes[k][1])
                    b_ = ab[1].to(dev) if ab else z(self.shapes[k][0], self.lora_rank)
                    ly[k] = self._reg_lora(name, Wm, self.types[k], a_, b_)
                else:
                    ly[k] = self._reg_matrix(name, Wm, self.types[k])
            for k in Q3_NORMS:
                n_ = hd if k in ("qn", "kn") else dim
                ly[k] = self._reg("l%d.%s" % (l, k), ml[k].to(dev) if ml else ones(n_), False)
            self.layers.append(ly)
        self.wte = self._reg("wte", vocab_rows(masters["wte"]) if masters else torch.cat([rnd(V, dim), z(Vp - V, dim)]), True, L.BF16)
        self.nf = self._reg("nf", masters["nf"].to(dev) if masters else ones(dim), False)
        self.head = self.wte if self.tied else self._reg("head", vocab_rows(masters["head"]) if masters else torch.cat([rnd(V, dim), z(Vp - V, dim)]), True, L.BF16)
        # activations of one step, all kept
        self.A = [dict(x=z(N, dim), h1=z(N, dim), r1=z(N, dt=f32), qraw=z(N, Cq), kraw=z(N, Ck), qkv=z(N, W_), rq=z(N * H, dt=f32), rk=z(N * KV, dt=f32), att=z(N, Cq),
                       x2=z(N, dim), h2=z(N, dim), r2=z(N, dt=f32), gate=z(N, ffn), up=z(N, ffn), act=z(N, ffn)) for _ in range(NL)]
        self.xf, self.hf, self.rf, self.logits, self.losses = z(N, dim), z(N, dim), z(N, dt=f32), z(N, Vp), z(N, dt=f32)
        self.dx, self.dh, self.dqkv, self.datt, self.dact, self.dgate = z(N, dim), z(N, dim), z(N, W_), z(N, Cq), z(N, ffn), z(N, ffn)
        self.vtmp, self.dqr, self.dkr, self.dvd = z(N, Ck), z(N, Cq), z(N, Ck), z(N, Ck)
        self.table = ctx.rope_table(T, hd, self.theta)
        hip, host = ctx.hip, ctx.host
        self._alloc_linear_scratch(self.layers[0], self.shapes, dim)
        self._sc_ln = torch.empty(hip.kf_norm_backward_scratch_bytes(N, dim, 0) // 8 + 1, dtype=torch.float64, device=dev)
        self._sc_at = torch.empty(hip.kf_attn_backward_scratch_bytes(T, H, B) // 4 + 1, dtype=torch.float32, device=dev)
        nqk = hip.kf_qknorm_rope_backward_scratch_bytes(N, H, KV, hd)
        if not nqk:
            raise L.KFError("Qwen3Step: kf_qknorm_rope_backward does not take %d / %d heads of %d (head_dim 64 or 128, n_head a multiple of n_kv)" % (H, KV, hd))
        self._sc_qk = torch.empty(nqk // 8 + 1, dtype=torch.float64, device=dev)

        # the step's sequencer: koifish::Qwen3Trainer of libkf_host.so over the buffers above -- every tensor registered once
        self.h = host.kfh_qwen3t_create(ctx.h, dim, NL, H, KV, hd, ffn, V, Vp, B, T, self.eps, int(self.tied))
        if not self.h:
            raise L.KFError("kfh_qwen3t_create refused the shape: %s" % host.kfh_qwen3t_last_error().decode())
        bufs = (self.xf, self.hf, self.rf, self.logits, self.losses, self.dx, self.dh, self.dqkv, self.datt, self.dact, self.dgate, self.vtmp, self.dqr, self.dkr, self.dvd, self.table)
        self._attach(bufs, (self._sc_ln, self._sc_at, self._sc_qk))

    # ---- supervised fine-tuning on packed documents (the layout: include/kf_abi.h; the reference's P_SFT phase pads one sample per batch row instead)
    _docs = None   # the active layout: dict(lens, rows, n_valid, and the device tensors the trainer reads), None: B sequences of T rows

    @classmethod
    def check_documents(cls, cfg, B, T, doc_lens, doc_rows=None, loss_mask=None):
        """every argument error of set_documents as a ValueError, without a device.  doc_lens: the documents' lengths, each in 1 .. T; doc_rows: their first rows in
        the B * T rows of a step, ascending and not overlapping (None: back to back from row 0); loss_mask: bool [B * T], True = this row's target counts (None: every
        document row).  A gap row -- a row in no document -- never counts.  Returns dict(lens, rows: int32 [n_doc]; pos: int32 [N], a row's position in its document, 0 in
        a gap; mask: int32 [N], 0x10000 (F_IGNORE_LOSS) on every row that does not count; n_valid: the rows that count)."""
        import numpy as np
        N = B * T
        try:
            lens = [int(x) for x in doc_lens]
            rows = None if doc_rows is None else [int(x) for x in doc_rows]
            if any(a != b for a, b in zip(lens, doc_lens)) or (rows is not None and any(a != b for a, b in zip(rows, doc_rows))):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError("set_documents: doc_lens and doc_rows must be sequences of ints") from None
        if not lens:
            raise ValueError("set_documents: at least one document (None switches documents off)")
        if rows is None:
            rows = [sum(lens[:d]) for d in range(len(lens))]
        if len(rows) != len(lens):
            raise ValueError("set_documents: %d lengths but %d first rows" % (len(lens), len(rows)))
        at = 0
        for d, (r, n) in enumerate(zip(rows, lens)):
            if not 1 <= n <= T:
                raise ValueError("set_documents: document %d has %d rows: 1 .. %d (the rope table's length)" % (d, n, T))
            if r < at:
                raise ValueError("set_documents: document %d starts at row %d, before row %d where the one before it ends: ascending, no overlap" % (d, r, at))
            if r + n > N:
                raise ValueError("set_documents: document %d ends at row %d, past the step's %d rows" % (d, r + n, N))
            at = r + n
        lens_a, rows_a = np.asarray(lens, dtype=np.int32), np.asarray(rows, dtype=np.int32)
        H, KV, hd = cfg["n_head"], cfg["n_kv"], cfg["head_dim"]
        if not L.load()[0].kf_attn_docs_table_bytes(rows_a.ctypes.data_as(C.c_void_p), lens_a.ctypes.data_as(C.c_void_p), len(lens), N, T, H, KV, hd):
            raise ValueError("set_documents: the attention entries do not take %d / %d heads of %d (head_dim 64 or 128, n_head / n_kv in 1, 2, 4, 8)" % (H, KV, hd))
        pos, in_doc = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
        for r, n in zip(rows, lens):
            pos[r:r + n], in_doc[r:r + n] = np.arange(n, dtype=np.int32), True
        if loss_mask is None:
            counts = in_doc
        else:
            counts = np.asarray(loss_mask.cpu() if torch.is_tensor(loss_mask) else loss_mask)
            if counts.dtype != np.bool_ or counts.shape != (N,):
                raise ValueError("set_documents: loss_mask must be bool [%d] (got %s %s)" % (N, counts.dtype, tuple(counts.shape)))
            counts = counts & in_doc
        n_valid = int(counts.sum())
        if n_valid == 0:
            raise ValueError("set_documents: no row counts in the loss (the mask selects no document row): the mean over zero rows is undefined")
        return dict(lens=lens_a, rows=rows_a, pos=pos, mask=np.where(counts, 0, L.F_IGNORE_LOSS).astype(np.int32), n_valid=n_valid)

    def set_documents(self, doc_lens, doc_rows=None, loss_mask=None):
        """Train on packed documents from here on (kept until changed, like set_distill): document d owns rows [doc_rows[d], doc_rows[d] + doc_lens[d]) of the B * T rows
        of ids / tgt, a row stands at its position inside its document and attends causally to its own document only, and the loss is the mean over the rows of
        loss_mask (None: every document row; a gap row never counts) -- sft_loss().  Documents may start at any row and cross the B row boundaries; rows in no document
        cost their share of the GEMMs and nothing else (their ids must still be valid token ids).  Plans on the host (kf_attn_docs_plan), uploads once; forward /
        backward then run kf_attn_prefill_docs, kf_attn_backward_docs and the _pos forms of the q/k-norm + RoPE entries.  Everything else -- train_target, Muon,
        clipping, as_model -- is row-wise and works unchanged; set_distill is refused while documents are set, and the other way round.  set_documents(None): back to B
        sequences of T rows, the plain step bit for bit."""
        import numpy as np
        if doc_lens is None:
            self._call("set_documents", None, None, None, None, 0, check=self._check_host)
            self._docs = None
            return
        d = self.check_documents(self.cfg, self.B, self.T, doc_lens, doc_rows, loss_mask)
        hip, cfg = self.ctx.hip, self.cfg
        geom = (len(d["lens"]), self.N, self.T, cfg["n_head"], cfg["n_kv"], cfg["head_dim"])
        lp, rp = d["lens"].ctypes.data_as(C.c_void_p), d["rows"].ctypes.data_as(C.c_void_p)
        table = np.zeros(hip.kf_attn_docs_table_bytes(rp, lp, *geom), dtype=np.uint8)
        L.check(hip.kf_attn_docs_plan(rp, lp, *geom, table.ctypes.data_as(C.c_void_p), table.size), "kf_attn_docs_plan")
        dev = {k: torch.from_numpy(v).to(self.ctx.device) for k, v in (("table", table), ("pos", d["pos"]), ("mask", d["mask"]))}
        self._call("set_documents", table.ctypes.data_as(C.c_void_p), dev["table"].data_ptr(), dev["pos"].data_ptr(), dev["mask"].data_ptr(), d["n_valid"], check=self._check_host)
        # only now: a refusal changes nothing in the trainer, which then still reads the tensors it had
        self._docs = dict(d, dev=dev)

    def documents(self):
        """the active layout: dict(lens, rows: int32 numpy [n_doc]; n_valid), or None"""
        return None if self._docs is None else {k: self._docs[k] for k in ("lens", "rows", "n_valid")}

    def sft_loss(self):
        """the mean loss of the last forward over the rows that count: losses.sum() / n_valid -- the one host read, made here and never inside forward / step"""
        if self._docs is None:
            raise L.KFError("sft_loss: no documents are set (set_documents)")
        return float(self.losses.sum()) / self._docs["n_valid"]

    def as_model(self, max_seq, adapters=False):
        """a Qwen3 decoder on the trainer's OWN blobs and norm tensors (set_weight / set_norm / tie_head with device pointers: no copy), vocabulary = the unpadded one.
        The step keeps a weak reference and calls weights_changed() on it after every update; the model must not outlive this object's buffers.
        adapters=True (train_target="lora" only): lora_state()'s VIEWS are attached (Qwen3.set_adapters, no copy), so the model scores, generates and measures perplexity
        with what has been trained so far, and a later step() is seen without attaching again.  Without it a "lora" trainer refuses: the frozen base alone is not the model."""
        import weakref
        from .runtime import DevWeight, Qwen3
        if adapters and self.train_target != "lora":
            raise L.KFError("as_model(adapters=True) under train_target=%r: only a 'lora' trainer has adapters" % (self.train_target,))
        if self.train_target == "lora" and not adapters:
            raise L.KFError("as_model under train_target='lora': the decode path does not apply adapters unless asked -- as_model(max_seq, adapters=True), or build a "
                            "plain model from merged_masters()")
        dim, V = self.cfg["dim"], self.V
        m = Qwen3(dict(self.cfg, max_seq=int(max_seq), rms_eps=self.eps, qk_eps=self.eps, theta=self.theta, tied=self.tied), device=self.ctx.device.index or 0)
        rows = lambda e: DevWeight(L.BF16, V, dim, e["blob"].blob[:V * dim * 2])   # the first V rows of the [Vp, dim] bf16 blob, the same memory
        m.set_weight(-1, 0, rows(self.wte))
        if self.tied:
            m.tie_head()
        else:
            m.set_weight(-1, 1, rows(self.head))
        m.set_norm(-1, 0, self.nf["p"])
        for li, ly in enumerate(self.layers):
            for si, k in enumerate(Q3_MATS):
                m.set_weight(li, si, ly[k]["blob"])
            for si, k in enumerate(Q3_NORMS):
                m.set_norm(li, si, ly[k]["p"])
        if adapters:
            m.set_adapters(self.lora_state(), self.lora_s)
        m._trainer = self   # the buffers live as long as the model does
        self._models.append(weakref.ref(m))
        return m

    def _ab(self, e):
        r, OC, IC = e["rank"], e["blob"].ne0, e["blob"].ne1
        return e["p"][:r * IC].view(r, IC), e["p"][r * IC:].view(OC, r)

    def lora_state(self):
        """{name: (a [r, in], b [out, r])} of every adapted matrix: views of the trained vectors (what adapters= takes back)"""
        return {e["name"]: self._ab(e) for e in self.params if e.get("lora")}

    def merged_masters(self):
        """a dict in the masters= layout (host bf16 tensors): every adapted matrix as bf16(dequant(W) + lora_s^2 b a), everything else as it stands -- what a plain bf16 or
        re-quantised model of the trained weights is built from.  Export, not the step: plain torch."""
        def mat(e):
            if not e.get("lora"):
                return e["p"].detach().cpu().clone()
            a, b = self._ab(e)
            W = self.ctx.dequant(e["blob"]).float() + (e["s"] * e["s"]) * (b.float() @ a.float())
            return W.to(torch.bfloat16).cpu()
        out = dict(wte=self.wte["p"].detach().cpu().clone(), nf=self.nf["p"].detach().cpu().clone(),
                   layers=[{k: mat(ly[k]) for k in Q3_MATS + Q3_NORMS} for ly in self.layers])
        if not self.tied:
            out["head"] = self.head["p"].detach().cpu().clone()
        return out

    def _weights_changed(self):
        live = []
        for r in self._models:
            m = r()
            if m is not None and getattr(m, "h", None):
                m.weights_changed()
                live.append(r)
        self._models = live

    def _after_update(self):
        """update() and step(): weights_changed() on every model handed out by as_model"""
        self._weights_changed()
