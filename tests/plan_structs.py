"""The ctypes mirrors of the C++ structs that the plan tests hand to the kfdbg_*_plan entries, each written once (kf::A8* live in a8_plan_mirror.py, kf::Attn* in
attn_plan_mirror.py).  Paths are relative to koifish_amd/."""
import ctypes as C

from koifish_amd import lib as L


class GemmMat(C.Structure):   # kf::GemmMat (csrc/kf_kernels.h)
    _fields_ = [(f, C.c_int) for f in ("type", "quant", "awq", "M", "K", "lgroup", "gama", "al")]


class GemmProblem(C.Structure):   # kf::GemmProblem (csrc/kf_gemm_plan.h)
    _fields_ = [("entry", C.c_int), ("n_w", C.c_int), ("w", GemmMat * 3), ("n", C.c_int), ("x_al", C.c_int), ("y_al", C.c_int), ("rope_ok", C.c_int), ("arena", C.c_int),
                ("capturing", C.c_int), ("arena_hit", C.c_int), ("arena_free", C.c_longlong), ("scratch", C.c_longlong)]


class GemmKern(C.Structure):   # kf::GemmKern (csrc/kf_gemm_plan.h)
    _fields_ = [(f, C.c_int) for f in ("fam", "fmt", "gshift", "form", "akm", "bkm", "gx", "gy", "block", "lds", "sk", "P", "S", "kp", "R")]


class GemmPlan(C.Structure):   # kf::GemmPlan (csrc/kf_gemm_plan.h)
    _fields_ = [("route", C.c_int), ("status", C.c_int), ("deq", C.c_int), ("deq_form", C.c_int), ("deq_bytes", C.c_longlong), ("ws_bytes", C.c_longlong), ("k", GemmKern)]


class ScoreProblem(C.Structure):   # kf::ScoreProblem (csrc/kf_score_plan.h)
    _fields_ = [("w", GemmMat), ("n", C.c_int), ("x_al", C.c_int), ("force", C.c_int), ("form", C.c_int)]


class ScorePlan(C.Structure):   # kf::ScorePlan (csrc/kf_score_plan.h)
    _fields_ = [(f, C.c_int) for f in ("route", "status", "form", "n_vt", "n_rb", "gx", "block", "lds", "panel_rows")] + [("scratch", C.c_longlong)]


class GemvProblem(C.Structure):   # kf::GemvProblem (csrc/kf_gemv_plan.h)
    _fields_ = [("mode", C.c_int), ("n_w", C.c_int), ("w", GemmMat * 3)] + [(f, C.c_int) for f in ("sparse", "n_hot", "norm", "canon", "q4_perm", "q2_tab", "q1_tab", "xf2")]


class GemvPlan(C.Structure):   # kf::GemvPlan (csrc/kf_gemv_plan.h)
    _fields_ = ([(f, C.c_int) for f in ("status", "fmt", "G", "mode", "sparse", "onejob", "canon", "xf", "xf2", "K", "nBlk", "lpr_log2", "iters", "lgroup", "gshift", "njobs")]
                + [("M", C.c_int * 3), ("slot0", C.c_int * 3)] + [(f, C.c_int) for f in ("spw", "total_slots", "stream_ok", "grid", "lds")])


class GemvRowsProblem(C.Structure):   # kf::GemvRowsProblem (csrc/kf_gemv_rows_plan.h)
    _fields_ = [("one", GemvProblem), ("n_rows", C.c_int)]


class GemvRowsPlan(C.Structure):   # kf::GemvRowsPlan (csrc/kf_gemv_rows_plan.h)
    _fields_ = ([(f, C.c_int) for f in ("status", "shared", "fmt", "mode", "xf", "NR", "K", "nBlk", "lpr_log2", "iters", "lgroup", "gshift", "norm_regs", "njobs")]
                + [("M", C.c_int * 3), ("slot0", C.c_int * 3)] + [(f, C.c_int) for f in ("spw", "total_slots", "n_panels", "panel_rows", "grid", "lds")])


class EngineLayer(C.Structure):   # struct kf_engine_layer (../include/kf_abi.h)
    _fields_ = [("w", L.Weight * 7), ("norm_in", C.c_void_p), ("norm_post", C.c_void_p), ("q_norm", C.c_void_p), ("k_norm", C.c_void_p), ("kcache", C.c_void_p),
                ("vcache", C.c_void_p), ("hot_ffn", C.c_void_p)]


class EngineDesc(C.Structure):   # struct kf_engine_desc (../include/kf_abi.h)
    _fields_ = [(f, C.c_int32) for f in ("n_layer", "dim", "n_head", "n_kv", "head_dim", "ffn", "kv_stride", "max_seq")] + [
        ("rms_eps", C.c_float), ("qk_eps", C.c_float), ("rope_table", C.c_void_p), ("layers", C.POINTER(EngineLayer))]
