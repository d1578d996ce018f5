"""The ctypes mirror of kf::AttnProblem / kf::AttnPlan (csrc/kf_attn_plan.h) and the calls of kfdbg_attn_plan / kfdbg_kv8_plan, once, for every test of the attention plan."""
import ctypes as C

DECODE, PROMPT, BATCH, BACKWARD, DECODE_KV8, PROMPT_KV8 = range(6)         # AttnProblem::entry
SLICED, PER_TOKEN, TILE, PAIRED, BWD, SLICED_KV8, TILE_KV8 = range(7)      # AttnPlan::route
Q_AL, OUT_AL = 1, 2                                                        # AttnProblem::al


class Problem(C.Structure):   # kf::AttnProblem
    _fields_ = ([(f, C.c_int) for f in ("entry", "n_head", "n_kv", "hd", "pos", "n_tok", "n_seq", "canon", "al")]
                + [(f, C.c_longlong) for f in ("q_stride", "out_stride", "kv_stride")])


class Plan(C.Structure):      # kf::AttnPlan
    _fields_ = ([(f, C.c_int) for f in ("status", "route", "canon", "gq", "nw", "hd", "kh", "kt", "gq_split", "n_splits", "chunk", "cnt_stride")]
                + [("grid", C.c_int * 3), ("grid_kv", C.c_int * 3), ("threads", C.c_int), ("lds", C.c_int), ("scratch", C.c_longlong)])


def plan(hip, entry, n_head, n_kv, hd=128, pos=0, n_tok=1, n_seq=1, canon=0, al=Q_AL | OUT_AL, q_stride=None, out_stride=0, kv_stride=None):
    """kf::attn_plan's answer, refusals included; the rows dense unless a stride is given"""
    hip.kfdbg_attn_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]
    q_stride = n_head * hd if q_stride is None else q_stride
    kv_stride = n_kv * hd if kv_stride is None else kv_stride
    out = Plan()
    assert hip.kfdbg_attn_plan(C.byref(Problem(entry, n_head, n_kv, hd, pos, n_tok, n_seq, canon, al, q_stride, out_stride, kv_stride)), C.byref(out)) == 0
    return out


def kv8_plan(hip, n_head, n_kv, hd, pos, kv_stride=None):
    """the plan of kf_attn_block_kv8, as the entry asks for it (argtypes: koifish_amd/lib.py)"""
    out = Plan()
    assert hip.kfdbg_kv8_plan(n_head, n_kv, hd, pos, n_kv * hd if kv_stride is None else kv_stride, C.byref(out)) == 0
    return out
