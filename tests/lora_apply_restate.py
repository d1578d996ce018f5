"""The yardstick of the inference-side adapter tests (tests/test_lora_apply_cpu.py, tests/test_gpu_lora_apply.py): kf_lora_apply's VECTOR form (n == 1) restated in
numpy in the order include/kf_abi.h states, fp32 operation by fp32 operation, so that the device's bits can be predicted:

    ax_j   lane l of 64 adds the products of the 8-element chunks l, l + 64, ... of the contraction to one fp32 accumulator, chunks ascending, k ascending inside a
           chunk; the 64 lane sums meet in a butterfly p_l <- p_l + p_(l xor m), m = 32, 16, 8, 4, 2, 1;  ax_j = bf16(s p_0)
    y_m    one fp32 chain over j ascending of ax_j b[m, j], then bf16(y_m + s sum) -- the multiply by s and the addition each round to fp32

The product of two bf16 values has at most 16 significant bits and is exact in fp32, so the device's fma and the multiply-then-add written here give the same bits.
The tile form (n >= 2) is kf_lora_forward's arithmetic and has tests/lora_restate.py.  Not a test module: no test_ functions."""
import numpy as np

from oracle import oracle as O

f32 = np.float32


def _bf(v):
    """fp32 -> bf16 bits (nearest even)"""
    return O.f32_to_bf16(np.asarray(v, dtype=f32))


def vec_ax_bits(a_bits, x_bits, s):
    """a [r, IC], x [IC] as bf16 bits -> ax [r] as bf16 bits, in the stated order"""
    a, x = O.bf16_to_f32(a_bits).astype(f32), O.bf16_to_f32(x_bits).astype(f32)
    r, IC = a.shape
    nch = IC // 8
    lanes = np.zeros((r, 64), dtype=f32)
    for c in range(nch):          # chunk c belongs to lane c % 64; a lane meets its chunks in ascending order
        l = c % 64
        for k in range(8 * c, 8 * c + 8):
            lanes[:, l] = (lanes[:, l] + a[:, k] * x[k]).astype(f32)   # the product is exact in fp32: one rounding, the sum's
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, idx ^ m]).astype(f32)
    return _bf(f32(s) * lanes[:, 0])


def exact_group(r, IC, OCs, seed, s=1):
    """integer operands for one vector-form launch: len(OCs) adapters of tests/lora_restate.py::lora_exact_case (a distinct a, b and prior y each) that share the
    input row of the first.  -> (x [IC], [(a, b, y0 [OC], y [OC])]) as bf16 bits.  Asserted: every y is a bf16 value and the terms' magnitudes sum to < 2^23, so every
    partial sum in every order is an fp32 value"""
    from tests import exact_inputs as E
    from tests import lora_restate as R
    cases = [R.lora_exact_case(OC, IC, 64, r, s, seed=seed + 101 * i) for i, OC in enumerate(OCs)]
    x = E.f64(cases[0]["x"][0])
    out = []
    for c in cases:
        a, b, y0 = E.f64(c["a"]), E.f64(c["b"]), E.f64(c["y0"][0])
        ax = s * (a @ x)
        y = y0 + s * (b @ ax)
        assert s * (np.abs(a) @ np.abs(x)).max() < 2.0 ** 23 and (np.abs(y0) + s * (np.abs(b) @ np.abs(ax))).max() < 2.0 ** 23
        E.exact_bits(ax)
        out.append((c["a"], c["b"], c["y0"][0], E.exact_bits(y)))
    return cases[0]["x"][0], out


def vec_apply_bits(a_bits, b_bits, x_bits, y_bits, s):
    """one adapter on one row: a [r, IC], b [OC, r], x [IC], y [OC] as bf16 bits -> the new y [OC] as bf16 bits"""
    ax = O.bf16_to_f32(vec_ax_bits(a_bits, x_bits, s)).astype(f32)
    b, y = O.bf16_to_f32(b_bits).astype(f32), O.bf16_to_f32(y_bits).astype(f32)
    v = np.zeros(b.shape[0], dtype=f32)
    for j in range(b.shape[1]):
        v = (v + ax[j] * b[:, j]).astype(f32)
    return _bf((y + (f32(s) * v).astype(f32)).astype(f32))
