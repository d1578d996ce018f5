"""NOT a test module: the seeded inputs of the kf_distill_classifier tests and their restated results, computed once per case and shared between
tests/test_distill_cpu.py (restatement against float64) and tests/test_gpu_distill.py (kernel against restatement)."""
import functools

import numpy as np

from tests import distill_restate as R

# (rows, V, P): the fused classifier test's own set -- several vector rounds per thread with a ragged last vector; a multiple of 8 below 1024 vectors; a few
# vectors; just over 1024 vectors, ragged; one ragged vector; one vector more than 1024 threads; one element
SHAPES = [(6, 50257, 50264), (3, 1000, 1000), (4, 66, 72), (2, 9001, 9008), (3, 7, 8), (2, 8193, 8200), (1, 1, 8)]
WEIGHTS = [(0.5, 0.5, 2.0), (0.0, 1.0, 1.0), (1.0, 0.25, 0.5)]   # (ce_weight, kd_weight, temperature)
TEACHERS = ["indep", "near"]   # scale 3, independent of the student (KL of a few nats); the student + noise of scale 2^-4 (small KL: the cancelling case)
NAN_BITS = 0x7fc1
LOSS_FILL = 0.5


def dloss_of(rows):
    return 1.0 / rows


@functools.lru_cache(maxsize=None)
def inputs(rows, V, P, teacher):
    """logits uint16 [rows, P], teacher uint16 [rows, P + 8] (a row stride of its own), targets int32 [rows]; NaN bit patterns in the padding of both"""
    rng = np.random.default_rng(1000 * rows + V + (7 if teacher == "near" else 0))
    z = (rng.standard_normal((rows, V)) * 2.0).astype(np.float32)
    zb = R.f32_to_bf16(z)
    if teacher == "near":
        u = R.bf16_to_f32(zb) + (rng.standard_normal((rows, V)) * 2.0 ** -4).astype(np.float32)
    else:
        u = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    logits = np.full((rows, P), NAN_BITS, dtype=np.uint16)
    teach = np.full((rows, P + 8), NAN_BITS, dtype=np.uint16)
    logits[:, :V], teach[:, :V] = zb, R.f32_to_bf16(u)
    targets = rng.integers(0, V, size=rows).astype(np.int32)
    for a in (logits, teach, targets):
        a.setflags(write=False)
    return logits, teach, targets


@functools.lru_cache(maxsize=None)
def restated(rows, V, P, teacher, weights):
    """(losses, kd, logits) of the restatement, losses pre-filled with LOSS_FILL"""
    logits, teach, targets = inputs(rows, V, P, teacher)
    a, b, tau = weights
    out = R.distill_classifier(logits, teach, np.full(rows, LOSS_FILL, np.float32), targets, V, dloss_of(rows), a, b, tau)
    for o in out:
        o.setflags(write=False)
    return out
