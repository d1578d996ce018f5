"""The yardstick of the gama tests (tests/test_gama_cpu.py, tests/test_gpu_gama.py): the (zero, step) gradients of a group-quantised weight restated in numpy fp64.
With w = step (q - qBias) - zero per group of 128 consecutive columns of a row, and dW = deltaIn^T . inp:
    g_zero[g] = - sum_{c in g} dW[r, c]        g_step[g] = + sum_{c in g} dW[r, c] (q[r, c] - qBias)
Not a test module: no test_ functions."""
import numpy as np

GROUP = 128


def gama_grads(dIn, inp, qmb):
    """dIn [n, OC], inp [n, IC] (fp64), qmb = q - qBias [OC, IC] (integers as fp64) -> (g [2 nGroup]: zero gradients then step gradients, A [2 nGroup]: the sums of the
    absolute products, the scale of the fp32 accumulation error)"""
    OC, IC = qmb.shape
    dW = dIn.T @ inp
    aW = np.abs(dIn).T @ np.abs(inp)
    grp = lambda m: m.reshape(OC, IC // GROUP, GROUP).sum(-1).reshape(-1)
    return np.concatenate([-grp(dW), grp(dW * qmb)]), np.concatenate([grp(aW), grp(aW * np.abs(qmb))])


def bound(ref, A, n):
    """|got - ref| <= 2^-8 |ref| (the bf16 store, one ulp) + (n + 128) 2^-23 A (first-order fp32 accumulation over a chain of n products and the 128-way reduction,
    doubled for the MFMA's internal order)"""
    return 2.0 ** -8 * np.abs(ref) + (n + GROUP) * 2.0 ** -23 * A
