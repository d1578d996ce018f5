"""EOE without a GPU: the draw kf_evolve is defined by (tests/evo_restate.py) has the moments the definition promises -- these are conditions on the draw, derived from
"the mean of three uniform bytes" and "one uniform byte against a threshold", not measurements of the kernel --, the boundary cases of the three algorithms are what the
definition says, and the entries exist in both libraries."""
import ctypes as C

import numpy as np
import pytest

import evo_restate as R

N = 1 << 20


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(2024)
    mk = lambda: R.rne_bf16(rng.normal(0, 0.02, N).astype(np.float32))
    return mk(), mk()


@pytest.mark.parametrize("seed", [1, 2])
def test_moments_of_the_draw(seed):
    _, r, _ = R.draw(N, seed)
    assert r.dtype == np.float32 and r.min() >= 0.0 and r.max() <= 1.0
    m, s = float(r.astype(np.float64).mean()), float(r.astype(np.float64).std())
    print("seed %d: mean %.5f std %.5f" % (seed, m, s))
    assert abs(m - 0.5) <= 0.002
    assert abs(s - 0.1673) <= 0.003


@pytest.mark.parametrize("seed", [1, 2])
def test_crossover_fraction(seed, pair):
    x, g = pair
    assert R.threshold(0.6) == 154
    _, _, b3 = R.draw(N, seed)
    frac = float((b3 < 154).mean())
    print("seed %d: fraction taken from the head %.5f" % (seed, frac))
    assert abs(frac - 154.0 / 256.0) <= 0.005
    ga, pso = R.evolve(x, g, "pso_ga", seed=seed), R.evolve(x, g, "pso", seed=seed)
    taken = b3 < 154
    assert np.array_equal(ga[taken], g[taken]) and np.array_equal(ga[~taken], pso[~taken])


def test_seeds_are_independent():
    _, r1, _ = R.draw(N, 1)
    _, r2, _ = R.draw(N, 2)
    assert float((r1 != r2).mean()) > 0.99


def test_boundaries(pair):
    x, g = pair
    x0 = x.copy()
    pso = R.evolve(x, g, "pso", seed=5)
    assert np.array_equal(x, x0), "the restatement must not modify its argument"
    assert not np.array_equal(pso, x) and not np.array_equal(pso, g)
    assert np.array_equal(R.evolve(x, g, "pso_ga", t_cross=0.0, seed=5), pso)          # thr = 0: no element is crossed over
    assert R.threshold(1.0) == 256
    assert np.array_equal(R.evolve(x, g, "pso_ga", t_cross=1.0, seed=5), g)            # thr = 256: every element is the head's
    assert np.array_equal(R.evolve(x, g, "pso_ga", social=0.0, t_cross=0.0, seed=5), x)
    assert np.array_equal(R.evolve(x, g, "mix", alpha=1.0), x)
    mix = R.evolve(x, g, "mix", alpha=0.9)
    ref = 0.9 * R.f32(x).astype(np.float64) + 0.1 * R.f32(g).astype(np.float64)
    assert np.abs(R.f32(mix) - ref).max() <= np.abs(ref).max() * 2.0 ** -8             # one bf16 rounding of the exact mix
    # social = 1, r = 1 would land on the head: the PSO value lies between x and the head's side of it for social * r <= 1
    s3, r, _ = R.draw(N, 5)
    one = R.evolve(x, g, "pso", social=1.0, seed=5)
    lo, hi = np.minimum(R.f32(x), R.f32(g)), np.maximum(R.f32(x), R.f32(g))
    ulp = np.maximum(np.abs(lo), np.abs(hi)) * 2.0 ** -7
    assert ((R.f32(one) >= lo - ulp) & (R.f32(one) <= hi + ulp)).all()


def test_entries_are_exported():
    from koifish_amd import lib as L
    hip, host = L.load()
    for f in ("kf_evolve", "kf_loss_mean"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f)
    for f in ("kfh_gpt2_set_branches", "kfh_gpt2_n_branches", "kfh_gpt2_set_active_branch", "kfh_gpt2_active_branch", "kfh_gpt2_evolve", "kfh_gpt2_eval", "kfh_gpt2_last_error"):
        assert hasattr(host, f), f
    assert (L.EVO_PSO, L.EVO_MIX, L.EVO_PSO_GA) == (R.PSO, R.MIX, R.PSO_GA) == (1, 2, 4)   # Fuyou_params::ALGORITHM
    assert L.EVO_ALGORITHMS == R.ALGORITHMS
    assert hip.kf_evolve(None, None, None, 8, 8, 1, 0.9, 2.0, 0.6, 0) == -20                 # no context: refused, nothing dereferenced
    assert hip.kf_loss_mean(None, None, None, 8, 0, 1) == -20
