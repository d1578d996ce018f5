"""Every block of device memory the host layer takes it gives back (koifish_amd/host/kf_devbuf.hpp, DESIGN.md "Who owns device memory").

kfdbg_live_allocations() counts the blocks handed out by kf_malloc / kf_tp_alloc and not yet returned to kf_free.  One cycle builds the synthetic `tiny` model (dim 256,
2 layers, 4 / 2 heads of 64, ffn 512, vocab 512; 4-bit layers, bf16 head), walks every path of the host that allocates -- decode on captured graphs and on the engine,
samplers, token batches, scoring, the verify pass, the int8 KV cache, int8 activations, a hot-row mask, weights_changed, the resident copies and the head screen (the long
variant: a 1040-token prefill reaches the 1024-row threshold), an XcdReplicas with one prefill, a batch prefill that grows the buffers, steps -- and closes the replicas,
the model and its context.  The count then equals what it was before anything was built; three cycles in one process.  A second identical call of a path that allocates
on first use must not move the count.  The out-of-memory paths are tests/test_devbuf_cpu.py's."""
import ctypes as C

import numpy as np
import pytest

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import XcdReplicas

pytestmark = pytest.mark.gpu


def _live():
    hip, _ = L.load()
    hip.kfdbg_live_allocations.restype = C.c_longlong
    hip.kfdbg_live_allocations.argtypes = []
    return int(hip.kfdbg_live_allocations())


def _cycle(max_seq):
    cfg = dict(synth.CONFIGS["tiny"], max_seq=max_seq)
    m = synth.build_from_raw(cfg, synth.raw_weights_numpy(cfg, 11, w_std=0.1), L.Q4, L.BF16)   # 1
    ctx = m._ctx
    m.set_canonical(True)
    m.forward(3, 0), m.forward(5, 1)                                                            # 2
    m.generate(prompt_ids(cfg, 6, seed=1), 70)          # captured graphs (two position buckets) or the engine's one-launch steps
    m.set_sampler(temperature=0.7, top_k=20)                                                    # 3
    m.generate(prompt_ids(cfg, 6, seed=2), 12)
    m.set_sampler(temperature=0.0)
    m.prefill(prompt_ids(cfg, 33, seed=3))                                                      # 4
    after_first = _live()
    m.prefill(prompt_ids(cfg, 33, seed=3))
    assert _live() == after_first, "a second prefill allocated"
    m.score(prompt_ids(cfg, 34, seed=4))                                                        # 5
    assert len(m.verify([1, 2, 3, 4], 0)) == 4
    for switch in (m.set_kv_int8, m.set_act_int8_q4):                                           # 6, 7
        switch(True)
        m.prefill(prompt_ids(cfg, 33, seed=5))
        m.run_steps(33, 1)
        switch(False)
    hot = np.ones(cfg["ffn"], dtype=np.int32)                                                   # 8
    hot[::2] = 0
    m.set_hot(0, hot)
    m.run_steps(34, 1)
    m.set_hot(0, None)
    m.weights_changed()                                                                         # 9
    m.run_steps(35, 1)
    if max_seq >= 1056:                                                                         # 10
        m.set_prefill_resident(True)
        m.prefill(prompt_ids(cfg, 1040, seed=6))
        assert m.resident_bytes() > 0, "the 1040-token prefill did not reach the resident copies"
        m.run_steps(1040, 16)
        m.set_prefill_resident(False)
    m.sync()
    m.engine_check()
    xr = XcdReplicas(m, 2)                                                                      # 11
    xr.prefill(0, prompt_ids(cfg, 20, seed=7))                                                  # 12
    T = max_seq // 2 + 12                               # two prompts of T tokens: 2 T rows > the max_seq rows the first prefill sized the token-batch buffers to
    prompts = [prompt_ids(cfg, T, seed=8), prompt_ids(cfg, T - 5, seed=9)]
    before_batch = _live()
    xr.prefill_batch((0, 1), prompts)                                                           # 13
    grown = _live()
    assert grown > before_batch, "the batch prefill did not take the growth path"
    xr.prefill_batch((0, 1), prompts)
    assert _live() == grown, "a second identical batch prefill allocated"
    xr.run_steps(4)                                                                             # 14
    m.sync()
    xr.check()
    xr.close()                                                                                  # 15
    m.close()
    ctx.close()


@pytest.mark.parametrize("max_seq", [96, 1056])
def test_the_host_returns_every_block_it_took(max_seq):
    start = _live()
    for cycle in range(3):
        _cycle(max_seq)
        assert _live() == start, "cycle %d left %d blocks behind" % (cycle, _live() - start)
