"""The 4-bit twin of a 3- or 2-bit row weight (helper of tests/test_rowq_cpu.py, test_gpu_rowq*.py): the same ids stored as nibbles and a 16-entry table per row whose
first 8 / 4 entries are the row's own.  With kf_set_row_unpack the library multiplies a 3- / 2-bit row form in exactly the order of this twin (include/kf_abi.h), so
every entry must give identical bits on the weight and on its twin, in both summation orders -- and in the canonical order O.linear(twin, x) is the expected pattern."""
import numpy as np

from oracle import oracle as O

FILL = 0x7F00   # the twin's unused entries (ids the stream never holds): a huge finite value, so a lookup that strays shows


def ids_of(ow):
    """[ne0, ne1] ids of a 3- / 2-bit O.LutWeight: the stream read most significant bit first (BIT_SET_k order)"""
    d = ow.data.astype(np.uint32)
    if ow.bits == 3:
        v = (d[0::3] << 16) | (d[1::3] << 8) | d[2::3]                       # 8 ids per 3 bytes
        ids = np.stack([(v >> (21 - 3 * i)) & 7 for i in range(8)], axis=1)
    else:
        assert ow.bits == 2
        ids = np.stack([(d >> (6 - 2 * i)) & 3 for i in range(4)], axis=1)  # 4 ids per byte
    return ids.reshape(ow.ne0, ow.ne1).astype(np.uint8)


def table_of(ow):
    """[ne0, 2^bits] bf16 bit patterns: the row's own entries; row RTN: O.dequant of ids 0 .. 3 under the row's (zero, step)"""
    if not ow.rtn:
        return ow.lut
    ids = np.tile(np.arange(8, dtype=np.uint8) & 3, (ow.ne0, 1))              # a probe weight of 8 columns holding ids 0 1 2 3 0 1 2 3 in every row
    data = np.packbits(((ids[..., None] >> np.array([1, 0])) & 1).astype(np.uint8).reshape(-1))
    return O.dequant(O.LutWeight(ow.ne0, 8, data, ow.lut, bits=2, rtn=True)).reshape(ow.ne0, 8)[:, :4]


def twin(ow):
    """the 4-bit twin as an O.LutWeight (bits 4)"""
    d = ow.data.astype(np.uint32)
    if ow.bits == 3:   # 3 stream bytes -> 4 nibble bytes, without the id matrix in between (the large shapes)
        v = (d[0::3] << 16) | (d[1::3] << 8) | d[2::3]
        nib = np.stack([(((v >> (21 - 6 * j)) & 7) << 4 | ((v >> (18 - 6 * j)) & 7)).astype(np.uint8) for j in range(4)], axis=1)
    else:              # 1 stream byte -> 2 nibble bytes
        nib = np.stack([(((d >> 6) & 3) << 4 | ((d >> 4) & 3)).astype(np.uint8), (((d >> 2) & 3) << 4 | (d & 3)).astype(np.uint8)], axis=1)
    own = table_of(ow)
    lut = np.full((ow.ne0, 16), FILL, dtype=np.uint16)
    lut[:, :own.shape[1]] = own
    return O.LutWeight(ow.ne0, ow.ne1, nib, lut, bits=4)


def blob(ow):
    """data || R_SCALE[ne0] C_SCALE[ne1] || the row tables: the device blob of any O.LutWeight (Context.upload_lut_blob)"""
    return np.concatenate([ow.data, np.full(ow.ne0 + ow.ne1, 0x3F80, np.uint16).view(np.uint8), np.ascontiguousarray(ow.lut).reshape(-1).view(np.uint8)])


class DevRowWeight:
    """a row weight in HBM whose row tables start 16-byte aligned whatever ne0: the stream, padding, then gama -- kf_weight takes the two pointers separately, so a
    height that is no multiple of 8 (9 x 3072) can still be multiplied from the stream; Context.upload_lut_blob's contiguous blob cannot place its tables there"""

    def __init__(self, ctx, ow):
        import torch
        self.ne0, self.ne1, self.bits, self.rtn = ow.ne0, ow.ne1, ow.bits, ow.rtn
        self.szData = ow.data.size
        self.pad = -(self.szData + 2 * (ow.ne0 + ow.ne1)) % 16
        b = blob(ow)
        host = np.concatenate([b[:self.szData], np.zeros(self.pad, np.uint8), b[self.szData:]])
        self.blob = torch.from_numpy(host.copy()).to(ctx.device)
        assert self.blob.data_ptr() % 16 == 0

    def desc(self):
        from koifish_amd import lib as L
        p = self.blob.data_ptr()
        return L.Weight(p, p + self.szData + self.pad, {4: L.Q4, 3: L.Q3, 2: L.Q2}[self.bits], self.ne0, self.ne1, 0, 0, 0, (1 << self.bits) - 1, 0, None, None,
                        L.QUANT_ROW_RTN if self.rtn else L.QUANT_ROW_LUT, 0)


def in_register(hip, dw):
    """kf::rowq_standin's answer for an uploaded weight: True when the switch sends it down the in-register routes (False: kf_linear's dequantise route would serve it,
    and a comparison would say nothing about the unpack)"""
    import ctypes as C
    from koifish_amd import lib as L
    hip.kfdbg_rowq_standin.argtypes = [C.POINTER(L.Weight), C.POINTER(C.c_int)]
    d, out = dw.desc(), (C.c_int * 8)()
    assert hip.kfdbg_rowq_standin(C.byref(d), out) == 0
    return out[0] == 0


def upload(ctx, ow):
    """(the weight on the device, its twin on the device, the twin as an oracle weight)"""
    tw = twin(ow)
    return DevRowWeight(ctx, ow), DevRowWeight(ctx, tw), tw


def random_weight(rng, kind, m, k, std=0.02):
    """kind "nf3": GeQuant::RT_NormalF at 3 bits of a normal matrix; "lut2" / "rtn2": random 2-bit ids with a random table / (zero, step) per row"""
    if kind == "nf3":
        return O.quantize_nf3(O.f32_to_bf16(rng.normal(0, std, size=(m, k)).astype(np.float32)), m, k)
    data = rng.integers(0, 256, size=m * k // 4, dtype=np.uint8)
    if kind == "lut2":
        return O.LutWeight(m, k, data, O.f32_to_bf16(rng.normal(0, std, size=(m, 4)).astype(np.float32)), bits=2)
    assert kind == "rtn2"
    zs = np.stack([rng.normal(-1.5 * std, 0.2 * std, size=m), rng.uniform(0.5 * std, 1.5 * std, size=m)], axis=1).astype(np.float32)
    return O.LutWeight(m, k, data, O.f32_to_bf16(zs), bits=2, rtn=True)


def random_nf3_ids(rng, m, k, std=0.02):
    """a 3-bit row weight of random ids and normal-float-shaped tables without running the quantiser (the large shapes)"""
    data = rng.integers(0, 256, size=m * k * 3 // 8, dtype=np.uint8)
    lut = O.f32_to_bf16((O.nf3_table()[None, :] * rng.uniform(2.0, 4.0, size=(m, 1)).astype(np.float32) * np.float32(std)))
    return O.LutWeight(m, k, data, lut, bits=3)
