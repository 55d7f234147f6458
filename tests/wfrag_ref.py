"""numpy yardstick of the weight images (csrc/dsphere_wfrag.h), written from the layouts' description, not from the header.

A fragment is 64 lanes x 16 bytes; lane l has eight slots j.  (lane, slot) holds the weight at
    32x32x16 / 32x32x2:  inner 8 (l >> 5) + j of a 16-long slice,  column l & 31 of a 32-column block
    16x16x32:            inner 8 (l >> 4) + j of a 32-long slice,  column l & 15 of a 16-column block
and a value is stored in one of five forms:
    fp32 steps   float at index j * 64 + l
    fp32 halves  float at byte (j >> 2) * 1024 + l * 16 + (j & 3) * 4
    bf16x3       hi = rne(v) at 16-bit index l * 8 + j, lo = rne(v - hi) 1 KiB behind
    bf16x6       hi = trunc(v), mid = trunc(v - hi), lo = rne(v - hi - mid), 1 KiB apart (lo: the rule the header states)
    f16x3        hi = f16(v), lo = f16(v - hi), 1 KiB apart
bf16 conversions are integer operations on the float's bits; f16 is numpy's float16 (round to nearest even).
"""

import numpy as np

FP32_STEPS, BF16X3, BF16X6, F16X3, FP32_HALVES = 0, 1, 2, 3, 4  # the first four: the precision codes of include/dsphere.h
FORMS = {"fp32_steps": FP32_STEPS, "fp32_halves": FP32_HALVES, "bf16x3": BF16X3, "bf16x6": BF16X6, "f16x3": F16X3}
FRAG = 1024


def group_bytes(form):
    return 3 * FRAG if form == BF16X6 else 2 * FRAG


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_trunc(x):
    """bits of the bf16 that keeps the upper 16 bits of the float"""
    return (f32_bits(x) >> 16).astype(np.uint16)


def bf16_rne(x):
    """bits of the bf16 nearest to the float, ties to the even one (finite inputs)"""
    u = f32_bits(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_bf16x3(v):
    v = np.asarray(v, dtype=np.float32)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - bf16_value(hi))


def split_bf16x6(v, third="rne"):
    v = np.asarray(v, dtype=np.float32)
    hi = bf16_trunc(v)
    r = v - bf16_value(hi)
    mid = bf16_trunc(r)
    q = r - bf16_value(mid)
    return hi, mid, (bf16_rne(q) if third == "rne" else bf16_trunc(q))


def split_f16x3(v):
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def gather(w, geometry, c, nb, Fin, Fout, K, k, pack, scale):
    """(64, 8) float32: the value of every (lane, slot) of slice c, column block nb; w is [rows, ld], row f K + k"""
    l = np.arange(64)[:, None]
    j = np.arange(8)[None, :]
    if geometry == 32:
        ch, col = 16 * c + 8 * (l >> 5) + j, 32 * nb + (l & 31) + 0 * j
    else:
        ch, col = 32 * c + 8 * (l >> 4) + j, 16 * nb + (l & 15) + 0 * j
    if pack:  # map q: inner indices [16 / pack * q, ..) against columns [64 / pack * q, ..), the layer's matrix in every diagonal block
        ci, cm = 16 // pack, 64 // pack
        live = ch // ci == col // cm
        ch, col = ch % ci, col % cm
        scale = 1.0
    else:
        live = np.ones(ch.shape, dtype=bool)
    live = live & (ch < Fin) & (col < Fout)
    out = np.zeros((64, 8), dtype=np.float32)  # padding: +0
    out[live] = np.float32(scale) * w[(ch * K + k)[live], col[live]]
    return out


def put(v, form):
    """bytes of one fragment group from its (64, 8) values"""
    l = np.arange(64)[:, None] + np.zeros((1, 8), dtype=np.int64)
    j = np.arange(8)[None, :] + np.zeros((64, 1), dtype=np.int64)
    img = np.zeros(group_bytes(form), dtype=np.uint8)
    if form == FP32_STEPS:
        img.view(np.float32)[j * 64 + l] = v
    elif form == FP32_HALVES:
        img.view(np.float32)[((j >> 2) * 1024 + l * 16 + (j & 3) * 4) // 4] = v
    elif form == BF16X3:
        hi, lo = split_bf16x3(v)
        img.view(np.uint16)[l * 8 + j] = hi
        img.view(np.uint16)[FRAG // 2 + l * 8 + j] = lo
    elif form == BF16X6:
        for t, part in enumerate(split_bf16x6(v)):
            img.view(np.uint16)[t * (FRAG // 2) + l * 8 + j] = part
    elif form == F16X3:
        hi, lo = split_f16x3(v)
        img.view(np.float16)[l * 8 + j] = hi
        img.view(np.float16)[FRAG // 2 + l * 8 + j] = lo
    else:
        raise ValueError(form)
    return img


def image(w, geometry, form, Fin, Fout, K, k, pack, slices, blocks, scale=1.0):
    return np.concatenate([put(gather(w, geometry, c, nb, Fin, Fout, K, k, pack, scale), form) for c in range(slices) for nb in range(blocks)])


def values(img, form):
    """the (lane, slot) values back out of one group: a list of (64, 8) float32 terms, largest first"""
    l = np.arange(64)[:, None] + np.zeros((1, 8), dtype=np.int64)
    j = np.arange(8)[None, :] + np.zeros((64, 1), dtype=np.int64)
    if form == FP32_STEPS:
        return [img.view(np.float32)[j * 64 + l]]
    if form == FP32_HALVES:
        return [img.view(np.float32)[((j >> 2) * 1024 + l * 16 + (j & 3) * 4) // 4]]
    if form == F16X3:
        return [img.view(np.float16)[t * (FRAG // 2) + l * 8 + j].astype(np.float32) for t in range(2)]
    return [bf16_value(img.view(np.uint16)[t * (FRAG // 2) + l * 8 + j]) for t in range(3 if form == BF16X6 else 2)]
