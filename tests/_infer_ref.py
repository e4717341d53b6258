"""NumPy twins of the prediction-pass kernels (csrc/infer.hip) and of the dump format, written on bit patterns and index arithmetic so
that they share nothing with the code under test:

  f32_to_f16_bits   fp32 bit patterns -> fp16 bit patterns, round to nearest even (overflow to +-inf, subnormals produced, NaN -> a NaN)
  bf16_to_f16_bits  bf16 bit patterns -> fp16 bit patterns: the bf16 value is an fp32 value with 16 zero bits behind it, rounded once
  node_records      the record builder of process_data: (idx[p // S], raw[p], pred[p]) for every flat p with raw[p] != -100, ascending p
  argmax_first      torch.argmax over the last axis: the first maximal class, a NaN counting as maximal
  csv_rows          the "idx,value" lines of the logits / hidden-state dump
"""
import base64
import json

import numpy as np

CURATED_F32 = np.array(
    [0.0, -0.0,
     2.0 ** -25, -2.0 ** -25,            # the tie between 0 and the smallest subnormal: to even = 0
     3 * 2.0 ** -25, -3 * 2.0 ** -25,    # the tie between 2^-24 and 2^-23: to even = 2^-23
     2.0 ** -24, 2.0 ** -14,             # the smallest subnormal, the smallest normal
     2.0 ** -14 - 2.0 ** -25,            # just under the smallest normal: rounds up into it
     65504.0, 65519.996, 65520.0, -65520.0,   # the largest fp16, the last value that rounds to it, the first that overflows
     np.inf, -np.inf, np.nan, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-30, -1e30], dtype=np.float32)


def f32_to_f16_bits(bits32) -> np.ndarray:
    """uint32 fp32 patterns -> uint16 fp16 patterns (RNE).  NaNs come back as 0x7e00 | sign (any NaN is a NaN to the tests)."""
    b = np.asarray(bits32, dtype=np.uint32).astype(np.uint64)
    sign = ((b >> 16) & 0x8000).astype(np.uint64)
    exp = ((b >> 23) & 0xFF).astype(np.int64)
    man = (b & 0x7FFFFF).astype(np.uint64)
    out = np.zeros(b.shape, dtype=np.uint64)
    is_nan = (exp == 255) & (man != 0)
    is_inf = (exp == 255) & (man == 0)
    # a finite, non-zero fp32 value is sig * 2^(e - 23) with sig = 2^23 | man (normals) or man with e = -126 (fp32 subnormals)
    sig = np.where(exp == 0, man, man | (1 << 23))
    e = np.where(exp == 0, -126, exp - 127)
    # fp16 keeps 10 fraction bits of a normal (e >= -14) and counts in units of 2^-24 below: drop `shift` low bits of sig
    shift = np.where(e >= -14, 13, 13 + (-14 - e))
    shift = np.minimum(shift, 40)                                  # (anything this small rounds to zero whatever the shift)
    kept = sig >> shift.astype(np.uint64)
    rest = sig & ((np.uint64(1) << shift.astype(np.uint64)) - np.uint64(1))
    half = np.uint64(1) << (shift.astype(np.uint64) - np.uint64(1))
    up = (rest > half) | ((rest == half) & ((kept & 1) == 1))
    kept = kept + up.astype(np.uint64)
    # normals: kept holds the implicit bit at 2^10, and adding (e + 14) << 10 on top makes a carry out of the fraction bump the exponent;
    # subnormals: kept IS the pattern (a carry into bit 10 is the smallest normal)
    normal = np.where(e >= -14, kept + ((e + 14).clip(min=0).astype(np.uint64) << np.uint64(10)), kept)
    normal = np.where(normal >= 0x7C00, 0x7C00, normal)            # overflow -> inf
    out = np.where(is_nan, 0x7E00, np.where(is_inf, 0x7C00, normal))
    return (out | sign).astype(np.uint16)


def bf16_to_f16_bits(bits16) -> np.ndarray:
    return f32_to_f16_bits(np.asarray(bits16, dtype=np.uint16).astype(np.uint32) << 16)


def f16_is_nan(bits) -> np.ndarray:
    b = np.asarray(bits, dtype=np.uint16)
    return ((b & 0x7C00) == 0x7C00) & ((b & 0x03FF) != 0)


def same_f16(got, want) -> bool:
    """bit equality, every NaN equal to every NaN"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = f16_is_nan(got), f16_is_nan(want)
    return got.shape == want.shape and bool(np.array_equal(gn, wn)) and bool(np.array_equal(got[~gn], want[~wn]))


def argmax_first(logits: np.ndarray) -> np.ndarray:
    """the first NaN of a row when it has one, else the first maximum"""
    lg = np.asarray(logits, dtype=np.float32)
    nan = np.isnan(lg)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, lg).argmax(-1)).astype(np.int64)


def node_records(pred, raw_node_idx, idx) -> np.ndarray:
    """i64 [n, 3]; pred / raw_node_idx [B, S], idx [B]"""
    pred, raw, idx = np.asarray(pred), np.asarray(raw_node_idx), np.asarray(idx)
    S = raw.shape[1]
    p = np.flatnonzero(raw.reshape(-1) != -100)                   # ascending flat positions
    return np.stack((idx.astype(np.int64)[p // S], raw.reshape(-1)[p].astype(np.int64), pred.reshape(-1)[p].astype(np.int64)), axis=1)


def csv_rows(idx, values_f16) -> str:
    """values_f16: float16 [N, C]"""
    lines = []
    for i, row in zip(np.asarray(idx).reshape(-1), values_f16):
        if values_f16.shape[1] == 1:
            field = repr(float(row[0]))         # (an f-string formats a NumPy scalar as the Python float it widens to: 65504.0, not 65500.0)
        else:
            inner = {"dtype": "float16", "shape": [int(row.shape[0])], "data": base64.b64encode(row.tobytes()).decode()}
            field = base64.urlsafe_b64encode(json.dumps(inner).encode()).decode()
        lines.append(f"{int(i)},{field}\n")
    return "".join(lines)
