"""The sampling and confidence kernels of the generation loop - token_sample_kernel and token_confidence_kernel (csrc/kernels.hip), which
decide every generated token and every confidence that ranks a reveal: seeded inputs, a float64 statement of the operation on the bf16
logits the kernel gets, the per-element bounds, the checks that hold an implementation to them, and a numpy float32 twin of the kernel
(`twin`, `conf_twin`) with the kernel's operation order per lane, which takes planted faults.  tests/test_gpu_sample.py feeds the checks
with the HIP kernels' outputs (through gget_op_token_sample_probs, which also shows the probabilities), tests/test_sample_reference.py
with the twin (which must pass) and with the twin's planted faults (which must not).

Statement (float64, on the bf16 logits x [R, V]; u = 2^-24, FLT_MIN = 2^-126, NEG = -FLT_MAX).
 1. s = x / T, s = x when T = 0 (T, alg_temp and top_p as the fp32 values the kernel receives).
 2. top-p (0 < top_p < 1): P = softmax(s); c is dropped iff the mass ranked strictly ahead of it (larger s, or equal s and lower index)
    exceeds fp32(top_p).  The first token has nothing ahead of it and always stays.
 3. top-k (top_k > 0), on the values after top-p with dropped tokens at NEG: c is dropped iff at least min(top_k, V) values are strictly
    larger; ties at the k-th value all survive.
 4. P = softmax over the survivors; a dropped token has probability +0.
 5. T = 0: the candidate is the lowest index of the maximum of P.  T > 0: with u32 = hash24(seed, 32, row) * 2^-24 (smtp._rng24) and C the
    inclusive CDF of P in index order, the candidate must belong to the ADMISSIBLE SET
        {c : c survives, P_c >= FLT_MIN, C_(c-1) - e <= u32 <= C_c + e},   e = (k + V) u        (k: below)
    - the first c with C_c > u32, give or take the rounding of an fp32 prefix sum of V terms over probabilities good to k u each.  The last
    survivor is always a member when u32 lies beyond the accumulated mass (the kernel's fallback branch).
 6. confidence: mode 0 P[candidate] (T > 0: of the candidate that was RETURNED); mode 1 largest - second largest P (0 for the second of a
    single survivor, V = 1 included); mode 2 sum_c P_c log(P_c + fp32(1e-10)).
 7. alg_temp > 0: conf / alg_temp - log(-log(a) + fp32(1e-9)), a = fp32(u33 + fp32(1e-9)) replayed in numpy float32 (one IEEE addition),
    u33 the stream-33 draw.

Input condition (every generator asserts it): two distinct values of s in a row differ by at least 2^-6, equal values are equal bit for
bit (x is exact in bf16 and x / T is monotone).  So two distinct tokens have fp32 probabilities that differ by ~1.5 %, far more than any
bound below; equal tokens have identical fp32 probabilities; the kernel's ordering (by probability) is the statement's (by s) wherever the
probabilities do not underflow - and tokens whose probabilities underflow all have mass ~1 ahead of them either way; top-k, which compares
the s themselves, is an exact rule with no tolerance.

Bounds (EXP_C0, EXP_CX, U, TINY of tests/_heads_ref.py).
 * probabilities: |p - P| <= k u P + TINY, k = EXP_C0 + EXP_CX max_survivors |s - max s| + n_survivors + 2 - the cross-entropy form of
   tests/_rows_ref.py (exponential, its argument, the sum of n terms in any order, the division, the division by T).  A dropped token is
   exactly +0 (exp(NEG - m) = 0); a survivor with P < FLT_MIN may be 0 (TINY).
 * top-p ambiguity: a token is AMBIGUOUS when |ahead - fp32(top_p)| <= (k + n_ahead) u ahead + TINY, n_ahead the number of tokens summed
   ahead of it and k the k of the softmax BEFORE the filters (all V tokens): the kernel's fp32 sum could fall on either side.  A row with
   an ambiguous token is ambiguous and skips only what depends on the kept set: probs, their zero pattern, tok, conf.  One exception,
   argued: a row whose logits are all equal, at V a power of two <= 2^23, has e = exp(0) = 1, z = V, p = 1 / V and every partial sum j / V
   EXACT in fp32 in any order - the comparison with fp32(top_p) is then decided exactly and the row is never ambiguous.  The case
   "exact-mass" uses it with top_p = 1/2 = the mass ahead of token V / 2: it stays (`>`), which is the only way to see `>=` there.
 * candidate, T > 0: membership in the admissible set above.  A row whose set has more than one member is NON-DECISIVE (still held to
   membership); mode 0 is checked against P of the returned token.
 * margin: the two probability bounds added; exactly +0 on an exact tie of the top two.
 * entropy: sum_c ((|log x_c| + P_c / x_c) dp_c + P_c dlog_c) + V u sum_c |term_c|, x_c = P_c + 1e-10, dp the probability bound,
   dlog = (LOG_REL |log x| + LOG_ABS) u the error of __logf at x.  The factor of dp is the whole derivative of p log(p + 1e-10),
   log x + p / x: without its second part the bound is 6e-8 for a row with P_1 = 1 - 6e-7, where the half ulp of z = 1 + 6e-7 alone moves
   P_1, and with it the term, by 6e-8 - the fp32 twin missed that bound on five rows of T0.05-V128-mode2 and meets this one.
 * Gumbel: g = -log(y), y = -log(a) + 1e-9: the inner logarithm errs by din = (LOG_REL |log a| + LOG_ABS) u, the addition by u y, which
   reach g as -log(1 - (din / y + u)) (infinite, i.e. the element is skipped and counted, when din >= y: a = 1 - 2^-24 comes close, its
   bound is 4.1 on g = 16.6); the outer logarithm adds (LOG_REL |log y| + LOG_ABS) u.  conf' = conf / alg_temp + g: dconf / alg_temp +
   u |conf / alg_temp| + dg + u |conf'|.
 * token_confidence: tok is the lowest index of the row maximum, always; conf as above with every token a survivor (mode 0: 1 / sum e,
   mode 1: 1 / sum e - exp(m2 - m1) / sum e: two probability bounds).  token_sample at T = 0 without filters and noise on the same logits:
   the same tok, conf within the two bounds added.

Constants.  LOG_REL = EXP_C0 = 4, LOG_ABS = 1: the starting values, and neither had to move.  Measured worst err / bound on the MI355X,
recorded through record_error by tests/test_gpu_sample.py (sample_elementwise/... in the parity-errors record):
   probs 0.46 (round2-1wave-V1025-R8195) | conf mode 0 0.30 (topk-gtV-V300), mode 1 0.13 (p-mode1-T0-alg0-V64-R259), mode 2 0.03
   (p-mode2-T1.3-alg0-V63-R259) | with Gumbel noise: mode 0 0.10, mode 1 0.16 (round2-1wave-V1025-R8195), mode 2 0.05; the row with
   a = 1 - 2^-24 0.01, the row with u33 = 0 0.12 | token_confidence: mode 0 0.06, mode 1 0.03, mode 2 0.02 (token_sample at T = 0
   without filters: the same figures, and the two kernels' confidences were identical) | every candidate a member of its admissible set,
   every zero pattern exact.  (The fp32 twin on the CPU: probs 0.58, conf 0.26.)

Vacuous shares, computed from the reference alone (`shares`), asserted on the CPU and again in the GPU test: ambiguous rows <= 5 % per
case, non-decisive rows <= 2 % per case, rows with an empty admissible set 0, and among the named rows 0 ambiguous and 0 non-decisive.

Inputs.  STRUCTURED rows: a head of 1..24 tokens at random columns, 4.0 and below in steps drawn from {0, 0.5, 0.75, 1, 1.5} (every fourth
row from {0, 0, 0, 0.5}: long flat heads that keep more than 8 tokens), tail tokens between -24 and -40 on a 0.5 grid; all exact in bf16.
T = 50 multiplies the row by 4 (grid 1: 1 / 50 >= 2^-6).  GAUSSIAN rows (V <= 128 only): 2 randn on a 2^-4 grid, |x| < 8.  Random rows of
either kind cannot test the filters at V >= 1024 (most would be ambiguous); structured rows can.
NAMED rows, in every case as far as V, the filters and R allow (R = 259 and above hold them all, ahead of the generic rows and again
behind them where R > 1000; smaller R take a window of the list that moves with the case):
   all-equal | tie-at-k: k - 1 values, then two equal ones at ranks k and k + 1, k + 1 tokens survive (top-k alone, or k <= 3 after top-p) |
   tie-at-p: n equal tokens on top, (j - 1) / n ahead of the j-th, the lower indices survive and the higher do not, n chosen so that no
   j / n comes within 1e-3 of top_p | top2-lane: the two largest at (c, c + 64), one lane, in either order | top2-xor-j: at (c, c ^ 2^j), j = 0..5, in either order, which
   meet at butterfly stage 2^j | top2-ends: at (0, V - 1) | max-last: the maximum in column V - 1 | head-past-70: the first 70 columns
   at the lowest value, dropped by any filter, so the first survivor lies beyond the first 64-lane chunk of the CDF scan | tail-past:
   the last 70 columns at the lowest value, the mirror image, where a draw beyond the mass must fall back on the last token WITH
   probability.
   The all-equal row is left out where top-p runs at V > 2048: its masses j / V are 1.2e-4 apart at V = 8192, the ambiguity bound there
   is 8e-4 - the row would be ambiguous whatever top_p is.  It is also left out where T > 0 at V > 512: its CDF steps are 1 / V apart and
   e is about 2 V u, so 4 V^2 u of all draws - a quarter at V = 1025 - would make it non-decisive.
Case-level settings are named cases: top_k = 1, top_k >= V, top_p = 1e-6 (one survivor, margin exactly p1, entropy within its bound of 0),
T = 0.05 (all but the largest probabilities underflow), T = 50 (a flat row), and four seeds for which a chosen row draws u24 = 0 or
2^24 - 1 on stream 32 (at head-past-70 / tail-past) or on stream 33 - obtained by inverting the hash's finaliser (`seed_for`; a search
over (seed, row) finds the same kind of seed in ~2^24 / R trials), verified with smtp._rng24.
The case none-mode1-T0.7-alg0-V1-R259 (V = 1, margin mode) is the one that caught the kernel returning p1 + 1 = 2 (fault 23 of the twin).
Pad columns [V, ld) of the logits hold bf16 NaN; ld = V (an odd pitch) at V = 65 and 1025, the next multiple of 64 elsewhere.
"""
import functools
import importlib

import numpy as np
import torch

from _heads_ref import EXP_C0, EXP_CX, TINY, U, held_equal, held_true, settle  # noqa: F401
from _rows_ref import Bounded, held  # noqa: F401

smtp = importlib.import_module("graph-gpt_amd.smtp")

F32, F64 = np.float32, np.float64
LOG_REL, LOG_ABS = EXP_C0, 1.0
FLT_MIN = 2.0 ** -126
NEG = -3.4028234663852886e38
EPS10, EPS9 = float(F32(1e-10)), float(F32(1e-9))
INV24 = F32(1.0 / 16777216.0)
U24_MAX = (1 << 24) - 1
SHARE_AMBIGUOUS, SHARE_NONDECISIVE = 0.05, 0.02
TOP_P = 0.8765          # V * TOP_P is no integer (and not within 0.1 of one) for any V of the cases: an all-equal row never sits on it


def align_up(x, a):
    return (x + a - 1) // a * a


# ------------------------------------------------------------------------------------------------------------------ the draws
def _inv32(c):
    return pow(c, -1, 1 << 32)


def seed_for(stream, row, u24, low8=0x5A):
    """The seed for which hash24(seed, stream, row, 0) = u24: the finaliser of smtp_rng is a bijection of 32-bit words, inverted here."""
    M = 0xFFFFFFFF
    x = ((u24 << 8) | low8) & M
    x ^= x >> 16
    x = (x * _inv32(0x846CA68B)) & M
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * _inv32(0x7FEB352D)) & M
    x ^= x >> 16
    seed = ((x - row * 0x85EBCA77) & M) ^ ((stream * 0x9E3779B1) & M)
    assert int(smtp._rng24(seed, stream, row, 0)) == u24
    return seed


def draw(seed, stream, R):
    """fp32 uniforms of rows 0..R-1 on `stream` (exact: 24 bits times 2^-24)."""
    return smtp._rng24(seed, stream, np.arange(R), 0).astype(F32) * INV24


# ------------------------------------------------------------------------------------------------------------------ rows
def _is_bf16(x):
    return bool((torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).float().numpy() == x).all())


def structured_rows(rng, R, V, scale=1.0):
    tail = -24.0 - 0.5 * rng.integers(0, 33, (R, V))
    H = min(24, V)
    h = rng.integers(1, H + 1, R)
    steps = rng.choice(np.array([0.0, 0.5, 0.75, 1.0, 1.5]), (R, H))
    flat = rng.choice(np.array([0.0, 0.0, 0.0, 0.5]), (R, H))
    steps[3::4] = flat[3::4]
    if R > 3:
        h[3::4] = H                                     # (the flat rows carry the longest heads)
    steps[:, 0] = 0.0
    vals = 4.0 - np.cumsum(steps, axis=1)
    pos = np.argsort(rng.random((R, V)), axis=1)[:, :H]
    x = tail
    cur = np.take_along_axis(x, pos, 1)
    np.put_along_axis(x, pos, np.where(np.arange(H)[None, :] < h[:, None], vals, cur), 1)
    return (x * scale).astype(F32)


def gaussian_rows(rng, R, V):
    return (np.clip(np.round(rng.standard_normal((R, V)) * 2.0 * 16.0), -127, 127) / 16.0).astype(F32)


def tie_n(top_p):
    """n equal tokens on top: (j - 1) / n ahead of the j-th; the smallest n that drops at least one, no j / n within 1e-3 of top_p."""
    n = int(np.ceil(1.0 / (1.0 - top_p))) + 1
    while min(abs(j / n - top_p) for j in range(1, n)) < 1e-3:
        n += 1
    return n


def named_rows(rng, V, T, top_p, top_k, scale=1.0):
    """[(name, row [V])] for the setting; see the module docstring."""
    lo, hi, second = -40.0, 4.0, 3.5
    filt_p = 0.0 < top_p < 1.0
    filt_k = 0 < top_k < V
    out = []

    def tail():
        return -24.0 - 0.5 * rng.integers(0, 32, V)       # (-24 .. -39.5: above `lo`)

    def top2(name, c1, c2):
        r = tail()
        r[c1], r[c2] = hi, second
        out.append((name, r))

    if not ((filt_p and V > 2048) or (T > 0 and V > 512)):
        out.append(("all-equal", np.full(V, 0.25)))
    if filt_k and top_k >= 2 and (not filt_p or top_k <= 3):
        r = tail()
        at = rng.permutation(V)[:top_k + 1]
        r[at] = hi - 0.25 * np.minimum(np.arange(top_k + 1), top_k - 1)
        out.append(("tie-at-k", r))
    if filt_p and V >= tie_n(top_p):
        r = tail()
        r[rng.permutation(V)[:tie_n(top_p)]] = hi
        out.append(("tie-at-p", r))
    if V >= 66:
        c = int(rng.integers(0, V - 64))
        top2("top2-lane", c + 64, c)              # (the larger one second in its lane: it must push the smaller down to m2)
        top2("top2-lane-swapped", c, c + 64)
    for j in range(6):
        if V > (1 << j):
            c = int(rng.integers(0, V)) | (1 << j)
            while c >= V:
                c = int(rng.integers(0, V)) | (1 << j)
            top2(f"top2-xor-{j}", c, c ^ (1 << j))           # (the larger one in the lane with bit j set: lane 0's side takes it over at stage 2^j)
            top2(f"top2-xor-{j}-swapped", c ^ (1 << j), c)
    if V >= 2:
        top2("top2-ends", V - 1, 0)
        top2("top2-ends-swapped", 0, V - 1)
    r = tail()
    r[V - 1] = hi
    if V > 2:
        r[V // 2] = second - 0.5
    out.append(("max-last", r))
    if V >= 100 and (filt_p or filt_k):
        for name, sl, inner in (("head-past-70", slice(0, 70), slice(70, V)), ("tail-past", slice(V - 70, V), slice(0, V - 70))):
            r = tail()
            n_in = inner.stop - inner.start
            at = inner.start + rng.permutation(n_in)[:min(6, n_in)]
            r[at] = hi - 0.5 * np.arange(len(at))
            r[sl] = lo
            out.append((name, r))
    return [(n, (r * scale).astype(F32)) for n, r in out]


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(name, V, R, mode, T, top_p, top_k, alg, rows="structured", seed=777, ld=None, pin=None, only=None, rowseed=0):
    """pin = (stream, named row, u24): the kernel seed is chosen so that the row of that name draws u24 on that stream.  only: the rows
    are copies of these named rows alone."""
    T, alg = float(F32(T)), float(F32(alg))               # (the values the kernel receives)
    return dict(name=name, V=V, R=R, mode=mode, T=T, top_p=float(top_p), top_k=int(top_k), alg=alg, rows=rows, seed=seed,
                ld=ld if ld is not None else (V if V in (65, 1025) else align_up(V, 64)), pin=pin, only=only, rowseed=rowseed,
                scale=4.0 if T > 16 else 1.0)


def _name_seed(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


@functools.lru_cache(maxsize=6)
def _inputs(key):
    c = CASES[key] if key in CASES else CONF_CASES[key]
    V, R = c["V"], c["R"]
    rng = np.random.default_rng(_name_seed(c["name"]) + 7919 * c["rowseed"])
    named = named_rows(rng, V, c["T"], c["top_p"], c["top_k"], c["scale"])
    if c["only"]:
        named = [(n, r) for n, r in named if n in c["only"]]
        assert named
        idx = [(i % len(named)) for i in range(R)]
        x = np.stack([named[i][1] for i in idx])
        names = [named[i][0] for i in idx]
    else:
        x = gaussian_rows(rng, R, V) if c["rows"] == "gaussian" else structured_rows(rng, R, V, c["scale"])
        names = [None] * R
        if R >= len(named) + 8:
            place = {j: nr for j, nr in enumerate(named)}
            if R > 1000:
                place.update({R - len(named) + j: nr for j, nr in enumerate(named)})
        else:                                             # a window of the list (three generic rows close the ring) that moves with the case
            ring = named + [None] * 3
            off = _name_seed(c["name"]) % len(ring)
            place = {r: ring[(off + r) % len(ring)] for r in range(R) if ring[(off + r) % len(ring)] is not None}
        for sp, (n, r) in place.items():
            x[sp], names[sp] = r, n
    assert _is_bf16(x)
    s = x.astype(F64) / c["T"] if c["T"] > 0 else x.astype(F64)
    srt = np.sort(s, axis=1)
    d = np.diff(srt, axis=1)
    assert not bool(((d != 0) & (d < 2.0 ** -6)).any()), "input condition: distinct scaled logits closer than 2^-6"
    seed = c["seed"]
    if c["pin"]:
        stream, who, u24 = c["pin"]
        seed = seed_for(stream, names.index(who), u24)
    xpad = np.full((R, c["ld"]), np.nan, F32)
    xpad[:, :V] = x
    return dict(c, x=x, xpad=xpad, names=names, seed=seed)


def inputs(key):
    """The case with x [R, V] fp32 (exact in bf16), xpad [R, ld] (NaN in the pad columns), names [R] and the kernel seed.  Cached:
    treat as read-only."""
    return _inputs(key)


def logits_bf16(i):
    return torch.from_numpy(i["xpad"]).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ float64 statement
def _softmax64(s, alive):
    m = np.where(alive, s, -np.inf).max(1, keepdims=True)
    e = np.where(alive, np.exp(np.where(alive, s - m, 0.0)), 0.0)
    P = e / e.sum(1, keepdims=True)
    span = np.where(alive, np.abs(s - m), 0.0).max(1)
    return P, EXP_C0 + EXP_CX * span + alive.sum(1) + 2


def _count_larger(v):
    """Per element of every row: how many values of the row are strictly larger."""
    R, V = v.shape
    order = np.argsort(-v, axis=1, kind="stable")
    d = np.take_along_axis(v, order, 1)
    j = np.broadcast_to(np.arange(V), (R, V))
    first = np.maximum.accumulate(np.where(np.concatenate([np.ones((R, 1), bool), d[:, 1:] != d[:, :-1]], 1), j, 0), axis=1)
    out = np.empty((R, V), np.int64)
    np.put_along_axis(out, order, first, 1)
    return out


@functools.lru_cache(maxsize=6)
def _reference(key):
    i = inputs(key)
    x, V, R, T = i["x"].astype(F64), i["V"], i["R"], i["T"]
    s = x / T if T > 0 else x
    every = np.ones((R, V), bool)
    amb_tok = np.zeros((R, V), bool)
    drop = np.zeros((R, V), bool)
    if 0.0 < i["top_p"] < 1.0:
        tp = float(F32(i["top_p"]))
        P0, k0 = _softmax64(s, every)
        order = np.argsort(-s, axis=1, kind="stable")
        Ps = np.take_along_axis(P0, order, 1)
        ahead_s = np.cumsum(Ps, axis=1) - Ps
        ahead = np.empty_like(P0)
        np.put_along_axis(ahead, order, ahead_s, 1)
        n_ahead = np.empty((R, V), np.int64)
        np.put_along_axis(n_ahead, order, np.broadcast_to(np.arange(V), (R, V)), 1)
        amb_tok = np.abs(ahead - tp) <= (k0[:, None] + n_ahead) * U * ahead + TINY
        exact = (s == s[:, :1]).all(1) & (V & (V - 1) == 0)          # all equal at a power of two: every sum is exact (docstring)
        amb_tok[exact] = False
        drop = ahead > tp
    s2 = np.where(drop, NEG, s)
    if i["top_k"] > 0:
        drop = drop | (_count_larger(s2) >= min(i["top_k"], V))
    alive = ~drop
    P, k = _softmax64(s, alive)
    pb = k[:, None] * U * P + TINY
    Ps = np.sort(P, axis=1)[:, ::-1]
    P1 = Ps[:, 0]
    P2 = Ps[:, 1] if V > 1 else np.zeros(R)
    lx = np.abs(np.log(P + EPS10))
    terms = P * np.log(P + EPS10)
    ent_b = ((lx + P / (P + EPS10)) * pb + P * (LOG_REL * lx + LOG_ABS) * U).sum(1) + V * U * np.abs(terms).sum(1)
    ref = dict(s=s, alive=alive, P=P, k=k, pb=pb, amb=amb_tok.any(1), tok0=P.argmax(1), P1=P1, P2=P2, ent=terms.sum(1), ent_b=ent_b,
               named=np.array([n is not None for n in i["names"]]))
    if T > 0:
        u = draw(i["seed"], 32, R).astype(F64)
        Cc = np.cumsum(P, axis=1)
        e = ((k + V) * U)[:, None]
        ref["adm"] = alive & (P >= FLT_MIN) & (Cc - P - e <= u[:, None]) & (u[:, None] <= Cc + e)
        ref["u32"] = u
    if i["alg"] > 0:
        a = (draw(i["seed"], 33, R) + F32(1e-9)).astype(F64)
        y = -np.log(a) + EPS9
        r = (LOG_REL * np.abs(np.log(a)) + LOG_ABS) * U / y + U
        prop = np.where(r < 1.0, -np.log1p(-np.where(r < 1.0, r, 0.0)), np.inf)
        ref["g"], ref["g_b"] = -np.log(y), prop + (LOG_REL * np.abs(np.log(y)) + LOG_ABS) * U
    return ref


def reference(key):
    """Cached: treat as read-only."""
    return _reference(key)


def shares(key):
    i, r = inputs(key), reference(key)
    out = dict(ambiguous=float(r["amb"].mean()), named_ambiguous=int((r["amb"] & r["named"]).sum()), nondecisive=0.0, named_nondecisive=0,
               empty=0)
    if i["T"] > 0:
        n = r["adm"].sum(1)
        out.update(nondecisive=float((n > 1).mean()), named_nondecisive=int(((n > 1) & r["named"]).sum()), empty=int((n == 0).sum()))
    return out


def shares_hold(key):
    s = shares(key)
    assert s["ambiguous"] <= SHARE_AMBIGUOUS, (key, s)
    assert s["nondecisive"] <= SHARE_NONDECISIVE, (key, s)
    assert s["empty"] == 0 and s["named_ambiguous"] == 0 and s["named_nondecisive"] == 0, (key, s)
    return s


def kept_counts(key):
    return reference(key)["alive"].sum(1)


# ------------------------------------------------------------------------------------------------------------------ checks
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _conf_ref(i, r, tok, rows):
    """(ref, bound, exact-zero rows) of the confidence before the noise, on `rows`; tok: the tokens that were returned."""
    P, pb = r["P"], r["pb"]
    zero = np.zeros(len(rows), bool)
    if i["mode"] == 0:
        t = np.clip(tok[rows], 0, i["V"] - 1) if i["T"] > 0 else r["tok0"][rows]
        return P[rows, t], pb[rows, t], zero
    if i["mode"] == 1:
        kk = r["k"][rows] * U
        return r["P1"][rows] - r["P2"][rows], kk * (r["P1"][rows] + r["P2"][rows]) + 2 * TINY, r["P1"][rows] == r["P2"][rows]
    return r["ent"][rows], r["ent_b"][rows], zero


def check(key, probs, conf, tok):
    """probs fp32 [R, V], conf fp32 [R], tok int64 [R] (numpy) of a token_sample implementation on the case -> results."""
    i, r = inputs(key), reference(key)
    V, R = i["V"], i["R"]
    dec = ~r["amb"]
    rows = np.nonzero(dec)[0]
    out = [held_true("tok in [0, V)", bool(((tok >= 0) & (tok < V)).all()), f"a token outside [0, {V}): {tok[(tok < 0) | (tok >= V)][:4]}"),
           held_true("conf and probs are finite (no pad column, no NaN reached them)", bool(np.isfinite(conf).all() and np.isfinite(probs).all()),
                     "a NaN or infinity in conf or probs")]
    if len(rows) == 0:
        return out
    dropped = ~r["alive"][rows]
    pz = probs[rows][dropped]
    out.append(held_true("probs zero pattern: a dropped token is +0", bool((pz.view(np.int32) == 0).all()),
                         f"{int((pz.view(np.int32) != 0).sum())} dropped tokens are not +0"))
    out.append(held("probs", _t(probs[rows]), _t(r["P"][rows]), _t(r["pb"][rows])))
    tk = np.clip(tok, 0, V - 1)
    if i["T"] > 0:
        ok = r["adm"][rows, tk[rows]]
        bad = rows[~ok]
        out.append(held_true("tok is a member of the admissible set", bool(ok.all()),
                             f"{len(bad)} rows, the first {bad[:4]}: tok {tok[bad[:4]]} u {r['u32'][bad[:4]]} "
                             f"admissible {[np.nonzero(r['adm'][b])[0][:4].tolist() for b in bad[:4]]} names {[i['names'][b] for b in bad[:4]]}"))
    else:
        ok = tok[rows] == r["tok0"][rows]
        bad = rows[~ok]
        out.append(held_true("tok is the lowest index of the maximum", bool(ok.all()),
                             f"{len(bad)} rows, the first {bad[:4]}: tok {tok[bad[:4]]} want {r['tok0'][bad[:4]]}"))
    ref, bound, zero = _conf_ref(i, r, tok, rows)
    got = conf[rows].astype(F64)
    if i["alg"] > 0:
        g, gb = r["g"][rows], r["g_b"][rows]
        ref = ref / i["alg"]
        bound = bound / i["alg"] + U * np.abs(ref) + gb + U * np.abs(ref + g)
        ref = ref + g
        fin = np.isfinite(bound)
        ref, bound, got = ref[fin], bound[fin], got[fin]
    elif bool(zero.any()):
        z = conf[rows][zero]
        out.append(held_true("margin of an exact tie is +0", bool((z.view(np.int32) == 0).all()), f"{z[z.view(np.int32) != 0][:4]}"))
    out.append(held("conf", _t(got)[:, None], _t(ref)[:, None], _t(bound)[:, None]))
    return out


# ------------------------------------------------------------------------------------------------------------------ the fp32 twin
def _tree(v):
    """wave_allreduce of csrc/common.h as a sum: pairs, quads, eights ... of the 64 lanes."""
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _lanes(a, fill):
    R, V = a.shape
    n = align_up(V, 64)
    out = np.full((R, n), fill, a.dtype)
    out[:, :V] = a
    return out.reshape(R, n // 64, 64)


def _wave_sum(a, upto=None):
    """Every lane sums its columns c = lane, lane + 64, ... in order, then the tree.  upto: columns >= upto are left out (a fault)."""
    if upto is not None:
        a = a.copy()
        a[:, upto:] = 0
    return _tree(np.cumsum(_lanes(a.astype(F32), F32(0)), axis=1, dtype=F32)[:, -1])


def _softmax32(s):
    m = s.max(1, keepdims=True)
    e = np.exp(s - m, dtype=F32)
    z = _wave_sum(e)
    return (e / z[:, None]).astype(F32)


def _top2(p, init, fault=None):
    """(m1, m2, i1): the lane scan and the butterfly of both kernels."""
    R, V = p.shape
    L = _lanes(p, F32(0))
    m1, m2 = np.full((R, 64), init, F32), np.full((R, 64), init, F32)
    i1 = np.full((R, 64), 0x7FFFFFFF, np.int64)
    lane = np.arange(64)
    for ch in range(L.shape[1]):
        c = ch * 64 + lane
        v, valid = L[:, ch], (c < V)[None, :]
        up1 = valid & ((v >= m1) if fault == 13 else (v > m1))
        up2 = valid & ~up1 & (v > m2)
        m2 = np.where(up1, m2 if fault == 14 else m1, np.where(up2, v, m2))
        i1 = np.where(up1, c[None, :], i1)
        m1 = np.where(up1, v, m1)
    for o in (32, 16, 8, 4, 2, 1):
        perm = lane ^ o
        om1, om2, oi1 = m1[:, perm], m2[:, perm], i1[:, perm]
        take = (om1 > m1) | ((om1 == m1) & ((oi1 > i1) if fault == 13 else (oi1 < i1)))
        m2 = np.where(take, om2 if (fault == 15 and o == 4) else np.maximum(m1, om2), np.maximum(m2, om1))
        m1, i1 = np.where(take, om1, m1), np.where(take, oi1, i1)
    return m1[:, 0], m2[:, 0], i1[:, 0]


def _entropy32(p, fault=None):
    V = p.shape[1]
    with np.errstate(all="ignore"):
        t = (p * np.log(p + F32(1e-10), dtype=F32)).astype(F32)
    return _wave_sum(t, upto=64 * (V // 64) if fault == 17 else None)


FAULTS = {
    1: "the top-p comparison >= instead of >", 2: "a top-p tie rule that prefers the higher index",
    3: "top-p drops the first token too (the mass up to and including the token is compared)", 4: "top-k counts >=: ties at k die",
    5: "top-k not clamped to V: the k-th value is read past the row, where nothing compares above it",
    6: "top-k without its snapshot: the comparison reads the probability buffer as it was left (unwritten for a wave's first row)",
    7: "the filters in the other order", 8: "a dropped token left at a tiny non-zero p", 9: "the CDF carry not added across chunks",
    10: "lanes c >= V take part in the scan", 11: ">= in the CDF hit: u = 0 picks a zero-probability token",
    12: "the fallback returns V - 1 instead of the last token with probability", 13: "an arg-max that prefers the higher index on ties",
    14: "the second maximum lost when both maxima sit in one lane", 15: "the second maximum lost at butterfly stage 4",
    16: "the margin taken from pre-filter probabilities", 17: "an entropy sum that drops the columns >= 64 floor(V / 64)",
    18: "mode-0 confidence at T > 0 taken as max p instead of p[x0]", 19: "Gumbel noise drawn from stream 32",
    20: "the noise added before the division by alg_temp", 21: "the temperature applied after the filters",
    22: "a row stride of V instead of ld",
    23: "the margin at V = 1 taken against the scan's initial -1 (what the kernel did until these checks: conf = 2)",
}


def twin(key, fault=None, info=None, mode=None):
    """(probs fp32 [R, V], conf fp32 [R], tok int64 [R]) of token_sample_kernel's arithmetic in numpy float32.  info (a dict) receives
    `fellback`, the rows that took the fallback branch; mode overrides the case's (the token_confidence cases carry none of their own)."""
    i = inputs(key)
    V, R, T, ld = i["V"], i["R"], i["T"], i["ld"]
    mode = i["mode"] if mode is None else mode
    with np.errstate(all="ignore"):
        flat = i["xpad"].reshape(-1)
        x = flat[np.arange(R)[:, None] * (V if fault == 22 else ld) + np.arange(V)[None, :]].astype(F32)
        Tn = F32(T)
        s = (x / Tn).astype(F32) if (T > 0 and fault != 21) else x.copy()
        cidx = np.arange(V)[None, :]
        p_pre = None

        def top_p(s):
            p = _softmax32(s)
            ahead = np.zeros((R, V), F32)
            for c in range(V):
                pi = p[:, c:c + 1]
                cond = (pi > p) | ((pi == p) & ((c > cidx) if fault == 2 else (c < cidx)))
                ahead += np.where(cond, pi, F32(0))
            tp = F32(i["top_p"])
            mass = ahead + p if fault == 3 else ahead
            return np.where((mass >= tp) if fault == 1 else (mass > tp), F32(NEG), s), p

        def top_k(s):
            kk = min(i["top_k"], V)
            if fault == 6:
                larger = np.zeros((R, V), np.int64)
            elif fault == 4:
                larger = (V - _count_larger(-s)) - 1            # how many OTHER values are >=
            else:
                larger = _count_larger(s)
            if fault == 5 and i["top_k"] > V:
                return np.full((R, V), F32(NEG))
            return np.where(larger >= kk, F32(NEG), s)

        on_p, on_k = 0.0 < i["top_p"] < 1.0, i["top_k"] > 0
        if fault == 7:
            if on_k:
                s = top_k(s)
            if on_p:
                s, p_pre = top_p(s)
        else:
            if on_p:
                s, p_pre = top_p(s)
            if on_k:
                s = top_k(s)
        if fault == 21 and T > 0:
            s = np.where(s == F32(NEG), s, (s / Tn).astype(F32))
        dropped = s == F32(NEG)
        p = _softmax32(s)
        if fault == 8:
            p = np.where(dropped, F32(1e-30), p)
        m1, m2, i1 = _top2(p, F32(-1), fault)
        if T > 0:
            u = draw(i["seed"], 32, R)
            run, found, last_pos = np.zeros(R, F32), np.full(R, -1, np.int64), np.full(R, -1, np.int64)
            L = _lanes(p, F32(1) if fault == 10 else F32(0))
            lane = np.arange(64)
            for ch in range(L.shape[1]):
                active = found < 0
                if not bool(active.any()):
                    break
                v = L[:, ch]
                pre = v.copy()
                for o in (1, 2, 4, 8, 16, 32):
                    t = pre.copy()
                    pre[:, o:] = t[:, o:] + t[:, :-o]
                valid = np.broadcast_to(((ch * 64 + lane) < V)[None, :], v.shape) if fault != 10 else np.ones(v.shape, bool)
                tot = (pre if fault == 9 else run[:, None] + pre)
                hit = valid & ((tot >= u[:, None]) if fault == 11 else (tot > u[:, None]))
                pos = valid & (v > 0)
                lp = ch * 64 + 63 - np.argmax(pos[:, ::-1], axis=1)
                last_pos = np.where(active & pos.any(1), lp, last_pos)
                found = np.where(active & hit.any(1), ch * 64 + np.argmax(hit, axis=1), found)
                run = (run + pre[:, 63]).astype(F32)
            fell = found < 0
            if info is not None:
                info["fellback"] = fell
            fb = np.full(R, V - 1, np.int64) if fault == 12 else np.where(last_pos >= 0, last_pos, i1)
            x0 = np.where(fell, fb, found)
            cf = p[np.arange(R), np.clip(x0, 0, V - 1)]
            if fault == 18:
                cf = m1
        else:
            x0, cf = i1, m1
        if mode == 1:
            if fault == 16 and p_pre is not None:
                q1, q2, _ = _top2(p_pre, F32(-1))
                cf = q1 - q2
            else:
                cf = m1 - (m2 if fault == 23 else np.maximum(m2, F32(0)))
        if mode == 2:
            cf = _entropy32(p, fault)
        if i["alg"] > 0:
            u2 = draw(i["seed"], 32 if fault == 19 else 33, R)
            g = -np.log(-np.log(u2 + F32(1e-9), dtype=F32) + F32(1e-9), dtype=F32)
            at = F32(i["alg"])
            cf = ((cf + g) / at) if fault == 20 else (cf / at + g)
        return p.astype(F32), np.asarray(cf, F32), x0.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ token_confidence
@functools.lru_cache(maxsize=6)
def _conf_reference(key):
    i = inputs(key)
    x = i["x"].astype(F64)
    R, V = x.shape
    P, k = _softmax64(x, np.ones((R, V), bool))
    part = -np.partition(-P, 1, axis=1)[:, :2]
    lx = np.abs(np.log(P + EPS10))
    terms = P * np.log(P + EPS10)
    pb = k[:, None] * U * P + TINY
    ent_b = ((lx + P / (P + EPS10)) * pb + P * (LOG_REL * lx + LOG_ABS) * U).sum(1) + V * U * np.abs(terms).sum(1)
    return dict(tok=x.argmax(1), P1=part[:, 0], P2=part[:, 1], k=k, ent=terms.sum(1), ent_b=ent_b)


def conf_reference(key):
    return _conf_reference(key)


def _conf_mode(r, mode):
    if mode == 0:
        return r["P1"], r["k"] * U * r["P1"] + TINY, None
    if mode == 1:
        return r["P1"] - r["P2"], r["k"] * U * (r["P1"] + r["P2"]) + 2 * TINY, r["P1"] == r["P2"]
    return r["ent"], r["ent_b"], None


def conf_check(key, mode, conf, tok, tag="token_confidence"):
    r = conf_reference(key)
    ref, bound, zero = _conf_mode(r, mode)
    bad = np.nonzero(tok != r["tok"])[0]
    out = [held_true(f"{tag} tok is the lowest index of the row maximum", len(bad) == 0,
                     f"{len(bad)} rows, the first {bad[:4]}: tok {tok[bad[:4]]} want {r['tok'][bad[:4]]}"),
           held_true(f"{tag} conf is finite", bool(np.isfinite(conf).all()), "a NaN or infinity in conf")]
    if zero is not None and bool(zero.any()):
        z = conf[zero]
        out.append(held_true(f"{tag} margin of an exact tie is +0", bool((z.view(np.int32) == 0).all()), f"{z[z.view(np.int32) != 0][:4]}"))
    out.append(held(f"{tag} conf", _t(conf.astype(F64))[:, None], _t(ref)[:, None], _t(bound)[:, None]))
    return out


def conf_pair_check(key, mode, conf_a, conf_b):
    """token_confidence against token_sample at T = 0 without filters and noise: both within the bound of the same reference."""
    _, bound, _ = _conf_mode(conf_reference(key), mode)
    return held("token_sample (T = 0, no filters) conf against token_confidence", _t(conf_a.astype(F64))[:, None], _t(conf_b.astype(F64))[:, None],
                _t(2 * bound)[:, None])


def conf_twin(key, mode, fault=None):
    i = inputs(key)
    x = i["xpad"][:, :i["V"]].astype(F32)
    with np.errstate(all="ignore"):
        m1, m2, i1 = _top2(x, F32(-np.inf), fault)
        e = np.exp(x - m1[:, None], dtype=F32)
        se = _wave_sum(e)
        if mode == 2:
            out = _entropy32((e / se[:, None]).astype(F32), fault)
        elif mode == 1:
            out = F32(1) / se - np.exp(m2 - m1, dtype=F32) / se
        else:
            out = F32(1) / se
    return np.asarray(out, F32), i1.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ the case lists
# generic rows of these cases re-drawn until the reference - alone - finds the case within the shares
ROWSEED = {"pk-mode1-T0-alg0-V8192-R8": 1}


def _build_cases():
    cases = {}

    def add(name, *a, **k):
        assert name not in cases
        k.setdefault("rowseed", ROWSEED.get(name, 0))
        cases[name] = make_case(name, *a, **k)

    Vs = (1, 2, 63, 64, 65, 128, 300, 1024, 1025, 8192)
    Ts = (1.0, 0.7, 1.3)
    n = 0
    for variant in range(2):
        for f, filt in enumerate(("p", "k", "pk", "none")):
            for mode in range(3):
                V = Vs[n % 10]
                R = 8 if V == 8192 else (1, 3, 259)[(n // 10 + n) % 3]
                T = Ts[n % 3] if variant == 0 else 0.0
                alg = 0.4 if (n % 2 == 1) == (variant == 0) else 0.0
                top_p = TOP_P if "p" in filt else 0.0
                top_k = 0 if "k" not in filt else (3 if filt == "pk" else max(1, min(20, V // 2)))
                add(f"{filt}-mode{mode}-T{T:g}-alg{alg:g}-V{V}-R{R}", V, R, mode, T, top_p, top_k, alg)
                n += 1
    # the second grid-stride round of both launch forms (four waves per block up to V = 1024, one beyond)
    add("round2-4wave-V64-R32773", 64, 4 * 8192 + 5, 0, 1.0, TOP_P, 3, 0.0)
    add("round2-1wave-V1025-R8195", 1025, 8192 + 3, 1, 0.7, 0.0, 20, 0.4)
    add("V8192-p-mode2", 8192, 8, 2, 1.0, TOP_P, 0, 0.0)
    add("V8192-k-mode0", 8192, 8, 0, 1.3, 0.0, 20, 0.0, rowseed=1)
    add("topk1-V300", 300, 259, 1, 1.0, 0.0, 1, 0.0)
    add("topk-geV-V65", 65, 259, 2, 1.0, 0.0, 65, 0.0)
    add("topk-gtV-V300", 300, 259, 0, 0.7, TOP_P, 1000, 0.0)
    add("topp1e-6-V300-mode1", 300, 259, 1, 1.0, 1e-6, 0, 0.0)
    add("topp1e-6-V65-mode2", 65, 259, 2, 0.7, 1e-6, 0, 0.0)
    add("T0.05-V300", 300, 259, 0, 0.05, TOP_P, 20, 0.0)
    add("T0.05-V128-mode2", 128, 259, 2, 0.05, 0.0, 0, 0.0)
    add("T50-V65-mode2", 65, 259, 2, 50.0, 0.0, 0, 0.0)
    add("T50-V128-p", 128, 259, 1, 50.0, TOP_P, 0, 0.0, rowseed=1)
    add("u32-zero-V300", 300, 259, 0, 1.0, TOP_P, 20, 0.0, pin=(32, "head-past-70", 0))
    add("u32-max-V300", 300, 259, 0, 1.0, TOP_P, 20, 0.0, pin=(32, "tail-past", U24_MAX))
    add("u33-zero-V300", 300, 259, 1, 1.0, TOP_P, 0, 0.4, pin=(33, "top2-lane", 0))
    add("u33-max-V300", 300, 259, 2, 1.0, 0.0, 20, 0.4, pin=(33, "top2-lane", U24_MAX))
    add("exact-mass-V64", 64, 3, 0, 1.0, 0.5, 0, 0.0, only=("all-equal",))
    add("gaussian-V128-p", 128, 259, 0, 1.0, 0.613, 0, 0.0, rows="gaussian")
    add("gaussian-V63-k-mode2", 63, 259, 2, 0.7, 0.0, 5, 0.4, rows="gaussian")
    add("k-mode1-T1-V300-R259", 300, 259, 1, 1.0, 0.0, 20, 0.0)
    add("p-mode1-T0.7-V300-R259", 300, 259, 1, 0.7, TOP_P, 0, 0.0)
    add("pk-mode0-T1-V300-R259", 300, 259, 0, 1.0, TOP_P, 3, 0.0)
    add("p-mode0-T1.3-V1024-R259", 1024, 259, 0, 1.3, TOP_P, 0, 0.0)
    return cases


def _build_conf_cases():
    cases = {}
    for V in (2, 63, 64, 65, 97, 41245):
        for R in (1, 3, 259):
            name = f"conf-V{V}-R{R}"
            cases[name] = make_case(name, V, R, 0, 0.0, 0.0, 0, 0.0, rows="gaussian" if V in (63, 97) else "structured",
                                    ld=41280 if V == 41245 else None)
    name = "conf-round2-V64-R16389"
    cases[name] = make_case(name, 64, 4 * 4096 + 5, 0, 0.0, 0.0, 0, 0.0)
    return cases


CASES = _build_cases()
CONF_CASES = _build_conf_cases()


def variant(key, **changes):
    """Registers (once) and names a copy of a case with some settings changed, e.g. other generic rows (rowseed)."""
    name = key + "#" + ",".join(f"{k}={v}" for k, v in sorted(changes.items()))
    if name not in CASES:
        CASES[name] = dict(CASES[key], name=name, **changes)
    return name
