"""The sampling and confidence kernels of the generation loop through the C ABI (gget_op_token_sample_probs, gget_op_token_sample,
gget_op_token_confidence): every probability, every candidate and every confidence against the float64 statement of tests/_sample_ref.py
on the same bf16 logits and on the draws the numpy twin of the counter hash gives - bounds, inputs, the admissible set of a candidate and
the vacuous shares are derived there, and tests/test_sample_reference.py shows on the CPU that the checks reject 22 planted faults.
Logits carry bf16 NaN in their pad columns; outputs land in buffers pre-filled with NaN sentinels with pad rows (and, for probs, pad
columns) behind them.  The old entry is held to the bits of the new one, with and without the probabilities written.  With them: the
exact small tests of gget_op_unmask_origin / _rows against generation.draws and of gget_op_smtp_rows against smtp.row_mask_selection at
the edges the older tests leave out."""
import importlib

import numpy as np
import pytest
import torch

import _sample_ref as S
from _gpu_out import SENT32, Out, P, ST
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
gen = importlib.import_module("graph-gpt_amd.generation")
smtp = importlib.import_module("graph-gpt_amd.smtp")
F32, I64 = torch.float32, torch.int64
PROBS_PAD = 3                        # pad columns of the probs output: ld_p = V + 3


@pytest.fixture(scope="module")
def lib():
    return L.load()


def finish(op, case, results):
    """Record max(err / bound) of the case - overall and per bounded quantity - then fail on whatever was out of bound."""
    ratio, msgs = S.settle(results)
    record_error(f"sample_elementwise/{op}", case, ratio, 1.0)
    worst = {}
    for t in results:
        if isinstance(t, S.Bounded):
            worst[t[0]] = max(worst.get(t[0], 0.0), t[1])
    for q, r in worst.items():
        record_error(f"sample_elementwise/{op}/{q}", case, r, 1.0)
    print(f"{op} {case}: " + ", ".join(f"{q} {r:.4f}" for q, r in worst.items()))
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


_LOGITS = {}


def device_logits(key):
    if key not in _LOGITS:
        _LOGITS.clear()                                  # (one case at a time on the device)
        _LOGITS[key] = S.logits_bf16(S.inputs(key)).cuda()
    return _LOGITS[key]


def run_sample(lib, key, entry="probs", mode=None, plain=False):
    """entry: "probs" (the new entry, probabilities written), "null" (the new entry, probs NULL), "old" (gget_op_token_sample).
    plain: T = 0, no filters, no noise, whatever the case says.  -> (probs [R, V] or None, conf [R], tok [R]) as numpy."""
    i = S.inputs(key)
    R, V = i["R"], i["V"]
    x = device_logits(key)
    conf, tok = Out(R, 1, F32), Out(R, 1, I64)
    pr = Out(R, V + PROBS_PAD, F32) if entry == "probs" else None
    sets = (0.0, 0.0, 0, 0.0) if plain else (i["T"], i["top_p"], i["top_k"], i["alg"])
    args = (P(x), i["ld"], R, V, i["mode"] if mode is None else mode, sets[0], sets[1], sets[2], sets[3], i["seed"], P(conf.buf), P(tok.buf))
    if entry == "old":
        L.check(lib.gget_op_token_sample(*args, ST()))
    else:
        L.check(lib.gget_op_token_sample_probs(*args, P(pr.buf) if pr else None, V + PROBS_PAD if pr else 0, ST()))
    probs = None
    if pr is not None:
        body = pr.body()
        assert bool((body[:, V:].contiguous().view(torch.int32) == SENT32).all()), "wrote into the pad columns of probs"
        probs = body[:, :V].contiguous().numpy()
    return probs, conf.body().view(-1).numpy(), tok.body().view(-1).numpy()


def same_bits(name, a, b):
    return S.held_true(name, bool(np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2], b[2])),
                       "conf or tok differ between the two entries")


# ------------------------------------------------------------------------------------------------------------------ token_sample
@pytest.mark.parametrize("key", list(S.CASES))
def test_token_sample(lib, key):
    S.shares_hold(key)
    new = run_sample(lib, key)
    results = S.check(key, *new)
    results.append(same_bits("gget_op_token_sample_probs without probs gives the same conf and tok", new, run_sample(lib, key, entry="null")))
    results.append(same_bits("gget_op_token_sample gives the bits of the new entry", new, run_sample(lib, key, entry="old")))
    finish("token_sample", key, results)


def test_token_sample_probs_rejects_bad_arguments(lib):
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device="cuda")
    big = torch.zeros(1, 8256, dtype=torch.bfloat16, device="cuda")
    conf, tok, pr = Out(4, 1, F32), Out(4, 1, I64), Out(4, 64, F32)

    def call(logits=x, ld=64, R=4, V=50, mode=0, T=1.0, top_p=0.9, top_k=5, alg=0.0, probs=pr, ld_p=64):
        return lib.gget_op_token_sample_probs(P(logits), ld, R, V, mode, T, top_p, top_k, alg, 1, P(conf.buf), P(tok.buf),
                                              P(probs.buf) if probs is not None else None, ld_p, ST())

    bad = dict(V8193=call(logits=big, ld=8256, R=1, V=8193, probs=None), V0=call(V=0), ld_below_V=call(ld=49), ldp_below_V=call(ld_p=49),
               negative_T=call(T=-1.0), negative_alg=call(alg=-0.5), negative_k=call(top_k=-1), mode3=call(mode=3), mode_neg=call(mode=-1))
    assert all(rc != 0 for rc in bad.values()), bad
    assert lib.gget_last_error()
    assert conf.untouched() and tok.untouched() and pr.untouched()
    assert call(ld_p=0, probs=None) == 0 and call(V=64, ld_p=64) == 0          # ld_p is not looked at without probs; ld_p = V is enough
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ token_confidence
@pytest.mark.parametrize("key", list(S.CONF_CASES))
def test_token_confidence(lib, key):
    i = S.inputs(key)
    R, V = i["R"], i["V"]
    x = device_logits(key)
    results = []
    for mode in range(3):
        conf, tok = Out(R, 1, F32), Out(R, 1, I64)
        L.check(lib.gget_op_token_confidence(P(x), i["ld"], R, V, mode, P(conf.buf), P(tok.buf), ST()))
        c, t = conf.body().view(-1).numpy(), tok.body().view(-1).numpy()
        results += [type(r)((f"[mode {mode}] {r[0]}", r[1], r[2])) for r in S.conf_check(key, mode, c, t)]
        if V <= 8192:                                    # token_sample at T = 0 without filters and noise: the same thing, computed its way
            _, c2, t2 = run_sample(lib, key, entry="null", mode=mode, plain=True)
            results += [type(r)((f"[mode {mode}] {r[0]}", r[1], r[2])) for r in S.conf_check(key, mode, c2, t2, tag="token_sample (T = 0, no filters)")]
            results.append(S.held_true(f"[mode {mode}] token_sample (T = 0, no filters) returns token_confidence's tok", bool(np.array_equal(t, t2)),
                                       "the two kernels return different tokens"))
            results.append(S.conf_pair_check(key, mode, c2, c))
    finish("token_confidence", key, results)


# ------------------------------------------------------------------------------------------------------------------ unmask_origin
MASK = 1


def _origin(lib, B, N, p, seed, it, rows, x, cand):
    """Runs gget_op_unmask_origin (p a number) or _rows (p fp32 [B]) in place on a copy of x with a sentinel tail; -> the result."""
    tail = 64
    buf = torch.full((B * N + tail,), -7, dtype=I64, device="cuda")
    buf[:B * N] = torch.from_numpy(x.reshape(-1)).cuda()
    cd = torch.from_numpy(cand).cuda()
    s = gen.iteration_seed(seed, it)
    if rows:
        pd = torch.from_numpy(np.asarray(p, np.float32)).cuda()
        L.check(lib.gget_op_unmask_origin_rows(P(buf), P(cd), B, N, P(pd), s, MASK, ST()))
    else:
        L.check(lib.gget_op_unmask_origin(P(buf), P(cd), B, N, float(p), s, MASK, ST()))
    torch.cuda.synchronize()
    assert bool((buf[B * N:] == -7).all()), "wrote behind x"
    return buf[:B * N].view(B, N).cpu().numpy()


@pytest.mark.parametrize("B,N", [(5, 77), (9, 1), (27, 38839)], ids=["B5-N77", "N1", "B27-N38839: 4096 x 256 + 77 cells, past one grid-stride round"])
def test_unmask_origin_edges(lib, B, N):
    rs = np.random.RandomState(B * 1000 + N)
    seed, it = 99, 4
    x = rs.randint(2, 90, (B, N)).astype(np.int64)
    x[rs.rand(B, N) < 0.5] = MASK
    x[0, 0], x[B - 1, N - 1] = MASK, MASK
    cand = rs.randint(100, 190, (B, N)).astype(np.int64)
    u = gen.draws(seed, it, B, N)[2].numpy()
    for rows in (False, True):
        for p in (0.0, 1.0, 0.37):
            pv = np.full(B, p, np.float32)
            got = _origin(lib, B, N, pv if rows else p, seed, it, rows, x, cand)
            want = np.where((x == MASK) & (u < np.float32(p)), cand, x)
            assert np.array_equal(got, want), (rows, p)
            if p == 0.0:
                assert np.array_equal(got, x)                               # nothing changes
            if p == 1.0:
                assert (got[x == MASK] == cand[x == MASK]).all() and np.array_equal(got[x != MASK], x[x != MASK])
    # "finished" samples (p = 0) next to live ones
    pv = np.where(np.arange(B) % 2 == 0, 0.0, 0.8).astype(np.float32)
    got = _origin(lib, B, N, pv, seed, it, True, x, cand)
    assert np.array_equal(got, np.where((x == MASK) & (u < pv[:, None]), cand, x)) and np.array_equal(got[0::2], x[0::2])
    if N > 1:
        assert (got[1::2] != x[1::2]).any()


# ------------------------------------------------------------------------------------------------------------------ smtp_rows
def _smtp_rows(lib, ids, lens, umr_min, umr_max, power, seed):
    B, Sq, F = ids.shape
    out, lab, w = Out(B, Sq * F, I64), Out(B, Sq * F, I64), Out(B, 1, F32)
    idd, ld = torch.from_numpy(ids).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    L.check(lib.gget_op_smtp_rows(P(idd), P(ld), P(out.buf), P(lab.buf), P(w.buf), B, Sq, F, umr_min, umr_max, power, seed, ST()))
    return out.body().numpy().reshape(B, Sq, F), lab.body().numpy().reshape(B, Sq, F), w.body().view(-1).numpy()


def test_smtp_rows_length_edges(lib):
    """Lengths of 0, of S, above S (clamped to S) and negative (clamped to 0), exactly against the twin."""
    B, Sq, F, seed = 6, 24, 5, 777
    rs = np.random.RandomState(5)
    ids = rs.randint(2, 700, (B, Sq, F)).astype(np.int64)
    ids[1, 3, 2] = 0                                     # a pad-valued cell inside a sequence: chosen cells keep the pad id
    lens = np.array([0, Sq, Sq + 9, -3, 7, 1])
    got_ids, got_lab, got_w = _smtp_rows(lib, ids, lens, 0.01, 0.99, 1.0, seed)
    sel = smtp.row_mask_selection(seed, lens, Sq, F)
    for b in range(B):
        idx, alpha, wgt = sel[b]
        n = min(max(int(lens[b]), 0), Sq) * F
        assert len(idx) == int(np.ceil(n * alpha)) and (len(idx) == 0) == (n == 0 or alpha == 0)
        chosen = np.zeros(Sq * F, bool)
        chosen[idx] = True
        flat = ids[b].reshape(-1)
        assert np.array_equal(got_lab[b].reshape(-1), np.where(chosen, flat, -100)), b
        assert np.array_equal(got_ids[b].reshape(-1), np.where(chosen & (flat != 0), 1, flat)), b
        assert abs(float(got_w[b]) - wgt) <= 1e-6 * wgt
    assert np.array_equal(got_ids[0], ids[0]) and np.array_equal(got_ids[3], ids[3]) and (got_lab[[0, 3]] == -100).all()
    assert (got_lab[2] != -100).sum() == len(sel[2][0]) > 0 and len(sel[1][0]) > 0


def test_smtp_rows_masks_nothing_at_mask_ratio_zero(lib):
    """umr_min = umr_max = 1: t = 1, alpha = 0, k = 0 - ids unchanged and every label -100."""
    B, Sq, F, seed = 4, 16, 3, 31
    ids = np.random.RandomState(6).randint(2, 700, (B, Sq, F)).astype(np.int64)
    lens = np.array([Sq, 5, 0, Sq + 2])
    for power in (1.0, 2.0):
        got_ids, got_lab, got_w = _smtp_rows(lib, ids, lens, 1.0, 1.0, power, seed)
        assert all(len(idx) == 0 and alpha == 0.0 for idx, alpha, _ in smtp.row_mask_selection(seed, lens, Sq, F, 1.0, 1.0, power))
        assert np.array_equal(got_ids, ids) and (got_lab == -100).all() and np.array_equal(got_w, np.full(B, power, np.float32))
