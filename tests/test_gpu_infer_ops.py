"""The collection kernels of the prediction passes (csrc/infer.hip) through the C ABI, exact against the NumPy twins of
tests/_infer_ref.py (themselves pinned against torch's CPU `.half()` and a torch statement of `process_data` in tests/test_infer_ref.py).

Geometry: `gget_op_infer_append` is one grid-stride launch of 256-lane workgroups, at most 2048 of them, a lane converting 8 hidden values
(16 bytes in, 16 out) or one logit per round: (1, 1, 0) is a single element without hidden states, (3, 2, 64) less than one workgroup,
(257, 37, 768) odd sizes over many workgroups, (1024, 128, 64) carries every bf16 pattern.  `gget_op_node_records` cuts the B * S
positions into chunks of 1024 (256 lanes x 4 rounds): S = 1, 8, 33, 72 stay inside one chunk with ragged rounds, (4, 256) fills one chunk
exactly, (2, 2048) is four chunks, (512, 2048) the 2^20 bound with 1024 chunks (every lane of the prefix sum owns four chunk counts)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import _infer_ref as R

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")

APPEND_SHAPES = [(1, 1, 0), (3, 2, 64), (64, 5, 128), (257, 37, 768), (1024, 128, 64)]
RECORD_SHAPES = [(1, 1, 2), (2, 8, 3), (5, 33, 1), (3, 72, 5), (4, 256, 2), (2, 2048, 7), (512, 2048, 2)]
LOGIT_CANARY, HIDDEN_CANARY, IDX_CANARY, REC_CANARY = 0x1234, 0x4321, -7, -5


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def u16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def dev_bits16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(dtype).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else None


def append_inputs(B, Cn, d, seed):
    rng = np.random.RandomState(seed)
    lb = rng.randint(0, 2 ** 32, B * Cn, dtype=np.uint64).astype(np.uint32)
    cur = R.CURATED_F32.view(np.uint32)
    lb[:min(len(cur), B * Cn)] = cur[:B * Cn]                     # the curated list first, random bit patterns behind it
    hb = None
    if d:
        hb = rng.randint(0, 2 ** 16, B * d, dtype=np.uint64).astype(np.uint16)
        if B * d == 65536:
            hb = rng.permutation(65536).astype(np.uint16)         # every bf16 pattern once
    idx = rng.randint(-2 ** 40, 2 ** 40, B).astype(np.int64)
    idx[0], idx[-1] = -3, 2 ** 31 + 5
    return lb.reshape(B, Cn), None if hb is None else hb.reshape(B, d), idx


@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("shape", APPEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_infer_append_is_exact_and_stays_in_its_rows(shape, row0):
    B, Cn, d = shape
    lib = L.load()
    lb, hb, idx = append_inputs(B, Cn, d, B * 7 + Cn)
    cap = row0 + B + 3
    logits = torch.from_numpy(lb.view(np.float32)).cuda()
    hidden = dev_bits16(hb, torch.bfloat16) if d else None
    idx_d = torch.from_numpy(idx).cuda()
    out_l = dev_bits16(np.full((cap, Cn), LOGIT_CANARY), torch.float16)
    out_h = dev_bits16(np.full((cap, d), HIDDEN_CANARY), torch.float16) if d else None
    out_i = torch.full((cap,), IDX_CANARY, dtype=torch.int64, device="cuda")
    rc = lib.gget_op_infer_append(ptr(logits), ptr(hidden), ptr(idx_d), ptr(out_l), ptr(out_h), ptr(out_i), row0, cap, B, Cn, d, stream())
    assert rc == 0, lib.gget_last_error()
    torch.cuda.synchronize()
    got_l, got_i = u16(out_l), out_i.cpu().numpy()
    rows = slice(row0, row0 + B)
    assert R.same_f16(got_l[rows], R.f32_to_f16_bits(lb))
    assert np.array_equal(got_i[rows], idx)
    outside = np.ones(cap, dtype=bool)
    outside[rows] = False
    assert (got_l[outside] == LOGIT_CANARY).all() and (got_i[outside] == IDX_CANARY).all()
    # what tensor.half() gives on this device, bit for bit (NaNs as NaNs)
    assert R.same_f16(got_l[rows], u16(logits.half()))
    if d:
        got_h = u16(out_h)
        assert R.same_f16(got_h[rows], R.bf16_to_f16_bits(hb)) and R.same_f16(got_h[rows], u16(hidden.half()))
        assert (got_h[outside] == HIDDEN_CANARY).all()
        if B * d == 65536:
            assert np.array_equal(np.sort(hb.reshape(-1)), np.arange(65536, dtype=np.uint16))


def test_infer_append_refuses_without_a_launch():
    lib = L.load()
    B, Cn, d = 4, 3, 64
    lb, hb, idx = append_inputs(B, Cn, d, 1)
    logits, hidden, idx_d = torch.from_numpy(lb.view(np.float32)).cuda(), dev_bits16(hb, torch.bfloat16), torch.from_numpy(idx).cuda()
    cap = 8
    out_l = dev_bits16(np.full((cap, Cn), LOGIT_CANARY), torch.float16)
    out_h = dev_bits16(np.full((cap, d), HIDDEN_CANARY), torch.float16)
    out_i = torch.full((cap,), IDX_CANARY, dtype=torch.int64, device="cuda")
    good = dict(logits=ptr(logits), hidden=ptr(hidden), idx=ptr(idx_d), out_l=ptr(out_l), out_h=ptr(out_h), out_i=ptr(out_i), row0=0, cap=cap,
                B=B, C=Cn, d=d)
    bad = [dict(row0=5), dict(row0=cap), dict(row0=-1), dict(cap=3), dict(cap=-1), dict(row0=2 ** 40, cap=2 ** 40 + 2),     # rows that do not fit
           dict(logits=None), dict(idx=None), dict(out_l=None), dict(out_i=None), dict(hidden=None), dict(out_h=None),     # null pointers
           dict(B=0), dict(C=0), dict(B=-1),                                                                             # empty shapes
           dict(d=32), dict(d=65), dict(d=-64), dict(d=0),                                                               # unsupported widths
           dict(hidden=ptr(hidden) + 2), dict(out_h=ptr(out_h) + 8)]                                                     # 16-byte alignment
    for change in bad:
        a = dict(good, **change)
        rc = lib.gget_op_infer_append(a["logits"], a["hidden"], a["idx"], a["out_l"], a["out_h"], a["out_i"], a["row0"], a["cap"], a["B"],
                                      a["C"], a["d"], stream())
        assert rc == 2 and lib.gget_last_error(), change
    torch.cuda.synchronize()
    assert (u16(out_l) == LOGIT_CANARY).all() and (u16(out_h) == HIDDEN_CANARY).all() and (out_i.cpu().numpy() == IDX_CANARY).all()
    # d = 0 without hidden states is a valid call; so is a hidden width the caller does not collect
    assert lib.gget_op_infer_append(good["logits"], None, good["idx"], good["out_l"], None, good["out_i"], 4, cap, B, Cn, 0, stream()) == 0
    torch.cuda.synchronize()
    assert (u16(out_l)[:4] == LOGIT_CANARY).all() and R.same_f16(u16(out_l)[4:], R.f32_to_f16_bits(lb)) and (u16(out_h) == HIDDEN_CANARY).all()


# ------------------------------------------------------------------------------------------------ node records
def record_inputs(B, S, Cn, kind, seed):
    rng = np.random.RandomState(seed)
    lg = rng.randn(B, S, Cn).astype(np.float32)
    flat = lg.reshape(-1, Cn)
    n = flat.shape[0]
    if Cn > 1:
        for r in rng.randint(0, n, max(2, min(n // 7, 3000))):             # planted ties: two maximal classes, and a whole row of one value
            a, b = rng.choice(Cn, 2, replace=False)
            flat[r, a] = flat[r, b] = 9.0
        flat[rng.randint(0, n, max(1, min(n // 11, 3000)))] = -0.5
        for r in rng.randint(0, n, max(2, min(n // 9, 3000))):             # NaNs: one, and (C > 2) two of them - the first wins
            flat[r, rng.randint(0, Cn)] = np.nan
            if Cn > 2:
                flat[r, rng.randint(0, Cn)] = np.nan
        flat[0, 0], flat[0, Cn - 1] = 0.0, -0.0                  # signed zeros tie
    raw = rng.randint(0, 2 ** 40, (B, S)).astype(np.int64)
    keep = {"none": np.zeros((B, S), bool), "all": np.ones((B, S), bool), "third": rng.rand(B, S) < 0.34,
            "sparse": rng.rand(B, S) < 1.0 / 97, "last": np.zeros((B, S), bool)}[kind]
    if kind == "last":
        keep[-1, -1] = True
    raw[~keep] = -100
    idx = rng.randint(-2 ** 40, 2 ** 40, B).astype(np.int64)
    return lg, raw, idx


def run_records(out, raw, idx, cap, records=None, state=None):
    """one gget_op_node_records call; `out` f32 [B,S,C] (logits) or i64 [B,S] (pred); the arena carries two canary rows behind cap"""
    lib = L.load()
    B, S = raw.shape
    is_logits = out.ndim == 3
    out_d, raw_d, idx_d = torch.from_numpy(out).cuda(), torch.from_numpy(raw).cuda(), torch.from_numpy(idx).cuda()
    if records is None:
        records = torch.full((cap + 2, 3), REC_CANARY, dtype=torch.int64, device="cuda")
        state = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = lib.gget_op_node_records(ptr(out_d) if is_logits else None, None if is_logits else ptr(out_d), ptr(raw_d), ptr(idx_d), ptr(records),
                                  ptr(state), cap, B, S, out.shape[2] if is_logits else 0, stream())
    torch.cuda.synchronize()
    return rc, records, state


@pytest.mark.parametrize("shape", RECORD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_node_records_are_exact_ordered_and_repeatable(shape):
    B, S, Cn = shape
    big = B * S >= 2 ** 20
    assert B * S <= L.NODE_RECORDS_MAX_POS
    first = None
    for k, kind in enumerate(("sparse", "last", "none") if big else ("none", "all", "third", "last")):
        lg, raw, idx = record_inputs(B, S, Cn, kind, 1000 * k + B + S)
        pred = R.argmax_first(lg)
        assert np.array_equal(pred, torch.argmax(torch.from_numpy(lg), -1).numpy())
        want = R.node_records(pred, raw, idx)
        n = len(want)
        assert n == {"none": 0, "all": B * S, "last": 1}.get(kind, n)
        rc, rec, st = run_records(lg, raw, idx, n)
        assert rc == 0, L.load().gget_last_error()
        got = rec.cpu().numpy()
        assert st.tolist() == [n, 0] and np.array_equal(got[:n], want), (kind, np.argwhere(got[:n] != want)[:4])
        assert (got[n:] == REC_CANARY).all()
        # two runs: identical bytes
        rc2, rec2, st2 = run_records(lg, raw, idx, n)
        assert rc2 == 0 and rec2.cpu().numpy().tobytes() == got.tobytes() and st2.tolist() == st.tolist()
        # the predictions given instead of logits
        rc3, rec3, st3 = run_records(pred, raw, idx, n)
        assert rc3 == 0 and st3.tolist() == [n, 0] and np.array_equal(rec3.cpu().numpy(), got)
        if n >= 3:
            # cap three short: the first cap records, the rest counted, nothing behind cap
            rc4, rec4, st4 = run_records(lg, raw, idx, n - 3)
            g4 = rec4.cpu().numpy()
            assert rc4 == 0 and st4.tolist() == [n - 3, 3] and np.array_equal(g4[:n - 3], want[:n - 3]) and (g4[n - 3:] == REC_CANARY).all()
        if first is None:
            first = (lg, raw, idx, want)
        else:
            # two consecutive calls share one cursor: the second batch's records follow the first's
            lg0, raw0, idx0, want0 = first
            total = len(want0) + n
            rc5, rec5, st5 = run_records(lg0, raw0, idx0, total)
            rc6, rec5, st5 = run_records(lg, raw, idx, total, rec5, st5)
            g5 = rec5.cpu().numpy()
            assert rc5 == 0 and rc6 == 0 and st5.tolist() == [total, 0]
            assert np.array_equal(g5[:total], np.concatenate([want0, want])) and (g5[total:] == REC_CANARY).all()
            if total >= 2:
                # ... and a full arena: the second call writes what fits and counts the rest on top of the first call's count
                cap = len(want0) - 1 if len(want0) >= 1 else 0
                rc7, rec7, st7 = run_records(lg0, raw0, idx0, cap)
                rc8, rec7, st7 = run_records(lg, raw, idx, cap, rec7, st7)
                g7 = rec7.cpu().numpy()
                assert rc7 == 0 and rc8 == 0 and st7.tolist() == [cap, total - cap]
                assert np.array_equal(g7[:cap], want0[:cap]) and (g7[cap:] == REC_CANARY).all()


def test_node_records_refuses_without_a_launch():
    lib = L.load()
    B, S, Cn = 2, 8, 3
    lg, raw, idx = record_inputs(B, S, Cn, "all", 3)
    pred = R.argmax_first(lg)
    lg_d, pred_d, raw_d, idx_d = (torch.from_numpy(a).cuda() for a in (lg, pred, raw, idx))
    rec = torch.full((B * S + 2, 3), REC_CANARY, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    good = dict(logits=ptr(lg_d), pred=None, raw=ptr(raw_d), idx=ptr(idx_d), rec=ptr(rec), st=ptr(st), cap=B * S, B=B, S=S, C=Cn)
    bad = [dict(pred=ptr(pred_d)), dict(logits=None),                       # both inputs, neither
           dict(raw=None), dict(idx=None), dict(rec=None), dict(st=None),   # null pointers
           dict(B=0), dict(S=0), dict(B=-2), dict(C=0), dict(C=-1), dict(cap=-1),
           dict(B=513, S=2048), dict(B=1, S=2 ** 20 + 1), dict(B=2 ** 16, S=2 ** 16)]       # past the 2^20 positions of one call
    for change in bad:
        a = dict(good, **change)
        rc = lib.gget_op_node_records(a["logits"], a["pred"], a["raw"], a["idx"], a["rec"], a["st"], a["cap"], a["B"], a["S"], a["C"], stream())
        assert rc == 2 and lib.gget_last_error(), change
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == REC_CANARY).all() and st.tolist() == [0, 0]
    assert b"1048576" in (lib.gget_op_node_records(good["logits"], None, good["raw"], good["idx"], good["rec"], good["st"], 4, 513, 2048, Cn,
                                                   stream()), lib.gget_last_error())[1]
    # C is not read with predictions given; cap = 0 counts everything
    rc, rec0, st0 = run_records(pred, raw, idx, 0)
    assert rc == 0 and st0.tolist() == [0, B * S] and (rec0.cpu().numpy() == REC_CANARY).all()
