"""The intra-instance token head (loss_type = "token_ce_intra"), one kernel launcher at a time through the C ABI (gget_op_tok_intra_fwd,
gget_op_tok_intra_bwd), every output element against the float64 statement of tests/_intra_ref.py on the same bf16 inputs (references,
bounds and their derivation are there; tests/test_intra_ref.py holds them to a correct fp32 statement and to planted faults).  Outputs
land in buffers pre-filled with NaN sentinels with pad rows behind them, in the style of tests/test_gpu_heads.py; the rows in front of
the first sample of the padded layout belong to no sample and must keep their sentinel."""
import ctypes as C
import importlib

import pytest
import torch

import _heads_ref as H
import _intra_ref as R
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")

SENT16 = 0x7FC1                      # bf16 NaN payload no kernel writes (as tests/test_gpu_heads.py)
SENT32 = 0x7FC01234                  # fp32 NaN payload
PAD_ROWS = 8


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    return L.load()


class Out:
    """[rows, cols] output of bf16 or fp32 filled with the NaN sentinel, PAD_ROWS more rows behind it."""

    def __init__(self, rows, cols, dtype):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        n = (rows + PAD_ROWS) * cols
        if dtype == torch.bfloat16:
            self.buf = torch.full((n,), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        else:
            self.buf = torch.full((n,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)

    def _intact(self, part):
        if self.dtype == torch.bfloat16:
            return bool((part.view(torch.int16) == SENT16).all())
        return bool((part.view(torch.int32) == SENT32).all())

    def body(self, lead=0):
        """The body on the CPU, after checking that nothing was written behind it or into its first `lead` rows."""
        torch.cuda.synchronize()
        assert self._intact(self.buf[self.rows * self.cols:]), f"wrote behind the {self.rows} x {self.cols} output"
        assert self._intact(self.buf[:lead * self.cols]), f"wrote into the {lead} rows in front of the first sample"
        return self.buf[:self.rows * self.cols].view(self.rows, self.cols).cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return self._intact(self.buf)


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def finish(op, case, results):
    """Record max(err / bound) of the case, then fail on whatever was out of bound."""
    ratio, msgs = H.settle(results)
    record_error(f"heads_elementwise/{op}", case, ratio, 1.0)
    print(f"heads_elementwise/{op} {case}: max err / bound = {ratio:.4f}")
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


def on_device(i):
    return i["hidden"].cuda(), i["row_start"].cuda(), i["cls_idx"].cuda(), i["dl"].cuda()


@pytest.mark.parametrize("d,Cn,lens,padded,place", params(R.INTRA_CASES))
def test_tok_intra_head(lib, request, d, Cn, lens, padded, place):
    i = R.intra_case(d, Cn, lens, padded, place)
    case = request.node.callspec.id
    lead = R.LEAD if padded else 0
    hidden, row_start, cls_idx, dl = on_device(i)       # (held in names: a freed block is reused)
    logits = Out(i["rows"], Cn, torch.float32)
    L.check(lib.gget_op_tok_intra_fwd(P(hidden), P(row_start), P(cls_idx), P(logits.buf), i["B"], Cn, d, ST()))
    finish("tok_intra_fwd", case, R.intra_fwd_check(i, logits.body(lead)))
    # backward with 1 / n = 1 / 64 (bf16(dl / n) is exact in the reference), twice: no atomics, the same bits; then with no labelled row
    stat = torch.tensor([123.0, 64.0, R.INV_N, 0.0], device="cuda")
    runs = []
    for _ in range(2):
        dh = Out(i["rows"], d, torch.bfloat16)
        L.check(lib.gget_op_tok_intra_bwd(P(dl), P(stat), P(hidden), P(row_start), P(cls_idx), P(dh.buf), i["B"], Cn, d, ST()))
        runs.append(dh.body(lead))
    finish("tok_intra_bwd", case, R.intra_bwd_check(i, R.INV_N, runs[0]))
    assert torch.equal(runs[0][lead:].view(torch.int16), runs[1][lead:].view(torch.int16)), "two backward runs differ"
    stat0 = torch.tensor([0.0, 0.0, 0.0, 0.0], device="cuda")
    dh = Out(i["rows"], d, torch.bfloat16)
    L.check(lib.gget_op_tok_intra_bwd(P(dl), P(stat0), P(hidden), P(row_start), P(cls_idx), P(dh.buf), i["B"], Cn, d, ST()))
    finish("tok_intra_bwd", case + " stat[2] = 0", R.intra_bwd_check(i, 0.0, dh.body(lead)))


def test_tok_intra_all_zero_hidden_row(lib):
    """F.normalize divides by max(|h|, 1e-12): an all-zero row has finite, zero logits (forward only), as an ordinary row and as a label
    row (then its column is zero for every row of the sample); the other logits keep their bounds."""
    i = R.intra_case(768, 5, (6, 13, 67, 1024), True, "last")
    rs, k = i["row_start"].tolist(), i["cls_idx"].tolist()
    plain, label = rs[2] + 1, rs[3] + k[3] + 2         # row 1 of the third sample, label row 2 of the fourth
    i["hidden"][plain] = 0
    i["hidden"][label] = 0
    hidden, row_start, cls_idx, _ = on_device(i)
    logits = Out(i["rows"], 5, torch.float32)
    L.check(lib.gget_op_tok_intra_fwd(P(hidden), P(row_start), P(cls_idx), P(logits.buf), i["B"], 5, 768, ST()))
    got = logits.body(R.LEAD)
    assert bool((got[plain] == 0).all()) and bool((got[rs[3]:rs[4], 2] == 0).all())
    finish("tok_intra_fwd", "d768-C5 with two all-zero rows", R.intra_fwd_check(i, got))


def test_tok_intra_rejects_unsupported_shapes(lib):
    """d % 64 != 0, d > 1024, C < 2 and C > 64 are refused with the error code; nothing is launched, the outputs stay untouched."""
    for d, Cn in ((96, 5), (1088, 5), (128, 1), (128, 65)):
        n = Cn + 3
        hidden = H.randn_bf16(H.gen(9), 2 * n, d).cuda()
        row_start = torch.tensor([0, n, 2 * n], dtype=torch.int32, device="cuda")
        cls_idx = torch.tensor([0, 3], dtype=torch.int64, device="cuda")
        dl, stat = torch.randn(2 * n, Cn, device="cuda"), torch.tensor([1.0, 64.0, R.INV_N, 0.0], device="cuda")
        logits, dh = Out(2 * n, Cn, torch.float32), Out(2 * n, d, torch.bfloat16)
        rc = lib.gget_op_tok_intra_fwd(P(hidden), P(row_start), P(cls_idx), P(logits.buf), 2, Cn, d, ST())
        assert rc == 2 and b"unsupported" in lib.gget_last_error(), (d, Cn, rc, lib.gget_last_error())
        rc = lib.gget_op_tok_intra_bwd(P(dl), P(stat), P(hidden), P(row_start), P(cls_idx), P(dh.buf), 2, Cn, d, ST())
        assert rc == 2 and b"unsupported" in lib.gget_last_error(), (d, Cn, rc, lib.gget_last_error())
        assert logits.untouched() and dh.untouched()
