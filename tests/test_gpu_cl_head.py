"""The contrastive pre-training head, one operator at a time through the C ABI (gget_op_cl_embed_fwd, gget_op_cl_loss_fwd,
gget_op_cl_bwd): every output element against the float64 statement of the same operation on the same inputs (tests/_cl_ref.py:
references, bounds and their derivation).  Outputs land in buffers pre-filled with NaN sentinels with pad rows behind them; the
accumulating outputs (dW, the pooled rows of dhidden) start from known non-zero values.  The cases: one pair; partial blocks of query
rows; several workgroups at the base width; the widest d with more rows than a wave pass; a gathered matrix with the local rows at
interleaved positions."""
import importlib

import pytest
import torch

import _cl_ref as R
from _gpu_out import Out, P, ST, dev
from _heads_ref import settle
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
ALL = [n for n, _ in R.CASES] + [R.GATHERED[0]]


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def cases():
    return {n: R.case(n) for n in ALL}


def finish(op, case, results):
    ratio, msgs = settle(results)
    record_error(f"cl_head_elementwise/{op}", case, ratio, 1.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


def run_embed(lib, i, d_in):
    B, d = i["B"], i["d"]
    z, e, rn = Out(B, d, torch.float32), Out(B, d, torch.float32), Out(1, B, torch.float32)
    L.check(lib.gget_op_cl_embed_fwd(P(d_in["hidden"]), P(d_in["pool_row"]), P(d_in["w"]), P(z.buf), P(e.buf), P(rn.buf), B, d, ST()))
    return z.body(), e.body(), rn.body().view(-1)


def run_loss(lib, i, d_in):
    N, d = i["N"], i["d"]
    stat, loss = Out(3, N, torch.float32), Out(1, 1, torch.float32)
    L.check(lib.gget_op_cl_loss_fwd(P(d_in["E"]), N, d, R.RATIO, P(stat.buf), P(loss.buf), ST()))
    return stat.body(), loss.body().view(())


def run_bwd(lib, i, d_in):
    N, B, d = i["N"], i["B"], i["d"]
    dz, dw = Out(B, d, torch.float32), Out(d, d, torch.float32, i["dw0"])
    dh = Out(i["rows"], d, torch.bfloat16, i["dh0"])
    L.check(lib.gget_op_cl_bwd(P(d_in["E"]), P(d_in["stat"]), P(d_in["row_map"]), P(d_in["rnorm"]), P(d_in["hidden"]), P(d_in["pool_row"]),
                               P(d_in["w"]), i["scale"], P(dz.buf), P(dw.buf), P(dh.buf), N, B, d, ST()))
    return dz.body(), dw.body(), dh.body()


def on_device(i):
    return {k: dev(i[k]) for k in ("hidden", "pool_row", "w", "E", "stat", "row_map", "rnorm")}


@pytest.mark.parametrize("name", ALL)
def test_cl_head_elementwise(lib, cases, name):
    i = cases[name]
    d_in = on_device(i)
    finish("embed_fwd", name, R.embed_check(i, *run_embed(lib, i, d_in)))
    finish("loss_fwd", name, R.loss_check(i, *run_loss(lib, i, d_in)))
    finish("bwd", name, R.bwd_check(i, *run_bwd(lib, i, d_in)))


@pytest.mark.parametrize("name", ["N64_d768", R.GATHERED[0]])
def test_cl_head_second_call_same_bits(lib, cases, name):
    """No atomics and a fixed order in every sum: two calls agree bit for bit, also in the reproducible mode of the launch menu."""
    i = cases[name]
    d_in = on_device(i)
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        first = run_embed(lib, i, d_in) + run_loss(lib, i, d_in) + run_bwd(lib, i, d_in)
        second = run_embed(lib, i, d_in) + run_loss(lib, i, d_in) + run_bwd(lib, i, d_in)
    for k, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), f"output {k} differs between two calls"


def test_cl_head_rejects_unsupported_shapes(lib, cases):
    """d % 64 != 0, d > 1024, N odd, N = 0 and N > 2048 return error 2 without a launch: the outputs keep their sentinels."""
    i = cases["N6_d128"]
    d_in = on_device(i)
    big = torch.zeros(2050 * 128, device="cuda")       # (enough memory behind every pointer for the shapes named, were one launched)
    stat, loss, z = Out(3, 2050, torch.float32), Out(1, 1, torch.float32), Out(8, 1088, torch.float32)
    dz, dw, dh = Out(8, 1088, torch.float32), Out(8, 1088, torch.float32), Out(i["rows"], 1088, torch.bfloat16)

    def refused(rc):
        assert rc == 2 and b"unsupported" in lib.gget_last_error(), (rc, lib.gget_last_error())

    for d in R.BAD_D:
        refused(lib.gget_op_cl_embed_fwd(P(big), P(d_in["pool_row"]), P(big), P(z.buf), P(z.buf), P(z.buf), 2, d, ST()))
        refused(lib.gget_op_cl_loss_fwd(P(big), 6, d, R.RATIO, P(stat.buf), P(loss.buf), ST()))
        refused(lib.gget_op_cl_bwd(P(big), P(big), None, P(big), P(big), P(d_in["pool_row"]), P(big), 1.0, P(dz.buf), P(dw.buf), P(dh.buf),
                                   6, 2, d, ST()))
    for N in R.BAD_N:
        refused(lib.gget_op_cl_loss_fwd(P(big), N, 128, R.RATIO, P(stat.buf), P(loss.buf), ST()))
        refused(lib.gget_op_cl_bwd(P(big), P(big), None, P(big), P(big), P(d_in["pool_row"]), P(big), 1.0, P(dz.buf), P(dw.buf), P(dh.buf),
                                   N, 2, 128, ST()))
    for o in (stat, loss, z, dz, dw, dh):
        assert o.untouched()
