"""The element-wise kernels of a training step, one launcher at a time through the C ABI (gget_op_geglu_fwd / _bwd, gget_op_gateup_geglu,
gget_op_down_dgrad_geglu, gget_op_rope, gget_op_qkv_rope, gget_op_rope_table, gget_op_rope_range_table, gget_op_clamp_positions,
gget_op_embed_fwd, gget_op_embed_long_ratio, gget_op_embed_bwd), every output element against a float64 statement of the same operation on
the same bf16 / fp32 inputs (tests/_elem_ref.py: references, bounds and their derivation).  Outputs land in buffers pre-filled with NaN
sentinels with pad rows behind them; accumulating outputs start from known non-zero values; launch-menu keys are set through L.debug_menu,
which restores them.  The shapes are the smallest that reach each launch form; the form is named next to the case."""
import importlib

import pytest
import torch

import _elem_ref as E
from _gpu_out import Out, P, ST, dev
from _util import record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64


@pytest.fixture(scope="module")
def lib():
    return L.load()


def params(cases):
    return [pytest.param(*args, id=name) for name, args in cases]


def tagged(tag, results):
    return [type(t)((f"[{tag}] {t[0]}", t[1], None if t[2] is None else f"[{tag}] {t[2]}")) for t in results]


def finish(op, case, results):
    """Record max(err / bound) of the case - overall, and per bounded quantity over the case's variants - then fail on whatever was out
    of bound."""
    ratio, msgs = E.settle(results)
    record_error(f"elementwise/{op}", case, ratio, 1.0)
    worst = {}
    for t in results:
        if isinstance(t, E.Bounded):          # (the bit-for-bit and the yes / no checks have no ratio)
            q = t[0].split("] ")[-1]
            worst[q] = max(worst.get(q, 0.0), t[1])
    for q, r in worst.items():
        record_error(f"elementwise/{op}/{q}", case, r, 1.0)
    assert not msgs, f"{op} {case}:\n" + "\n".join(msgs)


# ------------------------------------------------------------------------------------------------------------------ GEGLU
def run_geglu(lib, gu, dh):
    """(h, dgu) of gget_op_geglu_fwd / gget_op_geglu_bwd on device tensors gu [T, 2 ff], dh [T, ff]."""
    T, ff = dh.shape
    h, dgu = Out(T, ff, BF), Out(T, 2 * ff, BF)
    L.check(lib.gget_op_geglu_fwd(P(gu), P(h.buf), T, ff, ST()))
    L.check(lib.gget_op_geglu_bwd(P(gu), P(dh), P(dgu.buf), T, ff, ST()))
    return h.body(), dgu.body()


@pytest.mark.parametrize("T,ff,variants", params(E.GEGLU_CASES))
def test_geglu(lib, request, T, ff, variants):
    results = []
    for v in range(variants):
        i = E.geglu_inputs(T, ff, v)
        gu, dh = dev(i["gu"]), dev(i["dh"])
        h, dgu = run_geglu(lib, gu, dh)
        results += tagged(f"variant {v}", E.geglu_fwd_check(i, h) + E.geglu_bwd_check(i, dgu))
    finish("geglu", request.node.callspec.id, results)


@pytest.mark.parametrize("T,ff", params(E.GEGLU_FUSED_CASES))
def test_geglu_fused_on_exact_preactivations(lib, request, T, ff):
    """gget_op_gateup_geglu with d = 2 ff and wgu = identity, gget_op_down_dgrad_geglu with d = ff and wdown = identity: the GEMM hands
    the exhaustive gate patterns to the epilogue as they are; gu, h, dgu bit for bit what the element-wise kernels give."""
    results = []
    for v in range(2):
        i = E.geglu_inputs(T, ff, v)
        x, dy = dev(i["gu"]), dev(i["dh"])
        wgu, wdown = dev(E.identity_bf16(2 * ff)), dev(E.identity_bf16(ff))      # (named: a device tensor lives as long as its name)
        gu, h = Out(T, 2 * ff, BF), Out(T, ff, BF)
        L.check(lib.gget_op_gateup_geglu(P(x), P(wgu), P(gu.buf), P(h.buf), T, 2 * ff, ff, ST()))
        gu_w = gu.body()
        dgu = Out(T, 2 * ff, BF)
        L.check(lib.gget_op_down_dgrad_geglu(P(dy), P(wdown), P(x), P(dgu.buf), None, T, ff, ff, ST()))
        gu_d = dev(gu_w)
        h2, _ = run_geglu(lib, gu_d, dy)
        _, dgu2 = run_geglu(lib, x, dy)
        j = dict(i, gu=gu_w)
        j.pop("_ref", None)
        res = [E.held_equal("gu of the identity projection is x", gu_w, i["gu"]),
               E.held_bits("fused h is geglu_fwd of the gu written", h.body(), h2),
               E.held_bits("fused dgu is geglu_bwd of gu and dh = dy", dgu.body(), dgu2)]
        results += tagged(f"variant {v}", res + E.geglu_fwd_check(j, h.body()) + E.geglu_bwd_check(i, dgu.body()))
    finish("geglu_fused", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ RoPE
def run_rope(lib, i, x, inverse, D):
    out = Out(i["T"], x.shape[1], BF, x)
    L.check(lib.gget_op_rope(P(out.buf), P(D["cos"]), P(D["sin"]), P(D["pos"]), i["B"], i["S"], i["H"], inverse, ST()))
    return out.body()


@pytest.mark.parametrize("B,S,H,max_pos,positions", params(E.ROPE_CASES))
def test_rope(lib, request, B, S, H, max_pos, positions):
    i = E.rope_case(B, S, H, max_pos, positions)
    D = {k: dev(i[k]) for k in ("cos", "sin", "pos")}
    y = run_rope(lib, i, i["qkv"], 0, D)
    z = run_rope(lib, i, y, 1, D)
    results = (tagged("forward", E.rope_check(i, 0, y)) + tagged("inverse", E.rope_check(i, 1, run_rope(lib, i, i["qkv"], 1, D)))
               + E.rope_roundtrip_check(i, y, z))
    finish("rope", request.node.callspec.id, results)


def test_rope_grid_stride(lib, request):
    name, args = E.ROPE_BIG
    i = E.rope_case(*args)
    assert i["T"] * i["H"] * 8 > 4096 * 256
    D = {k: dev(i[k]) for k in ("cos", "sin", "pos")}
    finish("rope", name, E.rope_check(i, 0, run_rope(lib, i, i["qkv"], 0, D)))


@pytest.mark.parametrize("max_pos", E.TABLE_SIZES)
def test_rope_table(lib, request, max_pos):
    cos, sin = Out(max_pos, 32, F32), Out(max_pos, 32, F32)
    L.check(lib.gget_op_rope_table(P(cos.buf), P(sin.buf), max_pos, E.THETA, ST()))
    finish("rope_table", f"max_pos {max_pos}", E.table_check(cos.body(), sin.body(), max_pos, E.THETA))


@pytest.mark.parametrize("B,S", params(E.RANGE_CASES))
def test_rope_range_table(lib, request, B, S):
    i = E.range_inputs(B, S, seed=B + S)
    cos, sin, ids, pos = Out(B * S, 32, F32), Out(B * S, 32, F32), Out(B * S, 1, I64), dev(i["pos"])
    L.check(lib.gget_op_rope_range_table(P(pos), P(cos.buf), P(sin.buf), P(ids.buf), B, S, i["range"], i["theta"], ST()))
    finish("rope_range_table", request.node.callspec.id, E.range_check(i, cos.body(), sin.body(), ids.body()))


def test_clamp_positions(lib):
    n, max_pos = 300_000, 64            # (past the 1024 x 256 grid: a second grid-stride trip)
    results = []
    for clamped in (False, True):
        for flag0 in (0, 1):
            pos = E.clamp_inputs(n, max_pos, clamped, 5)
            out, flag, pos_d = Out(n, 1, I64), torch.tensor([flag0, 77], dtype=torch.int32, device="cuda"), dev(pos)
            L.check(lib.gget_op_clamp_positions(P(pos_d), P(out.buf), P(flag), n, max_pos, ST()))
            f = flag.cpu()
            assert int(f[1]) == 77
            results += tagged(f"{'clamped' if clamped else 'in range'}, flag preset {flag0}", E.clamp_check(pos, max_pos, flag0, out.body().view(-1), f[0]))
    finish("clamp_positions", "n300000-max_pos64", results)


@pytest.mark.parametrize("B,S,d,positions", params(E.QKV_ROPE_CASES))
def test_qkv_rope_on_exact_accumulators(lib, request, B, S, d, positions):
    """wqkv = three stacked d x d identities: the accumulators hold x, so the epilogue's q and k thirds meet gget_op_rope's bound on
    (x | x | x) and the v third is x bit for bit."""
    H = d // 64
    i = E.rope_case(B, S, H, 128, positions)
    x = i["qkv"][:, :d].contiguous()
    i = dict(i, qkv=torch.cat([x, x, x], dim=1))
    qkv = Out(i["T"], 3 * d, BF)
    D = {k: dev(v) for k, v in dict(x=x, w=E.identity_bf16(d, 3), cos=i["cos"], sin=i["sin"], pos=i["pos"]).items()}
    L.check(lib.gget_op_qkv_rope(P(D["x"]), P(D["w"]), P(qkv.buf), P(D["cos"]), P(D["sin"]), P(D["pos"]), i["T"], S, d, ST()))
    finish("qkv_rope", request.node.callspec.id, E.rope_check(i, 0, qkv.body()))


# ------------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("T,F,ldF,d,V,gated", params(E.EMBED_FWD_CASES))
def test_embed_fwd(lib, request, T, F, ldF, d, V, gated):
    i = E.embed_fwd_case(T, F, ldF, d, V, gated)
    out = Out(T, d, BF)
    D = {k: dev(i[k]) for k in ("ids", "emb", "gate")}
    L.check(lib.gget_op_embed_fwd(P(D["ids"]), P(D["emb"]), P(D["gate"]), P(out.buf), T, F, ldF, d, ST()))
    finish("embed_fwd", request.node.callspec.id, E.embed_fwd_check(i, out.body()))


@pytest.mark.parametrize("T,F,ldF,d", params(E.LONG_CASES))
def test_embed_long_ratio(lib, request, T, F, ldF, d):
    i = E.long_inputs(T, F, ldF, d, seed=T + F + d)
    x, ids = Out(T, d, BF, i["x"]), dev(i["ids"])
    L.check(lib.gget_op_embed_long_ratio(P(ids), P(x.buf), T, F, ldF, d, ST()))
    finish("embed_long_ratio", request.node.callspec.id, E.long_check(i, x.body()))


def run_embed_bwd(lib, i, D):
    demb = Out(i["V"], i["d"], F32, i["demb0"])
    dgate = Out(i["F"], i["d"], F32, i["dgate0"]) if i["gate"] is not None else None
    L.check(lib.gget_op_embed_bwd(P(D["ids"]), P(D["dx"]), P(D["emb"]), P(D["gate"]), P(demb.buf), P(dgate.buf) if dgate else None,
                                  i["T"], i["F"], i["ldF"], i["d"], i["V"], i["pad_id"], ST()))
    return demb.body(), dgate.body() if dgate else None


@pytest.mark.parametrize("T,F,ldF,d,V,pad_id,gated,layout", params(E.EMBED_SORTED_CASES))
def test_embed_bwd_sorted(lib, request, T, F, ldF, d, V, pad_id, gated, layout):
    """The sorted scatter-add: LDS histogram (V <= 8192) or ballot form; gated or V > 1024, so the count-matrix form is not taken."""
    i = E.embed_bwd_case(T, F, ldF, d, V, pad_id, gated, layout)
    assert gated or V > 1024
    D = {k: dev(i[k]) for k in ("ids", "dx", "emb", "gate")}
    results = E.embed_bwd_check(i, *run_embed_bwd(lib, i, D))
    if layout == "pad-only":
        results.append(E.held_equal("a batch of pad ids changes nothing", run_embed_bwd(lib, i, D)[0], i["demb0"]))
    finish("embed_bwd_sorted", request.node.callspec.id, results)


@pytest.mark.parametrize("T,F,ldF,d,V,pad_id,gated,layout", params(E.EMBED_BOTH_CASES))
def test_embed_bwd_both_forms(lib, request, T, F, ldF, d, V, pad_id, gated, layout):
    """Un-gated V <= 1024: the count-matrix product (KEY_EMBED_SORTED = 0) and the sorted scatter-add (= 1) on the same inputs, each
    against the one float64 reference."""
    i = E.embed_bwd_case(T, F, ldF, d, V, pad_id, gated, layout)
    D = {k: dev(i[k]) for k in ("ids", "dx", "emb", "gate")}
    results = []
    for key in (0, 1):
        with L.debug_menu({L.KEY_EMBED_SORTED: key}):
            demb, dgate = run_embed_bwd(lib, i, D)
        results += tagged("sorted" if key else "dense", E.embed_bwd_check(i, demb, dgate, dense=not key))
    finish("embed_bwd_both", request.node.callspec.id, results)


# ------------------------------------------------------------------------------------------------------------------ argument guards
def refused(lib, rc, name, *outs):
    assert rc != 0, f"{name}: the bad arguments were accepted"
    assert name.encode() in lib.gget_last_error(), (name, lib.gget_last_error())
    for o in outs:
        assert o.untouched(), f"{name}: an output was written although the call was refused"


def test_bad_shapes_are_refused_before_any_launch(lib):
    T, ff, d, F, V = 4, 16, 16, 3, 11
    gu, dh = torch.zeros(T, 2 * ff, dtype=BF, device="cuda"), torch.zeros(T, ff, dtype=BF, device="cuda")
    h, dgu = Out(T, ff, BF), Out(T, 2 * ff, BF)
    for bad_ff in (12, 0, -8):
        refused(lib, lib.gget_op_geglu_fwd(P(gu), P(h.buf), T, bad_ff, ST()), "geglu_fwd", h)
        refused(lib, lib.gget_op_geglu_bwd(P(gu), P(dh), P(dgu.buf), T, bad_ff, ST()), "geglu_bwd", dgu)
    refused(lib, lib.gget_op_geglu_fwd(None, P(h.buf), T, ff, ST()), "geglu_fwd", h)
    refused(lib, lib.gget_op_geglu_bwd(P(gu), None, P(dgu.buf), T, ff, ST()), "geglu_bwd", dgu)
    ids = torch.ones(T, F + 1, dtype=I64, device="cuda")
    emb, x = torch.zeros(V, d, dtype=BF, device="cuda"), torch.zeros(T, d, dtype=BF, device="cuda")
    out, xo, demb = Out(T, d, BF), Out(T, d, BF), Out(V, d, F32)
    for bd, bF, bld in ((12, F, F + 1), (0, F, F + 1), (d, 0, F + 1), (d, F, F - 1)):
        refused(lib, lib.gget_op_embed_fwd(P(ids), P(emb), None, P(out.buf), T, bF, bld, bd, ST()), "embed_fwd", out)
        refused(lib, lib.gget_op_embed_long_ratio(P(ids), P(xo.buf), T, bF, bld, bd, ST()), "embed_long_ratio", xo)
        for sorted_form in (0, 1):
            with L.debug_menu({L.KEY_EMBED_SORTED: sorted_form}):
                refused(lib, lib.gget_op_embed_bwd(P(ids), P(x), P(emb), None, P(demb.buf), None, T, bF, bld, bd, V, 0, ST()), "embed_bwd", demb)
    refused(lib, lib.gget_op_embed_bwd(P(ids), P(x), P(emb), None, P(demb.buf), None, T, F, F + 1, d, 0, 0, ST()), "embed_bwd", demb)
    refused(lib, lib.gget_op_embed_bwd(P(ids), P(x), P(emb), P(emb), P(demb.buf), None, T, F, F + 1, d, V, 0, ST()), "embed_bwd", demb)   # gate, no dgate
    refused(lib, lib.gget_op_embed_fwd(None, P(emb), None, P(out.buf), T, F, F + 1, d, ST()), "embed_fwd", out)
    cos, sin = torch.zeros(8, 32, device="cuda"), torch.zeros(8, 32, device="cuda")
    qkv = Out(4, 3 * 64, BF)
    refused(lib, lib.gget_op_rope(P(qkv.buf), P(cos), P(sin), None, 2, 2, 0, 0, ST()), "rope", qkv)
    refused(lib, lib.gget_op_rope(P(qkv.buf), P(cos), P(sin), None, 2, 0, 1, 0, ST()), "rope", qkv)
    refused(lib, lib.gget_op_rope(P(qkv.buf), None, P(sin), None, 2, 2, 1, 0, ST()), "rope", qkv)
