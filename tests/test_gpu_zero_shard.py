"""The sharded optimizer step (ZeRO stage 2) on the device: the ABI-level step against gget_adamw_step with injected gradients, the
loopback schedule of W = 2 / 4 / 8 ranks against world 1, the real one-rank RCCL communicator, and two / eight ranks on cuda:0 over
gloo against the replicated step.  Every comparison across runs uses the reproducible mode (GGET_DETERMINISTIC=1)."""
import importlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")


def _mods():
    return (importlib.import_module("graph-gpt_amd.modeling"), importlib.import_module("graph-gpt_amd.training"),
            importlib.import_module("graph-gpt_amd.synth"))


def _cfg(modeling):
    return modeling.GraphGPTConfig(hidden_act="gelu", vocab_size=756, hidden_size=128, intermediate_size=512, num_hidden_layers=2,
                                   num_attention_heads=2, max_position_embeddings=1024, causal_attention=False,
                                   stacked_feat=13, next_n_token=13)


def _batch(synth, rank, layout="padded"):
    b = synth.make_pretrain_batch(B=8, S=32, F=13, V=756, seed=700 + rank)
    d = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}
    if layout == "varlen":
        d["num_tokens"] = int(b["attention_mask"].sum())
    return d


def _state(e):
    torch.cuda.synchronize()
    return {k: getattr(e, a).detach().float().cpu().numpy().copy()
            for k, a in (("master", "master"), ("m", "adam_m"), ("v", "adam_v"), ("P", "param_bf16"))}


@pytest.fixture
def reproducible():
    with L.debug_menu({L.KEY_DETERMINISTIC: 1}):
        yield


def test_abi_sharded_step_world1_equals_replicated_step(reproducible):
    """Injected gradients, world 1: without clipping the sharded step is bit-identical to gget_adamw_step (one device function per
    element); with clipping the norm (another summation order) is within 1e-6 and the weights follow."""
    eng_mod = importlib.import_module("graph-gpt_amd.engine")
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("tiny", vocab_size=756, stacked_feat=13, next_n_token=13)
    state = importlib.import_module("graph-gpt_amd.weights").make_state_dict(spec, seed=7, std=0.05, head_std=0.1)
    for clip in (0.0, 0.05):
        a, b = (eng_mod.Engine(spec, max_tokens=256, max_batch=8) for _ in range(2))
        a.load_state_dict(state)
        b.load_state_dict(state)
        b.shard_init(1, 0)
        gen = torch.Generator(device="cuda").manual_seed(3)
        for step in range(3):
            g = (torch.randn(a.n_params, generator=gen, device="cuda") * 0.01).to(torch.bfloat16)
            for e in (a, b):
                for k, p in e.params.items():      # (gaps between the parameters stay zero)
                    e.view(k, "grad").copy_(g[p["offset"]: p["offset"] + p["numel"]].view(p["shape"]))
            na = float(a.adamw_step(1e-3, max_grad_norm=clip))
            b.shard_sqnorm_partials()
            nb = float(b.adamw_step_sharded(1e-3, max_grad_norm=clip))
            assert abs(na - nb) <= 1e-6 * na
            sa, sb = _state(a), _state(b)
            for k in sa:
                if clip == 0.0:
                    np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{k} step {step}")
                else:
                    np.testing.assert_allclose(sa[k], sb[k], rtol=1e-4, atol=1e-6, err_msg=f"{k} step {step}")
        assert not b.shard_stale


def test_shard_bucket_without_a_plan_is_an_error():
    """gget_shard_bucket reads the ACTIVE plan: before gget_shard_init, and after the plan is switched off, it returns an error and a
    message and leaves `out` alone"""
    import ctypes as C
    spec = importlib.import_module("graph-gpt_amd.spec").spec_from_size("tiny", vocab_size=756, stacked_feat=13, next_n_token=13, gated_agg=True)
    e = importlib.import_module("graph-gpt_amd.engine").Engine(spec, max_tokens=256, max_batch=8)
    out = (C.c_uint64 * 5)(7, 7, 7, 7, 7)
    for _ in range(2):
        assert e.lib.gget_shard_bucket(e.h, 0, out) != 0
        assert b"no plan is active" in e.lib.gget_last_error()
        assert list(out) == [7] * 5
        e.shard_init(1, 0)
        assert e.lib.gget_shard_bucket(e.h, 0, out) == 0 and tuple(out) == e.shard_buckets[0]
        assert e.lib.gget_shard_bucket(e.h, len(e.buckets), out) != 0 and b"out of range" in e.lib.gget_last_error()
        e.shard_init(0, 0)
        out = (C.c_uint64 * 5)(7, 7, 7, 7, 7)


def _loop_run(monkeypatch, world, zero, clip=0.05, k=1, backend="abi", fp32="0"):
    modeling, tr, synth = _mods()
    monkeypatch.setenv("GGET_DP_BACKEND", backend)
    monkeypatch.setenv("GGET_DP_LOOPBACK_WORLD", str(world) if backend == "abi" and world else "0")
    monkeypatch.setenv("GGET_FORCE_STAGED", "1")
    monkeypatch.setenv("GGET_ZERO_STAGE", str(zero))
    monkeypatch.setenv("GGET_DP_FP32_REDUCE", fp32)
    model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
    eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, max_grad_norm=clip, gradient_accumulation_steps=k))
    assert eng.sharded == (zero > 0)
    norms, states = [], []
    for s in range(3 * k):
        tr.batch_training(_batch(synth, s % 2), eng)
        if (s + 1) % k == 0:
            norms.append(float(eng.last_grad_norm))
            states.append(_state(model._engine))
    info = eng.describe_dp()
    e = model._engine
    if e.comm_world:
        e.comm_destroy()
    return norms, states, info


def test_loopback_worlds_equal_world1_sharded(monkeypatch, reproducible):
    """Loopback W = 2 / 4 / 8 (the schedule of a W-rank job: W x the gradients, 1/W in AdamW, W body slices per bucket) over three steps:
    master, m, v, P and the norm bit-identical to the world-1 sharded step (the norm's chunk grid does not depend on W)."""
    ref_n, ref_s, _ = _loop_run(monkeypatch, 1, 2)
    for W in (2, 4, 8):
        n, s, info = _loop_run(monkeypatch, W, 2)
        assert info["optimizer"] == "sharded" and info["zero_stage"] == 2
        assert info["owned_elements"]["body"] > 0, "the test model must have non-empty bucket bodies"
        assert n == ref_n, (W, n, ref_n)
        for step in range(3):
            for key in ref_s[step]:
                np.testing.assert_array_equal(s[step][key], ref_s[step][key], err_msg=f"W={W} step {step} {key}")


def test_sharded_accumulation_matches_replicated_without_clipping(monkeypatch, reproducible):
    """k = 2 gradient accumulation on a loopback world of 2: the sharded step equals the replicated one bit for bit with clipping off."""
    _, rep, _ = _loop_run(monkeypatch, 2, 0, clip=0.0, k=2)
    _, sh, _ = _loop_run(monkeypatch, 2, 2, clip=0.0, k=2)
    for step in range(3):
        for key in rep[step]:
            np.testing.assert_array_equal(sh[step][key], rep[step][key], err_msg=f"step {step} {key}")


def test_one_rank_rccl_communicator_reproduces_world1_sharded(monkeypatch, reproducible):
    """The real RCCL path of the C ABI (reduce-scatter + tail all-reduce in one group, the partial-vector and weight all-gathers), one
    rank with GGET_FORCE_STAGED=1, bf16 and fp32 reduction: the world-1 sharded step of the loopback, bit for bit."""
    ref_n, ref_s, _ = _loop_run(monkeypatch, 1, 2)
    for fp32 in ("0", "1"):
        n, s, info = _loop_run(monkeypatch, 0, 2, fp32=fp32)
        assert info["optimizer"] == "sharded" and info["backend"] == "rccl-via-c-abi"
        assert n == ref_n
        for step in range(3):
            for key in ref_s[step]:
                np.testing.assert_array_equal(s[step][key], ref_s[step][key], err_msg=f"fp32={fp32} step {step} {key}")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, overlap, layout, runs, tmp):
    os.environ["GGET_DP_OVERLAP"] = overlap
    os.environ["GGET_VARLEN"] = "0" if layout == "padded" else ""
    os.environ["GGET_DETERMINISTIC"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="env://")
    modeling, tr, synth = _mods()
    L.check(L.load().gget_debug_set(L.KEY_DETERMINISTIC, 1))
    out = {}
    for zero, clip in runs:
        model = modeling.GraphGPTPretrainBase(_cfg(modeling), seed=1)
        eng = tr.initialize(model, tr.OptimConfig(lr=1e-3, max_grad_norm=clip, zero_stage=zero))
        assert eng.sharded == (zero > 0) and eng.world == world
        data = _batch(synth, rank, layout)
        ps = []
        for _ in range(3):
            tr.batch_training(data, eng)
            model._engine.await_params()
            ps.append(model._engine.param_bf16.float().cpu().numpy())
        norm = float(eng.last_grad_norm)
        e = model._engine
        refused = None
        if zero:
            assert e.shard_stale
            refused = 0
            try:
                eng.save_checkpoint(os.path.join(tmp, f"r{rank}"))
            except RuntimeError:
                refused += 1
            try:
                model.state_dict()
            except RuntimeError:
                refused += 1
            eng.consolidate()
            assert not e.shard_stale
            if rank == 0 and clip == 0.0:
                eng.save_checkpoint(os.path.join(tmp, "sharded"))
        elif rank == 0 and clip == 0.0:
            eng.save_checkpoint(os.path.join(tmp, "replicated"))
        st = _state(e)
        out[(zero, clip)] = dict(P=ps, norm=norm, refused=refused, **{k: st[k] for k in ("master", "m", "v")})
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, overlap, layout, runs, tmp):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, overlap, layout, runs, str(tmp))) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda t: t[0])
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    return [r[1] for r in res]


@pytest.mark.parametrize("overlap,layout", [("1", "padded"), ("0", "padded"), ("1", "varlen")])
def test_two_ranks_gloo_sharded_equals_replicated(overlap, layout, tmp_path):
    """Two ranks on cuda:0 over gloo: P identical across ranks after every step; after consolidate() master, m and v identical across
    ranks; with clipping off bit-identical to the replicated two-rank step (a bf16 sum of two values does not depend on order), with
    clipping at 0.05 within 1e-6; save_checkpoint and state_dict refuse before the consolidation, and the files written after it hold
    the replicated run's weights."""
    res = _spawn(2, overlap, layout, [(0, 0.0), (2, 0.0), (0, 0.05), (2, 0.05)], tmp_path)
    for key in [(2, 0.0), (2, 0.05)]:
        for s in range(3):
            np.testing.assert_array_equal(res[0][key]["P"][s], res[1][key]["P"][s])
        for k in ("master", "m", "v"):
            np.testing.assert_array_equal(res[0][key][k], res[1][key][k])
        assert res[0][key]["refused"] == 2 and res[1][key]["refused"] == 2
    for r in range(2):
        sh, rep = res[r][(2, 0.0)], res[r][(0, 0.0)]
        for s in range(3):
            np.testing.assert_array_equal(sh["P"][s], rep["P"][s])
        for k in ("master", "m", "v"):
            np.testing.assert_array_equal(sh[k], rep[k])
        sh, rep = res[r][(2, 0.05)], res[r][(0, 0.05)]
        assert abs(sh["norm"] - rep["norm"]) <= 1e-6 * rep["norm"]
        np.testing.assert_allclose(sh["master"], rep["master"], rtol=1e-4, atol=1e-6)
    a = torch.load(tmp_path / "sharded" / "model.pt")
    b = torch.load(tmp_path / "replicated" / "model.pt")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    oa = torch.load(tmp_path / "sharded" / "optimizer.pt")
    ob = torch.load(tmp_path / "replicated" / "optimizer.pt")
    assert all(torch.equal(oa[w][k], ob[w][k]) for w in ("m", "v") for k in oa[w]) and oa["step"] == ob["step"]


def test_eight_ranks_gloo_sharded_state_identical(tmp_path):
    """Eight ranks on cuda:0 over gloo: P after every step and the consolidated fp32 state identical on every rank."""
    res = _spawn(8, "1", "padded", [(2, 0.05)], tmp_path)
    key = (2, 0.05)
    for r in range(1, 8):
        for s in range(3):
            np.testing.assert_array_equal(res[0][key]["P"][s], res[r][key]["P"][s])
        for k in ("master", "m", "v"):
            np.testing.assert_array_equal(res[0][key][k], res[r][key][k])
        assert res[r][key]["norm"] == res[0][key]["norm"]
