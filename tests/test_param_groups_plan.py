"""The work lists of a grouped optimizer step, without a device: gget_group_plan on the tiny (d128 / L2) model and the 2-layer d768
model of tests/test_gpu_adamw_exact.py, for frozen_layers in {-1, 0, 1, L}, the replicated step (world 0) and sharded worlds 1, 2
and 4 - every rank and rank = -1 (all ranks, the loopback communicator).  Scales: the reference's v1 layer-wise lr decay at 0.5 plus
weight-decay scale 0 on 1-D parameters.

Checked per configuration: the items tile exactly the share the step updates today, once each (the trainable ranges, or - sharded -
a rank's body slices plus the replicated tails, rebuilt here from gget_shard_plan's formula on the buckets' trainable share); every item
has cnt <= 2048 with off and cnt multiples of 4; no item crosses a parameter boundary at which a scale differs; every element carries
the scales of its parameter, a gap (and the pad rows behind lm_head.weight) those of the parameter in front of it."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _util import spec_mod

L = importlib.import_module("graph-gpt_amd._lib")
E = importlib.import_module("graph-gpt_amd.engine")
T = importlib.import_module("graph-gpt_amd.training")
CHUNK = L.SHARD_CHUNK
ITEM = 2048


@pytest.fixture(scope="module", autouse=True)
def _lib():
    importlib.import_module("graph-gpt_amd.build").build()
    return L.load()


def _spec(model):
    if model == "d768":
        return spec_mod.ModelSpec(kind=spec_mod.KIND_PRETRAIN, vocab_size=756, hidden_size=768, intermediate_size=3072, num_layers=2,
                                  num_heads=12, head_dim=64, stacked_feat=13, next_n_token=13, causal=False, max_position=1024)
    return spec_mod.spec_from_size(model, vocab_size=756, stacked_feat=13, next_n_token=13)


_MODELS = {}


def _model(model):
    """(cfg, parameter table, n_params, bucket ranges, lr scales, wd scales, per-element scale arrays)"""
    if model in _MODELS:
        return _MODELS[model]
    spec = _spec(model)
    cfg = E.make_config(spec, 256, 8)
    params = E.Engine.plan_params_of(cfg)
    sz = L.GgetSizes()
    L.check(L.load().gget_query_sizes(C.byref(cfg), C.byref(sz)))
    n = int(sz.n_params)
    buckets = [(p[0], p[1]) for p in E.Engine.shard_plan_of(cfg, 1, spec.num_layers + 2)]
    depth = T.layerwise_depths(params, spec.num_layers, 1, True)
    lr = np.array([0.5 ** depth[k] for k in params], dtype=np.float32)
    wd = np.array([0.0 if p["ndim"] == 1 else 1.0 for p in params.values()], dtype=np.float32)
    assert len(set(lr.tolist())) == spec.num_layers + 3 and 0.0 in wd and 1.0 in wd
    # the scales of every element: a parameter's reach to the next parameter's offset (gaps and pad rows ride with it)
    offs = [p["offset"] for p in params.values()]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 128 == 0 for o in offs)
    ends = offs[1:] + [n]
    el_lr, el_wd = np.empty(n, np.float32), np.empty(n, np.float32)
    for o, e, a, b in zip(offs, ends, lr, wd):
        el_lr[o:e], el_wd[o:e] = a, b
    assert any(e - o > p["numel"] for o, e, p in zip(offs, ends, params.values())), "the model must have gaps"
    _MODELS[model] = (spec, cfg, params, n, buckets, lr, wd, el_lr, el_wd)
    return _MODELS[model]


def _train_ranges(spec, params, n, k):
    """gget_trainable_ranges restated from the parameter table: [end of embed_tokens, start of layer 0) and [start of layer
    min(k, L), n_params); everything when k < 0"""
    if k < 0:
        return [(0, n)]
    al = lambda x: -(-x // 128) * 128       # noqa: E731
    emb = params["model.embed_tokens.weight"]
    emb_end = emb["offset"] + al(emb["numel"])
    layer0 = params["model.layers.0.input_layernorm.weight"]["offset"]
    k = min(k, spec.num_layers)
    start = params[f"model.layers.{k}.input_layernorm.weight" if k < spec.num_layers else "model.norm.weight"]["offset"]
    return [(o, c) for o, c in ((emb_end, layer0 - emb_end), (start, n - start)) if c > 0]


def _share(buckets, train, k, world, rank):
    """the element ranges the step updates: the trainable ranges (world 0), or the body slices of `rank` (-1: all) plus every tail
    of the buckets' trainable shares (include/gget.h gget_shard_plan: slice = floor(cnt / (world C)) C)"""
    if world == 0:
        return list(train)
    out = []
    for lo, cnt in buckets:
        hi = lo + cnt
        off, c = lo, 0
        for a, b in train:
            x, y = max(lo, a), min(hi, a + b)
            if x < y:
                off, c = x, y - x
                break
        sl = c // (world * CHUNK) * CHUNK
        for r in range(world):
            if rank < 0 or r == rank:
                out.append((off + r * sl, sl))
        out.append((off + world * sl, c - world * sl))
    return [(o, c) for o, c in out if c > 0]


@pytest.mark.parametrize("world", [0, 1, 2, 4])
@pytest.mark.parametrize("frozen", [-1, 0, 1, 2])
@pytest.mark.parametrize("model", ["tiny", "d768"])
def test_items_tile_the_share_and_carry_the_scales(model, frozen, world):
    spec, cfg, params, n, buckets, lr, wd, el_lr, el_wd = _model(model)
    assert spec.num_layers == 2      # (frozen = 2 is L)
    train = _train_ranges(spec, params, n, frozen)
    bounds = np.zeros(n + 1, dtype=bool)      # parameter offsets at which a scale differs from the element in front
    bounds[1:n] = (el_lr[1:] != el_lr[:-1]) | (el_wd[1:] != el_wd[:-1])
    assert bounds.sum() >= spec.num_layers + 2
    seen_all = np.zeros(n, dtype=np.int32)
    for rank in ([-1] if world == 0 else list(range(world)) + [-1]):
        items = E.Engine.group_plan_of(cfg, lr, wd, frozen, world, rank)
        want = np.zeros(n, dtype=np.int32)
        for o, c in _share(buckets, train, frozen, world, rank):
            want[o:o + c] += 1
        assert want.max() <= 1
        got = np.zeros(n, dtype=np.int32)
        for off, cnt, a, b in items:
            assert 0 < cnt <= ITEM and off % 4 == 0 and cnt % 4 == 0 and off + cnt <= n, (off, cnt)
            got[off:off + cnt] += 1
            assert not bounds[off + 1:off + cnt].any(), f"item ({off}, {cnt}) crosses a boundary where a scale changes"
            assert (el_lr[off:off + cnt] == np.float32(a)).all() and (el_wd[off:off + cnt] == np.float32(b)).all(), (off, cnt, a, b)
        assert np.array_equal(got, want), f"rank {rank}: the items do not tile the share once each"
        if rank >= 0:
            seen_all += got
    if world >= 1:
        # every rank's body slices are disjoint; the tails are updated by every rank
        want = np.zeros(n, dtype=np.int32)
        for r in range(world):
            for o, c in _share(buckets, train, frozen, world, r):
                want[o:o + c] += 1
        assert np.array_equal(seen_all, want)
        covered = np.zeros(n, dtype=bool)
        for o, c in train:
            covered[o:o + c] = True
        assert np.array_equal(seen_all > 0, covered), "all ranks together update exactly the trainable ranges"


def test_all_ones_cut_like_the_ungrouped_lists():
    """no table: one run, so the items are the ranges cut every 2048 elements (what the frozen and sharded lists are today)"""
    spec, cfg, params, n, buckets, *_ = _model("tiny")
    for frozen, world in ((-1, 0), (1, 0), (-1, 2), (1, 2)):
        items = E.Engine.group_plan_of(cfg, None, None, frozen, world, -1)
        want = [(o + x, min(ITEM, c - x), 1.0, 1.0) for o, c in _share(buckets, _train_ranges(spec, params, n, frozen), frozen, world, -1)
                for x in range(0, c, ITEM)]
        assert items == want


def test_bad_inputs_are_error_2():
    spec, cfg, params, n, buckets, lr, wd, *_ = _model("tiny")
    lib, fp = L.load(), C.POINTER(C.c_float)
    cnt = C.c_int32(-5)
    ptr = lambda a: a.ctypes.data_as(fp)     # noqa: E731
    call = lambda a, b, k, world=1, rank=0, frozen=-1: lib.gget_group_plan(C.byref(cfg), a, b, k, frozen, world, rank, None, 0, C.byref(cnt))   # noqa: E731
    assert call(ptr(lr), ptr(wd), len(lr)) == 0 and cnt.value > 0
    assert call(ptr(lr), ptr(wd), len(lr) - 1) == 2 and b"scales for" in lib.gget_last_error()
    assert call(ptr(lr), None, 0) == 2
    for bad in (-0.5, float("nan"), float("inf")):
        for which in (0, 1):
            arr = [lr.copy(), wd.copy()]
            arr[which][3] = bad
            assert call(ptr(arr[0]), ptr(arr[1]), len(lr)) == 2, (bad, which)
            msg = lib.gget_last_error().decode()
            assert ("lr_scale[3]", "wd_scale[3]")[which] in msg and list(params)[3] in msg
    assert call(ptr(lr), ptr(wd), len(lr), world=2, rank=2) == 2
    assert call(ptr(lr), ptr(wd), len(lr), world=2, rank=-2) == 2
    assert call(ptr(lr), ptr(wd), len(lr), frozen=-2) == 2
    # the handle-free parameter table: a bad configuration or index
    info = L.GgetParamInfo()
    assert lib.gget_plan_param_count(C.byref(L.GgetConfig())) == -1
    assert lib.gget_plan_param_info(C.byref(cfg), len(params), C.byref(info)) == 2
    assert lib.gget_plan_param_count(C.byref(cfg)) == len(params)
