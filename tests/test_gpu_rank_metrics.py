"""The HIP rank kernels behind the multi-label evaluation metrics (csrc/metrics.hip, include/gget.h gget_op_rank_metrics), op level
through the C ABI against the NumPy statement of the same counts (graph-gpt_amd/metrics.py `_rank_counts_numpy`, itself pinned against
scikit-learn in tests/test_metrics_multilabel.py), and model level: `ft_evaluate` with problem_type = "multi_label_classification" on
the `ft_tiny_ml` fixture.

Geometry of the launches (csrc/metrics.hip): a classification segment is 64 rows (kRankSeg; 4 segments x 64 columns per workgroup), a
workgroup of the count kernel owns a tile of 1024 positives (kRankTile = 256 lanes x 4), both lists stream through LDS in chunks of 1024
floats (kRankChunk) padded to a multiple of 4, the finish tree is 256 wide.  n = 63 / 65 straddle one segment, 257 a workgroup of
segments; C = 130 takes three column blocks (64 + 64 + 2); n = 5000 at a positive rate of 0.5 gives ~2500 positives (3 tiles, the last
ragged) and ~2500 negatives (3 chunks, the last ragged), at 0.01 ~50 positives (one ragged tile and chunk) and ~4950 negatives (5 chunks)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from _util import load_case, record_error

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-gpt_amd._lib")
met = importlib.import_module("graph-gpt_amd.metrics")
Mod = importlib.import_module("graph-gpt_amd.modeling")
tr = importlib.import_module("graph-gpt_amd.training")


def make_case(n, ncol, seed, pos_rate=0.4, nan_rate=0.3):
    """fp32 scores / labels [n, ncol]; column c is of kind c % 8: 0 random, 1 heavy ties (one decimal), 2 all-equal scores, 3 scores in
    {-0.0, +0.0}, 4 no positive, 5 no negative, 6 fully unlabelled, 7 random without NaN labels"""
    rng = np.random.RandomState(seed)
    kind = np.arange(ncol) % 8
    y = (rng.rand(n, ncol) < pos_rate).astype(np.float32)
    s = (rng.randn(n, ncol) + y).astype(np.float32)
    s[:, kind == 1] = np.round(s[:, kind == 1], 1)
    s[:, kind == 2] = 0.75
    s[:, kind == 3] = np.where(rng.rand(n, int((kind == 3).sum())) < 0.5, -0.0, 0.0).astype(np.float32)
    y[:, kind == 4], y[:, kind == 5] = 0.0, 1.0
    nan = rng.rand(n, ncol) < nan_rate
    nan[:, kind == 7] = False
    nan[:, kind == 6] = True
    y[nan] = np.nan
    return s, y


def run_op(s, y, ld_extra=0, ws_bytes=None):
    """gget_op_rank_metrics on device copies of s / y with row strides of ncol + ld_extra; returns (rc, the five outputs as NumPy)"""
    lib = L.load()
    n, ncol = s.shape
    ld = ncol + ld_extra
    sd = torch.full((max(n, 1), max(ld, 1)), float("nan"), device="cuda")
    yd = torch.full((max(n, 1), max(ld, 1)), 7.0, device="cuda")             # (the pad columns would all be "bad" if they were read)
    if n and ncol:
        sd[:n, :ncol], yd[:n, :ncol] = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    out = [torch.full((max(ncol, 1),), -3, dtype=dt, device="cuda") for dt in (torch.int64, torch.int64, torch.int64, torch.float64, torch.int32)]
    need = int(lib.gget_op_rank_metrics_workspace(n, ncol))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.gget_op_rank_metrics(sd.data_ptr(), ld, yd.data_ptr(), ld, n, ncol, *[o.data_ptr() for o in out], ws.data_ptr(), nbytes,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    n_pos, n_neg, auc2, ap_sum, n_bad = [o.cpu().numpy()[:ncol] for o in out]
    return rc, (n_pos, n_neg, auc2.view(np.uint64), ap_sum, n_bad)


def check_against_numpy(s, y, ld_extra, what):
    rc, got = run_op(s, y, ld_extra)
    assert rc == 0, L.load().gget_last_error()
    rc2, again = run_op(s, y, ld_extra)
    assert rc2 == 0
    want = met._rank_counts_numpy(s, y)
    n = s.shape[0]
    for name, g, w in zip(("n_pos", "n_neg", "auc2", "n_bad"), (got[0], got[1], got[2], got[4]), (want[0], want[1], want[2], want[4])):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)          # exact integers
    tol = n * 2.0 ** -52 * want[0]                                                       # n 2^-52 n_pos per column
    dev = np.abs(got[3] - want[3])
    print(f"{what}: ap_sum max |dev| {dev.max() if dev.size else 0.0:.3e} (largest bound {tol.max() if tol.size else 0.0:.3e})")
    assert (dev <= tol).all(), (what, dev.max(), got[3], want[3])
    invalid = (want[0] == 0) | (want[1] == 0)
    assert not got[2][invalid].any() and not got[3][invalid].any()                      # zeros where a class is missing
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes(), what                                         # bit-identical from run to run
    return got, want


@pytest.mark.parametrize("ncol", [1, 5, 130])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 5000])
def test_rank_op_matches_numpy_counts(n, ncol):
    ld_extra = 3 if (n + ncol) % 2 else 0                      # row strides ld_s, ld_y > C in half of the cases
    rates = (0.5, 0.01) if n == 5000 else (0.4,)
    for rate in rates:
        s, y = make_case(n, ncol, seed=1000 * n + ncol, pos_rate=rate, nan_rate=0.0 if n == 5000 else 0.3)
        got, want = check_against_numpy(s, y, ld_extra, f"n={n} C={ncol} rate={rate} ld=C+{ld_extra}")
        if n == 5000:                 # the shapes cross the tile / chunk sizes the docstring states
            np0, nn0 = int(want[0][0]), int(want[1][0])
            assert (np0 > 2048 and nn0 > 2048) if rate == 0.5 else (0 < np0 < 1024 and nn0 > 4096)
            assert np0 % 1024 and nn0 % 1024                     # ragged last tile / chunk
    if ncol == 1 and n >= 63:         # one column of heavy ties on its own (kind 0 is the only kind a single column takes)
        s, y = make_case(n, 1, seed=n)
        check_against_numpy(np.round(s, 1), y, 5, f"n={n} C=1 ties")


def test_rank_op_single_column_kinds_at_tile_crossing_size():
    """every degenerate kind with positives beyond one tile: ties, all-equal, +-0, no positive / negative, unlabelled (n = 2500, C = 8)"""
    s, y = make_case(2500, 8, seed=9, pos_rate=0.6, nan_rate=0.1)
    got, want = check_against_numpy(s, y, 8, "n=2500 C=8")
    assert want[0][[0, 1, 2, 3, 7]].min() > 1024
    half = want[0] * want[1]                                     # all-equal scores and +-0: every pair is a tie -> auc2 = n_pos n_neg
    assert got[2][2] == half[2] and got[2][3] == half[3]


def test_rank_op_workspace_and_empty_calls():
    lib = L.load()
    s, y = make_case(65, 5, seed=2)
    need = int(lib.gget_op_rank_metrics_workspace(65, 5))
    assert need > 0 and lib.gget_op_rank_metrics_workspace(0, 5) == 0 and lib.gget_op_rank_metrics_workspace(65, 0) == 0
    rc, got = run_op(s, y, ws_bytes=need - 1)
    assert rc != 0 and b"workspace" in lib.gget_last_error()
    assert all(((g.view(np.int64) if g.dtype == np.uint64 else g) == -3).all() for g in got)      # refused before any launch
    for n, ncol in ((0, 5), (65, 0), (0, 0)):
        assert lib.gget_op_rank_metrics(None, ncol, None, ncol, n, ncol, None, None, None, None, None, None, 0, None) == 0
    assert lib.gget_op_rank_metrics(None, 1, None, 1, -1, 1, None, None, None, None, None, None, 0, None) != 0
    r = met.rank_metrics(torch.zeros(0, 4, device="cuda"), torch.zeros(0, 4, device="cuda"))
    assert r["n_pos"].tolist() == [0] * 4 and np.isnan(r["ap"]).all()


def test_rank_op_bad_entry_guard():
    """label 2 and an infinite score on a labelled row are counted in n_bad and left out; a NaN score on an UNLABELLED row is not bad"""
    s, y = make_case(257, 5, seed=4)
    lab0 = np.flatnonzero(~np.isnan(y[:, 0]))
    y[lab0[0], 0] = 2.0
    s[lab0[1], 0] = np.inf
    s[lab0[2], 0] = np.nan
    s[np.isnan(y[:, 1]), 1] = np.nan
    got, want = check_against_numpy(s, y, 0, "bad entries")
    assert got[4].tolist() == [3, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="3 labelled entries"):
        met.rank_metrics(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
    # the Python surface on clean device tensors: the same vectors as the host path, through a row-strided view
    s, y = make_case(257, 5, seed=5)
    wide_s, wide_y = torch.zeros(257, 9, device="cuda"), torch.zeros(257, 9, device="cuda")
    wide_s[:, :5], wide_y[:, :5] = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    r_dev, r_host = met.rank_metrics(wide_s[:, :5], wide_y[:, :5]), met.rank_metrics(s, y)
    assert np.array_equal(r_dev["auroc"], r_host["auroc"], equal_nan=True)                 # exact counts, one division
    assert np.allclose(r_dev["ap"], r_host["ap"], rtol=0, atol=257 * 2.0 ** -52, equal_nan=True)


# ------------------------------------------------------------------------------------------------ model level
def _model_for(spec, state):
    cfg = Mod.GraphGPTConfig(hidden_act="gelu", vocab_size=spec.vocab_size, hidden_size=spec.hidden_size,
                             intermediate_size=spec.intermediate_size, num_hidden_layers=spec.num_layers,
                             num_attention_heads=spec.num_heads, max_position_embeddings=spec.max_position,
                             causal_attention=spec.causal, stacked_feat=spec.stacked_feat, num_labels=spec.num_labels,
                             problem_type="multi_label_classification", loss_type=None, layer_scale_init_value=spec.layer_scale_init,
                             rms_norm_eps=spec.rms_eps, pad_token_id=spec.pad_token_id,
                             stacked_feat_agg_method="gated" if spec.gated_agg else "sum")
    model = Mod.GraphGPTTaskModel(cfg, seed=1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.cuda()


def _loader(batch, n_parts, device_tensors):
    B = batch["input_ids"].shape[0]
    cuts = np.linspace(0, B, n_parts + 1).astype(int)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        d = {k: torch.from_numpy(np.ascontiguousarray(v[a:b])) for k, v in batch.items() if k != "lengths"}
        d["idx"] = torch.arange(a, b)
        out.append({k: v.cuda() for k, v in d.items()} if device_tensors else d)
    return out


@pytest.fixture(scope="module")
def ml_case():
    z, spec, state, batch = load_case("ft_tiny_ml")
    y = batch["task_labels"]
    valid = [(y[:, c] == 1).any() and (y[:, c] == 0).any() for c in range(y.shape[1])]
    assert sum(valid) >= 2, "the fixture holds fewer than two valid columns"           # (all 5 of its columns are: 6 rows suffice)
    return z, spec, _model_for(spec, state), batch


@pytest.mark.parametrize("device_tensors", [True, False])
@pytest.mark.parametrize("dataset_name", ["ogbg-molpcba", "ogbn-proteins"])
def test_ft_evaluate_multilabel_from_hip_logits(ml_case, dataset_name, device_tensors, monkeypatch):
    """`ft_evaluate` on the fixture cut in two parts.  Bounds from the logit deviation delta = max |y_pred - reference logits| (pair-margin
    argument of tests/test_gpu_metrics.py): going from the reference's order of a column to the engine's is a chain of adjacent swaps of
    pairs whose reference margin is <= 2 delta.  A (positive, negative) swap moves auc2 by at most 2 of its 2 n_pos n_neg, and one AP term
    g / (g + b) to g / (g + b +- 1), i.e. ap_sum by at most 1/2; a (positive, positive) pair changes ap_sum only by becoming a tie (the
    earlier one takes the later one's precision: d/dg g / (g + b) <= 1/4 per step).  So per column |d auroc| <= K_pn / (n_pos n_neg) and
    |d ap| <= (K_pn + K_pp) / (2 n_pos), K = pairs of that kind with margin <= 2 delta; the dataset figure is the mean over the columns."""
    z, spec, model, batch = ml_case
    calls = []
    real = met.rank_metrics
    monkeypatch.setattr(met, "rank_metrics", lambda s, y: (calls.append((s.device.type, y.device.type, tuple(s.shape))), real(s, y))[1])
    loss, m, res, d = tr.ft_evaluate(model, _loader(batch, 2, device_tensors), problem_type="multi_label_classification",
                                     num_labels=spec.num_labels, dataset_name=dataset_name)
    assert model.training                                                       # back in train mode
    y = batch["task_labels"]
    B, ncol = y.shape
    # compute() and the dataset evaluator both ranked on the device, on the whole accumulation
    assert calls == [("cuda", "cuda", (B, ncol))] * 2, calls
    assert all(v.device.type == "cpu" for v in d.values())                      # the one host transfer, after the metrics
    assert d["idx"].tolist() == list(range(B)) and np.array_equal(d["y_true"].numpy(), y, equal_nan=True)
    ref = z["logits"].astype(np.float64)
    hip = d["y_pred"].numpy().astype(np.float64)
    delta, scale = float(np.abs(hip - ref).max()), float(np.abs(ref).max())
    tag = f"{dataset_name} ({'device' if device_tensors else 'host'} batches)"
    record_error("ft_tiny_ml", f"metrics_logit_max_abs_dev_rel {tag}", delta / scale, 4e-2)
    assert delta <= 4e-2 * scale, (delta, scale)                                # the bf16-class logit tolerance of tests/test_gpu_metrics.py
    key = {"ogbg-molpcba": "ap", "ogbn-proteins": "rocauc"}[dataset_name]
    assert list(res) == [key]
    r_ref = real(z["logits"], y)
    bound = []
    for c in range(ncol):
        pos, neg = ref[y[:, c] == 1, c], ref[y[:, c] == 0, c]
        k_pn = int((np.abs(pos[:, None] - neg[None, :]) <= 2 * delta).sum())
        k_pp = (int((np.abs(pos[:, None] - pos[None, :]) <= 2 * delta).sum()) - len(pos)) // 2
        bound.append(k_pn / (len(pos) * len(neg)) if key == "rocauc" else (k_pn + k_pp) / (2 * len(pos)))
    want = float(np.mean(r_ref["auroc" if key == "rocauc" else "ap"]))
    tol = float(np.mean(bound)) + 1e-12
    print(f"{tag}: {key} {res[key]:.6f} reference {want:.6f} bound {tol:.3e} delta {delta:.3e}")
    record_error("ft_tiny_ml", f"{key}_abs_dev {tag}", abs(res[key] - want), tol)
    assert abs(res[key] - want) <= tol, (res[key], want, tol)
    # the metric object: per-task ROC-AUC of sigmoid(logits) (monotone: the same pair argument), mean over the 5 valid tasks
    pn = [int((np.abs(ref[y[:, c] == 1, c][:, None] - ref[y[:, c] == 0, c][None, :]) <= 2 * delta).sum()) /
          (int((y[:, c] == 1).sum()) * int((y[:, c] == 0).sum())) for c in range(ncol)]
    assert m.auroc_vec.shape == (ncol,) and (np.abs(m.auroc_vec - r_ref["auroc"]) <= np.array(pn) + 1e-12).all()
    assert m.results_in_dict() == {"auroc_mean": float(m.auroc_vec.mean())}
    assert np.isfinite(float(loss))
