"""One fine-tune step (gget_forward_task + gget_backward of a task-kind model with the Linear `score` head) replayed from outside the
engine, one launch at a time, through the operator entries of the C ABI (gget_op_*).  csrc/engine.hip calls the launchers those entries
call, so the engine's step is owed BIT EQUALITY with this replay wherever the launches are deterministic; together with the per-element
operator tests that makes the step "the right operators on the right operands".

What is here, in three parts:

 * the dispatch mirror (`forms`): which form every stage takes, decided from the configuration, B, S, the layout and the launch menu by
   the rule WRITTEN HERE.  The engine is never asked.  tests/test_step_replay_host.py spells the table out for the cases of
   tests/test_gpu_step_replay.py, so a change of the rule is a visible diff.  `rotation` is the three-buffer rule of the residual-stream
   gradient.
 * the comparer (`compare_bits`, `first_difference`): integers against integers, the first differing observable in step order, the
   count, the first (index, got, want) triples and whether the differing elements form whole rows.
 * `Replay`: the launches.  Every intermediate lives in a buffer of the replay's own (`Buf`): real rows pre-filled with the NaN sentinel
   of tests/_gpu_out.py, guard rows behind them, and - the engine's own rule, gget_create clears its workspace - ZEROS in the <= 63
   round-up rows of the var-len layout, which belong to no sample: the engine multiplies whatever finite values they hold by zero
   gradients, it never defines them.

Where equality is NOT owed (the reason is in the code, and said again at the stage below):
 * RMSNorm / LayerScale weight gradients in the default mode: fp32 atomics of many blocks into 8 replicas (kernels.hip, residual.hip).
 * score.weight / score.bias in EVERY mode: score_bwd_kernel cuts the batch into 16 slices per class and adds them with fp32 atomics
   (more than two adds onto zero: the order shows).  The reproducible mode (menu key 4) orders the RMSNorm sums only.
 * the sorted embedding backward (gated aggregation, or a vocabulary past the count-matrix form) and the gate gradient: the counting
   sort places equal ids in atomic order and runs cut by a segment boundary are added with atomics.
 * LayerScale vectors in the reproducible mode as well: residual.hip has no ordered form.
Those tensors are held to the float64 sum of their own terms, computed from the replay's stage inputs, under the bound tests/_rows_ref.py
states for such a sum (_accum_check: 2 (n + 1) u (sum of |term|), n terms in any order) plus the bf16 rounding of the conversion
(1.01 x 2^-8 |ref|, as _rows_ref's dx bounds write it).
"""
import ctypes as C
import importlib

import torch

L = importlib.import_module("graph-gpt_amd._lib")

SENT16 = 0x7FC1
SENT32 = 0x7FC01234
GUARD_ROWS = 8
BF = torch.bfloat16
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 2.0 ** -126
NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_RES = 0, 1
ACCUM_COPIES, ACCUM_COPY_MAX = 8, 8192       # csrc/kernels.h kAccumCopies / kAccumCopyMax


def align_up(x, a):
    return (x + a - 1) // a * a


# ================================================================================================== the plan, restated
def param_offsets(spec):
    """name -> (offset, count, layer) of the flat arenas: the state-dict order, every tensor padded to 128 elements (engine.hip make_plan)."""
    out, off = {}, 0
    for name, shape in spec.param_table().items():
        n = 1
        for s in shape:
            n *= int(s)
        if name.startswith("model.layers."):
            layer = int(name.split(".")[2])
        elif name in ("model.embed_tokens.weight", "stacked_feat_agg.weight"):
            layer = -1
        else:
            layer = spec.num_layers
        out[name] = (off, n, layer)
        off += align_up(n, 128)
    return out, off


def is_accum32(name, shape):
    """Gradients summed in the fp32 scratch: the embeddings, the gate, every vector and the score head."""
    return name in ("model.embed_tokens.weight", "stacked_feat_agg.weight", "score.weight", "score.bias") or len(shape) == 1


def scratch_layout(spec):
    """name -> (offset of replica 0, replicas, stride) in the fp32 scratch, and its length: parameters of up to 8192 elements have 8
    replicas `align_up(count, 128)` apart."""
    out, off = {}, 0
    for name, shape in spec.param_table().items():
        if not is_accum32(name, shape):
            continue
        n = 1
        for s in shape:
            n *= int(s)
        copies = ACCUM_COPIES if n <= ACCUM_COPY_MAX else 1
        out[name] = (off, copies, align_up(n, 128))
        off += align_up(n, 128) * copies
    return out, off


def bucket_of(layer, L_):
    """Gradient buckets in completion order: heads, layers L-1 .. 0, embeddings."""
    return 0 if layer == L_ else (L_ + 1 if layer < 0 else L_ - layer)


def segment_table(spec):
    """Per bucket, the (src, dst, count, copies, stride) rows of the fp32 -> bf16 conversion (engine.hip gget_create)."""
    offs, _ = param_offsets(spec)
    s32, _ = scratch_layout(spec)
    segs = [[] for _ in range(spec.num_layers + 2)]
    for name in spec.param_table():
        if name in s32:
            off, n, layer = offs[name]
            src, copies, stride = s32[name]
            segs[bucket_of(layer, spec.num_layers)].append((src, off, align_up(n, 128), copies, stride))
    return segs


def truncated(spec, frozen):
    """Nothing trainable upstream of layer 0: the backward stops at the lowest trainable unit."""
    return frozen >= 0 and not spec.gated_agg and spec.embed_dim == 0


# ================================================================================================== the dispatch mirror
def rotation(n_layers, first=0):
    """(dx_out, dx_mid, dx_in) of layer_backward for layers L-1 .. first over the three buffers 'a', 'b', 'c': gget_backward_begin leaves
    the gradient of the final-norm OUTPUT in 'b' and that of its input in 'a'; a layer reads dx_out = what the stage above wrote, uses the
    next buffer of the ring for dx_mid and the one after for dx_in."""
    ring, cur, out = "abc", 0, {}
    for i in range(n_layers - 1, first - 1, -1):
        out[i] = (ring[cur], ring[(cur + 1) % 3], ring[(cur + 2) % 3])
        cur = (cur + 2) % 3
    return out


def qkvo_split(T):
    """K slices of the q|k|v|o slab launch at d % 192 != 0 (engine.hip qkvo_wgrad_split)."""
    return 3 if T >= 3 * 1024 else 1


def forms(spec, B, S, num_tokens=None, frozen=-1, mlp_drop=0.0, reproducible=False, num_cu=256):
    """The form of every stage, by name.  num_tokens: the caller's real-token count (None: padded layout)."""
    d, ff, H, Ln = spec.hidden_size, spec.intermediate_size, spec.num_heads, spec.num_layers
    has_ls = spec.layer_scale_init > 0
    has_res = has_ls or spec.path_pdrop > 0 or spec.mlp_pdrop > 0
    t_rows = align_up(num_tokens, 64) if num_tokens else 0
    varlen = bool(num_tokens) and t_rows < B * S
    T = t_rows if varlen else B * S
    f = {"layout": "varlen" if varlen else "padded", "T": T}
    # the fragment-major o weights are built when a per-sample kernel CAN run in this step: S <= 32, or S <= 64 while the var-len layout may
    # still be chosen (a token count was handed over - whether or not it ends up compacting); one workgroup per sample, so B has to fill its
    # rounds of the CUs
    rounds = (B + num_cu - 1) // num_cu
    rounds_ok = B <= num_cu or B * 100 >= rounds * num_cu * 85
    wo_packed = (not has_res) and (S <= 32 or (S <= 64 and bool(num_tokens))) and rounds_ok and d % 64 == 0
    f["pack_wo"] = "per-forward" if wo_packed else "none"
    per_sample_h = H in (2, 4, 8, 12)
    f["attn_fwd"] = "per-sample" if (wo_packed and S <= 32 and per_sample_h) else ("ls-residual" if has_res else "three-launch")
    f["geglu"] = "fused" if (ff % 128 == 0 and d % 64 == 0) else "gemm+elementwise"
    f["mlp_bwd"] = "gemm+dropout+geglu'" if mlp_drop > 0 else f["geglu"]
    # the backward's per-sample kernel: S <= 32, or S <= 64 on the var-len layout (every sample by its own row count; the 33 .. 64-row
    # samples' attention backward is a second launch driven by long_list)
    bwd_ps = wo_packed and per_sample_h and (S <= 32 or (S <= 64 and varlen))
    f["attn_bwd"] = ("per-sample" if S <= 32 else "per-sample+long_list") if bwd_ps else ("ls-norm-bwd+dgrad+attn-bwd" if has_res else "norm-bwd+dgrad+attn-bwd")
    f["wgrad"] = "grouped-4" if (d % 192 == 0 and ff % 192 == 0) else f"grouped-2+qkvo-slabs-split{qkvo_split(T)}"
    trunc = truncated(spec, frozen)
    first = min(frozen, Ln) if trunc else 0
    f["first_layer"] = first
    # ln1 backward of layer i: fused with the LayerScale backward of layer i - 1's MLP branch (behind the weight gradients, which still read
    # dscaled) unless i == 0 or i is the boundary above a frozen prefix (weight gradient only)
    f["ln1_bwd"] = {i: ("dw-only" if (trunc and i == frozen) else ("fuse_next" if (has_res and i > 0) else "plain")) for i in range(first, Ln)}
    f["final_norm"] = "from-last-layer" if has_res else "own-launch"
    f["final_norm_bwd"] = "dw-only" if (trunc and frozen >= Ln) else ("fused-ls2" if has_res else "plain")
    dense_ok = (not spec.gated_agg) and align_up(spec.vocab_size, 64) <= 1024 and (spec.vocab_size * d) % 4 == 0
    f["embed_bwd"] = "none" if trunc else ("dense" if dense_ok else "sorted")
    f["rotation"] = rotation(Ln, first)
    f["reproducible"] = bool(reproducible)
    return f


def inexact_tensors(spec, f):
    """name -> why equality is not owed there (module docstring); everything else is bit-equal."""
    why = {}
    for name, shape in spec.param_table().items():
        if name.endswith("lambda_1") or name.endswith("lambda_2"):
            why[name] = "LayerScale: fp32 atomics, no ordered form"
        elif len(shape) == 1 and name != "score.bias" and not f["reproducible"]:
            why[name] = "RMSNorm weight gradient: fp32 atomics (default mode)"
        elif name in ("score.weight", "score.bias"):
            why[name] = "score_bwd: 16 batch slices per class added with fp32 atomics"
        elif name in ("model.embed_tokens.weight", "stacked_feat_agg.weight") and f["embed_bwd"] == "sorted":
            why[name] = "sorted embedding backward: atomic placement and boundary atomics"
    return why


# ================================================================================================== the comparer
def _as_int(t):
    if t.dtype == BF:
        return t.contiguous().view(torch.int16)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t


def compare_bits(name, got, want):
    """None when `got` and `want` hold the same bits; else the text: how many elements differ, the first (index, got, want) triples, and
    whether the differing elements are whole rows."""
    if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
        return f"{name}: shape / dtype {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    gi, wi = _as_int(got.cpu()), _as_int(want.cpu())
    bad = gi != wi
    n = int(bad.sum())
    if n == 0:
        return None
    cols = got.shape[-1] if got.dim() > 1 else 1
    b2 = bad.reshape(-1, cols)
    rows = b2.any(1)
    whole = bool((b2[rows].all(1)).all()) and cols > 1
    idx = b2.nonzero()[:4].tolist()
    g2, w2 = got.cpu().reshape(-1, cols), want.cpu().reshape(-1, cols)
    trip = "; ".join(f"({r}, {c}) got {float(g2[r, c])!r} want {float(w2[r, c])!r}" for r, c in idx)
    sent = int((gi == (SENT16 if got.dtype == BF else SENT32)).sum()) if got.dtype in (BF, torch.float32) else 0
    return (f"{name}: {n} of {bad.numel()} elements differ in {int(rows.sum())} row(s) "
            f"{rows.nonzero().flatten()[:6].tolist()} ({'WHOLE rows' if whole else 'scattered elements'}"
            f"{', ' + str(sent) + ' still at the sentinel' if sent else ''}); first: {trip}")


def first_difference(pairs):
    """pairs: [(name, got, want)] in step order.  None, or the text of the FIRST differing observable followed by the names of the others
    that differ (the first one localises the stage)."""
    msgs = [(n, compare_bits(n, g, w)) for n, g, w in pairs]
    bad = [(n, m) for n, m in msgs if m is not None]
    if not bad:
        return None
    also = [n for n, _ in bad[1:]]
    return f"first differing observable in step order - {bad[0][1]}" + (f"\n  also differing later: {also[:12]}" if also else "")


def held_sum(name, got, ref64, abs64, n_terms):
    """|got - ref| <= 1.01 x 2^-8 |ref| + 2 (n + 1) u sum|term| + tiny per element: (ratio, failure text or None)."""
    got, ref64, abs64 = got.double().reshape(-1), ref64.double().reshape(-1), abs64.double().reshape(-1)
    bound = 1.01 * UB * ref64.abs() + 2 * (n_terms + 1) * U * abs64 + TINY
    err = (got - ref64).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound).nan_to_num(float("inf")).max()) if err.numel() else 0.0
    if not bool(bad.any()):
        return ratio, None
    i = int(bad.nonzero()[0])
    return ratio, f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the float64 bound; first [{i}] got {float(got[i])!r} ref {float(ref64[i])!r} bound {float(bound[i]):.3g}"


# ================================================================================================== buffers
class Buf:
    """[rows, cols] of `dtype`: rows [0, real) at the NaN sentinel, rows [real, rows) zero (the var-len round-up rows), GUARD_ROWS rows of
    sentinel behind."""

    def __init__(self, rows, cols, dtype, real=None, zero=False, device="cuda"):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        n = (rows + GUARD_ROWS) * cols
        if dtype == BF:
            self.t = torch.full((n,), SENT16, dtype=torch.int16, device=device).view(BF)
        elif dtype == torch.float32:
            self.t = torch.full((n,), SENT32, dtype=torch.int32, device=device).view(torch.float32)
        else:
            self.t = torch.full((n,), -7, dtype=dtype, device=device)
        real = rows if real is None else real
        if zero:
            self.t[:rows * cols] = 0
        elif real < rows:
            self.t[real * cols: rows * cols] = 0

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr())

    def at(self, elems):
        return C.c_void_p(self.t.data_ptr() + elems * self.t.element_size())

    def body(self):
        return self.t[:self.rows * self.cols].view(self.rows, self.cols)

    def guard_intact(self):
        g = self.t[self.rows * self.cols:]
        if self.dtype == BF:
            return bool((g.view(torch.int16) == SENT16).all())
        if self.dtype == torch.float32:
            return bool((g.view(torch.int32) == SENT32).all())
        return bool((g == -7).all())

    def rows_at_sentinel(self):
        b = self.body()
        if self.dtype == BF:
            return (b.view(torch.int16) == SENT16).all(1)
        return (b.view(torch.int32) == SENT32).all(1)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def u32(x):
    return int(x) & 0xFFFFFFFF


# ================================================================================================== the replay
class Replay:
    """options: num_tokens (the caller's count or None), seed / path_p / mlp_p (gget_set_dropout / _ex, training mode), frozen,
    reproducible (menu key 4 is set by the CALLER around both runs - here it only selects which tensors are owed equality), staged
    (per-bucket conversion), audit (float64 checks of the GEMM-class launches; self.audit_ratio)."""

    def __init__(self, spec, arena, rope, max_position, num_tokens=None, seed=0, path_p=0.0, mlp_p=0.0, frozen=-1, reproducible=False,
                 staged=False, audit=False, problem=L.PROBLEM_SINGLE_LABEL):
        self.lib = L.load()
        self.spec, self.P_, self.max_position = spec, arena, max_position
        self.cos, self.sin = rope
        self.opt = dict(num_tokens=num_tokens, seed=u32(seed), path_p=float(path_p), mlp_p=float(mlp_p), frozen=frozen, staged=staged)
        self.reproducible, self.audit, self.problem = reproducible, audit, problem
        self.off, self.n_params = param_offsets(spec)
        self.s32_off, self.n_s32 = scratch_layout(spec)
        self.segs = segment_table(spec)
        self.audit_ratio = {}
        self.sums = {}
        self.sk_ws = torch.zeros(int(self.lib.gget_op_gemm_streamk_bytes()), dtype=torch.uint8, device="cuda")
        # the gradient arena of the replay: sentinel everywhere - a frozen range must still hold it afterwards
        self.G = Buf(self.n_params // 128, 128, BF)
        self.bounded = {}      # name -> (ratio, failure) of the tensors that are not owed equality

    # ---------------------------------------------------------------- small helpers
    def w(self, name):
        return C.c_void_p(self.P_.data_ptr() + 2 * self.off[name][0])

    def wt(self, name):
        o, n, _ = self.off[name]
        return self.P_[o:o + n]

    def g(self, name):
        return self.G.at(self.off[name][0])

    def grad(self, name):
        o, n, _ = self.off[name]
        return self.G.t[o:o + n].view(tuple(self.spec.param_table()[name]))

    def s(self, name):
        return C.c_void_p(self.s32.data_ptr() + 4 * self.s32_off[name][0])

    def ck(self, rc):
        L.check(rc)

    def gemm(self, mode, epi, A, B, Cb, R, M, N, K, lda, ldb, ldc):
        """A plain GEMM as engine.hip's gemm_nt / gemm_nn issue it: one problem, under the stream-K workspace of the call."""
        self.ck(self.lib.gget_op_gemm_streamk(mode, epi, A, B, Cb, R, M, N, K, lda, ldb, ldc, P(self.sk_ws), ST()))

    def elem(self, layer):
        """(elem_p, elem_seed, elem_rows) of mlp_drop(layer) (engine.h)."""
        return (self.opt["mlp_p"], u32(self.opt["seed"] + 0x7F4A7C15 * (layer + 1)), P(self.c2p) if self.f["layout"] == "varlen" else None)

    def path(self, layer, which):
        """(rate, seed, S, row_b) of path_drop(layer, which) (engine.h)."""
        Ln = self.spec.num_layers
        pp = self.opt["path_p"]
        rate = float(torch.tensor(pp, dtype=torch.float32) * torch.tensor(float(layer), dtype=torch.float32)
                     / torch.tensor(float(Ln - 1), dtype=torch.float32)) if (pp > 0 and Ln > 1) else 0.0
        return (rate, u32(self.opt["seed"] ^ u32(0xD6E8FEB8 * (layer * 2 + which + 1))), self.S, P(self.rowb) if self.f["layout"] == "varlen" else None)

    def attn_seed(self, layer):
        return u32(self.opt["seed"] + 0x9E37 * layer)

    # ---------------------------------------------------------------- float64 audit of the GEMM-class launches
    def _aud(self, key, got, ref, bound):
        if not self.audit:
            return
        err = (got.double() - ref).abs()
        r = float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
        bad = ~(err <= bound)
        assert not bool(bad.any()), (f"float64 audit of {key}: {int(bad.sum())} of {bad.numel()} elements out of bound (worst ratio {r:.3g}); "
                                     f"first {bad.nonzero()[:3].tolist()}")
        self.audit_ratio[key] = max(self.audit_ratio.get(key, 0.0), r)

    @staticmethod
    def _dot64(mode, A, B):
        a, b = A.double(), B.double()
        a = a.t() if mode == TN else a
        b = b.t() if mode == NT else b
        return a @ b, a.abs() @ b.abs()

    def audit_gemm(self, key, mode, A, B, got, K, R=None, c_acc=2.0):
        """tests/test_gpu_gemm_exact.py's random-operand bound (assert_elementwise): 2^-8 |ref| + c_acc K 2^-24 |A| |B|; c_acc = 1 + live slices
        for a single launch (check_single), 1 for the grouped one (check_grouped_random)."""
        if not self.audit:
            return
        ref, ab = self._dot64(mode, A, B)
        if R is not None:
            ref, ab = ref + R.double(), ab + R.double().abs()
        self._aud(key, got, ref, UB * ref.abs() + c_acc * K * U * ab)

    # ---------------------------------------------------------------- forward
    def forward(self, ids, mask, pos, labels, wgt=None):
        spec, lib = self.spec, self.lib
        d, ff, H, Ln, F = spec.hidden_size, spec.intermediate_size, spec.num_heads, spec.num_layers, spec.stacked_feat
        B, S = int(ids.shape[0]), int(ids.shape[1])
        self.B, self.S = B, S
        f = self.f = forms(spec, B, S, self.opt["num_tokens"], self.opt["frozen"], self.opt["mlp_p"], self.reproducible)
        T = self.T = f["T"]
        self.inexact = inexact_tensors(spec, f)
        varlen = f["layout"] == "varlen"
        tc = self.tc = self.opt["num_tokens"] if varlen else B * S
        eps = float(spec.rms_eps)
        i32 = torch.int32
        self.ids, self.mask, self.labels, self.wgt = ids, mask, labels, wgt
        # 1. lengths / pool rows
        self.key_len = torch.full((B + 8,), -7, dtype=i32, device="cuda")
        self.pool_row = torch.full((B + 8,), -7, dtype=i32, device="cuda")
        self.ck(lib.gget_op_lengths(P(mask), P(ids), F, spec.pad_token_id, P(self.key_len), P(self.pool_row), B, S, ST()))
        # 3. position clamp (before the plan: the plan compacts the clamped positions)
        self.pos_safe = torch.full((B * S + 8,), -7, dtype=torch.int64, device="cuda")
        self.pos_flag = torch.zeros(4, dtype=i32, device="cuda")
        self.ck(lib.gget_op_clamp_positions(P(pos), P(self.pos_safe), P(self.pos_flag), B * S, self.max_position, ST()))
        pos_rows, ids_rows, self.row_base, self.long_list = self.pos_safe, ids, None, None
        # 2. the var-len plan
        if varlen:
            self.cu = torch.full((B + 1 + 8,), -7, dtype=i32, device="cuda")
            self.ids_c = torch.full(((T + 1) * F,), -7, dtype=torch.int64, device="cuda")
            self.pos_c = torch.full((T + 8,), -7, dtype=torch.int64, device="cuda")
            self.rowb = torch.full((T + 8,), -7, dtype=i32, device="cuda")
            self.pad2c = torch.full((B * S + 8,), -7, dtype=i32, device="cuda")
            self.c2p = torch.full((T + 8,), -7, dtype=i32, device="cuda")
            self.vl_status = torch.zeros(8, dtype=i32, device="cuda")
            self.vl_long = torch.full((3 * B + 1 + 8,), -7, dtype=i32, device="cuda")
            self.ck(lib.gget_op_varlen_plan(P(ids), F, F, P(self.pos_safe), P(self.key_len), P(self.pool_row), P(self.cu), P(self.ids_c),
                                            P(self.pos_c), P(self.rowb), P(self.pad2c), P(self.c2p), P(self.vl_status), B, S, tc, T,
                                            spec.pad_token_id, P(self.vl_long), ST()))
            pos_rows, ids_rows, self.row_base, self.long_list = self.pos_c, self.ids_c, self.cu, self.vl_long
        self.pos_rows, self.ids_rows = pos_rows, ids_rows
        # the fragment-major o weights, rebuilt in every forward from the bf16 weights as they are NOW
        if f["pack_wo"] == "per-forward":
            self.wo_pack, self.wot_pack = Buf(Ln * d, d, BF), Buf(Ln * d, d, BF)
            stride = self.off["model.layers.1.self_attn.o_proj.weight"][0] - self.off["model.layers.0.self_attn.o_proj.weight"][0] if Ln > 1 else 0
            self.ck(lib.gget_op_pack_wo(self.w("model.layers.0.self_attn.o_proj.weight"), stride, self.wo_pack.p, self.wot_pack.p, d, Ln, ST()))
        # 4. embedding (+ gate)
        nb = lambda cols, dt=BF: Buf(T, cols, dt, real=tc)   # noqa: E731
        self.x = [nb(d) for _ in range(Ln + 1)]
        gate = self.w("stacked_feat_agg.weight") if spec.gated_agg else None
        self.ck(lib.gget_op_embed_fwd(P(ids_rows), self.w("model.embed_tokens.weight"), gate, self.x[0].p, T, F, F, d, ST()))
        self.lw = [dict(xn1=nb(d), qkv=nb(3 * d), attn=nb(d), lse=Buf(B * S, H, torch.float32), xmid=nb(d), xn2=nb(d), rstd1=nb(1, torch.float32),
                        rstd2=nb(1, torch.float32), gu=nb(2 * ff), h=nb(ff), araw=nb(d), mraw=nb(d)) for _ in range(Ln)]
        self.hidden, self.rstd_f = nb(d), nb(1, torch.float32)
        # 5. the layers
        for i in range(Ln):
            self.layer_forward(i)
        # 6. final norm (the LayerScale form normalised for it in the last layer's residual kernel)
        if f["final_norm"] == "own-launch":
            self.ck(lib.gget_op_rmsnorm_fwd(self.x[Ln].p, self.w("model.norm.weight"), self.hidden.p, self.rstd_f.p, T, d, eps, ST()))
        # 7. head, 8. loss
        Cn = spec.num_labels
        self.logits, self.dlogits = Buf(B, Cn, torch.float32), Buf(B, Cn, torch.float32)
        self.pooled = Buf(B, d, BF)
        self.loss = Buf(1, 1, torch.float32)
        bias = self.w("score.bias") if spec.score_bias else None
        self.ck(lib.gget_op_score_fwd(self.hidden.p, P(self.pool_row), self.w("score.weight"), bias, self.logits.p, self.pooled.p, B, Cn, d, ST()))
        self.ck(lib.gget_op_task_loss(self.logits.p, P(labels), P(wgt), self.problem, B, Cn, self.loss.p, self.dlogits.p, ST()))
        # (a wrong caller's count would poison the loss - k_poison_loss, no entry: the replay is given the right count and says so)
        torch.cuda.synchronize()
        if varlen:
            assert int(self.vl_status[0]) == 0, "the replay was handed a token count that is not the mask's"
        return self

    def layer_forward(self, i):
        spec, lib, f, T, B, S = self.spec, self.lib, self.f, self.T, self.B, self.S
        d, ff, H = spec.hidden_size, spec.intermediate_size, spec.num_heads
        eps, causal = float(spec.rms_eps), int(spec.causal)
        p = f"model.layers.{i}."
        w, x_in, x_out = self.lw[i], self.x[i], self.x[i + 1]
        fused_ls = f["attn_fwd"] == "ls-residual"
        if not (fused_ls and i > 0):     # (the LayerScale form: the residual kernel of the layer below normalised this layer's input)
            self.ck(lib.gget_op_rmsnorm_fwd(x_in.p, self.w(p + "input_layernorm.weight"), w["xn1"].p, w["rstd1"].p, T, d, eps, ST()))
        self.ck(lib.gget_op_qkv_rope(w["xn1"].p, self.w(p + "self_attn.q_proj.weight"), w["qkv"].p, P(self.cos), P(self.sin), P(self.pos_rows),
                                     T, S, d, ST()))
        self.audit_qkv(i)
        taken = C.c_int32(0)
        if f["attn_fwd"] == "per-sample":
            self.ck(lib.gget_op_attn_oproj_fwd(w["qkv"].p, P(self.key_len), P(self.row_base), w["attn"].p, w["lse"].p, self.wo_pack.at(i * d * d),
                                               x_in.p, w["xmid"].p, self.w(p + "post_attention_layernorm.weight"), w["xn2"].p, w["rstd2"].p,
                                               B, S, H, causal, eps, 0.0, self.attn_seed(i), ST(), C.byref(taken)))
            assert taken.value == 1, f"layer {i}: the mirror says per-sample forward, the launcher did not take it"
            self.gateup(i)
            self.gemm(NT, EPI_RES, w["h"].p, self.w(p + "mlp.down_proj.weight"), x_out.p, w["xmid"].p, T, d, ff, ff, ff, d)
            self.audit_gemm(f"down+residual L{i}", NT, w["h"].body(), self.wt(p + "mlp.down_proj.weight").view(d, ff), x_out.body(), ff, R=w["xmid"].body())
            return
        if self.row_base is None:
            self.ck(lib.gget_op_attn_fwd(w["qkv"].p, P(self.key_len), w["attn"].p, w["lse"].p, B, S, H, causal, None, None, None, 0.0,
                                         self.attn_seed(i), ST()))
        else:
            self.ck(lib.gget_op_attn_fwd_varlen(w["qkv"].p, P(self.key_len), P(self.row_base), w["attn"].p, w["lse"].p, B, S, H, causal, None, None,
                                                None, 1, 0.0, self.attn_seed(i), ST()))
        wo = self.w(p + "self_attn.o_proj.weight")
        if fused_ls:
            Ln = spec.num_layers
            lam1 = self.w(p + "lambda_1") if spec.layer_scale_init > 0 else None
            lam2 = self.w(p + "lambda_2") if spec.layer_scale_init > 0 else None
            self.gemm(NT, EPI_NONE, w["attn"].p, wo, w["araw"].p, None, T, d, d, d, d, d)
            self.audit_gemm(f"o L{i}", NT, w["attn"].body(), self.wt(p + "self_attn.o_proj.weight").view(d, d), w["araw"].body(), d)
            self.ck(lib.gget_op_ls_rmsnorm_fwd_drop(x_in.p, w["araw"].p, lam1, w["xmid"].p, self.w(p + "post_attention_layernorm.weight"),
                                                    w["xn2"].p, w["rstd2"].p, T, d, eps, 0.0, 0, None, *self.path(i, 0), ST()))
            self.gateup(i)
            ep = self.elem(i)
            self.ck(lib.gget_op_elem_dropout(w["h"].p, T, ff, 49, *ep, ST()))       # mlp_act_dropout (stream 49)
            self.gemm(NT, EPI_NONE, w["h"].p, self.w(p + "mlp.down_proj.weight"), w["mraw"].p, None, T, d, ff, ff, ff, d)
            self.audit_gemm(f"down L{i}", NT, w["h"].body(), self.wt(p + "mlp.down_proj.weight").view(d, ff), w["mraw"].body(), ff)
            last = i + 1 == Ln
            nw = self.w("model.norm.weight") if last else self.w(f"model.layers.{i + 1}.input_layernorm.weight")
            nxn = self.hidden if last else self.lw[i + 1]["xn1"]
            nrs = self.rstd_f if last else self.lw[i + 1]["rstd1"]
            self.ck(lib.gget_op_ls_rmsnorm_fwd_drop(w["xmid"].p, w["mraw"].p, lam2, x_out.p, nw, nxn.p, nrs.p, T, d, eps, *ep, *self.path(i, 1), ST()))
            return
        self.gemm(NT, EPI_RES, w["attn"].p, wo, w["xmid"].p, x_in.p, T, d, d, d, d, d)
        self.audit_gemm(f"o+residual L{i}", NT, w["attn"].body(), self.wt(p + "self_attn.o_proj.weight").view(d, d), w["xmid"].body(), d, R=x_in.body())
        self.ck(lib.gget_op_rmsnorm_fwd(w["xmid"].p, self.w(p + "post_attention_layernorm.weight"), w["xn2"].p, w["rstd2"].p, T, d, eps, ST()))
        self.gateup(i)
        self.gemm(NT, EPI_RES, w["h"].p, self.w(p + "mlp.down_proj.weight"), x_out.p, w["xmid"].p, T, d, ff, ff, ff, d)
        self.audit_gemm(f"down+residual L{i}", NT, w["h"].body(), self.wt(p + "mlp.down_proj.weight").view(d, ff), x_out.body(), ff, R=w["xmid"].body())

    def gateup(self, i):
        spec, w = self.spec, self.lw[i]
        d, ff = spec.hidden_size, spec.intermediate_size
        self.ck(self.lib.gget_op_gateup_geglu(w["xn2"].p, self.w(f"model.layers.{i}.mlp.gate_proj.weight"), w["gu"].p, w["h"].p, self.T, d, ff, ST()))
        if self.audit:
            wgu = self.P_[self.off[f"model.layers.{i}.mlp.gate_proj.weight"][0]:][:2 * ff * d].view(2 * ff, d)
            self.audit_gemm(f"gate|up L{i}", NT, w["xn2"].body(), wgu, w["gu"].body(), d)
            gu = w["gu"].body().double()
            gate, up = gu[:, :ff], gu[:, ff:]
            ref = 0.5 * gate * (1.0 + torch.erf(gate / 2.0 ** 0.5)) * up
            # (layer_forward_fused of tests/test_gpu_gemm_exact.py: two roundings of the gated product of the gate | up bits written)
            self._aud(f"geglu h L{i}", w["h"].body(), ref, 2.0 * UB * ref.abs() + 2.0 ** -20 * (1 + gate.abs()) * up.abs())

    def audit_qkv(self, i):
        if not self.audit:
            return
        d, w = self.spec.hidden_size, self.lw[i]
        wq = self.P_[self.off[f"model.layers.{i}.self_attn.q_proj.weight"][0]:][:3 * d * d].view(3 * d, d)
        ref, ab = self._dot64(NT, w["xn1"].body(), wq)
        T = self.T
        pos = self.pos_rows[:T].clamp(0, self.max_position - 1)
        c = self.cos.double()[pos][:, None, :].repeat(1, 1, 2)
        s = self.sin.double()[pos][:, None, :].repeat(1, 1, 2)
        hq, ha = ref[:, :2 * d].reshape(T, 2 * d // 64, 64), ab[:, :2 * d].reshape(T, 2 * d // 64, 64)
        rot = torch.cat((-hq[..., 32:], hq[..., :32]), -1)
        rot_a = torch.cat((ha[..., 32:], ha[..., :32]), -1)
        ref = torch.cat(((hq * c + rot * s).reshape(T, 2 * d), ref[:, 2 * d:]), 1)
        ab = torch.cat(((ha * c.abs() + rot_a * s.abs()).reshape(T, 2 * d), ab[:, 2 * d:]), 1)
        # (the q | k columns: the rotation's two products and sum, 2^-20 of the largest projection as the RoPE check of test_gpu_gemm_exact.py)
        real = self.tc
        self._aud(f"q|k|v + RoPE L{i}", w["qkv"].body()[:real], ref[:real], (UB * ref.abs() + 2.0 * d * U * ab + 2.0 ** -20 * ref.abs().max())[:real])

    # ---------------------------------------------------------------- backward
    def backward(self):
        spec, lib, f, T, B, S = self.spec, self.lib, self.f, self.T, self.B, self.S
        d, ff, H, Ln, F = spec.hidden_size, spec.intermediate_size, spec.num_heads, spec.num_layers, spec.stacked_feat
        tc = self.tc
        nb = lambda cols, dt=BF: Buf(T, cols, dt, real=tc)   # noqa: E731
        # what the backward relies on being clear (engine.hip: ONE k_zero_ranges launch): the fp32 accumulators, the gradient of the
        # final-norm output (the head writes the pooled rows only) and, var-len layout, the q|k|v gradient rows behind the last sample
        self.s32 = torch.zeros(self.n_s32 + 128, dtype=torch.float32, device="cuda")
        self.dx = {"a": nb(d), "b": Buf(T, d, BF, zero=True), "c": nb(d)}
        self.dxn, self.dqkv, self.dattn, self.dgu, self.dh = nb(d), nb(3 * d), nb(d), nb(2 * ff), nb(ff)
        self.delta = Buf(B * S, H, torch.float32)
        self.dsc, self.dsc2 = nb(d), nb(d)
        self.wg32 = Buf(3 * 4 * d, d, torch.float32)
        Cn = spec.num_labels
        dhid, dx0 = self.dx["b"], self.dx["a"]
        stride = align_up(d, 128)
        # 9. head backward
        self.ck(lib.gget_op_score_bwd(self.dlogits.p, self.hidden.p, P(self.pool_row), self.w("score.weight"), self.s("score.weight"),
                                      self.s("score.bias") if spec.score_bias else None, dhid.p, B, Cn, d, ST()))
        self.note_score()
        # 10. final-norm backward
        xl = self.x[Ln]
        self.note_norm("model.norm.weight", dhid, xl, self.rstd_f)
        if f["final_norm_bwd"] == "dw-only":
            self.ck(lib.gget_op_rmsnorm_dw(dhid.p, xl.p, self.rstd_f.p, self.s("model.norm.weight"), T, d, ACCUM_COPIES, stride, ST()))
        elif f["final_norm_bwd"] == "fused-ls2":
            li = Ln - 1
            lam2 = f"model.layers.{li}.lambda_2"
            has_ls = spec.layer_scale_init > 0
            self.ck(lib.gget_op_rmsnorm_bwd_ls_drop(dhid.p, xl.p, self.w("model.norm.weight"), self.rstd_f.p, None, dx0.p, self.s("model.norm.weight"),
                                                    self.lw[li]["mraw"].p, self.w(lam2) if has_ls else None, self.dsc.p,
                                                    self.s(lam2) if has_ls else None, T, d, *self.elem(li), *self.path(li, 1), ST()))
            self.note_lam(lam2, dx0, self.lw[li]["mraw"], li, 1)
        else:
            self.ck(lib.gget_op_rmsnorm_bwd_copies(dhid.p, xl.p, self.w("model.norm.weight"), self.rstd_f.p, None, dx0.p, self.s("model.norm.weight"),
                                                   T, d, ACCUM_COPIES, stride, ST()))
        self.ls2_done = f["final_norm_bwd"] == "fused-ls2"
        self.convert(0)
        # 11. the layers
        for i in range(Ln - 1, f["first_layer"] - 1, -1):
            self.layer_backward(i)
            self.convert(bucket_of(i, Ln))
        # 12. embedding backward
        if f["embed_bwd"] != "none":
            last = f["rotation"][0][2]
            gated = spec.gated_agg
            self.note_embed(self.dx[last])
            self.ck(lib.gget_op_embed_bwd(P(self.ids_rows), self.dx[last].p, self.w("model.embed_tokens.weight"),
                                          self.w("stacked_feat_agg.weight") if gated else None, self.s("model.embed_tokens.weight"),
                                          self.s("stacked_feat_agg.weight") if gated else None, T, F, F, d, spec.vocab_size, spec.pad_token_id, ST()))
            self.convert(Ln + 1)
        torch.cuda.synchronize()
        return self

    def convert(self, bucket):
        """13. fp32 replicas -> bf16, per bucket as the staged backward does it (the monolithic backward converts the same segments in one
        launch at the end: the segments are disjoint, the bits are the same)."""
        rows = self.segs[bucket]
        if not rows:
            return
        tab = torch.tensor(rows, dtype=torch.int64, device="cuda").reshape(-1)
        self._keep = getattr(self, "_keep", []) + [tab]
        self.ck(self.lib.gget_op_convert_segments(P(self.s32), self.G.p, P(tab), len(rows), ST()))

    def layer_backward(self, i):
        spec, lib, f, T, B, S = self.spec, self.lib, self.f, self.T, self.B, self.S
        d, ff, H = spec.hidden_size, spec.intermediate_size, spec.num_heads
        causal = int(spec.causal)
        p = f"model.layers.{i}."
        w = self.lw[i]
        has_ls = spec.layer_scale_init > 0
        has_res = f["attn_fwd"] == "ls-residual"
        o, m, n_ = f["rotation"][i]
        dx_out, dx_mid, dx_in = self.dx[o], self.dx[m], self.dx[n_]
        x_in = self.x[i]
        stride = align_up(d, 128)
        ln1, ln2 = p + "input_layernorm.weight", p + "post_attention_layernorm.weight"
        dy_down = dx_out
        if has_res:
            if not self.ls2_done:
                self.ck(lib.gget_op_ls_bwd(dx_out.p, w["mraw"].p, self.w(p + "lambda_2") if has_ls else None, self.dsc.p,
                                           self.s(p + "lambda_2") if has_ls else None, T, d, *self.elem(i), *self.path(i, 1), ST()))
                self.note_lam(p + "lambda_2", dx_out, w["mraw"], i, 1)
            self.ls2_done = False
            dy_down = self.dsc
        wdown = self.w(p + "mlp.down_proj.weight")
        if self.opt["mlp_p"] > 0:
            self.gemm(NN, EPI_NONE, dy_down.p, wdown, self.dh.p, None, T, ff, d, d, ff, ff)
            self.ck(lib.gget_op_elem_dropout(self.dh.p, T, ff, 49, *self.elem(i), ST()))
            self.ck(lib.gget_op_geglu_bwd(w["gu"].p, self.dh.p, self.dgu.p, T, ff, ST()))
        else:
            self.ck(lib.gget_op_down_dgrad_geglu(dy_down.p, wdown, w["gu"].p, self.dgu.p, self.dh.p, T, d, ff, ST()))
            self.audit_geglu_bwd(i, dy_down)
        self.gemm(NN, EPI_NONE, self.dgu.p, self.w(p + "mlp.gate_proj.weight"), self.dxn.p, None, T, d, 2 * ff, 2 * ff, d, d)
        taken = C.c_int32(0)
        dy_o = dx_mid
        self.note_norm(ln2, self.dxn, w["xmid"], w["rstd2"])
        if f["attn_bwd"].startswith("per-sample"):
            args = (self.dxn.p, w["xmid"].p, self.w(ln2), w["rstd2"].p, dx_out.p, dx_mid.p, self.s(ln2), ACCUM_COPIES, stride, self.wot_pack.at(i * d * d),
                    w["qkv"].p, w["lse"].p, P(self.key_len), P(self.row_base), self.dqkv.p, B, S, H, causal, P(self.cos), P(self.sin), P(self.pos_safe),
                    0.0, self.attn_seed(i), T, ST(), C.byref(taken), self.dattn.p)
            if self.row_base is None:
                self.ck(lib.gget_op_attn_oproj_bwd(*args))
            else:
                self.ck(lib.gget_op_attn_oproj_bwd_list(*args, P(self.long_list)))
            assert taken.value == 1, f"layer {i}: the mirror says per-sample backward, the launcher did not take it"
        else:
            if has_res:
                self.ck(lib.gget_op_rmsnorm_bwd_ls_drop(self.dxn.p, w["xmid"].p, self.w(ln2), w["rstd2"].p, dx_out.p, dx_mid.p, self.s(ln2), w["araw"].p,
                                                        self.w(p + "lambda_1") if has_ls else None, self.dsc2.p,
                                                        self.s(p + "lambda_1") if has_ls else None, T, d, 0.0, 0, None, *self.path(i, 0), ST()))
                self.note_lam(p + "lambda_1", dx_mid, w["araw"], i, 0)
                dy_o = self.dsc2
            else:
                self.ck(lib.gget_op_rmsnorm_bwd_copies(self.dxn.p, w["xmid"].p, self.w(ln2), w["rstd2"].p, dx_out.p, dx_mid.p, self.s(ln2), T, d,
                                                       ACCUM_COPIES, stride, ST()))
            self.gemm(NN, EPI_NONE, dy_o.p, self.w(p + "self_attn.o_proj.weight"), self.dattn.p, None, T, d, d, d, d, d)
            self.ck(lib.gget_op_attn_bwd_rotated(w["qkv"].p, w["attn"].p, self.dattn.p, w["lse"].p, P(self.key_len), P(self.row_base), self.dqkv.p,
                                                 self.delta.p, B, S, H, causal, P(self.cos), P(self.sin), P(self.pos_safe), 0.0, self.attn_seed(i),
                                                 None, 0, P(self.long_list), ST()))
        if self.f["layout"] == "varlen" and T > self.tc:
            # the pad-row rule: the q|k|v gradient rows behind the last sample are written by nobody (cleared at the start of the backward)
            pad = self.dqkv.body()[self.tc:]
            assert bool((pad.view(torch.int16) == 0).all()), f"layer {i}: a q|k|v gradient row behind the last sample was written"
        self.gemm(NN, EPI_NONE, self.dqkv.p, self.w(p + "self_attn.q_proj.weight"), self.dxn.p, None, T, d, 3 * d, 3 * d, d, d)
        form = f["ln1_bwd"][i]
        self.note_norm(ln1, self.dxn, x_in, w["rstd1"])
        if form == "dw-only":
            self.ck(lib.gget_op_rmsnorm_dw(self.dxn.p, x_in.p, w["rstd1"].p, self.s(ln1), T, d, ACCUM_COPIES, stride, ST()))
        elif form == "plain":
            self.ck(lib.gget_op_rmsnorm_bwd_copies(self.dxn.p, x_in.p, self.w(ln1), w["rstd1"].p, dx_mid.p, dx_in.p, self.s(ln1), T, d, ACCUM_COPIES,
                                                   stride, ST()))
        # the weight gradients (dW = dY^T X, K = T): all four pairs are still alive
        prob = {"gu": (self.dgu, w["xn2"], p + "mlp.gate_proj.weight", 2 * ff, d), "dn": (dy_down, w["h"], p + "mlp.down_proj.weight", d, ff),
                "qkv": (self.dqkv, w["xn1"], p + "self_attn.q_proj.weight", 3 * d, d), "o": (dy_o, w["attn"], p + "self_attn.o_proj.weight", d, d)}

        def grouped(keys):
            n = len(keys)
            PA, IA = C.c_void_p * n, C.c_int32 * n
            A = PA(*[prob[k][0].p.value for k in keys])
            Bm = PA(*[prob[k][1].p.value for k in keys])
            return A, Bm, IA(*[prob[k][3] for k in keys]), IA(*[prob[k][4] for k in keys]), IA(*[T] * n), IA(*[prob[k][3] for k in keys]), \
                IA(*[prob[k][4] for k in keys]), IA(*[prob[k][4] for k in keys]), PA, n

        if f["wgrad"] == "grouped-4":
            keys = ["gu", "dn", "qkv", "o"]
            A, Bm, M, N, K, lda, ldb, ldc, PA, n = grouped(keys)
            Cs = PA(*[self.g(prob[k][2]).value for k in keys])
            self.ck(lib.gget_op_gemm_grouped(TN, n, A, Bm, Cs, M, N, K, lda, ldb, ldc, ST()))
        else:
            keys = ["gu", "dn"]
            A, Bm, M, N, K, lda, ldb, ldc, PA, n = grouped(keys)
            Cs = PA(*[self.g(prob[k][2]).value for k in keys])
            self.ck(lib.gget_op_gemm_grouped(TN, n, A, Bm, Cs, M, N, K, lda, ldb, ldc, ST()))
            split = qkvo_split(T)
            assert split == L.slab_plan(L.SLAB_PLAN_QKVO, d, spec.vocab_size, T), "the mirror's K-slice rule is not the launcher's"
            slab = 4 * d * d
            keys2 = ["qkv", "o"]
            A, Bm, M, N, K, lda, ldb, ldc, PA, n = grouped(keys2)
            Cs = PA(self.wg32.p.value, self.wg32.at(3 * d * d).value)
            self.ck(lib.gget_op_gemm_grouped_slab(TN, n, A, Bm, Cs, M, N, K, lda, ldb, ldc, slab, split, ST()))
            self.ck(lib.gget_op_slab_reduce(self.wg32.p, slab, split, self.g(p + "self_attn.q_proj.weight"), 4 * d * d, 0, ST()))
        if self.audit:
            real = slice(0, T)
            for k in ("gu", "dn", "qkv", "o"):
                dy, xx, name, M_, N_ = prob[k]
                o_, _, _ = self.off[name]
                got = self.G.t[o_:o_ + M_ * N_].view(M_, N_)
                slabbed = f["wgrad"] != "grouped-4" and k in ("qkv", "o")
                # (grouped launch: check_grouped_random's c_acc = 1; the slab launch + reduce: check_single's 1 + live slices, and the bf16
                #  rounding of the reduce pass)
                self.audit_gemm(f"wgrad {k} L{i}" + (" (slab + reduce)" if slabbed else ""), TN, dy.body()[real], xx.body()[real], got, T,
                                c_acc=(1.0 + qkvo_split(T)) if slabbed else 1.0)
        if form == "fuse_next":
            pl = f"model.layers.{i - 1}."
            # behind the weight gradients: this launch overwrites dscaled, which the down_proj weight gradient above has just read
            self.ck(lib.gget_op_rmsnorm_bwd_ls_drop(self.dxn.p, x_in.p, self.w(ln1), w["rstd1"].p, dx_mid.p, dx_in.p, self.s(ln1), self.lw[i - 1]["mraw"].p,
                                                    self.w(pl + "lambda_2") if has_ls else None, self.dsc.p,
                                                    self.s(pl + "lambda_2") if has_ls else None, T, d, *self.elem(i - 1), *self.path(i - 1, 1), ST()))
            self.note_lam(pl + "lambda_2", dx_in, self.lw[i - 1]["mraw"], i - 1, 1)
            self.ls2_done = True

    def audit_geglu_bwd(self, i, dy_down):
        if not self.audit:
            return
        spec, w = self.spec, self.lw[i]
        d, ff = spec.hidden_size, spec.intermediate_size
        wd = self.wt(f"model.layers.{i}.mlp.down_proj.weight").view(d, ff)
        dh, ab = self._dot64(NN, dy_down.body(), wd)
        gu = w["gu"].body().double()
        gate, up = gu[:, :ff], gu[:, ff:]
        gelu = 0.5 * gate * (1.0 + torch.erf(gate / 2.0 ** 0.5))
        gelu_g = 0.5 * (1.0 + torch.erf(gate / 2.0 ** 0.5)) + gate * torch.exp(-0.5 * gate * gate) / (2.0 * torch.pi) ** 0.5
        # dh is rounded to bf16 inside the launch as the un-fused GEMM's output is: its single-launch bound (2^-8 |dh| + 2 K u |dy| |W|),
        # carried through the two products of layer_forward_fused's bound (1.25 x 2^-8, 2^-20 of the factors)
        dh_b = UB * dh.abs() + 2.0 * d * U * ab
        got = self.dgu.body()
        fg, fu = up * gelu_g, gelu
        self._aud(f"dh + GEGLU' (gate) L{i}", got[:, :ff], dh * fg, dh_b * fg.abs() * (1 + 1.25 * UB) + 1.25 * UB * (dh * fg).abs()
                  + 2.0 ** -20 * (dh.abs() + dh_b) * up.abs() * (1 + gate.abs()))
        self._aud(f"dh + GEGLU' (up) L{i}", got[:, ff:], dh * fu, dh_b * fu.abs() * (1 + 1.25 * UB) + 1.25 * UB * (dh * fu).abs()
                  + 2.0 ** -20 * (dh.abs() + dh_b) * (1 + gate.abs()))

    # ---------------------------------------------------------------- the sums that are not owed equality, in float64
    def note(self, name, terms_sum, terms_abs, n):
        """One stage's share of an accumulated gradient: the float64 sum of its terms, of their magnitudes, and how many there are."""
        if name not in self.inexact:
            return
        r, a, k = self.sums.get(name, (0.0, 0.0, 0))
        self.sums[name] = (r + terms_sum.reshape(-1), a + terms_abs.reshape(-1), k + n)

    def note_norm(self, name, dy, x, rstd):
        """RMSNorm weight gradient: dw[j] = sum over the rows of dy[t, j] x[t, j] rstd[t] (tests/_rows_ref.py _bwd_ref)."""
        if name in self.inexact:
            t = dy.body().double() * x.body().double() * rstd.body().double()
            self.note(name, t.sum(0), t.abs().sum(0), self.T)

    def note_lam(self, name, dx, y, layer, which):
        """LayerScale vector of branch `which` of `layer`: dlam[j] = sum over the rows of keep_b dx[t, j] bf16(y[t, j] em[t, j]) with the DropPath
        multiplier keep_b of the row's sample and - MLP branch - the mlp_dropout multiplier em (tests/_drop_ref.py _dlam_terms and its Python
        twins of the two hashes)."""
        if name not in self.inexact:
            return
        import numpy as np

        import _drop_ref as D
        T, d = self.T, self.spec.hidden_size
        if self.f["layout"] == "varlen":
            rows, sample = self.c2p[:T].cpu().numpy(), self.rowb[:T].cpu().numpy()
        else:
            rows = np.arange(T)
            sample = rows // self.S
        rate, pseed, _, _ = self.path(layer, which)
        keep = torch.from_numpy(D.path_keep(pseed, sample, rate)).double().cuda()
        yv = y.body().float()
        if which == 1 and self.opt["mlp_p"] > 0:
            ep, eseed, _ = self.elem(layer)
            em = torch.from_numpy(D.elem_keep(eseed, D.STREAM_MLP_OUT, rows[:, None], np.arange(d)[None, :], ep)).cuda()
            yv = (yv * em).to(BF).float()
        t = keep[:, None] * dx.body().double() * yv.double()
        self.note(name, t.sum(0), t.abs().sum(0), T)

    def note_score(self):
        dl = self.dlogits.body().double()
        h = self.hidden.body().double()[self.pool_row[:self.B].long()]
        self.note("score.weight", dl.t() @ h, dl.abs().t() @ h.abs(), self.B)
        if self.spec.score_bias:
            self.note("score.bias", dl.sum(0), dl.abs().sum(0), self.B)

    def note_embed(self, dx):
        """Sorted embedding backward: dE[v] = sum over the cells (t, f) with ids[t, f] = v != pad of g[f] dx[t] (g the gate row, or 1);
        dgate[f] = sum over those cells of dx[t] E[v]."""
        spec, T = self.spec, self.T
        F, d, V = spec.stacked_feat, spec.hidden_size, spec.vocab_size
        if "model.embed_tokens.weight" not in self.inexact:
            return
        ids = self.ids_rows[:T * F].view(T, F)
        dxv = dx.body().double()
        emb = self.wt("model.embed_tokens.weight").view(V, d).double()
        gate = self.wt("stacked_feat_agg.weight").view(F, d).double() if spec.gated_agg else None
        ref, ab = torch.zeros(V, d, dtype=torch.float64, device="cuda"), torch.zeros(V, d, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(V, dtype=torch.float64, device="cuda")
        gr, ga = torch.zeros(F, d, dtype=torch.float64, device="cuda"), torch.zeros(F, d, dtype=torch.float64, device="cuda")
        for fi in range(F):
            live = ids[:, fi] != spec.pad_token_id
            idv = ids[live, fi]
            term = dxv[live] * (gate[fi] if gate is not None else 1.0)
            ref.index_add_(0, idv, term)
            ab.index_add_(0, idv, term.abs())
            cnt.index_add_(0, idv, torch.ones_like(idv, dtype=torch.float64))
            if gate is not None:
                tg = dxv[live] * emb[idv]
                gr[fi], ga[fi] = tg.sum(0), tg.abs().sum(0)
        self.note("model.embed_tokens.weight", ref, ab, int(cnt.max()) + 1)
        if gate is not None:
            self.note("stacked_feat_agg.weight", gr, ga, T)

    def check_bounded(self, engine_grads, which="engine"):
        """The tensors that are not owed equality, against the float64 sums noted above: {name: (ratio, failure or None)}."""
        out = {}
        for name in self.inexact:
            if name not in self.sums:
                continue
            ref, ab, n = self.sums[name]
            out[name] = held_sum(f"{which} {name} [{self.inexact[name]}]", engine_grads[name].float().cuda().reshape(-1), ref, ab, n)
        return out
