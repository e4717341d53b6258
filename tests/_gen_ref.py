"""numpy twin of the generation-evaluation kernels (csrc/generation.hip) and of the schedules around them: the ranked reveal as a
lexsort over the masked cells, the batch step rule, the per-example schedule and the accuracy counts.  Test infrastructure: the
kernels are compared with this, and this is compared with the reference's recorded runs (tests/golden/gen_eval.npz) and with the
torch statement of the rule (generation.unmask_step / reveal_counts)."""
import numpy as np
import torch


def n_reveal(n_masked: int, p) -> int:
    """floor(n_masked * p) with ONE fp32 multiply: torch.floor(n_masked * p).int() and int(num_mask_token * (1 - s / t))."""
    return int(np.floor(np.float32(n_masked) * np.float32(p)))


def ranked_reveal(x, conf, cand, mask_id, p):
    """x i64 [B, N], conf f32 [B, N], cand i64 [B, N]; p a scalar or [B].  Every sample writes cand into its n_reveal most confident
    MASKED cells, ties to the lower cell index (-0.0 == +0.0 as floats).  Returns (new x, n_revealed i32 [B])."""
    x = np.array(x, dtype=np.int64, copy=True)
    conf = np.asarray(conf, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    B = x.shape[0]
    p = np.broadcast_to(np.asarray(p, dtype=np.float32).reshape(-1), (B,))
    n_out = np.zeros(B, np.int32)
    for b in range(B):
        idx = np.nonzero(x[b] == mask_id)[0]
        n = min(max(n_reveal(len(idx), p[b]), 0), len(idx))
        n_out[b] = n
        if n == 0:
            continue
        order = np.lexsort((idx, -conf[b, idx]))          # primary: confidence descending; secondary: index ascending
        take = idx[order[:n]]
        x[b, take] = cand[b, take]
    return x, n_out


def step_p_table(timesteps):
    """p of every step of one time grid, fp32: 1 - t[i+1] / t[i], the last entry 1.0 (reference generation_utils.py:177-178)."""
    ts = np.asarray(timesteps, dtype=np.float32)
    p = np.float32(1.0) - ts[1:] / ts[:-1]
    if p.size:
        p[-1] = np.float32(1.0)
    return p.astype(np.float32)


def plan_rule(max_n_masked: int, p_tab, i: int):
    """The batch step rule (reference :171-184) from the batch maximum of the masked counts: returns (i, p of the last rule
    iteration or 0 when none ran, any cell masked)."""
    p_last = np.float32(0.0)
    if max_n_masked > 0:
        while i < len(p_tab):
            p_last = np.float32(p_tab[i])
            i += 1
            if n_reveal(max_n_masked, p_last) >= 1:
                break
    return i, p_last, max_n_masked > 0


def batch_step(x, conf, cand, p_tab, i, mask_id):
    """One update of `sample_per_batch`'s ranked algorithms: the step rule, then the reveal.  Returns (new x, i)."""
    x = np.asarray(x)
    i, p, _ = plan_rule(int((x == mask_id).sum(axis=1).max()) if x.size else 0, p_tab, i)
    return ranked_reveal(x, conf, cand, mask_id, p)[0], i


def example_p_table(n_masked, steps, eps):
    """fp32 [max_b steps_b, B]: sample b walks linspace(1, eps, steps_b + 1) with steps_b = min(n_masked[b], steps) (reference
    :350-354; torch.linspace is the reference's definition of the grid), p = 0 once it has finished."""
    steps_b = [min(int(n), int(steps)) for n in n_masked]
    tab = np.zeros((max(steps_b, default=0), len(steps_b)), np.float32)
    for b, sb in enumerate(steps_b):
        if sb > 0:
            tab[:sb, b] = step_p_table(torch.linspace(1, eps, sb + 1).numpy())
    return tab


def per_example_loop(x0, mask_id, steps, eps, conf_fn):
    """The per-example schedule on a batch: conf_fn(it, x) -> (conf [B, N], cand [B, N]) of iteration `it`.  Returns (x, history)."""
    x = np.array(x0, dtype=np.int64, copy=True)
    tab = example_p_table((x == mask_id).sum(axis=1), steps, eps)
    hist = []
    for it in range(tab.shape[0]):
        conf, cand = conf_fn(it, x)
        x, _ = ranked_reveal(x, conf, cand, mask_id, tab[it])
        hist.append(x.copy())
    return x, hist


def acc_counts(gen, labels, ids, mask_id):
    """i32 [B, 2]: per sample {sum (gen == labels) & (ids == mask), sum (ids == mask)} (reference :448-463)."""
    B = np.asarray(ids).shape[0]
    gen, labels, ids = (np.asarray(a).reshape(B, -1) for a in (gen, labels, ids))
    m = ids == mask_id
    return np.stack([((gen == labels) & m).sum(axis=1), m.sum(axis=1)], axis=1).astype(np.int32)


def acc_from_counts(c):
    """float / float as torch divides them: 0 / 0 = NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return c[:, 0].astype(np.float32) / c[:, 1].astype(np.float32)
