"""use_bn AdaBN / AutoDIAL at the column and row counts the two BatchNorm launches branch on (ta3n_amd/csrc/ta3n_pointwise.hip:
bn_shared_fwd_kernel, bn_shared_bwd_kernel), as one table shared by tests/test_bn_shapes_cpu.py (inputs and plan, no GPU) and
tests/test_gpu_bn_shapes.py (the kernels).  The pattern, the hyper-parameters and most helpers are those of tests/limit_shapes.py.

What the launches branch on, and what `bn_facts` / `assert_runs_what_it_claims` read back from the PLAN for every case:
  * the column-group count ceil(F / 4) (one workgroup = BN_COLS = 4 columns of one domain).  Where it is a multiple of 64, i.e.
    fc_dim % 256 == 0, bn_column_group DEALS the workgroups over the groups (a permutation; it indexes the statistics, the affine pair,
    the eval-mode target statistics, the dropout counter, the twin stores and the sum-of-squares slot); otherwise launch order.
  * per domain, whether its rows (videos x segments) stay in registers between the passes (rows <= BN_THREADS x BN_KEEP = 5 120) or
    are streamed; inside the kept branch, the register rows per lane (tid + j x 1 024 < rows) and partly filled waves.
  * whether the step is the fused list or the unfused lists (fc_dim > 2048).
A case that silently lands on another branch is worth nothing.

Inputs: limit_shapes' (weights synth_state(seed=wseed, scale="trained"), batches synth_batch(seed=xseed + 7 step), beta, gamma, clip 20, no
dropout unless a test says so), with two additions.  synth_state leaves every BatchNorm weight at 1 and bias at 0, which a launch that read
the WRONG column's affine pair would reproduce: `initial_params` draws bn_shared_{S,T}.weight in 1 +- 0.25 and the biases in +- 0.2, different
per domain.  And the running statistics start from `initial_running` (means +- 0.3, variances 0.5 .. 1.5) instead of nn.BatchNorm1d's 0 / 1,
so that a column a launch leaves unwritten cannot pass as untouched."""
import functools

import numpy as np
import torch

import limit_shapes as ls
from limit_shapes import BETA, CLIP, GAMMA, LR      # noqa: F401 (the tests read them from here)
from oracle import ta3n_oracle as orc
from plan_interp import BN_COLS, PH_BN_BWD, PH_BN_FWD, plan_arrays
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_state

BN_THREADS = 1024      # ta3n_pointwise.hip: BN_THREADS - row lanes of a BatchNorm workgroup
BN_KEEP = 5            # ta3n_pointwise.hip: BN_KEEP - rows per lane that stay in registers (rows <= BN_THREADS * BN_KEEP: kept, else streamed)
BN_DEAL = 64           # ta3n_pointwise.hip: bn_column_group deals the workgroups where the group count is a multiple of this
HEADS_MAX_F = ls.HEADS_MAX_F
SHARED_BIAS = "fc_feature_shared_source.bias"      # in front of a BatchNorm: zero gradient in exact arithmetic
BN_PARAMS = ("bn_shared_S.weight", "bn_shared_S.bias", "bn_shared_T.weight", "bn_shared_T.bias")


def _case(Bs, Bt, T, D, F, C, why, use_bn=("AdaBN",), unfused_bn=(), **kw):
    """limit_shapes._case plus use_bn: the options the fused step runs with, and those the unfused lists run with as well."""
    c = ls._case(Bs, Bt, T, D, F, C, why, **kw)
    c.update(use_bn=tuple(use_bn), unfused_bn=tuple(unfused_bn))
    return c


BOTH = ("AdaBN", "AutoDIAL")
# Narrow launches first, the tall batches last (the order the GPU tests run in).
CASES = {
    "bn_n2_F36": _case(1, 1, 2, 40, 36, 5, "2 rows per domain (the fewest train-mode BatchNorm takes); 9 groups, launch order, one partly filled wave"),
    "bn_F256": _case(3, 2, 3, 256, 256, 7, "64 groups: the smallest dealt launch", use_bn=BOTH, unfused_bn=BOTH, arithmetics=True),
    "bn_F260": _case(3, 2, 3, 264, 260, 7, "65 groups: launch order again, one past the dealt count"),
    "bn_F512": _case(6, 4, 5, 512, 512, 12, "128 groups: the column count the benchmark's use_bn variant runs", arithmetics=True),
    "bn_F768": _case(4, 3, 3, 768, 768, 7, "192 = 3 x 64 groups: dealt with a group count that is no power of two"),
    "bn_F2048": _case(3, 2, 2, 2048, 2048, 12, "512 groups, the widest fused step"),
    "bn_F2304_unfused": _case(3, 2, 3, 2304, 2304, 2, "576 groups on the unfused lists (fc_dim > 2048)", use_bn=(), unfused_bn=("AdaBN",)),
    # (batch seed 21 leaves relation_domain_classifier_all.0.2.bias - a two-element sum over 65 videos - nearly cancelling: 2.5e-4 between
    # the fp32 and the float64 oracle, over the conditioning bound of tests/test_bn_shapes_cpu.py; as limit_shapes' T64_C64_b190)
    "bn_rows_wave": _case(32, 33, 2, 64, 32, 7, "64 / 66 rows: exactly one full wave, and one wave plus two lanes", xseed=22),
    "bn_rows_1024": _case(256, 257, 4, 64, 32, 7, "1 024 / 1 028 rows: source ends on the first register row per lane, target opens the second"),
    "bn_rows_5120": _case(1024, 1025, 5, 64, 32, 7, "5 120 rows kept (the last count that is) / 5 125 streamed, in the same launch", use_bn=BOTH,
                          ragged_second_step=True),
    "avg_bn_F256": _case(3, 2, 3, 256, 256, 7, "the TemPooling builder's BatchNorm wiring, dealt", agg="avgpool"),
    "avg_bn_rows_5120": _case(1024, 1025, 5, 64, 32, 7, "the TemPooling builder's BatchNorm wiring, kept / streamed", agg="avgpool"),
    "bn_Bt0": _case(3, 0, 3, 64, 64, 5, "the n == 0 early return of both launches"),
}
STEP_CASES = [n for n in CASES if n != "bn_Bt0"]      # (the oracle cannot run an empty domain: BatchNorm1d on zero rows raises)
TRN_CASES = [n for n in STEP_CASES if CASES[n]["agg"] == "trn-m"]
AVG_CASES = [n for n in STEP_CASES if CASES[n]["agg"] == "avgpool"]

# what each case must land on: (has_fused_step, column groups, dealt, (source rows kept, target rows kept))
EXPECT = {
    "bn_n2_F36": (True, 9, False, (True, True)), "bn_F256": (True, 64, True, (True, True)), "bn_F260": (True, 65, False, (True, True)),
    "bn_F512": (True, 128, True, (True, True)), "bn_F768": (True, 192, True, (True, True)), "bn_F2048": (True, 512, True, (True, True)),
    "bn_F2304_unfused": (False, 576, True, (True, True)), "bn_rows_wave": (True, 8, False, (True, True)),
    "bn_rows_1024": (True, 8, False, (True, True)), "bn_rows_5120": (True, 8, False, (True, False)),
    "avg_bn_F256": (True, 64, True, (True, True)), "avg_bn_rows_5120": (True, 8, False, (True, False)),
    "bn_Bt0": (True, 16, False, (True, True)),
}
assert set(EXPECT) == set(CASES)
# ... and between them: dealt and launch-order group counts, kept / kept and kept / streamed domains (streamed / streamed is
# tests/test_gpu_engine_bn.py's tall-batch test), fused and unfused, both aggregations - and the two dealt widths with odd multiples of 64
assert {e[2] for e in EXPECT.values()} == {True, False}
assert {e[3] for e in EXPECT.values()} == {(True, True), (True, False)}
assert {e[0] for e in EXPECT.values()} == {True, False} and any(e[2] for e in EXPECT.values() if not e[0])
assert {c["agg"] for c in CASES.values()} == {"trn-m", "avgpool"}
assert {(CASES[n]["agg"], e[2]) for n, e in EXPECT.items()} >= {("trn-m", True), ("trn-m", False), ("avgpool", True), ("avgpool", False)}
assert {(CASES[n]["agg"], e[3]) for n, e in EXPECT.items()} >= {("trn-m", (True, False)), ("avgpool", (True, False))}
assert {e[1] // BN_DEAL for e in EXPECT.values() if e[2]} >= {1, 2, 3, 8, 9}


def steps_of(case):
    return (0, 1) if case["ragged_second_step"] else (0,)


def make_plan(case, extra_flags=0):
    return ls.make_plan(case, _lib.FLAG_BN_SHARED | extra_flags)


def bn_facts(plan):
    """What the plan says about the BatchNorm launches of the step an engine runs on it."""
    _, _, phases, g, _, _ = plan_arrays(plan)
    groups = -(-int(g.F) // BN_COLS)
    rows = (int(g.Bs) * int(g.T), int(g.Bt) * int(g.T))
    run = (4,) if plan.has_fused_step else (0, 1, 2)
    return dict(has_fused_step=bool(plan.has_fused_step), F=int(g.F), groups=groups, dealt=groups % BN_DEAL == 0, rows=rows,
                kept=tuple(r <= BN_THREADS * BN_KEEP for r in rows),
                bn_launches=tuple(sum(1 for ph in phases if ph.kind == k and ph.group in run) for k in (PH_BN_FWD, PH_BN_BWD)),
                bn_launches_unfused=tuple(sum(1 for ph in phases if ph.kind == k and ph.group in (0, 1, 2)) for k in (PH_BN_FWD, PH_BN_BWD)),
                bn_slots=int(g.n_sumsq) > 0)


def assert_runs_what_it_claims(name, plan, fused=None):
    """fused: which step the caller runs (None: the fused one where the plan has it)."""
    case, (has_fused, groups, dealt, kept) = CASES[name], EXPECT[name]
    f = bn_facts(plan)
    assert f["has_fused_step"] == has_fused == (case["F"] <= HEADS_MAX_F), (name, f)
    assert f["F"] == min(case["F"], case["D"]) == case["F"] and f["F"] % BN_COLS == 0, (name, f)
    assert (f["groups"], f["dealt"]) == (groups, dealt) and dealt == (case["F"] % (BN_COLS * BN_DEAL) == 0), (name, f)
    assert f["rows"] == (case["Bs"] * case["T"], case["Bt"] * case["T"]) and f["kept"] == kept, (name, f)
    assert (f["bn_launches"] if fused in (None, has_fused) else f["bn_launches_unfused"]) == (1, 1), (name, f)
    return f


# ---- inputs ----
def oracle_cfg(case, use_bn="AdaBN", arithmetic="fp32", dropout_i=0.0):
    kw = dict(num_class=case["C"], num_segments=case["T"], feature_dim=case["D"], fc_dim=case["F"], dropout_i=dropout_i, dropout_v=0.0,
              arithmetic=arithmetic, use_bn=use_bn)
    if case["agg"] == "avgpool":
        kw.update(frame_aggregation="avgpool", place_adv=case["place_adv"], add_loss_DA="none", use_attn="none")
    return orc.Config(**kw)


def initial_params(case):
    p = synth_state(orc.param_shapes(oracle_cfg(case)), seed=case["wseed"], scale=case["scale"])
    rng = np.random.default_rng(1000 + case["wseed"])
    for k in BN_PARAMS:      # (see the module docstring; drawn in this order)
        u = rng.uniform(-1.0, 1.0, p[k].shape)
        p[k] = torch.tensor(1.0 + 0.25 * u if k.endswith("weight") else 0.2 * u, dtype=torch.float32)
    return p


def initial_running(case):
    """{state-dict name: fp32 [F]} of the four BatchNorm buffers an engine starts from."""
    rng = np.random.default_rng(2000 + case["wseed"])
    out = {}
    for dom in "ST":
        out[f"bn_shared_{dom}.running_mean"] = torch.tensor(rng.uniform(-0.3, 0.3, case["F"]), dtype=torch.float32)
        out[f"bn_shared_{dom}.running_var"] = torch.tensor(rng.uniform(0.5, 1.5, case["F"]), dtype=torch.float32)
    return out


batch = ls.batch


def oracle_step(case, params, momentum, xs, xt, ys, ns, nt, dtype, masks=None, use_bn="AdaBN", drop_i=None):
    """limit_shapes.oracle_step with use_bn (and, for the dropout test, the host's dropout_i masks)."""
    cast = lambda t: t.detach().cpu().to(dtype).clone()
    state = orc.TrainState(params={k: cast(v) for k, v in params.items()}, lr=LR)
    state.momentum = {k: cast(v) for k, v in (momentum or {}).items()}
    res = orc.train_step(state, cast(xs), cast(xt), ys, BETA, ls.gamma_of(case), oracle_cfg(case, use_bn), clip=CLIP, n_src=ns, n_tgt=nt,
                         masks=masks, drop_i=None if drop_i is None else tuple(cast(m) for m in drop_i))
    return res, state


@functools.lru_cache(maxsize=None)
def float64_reference(name, step=0):
    """limit_shapes.float64_reference on this table (free-running float64 oracle; shared, read-only)."""
    case = CASES[name]
    torch.set_num_threads(min(8, torch.get_num_threads()))
    if step == 0:
        params, momentum = initial_params(case), {}
    else:
        _, st = float64_reference(name, step - 1)
        params, momentum = {k: v.float() for k, v in st.params.items()}, {k: v.float() for k, v in st.momentum.items()}
    xs, xt, ys, ns, nt = batch(case, step)
    res, state = oracle_step(case, params, momentum, xs, xt, ys, ns, nt, torch.float64)
    return dict(res=res, params=params, momentum=momentum, batch=(xs, xt, ys, ns, nt)), state


def logit_keys(case):
    return ls.LOGIT_KEYS if case["agg"] == "trn-m" else ls.LOGIT_KEYS[:1] + ls.LOGIT_KEYS[2:]


# ---- comparisons ----
def split_shared_bias(name, step, got, want):
    """The shared FC's bias sits in front of a BatchNorm: its gradient is zero in exact arithmetic and round-off on both sides.  Both
    within F32_ATOL (as tests/test_gpu_weighted_loss.py), and the tensor left out of the relative comparison.  Returns (got, want)
    without it, and checks on the way that the four BatchNorm gradients are among the tensors that ARE compared."""
    got, want = dict(got), dict(want)
    g, w = got.pop(SHARED_BIAS), want.pop(SHARED_BIAS)
    assert float(torch.as_tensor(g).double().abs().max()) <= tol.F32_ATOL, (name, step, "engine", float(torch.as_tensor(g).abs().max()))
    assert float(torch.as_tensor(w).double().abs().max()) <= tol.F32_ATOL, (name, step, "reference", float(torch.as_tensor(w).abs().max()))
    assert all(k in want and k in got and bool(torch.as_tensor(want[k]).any()) for k in BN_PARAMS), (name, step)
    return got, want


def z0_statistics(z0, Bs, Bt, T):
    """float64 [2, 3, F] (per domain: mean, biased variance, 1 / sqrt(var + 1e-5)) and [2, F] unbiased variances of a [B T, F] matrix of
    BatchNorm inputs, rows [0, Bs T) source and the rest target - what bn_shared_fwd_kernel leaves in region bn_batch, and what the
    running variance moves towards."""
    z0 = torch.as_tensor(z0).double()
    st, unb = torch.zeros(2, 3, z0.shape[1], dtype=torch.float64), torch.zeros(2, z0.shape[1], dtype=torch.float64)
    for d, (lo, n) in enumerate(((0, Bs * T), (Bs * T, Bt * T))):
        if n == 0:
            continue
        z = z0[lo:lo + n]
        mean = z.mean(0)
        var = (z - mean).pow(2).mean(0)
        st[d, 0], st[d, 1], st[d, 2] = mean, var, 1.0 / torch.sqrt(var + 1e-5)
        unb[d] = var * (n / max(n - 1, 1))
    return st, unb


def interp_step(case, plan, params, xs, xt, ys, ns, nt, fused):
    return ls.interp_step(case, plan, params, xs, xt, ys, ns, nt, fused)
