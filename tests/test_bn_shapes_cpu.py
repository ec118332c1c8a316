"""The shapes of tests/bn_shapes.py without a GPU: each case lands on the branches of the BatchNorm launches it names, its fixed inputs
are well conditioned, and the plan's wiring is right there - so what tests/test_gpu_bn_shapes.py finds at these shapes is the kernels'.

 (a) Conditioning: the oracle in fp32 against the oracle in float64 on the same inputs and the float64 run's ReLU patterns, every step a
     case runs: every gradient tensor within F32_MASKED_GRAD_REL_L2 / 4 and their median within F32_MASKED_GRAD_REL_L2_MEDIAN / 4, the
     logits within a quarter of limit_shapes.logit_bound, the six loss scalars within 5e-4 / 4 relative (the factor 4: see
     tests/test_limit_shapes_cpu.py).  The shared FC's bias, in front of a BatchNorm, has a zero gradient in exact arithmetic: both
     evaluations <= F32_ATOL, left out of the relative comparison.  A case that fails here gets another seed, never a wider bound.
     bn_Bt0 has no target rows and the oracle's BatchNorm refuses an empty domain: its source forward alone is compared.
 (b) Wiring: the launch lists executed in float64 numpy (tests/plan_interp.py, which runs the BatchNorm phases and their sum-of-squares
     slots), fused and unfused, against the float64 oracle: gradients and logits as tests/test_limit_shapes_cpu.py compares them (1e-9),
     region bn_batch against the statistics of the shared-FC product formed here, the slots' total against the oracle's gradient norm.
 (c) use_bn with a fc_dim that is no multiple of 4 (38: nine and a half column groups) is refused with bn_shared_refusal's message."""
import numpy as np
import pytest
import torch

import bn_shapes as bs
import limit_shapes as ls
from dropout_masks import EXCLUDE_SHARE, dropout_masks, excluded, preactivation
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import ALL_FLAGS, dropout_seeds

LOSS_REL = 5e-4      # tests/test_gpu_bn_shapes.py (tests/test_gpu_parity.py's)
WIRING_MAX_ROWS = 1100
WIRING_CASES = [n for n in bs.STEP_CASES if max(bs.CASES[n]["Bs"], bs.CASES[n]["Bt"]) * bs.CASES[n]["T"] <= WIRING_MAX_ROWS] + ["bn_rows_5120"]


@pytest.mark.parametrize("name", list(bs.CASES))
def test_case_lands_on_the_branches_it_names(name):
    case = bs.CASES[name]
    plan = bs.make_plan(case)
    f = bs.assert_runs_what_it_claims(name, plan)
    assert f["bn_launches_unfused"] == (1, 1)      # (every plan keeps the unfused lists)
    assert all(k in plan.regions for k in ("Z0", "gZ0", "bn_batch", "bn_run")) and plan.regions["bn_batch"][1] == 6 * case["F"]
    live = {n for n, _, _, lv in plan.params if lv}
    assert set(bs.BN_PARAMS) <= live
    if case["agg"] == "avgpool":      # the general TemPooling builder (domain logits), no relations
        assert "Pv" in plan.regions and ls.plan_facts(plan)["n_rel"] == 0
    assert f["bn_slots"] or not f["has_fused_step"]      # the fused step's gradient norm comes from the sum-of-squares slots


def test_the_table_covers_every_branch_of_the_batchnorm_launches():
    facts = {n: bs.bn_facts(bs.make_plan(bs.CASES[n])) for n in bs.CASES}
    assert {f["dealt"] for f in facts.values()} == {True, False}
    assert {f["kept"] for f in facts.values()} == {(True, True), (True, False)}      # streamed / streamed: tests/test_gpu_engine_bn.py
    assert {f["has_fused_step"] for f in facts.values()} == {True, False}
    assert any(f["dealt"] and not f["has_fused_step"] for f in facts.values())
    assert {bs.CASES[n]["agg"] for n in facts} == {"trn-m", "avgpool"}
    for agg in ("trn-m", "avgpool"):
        mine = [f for n, f in facts.items() if bs.CASES[n]["agg"] == agg]
        assert {f["dealt"] for f in mine} == {True, False} and (True, False) in {f["kept"] for f in mine}, agg
    groups = sorted(f["groups"] for f in facts.values() if f["dealt"])
    assert groups[0] == 64 and groups[-1] == 576 and 192 in groups      # the smallest dealt launch, the widest, one that is no power of two
    assert {f["groups"] for f in facts.values() if not f["dealt"]} >= {8, 9, 65}
    rows = {r for f in facts.values() for r in f["rows"]}
    # the row counts at which the kept branch's per-lane register rows and the keep / stream decision change, and the smallest batch
    assert rows >= {0, 2, 64, 66, bs.BN_THREADS, bs.BN_THREADS + 4, bs.BN_THREADS * bs.BN_KEEP, bs.BN_THREADS * bs.BN_KEEP + 5}
    assert any(bs.CASES[n]["ragged_second_step"] and f["kept"] == (True, False) for n, f in facts.items())


def test_use_bn_refuses_a_fc_dim_that_is_no_multiple_of_four():
    with pytest.raises(ValueError) as e:      # (ta3n_plan_create: TA3N_ERR_INVALID)
        _lib.Plan(3, 2, 3, 40, 38, 7, ALL_FLAGS | _lib.FLAG_BN_SHARED)
    assert "use_bn: fc_dim must be a multiple of 4 (the BatchNorm launches move a row's four columns as one 16-byte access)" in str(e.value)
    _lib.Plan(3, 2, 3, 40, 36, 7, ALL_FLAGS | _lib.FLAG_BN_SHARED)      # (the neighbouring width is taken)


@pytest.mark.parametrize("name,step", [(n, s) for n in bs.STEP_CASES for s in bs.steps_of(bs.CASES[n])])
def test_inputs_are_well_conditioned(name, step, capsys):
    case = bs.CASES[name]
    ref, _ = bs.float64_reference(name, step)
    xs, xt, ys, ns, nt = ref["batch"]
    r32, _ = bs.oracle_step(case, ref["params"], ref["momentum"], xs, xt, ys, ns, nt, torch.float32, masks=ls.relu_patterns(ref["res"]))
    got, want = bs.split_shared_bias(name, step, r32["grads"], ref["res"]["grads"])
    worst, med, per = ls.assert_gradients(name, step, got, want, tol.F32_MASKED_GRAD_REL_L2 / 4, tol.F32_MASKED_GRAD_REL_L2_MEDIAN / 4)
    keys = bs.logit_keys(case)
    wl, gl = ls.oracle_logits(ref["res"], ns, nt, keys), ls.oracle_logits(r32, ns, nt, keys)
    errs = {}
    for k, w in wl.items():
        errs[k] = float((gl[k] - w).abs().max())
        assert errs[k] <= ls.logit_bound(w) / 4, (name, step, k, errs[k], float(w.abs().max()))
    want_s, got_s = ls.oracle_loss_scalars(case, ref["res"], ns, nt), ls.oracle_loss_scalars(case, r32, ns, nt)
    lerr = max(abs(got_s[k] - w) / max(1.0, abs(w)) for k, w in want_s.items())
    assert lerr <= LOSS_REL / 4, (name, step, got_s, want_s)
    with capsys.disabled():
        print(f"\n[bn shapes, fp32 oracle vs float64 oracle, same masks] {name} step {step}: gradients worst {worst:.1e} "
              f"({max(per, key=per.get)}), median {med:.1e}; logits max error {max(errs.values()):.1e} at max |logit| "
              f"{max(float(w.abs().max()) for w in wl.values()):.0f}; loss scalars {lerr:.1e}")


def test_the_source_forward_of_the_empty_target_case_is_well_conditioned():
    case = bs.CASES["bn_Bt0"]
    cfg = bs.oracle_cfg(case)
    params = bs.initial_params(case)
    xs, _, _, _, _ = bs.batch(case, 0)
    outs = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            outs.append(bs.orc.forward_domain({k: v.to(dt) for k, v in params.items()}, xs.to(dt), bs.BETA, cfg, domain="S")["out"].double())
    err = float((outs[1] - outs[0]).abs().max())
    assert err <= ls.logit_bound(outs[0]) / 4, err


def test_the_dropout_case_keeps_few_units_near_the_relu_kink():
    """tests/test_gpu_bn_shapes.py compares the zero pattern of F1 at bn_F256 away from the ReLU kink (tests/dropout_masks.py): the units
    it leaves out are at most EXCLUDE_SHARE of the tensor - a condition on the inputs, from the float64 oracle alone."""
    case = bs.CASES["bn_F256"]
    xs, xt, _, _, _ = bs.batch(case, 0)
    _, share = excluded(preactivation(bs.oracle_cfg(case, dropout_i=0.5), bs.initial_params(case), xs, xt))
    assert share <= EXCLUDE_SHARE, share


def test_the_dropout_case_is_well_conditioned():
    """... and its gradients, with the host's dropout_i masks of that step on both sides, are as well conditioned as the others'."""
    name = "bn_F256"
    case = bs.CASES[name]
    xs, xt, ys, ns, nt = bs.batch(case, 0)
    mk = dropout_masks(*dropout_seeds(0, 0), 0.5, 0.0, case["Bs"], case["Bt"], case["T"], case["F"], 256)
    params = bs.initial_params(case)
    r64, _ = bs.oracle_step(case, params, {}, xs, xt, ys, ns, nt, torch.float64, drop_i=mk["drop_i"])
    r32, _ = bs.oracle_step(case, params, {}, xs, xt, ys, ns, nt, torch.float32, masks=ls.relu_patterns(r64), drop_i=mk["drop_i"])
    got, want = bs.split_shared_bias(name, 0, r32["grads"], r64["grads"])
    ls.assert_gradients(name, 0, got, want, tol.F32_MASKED_GRAD_REL_L2 / 4, tol.F32_MASKED_GRAD_REL_L2_MEDIAN / 4)


@pytest.mark.parametrize("name,fused", [(n, f) for n in WIRING_CASES for f in (True, False) if f is False or bs.EXPECT[n][0]])
def test_plan_wiring_against_the_float64_oracle(name, fused):
    case = bs.CASES[name]
    ref, _ = bs.float64_reference(name)
    xs, xt, ys, ns, nt = ref["batch"]
    plan = bs.make_plan(case)
    bs.assert_runs_what_it_claims(name, plan, fused=fused)
    grads, it = bs.interp_step(case, plan, ref["params"], xs, xt, ys, ns, nt, fused)
    want = dict(ref["res"]["grads"])
    got = {k: torch.from_numpy(grads[k]) for k in want}
    # both sides float64: the shared bias's zero gradient is round-off at 1e-17, not F32_ATOL
    assert float(got.pop(bs.SHARED_BIAS).abs().max()) <= 1e-12 and float(want.pop(bs.SHARED_BIAS).abs().max()) <= 1e-12
    assert all(k in want for k in bs.BN_PARAMS)
    ls.assert_gradients(name, 0, got, want, 1e-9)
    B, T, F, g = case["Bs"] + case["Bt"], case["T"], case["F"], it.g
    out = dict(out=it.r(g.o_Y, (B, case["C"])), pred_vid=it.r(g.o_Pv, (B, 2)), pred_frm=it.r(g.o_Pf, (B, T, 2)))
    if case["agg"] == "trn-m":
        out["pred_rel"] = it.r(g.o_Pr, (B, T - 1, 2))
    for k, w in ls.oracle_logits(ref["res"], ns, nt, bs.logit_keys(case)).items():
        err = float((torch.from_numpy(out[k].copy()).reshape(w.shape) - w).abs().max())
        assert err <= 1e-9 * max(1.0, float(w.abs().max())), (name, k, err)
    # the batch statistics, against those of the shared-FC product formed here
    p = {k: v.double() for k, v in ref["params"].items()}
    z0 = torch.cat((xs, xt), 0).double().reshape(B * T, -1) @ p["fc_feature_shared_source.weight"].t() + p["fc_feature_shared_source.bias"]
    st, _ = bs.z0_statistics(z0, case["Bs"], case["Bt"], T)
    got_st = torch.from_numpy(it.r(g.o_bn_batch, (2, 3, F)).copy())
    assert torch.allclose(got_st, st, rtol=1e-9, atol=1e-12), (name, float((got_st - st).abs().max()))
    if fused:      # the slots hold the WHOLE squared norm, the BatchNorm workgroups' share included
        total = float(np.sqrt(it.ws[g.o_sumsq:g.o_sumsq + g.n_sumsq].sum()))
        assert abs(total - float(ref["res"]["total_norm"])) <= 1e-9 * float(ref["res"]["total_norm"]), (name, total)
