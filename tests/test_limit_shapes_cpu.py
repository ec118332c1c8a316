"""The shapes of tests/limit_shapes.py without a GPU: each case lands on the kernel variant it names, the plan's wiring is right there,
and the fixed inputs are well conditioned - so what tests/test_gpu_limit_shapes.py finds at these shapes is the kernels'.

 (a) Wiring: the launch lists executed in float64 numpy (tests/plan_interp.py; the fused list where the plan has one, and the unfused
     lists) against the float64 oracle: every gradient tensor within 1e-9 relative L2, logits within 1e-9 x max(1, max |want|).  Both
     sides are float64; measured worst 6.4e-12 (64 segments).
 (b) Conditioning: the oracle in fp32 against the oracle in float64 on the same inputs and the same ReLU patterns (the float64 run's):
     every gradient tensor within F32_MASKED_GRAD_REL_L2 / 4, the logits within a quarter of the GPU test's logit bound.  The 4 is the
     factor tests/test_gpu_adam.py allows between two fp32 evaluation orders of one computation: inputs on which ATen's own fp32 order
     already uses up the bound (a near-cancelling two-term sum: 4.1e-3 on one relation-discriminator bias at 3+2 videos x 64 segments)
     would make the GPU bound say nothing.  A case that fails here gets other seeds or more videos, never a wider bound."""
import pytest
import torch

import limit_shapes as ls
from ta3n_amd import tolerances as tol


@pytest.mark.parametrize("name", list(ls.CASES))
def test_case_lands_on_the_variant_it_names(name):
    case = ls.CASES[name]
    plan = ls.make_plan(case)
    if case["agg"] == "trn-m":
        ls.assert_runs_what_it_claims(name, plan)
    else:      # TemPooling: no relations, a fused list from either builder; the general builder is the one with domain logits
        f = ls.plan_facts(plan)
        assert f["has_fused_step"] and f["n_rel"] == 0 and f["heads_launches"] == 0
        assert ("Pv" in plan.regions) == (case["place_adv"] != ("N", "N", "N"))


def test_the_table_covers_every_heads_instantiation_and_both_loaders():
    facts = {n: ls.plan_facts(ls.make_plan(ls.CASES[n])) for n in ls.TRN_CASES}
    fused = [f for f in facts.values() if f["has_fused_step"]]
    assert {f["fq"] for f in fused} == {1, 2, 4, 16, 32}      # FQ 8 (fc_dim 512) is every earlier test's
    assert {(f["vpw"], f["pipe"]) for f in fused} == {(1, False), (1, True), (2, False), (2, True)}
    assert {(f["fq"], f["vpw"]) for f in fused} >= {(32, 1), (32, 2), (1, 2)}
    assert any(not f["has_fused_step"] for f in facts.values())
    assert max(f["n_rel"] for f in fused) == 63 and max(f["C"] for f in fused) == 64 and min(f["C"] for f in fused) == 1
    assert any(f["scalar_operands_per_gemm_launch"][0] for f in fused) and any(f["heads_rpw"] > 16 for f in fused)


@pytest.mark.parametrize("name,fused", [(n, f) for n in ls.TRN_CASES for f in (True, False) if f is False or ls.EXPECT[n][0]])
def test_plan_wiring_against_the_float64_oracle(name, fused):
    case = ls.CASES[name]
    ref, _ = ls.float64_reference(name)
    xs, xt, ys, ns, nt = ref["batch"]
    plan = ls.make_plan(case)
    assert plan.has_fused_step or not fused
    grads, it = ls.interp_step(case, plan, ref["params"], xs, xt, ys, ns, nt, fused)
    want = ref["res"]["grads"]
    worst, _, _ = ls.assert_gradients(name, 0, {k: torch.from_numpy(grads[k]) for k in want}, want, 1e-9)
    B, T, g = case["Bs"] + case["Bt"], case["T"], it.g
    got = dict(out=it.r(g.o_Y, (B, case["C"])), pred_rel=it.r(g.o_Pr, (B, T - 1, 2)), pred_vid=it.r(g.o_Pv, (B, 2)), pred_frm=it.r(g.o_Pf, (B, T, 2)))
    for k, w in ls.oracle_logits(ref["res"], ns, nt).items():
        err = float((torch.from_numpy(got[k].copy()).reshape(w.shape) - w).abs().max())
        assert err <= 1e-9 * max(1.0, float(w.abs().max())), (name, k, err)


@pytest.mark.parametrize("name,step", [(n, s) for n, c in ls.CASES.items() for s in ((0, 1) if c["ragged_second_step"] else (0,))])
def test_inputs_are_well_conditioned(name, step, capsys):
    case = ls.CASES[name]
    ref, _ = ls.float64_reference(name, step)
    xs, xt, ys, ns, nt = ref["batch"]
    r32, _ = ls.oracle_step(case, ref["params"], ref["momentum"], xs, xt, ys, ns, nt, torch.float32, masks=ls.relu_patterns(ref["res"]))
    worst, med, per = ls.assert_gradients(name, step, r32["grads"], ref["res"]["grads"], tol.F32_MASKED_GRAD_REL_L2 / 4)
    keys = ls.LOGIT_KEYS if case["agg"] == "trn-m" else ls.LOGIT_KEYS[:1] + (ls.LOGIT_KEYS[2:] if case["place_adv"] != ("N", "N", "N") else ())
    want, got = ls.oracle_logits(ref["res"], ns, nt, keys), ls.oracle_logits(r32, ns, nt, keys)
    errs = {}
    for k, w in want.items():
        errs[k] = float((got[k] - w).abs().max())
        assert errs[k] <= ls.logit_bound(w) / 4, (name, step, k, errs[k], float(w.abs().max()))
    with capsys.disabled():
        print(f"\n[fp32 oracle vs float64 oracle, same masks] {name} step {step}: gradients worst {worst:.1e} "
              f"({max(per, key=per.get)}), median {med:.1e}; logits max error {max(errs.values()):.1e} at max |logit| "
              f"{max(float(w.abs().max()) for w in want.values()):.0f}")
