"""use_bn AdaBN / AutoDIAL on the GPU at the column and row counts the two BatchNorm launches branch on (tests/bn_shapes.py): group
counts that bn_column_group deals (64, 128, 192, 512, 576 groups - fc_dim 256 .. 2304) and that stay in launch order (8, 9, 65), rows kept
in registers and streamed in ONE launch (5 120 / 5 125), the edges of the per-lane register rows (1 024 / 1 028), one full and one partly
filled wave (64 / 66, 2 / 2 rows), the fused step and the unfused lists, trn-m and TemPooling.  Every test first asserts from the ENGINE's
plan that it runs the branches its case names.  tests/test_bn_shapes_cpu.py shows without a GPU that the inputs are well conditioned and
that the plan's wiring is right at these shapes, so a failure here is a kernel's.

 (a) the fp32 step against the float64 oracle forced to the engine's ReLU patterns (tests/test_gpu_limit_shapes.py's scheme and bounds;
     TemPooling free-running at F32_GRAD_*), the four BatchNorm gradients among the tensors compared - and, since forced patterns
     follow the engine into a column it never wrote, F1 against the oracle's own ReLU of its BatchNorm output;
 (b) what the forward launch writes - region bn_batch and the running statistics - against float64 statistics of the engine's OWN Z0:
     every column of both domains, isolated from the GEMM in front (rtol 2e-4, atol 2e-5: tests/test_gpu_engine_bn.py's for the buffers),
     the means and variances also within the rounding-error bound of their sums (one row of 5 120 is worth 2e-4);
 (c) the fused gradient norm (the backward launch's sum-of-squares slots are indexed by the dealt group) against the norm of the gradients;
 (d) eval mode at a dealt width: validation through the target statistics, and a plain eval forward through each domain's own;
 (e) the bf16 and pair twins of F1 and gZ0 the launches store, bit for bit;
 (f) the dropout counter (row F + column, column from the dealt group) against the host restatement of the stream;
 (g) an empty target half: the n == 0 return of both launches.
Measured floors are printed (pytest -s) and recorded in profiles/limit_shapes_parity_floors.txt."""
import pytest
import torch

import bn_shapes as bs
import limit_shapes as ls
from dropout_masks import check_frame_pattern, dropout_masks, excluded, preactivation
from oracle import ta3n_oracle as orc
from plan_interp import plan_arrays
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, dropout_seeds
from test_gpu_masked_gradients import _engine_masks
from test_gpu_pair_twins import _split

pytestmark = pytest.mark.gpu

LOSS_REL = 5e-4                    # tests/test_gpu_parity.py
HIDDEN_REL = 2e-4                  # tests/test_gpu_masked_gradients.py
STAT_RTOL, STAT_ATOL = 2e-4, 2e-5  # tests/test_gpu_engine_bn.py, the BatchNorm buffers
U32 = 2.0 ** -24                   # unit round-off of fp32


def _engine(case, use_bn, fused=True, dropout_i=0.0, **kw):
    eng = TrainEngine(case["Bs"], case["Bt"], case["T"], case["D"], case["F"], case["C"], dropout_i=dropout_i, dropout_v=0.0, clip=bs.CLIP,
                      aggregation=case["agg"], flags=ls.flags_of(case), use_bn=use_bn, fused=fused, **kw)
    eng.load_state({**bs.initial_params(case), **bs.initial_running(case)})
    return eng


def _assert_branches(name, eng, fused):
    f = bs.assert_runs_what_it_claims(name, eng.plan, fused=fused)
    assert eng.fused == fused and eng.use_bn != "none", (name, eng.describe())
    return f


def _resynced(eng):
    return ({k: v.detach().cpu().clone() for k, v in eng.param_views().items()},
            {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()})


def _step(eng, case, xs, xt, ys, ns, nt, s):
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(bs.BETA, ls.gamma_of(case), bs.LR, valid_source=ns, valid_target=nt, seed=s)
    torch.cuda.synchronize()


STEP_PARAMS = ([(n, u, True) for n in bs.STEP_CASES for u in bs.CASES[n]["use_bn"]] +
               [(n, u, False) for n in bs.STEP_CASES for u in bs.CASES[n]["unfused_bn"]])
assert {n for n, _, _ in STEP_PARAMS} == set(bs.STEP_CASES)
assert {(n, f) for n, _, f in STEP_PARAMS} >= {("bn_F256", False), ("bn_F2304_unfused", False)}


@pytest.mark.parametrize("name,use_bn,fused", STEP_PARAMS)
def test_fp32_step_against_the_float64_oracle(name, use_bn, fused, capsys):
    """(a).  trn-m: the oracle forced to the engine's ReLU patterns, F32_MASKED_GRAD_*; TemPooling: free-running, F32_GRAD_*."""
    case = bs.CASES[name]
    T, trn = case["T"], case["agg"] == "trn-m"
    eng = _engine(case, use_bn, fused)
    _assert_branches(name, eng, fused)
    if not bs.EXPECT[name][0]:      # fc_dim > 2048: asking for the fused step gives the unfused lists, and the engine says so
        asked = _engine(case, use_bn, True)
        assert not asked.plan.has_fused_step and not asked.fused and "unfused" in asked.describe()
    n_tuples = sum(len(sc) for sc in orc.selected_relations(T)) if trn else 0
    bound, median = ((tol.F32_MASKED_GRAD_REL_L2, tol.F32_MASKED_GRAD_REL_L2_MEDIAN) if trn else
                     (tol.F32_GRAD_REL_L2, tol.F32_GRAD_REL_L2_MEDIAN))
    lines = []
    for s in bs.steps_of(case):
        xs, xt, ys, ns, nt = bs.batch(case, s)
        params, momentum = _resynced(eng)      # (the ragged second step starts from the engine's own state)
        _step(eng, case, xs, xt, ys, ns, nt, s)
        masks = None
        if trn:
            masks, act = _engine_masks(eng, n_tuples)
        res, _ = bs.oracle_step(case, params, momentum, xs, xt, ys, ns, nt, torch.float64, masks=masks, use_bn=use_bn)
        if trn:
            for d, (dom, nv) in enumerate((("src", ns), ("tgt", nt))):      # the hidden activations themselves, valid rows
                for k, a in act[d].items():
                    want = res[dom]["hidden"][k].detach()
                    rows = nv * T if k in ("F1", "Hf") else nv
                    err = (a[:rows].double() - want[:rows]).abs().max().item()
                    assert err <= HIDDEN_REL * max(1.0, want[:rows].abs().max().item()), (name, s, dom, k, err)
                # The forced patterns are the ENGINE's: a column the BatchNorm launch never wrote reads as "every unit off", the oracle
                # follows, and activations, gradients and logits all agree on the dead column (seen with a dealing that skipped every
                # other group).  So F1 also goes against the oracle's OWN ReLU of its BatchNorm output, every row: the two sides of the
                # kink meet at zero, so a unit that lands on the other side differs by round-off, a dead column by O(1).
                want = torch.relu(res[dom]["pre_f1"].detach())
                got_f1 = eng.region("F1", (eng.B * T, eng.F)).cpu().double()[d * eng.Bs * T:][:want.shape[0]]
                err = (got_f1 - want).abs().max().item()
                assert err <= HIDDEN_REL * max(1.0, want.abs().max().item()), (name, s, dom, "F1 against the free-running ReLU", err)
        got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res["grads"]}
        assert set(got) == set(res["grads"]) == set(eng.live_names())
        got, want = bs.split_shared_bias(name, s, got, res["grads"])
        worst, med, per = ls.assert_gradients(name, s, got, want, bound, median)
        if not trn:
            for k, w in want.items():
                assert float((got[k].double().reshape(w.shape) - w).abs().max()) <= tol.F32_GRAD_MAX_SCALE * float(w.abs().max()), (name, k)
        o = eng.outputs()
        lerr, lmax = 0.0, 0.0
        for k, w in ls.oracle_logits(res, case["Bs"], case["Bt"], bs.logit_keys(case)).items():      # every row, dummy rows included
            err = float((o[k].detach().cpu().double().reshape(w.shape) - w).abs().max())
            lerr, lmax = max(lerr, err), max(lmax, float(w.abs().max()))
            assert err <= ls.logit_bound(w), (name, s, k, err, float(w.abs().max()))
        got_l, want_l = eng.losses(), ls.oracle_loss_scalars(case, res, ns, nt)
        if not trn:      # TemPooling logs the relation slot's term (the video logits once more) with the video level's: compared as one sum
            adv = ("loss_adv_rel", "loss_adv_vid", "loss_adv_frm")
            got_l, want_l = ({"loss": l["loss"], "loss_c": l["loss_c"], "loss_e": l["loss_e"], "loss_adv": sum(l[k] for k in adv)}
                             for l in (got_l, want_l))
        for k, w in want_l.items():
            assert abs(got_l[k] - w) <= LOSS_REL * max(1.0, abs(w)), (name, s, k, got_l[k], w)
        loss_err = max(abs(got_l[k] - w) / max(1.0, abs(w)) for k, w in want_l.items())
        bn_worst = max(per[k] for k in bs.BN_PARAMS)
        lines.append(f"[bn shapes, {'masked' if trn else 'free-running'} fp32] {name} {use_bn} {'fused' if fused else 'unfused'} step {s}: "
                     f"rel. L2 worst {worst:.2e} ({max(per, key=per.get)}), median {med:.2e}, BatchNorm affine worst {bn_worst:.2e}; "
                     f"logits max error {lerr:.1e} at max |logit| {lmax:.0f}; loss scalars {loss_err:.1e}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


STAT_PARAMS = ([(n, True) for n in bs.STEP_CASES if bs.EXPECT[n][0]] +
               [(n, False) for n in bs.STEP_CASES if bs.CASES[n]["unfused_bn"]])


@pytest.mark.parametrize("name,fused", STAT_PARAMS)
def test_statistics_the_forward_launch_writes_against_its_own_input(name, fused, capsys):
    """(b).  Z0 is what the shared-FC launch left; the statistics of EVERY column of both domains (mean, biased variance,
    1 / sqrt(var + 1e-5)) and the running buffers 0.9 old + 0.1 new (unbiased variance) are the BatchNorm launch's alone.  A column or
    row it mishandles is wrong by O(1).  The buffers start from non-trivial values; on the ragged step the dummy rows count."""
    case = bs.CASES[name]
    Bs, Bt, T, F = case["Bs"], case["Bt"], case["T"], case["F"]
    eng = _engine(case, (case["use_bn"] if fused else case["unfused_bn"])[0], fused)
    _assert_branches(name, eng, fused)
    start = bs.initial_running(case)
    old = torch.stack([torch.stack((start[f"bn_shared_{d}.running_mean"], start[f"bn_shared_{d}.running_var"])) for d in "ST"]).double()
    assert torch.equal(eng.bn_running.cpu().double(), old)
    lines = []
    for s in bs.steps_of(case):
        xs, xt, ys, ns, nt = bs.batch(case, s)
        _step(eng, case, xs, xt, ys, ns, nt, s)
        st, unb = bs.z0_statistics(eng.region("Z0", ((Bs + Bt) * T, F)).cpu(), Bs, Bt, T)
        got_st = eng.region("bn_batch").view(2, 3, F).cpu().double()
        run = eng.bn_running.cpu().double()
        want_run = torch.stack((0.9 * old[:, 0] + 0.1 * st[:, 0], 0.9 * old[:, 1] + 0.1 * unb), 1)
        errs = []
        for what, g, w in (("batch statistics", got_st, st), ("running statistics", run, want_run)):
            d = (g - w).abs()
            errs.append(float((d / (STAT_ATOL + STAT_RTOL * w.abs())).max()))
            bad = (d > STAT_ATOL + STAT_RTOL * w.abs()).nonzero()
            assert bad.numel() == 0, (name, s, what, bad.shape[0], "of", g.numel(), "first [domain, statistic, column]", bad[:4].tolist())
        # That tolerance is what a ROW costs only at small batches: one row of 5 120 left out of a sum moves a mean by |z - mean| / 5 120,
        # 2e-4.  So the two sums are also held to their rounding-error bound (u = 2^-24; a value reaches the total through at most
        # `depth` fp32 additions: ceil(rows / 1024) in its lane, six butterfly steps in its wave, sixteen waves in order):
        #   |mean - exact| <= (depth + 2) u mean|z|                      (+ 1: the division, + 1: second-order terms)
        #   |var - exact|  <= (depth + 5) u var + 2 (bound of the mean)^2   (z - mean rounded once: 2 u on its square; the division;
        #                                                                  sum (z - m')^2 = rows var + rows (m' - mean)^2 exactly)
        z0 = eng.region("Z0", ((Bs + Bt) * T, F)).cpu().double()
        sums = []
        for d_, (lo, n) in enumerate(((0, Bs * T), (Bs * T, Bt * T))):
            depth = -(-n // bs.BN_THREADS) + 6 + 16
            mean_bound = (depth + 2) * U32 * z0[lo:lo + n].abs().mean(0)
            var_bound = (depth + 5) * U32 * st[d_, 1] + 2 * mean_bound.pow(2)
            for what, i, bound in (("mean", 0, mean_bound), ("variance", 1, var_bound)):
                over = (got_st[d_, i] - st[d_, i]).abs() / bound
                sums.append(float(over.max()))
                assert sums[-1] <= 1.0, (name, s, "ST"[d_], what, "rounding-error bound", sums[-1], "column", int(over.argmax()))
        assert eng.bn_batches == s + 1
        old = run
        lines.append(f"[bn shapes, statistics vs float64 of the engine's Z0] {name} {'fused' if fused else 'unfused'} step {s}: worst error "
                     f"over its tolerance, batch {errs[0]:.1e}, running {errs[1]:.1e}; means and variances over their rounding-error "
                     f"bound {max(sums):.2f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", ["bn_F256", "bn_F768", "bn_F2048"])
def test_fused_gradient_norm_holds_the_dealt_batchnorm_slots(name):
    """(c).  The backward launch's workgroups leave their share of the squared norm in the slot of the column group they were DEALT."""
    case = bs.CASES[name]
    eng = _engine(case, case["use_bn"][0], True)
    f = _assert_branches(name, eng, True)
    assert f["dealt"] and f["bn_slots"]
    xs, xt, ys, ns, nt = bs.batch(case, 0)
    _step(eng, case, xs, xt, ys, ns, nt, 0)
    want = float(eng.G[:eng.plan.live_floats].double().norm())
    got = float(eng.region("grad_norm")[0])
    assert want > 0 and abs(got - want) <= tol.F32_RTOL * want, (name, got, want)
    # ... and each slot is its own group's share: a permutation of the slots would leave the total alone
    g = plan_arrays(eng.plan)[3]
    slots = eng.ws[g.o_sumsq + g.n_sumsq - 2 * f["groups"]:g.o_sumsq + g.n_sumsq].view(2, f["groups"]).cpu().double()
    grads = eng.param_views(eng.G)
    for d, dom in enumerate("ST"):
        w = sum(grads[f"bn_shared_{dom}.{k}"].cpu().double().pow(2).view(f["groups"], 4).sum(1) for k in ("weight", "bias"))
        assert torch.allclose(slots[d], w, rtol=tol.F32_RTOL, atol=1e-12), (name, dom, float((slots[d] - w).abs().max()))


@pytest.mark.parametrize("use_bn", ["AdaBN", "AutoDIAL"])
def test_eval_mode_at_a_dealt_width(use_bn):
    """(d).  bn_F256 after two train steps: evaluate_batch scores every video through the TARGET domain's affine pair and running
    statistics (read by the dealt group), a plain eval forward sends each domain through its own; neither moves the buffers."""
    name = "bn_F256"
    case = bs.CASES[name]
    Bs, Bt = case["Bs"], case["Bt"]
    eng = _engine(case, use_bn, True)
    assert _assert_branches(name, eng, True)["dealt"]
    for s in range(2):
        xs, xt, ys, ns, nt = bs.batch(case, s)
        _step(eng, case, xs, xt, ys, ns, nt, s)
    run, batches = eng.bn_running.clone(), eng.bn_batches
    assert batches == 2
    cfg = bs.oracle_cfg(case, use_bn)
    p = {k: v.detach().cpu().double() for k, v in eng.param_views().items()}
    stats = lambda d: (run[d, 0].cpu().double(), run[d, 1].cpu().double())
    fwd = lambda x, dom, d: orc.forward_domain(p, x.double(), [0.0, 0.0, 0.0], cfg, domain=dom, bn_running=stats(d))["out"].detach()
    eng.evaluate_batch(xs.cuda(), ys.cuda(), reset=True)
    torch.cuda.synchronize()
    want = fwd(xs, "T", 1)
    got = eng.outputs()["out"][:Bs].cpu().double()
    assert float((got - want).abs().max()) <= ls.logit_bound(want), ("validation", float((got - want).abs().max()))
    assert float((got - fwd(xs, "S", 0)).abs().max()) > 10 * ls.logit_bound(want)      # (the two domains' BatchNorms do differ here)
    assert torch.equal(eng.bn_running, run) and eng.bn_batches == batches
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.set_hyper([0.0, 0.0, 0.0], 0.0, 0.0, train=False)
    eng.forward()
    torch.cuda.synchronize()
    out = eng.outputs()["out"].cpu().double()
    for what, g_, w in (("source", out[:Bs], fwd(xs, "S", 0)), ("target", out[Bs:], fwd(xt, "T", 1))):
        assert float((g_ - w).abs().max()) <= ls.logit_bound(w), (what, float((g_ - w).abs().max()))
    assert torch.equal(eng.bn_running, run) and eng.bn_batches == batches


@pytest.mark.parametrize("arith", ["bf16", "f32x3p"])
@pytest.mark.parametrize("name", ["bn_F256", "bn_F512"])
def test_twins_of_the_batchnorm_outputs_are_the_split_of_their_fp32_regions(name, arith):
    """(e).  With TA3N_FLAG_BF16_STORE the two launches store the twins of F1 and gZ0 beside the fp32 values, at the dealt columns: the
    hi plane is the round-to-nearest-even bf16 of the region, the lo plane (pair twins, at pair_delta) that of the remainder."""
    case = bs.CASES[name]
    assert case["arithmetics"]
    kw = dict(bf16=True, bf16_store=True) if arith == "bf16" else dict(f32_split=True, bf16_store=True)
    eng = _engine(case, case["use_bn"][0], True, **kw)
    assert _assert_branches(name, eng, True)["dealt"] and eng.bf16_store
    g = plan_arrays(eng.plan)[3]
    pairs = arith == "f32x3p"
    assert (g.pair_delta > 0) == pairs == ("ws16_lo" in eng.plan.regions) and g.o_ws16 == eng.plan.regions["ws16"][0]
    if pairs:
        assert eng.plan.regions["ws16_lo"][0] - eng.plan.regions["ws16"][0] == g.pair_delta
    xs, xt, ys, ns, nt = bs.batch(case, 0)
    _step(eng, case, xs, xt, ys, ns, nt, 0)
    assert torch.isfinite(eng.P).all()
    for rname in ("F1", "gZ0"):
        off, size = eng.plan.regions[rname]
        src = eng.region(rname)
        assert float(src.abs().max()) > 0 and 2 * eng.plan.regions["ws16"][1] >= off + size
        want_hi, want_lo = _split(src)
        hi = eng.region("ws16").view(torch.int16)[off:off + size]
        assert torch.equal(hi, want_hi), (name, arith, rname, "hi plane", int((hi != want_hi).sum()), size)
        if pairs:
            lo = eng.region("ws16_lo").view(torch.int16)[off:off + size]
            assert torch.equal(lo, want_lo), (name, arith, rname, "lo plane", int((lo != want_lo).sum()), size)


def test_dropout_counter_at_a_dealt_width(capsys):
    """(f).  bn_F256, dropout_i 0.5, fused: dropout_i sits in bn_shared_fwd_kernel, its element id is row F + column with the column from
    the dealt group.  F1 is zero exactly where the host's restatement of the stream drops (tests/dropout_masks.py), nonzero where it keeps
    a unit whose float64 pre-activation is clearly positive, and a kept unit is twice its pre-activation."""
    name = "bn_F256"
    case = bs.CASES[name]
    Bs, Bt, T, F = case["Bs"], case["Bt"], case["T"], case["F"]
    eng = _engine(case, "AdaBN", True, dropout_i=0.5)
    assert _assert_branches(name, eng, True)["dealt"]
    params, momentum = _resynced(eng)
    xs, xt, ys, ns, nt = bs.batch(case, 0)
    _step(eng, case, xs, xt, ys, ns, nt, 0)
    mk = dropout_masks(*dropout_seeds(0, 0), 0.5, 0.0, Bs, Bt, T, F, 256)
    keep = torch.cat(mk["keep_i"])
    assert 0.4 < float(keep.mean()) < 0.6
    pre = preactivation(bs.oracle_cfg(case, "AdaBN", dropout_i=0.5), params, xs, xt)
    F1 = eng.region("F1", ((Bs + Bt) * T, F)).cpu().double()
    share = check_frame_pattern(F1, pre, keep, name)
    on = (keep == 1) & (pre > 0) & ~excluded(pre)[0]
    err = float((F1[on] - 2.0 * pre[on]).abs().max())
    assert err <= HIDDEN_REL * max(1.0, 2.0 * float(pre[on].max())), err
    # ... and the way back through the dropped units: the step's gradients against the oracle on the HOST's masks and the engine's ReLU
    # patterns (tests/test_gpu_dropout_parity.py's scheme; conditioning of these inputs: tests/test_bn_shapes_cpu.py)
    masks, _ = _engine_masks(eng, sum(len(sc) for sc in orc.selected_relations(T)))
    res, _ = bs.oracle_step(case, params, momentum, xs, xt, ys, ns, nt, torch.float64, masks=masks, drop_i=mk["drop_i"])
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res["grads"]}
    got, want = bs.split_shared_bias(name, 0, got, res["grads"])
    worst, med, per = ls.assert_gradients(name, 0, got, want, tol.F32_MASKED_GRAD_REL_L2, tol.F32_MASKED_GRAD_REL_L2_MEDIAN)
    with capsys.disabled():
        print(f"\n[bn shapes, dropout_i in the BatchNorm launch] {name}: excluded share of the pattern check {share:.2%}, kept units vs 2 x "
              f"float64 pre-activation max error {err:.1e}; gradients rel. L2 worst {worst:.2e} ({max(per, key=per.get)}), median {med:.2e}")


def test_empty_target_half():
    """(g).  bn_Bt0: ta3n_plan_create takes use_bn with no target videos (tests/test_bn_shapes_cpu.py), so both launches meet n == 0 for
    their target workgroups.  The reference cannot run this (BatchNorm1d on zero rows raises), so only what follows from the source
    half is asserted: its class logits against the oracle's source forward on the engine's parameters, finite parameters, and a target
    BatchNorm that receives no gradient and whose running statistics stay where they were."""
    name = "bn_Bt0"
    case = bs.CASES[name]
    eng = _engine(case, "AdaBN", True)
    f = _assert_branches(name, eng, True)
    assert f["rows"] == (case["Bs"] * case["T"], 0)
    start = bs.initial_running(case)
    cfg = bs.oracle_cfg(case)
    for s in range(2):
        xs, xt, ys, ns, nt = bs.batch(case, s)
        assert xt.shape[0] == 0 and nt == 0
        p = {k: v.detach().cpu().double() for k, v in eng.param_views().items()}
        _step(eng, case, xs, xt, ys, ns, nt, s)
        with torch.no_grad():
            want = orc.forward_domain(p, xs.double(), bs.BETA, cfg, domain="S")["out"]
        got = eng.outputs()["out"][:case["Bs"]].cpu().double()
        assert float((got - want).abs().max()) <= ls.logit_bound(want), (s, float((got - want).abs().max()))
        grads = eng.param_views(eng.G)
        for k in ("bn_shared_T.weight", "bn_shared_T.bias"):
            assert float(grads[k].abs().max()) == 0.0, (s, k)
        for k in ("bn_shared_S.weight", "bn_shared_S.bias"):
            assert float(grads[k].abs().max()) > 0.0, (s, k)
        assert torch.isfinite(eng.P).all() and torch.isfinite(eng.region("grad_norm")[:2]).all()
        assert torch.equal(eng.bn_running[1, 0].cpu(), start["bn_shared_T.running_mean"])
        assert torch.equal(eng.bn_running[1, 1].cpu(), start["bn_shared_T.running_var"])
        assert not torch.equal(eng.bn_running[0, 0].cpu(), start["bn_shared_S.running_mean"])
