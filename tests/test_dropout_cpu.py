"""Dropout ON, on the CPU: the launch plans executed with numpy in float64 (tests/plan_interp.py) against the float64 oracle on the masks
tests/dropout_masks.py builds from the element-id formulas alone - losses and every element of every gradient tensor.  This pins the
helper's formulas AND the plans' drop_ld / pad2 / gamma_kind / seed choice (the GEMM epilogues' EPI_DROP_I / EPI_DROP_V, the unfused
backward through dropout_v, the pointwise launches' specification) before any GPU time is spent; tests/test_gpu_dropout_parity.py then
holds the kernels to the same masks.

Bound: both sides are float64 and free-running (no ReLU synchronisation needed: a pre-activation within 1e-16 of zero does not occur),
so what is left is float64 summation order - rtol 1e-9 / atol 1e-12, what tests/test_plan_cpu.py asks of two float64 executions of one
plan (the dropout-off comparisons with the reference's fp32 fixtures there carry 1e-4 / 2e-5 for the fixtures' own precision)."""
import numpy as np
import pytest
import torch

from dropout_masks import (GAMMA, LR, batch, check_frame_pattern, check_video_pattern, dropout_masks, excluded, oracle_cases, preactivation,
                           rel_l2)
from golden_util import Golden, case_config
from oracle import ta3n_oracle as orc
from plan_interp import Interp
from ta3n_amd import _lib
from ta3n_amd.engine import dropout_seeds, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

ALL_FLAGS = (_lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN)
BETA = [0.75, 0.75, 0.5]
RTOL, ATOL = 1e-9, 1e-12


def hyper(Bs, Bt, T, ns, nt, p_i, p_v, step, gamma=0.003, clip=20.0, lr=2e-3):
    si, sv = dropout_seeds(step, 0)
    return dict(beta=list(BETA), gamma=gamma, lr=lr, momentum=0.9, weight_decay=1e-4, clip=clip, p_drop_i=p_i, p_drop_v=p_v, seed_i=si, seed_v=sv,
                inv_n_cls=1.0 / ns, inv_n_rel=1.0 / ((ns + nt) * (T - 1)) if T > 1 else 0.0, inv_n_vid=1.0 / (ns + nt),
                inv_n_frm=1.0 / ((ns + nt) * T), inv_n_ent=1.0 / (ns + nt), valid_source=ns, valid_target=nt, train=1)


def interp_step(plan, params, xs, xt, ys, hy, fused):
    """One forward + loss + backward of `plan` in the float64 interpreter; returns it (gradients in it.G, losses in the workspace)."""
    it = Interp(plan)
    it.set_params(params)
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:xs.size(0)] = ys.numpy()
    it.hy = hy
    it.G[:] = 0
    for grp in ((4,) if fused else (0, 1, 2)):
        it.run_group(grp)
    return it


def oracle_step(cfg, params, xs, xt, ys, ns, nt, mk, gamma=0.003, masks=None, **kw):
    """The float64 oracle on the helper's masks `mk` (dropout_masks()); gradients raw (clip=None)."""
    state = orc.TrainState(params={k: v.detach().double().clone() for k, v in params.items()}, lr=2e-3)
    return orc.train_step(state, xs.double(), xt.double(), ys, BETA, gamma, cfg, clip=None, n_src=ns, n_tgt=nt, masks=masks,
                          drop_i=mk["drop_i"], drop_v=mk["drop_v"], **kw)


def compare(it, res, what):
    """Losses and every element of every gradient tensor of an interpreter run against an oracle result."""
    L = it.ws[it.g.o_losses:it.g.o_losses + 6]
    parts = res["parts"]
    assert abs(L[0] - parts["loss"].item()) <= RTOL * abs(parts["loss"].item()) + ATOL, (what, "loss", L[0], parts["loss"].item())
    assert abs(L[1] - parts["loss_c"].item()) <= RTOL * abs(parts["loss_c"].item()) + ATOL, (what, "loss_c")
    if "loss_a" in parts:
        assert abs(L[2] + L[3] + L[4] - parts["loss_a"].item()) <= RTOL * abs(parts["loss_a"].item()) + ATOL, (what, "loss_a")
    if "loss_e" in parts:
        assert abs(L[5] - parts["loss_e"].item()) <= RTOL * abs(parts["loss_e"].item()) + ATOL, (what, "loss_e")
    got = it.get_params(it.G)
    live = {n for n, _, _, lv in it.plan.params if lv}
    assert live == set(res["grads"]), (what, live ^ set(res["grads"]))
    for k, w in res["grads"].items():
        w = w.double().numpy()
        assert np.abs(w).max() > 0 or k.endswith("shared_source.bias"), (what, k, "reference gradient is all zero")
        assert np.allclose(got[k], w, rtol=RTOL, atol=ATOL * max(1.0, np.abs(w).max())), (what, k, np.abs(got[k] - w).max(), np.abs(w).max())


TRN = dict(Bs=6, Bt=4, T=5, D=512, F=64, C=12)
RAGGED = dict(Bs=40, Bt=30, T=3, D=256, F=128, C=7)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape,p_i,p_v,valid", [(TRN, 0.5, 0.5, None), (TRN, 0.3, 0.8, None), (RAGGED, 0.3, 0.8, (37, 25))],
                         ids=["tiny_0.5_0.5", "tiny_0.3_0.8", "ragged_0.3_0.8"])
def test_trn_m_plan_with_dropout_matches_the_oracle_on_host_masks(shape, p_i, p_v, valid, fused):
    Bs, Bt, T, D, Fc, Cn = (shape[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    ns, nt = valid or (Bs, Bt)
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=p_i, dropout_v=p_v)
    params = synth_state(orc.param_shapes(cfg), seed=12 if shape is RAGGED else 11, scale="trained")      # (12: RAGGED_WSEED of the GPU test)
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=21)
    xs[ns:] = 0; xt[nt:] = 0
    step = 1
    mk = dropout_masks(*dropout_seeds(step, 0), p_i, p_v, Bs, Bt, T, Fc, 256)
    plan = _lib.Plan(Bs, Bt, T, D, Fc, Cn, ALL_FLAGS)
    it = interp_step(plan, params, xs, xt, ys, hyper(Bs, Bt, T, ns, nt, p_i, p_v, step), fused)
    res = oracle_step(cfg, params, xs, xt, ys, ns, nt, mk)
    g = it.g
    pre = torch.cat((res["src"]["pre_f1"], res["tgt"]["pre_f1"])).detach()
    check_frame_pattern(it.r(g.o_F1, (g.B * T, Fc)), pre, torch.cat(mk["keep_i"]), "F1")
    check_video_pattern(it.r(g.o_V, (g.B, 256)), it.r(g.o_Vd, (g.B, 256)), it.r(g.o_gVt, (g.B, 256)), torch.cat(mk["keep_v"]), p_v, "Vd")
    compare(it, res, (p_i, p_v, fused))


def test_the_comparison_sees_the_bugs_it_is_for():
    """Negative controls of the comparator on the tiny trn-m case: the oracle on masks of seed + 1, with drop_v left without its
    1 / (1 - p_v), and with the target rows' ids counted from 0 must each land far from the plan's gradients (worst per-tensor relative
    L2 above 100 x the GPU test's fp32 bound F32_MASKED_GRAD_REL_L2) - the plan itself agrees to 1e-9."""
    from ta3n_amd import tolerances as tol
    Bs, Bt, T, D, Fc, Cn = (TRN[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    p_i, p_v = 0.5, 0.5
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=p_i, dropout_v=p_v)
    params = synth_state(orc.param_shapes(cfg), seed=11, scale="trained")
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=21)
    si, sv = dropout_seeds(0, 0)
    it = interp_step(_lib.Plan(Bs, Bt, T, D, Fc, Cn, ALL_FLAGS), params, xs, xt, ys, hyper(Bs, Bt, T, Bs, Bt, p_i, p_v, 0), True)
    got = it.get_params(it.G)
    good = oracle_step(cfg, params, xs, xt, ys, Bs, Bt, dropout_masks(si, sv, p_i, p_v, Bs, Bt, T, Fc, 256))
    assert max(rel_l2(got, good["grads"]).values()) < 1e-9
    for name, mk in (("seed + 1", dropout_masks(si + 1, sv + 1, p_i, p_v, Bs, Bt, T, Fc, 256)),
                     ("drop_v unscaled", dropout_masks(si, sv, p_i, p_v, Bs, Bt, T, Fc, 256, scale_v=False)),
                     ("target rows from 0", dropout_masks(si, sv, p_i, p_v, Bs, Bt, T, Fc, 256, target_row0=0))):
        bad = oracle_step(cfg, params, xs, xt, ys, Bs, Bt, mk)
        assert max(rel_l2(got, bad["grads"]).values()) > 100 * tol.F32_MASKED_GRAD_REL_L2, name


def _avgpool_da():
    g = Golden("tiny_avgpool_da")
    c = case_config(g)
    cfg = lambda p_i, p_v: orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"], dropout_i=p_i, dropout_v=p_v,
                                      place_adv=c["place_adv"], add_loss_DA="none", use_attn="none", frame_aggregation="avgpool")
    return c, cfg, flags_from_options(c["place_adv"], "none", "none", "RevGrad", "uSv")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_avgpool_da_plan_with_dropout_matches_the_oracle_on_host_masks(fused):
    """TemPooling + RevGrad (config of tiny_avgpool_da): dropout_v on the F-wide mean feature (NV = F), p 0.3 / 0.8."""
    c, mkcfg, flags = _avgpool_da()
    Bs, Bt, T, D, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["C"], 0.3, 0.8
    cfg = mkcfg(p_i, p_v)
    Fc = cfg.feat_dim
    params = synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    mk = dropout_masks(*dropout_seeds(1, 0), p_i, p_v, Bs, Bt, T, Fc, Fc)
    plan = _lib.Plan(Bs, Bt, T, D, c["fc_dim"], Cn, flags, aggregation=_lib.AGG_AVGPOOL)
    it = interp_step(plan, params, xs, xt, ys, hyper(Bs, Bt, T, Bs, Bt, p_i, p_v, 1, gamma=0.0), fused)
    res = oracle_step(cfg, params, xs, xt, ys, Bs, Bt, mk, gamma=0.0)
    g = it.g
    pre = torch.cat((res["src"]["pre_f1"], res["tgt"]["pre_f1"])).detach()
    check_frame_pattern(it.r(g.o_F1, (g.B * T, Fc)), pre, torch.cat(mk["keep_i"]), "F1")
    check_video_pattern(it.r(g.o_V, (g.B, Fc)), it.r(g.o_Vd, (g.B, Fc)), it.r(g.o_gVt, (g.B, Fc)), torch.cat(mk["keep_v"]), p_v, "Vd")
    compare(it, res, ("avgpool", fused))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_avgpool_source_only_plan_with_dropout_matches_the_oracle_on_host_masks(fused):
    """TemPooling, source-only (config of tiny_avgpool; no adversarial flag): the PH_POOL_CLS launch - mean, dropout_v, classifier,
    cross-entropy and the way back to gZ1 in one kernel - at p 0.3 / 0.8."""
    c = case_config(Golden("tiny_avgpool"))
    Bs, Bt, T, D, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["C"], 0.3, 0.8
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=c["fc_dim"], dropout_i=p_i, dropout_v=p_v, place_adv=("N", "N", "N"),
                     add_loss_DA="none", use_attn="none", frame_aggregation="avgpool")
    Fc = cfg.feat_dim
    params = synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    mk = dropout_masks(*dropout_seeds(1, 0), p_i, p_v, Bs, Bt, T, Fc, Fc)
    plan = _lib.Plan(Bs, Bt, T, D, c["fc_dim"], Cn, 0, aggregation=_lib.AGG_AVGPOOL)
    from plan_interp import PH_POOL_CLS
    it = interp_step(plan, params, xs, xt, ys, hyper(Bs, Bt, T, Bs, Bt, p_i, p_v, 1, gamma=0.0), fused)
    assert any(ph.kind == PH_POOL_CLS for ph in it.phases if ph.group == (4 if fused else 0))
    res = oracle_step(cfg, params, xs, xt, ys, Bs, Bt, mk, gamma=0.0)
    g = it.g
    pre = torch.cat((res["src"]["pre_f1"], res["tgt"]["pre_f1"])).detach()
    check_frame_pattern(it.r(g.o_F1, (g.B * T, Fc)), pre, torch.cat(mk["keep_i"]), "F1")
    gZ1 = np.abs(it.r(g.o_gZ1, (g.B, T, Fc))).max(1)      # (no gVt in this plan: the kernel goes from the logit gradient to gZ1 at once)
    check_video_pattern(it.r(g.o_V, (g.B, Fc)), it.r(g.o_Vd, (g.B, Fc)), gZ1, torch.cat(mk["keep_v"]), p_v, "Vd")
    assert gZ1[:Bs].max() > 0
    compare(it, res, ("avgpool source-only", fused))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("p_i,p_v", [(0.5, 0.5), (0.3, 0.8)])
def test_adabn_plan_with_dropout_matches_the_oracle_on_host_masks(p_i, p_v, fused):
    """use_bn AdaBN (config of tiny_adabn): dropout_i leaves the GEMM epilogue for the BatchNorm launch; the pattern is checked on the
    post-BatchNorm pre-activation."""
    c = case_config(Golden("tiny_adabn"))
    Bs, Bt, T, D, Cn = c["Bs"], c["Bt"], c["T"], c["D"], c["C"]
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=c["fc_dim"], dropout_i=p_i, dropout_v=p_v, use_bn=c["use_bn"])
    Fc = cfg.feat_dim
    params = synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    mk = dropout_masks(*dropout_seeds(1, 0), p_i, p_v, Bs, Bt, T, Fc, 256)
    plan = _lib.Plan(Bs, Bt, T, D, c["fc_dim"], Cn, ALL_FLAGS | _lib.FLAG_BN_SHARED)
    it = interp_step(plan, params, xs, xt, ys, hyper(Bs, Bt, T, Bs, Bt, p_i, p_v, 1), fused)
    res = oracle_step(cfg, params, xs, xt, ys, Bs, Bt, mk)
    g = it.g
    pre = torch.cat((res["src"]["pre_f1"], res["tgt"]["pre_f1"])).detach()
    check_frame_pattern(it.r(g.o_F1, (g.B * T, Fc)), pre, torch.cat(mk["keep_i"]), "F1")
    check_video_pattern(it.r(g.o_V, (g.B, 256)), it.r(g.o_Vd, (g.B, 256)), it.r(g.o_gVt, (g.B, 256)), torch.cat(mk["keep_v"]), p_v, "Vd")
    compare(it, res, ("adabn", p_i, p_v, fused))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_stacked_layer_draws_the_offset_stream_in_the_interpreter(fused):
    """tiny_addfc2 with dropout on: layer 2's nonzero pattern is the helper's mask at the pad2 offset (B T F past layer 1's ids), NOT
    layer 1's mask - the kernel's rule (ta3n_gemm_kernel.h).  An interpreter that ignores Task.pad2 repeats layer 1's mask and fails here."""
    g_ = Golden("tiny_addfc2")
    c = case_config(g_)
    Bs, Bt, T, D, Fc, Cn, p_i, p_v = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], 0.5, 0.3
    plan = _lib.Plan(Bs, Bt, T, D, Fc, Cn, ALL_FLAGS, shared_fc_layers=2)
    params = synth_state({n: s for n, _, s, _ in plan.params}, seed=c["wseed"], scale=c["wscale"])
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    it = interp_step(plan, params, xs, xt, ys, hyper(Bs, Bt, T, Bs, Bt, p_i, p_v, 0), fused)
    B = Bs + Bt
    seeds = dropout_seeds(0, 0)
    m1 = dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, 256, layer=1)
    m2 = dropout_masks(*seeds, p_i, p_v, Bs, Bt, T, Fc, 256, layer=2)
    k1, k2 = torch.cat(m1["keep_i"]), torch.cat(m2["keep_i"])
    assert 0.4 < (k1 == k2).double().mean().item() < 0.6          # two independent p = 0.5 masks
    P = {k: v.double() for k, v in params.items()}
    X = torch.cat((xs, xt), 0).double().reshape(B * T, D)
    Fl1 = torch.from_numpy(it.r(plan.region("F_l1")[0], (B * T, Fc)).copy())
    F2 = torch.from_numpy(it.r(it.g.o_F1, (B * T, Fc)).copy())
    pre1 = X @ P["fc_feature_shared_source.weight"].t() + P["fc_feature_shared_source.bias"]
    pre2 = Fl1 @ P["fc_feature_shared_2_source.weight"].t() + P["fc_feature_shared_2_source.bias"]
    check_frame_pattern(Fl1, pre1, k1, "layer 1")
    check_frame_pattern(F2, pre2, k2, "layer 2")
    on = (pre2 > 0) & ~excluded(pre2)[0]
    assert not torch.equal((F2 != 0)[on], (k1 == 1)[on])          # ... and it is not layer 1's mask once more
    assert torch.allclose(F2[on & (k2 == 1)], 2.0 * pre2[on & (k2 == 1)], rtol=1e-12)      # kept units carry 1 / (1 - p_i)


def test_excluded_shares_of_the_gpu_cases(capsys):
    """The condition of tests/test_gpu_dropout_parity.py's pattern check, from the float64 oracle alone: at the seeds that file uses,
    at most 1 % of the shared frame layer's pre-activations lie within 1e-4 of the tensor's largest magnitude of the ReLU kink - in
    every step (the oracle, on the helper's masks, advances the parameters the way the engine will)."""
    lines = []
    for case, (mkcfg, shape, wseed, wscale, xseed, ps, valid) in oracle_cases().items():
        Bs, Bt, T, Fc = shape["Bs"], shape["Bt"], shape["T"], shape["F"]
        for p_i, p_v in ps:
            cfg = mkcfg(p_i, p_v)
            NV = Fc if cfg.frame_aggregation == "avgpool" else 256
            state = orc.TrainState(params=synth_state(orc.param_shapes(cfg), seed=wseed, scale=wscale), lr=LR)
            for s, (ns, nt) in enumerate(valid):
                xs, xt, ys = batch(shape, xseed, s, ns, nt)
                share = excluded(preactivation(cfg, state.params, xs, xt))[1]
                lines.append(f"{case} p {p_i}/{p_v} step {s}: excluded share {share:.3%}")
                assert share <= 0.01, lines[-1]
                mk = dropout_masks(*dropout_seeds(s, 0), p_i, p_v, Bs, Bt, T, Fc, NV)
                orc.train_step(state, xs, xt, ys, BETA, 0.0 if NV == Fc else GAMMA, cfg, clip=20.0, n_src=ns, n_tgt=nt,
                               drop_i=tuple(m.float() for m in mk["drop_i"]), drop_v=tuple(m.float() for m in mk["drop_v"]))
    for name in ("tiny_addfc2", "tiny_faf_T5"):      # (first layer; the second layer of add_fc 2 is checked on the engine's own layer-1 output)
        c = case_config(Golden(name))
        plan = _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], ALL_FLAGS, shared_fc_layers=2 if name == "tiny_addfc2" else 1)
        P = synth_state({n: s_ for n, _, s_, _ in plan.params}, seed=c["wseed"], scale=c["wscale"])      # (the engine's own parameter table)
        xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=c["xseed"])
        pre = torch.cat((xs, xt)).double().reshape(-1, c["D"]) @ P["fc_feature_shared_source.weight"].double().t() + P["fc_feature_shared_source.bias"].double()
        share = excluded(pre)[1]
        lines.append(f"{name} step 0: excluded share {share:.3%}")
        assert share <= 0.01, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_oracle_mcd_reversed_pass_takes_its_own_masks():
    """oracle.train_step(drop_rev=): None is the behaviour of before (the reversed pass reuses the first pass's target masks, bit for
    bit); its own masks change loss_s and the gradients; masks_rev set to the pass's own ReLU patterns changes nothing."""
    c = case_config(Golden("tiny_mcd"))
    Bs, Bt, T, D, Fc, Cn = c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"]
    cfg = orc.Config(num_class=Cn, num_segments=T, feature_dim=D, fc_dim=Fc, dropout_i=0.5, dropout_v=0.5, ens_DA="MCD")
    params = synth_state(orc.param_shapes(cfg), seed=c["wseed"], scale=c["wscale"])
    xs, xt, ys, yt = synth_batch(Cn, T, D, Bs, Bt, seed=c["xseed"])
    assert excluded(preactivation(cfg, params, xs, xt))[1] <= 0.01
    s1 = dropout_seeds(0, 0)
    mk1 = dropout_masks(*s1, 0.5, 0.5, Bs, Bt, T, Fc, 256)
    mk2 = dropout_masks(*dropout_seeds(s1[0] ^ 0x5bd1e995, 0), 0.5, 0.5, Bs, Bt, T, Fc, 256)
    run = lambda **kw: oracle_step(cfg, params, xs, xt, ys, Bs, Bt, mk1, mu=c["mu"], **kw)
    base, same = run(), run(drop_rev=(mk1["drop_i"][1], mk1["drop_v"][1]))
    assert all(torch.equal(base["grads"][k], same["grads"][k]) for k in base["grads"]) and torch.equal(base["loss"], same["loss"])
    own = run(drop_rev=(mk2["drop_i"][1], mk2["drop_v"][1]))
    assert abs(own["parts"]["loss_s"].item() - base["parts"]["loss_s"].item()) > 1e-6
    assert max(rel_l2(own["grads"], base["grads"]).values()) > 1e-3
    pats = {k: v > 0 for k, v in own["tgt_rev"]["hidden"].items()}
    forced = run(drop_rev=(mk2["drop_i"][1], mk2["drop_v"][1]), masks_rev=pats)
    assert max(rel_l2(forced["grads"], own["grads"]).values()) < 1e-12
