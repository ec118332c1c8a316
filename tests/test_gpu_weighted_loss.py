"""The weighted criteria on the MI355X (--weighted_class_loss / --weighted_class_loss_DA, reference main.py:156-167, 205-206; TrainEngine
class_weights / domain_weights): every kernel that forms a class or a domain cross-entropy against F.cross_entropy(..., weight=w) on the
oracle's forward (tests/weighted_loss_cases.py): loss terms, logits, the logit gradients, every gradient element of one step without
clipping and the parameters after it, under the bounds of ta3n_amd/tolerances.py for the same tensors.  Each case first asserts, on the
reference alone, that the weighted and the unweighted logit gradients are more than 100 x that bound apart."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import weighted_loss_cases as wl
from oracle import ta3n_oracle as orc
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(name, cw, dw, **more):
    from ta3n_amd.engine import TrainEngine
    c = wl.CASES[name]
    kw = dict(wl.case_setup(name)[1], **more)
    clip = kw.pop("clip", 0.0)      # 0: no clipping
    return TrainEngine(c["Bs"], c["Bt"], c["T"], wl.D, wl.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=clip, class_weights=cw,
                       domain_weights=dw, **kw)


def _assert_distinct(name):
    for grp in wl.distinct_from_unweighted(name):
        assert max(grp.values()) > 100 * wl.LOGIT_GRAD_REL_L2, (name, grp)


def _grad_metrics(got, want):
    out = {}
    for k, w in want.items():
        w = w.detach().double().cpu()
        g = got[k].detach().double().cpu().reshape(w.shape)
        d = g - w
        out[k] = ((d.norm() / (w.norm() + 1e-300)).item(), d.abs().max().item() / (w.abs().max().item() + 1e-300))
    return out


def _compare_step(name, eng, ref, cfg, ns, nt, cw, dw, arith="f32", frame_logit_grads=True):
    """Everything one step leaves behind against the reference step `ref`."""
    Bs = eng.Bs
    # logits (valid rows: the padding rows of the engine's batch are computed too, the reference's as well - same inputs)
    o = eng.outputs()
    bf16 = arith == "bf16"
    for key, want in (("out", ref["out"]), ("pred_vid", ref["pred_vid"])):
        if key not in o:
            continue
        got = o[key].cpu().reshape(want.shape)
        err = (got - want).abs().max().item()
        bound = tol.BF16_LOGIT_REL_RMS * want.pow(2).mean().sqrt().item() + 1e-7 if bf16 else tol.LOGIT_ATOL
        print(f"[weighted {name} {arith}] {key}: max err {err:.2e} (bound {bound:.1e})")
        assert err <= bound, (name, key, err)
    # loss terms
    L = eng.losses()
    P = ref["parts"]
    want_l = dict(loss=P["loss"] - P.get("loss_c2", 0.0) - P.get("loss_s", 0.0), loss_c=P["loss_c1"], loss_a=P.get("loss_a", 0.0),
                  loss_e=P.get("loss_e", 0.0))
    got_l = dict(loss=L["loss"], loss_c=L["loss_c"], loss_a=L["loss_adv_rel"] + L["loss_adv_vid"] + L["loss_adv_frm"], loss_e=L["loss_e"])
    if cfg.frame_aggregation == "trn-m":
        for k in ("loss_adv_rel", "loss_adv_vid", "loss_adv_frm"):
            want_l[k], got_l[k] = P.get(k, 0.0), L[k]
    rel = tol.BF16_LOSS_REL if bf16 else 2e-4
    for k, w in want_l.items():
        print(f"[weighted {name} {arith}] {k}: {got_l[k]:.6f} want {w:.6f}")
        if cfg.ens_DA == "MCD" and k in ("loss", "loss_e"):
            continue      # (the entropy term of the target rows moves to the second pass: compared through loss_e_shift by the MCD case)
        assert abs(got_l[k] - w) <= rel * max(1.0, abs(w)), (name, k, got_l[k], w)
    # logit gradients: the tensors the weights act on directly, each domain half on its own
    if not bf16:
        got_lg = wl.engine_logit_grads(eng, frame=frame_logit_grads)
        for grp in wl.affected_logit_grads(cfg, cw, dw):
            for k in grp:
                if k not in got_lg or (cfg.ens_DA == "MCD" and k != "gY"):
                    continue
                want = ref["logit_grads"][k]
                got = got_lg[k]
                if cfg.ens_DA == "MCD":
                    got, want = got[:Bs], want[:Bs]
                d = wl.rel_l2(got, want)
                print(f"[weighted {name} {arith}] logit gradient {k}: rel. L2 {d:.2e} (bound {wl.LOGIT_GRAD_REL_L2:.1e})")
                assert d <= wl.LOGIT_GRAD_REL_L2, (name, k, d)
    # every gradient element
    got_g = {k: v for k, v in eng.param_views(eng.G).items() if k in ref["grads"]}
    want_g = dict(ref["grads"])
    if cfg.use_bn != "none":      # a bias in front of a BatchNorm has no gradient: both sides hold round-off there (as tests/limit_shapes.py treats it)
        k = "fc_feature_shared_source.bias"
        assert float(got_g.pop(k).abs().max()) <= tol.F32_ATOL and float(want_g.pop(k).abs().max()) <= tol.F32_ATOL
    m = _grad_metrics(got_g, want_g)
    l2_tol, med_tol, mx_tol = {"f32": (tol.F32_GRAD_REL_L2, tol.F32_GRAD_REL_L2_MEDIAN, tol.F32_GRAD_MAX_SCALE),
                               "f32x3": (tol.F32X3_GRAD_REL_L2, tol.F32X3_GRAD_REL_L2_MEDIAN, tol.F32X3_GRAD_MAX_SCALE),
                               "bf16": (tol.BF16_GRAD_REL_L2, tol.BF16_GRAD_REL_L2_MEDIAN, tol.BF16_GRAD_MAX_SCALE)}[arith]
    worst = max(m, key=lambda k: m[k][0])
    med = float(np.median([v[0] for v in m.values()]))
    print(f"[weighted {name} {arith}] gradients: median rel. L2 {med:.2e} (bound {med_tol:.1e}), worst {worst} {m[worst][0]:.2e} max/scale {m[worst][1]:.2e}")
    assert set(m) == set(want_g) and set(eng.live_names()) >= set(m)
    for k, (l2, mx) in m.items():
        assert l2 <= l2_tol and mx <= mx_tol, (name, k, l2, mx)
    assert med <= med_tol, (name, med)
    return m


def _compare_params(name, eng, ref, arith="f32"):
    new = eng.param_views()
    for k, v in ref["params"].items():
        got = new[k].cpu()
        if arith == "bf16":
            d = (got.double() - v.double()).norm().item()
            assert d <= tol.BF16_GRAD_REL_L2 * max((ref["params"][k] - ref["start"][k]).double().norm().item(), 1e-30) + 1e-9, (name, k, d)
        else:
            assert torch.allclose(got, v.float(), rtol=tol.F32_RTOL, atol=tol.F32_ATOL), (name, k, (got - v).abs().max().item())


def _run_case(name, arith="f32", engine_more=None, oracle_cfg=None, frame_logit_grads=True):
    _assert_distinct(name)
    cfg, kw, params, xs, xt, ys, ns, nt, cw, dw = wl.case_setup(name)
    eng = _engine(name, cw, dw, **(engine_more or {}))
    eng.load_state(params)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(list(wl.BETA), wl.GAMMA, wl.LR, valid_source=ns, valid_target=nt)
    torch.cuda.synchronize()
    rcfg = oracle_cfg or cfg
    ref = wl.reference_step(rcfg, params, xs, xt, ys, ns, nt, cw, dw, mu=getattr(eng, "mu", 0.0))
    ref["start"] = params
    _compare_step(name, eng, ref, cfg, ns, nt, cw, dw, arith=arith, frame_logit_grads=frame_logit_grads)
    _compare_params(name, eng, ref, arith=arith)
    return eng, ref


@pytest.mark.parametrize("name", ["trn_fp32", "trn_ragged", "trn_70", "trn_C64", "trn_C1", "class_only", "domain_only", "adv_YNY", "adv_NYN",
                                  "adabn", "addfc2"])
def test_fused_step_with_weighted_criteria(name):
    """The fused heads kernel's class CE (stage D) and its video / relation / frame domain CEs: both weights, one of them, padding rows that
    carry the heaviest class, a label sum of more than one trip per lane (70 source rows), 64 classes and 1, levels switched off, the
    BatchNorm and stacked-layer variants of the step."""
    eng, _ = _run_case(name)
    assert eng.fused
    assert ("class weights" in eng.describe()) == wl.CASES[name].get("cw", True)
    assert ("domain weights" in eng.describe()) == wl.CASES[name].get("dw", True)


@pytest.mark.parametrize("waves", [4, 8])
def test_heads_kernel_of_four_and_of_eight_waves(waves):
    L = _lib.lib()
    try:
        assert L.ta3n_set_heads_waves(waves) == 0
        eng, _ = _run_case("trn_ragged")
        assert L.ta3n_get_heads_waves(eng.plan.handle) == waves
    finally:
        L.ta3n_set_heads_waves(0)


def test_two_videos_per_heads_workgroup():
    """More than 224 videos: heads_vpw 2 (an odd count: the last workgroup holds one video)."""
    from ta3n_amd.engine import TrainEngine
    Bs, Bt, T, C = 150, 77, 3, 12
    cfg = orc.Config(num_class=C, num_segments=T, feature_dim=wl.D, fc_dim=wl.FC, dropout_i=0.0, dropout_v=0.0)
    params = synth_state(orc.param_shapes(cfg), seed=11)
    from ta3n_amd.synthetic import synth_batch
    xs, xt, _, _ = synth_batch(C, T, wl.D, Bs, Bt, seed=21)
    cw = wl.class_weights(C)
    p = np.array(wl.skewed_counts(C), dtype=np.float64)
    ys = torch.tensor(np.random.default_rng(3).choice(C, size=Bs, p=p / p.sum()), dtype=torch.long)
    ns, nt = 149, 75
    ys[ns:] = int(np.argmax(cw))
    eng = TrainEngine(Bs, Bt, T, wl.D, wl.FC, C, dropout_i=0.0, dropout_v=0.0, clip=0.0, class_weights=cw, domain_weights=wl.DOMAIN_W)
    assert eng.fused and eng.B > 224      # (the plan builder's threshold for two videos per workgroup)
    eng.load_state(params)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(list(wl.BETA), wl.GAMMA, wl.LR, valid_source=ns, valid_target=nt)
    torch.cuda.synchronize()
    ref = wl.reference_step(cfg, params, xs, xt, ys, ns, nt, cw, wl.DOMAIN_W)
    ref["start"] = params
    u = wl.reference_step(cfg, params, xs, xt, ys, ns, nt, None, None)
    assert wl.rel_l2(u["logit_grads"]["gY"], ref["logit_grads"]["gY"]) > 100 * wl.LOGIT_GRAD_REL_L2
    _compare_step("vpw2", eng, ref, cfg, ns, nt, cw, wl.DOMAIN_W)
    _compare_params("vpw2", eng, ref)


def test_unfused_lists_and_frame_attention():
    """The `loss` kernel of the unfused launch lists, and --use_attn_frame TransAttn, which runs on them."""
    eng, _ = _run_case("unfused")
    assert not eng.fused
    # frame attention: the oracle holds no frame attention - the engine's own unweighted run is the reference of everything the weights
    # do not touch, so here the WEIGHTED logit gradients are checked against the weighted criterion on the engine's logits
    cfg, kw, params, xs, xt, ys, ns, nt, cw, dw = wl.case_setup("trn_ragged")
    from ta3n_amd.engine import TrainEngine, flags_from_options
    c = wl.CASES["trn_ragged"]
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], wl.D, wl.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=0.0, class_weights=cw, domain_weights=dw,
                      flags=flags_from_options(use_attn_frame="TransAttn"))
    assert eng.frame_attn and not eng.fused
    eng.load_state(params)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.set_hyper(list(wl.BETA), 0.0, wl.LR, valid_source=ns, valid_target=nt)      # gamma 0: gY and gPf are the two criteria alone
    eng.forward(); eng.loss()
    torch.cuda.synchronize()
    o = eng.outputs()
    y = o["out"].cpu().double().requires_grad_(True)
    pf = o["pred_frm"].cpu().double().requires_grad_(True)
    Bs, T = c["Bs"], c["T"]
    loss_c = F.cross_entropy(y[:ns], ys[:ns], weight=torch.tensor(cw, dtype=torch.float64))
    pd = torch.cat((pf[:ns].reshape(-1, 2), pf[Bs:Bs + nt].reshape(-1, 2)))
    lab = torch.cat((torch.zeros(ns * T), torch.ones(nt * T))).long()
    loss_f = F.cross_entropy(pd, lab, weight=torch.tensor(dw, dtype=torch.float64))
    gy, gpf = torch.autograd.grad(loss_c + loss_f, (y, pf))
    assert wl.rel_l2(eng.region("gY", (eng.B, eng.C)), gy) <= wl.LOGIT_GRAD_REL_L2
    assert wl.rel_l2(eng.region("gPf", (eng.B, T, 2)), gpf) <= wl.LOGIT_GRAD_REL_L2
    L = eng.losses()
    for got, want in ((L["loss_c"], float(loss_c.detach())), (L["loss_adv_frm"], float(loss_f.detach()))):
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (got, want)
    # ... and the backward launches of the frame-attention lists under the flag: a whole step with class weights all 1 and equal domain weights
    # against the unflagged engine's (the oracle holds no frame attention), every gradient tensor and every parameter
    runs = []
    for cw1, dw1 in (([1.0] * c["C"], (0.5, 0.5)), (None, None)):
        e = TrainEngine(c["Bs"], c["Bt"], c["T"], wl.D, wl.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=0.0, class_weights=cw1, domain_weights=dw1,
                        flags=flags_from_options(use_attn_frame="TransAttn"))
        e.load_state(params)
        e.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        e.train_step(list(wl.BETA), wl.GAMMA, wl.LR, valid_source=ns, valid_target=nt)
        torch.cuda.synchronize()
        runs.append(({k: v.clone().cpu() for k, v in e.param_views(e.G).items() if k in set(e.live_names())}, {k: v.clone().cpu() for k, v in e.param_views().items()}))
    (g1, p1), (g0, p0) = runs
    m = _grad_metrics(g1, g0)
    assert m and all(l2 <= tol.F32_GRAD_REL_L2_MEDIAN for l2, _ in m.values()), max(m.items(), key=lambda kv: kv[1][0])
    assert all(torch.allclose(p1[k], p0[k], rtol=tol.F32_RTOL, atol=tol.F32_ATOL) for k in p0)
    assert any(not torch.equal(p0[k], params[k]) for k in p0)


@pytest.mark.parametrize("name", ["avgpool_da", "avgpool_src"])
def test_avgpool_with_weighted_criteria(name):
    """TemPooling with the RevGrad branches (loss kernel: the video-level CE counted twice) and source-only (pool_cls)."""
    eng, _ = _run_case(name)
    kinds = [ph["kind"] for ph in eng.plan.description["phases"]]
    assert (7 in kinds) == (name == "avgpool_src")      # PH_POOL_CLS


def test_mcd_both_classifiers():
    """ens_DA MCD: ta3n_mcd_source_loss is the weighted CE of the second classifier, its logit gradient lands in gY2; every parameter gradient
    of the two passes against autograd."""
    from ta3n_amd.engine import TrainEngine
    name = "trn_ragged"
    _assert_distinct(name)
    cfg, kw, params, xs, xt, ys, ns, nt, cw, dw = wl.case_setup(name)
    cfg = orc.Config(**dict(cfg.__dict__, ens_DA="MCD"))
    params = synth_state(wl.param_shapes(cfg), seed=11)
    c = wl.CASES[name]
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], wl.D, wl.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=0.0, class_weights=cw, domain_weights=dw,
                      ens_DA="MCD", mu=0.4)
    eng.load_state(params)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(list(wl.BETA), wl.GAMMA, wl.LR, valid_source=ns, valid_target=nt)
    torch.cuda.synchronize()
    ref = wl.reference_step(cfg, params, xs, xt, ys, ns, nt, cw, dw, mu=0.4)
    ref["start"] = params
    P = ref["parts"]
    assert abs(float(eng.loss_c2) - P["loss_c2"]) <= 2e-4 * max(1.0, abs(P["loss_c2"])), (float(eng.loss_c2), P["loss_c2"])
    assert abs(float(eng.loss_s) - P["loss_s"]) <= 2e-4
    total = eng.losses()["loss"] + float(eng.loss_c2) + float(eng.loss_s) + (float(eng.loss_e_shift[0]) if eng.loss_e_shift is not None else 0.0)
    assert abs(total - P["loss"]) <= 2e-4 * max(1.0, abs(P["loss"])), (total, P["loss"])
    g2 = eng.region("gY2", (eng.B, eng.C))[:c["Bs"]]
    assert wl.rel_l2(g2, ref["logit_grads"]["gY2_s"]) <= wl.LOGIT_GRAD_REL_L2
    _compare_step("mcd", eng, ref, cfg, ns, nt, cw, dw)
    _compare_params("mcd", eng, ref)


@pytest.mark.parametrize("arith", ["bf16", "f32x3"])
def test_other_arithmetics(arith):
    """bf16 against the bf16-operand oracle policy and its bounds (tests/test_gpu_bf16.py), the split arithmetic against the fp32 reference."""
    name = "trn_fp32"
    cfg = wl.case_setup(name)[0]
    if arith == "bf16":
        _run_case(name, arith="bf16", engine_more=dict(bf16=True, bf16_store=True),
                  oracle_cfg=orc.Config(**dict(cfg.__dict__, arithmetic="bf16", bf16_twins=True)))
    else:
        _run_case(name, arith="f32x3", engine_more=dict(f32_split=True))


def test_adam_two_steps():
    """--optimizer Adam: the weighted gradients through two updates - the parameters after the second step, and exp_avg / exp_avg_sq, against
    torch.optim.Adam on the reference gradients."""
    name = "trn_fp32"
    cfg, kw, params, xs, xt, ys, ns, nt, cw, dw = wl.case_setup(name)
    eng = _engine(name, cw, dw, optimizer="Adam", weight_decay=1e-4)
    eng.load_state(params)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam([p[k] for k in sorted(p)], 1e-3, weight_decay=1e-4)
    for s in range(2):
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step(list(wl.BETA), wl.GAMMA, 1e-3, valid_source=ns, valid_target=nt)
        torch.cuda.synchronize()
        ref = wl.reference_step(cfg, {k: v.detach() for k, v in p.items()}, xs, xt, ys, ns, nt, cw, dw)
        opt.zero_grad()
        for k, g in ref["grads"].items():
            p[k].grad = g.clone()
        opt.step()
    bound = tol.F32_GRAD_REL_L2 * tol.GOLDEN_DRIFT_FACTOR
    named = {id(p[k]): k for k in p}
    for prm, st in opt.state.items():
        k = named[id(prm)]
        m_view, v_view = eng.adam_views()[k]
        for got, want in ((m_view, st["exp_avg"]), (v_view, st["exp_avg_sq"])):
            assert wl.rel_l2(got, want) <= bound, (k, wl.rel_l2(got, want))
    # the parameters after two steps, every tensor (the second step stands on parameters that differ by the first one's round-off)
    new = eng.param_views()
    live = set(eng.live_names())
    assert {named[id(prm)] for prm in opt.state} == live
    worst = 0.0
    for k, v in p.items():
        got, want = new[k].cpu(), v.detach()
        worst = max(worst, (got - want).abs().max().item())
        assert torch.allclose(got, want, rtol=tol.F32_RTOL * tol.GOLDEN_DRIFT_FACTOR, atol=tol.F32_ATOL * tol.GOLDEN_DRIFT_FACTOR), \
            (k, (got - want).abs().max().item())
        if k in live:
            assert not torch.equal(got, params[k]), k      # (it moved)
    print(f"[weighted adam] parameters after two steps: max |got - want| {worst:.2e}")


def test_three_steps_in_one_call_on_device_gathered_batches():
    """ta3n_train_steps with the batches gathered on the device from a FeatureStore: the labels, and with them the sum of the weights, change
    every step and never pass through the host.  Losses of the last step and the final parameters against the same three steps on the
    reference side."""
    from ta3n_amd.engine import TrainEngine
    from ta3n_amd.feature_store import FeatureStore
    Bs, Bt, T, C, n = 6, 4, 5, 12, 3
    cw, dw = wl.class_weights(C), wl.DOMAIN_W
    gen = torch.Generator().manual_seed(9)

    def store(n_videos, labels):
        nf = torch.tensor([T + (3 * v) % 7 for v in range(n_videos)])
        rows = torch.randn(int(nf.sum()), wl.D, generator=gen).abs()
        return FeatureStore.from_tensors(rows.cuda().contiguous(), nf.cuda(), labels.cuda())
    heavy = int(np.argmax(cw))
    lab_s = torch.tensor([(5 * v) % C for v in range(16)])
    lab_s[::5] = heavy
    src, tgt = store(16, lab_s), store(9, torch.zeros(9, dtype=torch.long))
    ids_s = torch.stack([torch.randperm(16, generator=gen)[:Bs] for _ in range(n)]).to(torch.int32).cuda()
    ids_t = torch.stack([torch.randperm(9, generator=gen)[:Bt] for _ in range(n)]).to(torch.int32).cuda()
    sums = {round(sum(cw[int(lab_s[i])] for i in row), 3) for row in ids_s.cpu().tolist()}
    assert len(sums) == n      # a normaliser of its own per step
    cfg = orc.Config(num_class=C, num_segments=T, feature_dim=wl.D, fc_dim=wl.FC, dropout_i=0.0, dropout_v=0.0)
    params = synth_state(orc.param_shapes(cfg), seed=11)
    eng = TrainEngine(Bs, Bt, T, wl.D, wl.FC, C, dropout_i=0.0, dropout_v=0.0, clip=20.0, class_weights=cw, domain_weights=dw)
    eng.load_state(params)
    sched = [(list(wl.BETA), wl.GAMMA, wl.LR) for _ in range(n)]
    eng.train_steps(sched, feeds=((src, ids_s), (tgt, ids_t)))
    eng.flush()
    torch.cuda.synchronize()
    cur, mom, ref = params, None, None
    for k in range(n):
        xs, ys = src.gather(ids_s[k], T)
        xt, _ = tgt.gather(ids_t[k], T)
        ref = wl.reference_step(cfg, cur, xs.cpu().clone(), xt.cpu().clone(), ys.cpu().long(), Bs, Bt, cw, dw, momentum=mom, clip=20.0)
        cur, mom = ref["params"], ref["momentum"]
    L = eng.losses()
    for k, w in (("loss", ref["parts"]["loss"]), ("loss_c", ref["parts"]["loss_c1"])):
        assert abs(L[k] - w) <= 2e-4 * max(1.0, abs(w)), (k, L[k], w)
    new = eng.param_views()
    for k, v in cur.items():
        assert torch.allclose(new[k].cpu(), v, rtol=tol.F32_RTOL, atol=tol.F32_ATOL), (k, (new[k].cpu() - v).abs().max().item())


def test_validation_loss_is_the_batch_weighted_average_of_weighted_means():
    """evaluate_batch over two batches of 5 and 3 videos: metrics[0] / metrics[3] is main.validate's figure (criterion(pred, label) per batch,
    averaged by batch size); top-1 / top-5 and the confusion matrix are those of the unweighted engine."""
    from ta3n_amd.engine import TrainEngine
    from ta3n_amd.synthetic import synth_batch
    Bs, Bt, T, C = 6, 4, 5, 12
    cw = wl.class_weights(C)
    cfg = orc.Config(num_class=C, num_segments=T, feature_dim=wl.D, fc_dim=wl.FC, dropout_i=0.0, dropout_v=0.0)
    params = synth_state(orc.param_shapes(cfg), seed=11)
    x, _, _, _ = synth_batch(C, T, wl.D, 8, 1, seed=33)
    y = torch.tensor([int(np.argmax(cw)), 1, 2, 3, 1, 5, int(np.argmin(cw)), 7])
    res = {}
    for weighted in (True, False):
        eng = TrainEngine(Bs, Bt, T, wl.D, wl.FC, C, dropout_i=0.0, dropout_v=0.0, class_weights=cw if weighted else None)
        eng.load_state(params)
        eng.evaluate_batch(x[:5].cuda(), y[:5].cuda(), reset=True)
        logits = [eng.outputs()["out"][:5].cpu().clone()]
        eng.evaluate_batch(x[5:].cuda(), y[5:].cuda())
        logits.append(eng.outputs()["out"][:3].cpu().clone())
        res[weighted] = (eng.eval_results(), logits)
    (rw, lw), (ru, lu) = res[True], res[False]
    w64 = torch.tensor(cw, dtype=torch.float64)
    want = (5 * F.cross_entropy(lw[0].double(), y[:5], weight=w64) + 3 * F.cross_entropy(lw[1].double(), y[5:], weight=w64)) / 8
    plain = (5 * F.cross_entropy(lu[0].double(), y[:5]) + 3 * F.cross_entropy(lu[1].double(), y[5:])) / 8
    assert abs(float(want) - float(plain)) > 100 * 2e-4 * max(1.0, float(want))
    assert abs(rw["loss"] - float(want)) <= 2e-4 * max(1.0, float(want)), (rw["loss"], float(want))
    assert abs(ru["loss"] - float(plain)) <= 2e-4 * max(1.0, float(plain))
    assert rw["n"] == ru["n"] == 8 and rw["prec1"] == ru["prec1"] and rw["prec5"] == ru["prec5"] and torch.equal(rw["confusion"], ru["confusion"])


def test_unit_weights_equal_the_unflagged_step(capsys):
    """Class weights all 1 and equal domain weights: the unweighted mean.  Within the fp32 bounds; whether it is also bit-equal is reported."""
    name = "trn_fp32"
    cfg, kw, params, xs, xt, ys, ns, nt, _, _ = wl.case_setup(name)
    runs = []
    for cw, dw in (([1.0] * cfg.num_class, (0.5, 0.5)), (None, None)):
        eng = _engine(name, cw, dw)
        eng.load_state(params)
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step(list(wl.BETA), wl.GAMMA, wl.LR, valid_source=ns, valid_target=nt)
        torch.cuda.synchronize()
        runs.append((eng.P.clone().cpu(), eng.G.clone().cpu(), eng.region("losses")[:6].clone().cpu()))
    (p1, g1, l1), (p0, g0, l0) = runs
    with capsys.disabled():
        print(f"\n[weighted unit weights] bit-equal to the unflagged step: parameters {torch.equal(p1, p0)}, gradients {torch.equal(g1, g0)}, "
              f"losses {torch.equal(l1, l0)}; max |d grad| {(g1 - g0).abs().max().item():.2e}")
    assert torch.allclose(p1, p0, rtol=tol.F32_RTOL, atol=tol.F32_ATOL)
    assert (g1 - g0).norm().item() <= tol.F32_GRAD_REL_L2_MEDIAN * g0.norm().item()
    assert torch.allclose(l1, l0, rtol=2e-4, atol=2e-4)


def test_main_py_trains_both_weighted_criteria_on_the_fused_step(tmp_path):
    """main.py --weighted_class_loss Y --weighted_class_loss_DA Y on a skewed source list, two epochs without dropout: the fused step logs the
    loss columns the module path (TA3N_MAIN_FAST=0: the two torch criteria) logs, to 2e-4; the engine says that the weights are on."""
    from fixture_t7 import make_dataset
    data = list(make_dataset(str(tmp_path / "data")))
    keep = {0: 5, 1: 4, 2: 2, 3: 1, 4: 1}      # videos per class of the source list: weights between 2.6 and 13
    lines, seen = [], {}
    for ln in open(data[1]):
        c = int(ln.split()[2])
        seen[c] = seen.get(c, 0) + 1
        if seen[c] <= keep[c]:
            lines.append(ln)
    skewed = str(tmp_path / "list_source_skewed.txt")
    open(skewed, "w").writelines(lines)
    outs = []
    for fast in ("0", "1"):
        exp = str(tmp_path / f"exp{fast}")
        cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", skewed, data[2], data[3], "--exp_path", exp + "/",
               "--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
               "--add_loss_DA", "attentive_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.003", "--lr_adaptive", "dann",
               "--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0", "--dropout_v", "0", "-b", "8", "6", "8",
               "--lr", "0.03", "--epochs", "2", "-j", "0", "--print_freq", "1", "--no_partialbn", "--weighted_class_loss", "Y",
               "--weighted_class_loss_DA", "Y", "--save_best_log", str(tmp_path / f"best{fast}.log")]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        said = [ln for ln in r.stdout.splitlines() if ln.startswith("[ta3n]") and "class weights" in ln and "domain weights" in ln]
        assert bool(said) == (fast == "1"), r.stdout[-2000:]
        if said:
            assert "fused step" in said[0]
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
    print("# train.log, module path then fused step\n" + "".join(outs[0]) + "# ----\n" + "".join(outs[1]))
    assert len(outs[0]) == len(outs[1]) == 4      # 2 epochs x ceil(13 / 8) steps
    num = re.compile(r"(Loss|loss_c|loss_a|loss_e) (-?[0-9.]+)")
    for a, b in zip(*outs):
        fa, fb = num.findall(a), num.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb] and len(fa) == 4
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-4 * max(1.0, abs(float(y))), (k, x, y, a, b)


@pytest.mark.parametrize("name", wl.FIXTURES)
def test_engine_follows_the_reference_trajectory_with_weighted_criteria(name):
    """The fixtures the reference's own main.train wrote with the two criteria weighted (tests/golden/make_golden_weighted.py), replayed
    through TrainEngine: the logged losses, clipped gradients and parameters after every step."""
    from golden_util import step_schedule
    from ta3n_amd.engine import TrainEngine, flags_from_options
    from ta3n_amd.synthetic import synth_batch
    g, c, cfg, cw, dw = wl.fixture_setup(name)
    avg = c["agg"] == "avgpool"
    flags = flags_from_options(place_adv=c["place_adv"], add_loss_DA="none", use_attn="none") if avg else None
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, dropout_i=0.0, dropout_v=0.0, clip=c["clip"],
                      aggregation=c["agg"], class_weights=cw, domain_weights=dw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    live = set(eng.live_names())
    assert live == set(str(k) for k in g.meta("live"))
    log = str(g.meta("log")).strip().splitlines()
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step([0.75, 0.75, 0.5], 0.0 if avg else 0.003, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        L = eng.losses()
        got = dict(Loss=L["loss"], loss_c=L["loss_c"], loss_a=L["loss_adv_rel"] + L["loss_adv_vid"] + L["loss_adv_frm"], loss_e=L["loss_e"])
        for k, w in wl.log_numbers(log[s]).items():
            assert abs(got[k] - w) <= 2e-4 * max(1.0, abs(w)), (name, s, k, got[k], w)
        coef = eng.region("grad_norm")[1].item()
        grads = eng.param_views(eng.G)
        for k, v in eng.param_views().items():
            if k in live:
                if s == 0 or avg:      # (later steps of the trn-m step stand on parameters that differ by round-off: relative L2, as tests/test_gpu_parity.py)
                    g.check(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef, 1e-3, 2e-5, rms_atol=1e-2)
                assert g.rel_l2(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) <= tol.F32_GRAD_REL_L2 * (1 if s == 0 else tol.GOLDEN_DRIFT_FACTOR), (name, s, k)
            g.check(f"step{s}/param/{k}", v.cpu(), tol.F32_RTOL, tol.F32_ATOL)
