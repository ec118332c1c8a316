"""--use_target Sv and --add_loss_DA target_entropy on the MI355X (reference main.py:439-446, 542-545; TA3N_FLAG_TARGET_LABELS /
TA3N_FLAG_TARGET_ENTROPY): every kernel that forms the class cross-entropy or the entropy term - the fused heads kernel, the unfused loss
kernel (also under BatchNorm, the discrepancy loss, frame attention and on TemPooling), the device batch assembly that delivers the target
labels - against the reference assembly of tests/target_cases.py: every loss term, the two row blocks of gY each as a tensor of its own, gPv,
every gradient tensor of one step without clipping and the parameters after it, under the bounds of ta3n_amd/tolerances.py.  Each case first
asserts, on the reference alone, that the options it runs cannot be mistaken for their neighbours (target_cases.distinct)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import target_cases as tc
from oracle import ta3n_oracle as orc
from ta3n_amd import _lib
from ta3n_amd import loss as L
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_state

pytestmark = pytest.mark.gpu
wl = tc.wl


def _engine(name, **more):
    from ta3n_amd.engine import TrainEngine
    c = tc.CASES[name]
    cfg, kw, params, xs, xt, labels, ns, nt, cw = tc.case_setup(name)
    kw = dict(kw, **more)
    clip = kw.pop("clip", 0.0)      # 0: no clipping
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], tc.D, tc.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=clip, class_weights=cw, **kw)
    eng.load_state(params)
    return eng


def _set_batch(eng, xs, xt, labels):
    Bs = eng.Bs
    eng.set_batch(xs.cuda(), xt.cuda(), labels[:Bs].cuda(), target_label=labels[Bs:].cuda() if eng.target_labels else None)


def _assert_distinct(name):
    for k, v in tc.distinct(name).items():
        assert v >= 100 * tc.LOGIT_GRAD_REL_L2["f32"], (name, k, v)


def _grad_metrics(got, want):
    out = {}
    for k, w in want.items():
        w = w.detach().double().cpu()
        g = got[k].detach().double().cpu().reshape(w.shape)
        d = g - w
        out[k] = ((d.norm() / (w.norm() + 1e-300)).item(), d.abs().max().item() / (w.abs().max().item() + 1e-300))
    return out


def _compare_step(name, eng, ref, cfg, arith="f32"):
    """Everything one step leaves behind against the reference step `ref`."""
    o = eng.outputs()
    bf16 = arith == "bf16"
    for key, want in (("out", ref["out"]), ("pred_vid", ref["pred_vid"])):
        if key not in o or (key == "pred_vid" and cfg.place_adv[1] != "Y" and cfg.place_adv[0] != "Y"):
            continue
        got = o[key].cpu().reshape(want.shape)
        err = (got - want).abs().max().item()
        bound = tol.BF16_LOGIT_REL_RMS * want.pow(2).mean().sqrt().item() + 1e-7 if bf16 else tol.LOGIT_ATOL
        print(f"[target {name} {arith}] {key}: max err {err:.2e} (bound {bound:.1e})")
        assert err <= bound, (name, key, err)
    # every loss term
    Lg = eng.losses()
    P = ref["parts"]
    want_l = dict(loss=P["loss"] - eng.alpha * P.get("loss_d", 0.0), loss_c=P["loss_c"], loss_a=P.get("loss_a", 0.0), loss_e=P.get("loss_e", 0.0))
    got_l = dict(loss=Lg["loss"], loss_c=Lg["loss_c"], loss_a=Lg["loss_adv_rel"] + Lg["loss_adv_vid"] + Lg["loss_adv_frm"], loss_e=Lg["loss_e"])
    if cfg.frame_aggregation == "trn-m":
        for k in ("loss_adv_rel", "loss_adv_vid", "loss_adv_frm"):
            want_l[k], got_l[k] = P.get(k, 0.0), Lg[k]
    if "loss_d" in P:
        want_l["loss_d"], got_l["loss_d"] = P["loss_d"], float(eng.loss_d)
    rel = tol.BF16_LOSS_REL if bf16 else 2e-4
    for k, w in want_l.items():
        print(f"[target {name} {arith}] {k}: {got_l[k]:.6f} want {w:.6f} (|d| {abs(got_l[k] - w):.1e})")
        assert abs(got_l[k] - w) <= rel * max(1.0, abs(w)), (name, k, got_l[k], w)
    # the logit gradients: source-row and target-row block of gY each on its own, gPv
    got_lg = tc.engine_logit_grads(eng)
    bound = tc.LOGIT_GRAD_REL_L2[arith]
    for k in ("gY_s", "gY_t", "gPv"):
        want = ref["logit_grads"][k]
        if k not in got_lg:
            continue
        if float(want.abs().max()) == 0.0:      # a block the options leave empty (one class: p - 1 = 0; no video-level term): zero on the device too
            assert float(got_lg[k].abs().max()) <= (1e-30 if not bf16 else 1e-6), (name, k)
            print(f"[target {name} {arith}] logit gradient {k}: zero on both sides")
            continue
        d = wl.rel_l2(got_lg[k], want)
        print(f"[target {name} {arith}] logit gradient {k}: rel. L2 {d:.2e} (bound {bound:.1e})")
        assert d <= bound, (name, k, d)
    # every gradient tensor
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
    print(f"[target {name} {arith}] gradients: median rel. L2 {med:.2e} (bound {med_tol:.1e}), worst {worst} {m[worst][0]:.2e} max/scale {m[worst][1]:.2e}")
    assert set(m) == set(want_g) and set(eng.live_names()) >= set(m)
    for k, (l2, mx) in m.items():
        assert l2 <= l2_tol and mx <= mx_tol, (name, k, l2, mx)
    assert med <= med_tol, (name, med)


def _compare_params(name, eng, ref, start, arith="f32"):
    new = eng.param_views()
    for k, v in ref["params"].items():
        got = new[k].cpu()
        if arith == "bf16":
            d = (got.double() - v.double()).norm().item()
            assert d <= tol.BF16_GRAD_REL_L2 * max((v - start[k]).double().norm().item(), 1e-30) + 1e-9, (name, k, d)
        else:
            assert torch.allclose(got, v.float(), rtol=tol.F32_RTOL, atol=tol.F32_ATOL), (name, k, (got - v).abs().max().item())
    assert any(not torch.equal(new[k].cpu(), start[k]) for k in eng.live_names())


def _run_case(name, arith="f32", engine_more=None, oracle_more=None):
    _assert_distinct(name)
    cfg, kw, params, xs, xt, labels, ns, nt, cw = tc.case_setup(name)
    use_target, ent, gamma = tc.options(name)
    eng = _engine(name, **(engine_more or {}))
    assert eng.target_labels == (use_target == "Sv") and eng.target_entropy == (ent == "target_entropy")
    assert ("target labels" in eng.describe()) == eng.target_labels and ("target entropy" in eng.describe()) == eng.target_entropy
    _set_batch(eng, xs, xt, labels)
    eng.train_step(list(tc.BETA), gamma, tc.LR, valid_source=ns, valid_target=nt)
    torch.cuda.synchronize()
    if oracle_more:
        rcfg = orc.Config(**dict(cfg.__dict__, **oracle_more))
        ref = tc.reference_step(rcfg, params, xs, xt, labels, ns, nt, use_target, ent, cw, gamma=gamma, alpha=eng.alpha)
    else:
        ref = tc.shared_reference(name)
    _compare_step(name, eng, ref, cfg, arith=arith)
    _compare_params(name, eng, ref, params, arith=arith)
    return eng, ref


@pytest.mark.parametrize("name", ["base", "ragged", "s70", "t70", "vpw2", "C64", "C1", "sv_only", "tent_only", "tent_g003", "sv_cw", "tent_plain", "adabn", "addfc2"])
def test_fused_step(name):
    """Stage D of the fused heads kernel: Sv, target entropy, both; padding rows that carry a label; target labels at an offset that is no
    multiple of 64 and a weight sum of more than one trip per lane (70 + 3), more target than source rows (3 + 70); two videos per workgroup (150 + 77); 64 classes and 1; the sum
    of the class weights over both halves; the term without attention or any adversarial branch; the BatchNorm and stacked-layer steps."""
    eng, _ = _run_case(name)
    assert eng.fused
    if name == "vpw2":
        assert eng.B > 224      # (the plan builder's threshold for two videos per heads workgroup; an odd count: the last workgroup holds one)


@pytest.mark.parametrize("waves", [4, 8])
def test_heads_kernel_of_four_and_of_eight_waves(waves):
    Lb = _lib.lib()
    try:
        assert Lb.ta3n_set_heads_waves(waves) == 0
        eng, _ = _run_case("ragged")
        assert Lb.ta3n_get_heads_waves(eng.plan.handle) == waves
    finally:
        Lb.ta3n_set_heads_waves(0)


@pytest.mark.parametrize("name", ["unfused", "dan"])
def test_unfused_lists(name):
    """The `loss` kernel of the unfused launch lists, alone and with the discrepancy loss (dis_DA DAN) entering between forward and backward."""
    eng, ref = _run_case(name)
    assert not eng.fused
    if name == "dan":
        assert ref["parts"]["loss_d"] != 0.0


def test_frame_attention_lists():
    """--use_attn_frame TransAttn runs on the unfused lists.  The oracle holds no frame attention: the loss kernel's terms and logit gradients
    under both options against autograd on the engine's own logits, and a whole step that moves every live parameter."""
    from ta3n_amd.engine import TrainEngine, flags_from_options
    cfg, _, params, xs, xt, labels, ns, nt, _ = tc.case_setup("ragged")
    c = tc.CASES["ragged"]
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], tc.D, tc.FC, c["C"], dropout_i=0.0, dropout_v=0.0, clip=0.0,
                      flags=flags_from_options(add_loss_DA="target_entropy", use_target="Sv", use_attn_frame="TransAttn"))
    assert eng.frame_attn and not eng.fused and eng.target_labels and eng.target_entropy
    eng.load_state(params)
    _set_batch(eng, xs, xt, labels)
    eng.set_hyper(list(tc.BETA), tc.GAMMA_HU, tc.LR, valid_source=ns, valid_target=nt)
    eng.forward(); eng.loss()
    torch.cuda.synchronize()
    Bs = c["Bs"]
    y = eng.outputs()["out"].cpu().double().requires_grad_(True)
    loss_c = F.cross_entropy(torch.cat((y[:ns], y[Bs:Bs + nt])), torch.cat((labels[:ns], labels[Bs:Bs + nt])))
    loss_e = L.cross_entropy_soft(y[Bs:Bs + nt])
    gy, = torch.autograd.grad(loss_c + tc.GAMMA_HU * loss_e, y)
    got = eng.region("gY", (eng.B, eng.C))
    for k, sl in (("gY_s", slice(0, Bs)), ("gY_t", slice(Bs, None))):
        d = wl.rel_l2(got[sl], gy[sl])
        print(f"[target frame_attn f32] logit gradient {k}: rel. L2 {d:.2e} (bound {tc.LOGIT_GRAD_REL_L2['f32']:.1e})")
        assert d <= tc.LOGIT_GRAD_REL_L2["f32"], (k, d)
    Lg = eng.losses()
    for k, g, w in (("loss_c", Lg["loss_c"], float(loss_c.detach())), ("loss_e", Lg["loss_e"], float(loss_e.detach()))):
        print(f"[target frame_attn f32] {k}: {g:.6f} want {w:.6f}")
        assert abs(g - w) <= 2e-4 * max(1.0, abs(w)), (k, g, w)
    eng.train_step(list(tc.BETA), tc.GAMMA_HU, tc.LR, valid_source=ns, valid_target=nt)
    torch.cuda.synchronize()
    new = eng.param_views()
    assert all(torch.isfinite(v).all() for v in new.values()) and all(not torch.equal(new[k].cpu(), params[k]) for k in eng.live_names())


def test_avgpool_general_plan():
    """TemPooling with the RevGrad branches under Sv: the loss kernel with zero relation rows (the video-level CE counted twice)."""
    eng, _ = _run_case("avgpool_sv")
    kinds = [ph["kind"] for ph in eng.plan.description["phases"]]
    assert 7 not in kinds      # not PH_POOL_CLS: the source-only plan, which refuses the flag


@pytest.mark.parametrize("arith", ["bf16", "f32x3"])
def test_other_arithmetics(arith):
    """bf16 against the bf16-operand oracle policy and its bounds (tests/test_gpu_bf16.py), the split arithmetic against the fp32 reference."""
    if arith == "bf16":
        _run_case("base", arith="bf16", engine_more=dict(bf16=True, bf16_store=True), oracle_more=dict(arithmetic="bf16", bf16_twins=True))
    else:
        _run_case("base", arith="f32x3", engine_more=dict(f32_split=True))


def test_target_label_is_required_under_sv_and_refused_without_it():
    cfg, _, params, xs, xt, labels, ns, nt, _ = tc.case_setup("base")
    eng = _engine("sv_only")
    with pytest.raises(ValueError, match="use_target Sv .* needs target_label"):
        eng.set_batch(xs.cuda(), xt.cuda(), labels[:6].cuda())
    eng = _engine("tent_only")      # the flag off
    with pytest.raises(ValueError, match="target_label without use_target Sv"):
        eng.set_batch(xs.cuda(), xt.cuda(), labels[:6].cuda(), target_label=labels[6:].cuda())
    with pytest.raises(ValueError, match="--add_loss_DA target_entropy"):      # a step without a valid target row
        eng.train_step(list(tc.BETA), tc.GAMMA_HU, tc.LR, valid_source=6, valid_target=0)


def test_sv_with_a_fully_padded_target_half_is_the_usv_step_bit_for_bit():
    """valid_target = 0: the class CE runs over the source rows alone with inv_n_cls = 1 / n_s - the uSv step's loss and gradients, bit for bit."""
    from ta3n_amd.engine import ALL_FLAGS, TrainEngine
    cfg, _, params, xs, xt, labels, _, _, _ = tc.case_setup("sv_only")
    labels = labels.clone()
    labels[6:] = labels[0]
    runs = []
    for flags in (ALL_FLAGS | _lib.FLAG_TARGET_LABELS, ALL_FLAGS):
        eng = TrainEngine(6, 4, 5, tc.D, tc.FC, 12, flags=flags, dropout_i=0.0, dropout_v=0.0, clip=0.0)
        eng.load_state(params)
        _set_batch(eng, xs, xt, labels)
        eng.train_step(list(tc.BETA), tc.GAMMA_SMALL, tc.LR, valid_source=5, valid_target=0)
        torch.cuda.synchronize()
        assert eng._hyper.inv_n_cls == np.float32(1 / 5)
        runs.append((eng.G.clone().cpu(), eng.region("losses")[:6].clone().cpu(), eng.region("gY").clone().cpu(), eng.P.clone().cpu()))
    for a, b, what in zip(runs[0], runs[1], ("gradients", "losses", "gY", "parameters")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
    assert runs[0][1][1] > 0 and runs[0][0].abs().sum() > 0


def _stores(T, C, gen):
    from ta3n_amd.feature_store import FeatureStore

    def store(n_videos, labels):
        nf = torch.tensor([T + (3 * v) % 7 for v in range(n_videos)])
        rows = torch.randn(int(nf.sum()), tc.D, generator=gen).abs()
        return FeatureStore.from_tensors(rows.cuda().contiguous(), nf.cuda(), labels.cuda())
    return store(16, torch.tensor([(5 * v) % C for v in range(16)])), store(9, torch.tensor([(7 * v + 3) % C for v in range(9)]))


def _bits(t):
    return t.detach().clone().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("schedule", ["repeats", "short"])
def test_device_gathered_batches_under_sv(schedule):
    """train_steps(feeds=...) and gather_into deliver the target labels to ws["labels"][Bs:] under Sv: bit-identical to the same steps driven
    by set_batch with the labels copied by the host.  repeats: five steps whose id rows come back (0 1 0 2 1); short: three steps whose last
    call piece is one step and whose target feed assembles one video fewer than the half (the row it leaves stays as set)."""
    from ta3n_amd.engine import TrainEngine, flags_from_options
    Bs, Bt, T, C = 6, 4, 5, 12
    gen = torch.Generator().manual_seed(9)
    src, tgt = _stores(T, C, gen)
    rows_s = [torch.randperm(16, generator=gen)[:Bs] for _ in range(3)]
    n_t = Bt if schedule == "repeats" else Bt - 1
    rows_t = [torch.randperm(9, generator=gen)[:n_t] for _ in range(3)]
    order = [0, 1, 0, 2, 1] if schedule == "repeats" else [0, 1, 2]
    ids_s = torch.stack([rows_s[i] for i in order]).to(torch.int32).cuda()
    ids_t = torch.stack([rows_t[i] for i in order]).to(torch.int32).cuda()
    n = len(order)
    sched = [(list(tc.BETA), tc.GAMMA_HU, tc.LR * (1.0 + 0.05 * k)) for k in range(n)]
    cfg = orc.Config(num_class=C, num_segments=T, feature_dim=tc.D, fc_dim=tc.FC, dropout_i=0.0, dropout_v=0.0)
    params = synth_state(orc.param_shapes(cfg), seed=11)
    flags = flags_from_options(add_loss_DA="target_entropy", use_target="Sv")
    states = {}
    for how in ("host", "gather_into", "feeds"):
        eng = TrainEngine(Bs, Bt, T, tc.D, tc.FC, C, flags=flags, dropout_i=0.0, dropout_v=0.0, clip=20.0)
        eng.load_state(params)
        eng.X.zero_(); eng._labels.zero_()
        if how == "feeds":
            assert eng.can_batch_steps()
            eng.train_steps(sched, feeds=((src, ids_s), (tgt, ids_t)))
        else:
            for k, (beta, gamma, lr) in enumerate(sched):
                if how == "host":
                    xs, ys = src.gather(ids_s[k], T)
                    xt, yt = tgt.gather(ids_t[k], T)
                    xt_full, yt_full = torch.zeros(Bt, T, tc.D, device="cuda"), torch.zeros(Bt, dtype=torch.int32, device="cuda")
                    xt_full[:n_t], yt_full[:n_t] = xt, yt
                    eng.set_batch(xs, xt_full, ys, target_label=yt_full)
                else:
                    src.gather_into(eng, ids_s[k], 0, labels_out=eng._labels[:Bs])
                    tgt.gather_into(eng, ids_t[k], Bs, labels_out=eng._labels[Bs:])
                eng.train_step_pipelined(beta, gamma, lr)
        eng.flush()
        torch.cuda.synchronize()
        want_t = torch.zeros(Bt, dtype=torch.int32)
        want_t[:n_t] = tgt.labels[ids_t[-1].long()].cpu().to(torch.int32)
        assert torch.equal(eng._labels[Bs:].cpu(), want_t), how
        assert torch.equal(eng._labels[:Bs].cpu(), src.labels[ids_s[-1].long()].cpu().to(torch.int32)), how
        states[how] = dict(P=_bits(eng.P), M=_bits(eng.M), G=_bits(eng.G), losses=_bits(eng.region("losses")[:6]), X=_bits(eng.X))
        assert eng.losses()["loss_c"] > 0 and eng.losses()["loss_e"] > 0
    for how in ("gather_into", "feeds"):
        for k, v in states["host"].items():
            assert torch.equal(v, states[how][k]), f"{how}: {k} differs at {(v != states[how][k]).sum().item()} of {v.numel()} elements"
    # ... and the labels matter: the same steps with the target labels all of one class end elsewhere
    assert len(set(tgt.labels[ids_t[-1].long()].cpu().tolist())) > 1


def test_target_half_of_the_labels_keeps_its_sentinel_without_the_flag():
    from ta3n_amd.engine import TrainEngine
    Bs, Bt, T, C = 6, 4, 5, 12
    gen = torch.Generator().manual_seed(9)
    src, tgt = _stores(T, C, gen)
    ids_s = torch.stack([torch.randperm(16, generator=gen)[:Bs] for _ in range(3)]).to(torch.int32).cuda()
    ids_t = torch.stack([torch.randperm(9, generator=gen)[:Bt] for _ in range(3)]).to(torch.int32).cuda()
    eng = TrainEngine(Bs, Bt, T, tc.D, tc.FC, C, dropout_i=0.0, dropout_v=0.0, clip=20.0)
    cfg = orc.Config(num_class=C, num_segments=T, feature_dim=tc.D, fc_dim=tc.FC, dropout_i=0.0, dropout_v=0.0)
    eng.load_state(synth_state(orc.param_shapes(cfg), seed=11))
    eng._labels.fill_(-7)
    assert eng.can_batch_steps() and not eng.target_labels
    eng.train_steps([(list(tc.BETA), tc.GAMMA_SMALL, tc.LR)] * 3, feeds=((src, ids_s), (tgt, ids_t)))
    eng.flush()
    torch.cuda.synchronize()
    assert (eng._labels[Bs:] == -7).all()
    assert torch.equal(eng._labels[:Bs].cpu(), src.labels[ids_s[-1].long()].cpu().to(torch.int32))


@pytest.mark.parametrize("name", tc.FIXTURES)
def test_engine_follows_the_reference_trajectory(name):
    """The fixtures the reference's own main.train wrote under --use_target Sv (tests/golden/make_golden_target.py; tiny_sv_tent with
    --add_loss_DA target_entropy at gamma 0.3), replayed through TrainEngine: the logged losses, clipped gradients and parameters after
    every step, the last of which is short."""
    from golden_util import step_schedule
    from ta3n_amd.engine import TrainEngine, flags_from_options
    g, c, cfg, use_target, ent, gamma = tc.fixture_setup(name)
    avg = c["agg"] == "avgpool"
    flags = (flags_from_options(place_adv=c["place_adv"], add_loss_DA="none", use_attn="none", use_target=use_target) if avg else
             flags_from_options(add_loss_DA=ent, use_target=use_target))
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, dropout_i=0.0, dropout_v=0.0, clip=c["clip"],
                      aggregation=c["agg"])
    assert eng.target_labels and eng.target_entropy == (ent == "target_entropy")
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    live = set(eng.live_names())
    assert live == set(str(k) for k in g.meta("live"))
    log = str(g.meta("log")).strip().splitlines()
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = tc.fixture_batch(c, st)
        _set_batch(eng, xs, xt, labels)
        eng.train_step([0.75, 0.75, 0.5], gamma, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        Lg = eng.losses()
        got = dict(Loss=Lg["loss"], loss_c=Lg["loss_c"], loss_a=Lg["loss_adv_rel"] + Lg["loss_adv_vid"] + Lg["loss_adv_frm"], loss_e=Lg["loss_e"])
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
