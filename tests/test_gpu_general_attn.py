"""--use_attn general on the MI355X (models.py:320-325, 359-366, 379-388): the engine's unfused launch lists with the two general-attention
kernels against fixtures the reference produced (tests/golden/make_golden_general_attn.py) - forward tensors and the attention weights,
the trajectory of clipped gradients and parameters - the two kernels alone at the segment limits against float64 torch, the dropout
stream, the bf16 arithmetics, the module path (VideoModel + the torch loss assembly + autograd), checkpoints and Adam."""
import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

GA_CASES = ["tiny_ga_T5", "tiny_ga_T2", "tiny_ga_odd", "tiny_ga_relN", "tiny_ga_T9", "mid_ga"]
# the fp32 reference record of the very same case (weight seed, batches, options) with use_attn TransAttn: tiny_ga_T5 is make_golden's tiny_T5
# with the option on; mid_ga_plain is mid_ga run through the reference with TransAttn (make_golden_general_attn.PLAIN_CASES)
PLAIN_OF = {"tiny_ga_T5": "tiny_T5", "mid_ga": "mid_ga_plain"}
ATTN_PARAMS = ["attn_layer.0.weight", "attn_layer.0.bias", "attn_layer.2.weight", "attn_layer.2.bias"]
BETA, GAMMA = [0.75, 0.75, 0.5], 0.003


def _engine(name, **kw):
    g = Golden(name)
    c = case_config(g)
    use_attn = str(g.meta("use_attn")) if g.has_meta("use_attn") else "TransAttn"
    flags = flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), c["add_loss_DA"] or "attentive_entropy", use_attn, "RevGrad", "uSv")
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, dropout_i=0.0, dropout_v=0.0, clip=c["clip"], **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    return g, c, eng


def _set_batch(eng, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())


# ---- 1. forward against every fixture ----
@pytest.mark.parametrize("name", GA_CASES)
def test_forward_matches_reference(name):
    g, c, eng = _engine(name)
    assert eng.general_attn and not eng.fused and not eng.plan.has_fused_step and "general attention" in eng.describe()
    assert set(eng.live_names()) == set(str(k) for k in g.meta("live"))
    st = step_schedule(c)[0]
    _set_batch(eng, c, st)
    eng.set_hyper(BETA, GAMMA, st["lr"], train=True)
    eng.forward()
    torch.cuda.synchronize()
    o = {k: v.detach().cpu() for k, v in eng.outputs().items()}
    B, Bs, T = c["Bs"] + c["Bt"], c["Bs"], c["T"]
    assert o["attn"].shape == (B, T - 1)
    assert float((o["attn"].double().sum(1) - 1).abs().max()) <= tol.F32_ATOL
    for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
        g.check(f"fwd/out_{dom}", o["out"][sl], 0, tol.LOGIT_ATOL, "class logits")
        for nm, key in (("rel", "pred_rel"), ("vid", "pred_vid"), ("frm", "pred_frm")):
            g.check(f"fwd/pd_{dom}_{nm}", o[key][sl], 0, tol.LOGIT_ATOL, "domain logits")
        g.check(f"fwd/attn_{dom}", o["attn"][sl], tol.F32_RTOL, tol.F32_ATOL)
        g.check(f"fwd/feat_{dom}_f1", o["feat_f1"][sl], tol.F32_RTOL, tol.F32_ATOL)
        g.check(f"fwd/feat_{dom}_v", o["feat_v"][sl], tol.F32_RTOL, tol.F32_ATOL)


# ---- 2. trajectory against every fixture ----
@pytest.mark.parametrize("name", GA_CASES)
def test_trajectory_matches_reference(name):
    """Clipped gradients and parameters after every step (bounds of tests/test_gpu_frame_attn.py::test_trajectory_matches_reference,
    GOLDEN_DRIFT_FACTOR from the second step on); attn_layer.2.bias - mathematically zero, ~1e-8 from the reference's autograd - with the
    absolute term only.  The last step of tiny_ga_T5 runs with padded videos, whose rows of gUa, gRa and gs must be exactly zero; at
    tiny_ga_T2 (one relation) the four attention gradients are exactly zero and the parameters still move by weight decay."""
    g, c, eng = _engine(name)
    live = set(eng.live_names())
    B, NR = c["Bs"] + c["Bt"], c["T"] - 1
    for s, st in enumerate(step_schedule(c)):
        before = {k: eng.param_views()[k].clone() for k in ATTN_PARAMS}
        _set_batch(eng, c, st)
        eng.train_step(BETA, GAMMA, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        coef = eng.region("grad_norm")[1].item()
        grads = eng.param_views(eng.G)
        f = 1.0 if s == 0 else tol.GOLDEN_DRIFT_FACTOR
        for k, v in eng.param_views().items():
            if k in live:
                rtol, rms = (0.0, 0.0) if k == "attn_layer.2.bias" else (2e-4 * f, 2e-4 * f)
                g.check(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef, rtol, 5e-6 * f, rms_atol=rms)
            g.check(f"step{s}/param/{k}", v.cpu(), 2e-4 * f, 5e-6 * f)
        if st["n_src"] < c["Bs"]:
            pad = [st["n_src"], c["Bs"] + st["n_tgt"]]
            for region, width in (("gUa", 256), ("gRa", 256), ("gs", 1)):
                assert (eng.region(region, (B, NR, width))[pad] == 0).all(), region
            assert (eng.region("gUa", (B, NR, 256))[:st["n_src"]] != 0).any()
        if NR == 1:
            assert (eng.region("attn") == 1).all()
            for k in ATTN_PARAMS:
                assert (grads[k] == 0).all(), k
                if k.endswith("weight"):
                    assert not torch.equal(eng.param_views()[k], before[k]), k      # weight decay
    assert eng.step_count == c["steps"]


# ---- 3. the two kernels at the segment limits, without fixtures ----
@pytest.mark.parametrize("T,Bs,Bt", [(2, 2, 2), (3, 2, 2), (64, 2, 2), (3, 5, 4)], ids=["T2", "T3", "T64", "T3_9videos"])
def test_kernels_against_float64(T, Bs, Bt):
    """forward() / loss() / backward() of an engine at fc_dim 8, 3 classes: one relation, two, 63 (the last lane that holds a score), and
    nine videos (a partly filled last workgroup).  w, V, gs, gUa, gRa are recomputed in float64 torch - the backward quantities by autograd
    of the forward function - from what the kernels themselves read (R, A = tanh(U) as stored, the attention layer, gVt, g_attn - the latter
    filled with random numbers, as a caller of the module path would) and compared with F32_RTOL / F32_ATOL; A itself against
    tanh(R Wa1^T + ba1)."""
    D, F, C = 16, 8, 3
    B, NR, NB = Bs + Bt, T - 1, 256
    eng = TrainEngine(Bs, Bt, T, D, F, C, flags=flags_from_options(use_attn="general"), dropout_i=0.0, dropout_v=0.0)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=71 + T, scale="trained"))
    xs, xt, ys, yt = synth_batch(C, T, D, Bs, Bt, seed=700 + T)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.set_hyper(BETA, GAMMA, 1e-3, train=True)
    eng.forward(); eng.loss()
    ga = torch.randn(B, NR, generator=torch.Generator().manual_seed(T), dtype=torch.float32)
    eng.region("g_attn", (B, NR)).copy_(ga.cuda())
    eng.backward()
    torch.cuda.synchronize()
    P = {k: v.double().cpu() for k, v in eng.param_views().items() if k in ATTN_PARAMS}
    R = eng.region("R", (B, NR, NB)).double().cpu()
    A = eng.region("Ua", (B, NR, NB)).double().cpu().requires_grad_(True)
    Rl = R.clone().requires_grad_(True)
    gv = eng.region("gVt", (B, NB)).double().cpu()
    s = A @ P["attn_layer.2.weight"][0] + P["attn_layer.2.bias"]
    s.retain_grad()
    w = torch.softmax(s, 1)
    Vfull = ((1 + w).unsqueeze(-1) * Rl).sum(1)      # (R a leaf of its own: the weights' path to R runs through A, U and the relation-level launch)
    ((Vfull * gv).sum() + (w * ga.double()).sum()).backward()

    def close(name, got, want):
        got, want = got.double().cpu(), want.detach()
        err = (got - want).abs()
        assert bool((err <= tol.F32_ATOL + tol.F32_RTOL * want.abs()).all()), f"{name}: max err {float(err.max()):.3e} (ref absmax {float(want.abs().max()):.3e})"
    close("A", A, torch.tanh(R @ P["attn_layer.0.weight"].T + P["attn_layer.0.bias"]))
    close("attn", eng.region("attn", (B, NR)), w)
    close("V", eng.region("V", (B, NB)), Vfull)
    assert torch.equal(eng.region("Vd"), eng.region("V"))
    close("gs", eng.region("gs", (B, NR)), s.grad)
    close("gUa", eng.region("gUa", (B, NR, NB)), A.grad * (1 - A.detach() ** 2))
    close("gRa", eng.region("gRa", (B, NR, NB)), Rl.grad)
    assert torch.equal(eng.region("gPrT"), eng.region("gPr"))      # the relation discriminators: their loss gradient alone
    assert float((eng.region("attn", (B, NR)).double().sum(1) - 1).abs().max()) <= tol.F32_ATOL
    assert float(s.grad.abs().max()) > 0 or NR == 1
    if NR == 1:
        assert (eng.region("attn") == 1).all() and (eng.region("gs") == 0).all() and (eng.region("gUa") == 0).all()


# ---- 4. dropout ----
def test_dropout_stream_is_the_pooling_kernels():
    """dropout_v 0.5: every element of Vd is 0 or V / keep, and the zero pattern is the one a TransAttn engine of the same shape draws with
    the same seed (pool_fwd_kernel's hash on the same element index)."""
    def run(use_attn):
        eng = TrainEngine(6, 4, 5, 512, 64, 12, flags=flags_from_options(use_attn=use_attn), dropout_i=0.0, dropout_v=0.5, fused=False)
        eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7, scale="trained"))
        xs, xt, ys, yt = synth_batch(12, 5, 512, 6, 4, seed=1234)
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.set_hyper(BETA, GAMMA, 1e-3, train=True, seed=5)
        eng.forward()
        torch.cuda.synchronize()
        return eng.region("V").clone(), eng.region("Vd").clone()
    v, vd = run("general")
    pv, pvd = run("TransAttn")
    live = (v != 0) & (pv != 0)      # (a channel whose every tuple activation is zero tells nothing)
    assert float(live.float().mean()) > 0.9
    kept = vd != 0
    assert torch.equal(vd[kept], v[kept] * 2.0)
    assert 0.35 < float(kept[live].float().mean()) < 0.65
    assert torch.equal((pvd != 0)[live], kept[live])


# ---- 5. bf16 with and without twins ----
def _bf16_distance(name, twins):
    """One step of the bf16 unfused engine against the fp32 fixture `name`: (logit max error / rms, {tensor: (relative L2 of the
    clipped gradient, elements)}, engine)."""
    g, c, eng = _engine(name, fused=False, bf16=True, bf16_store=twins)
    assert not eng.fused
    st = step_schedule(c)[0]
    _set_batch(eng, c, st)
    eng.set_hyper(BETA, GAMMA, st["lr"], train=True)
    eng.forward(); eng.loss(); eng.backward()
    raw = {k: v.clone() for k, v in eng.param_views(eng.G).items()}
    eng.sgd_step()
    torch.cuda.synchronize()
    coef = eng.region("grad_norm")[1].item()
    y = eng.outputs()["out"].cpu()
    Bs = c["Bs"]
    logit = max(float(np.abs(y[sl].double().numpy() - g.z[f"fwd/out_{dom}#full"].astype(np.float64)).max()) / g.rms(f"fwd/out_{dom}")
                for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, None))))
    rel = {k: (g.rel_l2(f"step0/clipped_grad/{k}", raw[k].cpu() * coef), raw[k].numel()) for k in eng.live_names()}
    return logit, rel, eng


@pytest.mark.parametrize("twins", [False, True], ids=["bf16", "bf16_store"])
@pytest.mark.parametrize("name", list(PLAIN_OF))
def test_bf16_is_as_close_to_fp32_as_the_plain_lists(name, twins, capsys):
    """bf16 MFMA operands, with and without twins.  Reference: the fp32 fixture.  Metrics (BF16_REF_*): logit max error / rms, relative L2
    per clipped-gradient tensor (worst over the tensors of >= 4096 elements, median over all).  Bound: the TransAttn bf16 unfused engine is
    measured first, against the reference's record of the same case with use_attn TransAttn (PLAIN_OF); general attention - another
    implementation of the same bf16 contract, one more contraction in front of the pooling - may be BF16_REF_GRAD_CONTRACT_FACTOR x as far
    plus BF16_REF_GRAD_FLOOR, and never beyond the absolute caps.  The test prints the pairs (plain -> general attention) before it asserts;
    DESIGN.md 8 records them."""
    pg, pc = Golden(PLAIN_OF[name]), case_config(Golden(PLAIN_OF[name]))
    fc = case_config(Golden(name))
    same = ("C", "T", "D", "fc_dim", "Bs", "Bt", "wseed", "wscale", "xseed", "lr", "clip", "place_adv")
    assert not pg.has_meta("use_attn") and {k: pc[k] for k in same} == {k: fc[k] for k in same}, "the baseline must be the same case"
    p_logit, p_rel, _ = _bf16_distance(PLAIN_OF[name], twins)
    f_logit, f_rel, eng = _bf16_distance(name, twins)

    def worst(rel):
        return max(v for v, n in rel.values() if n >= 4096)

    def median(rel):
        return float(np.median([v for v, _ in rel.values()]))
    pairs = dict(worst=(worst(p_rel), worst(f_rel)), median=(median(p_rel), median(f_rel)), logits=(p_logit, f_logit))
    with capsys.disabled():
        print(f"\n[bf16 vs fp32 fixture] {name} twins={twins}: " + " | ".join(f"{k} plain {a:.3e} -> general attention {b:.3e}" for k, (a, b) in pairs.items()))
    for k, (plain, ga) in pairs.items():
        bound = tol.BF16_REF_GRAD_CONTRACT_FACTOR * plain + tol.BF16_REF_GRAD_FLOOR
        assert ga <= bound, f"{k}: general attention {ga:.3e} > {bound:.3e} (plain lists: {plain:.3e})"
    assert pairs["worst"][1] <= tol.BF16_REF_GRAD_REL_L2 and pairs["median"][1] <= tol.BF16_REF_GRAD_REL_L2_MEDIAN
    assert f_logit <= tol.BF16_REF_LOGIT_REL_RMS
    if twins:      # the launch of Hr, Pf and Ua keeps reading twins
        third = [ph for ph in eng.plan.description["phases"] if ph["group"] == 0 and ph["kind"] == 0][2]
        assert (third["tile"] // 1000) & 16, third


# ---- 6. module path, state_dict order, checkpoints ----
def _video_model(c):
    from ta3n_amd.models import VideoModel
    m = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   dropout_i=0.0, dropout_v=0.0, partial_bn=False, verbose=False, use_attn="general")
    sd = m.state_dict()
    sd.update(synth_state({k: tuple(v.shape) for k, v in sd.items()}, seed=c["wseed"], scale=c["wscale"]))
    m.load_state_dict(sd)
    return m, sd


def test_module_path_matches_reference_gradients():
    """VideoModel(use_attn='general') forward, the reference's loss assembly in torch ops (oracle.total_loss, main.py:439-562), backward()
    through ta3n_backward, clip_grad_norm_: every .grad against step 0 of tiny_ga_T5; eval mode = train mode (dropout 0); the
    state_dict's key order is the reference's."""
    from oracle import ta3n_oracle as orc
    g = Golden("tiny_ga_T5")
    c = case_config(g)
    m, sd = _video_model(c)
    assert list(sd.keys()) == [str(k) for k in g.meta("state_keys")]
    m = m.cuda()
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    m.eval()
    with torch.no_grad():
        ev = m(xs, xt, BETA, 0, False, False)
    m.train()
    out = m(xs, xt, BETA, 0, True, False)
    assert torch.equal(ev[1], out[1]) and torch.equal(ev[6], out[6]) and torch.equal(ev[0], out[0])
    g.check("fwd/out_s", out[1].detach().cpu(), 0, tol.LOGIT_ATOL)
    g.check("fwd/out_t", out[6].detach().cpu(), 0, tol.LOGIT_ATOL)
    g.check("fwd/attn_s", out[0].detach().cpu(), tol.F32_RTOL, tol.F32_ATOL)      # attn_relation_source / _target as the reference returns them
    g.check("fwd/attn_t", out[5].detach().cpu(), tol.F32_RTOL, tol.F32_ATOL)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"])
    loss, _ = orc.total_loss(dict(out=out[1], pred_domain=out[3]), dict(out=out[6], pred_domain=out[8]), ys.cuda(), GAMMA, cfg, c["Bs"], c["Bt"])
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), c["clip"])
    live = set(str(k) for k in g.meta("live"))
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k in live), k
        if k in live:
            g.check(f"step0/clipped_grad/{k}", p.grad.cpu(), 0 if k == "attn_layer.2.bias" else 2e-4, 5e-6, rms_atol=0 if k == "attn_layer.2.bias" else 2e-4)
    assert list(m.state_dict().keys()) == list(sd.keys())


def test_checkpoint_round_trip_is_bit_identical():
    """A checkpoint written by the engine (keys in the reference's order, attn_layer.* last) loads into VideoModel and back into an engine."""
    from ta3n_amd.checkpoint import engine_checkpoint, load_into_engine
    g, c, eng = _engine("tiny_ga_T5")
    st = step_schedule(c)[0]
    _set_batch(eng, c, st)
    eng.train_step(BETA, GAMMA, st["lr"])
    m, _ = _video_model(c)
    ck = engine_checkpoint(eng, m, 3, "resnet18", st["lr"], 0.0, 0.0)
    assert list(ck["state_dict"].keys()) == ["module." + str(k) for k in g.meta("state_keys")]
    m.load_state_dict({k[len("module."):]: v for k, v in ck["state_dict"].items()})
    mine = eng.state_dict()
    for k, v in mine.items():      # (the model's BatchNorm buffers are not the engine's)
        assert torch.equal(m.state_dict()[k].cpu(), v.cpu()), k
    _, _, back = _engine("tiny_ga_T5")
    ck2 = dict(ck, state_dict={"module." + k: v for k, v in m.state_dict().items()})
    assert load_into_engine(back, m, ck2)["start_epoch"] == 4
    torch.cuda.synchronize()
    assert torch.equal(back.P, eng.P)


# ---- 7. Adam ----
def test_adam_three_steps_and_train_steps_are_bit_identical():
    def run(batched):
        g, c, eng = _engine("tiny_ga_odd", optimizer="Adam")
        _set_batch(eng, c, step_schedule(c)[0])
        sched = [(BETA, GAMMA, 2e-3 * (1.0 - 0.1 * k)) for k in range(3)]
        if batched:
            eng.train_steps(sched)
        else:
            for b, gm, lr in sched:
                eng.train_step(b, gm, lr)
        eng.flush()
        torch.cuda.synchronize()
        return eng
    a, b = run(False), run(True)
    assert a.adam_step_count == b.adam_step_count == 3 and a.step_count == 3
    assert torch.equal(a.P, b.P) and torch.equal(a.M, b.M) and torch.equal(a.V, b.V)
    views = a.adam_views()
    for k in ATTN_PARAMS:
        assert float(views[k][1].abs().max()) > 0, k      # the attention layer takes part in the update
    fresh = _engine("tiny_ga_odd", optimizer="Adam")[2]
    assert not torch.equal(a.param_views()["attn_layer.0.weight"], fresh.param_views()["attn_layer.0.weight"])
