"""--use_attn_frame TransAttn on the MI355X (models.py:368-377, 612-614): the engine's unfused launch lists with the two frame-attention
kernels against fixtures the reference produced (tests/golden/make_golden_frame_attn.py) - forward tensors and the frame weights,
the trajectory of clipped gradients and parameters - the bf16 arithmetics against the same fixtures, the twin of F1a, and the module
path (VideoModel + the torch loss assembly + autograd)."""
import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

FAF_CASES = ["tiny_faf_T5", "tiny_faf_T2", "tiny_faf_odd", "tiny_faf_advN", "mid_faf", "tiny_faf_wide"]
# the fp32 reference record of the very same case (weights, batches, options) with use_attn_frame none: tiny_faf_T5 is make_golden's tiny_T5 with
# the option on; mid_faf_plain is mid_faf run through the reference without it (make_golden_frame_attn.PLAIN_CASES)
PLAIN_OF = {"tiny_faf_T5": "tiny_T5", "mid_faf": "mid_faf_plain"}
BETA, GAMMA = [0.75, 0.75, 0.5], 0.003


def _engine(name, **kw):
    g = Golden(name)
    c = case_config(g)
    faf = g.has_meta("use_attn_frame")
    flags = flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), "attentive_entropy", "TransAttn", "RevGrad", "uSv",
                               use_attn_frame="TransAttn" if faf else "none")
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, dropout_i=0.0, dropout_v=0.0, clip=c["clip"], **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    return g, c, eng


def _set_batch(eng, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())


@pytest.mark.parametrize("name", FAF_CASES)
def test_forward_matches_reference(name):
    g, c, eng = _engine(name)
    assert eng.frame_attn and not eng.fused and not eng.plan.has_fused_step
    assert set(eng.live_names()) == set(str(k) for k in g.meta("live"))
    st = step_schedule(c)[0]
    _set_batch(eng, c, st)
    eng.set_hyper(BETA, GAMMA, st["lr"], train=True)
    eng.forward()
    torch.cuda.synchronize()
    o = {k: v.detach().cpu() for k, v in eng.outputs().items()}
    B, Bs, T = c["Bs"] + c["Bt"], c["Bs"], c["T"]
    assert o["attn_frame"].shape == (B, T)
    for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
        g.check(f"fwd/out_{dom}", o["out"][sl], 0, tol.LOGIT_ATOL, "class logits")
        for nm, key in (("rel", "pred_rel"), ("vid", "pred_vid"), ("frm", "pred_frm")):
            g.check(f"fwd/pd_{dom}_{nm}", o[key][sl], 0, tol.LOGIT_ATOL, "domain logits")
        g.check(f"fwd/attn_frame_{dom}", o["attn_frame"][sl], tol.F32_RTOL, tol.F32_ATOL)
        g.check(f"fwd/attn_{dom}", o["attn"][sl], tol.F32_RTOL, tol.F32_ATOL)
        g.check(f"fwd/feat_{dom}_f1", o["feat_f1"][sl], tol.F32_RTOL, tol.F32_ATOL)      # feat[2]: un-attended
        g.check(f"fwd/feat_{dom}_v", o["feat_v"][sl], tol.F32_RTOL, tol.F32_ATOL)
    # what the TRN read: (1 + w) F1, row by row
    f1a = eng.region("F1a", (B, T, eng.F)).cpu()
    assert torch.equal(f1a, (o["attn_frame"] + 1.0).unsqueeze(-1) * o["feat_f1"])


@pytest.mark.parametrize("name", FAF_CASES)
def test_trajectory_matches_reference(name):
    """Clipped gradients and parameters after every step (bounds of tests/test_gpu_engine_avgpool_da.py, GOLDEN_DRIFT_FACTOR from the
    second step on: its inputs are the previous step's fp32 results); the last step of tiny_faf_T5 runs with padded videos, whose
    rows must add nothing to any gradient."""
    g, c, eng = _engine(name)
    live = set(eng.live_names())
    for s, st in enumerate(step_schedule(c)):
        _set_batch(eng, c, st)
        eng.train_step(BETA, GAMMA, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        coef = eng.region("grad_norm")[1].item()
        grads = eng.param_views(eng.G)
        f = 1.0 if s == 0 else tol.GOLDEN_DRIFT_FACTOR
        for k, v in eng.param_views().items():
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef, 2e-4 * f, 5e-6 * f, rms_atol=2e-4 * f)
            g.check(f"step{s}/param/{k}", v.cpu(), 2e-4 * f, 5e-6 * f)
        if st["n_src"] < c["Bs"]:
            B, T = c["Bs"] + c["Bt"], c["T"]
            pad = [st["n_src"], c["Bs"] + st["n_tgt"]]
            for region, width in (("gF1a", eng.F), ("gPfT", 2), ("gZ1", eng.F)):
                assert (eng.region(region, (B, T, width))[pad] == 0).all(), region
    assert eng.step_count == c["steps"]


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
    logit = max(float(np.abs(y[sl].double().numpy() - _full(g, f"fwd/out_{dom}")).max()) / g.rms(f"fwd/out_{dom}")
                for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, None))))
    rel = {k: (g.rel_l2(f"step0/clipped_grad/{k}", raw[k].cpu() * coef), raw[k].numel()) for k in eng.live_names()}
    return logit, rel, eng


def _full(g, key):
    return g.z[key + "#full"].astype(np.float64)


@pytest.mark.parametrize("twins", [False, True], ids=["bf16", "bf16_store"])
@pytest.mark.parametrize("name", list(PLAIN_OF))
def test_bf16_is_as_close_to_fp32_as_the_plain_lists(name, twins, capsys):
    """bf16 MFMA operands, with and without twins.  Reference: the fp32 fixture.  Metrics (BF16_REF_*): logit max error / rms, relative L2
    per clipped-gradient tensor (worst over the tensors of >= 4096 elements, median over all).  Bound: the flag-off bf16 unfused engine
    is measured first, on the same weights and batches against the reference's record of that case without the option (PLAIN_OF);
    frame attention - another implementation of the same bf16 contract, one more rounded operand in front of the TRN - may be
    BF16_REF_GRAD_CONTRACT_FACTOR x as far plus BF16_REF_GRAD_FLOOR, and never beyond the absolute caps.  The test prints the pairs
    (plain -> frame attention) before it asserts; DESIGN.md 8 records them."""
    pg, pc = Golden(PLAIN_OF[name]), case_config(Golden(PLAIN_OF[name]))
    fc = case_config(Golden(name))
    same = ("C", "T", "D", "fc_dim", "Bs", "Bt", "wseed", "wscale", "xseed", "lr", "clip", "place_adv")
    assert not pg.has_meta("use_attn_frame") and {k: pc[k] for k in same} == {k: fc[k] for k in same}, "the baseline must be the same case"
    p_logit, p_rel, _ = _bf16_distance(PLAIN_OF[name], twins)
    f_logit, f_rel, eng = _bf16_distance(name, twins)

    def worst(rel):
        return max(v for v, n in rel.values() if n >= 4096)

    def median(rel):
        return float(np.median([v for v, _ in rel.values()]))
    pairs = dict(worst=(worst(p_rel), worst(f_rel)), median=(median(p_rel), median(f_rel)), logits=(p_logit, f_logit))
    with capsys.disabled():
        print(f"\n[bf16 vs fp32 fixture] {name} twins={twins}: " + " | ".join(f"{k} plain {a:.3e} -> frame attention {b:.3e}" for k, (a, b) in pairs.items()))
    for k, (plain, faf) in pairs.items():
        bound = tol.BF16_REF_GRAD_CONTRACT_FACTOR * plain + tol.BF16_REF_GRAD_FLOOR
        assert faf <= bound, f"{k}: frame attention {faf:.3e} > {bound:.3e} (plain lists: {plain:.3e})"
    assert pairs["worst"][1] <= tol.BF16_REF_GRAD_REL_L2 and pairs["median"][1] <= tol.BF16_REF_GRAD_REL_L2_MEDIAN
    assert f_logit <= tol.BF16_REF_LOGIT_REL_RMS
    if twins:      # the twin of F1a is round_bf16(F1a), bit for bit, and the tuple launch reads it
        o16, _ = eng.plan.region("ws16")
        oF, n = eng.plan.region("F1a")
        twin = eng.ws[o16:].view(torch.int16)[oF:oF + n]
        assert torch.equal(twin, eng.region("F1a").to(torch.bfloat16).view(torch.int16))
        tuples = [ph for ph in eng.plan.description["phases"] if ph["group"] == 0 and ph["kind"] == 0][3]
        assert (tuples["tile"] // 1000) & 16, tuples


def test_module_path_matches_reference_gradients():
    """VideoModel(use_attn_frame='TransAttn') forward, the reference's loss assembly in torch ops (oracle.total_loss, main.py:439-562),
    backward() through ta3n_backward, clip_grad_norm_: every .grad against step 0 of tiny_faf_T5; eval mode = train mode (dropout 0)."""
    from oracle import ta3n_oracle as orc
    from ta3n_amd.models import VideoModel
    g = Golden("tiny_faf_T5")
    c = case_config(g)
    m = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   dropout_i=0.0, dropout_v=0.0, partial_bn=False, verbose=False, use_attn="TransAttn", use_attn_frame="TransAttn")
    sd = m.state_dict()
    sd.update(synth_state({k: tuple(v.shape) for k, v in sd.items()}, seed=c["wseed"], scale=c["wscale"]))
    m.load_state_dict(sd)
    m = m.cuda()
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    m.eval()
    with torch.no_grad():
        ev = m(xs, xt, BETA, 0, False, False)
    m.train()
    out = m(xs, xt, BETA, 0, True, False)
    assert torch.equal(ev[1], out[1]) and torch.equal(ev[6], out[6]) and torch.equal(ev[9][1], out[9][1])
    g.check("fwd/out_s", out[1].detach().cpu(), 0, tol.LOGIT_ATOL)
    g.check("fwd/out_t", out[6].detach().cpu(), 0, tol.LOGIT_ATOL)
    g.check("fwd/feat_s_f1", out[4][2].detach().cpu(), tol.F32_RTOL, tol.F32_ATOL)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"])
    loss, _ = orc.total_loss(dict(out=out[1], pred_domain=out[3]), dict(out=out[6], pred_domain=out[8]), ys.cuda(), GAMMA, cfg, c["Bs"], c["Bt"])
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), c["clip"])
    live = set(str(k) for k in g.meta("live"))
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k in live), k
        if k in live:
            g.check(f"step0/clipped_grad/{k}", p.grad.cpu(), 2e-4, 5e-6, rms_atol=2e-4)
    assert list(m.state_dict().keys()) == list(sd.keys())
