"""--share_params N on the MI355X (models.py:174-192, 296-305, 565-566, 686-687): the engine's unfused launch lists with five GEMMs cut at
the domain boundary against fixtures the reference produced (tests/golden/make_golden_unshared.py) - forward tensors, the trajectory of
clipped gradients and parameters - against the plain unfused lists on equal weights, the dropout masks at the global row, the bf16
arithmetics, Adam, validation through the target layers, and main.py with the option (fast path, module path, checkpoint, --resume)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import N_SAMP, Golden, case_config, sample_index, step_schedule
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP_CASES = ["tiny_sp_T5", "tiny_sp_T2", "tiny_sp_odd", "tiny_sp_one", "tiny_sp_noent", "tiny_sp_sv", "mid_sp"]
# the fp32 reference record of the very same case (weight seed, batches, options) with share_params Y: tiny_sp_T5 is make_golden's tiny_T5
# with the option on; mid_sp_plain is mid_sp run through the reference with share_params Y (make_golden_unshared.PLAIN_CASES)
PLAIN_OF = {"tiny_sp_T5": "tiny_T5", "mid_sp": "mid_sp_plain"}
TWIN_OF = {"fc_feature_shared_target": "fc_feature_shared_source", "fc_classifier_video_target": "fc_classifier_video_source",
           "fc_feature_target": "fc_feature_source", "fc_classifier_target": "fc_classifier_source",
           "fc_feature_video_target": "fc_feature_video_source", "fc_feature_video_target_2": "fc_feature_video_source_2"}
BETA, GAMMA = [0.75, 0.75, 0.5], 0.003


def _engine(name, share_params=None, **kw):
    g = Golden(name)
    c = case_config(g)
    use_target = str(g.meta("use_target")) if g.has_meta("use_target") else "uSv"
    flags = flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), c["add_loss_DA"] or "attentive_entropy", "TransAttn", "RevGrad", use_target)
    sp = share_params or (str(g.meta("share_params")) if g.has_meta("share_params") else "Y")
    kw.setdefault("dropout_i", 0.0); kw.setdefault("dropout_v", 0.0)
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, clip=c["clip"], share_params=sp, **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    return g, c, eng


def _set_batch(eng, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda(), **(dict(target_label=yt.cuda()) if eng.target_labels else {}))


def _stored(g, key, t):
    """(entries of tensor t that record `key` stores, the stored reference entries) as float64 arrays"""
    a = t.detach().double().cpu().numpy().reshape(-1)
    if key + "#full" in g.z:
        return a, g.z[key + "#full"].astype(np.float64).reshape(-1)
    ref = np.concatenate([g.z[key + "#head"], g.z[key + "#samp"]]).astype(np.float64)
    return np.concatenate([a[:N_SAMP], a[sample_index(a.size)]]), ref


def _grad_distance(g, key, t):
    """(relative L2, max |error| / max |reference|) over the stored entries; (None, max |ours|) where the reference tensor is all zero"""
    a, ref = _stored(g, key, t)
    if not np.any(ref):
        return None, float(np.abs(a).max())
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref)), float(np.abs(a - ref).max() / np.abs(ref).max())


# ---- 1. fp32 trajectories against every fixture ----
@pytest.mark.parametrize("name", SP_CASES)
def test_fp32_trajectory_matches_reference(name, capsys):
    """TrainEngine(share_params="N") against the reference's run: class and domain logits within LOGIT_ATOL, features / attention /
    parameters within F32_RTOL / F32_ATOL, every clipped-gradient tensor within F32_GRAD_REL_L2 / F32_GRAD_MAX_SCALE and their median
    within F32_GRAD_REL_L2_MEDIAN; GOLDEN_DRIFT_FACTOR from the second step on.  The measured distances are printed
    (profiles/unshared_parity_floors.txt records them)."""
    g, c, eng = _engine(name)
    assert eng.unshared and not eng.fused and not eng.plan.has_fused_step and "unshared target layers (share_params N)" in eng.describe()
    assert eng._flags & _lib.FLAG_UNSHARED
    live = set(eng.live_names())
    assert live == set(str(k) for k in g.meta("live"))
    B, Bs, T = c["Bs"] + c["Bt"], c["Bs"], c["T"]
    lines = []
    for s, st in enumerate(step_schedule(c)):
        _set_batch(eng, c, st)
        eng.train_step(BETA, GAMMA, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        f = 1.0 if s == 0 else tol.GOLDEN_DRIFT_FACTOR
        if s == 0:
            o = {k: v.detach().cpu() for k, v in eng.outputs().items()}
            worst_logit = 0.0
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                worst_logit = max(worst_logit, g.check(f"fwd/out_{dom}", o["out"][sl], 0, tol.LOGIT_ATOL, "class logits"))
                for nm, key in (("rel", "pred_rel"), ("vid", "pred_vid"), ("frm", "pred_frm")):
                    worst_logit = max(worst_logit, g.check(f"fwd/pd_{dom}_{nm}", o[key][sl], 0, tol.LOGIT_ATOL, "domain logits"))
                g.check(f"fwd/attn_{dom}", o["attn"][sl], tol.F32_RTOL, tol.F32_ATOL)
                g.check(f"fwd/feat_{dom}_f1", o["feat_f1"][sl], tol.F32_RTOL, tol.F32_ATOL)
                g.check(f"fwd/feat_{dom}_v", o["feat_v"][sl], tol.F32_RTOL, tol.F32_ATOL)
            lines.append(f"[unshared fp32] {name}: worst logit error {worst_logit:.2e} (bound {tol.LOGIT_ATOL:.0e})")
        coef = eng.region("grad_norm")[1].item()
        grads = eng.param_views(eng.G)
        dist = {}
        for k, v in eng.param_views().items():
            if k in live:
                l2, mx = _grad_distance(g, f"step{s}/clipped_grad/{k}", grads[k] * coef)
                if l2 is None:
                    assert mx <= tol.F32_ATOL, (name, s, k, mx)
                else:
                    dist[k] = (l2, mx)
        worst = max(dist, key=lambda k: dist[k][0])
        med = float(np.median([v[0] for v in dist.values()]))
        lines.append(f"[unshared fp32] {name} step {s}: gradients median rel. L2 {med:.2e} (bound {tol.F32_GRAD_REL_L2_MEDIAN * f:.1e}), worst {worst} "
                     f"{dist[worst][0]:.2e} (bound {tol.F32_GRAD_REL_L2 * f:.1e}), max/scale {max(v[1] for v in dist.values()):.2e} "
                     f"(bound {tol.F32_GRAD_MAX_SCALE * f:.1e}); " +
                     ", ".join(f"{k} {dist[k][0]:.2e}" for k in dist if "_target" in k))
        with capsys.disabled():
            print("\n" + "\n".join(lines[-2:] if s == 0 else lines[-1:]))
        for k, (l2, mx) in dist.items():
            assert l2 <= tol.F32_GRAD_REL_L2 * f and mx <= tol.F32_GRAD_MAX_SCALE * f, (name, s, k, l2, mx)
        assert med <= tol.F32_GRAD_REL_L2_MEDIAN * f, (name, s, med)
        for k, v in eng.param_views().items():
            g.check(f"step{s}/param/{k}", v.cpu(), tol.F32_RTOL * f, tol.F32_ATOL * f)
    assert eng.step_count == c["steps"]


# ---- 2. equal weights: the flagged lists beside the plain unfused lists ----
@pytest.mark.parametrize("name", ["tiny_sp_odd", "mid_sp"])
def test_equal_weights_give_the_plain_lists_numbers(name, capsys):
    """The target layers loaded with their source twins, one step at dropout 0 beside a plain TrainEngine(fused=False) on the same batch:
    forward tensors within F32_RTOL / F32_ATOL; dWsh_s + dWsh_t against dWsh, the two classifier gradients' sum against dWcv and every
    unsplit gradient tensor within F32_MASKED_GRAD_REL_L2 (the project's bound for summation order alone)."""
    g, c, eng = _engine(name)
    _, _, plain = _engine(name, share_params="Y", fused=False)
    assert eng.unshared and not plain.unshared and not plain.fused
    state = _equal_state(c, eng.plan)
    eng.load_state(state); plain.load_state(state)
    st = step_schedule(c)[0]
    for e in (eng, plain):
        _set_batch(e, c, st)
        e.set_hyper(BETA, GAMMA, st["lr"], train=True)
        e.forward(); e.loss(); e.backward()
    torch.cuda.synchronize()
    a, b = eng.outputs(), plain.outputs()
    for k in b:
        assert torch.allclose(a[k], b[k], rtol=tol.F32_RTOL, atol=tol.F32_ATOL), (k, float((a[k] - b[k]).abs().max()))
    ga, gb = eng.param_views(eng.G), plain.param_views(plain.G)
    summed = {"fc_feature_shared_source": "fc_feature_shared_target", "fc_classifier_video_source": "fc_classifier_video_target"}
    worst = {}
    for k in plain.live_names():
        layer, leaf = k.rsplit(".", 1)
        mine = ga[k].double() + (ga[f"{summed[layer]}.{leaf}"].double() if layer in summed else 0.0)
        want = gb[k].double()
        worst[k] = float((mine - want).norm() / want.norm())
    with capsys.disabled():
        top = sorted(worst, key=worst.get)[-3:]
        print(f"\n[unshared equal weights] {name}: " + ", ".join(f"{k} {worst[k]:.2e}" for k in [f"{s}.weight" for s in summed] + top) +
              f" (bound {tol.F32_MASKED_GRAD_REL_L2:.0e})")
    for k, v in worst.items():
        assert v <= tol.F32_MASKED_GRAD_REL_L2, (name, k, v)
    for tgt in summed.values():      # each half carries a share of its own
        assert float(ga[tgt + ".weight"].abs().max()) > 0


# ---- 3. dropout masks at the global row ----
def test_dropout_masks_are_keyed_by_the_global_row():
    """mid_sp, dropout_i = dropout_v = 0.5: F1 equals the dropout-free F1 times the host mirror's mask (tests/dropout_masks.py) at the GLOBAL
    row index, Vd the Vd of a forward with the same frame mask and no video dropout times the video mask - exactly, for source and target
    rows; a mask that restarts at row 0 for the target half is a different mask."""
    import dropout_masks as dm
    g, c, eng = _engine("mid_sp")
    Bs, Bt, T, F, NV = c["Bs"], c["Bt"], c["T"], c["fc_dim"], 256
    _set_batch(eng, c, step_schedule(c)[0])

    def forward(p_i, p_v):
        eng.dropout_i, eng.dropout_v = p_i, p_v
        eng.set_hyper(BETA, GAMMA, 1e-3, train=True, seed=5)
        eng.forward()
        torch.cuda.synchronize()
        return (eng.region("F1", ((Bs + Bt) * T, F)).double().cpu(), eng.region("V", (Bs + Bt, NV)).double().cpu(),
                eng.region("Vd", (Bs + Bt, NV)).double().cpu())
    f1_on, v_on, vd_on = forward(0.5, 0.5)
    seeds = (int(eng._hyper.seed_i), int(eng._hyper.seed_v))
    f1_off, _, _ = forward(0.0, 0.0)
    f1_i, v_i, vd_i = forward(0.5, 0.0)
    m = dm.dropout_masks(seeds[0], seeds[1], 0.5, 0.5, Bs, Bt, T, F, NV)
    drop_i, drop_v = torch.cat(m["drop_i"]), torch.cat(m["drop_v"])
    assert torch.equal(f1_on, f1_off * drop_i)
    assert torch.equal(f1_i, f1_on) and torch.equal(vd_i, v_i) and torch.equal(v_i, v_on)
    assert torch.equal(vd_on, vd_i * drop_v)
    for t in (f1_on[Bs * T:], vd_on[Bs:], f1_on[:Bs * T], vd_on[:Bs]):
        assert 0.05 < float((t != 0).double().mean()) < 0.6
    wrong = dm.dropout_masks(seeds[0], seeds[1], 0.5, 0.5, Bs, Bt, T, F, NV, target_row0=0)      # the bug this test is for
    assert not torch.equal(f1_on, f1_off * torch.cat(wrong["drop_i"])) and not torch.equal(vd_on, vd_i * torch.cat(wrong["drop_v"]))


# ---- 4. bf16 with and without twins ----
def _equal_state(c, plan):
    """the case's weights with the target layers overwritten by their source twins: the share_params Y model of the same case"""
    # (synth_state draws the tensors one after the other in the order of their names: the share_params Y model's names alone)
    state = synth_state({n: s for n, _, s, _ in plan.params if n.rsplit(".", 1)[0] not in TWIN_OF}, seed=c["wseed"], scale=c["wscale"])
    for tgt, src in TWIN_OF.items():
        for leaf in (".weight", ".bias"):
            state[tgt + leaf] = state[src + leaf].clone()
    return state


def _bf16_distance(name, twins, against=None):
    """One step of the bf16 unfused engine of fixture `name` against its fp32 record: (logit max error / rms, {tensor: (relative L2 of the
    clipped gradient, elements)}, engine).  against: the share_params Y fixture of the same case - the engine then runs on equal weights
    (_equal_state), which makes it that fixture's model, and the gradients of a layer's two halves are added before they are compared."""
    g, c, eng = _engine(name, fused=False, bf16=True, bf16_store=twins)
    assert not eng.fused
    if against is not None:
        g = Golden(against)
        eng.load_state(_equal_state(c, eng.plan))
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
    names = [k for k in eng.live_names() if against is None or k.rsplit(".", 1)[0] not in TWIN_OF]
    halves = {v: k for k, v in TWIN_OF.items()} if against is not None else {}

    def grad(k):
        layer, leaf = k.rsplit(".", 1)
        return raw[k] + (raw[f"{halves[layer]}.{leaf}"] if layer in halves and f"{halves[layer]}.{leaf}" in raw and eng.unshared else 0.0)
    if against is not None:      # clip_grad_norm_ of the share_params Y model: the norm over the ADDED halves (two halves' norms are not their sum's)
        total = float(torch.sqrt(sum((grad(k).double() ** 2).sum() for k in names)))
        coef = min(c["clip"] / (total + 1e-6), 1.0) if c["clip"] > 0 else 1.0
    rel = {k: (g.rel_l2(f"step0/clipped_grad/{k}", grad(k).cpu() * coef), raw[k].numel()) for k in names}
    return logit, rel, eng


def _worst(rel):
    return max(v for v, n in rel.values() if n >= 4096)


def _median(rel):
    return float(np.median([v for v, _ in rel.values()]))


def _same_case(name):
    pg, pc = Golden(PLAIN_OF[name]), case_config(Golden(PLAIN_OF[name]))
    fc = case_config(Golden(name))
    same = ("C", "T", "D", "fc_dim", "Bs", "Bt", "wseed", "wscale", "xseed", "lr", "clip", "place_adv")
    assert (not pg.has_meta("share_params") or str(pg.meta("share_params")) == "Y") and {k: pc[k] for k in same} == {k: fc[k] for k in same}, \
        "the baseline must be the same case"


@pytest.mark.parametrize("twins", [False, True], ids=["bf16", "bf16_store"])
@pytest.mark.parametrize("name", list(PLAIN_OF))
def test_bf16_is_as_close_to_fp32_as_the_plain_lists(name, twins, capsys):
    """bf16 MFMA operands, rounded in registers and read from twins.  Reference: the fp32 fixture.  Metrics (BF16_REF_*), as in
    tests/test_gpu_general_attn.py: logit max error / rms, relative L2 per clipped-gradient tensor (worst over the tensors of >= 4096
    elements, median over all).  Bound: the plain bf16 unfused engine is measured first, against the reference's record of the same case
    with share_params Y (PLAIN_OF); the flagged lists - the same contractions cut in two - may be BF16_REF_GRAD_CONTRACT_FACTOR x as far
    plus BF16_REF_GRAD_FLOOR, and no tensor goes beyond the absolute caps.  The pairs (plain -> unshared), every tensor's included, are
    printed before anything is asserted.
    The single tensors' pairs are printed, not bounded, here: the two records hold different target weights, so the target rows carry
    other numbers, and at these sizes one tensor's relative bf16 error moves by an order of magnitude with the data in EITHER direction -
    measured on tiny_sp_T5, rounding in registers: relation_domain_classifier_all.0.0.bias 3.2e-3 -> 2.4e-2 and fc_feature_domain_video.weight
    6.6e-2 -> 3.8e-3, both computed by launches the flag does not touch.  The tensor-by-tensor bound is asserted where it means something,
    on the same numbers: test_bf16_per_tensor_on_equal_weights."""
    _same_case(name)
    p_logit, p_rel, _ = _bf16_distance(PLAIN_OF[name], twins)
    f_logit, f_rel, eng = _bf16_distance(name, twins)
    pairs = dict(worst=(_worst(p_rel), _worst(f_rel)), median=(_median(p_rel), _median(f_rel)), logits=(p_logit, f_logit))
    per = {}
    for k, (v, _) in f_rel.items():
        layer, leaf = k.rsplit(".", 1)
        per[k] = (p_rel[f"{TWIN_OF.get(layer, layer)}.{leaf}"][0], v)
    with capsys.disabled():
        print(f"\n[bf16 vs fp32 fixture] {name} twins={twins}: " + " | ".join(f"{k} plain {a:.3e} -> unshared {b:.3e}" for k, (a, b) in pairs.items()))
        print("    per tensor: " + ", ".join(f"{k} {a:.2e} -> {b:.2e}" for k, (a, b) in per.items()))
    for k, (plain, mine) in pairs.items():
        bound = tol.BF16_REF_GRAD_CONTRACT_FACTOR * plain + tol.BF16_REF_GRAD_FLOOR
        assert mine <= bound, f"{k}: unshared {mine:.3e} > {bound:.3e} (plain lists: {plain:.3e})"
    assert max(v for v, _ in f_rel.values()) <= tol.BF16_REF_GRAD_REL_L2 and pairs["median"][1] <= tol.BF16_REF_GRAD_REL_L2_MEDIAN
    assert f_logit <= tol.BF16_REF_LOGIT_REL_RMS
    if twins:      # the launches keep reading twins where the plain lists' do
        ours = [bool((ph["tile"] // 1000) & 16) for ph in eng.plan.description["phases"] if ph["group"] in (0, 2) and ph["kind"] == 0]
        assert any(ours) and ours[0]


@pytest.mark.parametrize("twins", [False, True], ids=["bf16", "bf16_store"])
@pytest.mark.parametrize("name", list(PLAIN_OF))
def test_bf16_per_tensor_on_equal_weights(name, twins, capsys):
    """The tensor-by-tensor form of the bound above, on the same numbers: with the target layers loaded with their source twins the flagged
    engine IS the share_params Y model of the case, so the plain fixture is the fp32 record of both engines.  Per clipped-gradient tensor
    (the two halves of a cut layer added), and for the logits: the flagged bf16 engine's distance from that record is at most
    BF16_REF_GRAD_CONTRACT_FACTOR x the plain bf16 unfused engine's plus BF16_REF_GRAD_FLOOR.  Pairs printed before asserting."""
    _same_case(name)
    p_logit, p_rel, _ = _bf16_distance(PLAIN_OF[name], twins)
    f_logit, f_rel, eng = _bf16_distance(name, twins, against=PLAIN_OF[name])
    assert eng.unshared and set(f_rel) == set(p_rel)
    pairs = dict({k: (p_rel[k][0], f_rel[k][0]) for k in p_rel}, logits=(p_logit, f_logit))
    with capsys.disabled():
        far = sorted(pairs, key=lambda k: pairs[k][1] / max(pairs[k][0], 1e-30))[-4:]
        print(f"\n[bf16 equal weights] {name} twins={twins}: " + ", ".join(f"{k} {pairs[k][0]:.2e} -> {pairs[k][1]:.2e}" for k in
                                                                          ["fc_feature_shared_source.weight", "fc_classifier_video_source.weight", "logits"] + far))
    for k, (plain, mine) in pairs.items():
        bound = tol.BF16_REF_GRAD_CONTRACT_FACTOR * plain + tol.BF16_REF_GRAD_FLOOR
        assert mine <= bound, f"{k}: unshared {mine:.3e} > {bound:.3e} (plain lists: {plain:.3e})"


# ---- 5. Adam ----
def test_adam_two_steps_update_the_live_tensors_like_torch():
    """tiny_sp_T5, two steps of optimizer="Adam": moments exist for the live tensors only (the four never-live target layers have none),
    one step count; the first step's clipped gradients are the fixture's; the parameters are within test_gpu_adam.py's bound of
    clip_grad_norm_ + torch.optim.Adam stepped on the step's gradients (ratio of the distances from float64 torch: ours / torch fp32's)."""
    from test_gpu_adam import BOUND, _cpu_adam
    g, c, eng = _engine("tiny_sp_T5", optimizer="Adam")
    live = eng.live_names()
    assert set(live) == set(str(k) for k in g.meta("live"))
    assert set(eng.adam_views()) == set(live) and eng.M.numel() == eng.V.numel() == eng.plan.live_floats
    assert not any(k.rsplit(".", 1)[0] in ("fc_feature_target", "fc_classifier_target", "fc_feature_video_target", "fc_feature_video_target_2")
                   for k in eng.adam_views())
    n = eng.plan.live_floats
    p0 = eng.P[:n].detach().cpu().clone()
    dead0 = eng.P[n:].detach().cpu().clone()
    grads, lrs = [], []
    for s, st in enumerate(step_schedule(c)[:2]):
        _set_batch(eng, c, st)
        eng.train_step(BETA, GAMMA, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
        torch.cuda.synchronize()
        grads.append(eng.G[:n].detach().cpu().clone()); lrs.append(st["lr"])
        if s == 0:
            coef = eng.region("grad_norm")[1].item()
            for k, v in eng.param_views(eng.G).items():
                if k in live:
                    l2, mx = _grad_distance(g, f"step0/clipped_grad/{k}", v * coef)
                    assert l2 is None or l2 <= tol.F32_GRAD_REL_L2, (k, l2)
    assert eng.adam_step_count == 2
    r32 = _cpu_adam(p0, grads, lrs, eng.weight_decay, c["clip"], torch.float32, eng.betas, eng.eps)
    r64 = _cpu_adam(p0, grads, lrs, eng.weight_decay, c["clip"], torch.float64, eng.betas, eng.eps)
    for what, gpu, a32, a64 in zip(("P", "exp_avg", "exp_avg_sq"), (eng.P[:n], eng.M, eng.V), r32, r64):
        ours = (gpu.detach().cpu().double() - a64).abs().max().item()
        torchs = (a32.double() - a64).abs().max().item()
        print(f"[unshared adam] {what}: max|gpu - f64| = {ours:.3e}, max|torch fp32 - f64| = {torchs:.3e}, ratio {ours / torchs:.2f}")
        assert ours <= BOUND * torchs, (what, ours, torchs)
    assert torch.equal(eng.P[n:].cpu(), dead0)      # nothing behind the live prefix moved (no weight decay there either)
    for k in ("fc_feature_shared_target.weight", "fc_classifier_video_target.weight"):
        assert float(eng.adam_views()[k][1].abs().max()) > 0, k


# ---- 6. validation through the target layers ----
def test_evaluate_batch_scores_the_target_branch():
    """main.validate calls model(val_data, val_data) and scores the target branch (main.py:707): evaluate_batch places the videos in the
    target half.  Logits against eval/out_t within LOGIT_ATOL - and far from eval/out_s, the source branch's, so the test tells the two
    apart; the metrics are those of the fixture's logits."""
    g, c, eng = _engine("tiny_sp_T5")
    Bs, Bt = c["Bs"], c["Bt"]
    xs, _, ys, _ = synth_batch(c["C"], c["T"], c["D"], Bs, Bt, seed=c["xseed"])
    want_t = torch.from_numpy(g.z["eval/out_t#full"]).double()
    want_s = torch.from_numpy(g.z["eval/out_s#full"]).double()
    assert float((want_t - want_s).abs().max()) > 10 * tol.LOGIT_ATOL
    with pytest.raises(ValueError, match="share_params N"):
        eng.evaluate_batch(xs[:Bt + 1].cuda(), ys[:Bt + 1].cuda(), reset=True)
    got = []
    for lo in range(0, Bs, Bt):
        n = min(Bt, Bs - lo)
        eng.evaluate_batch(xs[lo:lo + n].cuda(), ys[lo:lo + n].cuda(), reset=lo == 0)
        torch.cuda.synchronize()
        got.append(eng.outputs()["out"][Bs:Bs + n].double().cpu())
    got = torch.cat(got)
    assert float((got - want_t).abs().max()) <= tol.LOGIT_ATOL
    assert float((got - want_s).abs().max()) > 10 * tol.LOGIT_ATOL
    res = eng.eval_results()
    lp = torch.log_softmax(want_t, 1)
    assert res["n"] == Bs
    assert abs(res["loss"] - float(-lp[torch.arange(Bs), ys].mean())) <= 1e-3
    assert abs(res["prec1"] - 100.0 * float((want_t.argmax(1) == ys).double().mean())) <= 1e-3
    assert int(res["confusion"].sum()) == Bs


# ---- 7. module path ----
def test_module_path_matches_reference_gradients_and_leaves_grad_none_where_it_does():
    """VideoModel(share_params='N') forward, the reference's loss assembly in torch ops (oracle.total_loss, main.py:439-562), backward()
    through ta3n_backward, clip_grad_norm_: every .grad against step 0 of tiny_sp_T5, None exactly where the reference leaves it (the four
    never-live target layers among them).  With the cross-entropy of the source logits as the only loss no target layer receives a gradient."""
    from oracle import ta3n_oracle as orc
    from ta3n_amd.models import VideoModel
    g = Golden("tiny_sp_T5")
    c = case_config(g)
    m = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc_dim"],
                   dropout_i=0.0, dropout_v=0.0, partial_bn=False, verbose=False, share_params="N")
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g.meta("state_keys")]
    sd.update(synth_state({k: tuple(v.shape) for k, v in sd.items()}, seed=c["wseed"], scale=c["wscale"]))
    m.load_state_dict(sd)
    m = m.cuda()
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    m.train()
    out = m(xs, xt, BETA, 0, True, False)
    g.check("fwd/out_s", out[1].detach().cpu(), 0, tol.LOGIT_ATOL)
    g.check("fwd/out_t", out[6].detach().cpu(), 0, tol.LOGIT_ATOL)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"])
    loss, _ = orc.total_loss(dict(out=out[1], pred_domain=out[3]), dict(out=out[6], pred_domain=out[8]), ys.cuda(), GAMMA, cfg, c["Bs"], c["Bt"])
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), c["clip"])
    live = set(str(k) for k in g.meta("live"))
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k in live), k
        if k in live:
            l2, mx = _grad_distance(g, f"step0/clipped_grad/{k}", p.grad)
            assert l2 is None or (l2 <= tol.F32_GRAD_REL_L2 and mx <= tol.F32_GRAD_MAX_SCALE), (k, l2, mx)
    m.zero_grad(set_to_none=True)
    out = m(xs, xt, BETA, 0, True, False)
    torch.nn.functional.cross_entropy(out[1], ys.cuda()).backward()
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert not any("_target" in k for k in got) and "fc_feature_shared_source.weight" in got and "fc_classifier_video_source.weight" in got
    assert not any(k.startswith(("fc_feature_domain", "fc_classifier_domain")) for k in got)      # (the relation discriminators weigh the relations: TransAttn)


# ---- 8. main.py ----
OPTS = ["--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
        "--add_loss_DA", "attentive_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.003", "--lr_adaptive", "dann", "--share_params", "N"]
COMMON = ["--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "--dropout_i", "0.5", "--dropout_v", "0.5", "-b", "8", "6", "8",
          "--lr", "0.03", "-j", "0", "--print_freq", "1", "--save_model", "--no_partialbn"]
NEW_KEYS = [f"module.{layer}.{leaf}" for layer in TWIN_OF for leaf in ("weight", "bias")]


def _main(data, exp, tmp_path, fast, epochs, more=()):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *OPTS, *COMMON,
           "--epochs", str(epochs), "--save_best_log", str(tmp_path / f"best{fast}.log"), *more]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_own_main_fast_path_logs_what_the_module_path_logs(tmp_path):
    """main.py --share_params N on the tests/fixture_t7.py dataset: the engine (TA3N_MAIN_FAST=1) and the module path (=0) write the same
    Train: lines to 2e-4, their checkpoints agree within F32_RTOL / F32_ATOL and hold the twelve new keys in the reference's order, and
    --resume continues from the checkpoint."""
    from fixture_t7 import make_dataset
    from ta3n_amd.models import VideoModel
    data = make_dataset(str(tmp_path / "data"))
    outs, cks = [], []
    for fast in ("1", "0"):
        exp = str(tmp_path / f"exp{fast}")
        r = _main(data, exp, tmp_path, fast, 2)
        said = [ln for ln in r.stdout.splitlines() if ln.startswith("[ta3n]") and "unshared target layers (share_params N)" in ln]
        assert bool(said) == (fast == "1"), r.stdout[-2000:]
        if said:
            assert "unfused launch lists" in said[0]
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
        cks.append(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False))
    print("# train.log of main.py --share_params N on the engine (TA3N_MAIN_FAST=1), then on the module path (=0)\n" +
          "".join(outs[0]) + "# ----\n" + "".join(outs[1]))
    assert len(outs[0]) == len(outs[1]) == 6      # 2 epochs x ceil(24 / 8) steps, print_freq 1
    num = re.compile(r"(Prec@1|Prec@5|Loss|loss_c|loss_a|loss_e|lr:) (-?[0-9.]+)")
    for a, b in zip(*outs):
        fa, fb = num.findall(a), num.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb] and {"Prec@1", "Loss", "loss_c", "loss_a", "loss_e"} <= {k for k, _ in fa}
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-4 * max(1.0, abs(float(y))), (k, x, y, a, b)
    net = VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, verbose=False, share_params="N")
    fresh = {"module." + k: v.clone() for k, v in net.state_dict().items()}
    for ck in cks:
        assert list(ck["state_dict"].keys()) == list(fresh)
        assert set(NEW_KEYS) <= set(ck["state_dict"]) and len(NEW_KEYS) == 12
        torch.nn.DataParallel(net).load_state_dict(ck["state_dict"])
        opt = torch.optim.SGD(net.parameters(), 0.1, momentum=0.9, nesterov=True)
        opt.load_state_dict(ck["optimizer"])
    for k, v in cks[1]["state_dict"].items():
        if v.dtype.is_floating_point:
            assert torch.allclose(cks[0]["state_dict"][k], v, rtol=tol.F32_RTOL, atol=tol.F32_ATOL), (k, float((cks[0]["state_dict"][k] - v).abs().max()))
    for k in ("module.fc_feature_shared_target.weight", "module.fc_classifier_video_target.weight"):      # trained, not carried along
        assert not torch.equal(cks[0]["state_dict"][k], fresh[k]), k
    # --resume: a third epoch from the engine's checkpoint
    exp = str(tmp_path / "resumed")
    r = _main(data, exp, tmp_path, "1", 3, more=["--resume", str(tmp_path / "exp1" / "RGB" / "checkpoint.pth.tar")])
    assert "=> loaded checkpoint" in r.stdout
    lines = [ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")]
    assert len(lines) == 3 and all(ln.startswith("Train: [3]") for ln in lines), lines
    ck = torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 3 and list(ck["state_dict"].keys()) == list(fresh)
    assert not torch.equal(ck["state_dict"]["module.fc_feature_shared_target.weight"], cks[0]["state_dict"]["module.fc_feature_shared_target.weight"])
