"""Cases and the reference of --use_target Sv (reference main.py:439-446) and --add_loss_DA target_entropy (main.py:542-545, loss.py:8-12),
shared by tests/test_target_cpu.py and tests/test_gpu_target.py.

Logits and domain predictions come from oracle.ta3n_oracle.forward_domain; the loss is assembled here as oracle.total_loss assembles it, with
the two new terms written as the reference writes them - F.cross_entropy on the concatenation of the source and target logits, and
loss.cross_entropy_soft on the target logits - and differentiated by autograd.  The update behind it is oracle.train_step's (Nesterov SGD).

gamma: the target-entropy cases run with the reference's H->U value 0.3 (script_train_val.sh:90); at 0.003 the term is ~0.3 % of the logit
gradient, below the per-tensor bound, so a kernel that ignored it could pass.  One case (tent_g003) keeps 0.003 beside it.

distinct(): on the reference alone, the block of gY the new option acts on differs from the block under the option it could be mistaken
for by at least 100 x the bound the GPU test applies to that block (LOGIT_GRAD_REL_L2)."""
import numpy as np
import torch
import torch.nn.functional as F

import weighted_loss_cases as wl
from oracle import ta3n_oracle as orc
from ta3n_amd import loss as L
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_batch, synth_state

BETA, LR = (0.75, 0.75, 0.5), 2e-3
GAMMA_HU, GAMMA_SMALL = 0.3, 0.003
ALPHA = 0.5
# The bound on the two row blocks of gY (rel. L2 per block).  gY is a smooth function of the logits (softmax, log): no ReLU unit can land
# on another side between the logits and it, which is the situation tolerances.F32_MASKED_GRAD_REL_L2 is the per-tensor bound of; the f32x3
# and bf16 cases take their arithmetic's per-tensor bound.
LOGIT_GRAD_REL_L2 = {"f32": tol.F32_MASKED_GRAD_REL_L2, "f32x3": tol.F32X3_GRAD_REL_L2, "bf16": tol.BF16_GRAD_REL_L2}
D, FC = 512, 64

_TA3N = dict()                                                                   # oracle Config defaults: place_adv Y Y Y, TransAttn, attentive entropy
_NO_ENT = dict(add_loss_DA="none")
# name -> shape and options.  sv: --use_target Sv; ent: --add_loss_DA value; cw: class weights; valid: (valid_source, valid_target);
# kw: TrainEngine keywords; cfg: oracle Config fields (its add_loss_DA is set from `ent`)
CASES = {
    "base": dict(Bs=6, Bt=4, T=5, C=12, sv=True, ent="target_entropy"),
    "ragged": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="target_entropy"),
    "s70": dict(Bs=70, Bt=3, T=3, C=12, valid=(67, 3), sv=True, ent="target_entropy", cw=True),
    "t70": dict(Bs=3, Bt=70, T=3, C=12, valid=(3, 67), sv=True, ent="target_entropy", cw=True),
    "vpw2": dict(Bs=150, Bt=77, T=3, C=12, valid=(149, 75), sv=True, ent="target_entropy"),      # more than 224 videos: two per heads workgroup
    "C64": dict(Bs=6, Bt=4, T=2, C=64, sv=True, ent="target_entropy"),
    "C1": dict(Bs=6, Bt=4, T=2, C=1, sv=True, ent="target_entropy"),
    "sv_only": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="attentive_entropy"),
    "tent_only": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=False, ent="target_entropy"),
    "tent_g003": dict(Bs=6, Bt=4, T=5, C=12, sv=False, ent="target_entropy", gamma=GAMMA_SMALL),
    "sv_cw": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="attentive_entropy", cw=True),
    "tent_plain": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=False, ent="target_entropy", cfg=dict(place_adv=("N", "N", "N"), use_attn="none")),
    "unfused": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="target_entropy", kw=dict(fused=False)),
    "adabn": dict(Bs=6, Bt=4, T=5, C=12, sv=True, ent="target_entropy", cfg=dict(use_bn="AdaBN")),
    "addfc2": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="target_entropy", cfg=dict(add_fc=2)),
    "dan": dict(Bs=6, Bt=4, T=5, C=12, sv=True, ent="target_entropy", cfg=dict(dis_DA="DAN"), kw=dict(dis_DA="DAN", alpha=ALPHA)),
    "avgpool_sv": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), sv=True, ent="none", cfg=dict(frame_aggregation="avgpool", use_attn="none")),
}
# (--use_attn_frame TransAttn runs on the unfused lists too; the oracle holds no frame attention: tests/test_gpu_target.py compares that
# case's loss kernel against autograd on the engine's own logits)


def options(name):
    """(use_target, add_loss_DA, gamma) of a case."""
    c = CASES[name]
    return ("Sv" if c["sv"] else "uSv"), c["ent"], c.get("gamma", GAMMA_HU)


def case_setup(name, wseed=11, xseed=21):
    """(oracle Config, TrainEngine keywords, parameters, xs, xt, labels [Bs + Bt] (source rows, then target rows), n_src, n_tgt, class
    weights or None)."""
    c = CASES[name]
    use_target, ent, _ = options(name)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=D, fc_dim=FC, dropout_i=0.0, dropout_v=0.0,
                     **dict(dict(add_loss_DA=ent if ent == "attentive_entropy" else "none"), **c.get("cfg", {})))
    params = synth_state(wl.param_shapes(cfg), seed=wseed)
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], D, c["Bs"], c["Bt"], seed=xseed)
    ns, nt = c.get("valid", (c["Bs"], c["Bt"]))
    cw = wl.class_weights(c["C"]) if c.get("cw") else None
    if cw is not None:
        # the source labels follow the skew (mostly common classes), the target labels run against it (mostly rare, heavy classes): the sum
        # of the weights over both halves is then far from the sum over the source half
        rng = np.random.default_rng(xseed + 1)
        p = np.array(wl.skewed_counts(c["C"]), dtype=np.float64)
        ys = torch.tensor(rng.choice(c["C"], size=c["Bs"], p=p / p.sum()), dtype=torch.long)
        q = 1.0 / p
        yt = torch.tensor(rng.choice(c["C"], size=c["Bt"], p=q / q.sum()), dtype=torch.long)
    heavy = int(np.argmax(cw)) if cw is not None else c["C"] - 1
    ys, yt = ys.clone(), yt.clone()
    ys[ns:] = heavy          # padding rows: a label that would move the loss and the sum of the weights if a kernel let it in
    yt[nt:] = heavy          # (the padding rows keep their features too)
    return cfg, engine_kw(name, cfg), params, xs, xt, torch.cat((ys, yt)), ns, nt, cw


def engine_flags(cfg, use_target, ent):
    from ta3n_amd.engine import flags_from_options
    adv_on = any(p == "Y" for p in cfg.place_adv)
    return flags_from_options(cfg.place_adv, ent, cfg.use_attn, "RevGrad" if adv_on else "none", use_target)


def engine_kw(name, cfg):
    c = CASES[name]
    use_target, ent, _ = options(name)
    kw = dict(flags=engine_flags(cfg, use_target, ent), aggregation=cfg.frame_aggregation, use_bn=cfg.use_bn, add_fc=cfg.add_fc)
    kw.update(c.get("kw", {}))
    return kw


def class_ce(out, label, class_w, source_rows=None):
    """criterion(out, label) (main.py:446).  source_rows: the MISTAKEN weighted mean that divides by the sum of the weights of the first
    `source_rows` rows only (what a kernel that kept the one-range sum would compute) - for distinct()."""
    cw = None if class_w is None else torch.tensor(class_w, dtype=out.dtype)
    if source_rows is None or cw is None:
        return F.cross_entropy(out, label, weight=cw)
    w = cw[label]
    return (w * F.cross_entropy(out, label, reduction="none")).sum() / w[:source_rows].sum()


def target_total_loss(src, tgt, labels, gamma, cfg, n_src, n_tgt, use_target, ent, class_w=None, alpha=0.0, source_sum_only=False):
    """oracle.total_loss with the classification loss of main.py:439-446 and the target entropy of :542-545."""
    Bs = src["out"].size(0)
    out_s, out_t = src["out"][:n_src], tgt["out"][:n_tgt]
    out, label = out_s, labels[:n_src]
    if use_target == "Sv":                                                   # :442-444
        out = torch.cat((out, out_t))
        label = torch.cat((label, labels[Bs:Bs + n_tgt]))
    loss_c = class_ce(out, label, class_w, n_src if source_sum_only else None)
    loss = loss_c
    parts = {"loss_c": loss_c}
    if cfg.dis_DA != "none":                                                 # :452-505
        parts["loss_d"] = orc.discrepancy_loss(src, tgt, cfg, n_src, n_tgt)
        loss = loss + alpha * parts["loss_d"]
    pred_all, loss_a = [], 0
    for l, key in enumerate(("loss_adv_rel", "loss_adv_vid", "loss_adv_frm")):   # :508-538
        if cfg.place_adv[l] == "Y":
            ps = src["pred_domain"][l][:n_src].reshape(-1, 2)
            pt = tgt["pred_domain"][l][:n_tgt].reshape(-1, 2)
            lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long()
            pd = torch.cat((ps, pt), 0)
            pred_all.append(pd)
            parts[key] = F.cross_entropy(pd, lab)
            loss_a = loss_a + parts[key]
    if pred_all:
        loss = loss + loss_a
        parts["loss_a"] = loss_a
    if ent == "target_entropy":                                              # :542-545
        parts["loss_e"] = L.cross_entropy_soft(out_t)
        loss = loss + gamma * parts["loss_e"]
    if ent == "attentive_entropy" and cfg.use_attn != "none":                # :559-562
        parts["loss_e"] = orc.attentive_entropy(torch.cat((out_s, out_t), 0), pred_all[1])
        loss = loss + gamma * parts["loss_e"]
    parts["loss"] = loss
    return loss, parts


def reference_step(cfg, params, xs, xt, labels, n_src, n_tgt, use_target, ent, class_w=None, beta=BETA, gamma=GAMMA_HU, lr=LR, alpha=0.0,
                   momentum=None, clip=None, dtype=torch.float32, mom_coef=0.9, weight_decay=1e-4, source_sum_only=False):
    """One step of the reference arithmetic.  Returns dict(parts, out [B, C], pred_vid [B, 2], grads {name: tensor}, logit_grads {"gY_s",
    "gY_t": the class logits' by half, "gPv": the video-level domain logits' [B, 2]}, params and momentum after the step)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    xs, xt = xs.to(dtype), xt.to(dtype)
    fwd = wl._forward(cfg, beta)
    src, tgt = fwd(p, xs, "S"), fwd(p, xt, "T")
    loss, parts = target_total_loss(src, tgt, labels, gamma, cfg, n_src, n_tgt, use_target, ent, class_w, alpha, source_sum_only)
    names = [k for k in p if orc.is_live(k)]
    logit_t = [src["out"], tgt["out"], src["pred_domain"][1], tgt["pred_domain"][1]]
    got = torch.autograd.grad(loss, [p[k] for k in names] + logit_t, allow_unused=True)
    g = {k: gi.detach() for k, gi in zip(names, got[:len(names)]) if gi is not None}
    lg = [torch.zeros_like(t) if gi is None else gi.detach() for t, gi in zip(logit_t, got[len(names):])]
    logit_grads = {"gY_s": lg[0], "gY_t": lg[1], "gPv": torch.cat((lg[2], lg[3]), 0)}
    raw = {k: v.clone() for k, v in g.items()}
    clip_coef = 1.0
    if clip:
        total_norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(v) for v in g.values()]))
        coef = torch.clamp(clip / (total_norm + 1e-6), max=1.0)
        clip_coef = float(coef)
        g = {k: v * coef for k, v in g.items()}
    new_params = {k: v.detach().to(dtype).clone() for k, v in params.items()}
    new_mom = {}
    for k, gi in g.items():
        d = gi + weight_decay * new_params[k]
        buf = None if momentum is None else momentum.get(k)
        buf = d.clone() if buf is None else mom_coef * buf.to(dtype) + d
        new_mom[k] = buf
        d = d + mom_coef * buf
        new_params[k] = new_params[k] - lr * d
    return dict(clip_coef=clip_coef, parts={k: float(v.detach()) for k, v in parts.items()}, out=torch.cat((src["out"], tgt["out"]), 0).detach(),
                pred_vid=torch.cat((src["pred_domain"][1], tgt["pred_domain"][1]), 0).detach(), grads=raw, logit_grads=logit_grads,
                params=new_params, momentum=new_mom)


def case_reference(name, **kw):
    """reference_step of a case under its own options (kw: options replaced, for distinct())."""
    cfg, _, params, xs, xt, labels, ns, nt, cw = case_setup(name)
    use_target, ent, gamma = options(name)
    opt = dict(use_target=use_target, ent=ent, class_w=cw, gamma=gamma, alpha=CASES[name].get("kw", {}).get("alpha", 0.0))
    opt.update(kw)
    if opt["ent"] != ent:      # the oracle Config carries the attentive entropy's switch
        cfg = orc.Config(**dict(cfg.__dict__, add_loss_DA=opt["ent"] if opt["ent"] == "attentive_entropy" else "none"))
    return reference_step(cfg, params, xs, xt, labels, ns, nt, **opt)


_REF = {}


def shared_reference(name):
    """The case's reference, computed once per process and left unchanged."""
    if name not in _REF:
        _REF[name] = case_reference(name)
    return _REF[name]


def distinct(name):
    """{pair: rel. L2 distance between the block of gY under the case's option and under the option it could be mistaken for}.  Pairs:
    Sv vs uSv (target rows), target_entropy vs none (target rows), target_entropy vs attentive_entropy (source rows; where the case's model can
    form the attentive entropy at all: TransAttn, place_adv Y Y *), the sum of the weights over both halves vs over the source half (both
    blocks).  With one class every block is zero (p - 1 = 0, H = 0) under every option: no pair.  The 0.003 case keeps the pairs that do not
    rest on gamma (see the module docstring: that gamma cannot tell the entropy terms apart on rows that carry a cross-entropy too)."""
    c = CASES[name]
    cfg = case_setup(name)[0]
    use_target, ent, gamma = options(name)
    if c["C"] == 1:
        return {}
    ref = shared_reference(name)["logit_grads"]
    out = {}
    if use_target == "Sv":
        out["Sv|uSv gY_t"] = wl.rel_l2(case_reference(name, use_target="uSv")["logit_grads"]["gY_t"], ref["gY_t"])
    if ent == "target_entropy":
        out["tent|none gY_t"] = wl.rel_l2(case_reference(name, ent="none")["logit_grads"]["gY_t"], ref["gY_t"])
        if cfg.use_attn != "none" and cfg.place_adv[0] == "Y" and cfg.place_adv[1] == "Y" and gamma >= GAMMA_HU and cfg.frame_aggregation == "trn-m":
            out["tent|attentive gY_s"] = wl.rel_l2(case_reference(name, ent="attentive_entropy")["logit_grads"]["gY_s"], ref["gY_s"])
    if c.get("cw") and use_target == "Sv":
        alt = case_reference(name, source_sum_only=True)["logit_grads"]
        out["w both|source gY_s"] = wl.rel_l2(alt["gY_s"], ref["gY_s"])
        out["w both|source gY_t"] = wl.rel_l2(alt["gY_t"], ref["gY_t"])
    return out


def engine_logit_grads(eng):
    B, Bs = eng.B, eng.Bs
    gy = eng.region("gY", (B, eng.C))
    out = {"gY_s": gy[:Bs], "gY_t": gy[Bs:]}
    if "gPv" in eng.plan.regions:
        out["gPv"] = eng.region("gPv", (B, 2))
    return out


# ---- fixtures the reference itself produced with the two options on (tests/golden/make_golden_target.py) ----
FIXTURES = ["tiny_sv_tent", "tiny_avgpool_da_sv"]


def fixture_setup(name):
    """(Golden, case_config, oracle Config, use_target, add_loss_DA, gamma) of a fixture."""
    from golden_util import Golden, case_config
    g = Golden(name)
    c = case_config(g)
    avg = c["agg"] == "avgpool"
    ent = c["add_loss_DA"] or ("none" if avg else "attentive_entropy")
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                     **(dict(frame_aggregation="avgpool", use_attn="none", add_loss_DA="none", place_adv=c["place_adv"]) if avg else
                        dict(add_loss_DA=ent if ent == "attentive_entropy" else "none")))
    gamma = 0.0 if avg else (float(g.meta("gamma")) if g.has_meta("gamma") else GAMMA_SMALL)
    return g, c, cfg, str(g.meta("use_target")), ent, gamma


def fixture_batch(c, st):
    """The batch of one step as make_golden.run_case feeds it: (xs, xt, labels [Bs + Bt]) with the rows past the step's counts zeroed."""
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0
    xt[st["n_tgt"]:] = 0
    return xs, xt, torch.cat((ys, yt))
