"""Cases and the reference of the weighted criteria (--weighted_class_loss / --weighted_class_loss_DA; reference main.py:156-167, 205-206),
shared by tests/test_weighted_loss_cpu.py and tests/test_gpu_weighted_loss.py.

The arithmetic under test IS F.cross_entropy(..., weight=w).  The expected values come from oracle.ta3n_oracle.forward_domain; the loss is
assembled here exactly as oracle.total_loss assembles it, with the two criteria weighted, and differentiated by autograd: every loss
term, the logit gradients and every gradient element.  The update behind it is oracle.train_step's (clip_grad_norm_, Nesterov SGD).

Weights: class weights are 1 / freq of a deliberately skewed label list (SKEW: about 20 x between the rarest and the commonest class), the
domain weights (1 / 37, 1 / 1438).  distinct_from_unweighted() is the check that a kernel which ignored the weights, or divided by n
instead of the sum of the weights, cannot pass: the weighted and the unweighted logit gradients of the reference differ by more than 100 x
the bound the GPU test applies to them."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ta3n_oracle as orc
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_batch, synth_state

DOMAIN_W = (1.0 / 37, 1.0 / 1438)
SKEW = 20.0
BETA, GAMMA, LR = (0.75, 0.75, 0.5), 0.003, 2e-3
LOGIT_GRAD_REL_L2 = tol.F32_GRAD_REL_L2      # the bound on the logit gradients (rel. L2 per tensor); distinct_from_unweighted() asks 100 x it


def skewed_counts(C):
    """Videos per class of the made-up source list: geometric between 1 and SKEW x, dealt so that neighbouring classes differ."""
    if C == 1:
        return [3]
    order = [(7 * c + 3) % C for c in range(C)] if C % 7 else list(range(C))
    return [max(1, int(round(3 * SKEW ** (order[c] / (C - 1))))) for c in range(C)]


def class_weights(C):
    """main.py:156-164 on skewed_counts: 1 / (count / total)."""
    n = skewed_counts(C)
    total = float(sum(n))
    return [1.0 / (k / total) for k in n]


# name -> shape, options.  valid: (valid_source, valid_target); cw / dw: class / domain weights on; kw: TrainEngine keywords; cfg: oracle Config fields
CASES = {
    "trn_fp32": dict(Bs=6, Bt=4, T=5, C=12),
    "trn_ragged": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3)),
    "trn_70": dict(Bs=70, Bt=3, T=3, C=12, valid=(67, 3)),
    "trn_C64": dict(Bs=6, Bt=4, T=2, C=64),
    "trn_C1": dict(Bs=6, Bt=4, T=2, C=1),
    "class_only": dict(Bs=6, Bt=4, T=5, C=12, dw=False),
    "domain_only": dict(Bs=6, Bt=4, T=5, C=12, cw=False),
    "adv_YNY": dict(Bs=6, Bt=4, T=5, C=12, cw=False, cfg=dict(place_adv=("Y", "N", "Y"), add_loss_DA="none")),
    "adv_NYN": dict(Bs=6, Bt=4, T=5, C=12, cw=False, cfg=dict(place_adv=("N", "Y", "N"), add_loss_DA="none")),
    "unfused": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), kw=dict(fused=False)),
    "avgpool_da": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), cfg=dict(frame_aggregation="avgpool", use_attn="none", add_loss_DA="none")),
    "avgpool_src": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 4), dw=False,
                        cfg=dict(frame_aggregation="avgpool", use_attn="none", add_loss_DA="none", place_adv=("N", "N", "N"))),
    "adabn": dict(Bs=6, Bt=4, T=5, C=12, cfg=dict(use_bn="AdaBN")),
    "addfc2": dict(Bs=6, Bt=4, T=5, C=12, valid=(5, 3), cfg=dict(add_fc=2)),
}
D, FC = 512, 64


def case_setup(name, wseed=11, xseed=21):
    """(oracle Config, TrainEngine keywords, parameters, xs, xt, labels, n_src, n_tgt, class weights or None, domain weights or None)."""
    c = CASES[name]
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=D, fc_dim=FC, dropout_i=0.0, dropout_v=0.0, **c.get("cfg", {}))
    params = synth_state(param_shapes(cfg), seed=wseed)
    xs, xt, ys, _ = synth_batch(c["C"], c["T"], D, c["Bs"], c["Bt"], seed=xseed)
    ns, nt = c.get("valid", (c["Bs"], c["Bt"]))
    cw = class_weights(c["C"]) if c.get("cw", True) else None
    dw = DOMAIN_W if c.get("dw", True) else None
    if cw is not None:
        # the batch's labels follow the skew too (mostly common classes, a few rare ones): the weighted mean is then far from the plain one
        rng = np.random.default_rng(xseed + 1)
        p = np.array(skewed_counts(c["C"]), dtype=np.float64)
        ys = torch.tensor(rng.choice(c["C"], size=c["Bs"], p=p / p.sum()), dtype=torch.long)
        if c["C"] > 1:
            ys[0] = int(np.argmax(cw))      # one video of the rarest class
        ys[ns:] = int(np.argmax(cw))        # padding rows: the heaviest class - counted, they would change the sum of the weights
    # (the padding rows keep their features: a kernel that let them in would change the loss, not only the normaliser)
    return cfg, engine_kw(name, cfg), params, xs, xt, ys, ns, nt, cw, dw


def param_shapes(cfg):
    s = orc.param_shapes(cfg)
    if cfg.add_fc > 1:      # --add_fc 2 / 3 (models.py:145-153): the stacked shared layers
        for k in range(2, cfg.add_fc + 1):
            s[f"fc_feature_shared_{k}_source.weight"] = (cfg.feat_dim, cfg.feat_dim)
            s[f"fc_feature_shared_{k}_source.bias"] = (cfg.feat_dim,)
    return s


def engine_kw(name, cfg):
    from ta3n_amd.engine import flags_from_options
    c = CASES[name]
    adv_on = any(p == "Y" for p in cfg.place_adv)
    kw = dict(flags=flags_from_options(cfg.place_adv, cfg.add_loss_DA, cfg.use_attn, "RevGrad" if adv_on else "none", "uSv" if adv_on else "none"),
              aggregation=cfg.frame_aggregation, use_bn=cfg.use_bn, add_fc=cfg.add_fc, ens_DA=cfg.ens_DA)
    kw.update(c.get("kw", {}))
    return kw


def weighted_total_loss(src, tgt, label_source, gamma, cfg, n_src, n_tgt, class_w=None, domain_w=None, tgt_rev=None):
    """oracle.total_loss with criterion = CrossEntropyLoss(weight=class_w) and criterion_domain = CrossEntropyLoss(weight=domain_w)
    (main.py:205-206, 446-448, 533); the attentive entropy and dis_MCD are not weighted."""
    out_s, out_t = src["out"][:n_src], tgt["out"][:n_tgt]
    dt = out_s.dtype
    cw = None if class_w is None else torch.tensor(class_w, dtype=dt)
    dw = None if domain_w is None else torch.tensor(domain_w, dtype=dt)
    loss_c = F.cross_entropy(out_s, label_source[:n_src], weight=cw)
    parts = {"loss_c1": loss_c}
    if cfg.ens_DA == "MCD":
        parts["loss_c2"] = F.cross_entropy(src["out2"][:n_src], label_source[:n_src], weight=cw)
        loss_c = loss_c + parts["loss_c2"]
    loss = loss_c
    parts["loss_c"] = loss_c
    pred_all, loss_a = [], 0
    for l, key in enumerate(("loss_adv_rel", "loss_adv_vid", "loss_adv_frm")):
        if cfg.place_adv[l] == "Y":
            ps = src["pred_domain"][l][:n_src].reshape(-1, 2)
            pt = tgt["pred_domain"][l][:n_tgt].reshape(-1, 2)
            lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long()
            pd = torch.cat((ps, pt), 0)
            pred_all.append(pd)
            parts[key] = F.cross_entropy(pd, lab, weight=dw)
            loss_a = loss_a + parts[key]
    if pred_all:
        loss = loss + loss_a
        parts["loss_a"] = loss_a
    if cfg.ens_DA == "MCD":
        parts["loss_s"] = -orc.dis_mcd(tgt_rev["out"][:n_tgt], tgt_rev["out2"][:n_tgt])
        loss = loss + parts["loss_s"]
    if cfg.add_loss_DA == "attentive_entropy" and cfg.use_attn != "none":
        out_t_e = tgt_rev["out"][:n_tgt] if cfg.ens_DA == "MCD" else out_t
        parts["loss_e"] = orc.attentive_entropy(torch.cat((out_s, out_t_e), 0), pred_all[1])
        loss = loss + gamma * parts["loss_e"]
    parts["loss"] = loss
    return loss, parts


def _forward(cfg, beta):
    """forward_domain of the oracle; --add_fc 2 (models.py:145-153, 581-603: one more Linear(F, F) -> ReLU on the shared frame FC, which the
    oracle does not hold) as the first layer applied here and the oracle run on its output with the second layer in the shared FC's place."""
    def fwd(p, x, dom, mu=None):
        if cfg.add_fc == 2:
            B, T, Din = x.shape
            f1 = torch.relu(F.linear(x.reshape(-1, Din), p["fc_feature_shared_source.weight"], p["fc_feature_shared_source.bias"]))
            p = dict(p, **{"fc_feature_shared_source.weight": p["fc_feature_shared_2_source.weight"],
                           "fc_feature_shared_source.bias": p["fc_feature_shared_2_source.bias"]})
            x = f1.view(B, T, -1)
        return orc.forward_domain(p, x, list(beta), cfg, None, None, reverse_mu=mu, domain=dom)
    assert cfg.add_fc in (1, 2)
    return fwd


def reference_step(cfg, params, xs, xt, labels, n_src, n_tgt, class_w, domain_w, beta=BETA, gamma=GAMMA, lr=LR, momentum=None, clip=None,
                   mu=0.0, dtype=torch.float32, mom_coef=0.9, weight_decay=1e-4, forward=None):
    """One step of the reference arithmetic with the weighted criteria.  Returns dict(parts, out [B, C], pred_vid [B, 2], grads {name: tensor},
    logit_grads {"gY": [B, C], "gPv_s" / "gPv_t": the video-level domain logits' by half, "gPf_s" / "gPf_t": the frame-level ones'}, params after the step, momentum after the step)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    xs, xt = xs.to(dtype), xt.to(dtype)
    fwd = forward or _forward(cfg, beta)
    src, tgt = fwd(p, xs, "S"), fwd(p, xt, "T")
    tgt_rev = fwd(p, xt, "T", mu) if cfg.ens_DA == "MCD" else None
    loss, parts = weighted_total_loss(src, tgt, labels, gamma, cfg, n_src, n_tgt, class_w, domain_w, tgt_rev=tgt_rev)
    names = [k for k in p if orc.is_live(k)]
    logit_t = ([src["out"], tgt["out"], src["pred_domain"][1], tgt["pred_domain"][1], src["pred_domain"][2], tgt["pred_domain"][2]] +
               ([src["out2"]] if cfg.ens_DA == "MCD" else []))
    got = torch.autograd.grad(loss, [p[k] for k in names] + logit_t, allow_unused=True)
    g = {k: gi.detach() for k, gi in zip(names, got[:len(names)]) if gi is not None}
    lg = [torch.zeros_like(t) if gi is None else gi.detach() for t, gi in zip(logit_t, got[len(names):])]
    # the domain logits' gradients by half: the two domains' rows carry different factors, and each half is held to the bound on its own
    logit_grads = {"gY": torch.cat((lg[0], lg[1]), 0), "gPv_s": lg[2], "gPv_t": lg[3], "gPf_s": lg[4], "gPf_t": lg[5]}
    if cfg.ens_DA == "MCD":
        logit_grads["gY2_s"] = lg[6]
    raw = {k: v.clone() for k, v in g.items()}
    clip_coef = 1.0
    total_norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(v) for v in g.values()]))
    if clip:
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
                params=new_params, momentum=new_mom, src=src, tgt=tgt)


def rel_l2(got, want):
    want = want.detach().double().reshape(-1)
    got = got.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / (want.norm() + 1e-300))


def affected_logit_grads(cfg, class_w, domain_w):
    """The logit gradients the enabled weights change, as groups of which the weights must move at least one member far: the class logits'
    (more than one class: with one, p - 1 = 0 whatever the weight), and the domain logits' of an enabled level, by half (with n_s >> n_t
    the source rows' factor is close to 1 and the target rows' far from it)."""
    groups = []
    if class_w is not None and cfg.num_class > 1:
        groups.append(("gY",))
    if domain_w is not None and cfg.place_adv[1] == "Y":
        groups.append(("gPv_s", "gPv_t"))
    if domain_w is not None and cfg.place_adv[2] == "Y":
        groups.append(("gPf_s", "gPf_t"))
    return groups


def engine_logit_grads(eng, frame=True):
    """The same tensors from the engine's workspace (region gPf carries the frame-level adversarial CE alone)."""
    B, Bs = eng.B, eng.Bs
    out = {"gY": eng.region("gY", (B, eng.C))}
    if "gPv" in eng.plan.regions:
        gpv = eng.region("gPv", (B, 2))
        out.update(gPv_s=gpv[:Bs], gPv_t=gpv[Bs:])
    if frame and "gPf" in eng.plan.regions:
        gpf = eng.region("gPf", (B, eng.T, 2))
        out.update(gPf_s=gpf[:Bs], gPf_t=gpf[Bs:])
    return out


def distinct_from_unweighted(name):
    """[{logit gradient: rel. L2 distance between the weighted and the unweighted reference}] per group of affected_logit_grads."""
    cfg, _, params, xs, xt, ys, ns, nt, cw, dw = case_setup(name)
    w = reference_step(cfg, params, xs, xt, ys, ns, nt, cw, dw)
    u = reference_step(cfg, params, xs, xt, ys, ns, nt, None, None)
    return [{k: rel_l2(u["logit_grads"][k], w["logit_grads"][k]) for k in grp} for grp in affected_logit_grads(cfg, cw, dw)]


# ---- fixtures the reference itself produced with the two criteria weighted (tests/golden/make_golden_weighted.py) ----
FIXTURES = ["tiny_wcls_wdom", "tiny_avgpool_da_wcls"]


def fixture_setup(name):
    """(Golden, case_config, oracle Config, class weights or None, domain weights or None) of a weighted fixture."""
    from golden_util import Golden, case_config
    g = Golden(name)
    c = case_config(g)
    avg = c["agg"] == "avgpool"
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                     **(dict(frame_aggregation="avgpool", use_attn="none", add_loss_DA="none", place_adv=c["place_adv"]) if avg else {}))
    cw = [float(v) for v in g.meta("class_w")]
    dw = tuple(float(v) for v in g.meta("domain_w"))
    return g, c, cfg, (None if all(v == 1.0 for v in cw) else cw), (None if dw == (1.0, 1.0) else dw)


def log_numbers(line):
    """{Loss, loss_c, loss_a, loss_e: value} of one line of the reference's train log (main.py:590-617)."""
    import re
    return {k: float(v) for k, v in re.findall(r"(Loss|loss_c|loss_a|loss_e) (-?[0-9.]+)", line)}
