"""frame_aggregation 'temconv' (reference models.py:44-56, 228-243, 654-672) restated with torch's own nn.Conv2d on the CPU, float64 by
default - for shapes and dropout masks the reference's fixtures (tests/golden/make_golden_temconv.py) do not hold - plus what the
temconv tests share: the fixtures' names, their configuration, one step's inputs.  Test infrastructure."""
import numpy as np
import torch
import torch.nn.functional as Fn

from golden_util import Golden, case_config, step_schedule  # noqa: F401
from ta3n_amd import _lib
from ta3n_amd.engine import flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state, synth_temconv_state  # noqa: F401

FIXTURES = ["tiny_tc_T5", "tiny_tc_T2", "tiny_tc_T3_direct", "tiny_tc_odd", "tiny_tc_src", "tiny_tc_sv_wcls", "mid_tc", "tiny_tc_eval"]
BETA = [0.75, 0.75, 0.5]
W, C0 = "tcl_3_1.conv2d.weight", "tcl_3_1.conv2d.bias"


def setup(name):
    """(Golden, case dict with use_target / class_w (None: unweighted) / flags / beta)."""
    g = Golden(name)
    c = case_config(g)
    assert str(g.meta("agg")) == "temconv" and str(g.meta("reference_patch")) == "attn placeholders bound"
    c["use_target"] = str(g.meta("use_target"))
    cw = np.asarray(g.z["meta/class_w"], np.float32)
    c["class_w"] = None if np.all(cw == 1) else cw
    adv = c["place_adv"] is not None
    c["flags"] = (flags_from_options(c["place_adv"] if adv else ("N", "N", "N"), "none", "none", "RevGrad" if adv else "none", c["use_target"]) |
                  (_lib.FLAG_CLASS_WEIGHTS if c["class_w"] is not None else 0))
    c["beta"] = BETA if adv else [0.0, 0.0, 0.0]
    return g, c


def make_plan(c, T=None, flags=None, **kw):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"] if T is None else T, c["D"], c["fc_dim"], c["C"], c["flags"] if flags is None else flags,
                     aggregation=_lib.AGG_TEMCONV, **kw)


def state_of(shapes, c):
    st = synth_state({k: s for k, s in shapes.items() if not k.startswith(("tcl_", "conv_fusion."))}, seed=c["wseed"], scale=c["wscale"])
    st.update(synth_temconv_state(shapes, seed=c["wseed"]))
    return st


def step_batch(c, st):
    """One step's batch as make_golden.run_case feeds it: rows past the step's counts zeroed; labels [Bs + Bt]."""
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    return xs, xt, torch.cat((ys, yt))


def normalisers(c, st):
    """inv_n_* of one step (ta3n_amd.parallel.loss_normalisers: under use_target Sv the class CE averages over both halves)."""
    from ta3n_amd import parallel
    return parallel.loss_normalisers(st["n_src"], st["n_tgt"], c["T"], c["flags"] & (_lib.FLAG_TARGET_LABELS | _lib.FLAG_TARGET_ENTROPY))


def aggregate(F1, w, b):
    """models.py:654-672: [B, T, F] -> [B, 1, T, F] through Conv2d(1, 1, (3, 1), padding (1, 0)), ReLU, the mean over the segments."""
    conv = torch.nn.Conv2d(1, 1, kernel_size=(3, 1), padding=(1, 0)).to(F1.dtype)
    z = torch.func.functional_call(conv, {"weight": w.reshape(1, 1, 3, 1), "bias": b.reshape(1)}, (F1.unsqueeze(1),))
    return torch.relu(z).mean(2).squeeze(1)


def step(params, x, labels, Bs, n_src, n_tgt, place_adv, beta=BETA, mask_i=None, mask_v=None, class_w=None, target_labels=False,
         extra_v=None, dtype=torch.float64):
    """Forward, the reference's loss (main.py:439-451, 508-538: class CE on the valid source rows - both halves with target_labels -
    plus the adversarial CEs of the levels in place_adv, the video level once more for place_adv[0]) and backward.
    x [B, T, D]; mask_i [B, T, F] / mask_v [B, F]: dropout factors (0 or 1 / keep), None = 1; extra_v [F]: adds 0.1 <V, extra_v> summed
    over all videos to the loss (a gradient of the caller's own at the video feature).  Returns (dict of forward tensors,
    {name: gradient} over the parameters that received one, loss)."""
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    B, T, _ = x.shape
    x = x.to(dtype)
    F1 = torch.relu(x @ P["fc_feature_shared_source.weight"].t() + P["fc_feature_shared_source.bias"])
    if mask_i is not None:
        F1 = F1 * mask_i.to(dtype)
    V = aggregate(F1, P[W], P[C0])
    Vd = V if mask_v is None else V * mask_v.to(dtype)
    lin = lambda t, n: t @ P[n + ".weight"].t() + P[n + ".bias"]
    Y = lin(Vd, "fc_classifier_video_source")
    Pv = lin(torch.relu(lin(Vd, "fc_feature_domain_video")), "fc_classifier_domain_video")
    Pf = lin(torch.relu(lin(F1, "fc_feature_domain")), "fc_classifier_domain")
    src, tgt = torch.arange(n_src), Bs + torch.arange(n_tgt)
    rows = torch.cat((src, tgt)) if target_labels else src
    cw = None if class_w is None else torch.as_tensor(class_w, dtype=dtype)
    loss = Fn.cross_entropy(Y[rows], labels[rows], weight=cw)
    dom = torch.cat((torch.zeros(n_src), torch.ones(n_tgt))).long()
    both = torch.cat((src, tgt))

    class Rev(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, b):
            ctx.b = b
            return t.view_as(t)

        @staticmethod
        def backward(ctx, gr):
            return -gr * ctx.b, None
    if place_adv[0] == "Y" or place_adv[1] == "Y":
        Pv_r = lin(torch.relu(lin(Rev.apply(Vd, beta[1]), "fc_feature_domain_video")), "fc_classifier_domain_video")
        loss = loss + Fn.cross_entropy(Pv_r[both], dom) * ((place_adv[0] == "Y") + (place_adv[1] == "Y"))
    if place_adv[2] == "Y":
        Pf_r = lin(torch.relu(lin(Rev.apply(F1, beta[2]), "fc_feature_domain")), "fc_classifier_domain")
        loss = loss + Fn.cross_entropy(Pf_r[both].reshape(-1, 2), dom.repeat_interleave(T))
    if extra_v is not None:
        loss = loss + 0.1 * (V * extra_v.to(dtype)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in P.items() if v.grad is not None}
    return dict(F1=F1.detach(), V=V.detach(), Vd=Vd.detach(), Y=Y.detach(), Pv=Pv.detach(), Pf=Pf.detach()), grads, float(loss.detach())
