#!/usr/bin/env python
"""Generate the fixtures of --pretrain_source (tests/golden/tiny_pre_*.npz, tiny_avgpool_pre.npz) by running the REFERENCE ITSELF on CPU.

Run in the build container only (needs the reference checkout, like make_golden.py):
    python tests/golden/make_golden_pretrain.py [case ...]
Same recipe and record names as make_golden.run_case - the reference's VideoModel.forward and main.train, weights and batches from
ta3n_amd.synthetic, dropout 0 - with args.pretrain_source on (main.py:388-414): every training iteration first runs a source-only pass
with an optimiser step of its own.  main.train is not touched; a torch optimiser step hook copies the parameters after every
optimizer.step(), and the first of an iteration's two is the pass's.  On top of run_case's records every fixture holds
  step<s>/pre/param/<name>   the parameters the source-only pass of iteration s reached, after it (step<s>/param/<name>: every parameter
                             after the iteration's step proper; the pass leaves the others bit-unchanged, checked here); no fwd/ records
  meta/pre_live              the parameters that pass reached (grad not None after its backward)
  meta/use_attn, meta/use_target, meta/class_w (all 1 when the class criterion is unweighted)
  meta/min_trn_preact_over_rms   the smallest |pre-activation| / rms over every TRN bottleneck output of the run (see TIE below)
"""
import os
import sys

import numpy as np
import torch
from torch.optim.optimizer import register_optimizer_step_post_hook, register_optimizer_step_pre_hook

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)
from make_golden_weighted import class_weights, weighted_criteria  # noqa: E402

EXTRA = ("use_attn", "use_target", "class_counts")
TIE = 2.0 ** -19


def run_case(name, case):
    use_attn, use_target = case.get("use_attn", "TransAttn"), case.get("use_target", "uSv")
    plain = {k: v for k, v in case.items() if k not in EXTRA}
    class_w = class_weights(case["class_counts"]) if case.get("class_counts") else torch.ones(case["C"])
    orig_args, orig_model = mg.make_args, mg.build_model

    def make_args(c):
        a = orig_args(c)
        a.pretrain_source = True
        if c.get("agg", "trn-m") != "avgpool":
            a.use_attn, a.use_target = use_attn, use_target
            if use_attn == "none":
                a.add_loss_DA = "none"
        return a

    def build_model(c):
        m = orig_model(c)
        if use_attn != "TransAttn" and c.get("agg", "trn-m") != "avgpool":
            sd = m.state_dict()
            torch.manual_seed(1)
            m = mg.RefVideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model=c["arch"], add_fc=1,
                                 fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0, partial_bn=False, use_bn="none", ens_DA="none",
                                 use_attn=use_attn, n_attn=1, use_attn_frame="none", verbose=False, share_params="Y")
            m.load_state_dict(sd)
        if hasattr(m, "TRN"):      # every pre-activation the TRN bottlenecks hand to the ReLU behind them, relative to the layer's rms
            for seq in m.TRN.fc_fusion_scales:
                seq[1].register_forward_hook(lambda mod, inp, out: ties.append(float(out.detach().abs().min() / out.detach().pow(2).mean().sqrt())))
        return m

    calls, pre_live, ties = [], [], []

    def before(opt, args, kwargs):
        if len(calls) % 2 == 0:
            pre_live.append([i for i, p in enumerate(opt.param_groups[0]["params"]) if p.grad is not None])

    def after(opt, args, kwargs):
        calls.append([p.detach().clone() for p in opt.param_groups[0]["params"]])
    mg.make_args, mg.build_model = make_args, build_model
    handles = [register_optimizer_step_pre_hook(before), register_optimizer_step_post_hook(after)]
    try:
        with weighted_criteria(class_w, torch.Tensor([1, 1])):
            mg.run_case(name, plain)
        names = [k for k, _ in build_model(plain).named_parameters()]
    finally:
        mg.make_args, mg.build_model = orig_args, orig_model
        for h in handles:
            h.remove()
    n_steps = plain.get("steps", 1)
    assert len(calls) == 2 * n_steps, (len(calls), n_steps)
    # A fixture must pin the arithmetic, not a coin toss.  With 6 + 4 videos ONE bottleneck unit whose pre-activation lies within fp32
    # round-off of zero decides a whole row of its layer's weight gradient (and, three updates later, the trajectory): two correct fp32
    # evaluations land on either side of the ReLU.  Round-off of a K <= 256 term fp32 dot product: 2^-23 sqrt(K) ~ 2^-19 of the layer's rms.
    # By the reference's own numbers such a case is refused here - take another seed.  (tiny_pre_sv_wcls at wseed 43 / xseed 431 was one:
    # scale 1, source video 5, unit 0 at 4.8e-8 of rms 0.57 in iteration 1's main forward, float64 run of the same reference code.)
    if ties:
        assert min(ties) > TIE, f"{name}: a TRN pre-activation at {min(ties):.1e} of its layer's rms sits on the ReLU's edge (< 2^-19): another seed"
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    for s in range(n_steps):
        assert len(calls[2 * s]) == len(names)
        assert pre_live[s] == pre_live[0]
        before_pass = calls[2 * s - 1] if s else None
        for i, (k, v) in enumerate(zip(names, calls[2 * s])):
            if i in pre_live[s]:
                mg.put(store, f"step{s}/pre/param/{k}", v)
            elif before_pass is not None:      # (not stored: the pass leaves it as the step before left it, bit for bit)
                assert torch.equal(v, before_pass[i]), k
    store = {k: v for k, v in store.items() if not k.startswith("fwd/")}      # (the plain forward of run_case: not what these fixtures are for)
    store["meta/pre_live"] = np.array([names[i] for i in pre_live[0]])
    store["meta/use_attn"] = np.array(use_attn)
    store["meta/use_target"] = np.array(use_target)
    store["meta/class_w"] = class_w.numpy().astype(np.float32)
    store["meta/min_trn_preact_over_rms"] = np.array([min(ties) if ties else 1.0])
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path) // 1024, "KiB; the pass reaches", len(pre_live[0]), "of", len(names), "parameters")


T5 = dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=3, lr=2e-3)
CASES = {
    # the TA3N options of the headline command at the tiny_T5 shape: 6 + 4 videos, T 5, D 512, F 64, C 12
    "tiny_pre_T5": dict(T5),
    # one relation: the smallest relation-discriminator range
    "tiny_pre_T2": dict(arch="resnet18", fc_dim=32, T=2, C=5, Bs=3, Bt=2, wseed=10, wscale="trained", xseed=5, steps=3, lr=2e-3),
    # use_attn none: the pass does not reach the relation discriminators
    "tiny_pre_noattn": dict(T5, wseed=41, xseed=411, use_attn="none"),
    # a clip value that both passes exceed
    "tiny_pre_clip": dict(T5, wseed=45, xseed=451, clip=0.05),
    # ragged last batch
    "tiny_pre_short": dict(T5, wseed=42, xseed=421, short_last=(5, 3)),
    # use_target Sv + weighted class loss: the pass keeps the weights and drops the target rows
    "tiny_pre_sv_wcls": dict(T5, wseed=44, xseed=441, use_target="Sv", class_counts=(13, 3, 46, 8, 27, 5, 60, 10, 35, 4, 20, 6)),
    # TemPooling + RevGrad (video and frame level)
    "tiny_avgpool_pre": dict(agg="avgpool", place_adv=("N", "Y", "Y"), arch="resnet18", fc_dim=64, T=5, C=5, Bs=6, Bt=4, wseed=15,
                             wscale="trained", xseed=57, steps=3, lr=2e-3),
}

if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES):
        run_case(nm, CASES[nm])
