#!/usr/bin/env python
"""Generate the --frame_aggregation temconv fixtures (tests/golden/*_tc_*.npz, mid_tc.npz, temconv_init.npz) by running the REFERENCE'S
OWN LAYERS and its own main.train on CPU.

Needs the reference checkout, like make_golden.py:
    python tests/golden/make_golden_temconv.py [case ...]

One fact about the reference first.  Its VideoModel.forward computes everything on the temconv branch (models.py:654-672: tcl_3_1, ReLU,
the mean over the segments) and then fails at its return with UnboundLocalError: the avgpool / rnn branch and the trn branch bind the two
attention placeholders attn_relation_source / attn_relation_target, the temconv branch forgets to.  Nothing of the loss reads them
(main.train only slices them in removeDummy).  So the model that writes these fixtures is a subclass of the reference's VideoModel whose
forward is the reference's own source - taken with inspect.getsource when this script runs; no line of it is written here - with ONE
statement of this script's inserted in front of the single line `if self.baseline_type == 'video':` that follows the aggregation
branches: on temconv it binds the two names to column 0 of the two video features (before dropout_v), which is what the other non-TRN
branches bind them to.  The script asserts that the anchor line occurs exactly once, that the unpatched reference still raises
UnboundLocalError (so a repaired reference is noticed), and that the patched and the unpatched model have identical state_dicts.
Every fixture records meta/reference_patch = "attn placeholders bound".

Otherwise the recipe and record layout of make_golden.run_case, with the option set of make_golden's TemPooling cases (RevGrad with the
case's place_adv, or use_target none without one).  The two live temconv tensors come from ta3n_amd.synthetic.synth_temconv_state.  On
top of run_case's records every fixture holds meta/agg 'temconv', meta/state_keys (the reference's state_dict key order),
meta/use_target, meta/class_w, and - where the case has a val_T - meta/val_T, eval/out_t, eval/feat_t_v: an eval-mode forward of the
untrained weights on val_T segments.

A case is refused when the option does not matter (no class logit of the plain forward differs from the same weights' avgpool logits
by 10 x LOGIT_ATOL), when on any of its batches fewer than 10 % or more than 90 % of the entries of Z = conv(F1) are positive (the ReLU
must cut: F1 >= 0, so all-positive taps never would), or when a nonzero |Z| lies below 1e-6 x max |Z| (its sign would be the rounding's).
temconv_init.npz: the state_dict right after construction under torch.manual_seed(1).
"""
import contextlib
import inspect
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)
from make_golden_weighted import class_weights, weighted_criteria  # noqa: E402

import models as ref_models  # noqa: E402  (the reference's, through the shim's sys.path)

from ta3n_amd.synthetic import synth_temconv_state  # noqa: E402
from ta3n_amd.tolerances import LOGIT_ATOL  # noqa: E402

ANCHOR = "if self.baseline_type == 'video':"
PATCH_NOTE = "attn placeholders bound"


def _placeholders(v_source, v_target):
    """What the avgpool / rnn branch binds the two attention placeholders to: column 0 of the video features."""
    return v_source[:, 0], v_target[:, 0]


def _patched_class():
    src = textwrap.dedent(inspect.getsource(mg.RefVideoModel.forward))
    lines = src.splitlines()
    hits = [i for i, ln in enumerate(lines) if ln.strip() == ANCHOR]
    assert len(hits) == 1, f"anchor line occurs {len(hits)} times in the reference's forward"
    at = hits[0]
    indent = lines[at][:len(lines[at]) - len(lines[at].lstrip())]
    mine = (indent + "if self.frame_aggregation == 'temconv': attn_relation_source, attn_relation_target = "
            "_placeholders(feat_fc_video_source, feat_fc_video_target)")
    env = dict(vars(ref_models))
    env["_placeholders"] = _placeholders
    exec(compile("\n".join(lines[:at] + [mine] + lines[at:]), "<reference forward, attn placeholders bound>", "exec"), env)
    return type("PatchedRefVideoModel", (mg.RefVideoModel,), {"forward": env["forward"]})


Patched = _patched_class()


def _construct(cls, case, agg="temconv"):
    torch.manual_seed(1)
    return cls(case["C"], "video", agg, "RGB", train_segments=case["T"], val_segments=case.get("val_T", case["T"]),
               base_model=case["arch"], add_fc=1, fc_dim=case["fc_dim"], dropout_i=0.0, dropout_v=0.0, partial_bn=False, use_bn="none",
               ens_DA="none", use_attn="none", n_attn=1, use_attn_frame="none", verbose=False, share_params="Y")


def build_model(case, agg="temconv", cls=None):
    m = _construct(cls or Patched, case, agg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = m.state_dict()
    # (the temconv layers take no draw from synth_state's stream - the other tensors are what a plan's parameter list gives; the layers
    # the forward never calls keep their construction values)
    sd.update(mg.synth_state({k: s for k, s in shapes.items() if not k.startswith(("tcl_", "conv_fusion."))}, seed=case["wseed"], scale=case["wscale"]))
    sd.update(synth_temconv_state(shapes, seed=case["wseed"]))
    m.load_state_dict(sd)
    return m


def check_the_patch(case):
    """The unpatched reference still fails, by the error this script works around; the patch changes no parameter."""
    plain, mine = _construct(mg.RefVideoModel, case), _construct(Patched, case)
    a, b = plain.state_dict(), mine.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], plain.feature_dim, 2, 2, seed=1)
    try:
        with torch.no_grad():
            plain(xs, xt, [0, 0, 0], 0, True, False)
    except UnboundLocalError as e:
        assert "attn_relation_source" in str(e), e
    else:
        raise SystemExit("the reference's temconv forward no longer raises: the patch of this script is not needed any more")


_orig_make_args = mg.make_args
_orig_build_model = mg.build_model


def make_args(case):
    a = _orig_make_args(dict(case, agg="avgpool"))      # the TemPooling option set: use_attn none, RevGrad with place_adv or everything off
    if case.get("use_target"):
        a.use_target = case["use_target"]
    return a


def _refusal(case):
    """'' or why this case must not become a fixture."""
    on, off = build_model(case), build_model(case, "avgpool")
    off.load_state_dict({k: v for k, v in on.state_dict().items() if k in off.state_dict()})
    worst = 0.0
    for s in range(case.get("steps", 1)):
        xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], on.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"] + 100 * s)
        on.train(); off.train()
        with torch.no_grad():
            a, b = on(xs, xt, [0, 0, 0], 0, True, False), off(xs, xt, [0, 0, 0], 0, True, False)
            worst = max(worst, float((a[1] - b[1]).abs().max()), float((a[6] - b[6]).abs().max()))
            f1 = torch.cat((a[4][2], a[9][2]))
            z = on.tcl_3_1(f1.unsqueeze(1)).squeeze(1)
        pos = float((z > 0).float().mean())
        if not 0.1 <= pos <= 0.9:
            return f"{100 * pos:.1f} % of the entries of Z are positive on the batch of step {s} (10 % .. 90 %)"
        az = z.abs()
        if bool(((az > 0) & (az < 1e-6 * az.max())).any()):
            return f"a nonzero |Z| lies below 1e-6 x max |Z| on the batch of step {s}"
    if worst < 10 * LOGIT_ATOL:
        return f"the aggregation moves no class logit by {10 * LOGIT_ATOL} (largest difference from avgpool: {worst:.3g})"
    return ""


def run_case(name, case):
    check_the_patch(case)
    why = _refusal(case)
    if why:
        raise SystemExit(f"{name}: {why}")
    class_w = class_weights(case["class_counts"]) if case.get("class_counts") else torch.ones(case["C"])
    plain = {k: v for k, v in case.items() if k not in ("class_counts", "use_target", "val_T")}
    plain["agg"] = "avgpool"      # run_case's own switches (beta, gamma, which records): those of its TemPooling cases
    mg.build_model = lambda c: build_model(case)
    mg.make_args = lambda c: make_args(case)
    try:
        with weighted_criteria(class_w, torch.Tensor([1, 1])) if case.get("class_counts") else contextlib.nullcontext():
            mg.run_case(name, plain)
    finally:
        mg.build_model, mg.make_args = _orig_build_model, _orig_make_args
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    store["meta/agg"] = np.array("temconv")
    store["meta/reference_patch"] = np.array(PATCH_NOTE)
    store["meta/use_target"] = np.array(make_args(case).use_target)
    store["meta/class_w"] = class_w.numpy().astype(np.float32)
    model = build_model(case)
    store["meta/state_keys"] = np.array(list(model.state_dict().keys()))
    if case.get("val_T"):      # main.validate's call (main.py:707): the validation clip in both slots, eval mode
        xv, _, _, _ = mg.synth_batch(case["C"], case["val_T"], model.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"] + 7)
        model.eval()
        with torch.no_grad():
            ev = model(xv, xv, [0, 0, 0], 0, False, False)
        store["meta/val_T"] = np.array([case["val_T"]])
        mg.put(store, "eval/out_t", ev[6]); mg.put(store, "eval/feat_t_v", ev[9][1])
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path), "bytes")


def run_init(name):
    case = dict(C=7, T=5, arch="resnet18", fc_dim=32)
    check_the_patch(case)
    sd = _construct(mg.RefVideoModel, case).state_dict()
    store = {"keys": np.array(list(sd.keys())), "meta/reference_patch": np.array(PATCH_NOTE)}
    for k, v in sd.items():
        store[f"state/{k}"] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path), "bytes")


_T5 = dict(arch="resnet18", fc_dim=64, T=5, C=5, Bs=6, Bt=4, wscale="trained", lr=2e-3)
_F32 = dict(arch="resnet18", fc_dim=32, C=5, Bs=5, Bt=4, wscale="trained", lr=2e-3)
CASES = {
    # padded videos in the last batch, later steps
    "tiny_tc_T5": dict(_T5, place_adv=("N", "Y", "Y"), steps=3, short_last=(5, 3), wseed=61, xseed=601),
    # every row touches the zero padding; place_adv[0] = Y: the video-level loss counted twice
    "tiny_tc_T2": dict(_F32, T=2, place_adv=("Y", "Y", "Y"), steps=2, wseed=62, xseed=602),
    # no frame discriminator: the kernel writes gZ1 itself
    "tiny_tc_T3_direct": dict(_F32, T=3, place_adv=("N", "Y", "N"), steps=2, wseed=63, xseed=603),
    # rows not 32-byte aligned
    "tiny_tc_odd": dict(arch="resnet18", fc_dim=20, T=7, C=7, Bs=5, Bt=4, wscale="trained", lr=2e-3, place_adv=("N", "Y", "Y"), steps=2,
                        wseed=74, xseed=604),
    # use_target none: no flag at all on the general builder
    "tiny_tc_src": dict(_T5, steps=2, wseed=65, xseed=605),
    # the weighted and labelled loss paths
    "tiny_tc_sv_wcls": dict(_T5, place_adv=("N", "Y", "Y"), steps=2, short_last=(5, 3), wseed=66, xseed=606, use_target="Sv",
                            class_counts=(40, 2, 9, 21, 4)),
    # several tiles per launch; 64 partial rows in the parameter-gradient sum
    "mid_tc": dict(arch="resnet18", fc_dim=128, T=5, C=12, Bs=40, Bt=24, wscale="trained", lr=2e-3, place_adv=("N", "Y", "Y"), steps=2,
                   wseed=67, xseed=607),
    # validation on another segment count: a second plan
    "tiny_tc_eval": dict(_F32, T=5, val_T=25, place_adv=("N", "Y", "Y"), steps=1, wseed=78, xseed=608),
}

if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + ["temconv_init"]:
        if nm == "temconv_init":
            run_init(nm)
        else:
            run_case(nm, CASES[nm])
