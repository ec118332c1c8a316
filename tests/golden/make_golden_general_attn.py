#!/usr/bin/env python
"""Generate the --use_attn general fixtures (tests/golden/*_ga*.npz) by running the REFERENCE ITSELF on CPU.

Needs the reference checkout, like make_golden.py:
    python tests/golden/make_golden_general_attn.py [case ...]
Same recipe as make_golden.run_case - the reference's VideoModel.forward and main.train, weights from
ta3n_amd.synthetic - with use_attn='general' threaded into the model and the argument namespace
(make_golden.py builds use_attn='TransAttn' only; models.py:320-325, 359-366, 379-388).  On top of run_case's records
(meta/live and fwd/attn_{s,t}, the softmax weights, among them) every fixture holds
  meta/use_attn      'general'
  meta/state_keys    the reference's state_dict key order (attn_layer.* last)
Every case is checked to DEPEND on the option: the class logits of the plain forward differ from the same weights'
with use_attn='none' by more than 10 x LOGIT_ATOL somewhere and - except with one relation (T = 2: the softmax over one
score is 1) - the attention weights of some video spread by more than 0.05; otherwise another weight seed is taken.
PLAIN_CASES are the other side of the bf16 distance test (tests/test_gpu_general_attn.py): the same case - weight seed,
batches, options - run through the reference with use_attn='TransAttn', so that the TransAttn unfused engine has an fp32
record on the very same inputs.  (tiny_ga_T5 needs none: it is make_golden's tiny_T5 with the option on.)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)

from ta3n_amd.tolerances import LOGIT_ATOL  # noqa: E402

_orig_make_args = mg.make_args


def build_model(case, use_attn="general"):
    """make_golden.build_model with the kind of relation attention as an argument (models.py:320-325)."""
    torch.manual_seed(1)
    m = mg.RefVideoModel(case["C"], "video", "trn-m", "RGB", train_segments=case["T"], val_segments=case["T"],
                         base_model=case["arch"], add_fc=1, fc_dim=case["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                         partial_bn=False, use_bn="none", ens_DA="none", use_attn=use_attn, n_attn=1,
                         use_attn_frame="none", verbose=False, share_params="Y")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = m.state_dict()
    sd.update(mg.synth_state(shapes, seed=case["wseed"], scale=case["wscale"]))
    m.load_state_dict(sd)
    return m


def make_args(case, use_attn="general"):
    a = _orig_make_args(case)
    a.use_attn = use_attn
    if case.get("place_adv"):      # (make_golden reads place_adv for avgpool cases only)
        a.place_adv = list(case["place_adv"])
    return a


def _thread(use_attn):
    mg.build_model = lambda case: build_model(case, use_attn)
    mg.make_args = lambda case: make_args(case, use_attn)


def _plain_forward(case, model):
    xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], model.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"])
    model.train()
    with torch.no_grad():
        return model(xs, xt, [0.75, 0.75, 0.5], 0, True, False)


def _depends_on_the_option(case):
    """(largest class-logit difference against use_attn none on the same weights, largest spread of one video's weights)."""
    on = build_model(case, "general")
    off = build_model(case, "none")
    off.load_state_dict({k: v for k, v in on.state_dict().items() if not k.startswith("attn_layer.")})
    a, b = _plain_forward(case, on), _plain_forward(case, off)
    logit = max(float((a[1] - b[1]).abs().max()), float((a[6] - b[6]).abs().max()))
    w = torch.cat((a[0], a[5]), 0)
    assert float((w.sum(1) - 1).abs().max()) < 1e-5
    return logit, float((w.max(1).values - w.min(1).values).max())


def run_case(name, case):
    case = dict(case)
    for _ in range(8):      # the option has to matter at this weight seed
        logit, spread = _depends_on_the_option(case)
        if logit > 10 * LOGIT_ATOL and (case["T"] == 2 or spread > 0.05):
            break
        case["wseed"] += 1000
    else:
        raise SystemExit(f"{name}: general attention moves no class logit by more than {10 * LOGIT_ATOL} / spreads no video's weights by 0.05")
    _thread("general")
    mg.run_case(name, case)
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    store["meta/use_attn"] = np.array("general")
    store["meta/state_keys"] = np.array(list(build_model(case, "general").state_dict().keys()))
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path), "bytes, wseed", case["wseed"], f"logit difference {logit:.3g}, weight spread {spread:.3g}")


CASES = {
    # make_golden's tiny_T5 verbatim (the headline options at the tiny shape; short last batch: padded videos) with the option on: the
    # bf16 test compares this case's distance from fp32 with the TransAttn lists' distance from tiny_T5 on the same batches
    "tiny_ga_T5": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=3,
                       short_last=(5, 3), lr=2e-3),
    # one relation: w = 1 exactly, the attention layer's gradients are zero but live (weight decay and momentum move it)
    "tiny_ga_T2": dict(arch="resnet18", fc_dim=32, T=2, C=5, Bs=3, Bt=2, wseed=62, wscale="trained", xseed=602, steps=1, lr=2e-3),
    # fc_dim no multiple of 8: rows not 16-byte aligned, no twins
    "tiny_ga_odd": dict(arch="resnet18", fc_dim=20, T=4, C=6, Bs=5, Bt=4, wseed=63, wscale="trained", xseed=603, steps=2, lr=2e-3),
    # no relation-level adversarial loss and no attentive entropy: the relation discriminators are dead, the attention layer is live
    "tiny_ga_relN": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=64, wscale="trained", xseed=604, steps=2, lr=2e-3,
                         place_adv=("N", "Y", "Y"), add_loss_DA="none"),
    # eight relations, three sampled tuples per scale
    "tiny_ga_T9": dict(arch="resnet18", fc_dim=32, T=9, C=30, Bs=5, Bt=5, wseed=65, wscale="trained", xseed=605, steps=2, lr=2e-3),
    # several tiles per launch; K = B (T - 1) = 256 in the tile of the attention layer's weight gradient
    "mid_ga": dict(arch="resnet18", fc_dim=128, T=5, C=12, Bs=40, Bt=24, wseed=66, wscale="trained", xseed=616, steps=2, lr=2e-3),
}

# the same inputs with use_attn TransAttn; one step: the bf16 test reads step 0 (p and lr of step 0 do not depend on the step count)
PLAIN_CASES = {"mid_ga_plain": dict(CASES["mid_ga"], steps=1)}


def run_plain_case(name, case):
    _thread("TransAttn")
    mg.run_case(name, case)


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + list(PLAIN_CASES):
        run_plain_case(nm, PLAIN_CASES[nm]) if nm in PLAIN_CASES else run_case(nm, CASES[nm])
