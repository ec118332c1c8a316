#!/usr/bin/env python
"""Generate the --use_attn_frame TransAttn fixtures (tests/golden/*_faf*.npz) by running the REFERENCE ITSELF on CPU.

Needs the reference checkout, like make_golden.py:
    python tests/golden/make_golden_frame_attn.py [case ...]
Same recipe as make_golden.run_case - the reference's VideoModel.forward and main.train, weights from
ta3n_amd.synthetic - with use_attn_frame='TransAttn' threaded into the model and the argument namespace
(make_golden.py builds use_attn_frame='none' only; models.py:368-377, 612-614).  On top of run_case's records
(meta/live among them) every fixture holds
  fwd/attn_frame_{s,t}    the reference's get_trans_attn on its own frame-level domain logits, [B, T]
  meta/use_attn_frame     'TransAttn'
Every case is checked to DEPEND on the option: the class logits of the plain forward differ from the same model's
with use_attn_frame='none' by more than 10 x LOGIT_ATOL somewhere, or another weight seed is taken.
PLAIN_CASES are the other side of the bf16 distance test (tests/test_gpu_frame_attn.py): the same case - weights, batches,
options - run through the reference with use_attn_frame='none', so that the flag-off engine has an fp32 record on the very
same inputs.  (tiny_faf_T5 needs none: it is make_golden's tiny_T5 with the option on.)
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


def build_model(case, use_attn_frame="TransAttn"):
    """make_golden.build_model with frame-level attention (models.py:612-614)."""
    torch.manual_seed(1)
    m = mg.RefVideoModel(case["C"], "video", "trn-m", "RGB", train_segments=case["T"], val_segments=case["T"],
                         base_model=case["arch"], add_fc=1, fc_dim=case["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                         partial_bn=False, use_bn="none", ens_DA="none", use_attn="TransAttn", n_attn=1,
                         use_attn_frame=use_attn_frame, verbose=False, share_params="Y")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = m.state_dict()
    sd.update(mg.synth_state(shapes, seed=case["wseed"], scale=case["wscale"]))
    m.load_state_dict(sd)
    return m


def make_args(case, use_attn_frame="TransAttn"):
    a = _orig_make_args(case)
    a.use_attn_frame = use_attn_frame
    if case.get("place_adv"):      # (make_golden reads place_adv for avgpool cases only)
        a.place_adv = list(case["place_adv"])
    return a


def _thread(use_attn_frame):
    mg.build_model = lambda case: build_model(case, use_attn_frame)
    mg.make_args = lambda case: make_args(case, use_attn_frame)


def _plain_forward(case, use_attn_frame):
    model = build_model(case, use_attn_frame)
    xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], model.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"])
    model.train()
    with torch.no_grad():
        out = model(xs, xt, [0.75, 0.75, 0.5], 0, True, False)
    return model, out


def run_case(name, case):
    case = dict(case)
    for _ in range(8):      # the option has to matter at this weight seed
        _, on = _plain_forward(case, "TransAttn")
        _, off = _plain_forward(case, "none")
        if float((on[1] - off[1]).abs().max()) > 10 * LOGIT_ATOL:
            break
        case["wseed"] += 1000
    else:
        raise SystemExit(f"{name}: frame attention moves no class logit by more than {10 * LOGIT_ATOL}")
    _thread("TransAttn")
    mg.run_case(name, case)
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    model, out = _plain_forward(case, "TransAttn")
    for dom, pd in (("s", out[3]), ("t", out[8])):      # pred_domain = [relation, video, frame [B, T, 2]]
        frm = pd[2]
        mg.put(store, f"fwd/attn_frame_{dom}", model.get_trans_attn(frm.reshape(-1, 2)).view(frm.shape[0], frm.shape[1]))
    store["meta/use_attn_frame"] = np.array("TransAttn")
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path) // 1024, "KiB (with the frame attention weights), wseed", case["wseed"])


CASES = {
    # the headline command's options at the tiny shape; fc_dim % 4 == 0: 16-byte rows; short last batch: padded videos.  The weights and
    # batches of make_golden's tiny_T5 on purpose: the bf16 test compares this case's distance from fp32 with the plain lists' distance
    # from tiny_T5, and the project's rule for such a comparison (ta3n_amd/tolerances.py: BF16_REF_GRAD_CONTRACT_FACTOR) is that both
    # sides run "on the very same inputs" - at ten videos one ReLU unit that another draw flips is a tenth of a weight gradient
    "tiny_faf_T5": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=3,
                        short_last=(5, 3), lr=2e-3),
    # one relation of two-frame tuples
    "tiny_faf_T2": dict(arch="resnet18", fc_dim=32, T=2, C=5, Bs=3, Bt=2, wseed=52, wscale="trained", xseed=502, steps=1, lr=2e-3),
    # fc_dim no multiple of 8 (no twins) or 64 (a partly filled wavefront)
    "tiny_faf_odd": dict(arch="resnet18", fc_dim=20, T=4, C=6, Bs=5, Bt=4, wseed=53, wscale="trained", xseed=503, steps=2, lr=2e-3),
    # no frame-level adversarial loss: the frame discriminator is live through the attention weights alone
    "tiny_faf_advN": dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=54, wscale="trained", xseed=504, steps=2,
                          lr=2e-3, place_adv=("Y", "Y", "N")),
    # several tiles per launch in the re-ordered GEMM phases.  (xseed 505 puts one relation-discriminator unit of one video 3e-8 above
    # zero in step 1: the reference's fp32 sum and an fp64 sum disagree on its ReLU, a whole row's contribution to one bias gradient)
    "mid_faf": dict(arch="resnet18", fc_dim=128, T=5, C=12, Bs=40, Bt=24, wseed=55, wscale="trained", xseed=515, steps=2, lr=2e-3),
    # T * fc_dim > (T - 1) * 256: the scaled TRN input gradient no longer fits the relation level's region and gets one of its own
    "tiny_faf_wide": dict(arch="resnet18", fc_dim=512, T=3, C=5, Bs=3, Bt=2, wseed=56, wscale="trained", xseed=506, steps=1, lr=2e-3),
}

# the same inputs without the option; one step: the bf16 test reads step 0 (p and lr of step 0 do not depend on the step count)
PLAIN_CASES = {"mid_faf_plain": dict(CASES["mid_faf"], steps=1)}


def run_plain_case(name, case):
    _thread("none")
    mg.run_case(name, case)


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + list(PLAIN_CASES):
        run_plain_case(nm, PLAIN_CASES[nm]) if nm in PLAIN_CASES else run_case(nm, CASES[nm])
