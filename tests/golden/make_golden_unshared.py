#!/usr/bin/env python
"""Generate the --share_params N fixtures (tests/golden/*_sp*.npz) by running the REFERENCE ITSELF on CPU.

Needs the reference checkout, like make_golden.py:
    python tests/golden/make_golden_unshared.py [case ...]
Same recipe as make_golden.run_case - the reference's VideoModel.forward and main.train, weights from ta3n_amd.synthetic - with
share_params='N' threaded into the model (make_golden.py builds share_params='Y' only; models.py:174-192, 296-305, 565-566,
686-687) and use_target / add_loss_DA / place_adv of the case into the argument namespace.  On top of run_case's records (meta/live
among them) every fixture holds
  meta/share_params            'N' ('Y' for PLAIN_CASES)
  meta/state_keys              the reference's state_dict key order
  meta/use_target              the value of --use_target the reference ran with
  eval/out_t, eval/feat_t_v    an eval-mode model(xs, xs, [0, 0, 0], 0, False, False) on the INITIAL weights: main.validate's call
                               (main.py:707), whose target branch runs through the target layers
  eval/out_s                   the same call's source branch (what a validation through the wrong layers would score)
Every case is checked to DEPEND on the option: the target class logits of the plain forward differ from those of the same
weights with the target layers overwritten by their source twins by more than 10 x LOGIT_ATOL somewhere; otherwise another weight
seed is taken.
PLAIN_CASES are the other side of the bf16 distance test (tests/test_gpu_unshared.py): the same case - weight seed, batches,
options - run through the reference with share_params='Y'.  (tiny_sp_T5 needs none: it is make_golden's tiny_T5 with the option on.)
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

TWINS = {"fc_feature_shared_target": "fc_feature_shared_source", "fc_feature_target": "fc_feature_source",
         "fc_classifier_target": "fc_classifier_source", "fc_feature_video_target": "fc_feature_video_source",
         "fc_feature_video_target_2": "fc_feature_video_source_2", "fc_classifier_video_target": "fc_classifier_video_source"}


def build_model(case, share_params="N"):
    """make_golden.build_model with share_params as an argument (models.py:174-192, 296-305)."""
    torch.manual_seed(1)
    m = mg.RefVideoModel(case["C"], "video", "trn-m", "RGB", train_segments=case["T"], val_segments=case["T"],
                         base_model=case["arch"], add_fc=1, fc_dim=case["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                         partial_bn=False, use_bn="none", ens_DA="none", use_attn="TransAttn", n_attn=1,
                         use_attn_frame="none", verbose=False, share_params=share_params)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = m.state_dict()
    sd.update(mg.synth_state(shapes, seed=case["wseed"], scale=case["wscale"]))
    m.load_state_dict(sd)
    return m


def make_args(case):
    a = _orig_make_args(case)      # (takes the case's add_loss_DA itself)
    a.use_target = case.get("use_target", "uSv")
    if case.get("place_adv"):      # (make_golden reads place_adv for avgpool cases only)
        a.place_adv = list(case["place_adv"])
    return a


def _thread(share_params):
    mg.build_model = lambda case: build_model(case, share_params)
    mg.make_args = make_args


def _target_logits(case, model):
    xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], model.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"])
    model.train()
    with torch.no_grad():
        return model(xs, xt, [0.75, 0.75, 0.5], 0, True, False)[6]


def _depends_on_the_option(case):
    """Largest target class-logit difference against the same weights with the target layers overwritten by their source twins."""
    on, off = build_model(case), build_model(case)
    sd = off.state_dict()
    for tgt, src in TWINS.items():
        for leaf in ("weight", "bias"):
            sd[f"{tgt}.{leaf}"] = sd[f"{src}.{leaf}"].clone()
    off.load_state_dict(sd)
    return float((_target_logits(case, on) - _target_logits(case, off)).abs().max())


def _eval_records(case, share_params):
    model = build_model(case, share_params)
    xs, _, _, _ = mg.synth_batch(case["C"], case["T"], model.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"])
    model.eval()
    with torch.no_grad():
        ev = model(xs, xs, [0, 0, 0], 0, False, False)
    rec = {}
    mg.put(rec, "eval/out_t", ev[6]); mg.put(rec, "eval/feat_t_v", ev[9][1]); mg.put(rec, "eval/out_s", ev[1])
    return rec, list(model.state_dict().keys())


def _finish(name, case, share_params):
    path = os.path.join(HERE, name + ".npz")
    store = dict(np.load(path, allow_pickle=False))
    rec, keys = _eval_records(case, share_params)
    store.update(rec)
    store["meta/share_params"] = np.array(share_params)
    store["meta/state_keys"] = np.array(keys)
    store["meta/use_target"] = np.array(case.get("use_target", "uSv"))
    np.savez_compressed(path, **store)
    return path


def run_case(name, case):
    case = dict(case)
    for _ in range(8):      # the option has to matter at this weight seed
        logit = _depends_on_the_option(case)
        if logit > 10 * LOGIT_ATOL:
            break
        case["wseed"] += 1000
    else:
        raise SystemExit(f"{name}: the target layers move no target class logit by more than {10 * LOGIT_ATOL}")
    _thread("N")
    mg.run_case(name, case)
    path = _finish(name, case, "N")
    print(name, "->", path, os.path.getsize(path), "bytes, wseed", case["wseed"], f"target logit difference {logit:.3g}")


TINY_T5 = dict(arch="resnet18", fc_dim=64, T=5, C=12, Bs=6, Bt=4, wseed=7, wscale="trained", xseed=1234, steps=3, short_last=(5, 3), lr=2e-3)

CASES = {
    # make_golden's tiny_T5 verbatim (the headline options at the tiny shape; short last batch: padded videos in both halves) with the option on
    "tiny_sp_T5": dict(TINY_T5),
    # one relation; the boundary at row 6
    "tiny_sp_T2": dict(arch="resnet18", fc_dim=32, T=2, C=5, Bs=3, Bt=2, wseed=72, wscale="trained", xseed=702, steps=1, lr=2e-3),
    # fc_dim no multiple of 8: rows not 16-byte aligned, no twins; the boundary at row 20
    "tiny_sp_odd": dict(arch="resnet18", fc_dim=20, T=4, C=6, Bs=5, Bt=4, wseed=73, wscale="trained", xseed=703, steps=2, lr=2e-3),
    # each half a single video
    "tiny_sp_one": dict(arch="resnet18", fc_dim=32, T=3, C=5, Bs=1, Bt=1, wseed=74, wscale="trained", xseed=704, steps=1, lr=2e-3),
    # no loss reads the target class logits: fc_classifier_video_target is dead, fc_feature_shared_target is live
    "tiny_sp_noent": dict(TINY_T5, add_loss_DA="none"),
    # the target classifier is trained by the cross-entropy
    "tiny_sp_sv": dict(TINY_T5, use_target="Sv"),
    # several tiles per spec; the boundary at row 200 and video 40, inside a tile on every tile height (one step: two make the file
    # larger than headline.npz)
    "mid_sp": dict(arch="resnet18", fc_dim=128, T=5, C=12, Bs=40, Bt=24, wseed=76, wscale="trained", xseed=716, steps=1, lr=2e-3),
}

# the same inputs with share_params Y
PLAIN_CASES = {"mid_sp_plain": dict(CASES["mid_sp"])}


def run_plain_case(name, case, of="mid_sp"):
    case = dict(case)
    done = os.path.join(HERE, of + ".npz")      # the weight seed the flagged case settled on
    if os.path.exists(done):
        case["wseed"] = int(np.load(done)["meta/wseed"][0])
    _thread("Y")
    mg.run_case(name, case)
    path = _finish(name, case, "Y")
    print(name, "->", path, os.path.getsize(path), "bytes, wseed", case["wseed"])


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + list(PLAIN_CASES):
        run_plain_case(nm, PLAIN_CASES[nm]) if nm in PLAIN_CASES else run_case(nm, CASES[nm])
