#!/usr/bin/env python
"""Generate the --frame_aggregation rnn fixtures (tests/golden/*_rnn_*.npz, rnn_init.npz, rnn_slots_golden.npz) by running the REFERENCE
ITSELF on CPU.

Needs the reference checkout, like make_golden.py:
    python tests/golden/make_golden_rnn.py [case ...]
Same recipe and record layout as make_golden.run_case - the reference's VideoModel.forward and main.train, weights and batches from
ta3n_amd.synthetic - with frame_aggregation='rnn', rnn_cell, n_ts and use_attn='none' threaded into the model and the argument
namespace (models.py:202-215, 392-422; the DA options are those of make_golden's TemPooling cases: RevGrad with the case's place_adv,
or use_target none without one).  The four rnn.* tensors come from ta3n_amd.synthetic.synth_rnn_state - weights N(0, 1 / fan_in), biases
N(0, 0.01) - because synth_state's 'trained' scale leaves them at 0.01 (every gate within a few hundredths of its value at 0).  On top of
run_case's records every fixture holds
  meta/agg 'rnn', meta/rnn_cell, meta/n_ts, meta/state_keys (the reference's state_dict key order), meta/use_target, meta/class_w
  meta/val_T and eval/out_t, eval/feat_t_v where the case has a val_T: an eval-mode forward of the untrained weights on val_T segments
A case is refused when the option does not matter (no class logit of the plain forward differs from the same weights' avgpool logits
by 10 x LOGIT_ATOL), when a pooling window of any of its batches holds two distinct frames with equal positive maxima (the argmax
would need a rule of its own), or when every gate pre-activation is saturated (|x| > 8).
rnn_init.npz: the state_dict right after construction under torch.manual_seed(1), both cells.  rnn_slots_golden.npz: the reference's own
pooling lines of aggregate_frames on a [1, T, 1] ramp (frame t holds t + 1) for T 1..64, n_ts 1..8 - each window's maximum, or -1
everywhere where the reference raised.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim, imports the reference's main / models)
from make_golden_weighted import class_weights, weighted_criteria  # noqa: E402

from ta3n_amd import _lib  # noqa: E402
from ta3n_amd.synthetic import synth_rnn_state  # noqa: E402
from ta3n_amd.tolerances import LOGIT_ATOL  # noqa: E402

_orig_make_args = mg.make_args


def build_model(case, agg="rnn"):
    torch.manual_seed(1)
    m = mg.RefVideoModel(case["C"], "video", agg, "RGB", train_segments=case["T"], val_segments=case.get("val_T", case["T"]),
                         base_model=case["arch"], add_fc=1, fc_dim=case["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                         partial_bn=False, use_bn="none", ens_DA="none", use_attn="none", n_attn=1, use_attn_frame="none",
                         verbose=False, share_params="Y", n_rnn=1, rnn_cell=case["rnn_cell"], n_directions=1, n_ts=case["n_ts"])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = m.state_dict()
    sd.update(mg.synth_state(shapes, seed=case["wseed"], scale=case["wscale"]))
    sd.update(synth_rnn_state(shapes, seed=case["wseed"]))
    m.load_state_dict(sd)
    return m


def make_args(case):
    a = _orig_make_args(dict(case, agg="avgpool"))      # the TemPooling option set: use_attn none, RevGrad with place_adv or everything off
    if case.get("use_target"):
        a.use_target = case["use_target"]
    return a


def _windows(f1, n_ts):
    """([B, n_ts, len_ts, F] frame features per pooling slot, [n_ts, len_ts] frame of each slot) by the library's slot table
    (ta3n_rnn_slots; rnn_slots_golden.npz pins it to the reference's pooling)."""
    len_ts, frames = _lib.rnn_slots(f1.shape[1], n_ts)
    frames = torch.tensor(frames).view(n_ts, len_ts)
    return f1[:, frames, :], frames


def _refusal(case):
    """'' or why this case must not become a fixture."""
    on, off = build_model(case), build_model(case, "avgpool")
    off.load_state_dict({k: v for k, v in on.state_dict().items() if k in off.state_dict()})
    worst, unsaturated = 0.0, False
    steps = case.get("steps", 1)
    for s in range(steps):
        xs, xt, _, _ = mg.synth_batch(case["C"], case["T"], on.feature_dim, case["Bs"], case["Bt"], seed=case["xseed"] + 100 * s)
        on.train(); off.train()
        with torch.no_grad():
            a, b = on(xs, xt, [0, 0, 0], 0, True, False), off(xs, xt, [0, 0, 0], 0, True, False)
        worst = max(worst, float((a[1] - b[1]).abs().max()), float((a[6] - b[6]).abs().max()))
        for f1 in (a[4][2], a[9][2]):
            w, frames = _windows(f1, case["n_ts"])
            mx = w.max(2, keepdim=True).values
            hit = (w == mx) & (mx > 0)
            for j in range(case["n_ts"]):
                for k in range(frames.shape[1]):
                    for l in range(k + 1, frames.shape[1]):
                        if frames[j, k] != frames[j, l] and bool((hit[:, j, k] & hit[:, j, l]).any()):
                            return f"window {j} of step {s} holds two frames with equal positive maxima"
            xp = w.max(2).values
            pre = xp @ on.rnn.weight_ih_l0.t() + on.rnn.bias_ih_l0 + on.rnn.bias_hh_l0      # (first step: h = 0)
            unsaturated = unsaturated or bool((pre.abs() <= 8).any())
    if worst < 10 * LOGIT_ATOL:
        return f"the aggregation moves no class logit by {10 * LOGIT_ATOL} (largest difference from avgpool: {worst:.3g})"
    if not unsaturated:
        return "every gate pre-activation is saturated (|x| > 8)"
    return ""


def run_case(name, case):
    why = _refusal(case)
    if why:
        raise SystemExit(f"{name}: {why}")
    class_w = class_weights(case["class_counts"]) if case.get("class_counts") else torch.ones(case["C"])
    plain = {k: v for k, v in case.items() if k not in ("class_counts", "use_target", "rnn_cell", "val_T")}
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
    store["meta/agg"] = np.array("rnn")
    store["meta/rnn_cell"] = np.array(case["rnn_cell"])
    store["meta/n_ts"] = np.array([case["n_ts"]])
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


_orig_build_model = mg.build_model


def run_init(name):
    store = {}
    for cell in ("LSTM", "GRU"):
        torch.manual_seed(1)
        m = mg.RefVideoModel(7, "video", "rnn", "RGB", train_segments=5, val_segments=5, base_model="resnet18", add_fc=1, fc_dim=32,
                             partial_bn=False, use_attn="none", verbose=False, rnn_cell=cell, n_ts=5)
        sd = m.state_dict()
        store[f"{cell}/keys"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            store[f"{cell}/state/{k}"] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **store)
    print(name, "->", path, os.path.getsize(path), "bytes")


class _Capture(torch.nn.Module):
    """Stands where the reference's nn.LSTM stands: keeps what aggregate_frames hands to it (the pooled windows)."""

    def flatten_parameters(self):
        pass

    def forward(self, x, h):
        self.x = x
        return x, None


def run_slots(name):
    torch.manual_seed(1)
    m = mg.RefVideoModel(7, "video", "rnn", "RGB", train_segments=5, val_segments=5, base_model="resnet18", add_fc=1, fc_dim=32,
                         partial_bn=False, use_attn="none", verbose=False, rnn_cell="LSTM", n_ts=5)
    m.rnn = _Capture()
    out = np.full((65, 9, 8), -1, np.int32)      # [T][n_ts][window]: the maximum of the ramp = 1 + the highest frame of the window
    for T in range(1, 65):
        for n_ts in range(1, 9):
            m.n_ts = n_ts
            ramp = torch.arange(1, T + 1, dtype=torch.float32).view(T, 1)
            try:
                m.aggregate_frames(ramp, T, None)
            except Exception:
                continue
            out[T, n_ts, :n_ts] = m.rnn.x.view(-1).to(torch.int32).numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, window_max=out)
    print(name, "->", path, os.path.getsize(path), "bytes;", int((out[1:, 1:, 0] < 0).sum()), "of 512 pairs raise")


_T5 = dict(arch="resnet18", fc_dim=64, T=5, n_ts=5, C=5, Bs=6, Bt=4, wscale="trained", lr=2e-3)
_F32 = dict(arch="resnet18", fc_dim=32, C=5, Bs=5, Bt=4, wscale="trained", lr=2e-3)
CASES = {
    # no pooling (one frame per step), padded videos in the last batch, later steps
    "tiny_rnn_lstm_T5": dict(_T5, rnn_cell="LSTM", place_adv=("N", "Y", "Y"), steps=3, short_last=(5, 3), wseed=41, xseed=401),
    "tiny_rnn_gru_T5": dict(_T5, rnn_cell="GRU", place_adv=("N", "Y", "Y"), steps=3, short_last=(5, 3), wseed=42, xseed=402),
    # len_ts 2 on 8 frames: the last frame repeated twice; place_adv[0] = Y: the video-level loss counted twice
    "tiny_rnn_lstm_T8": dict(_F32, rnn_cell="LSTM", T=8, n_ts=5, place_adv=("Y", "Y", "Y"), steps=2, wseed=43, xseed=403),
    # len_ts 1 on 7 frames: frames 5 and 6 dropped - no frame discriminator, so their rows of gZ1 are exactly zero
    "tiny_rnn_gru_T7": dict(_F32, rnn_cell="GRU", T=7, n_ts=5, place_adv=("N", "Y", "N"), steps=2, wseed=44, xseed=404),
    # half to even: round(2.5) = 2 (truncate to 4 frames), round(3.5) = 4 (repeat up to 8)
    "tiny_rnn_lstm_half5": dict(_F32, rnn_cell="LSTM", T=5, n_ts=2, place_adv=("N", "Y", "Y"), steps=1, wseed=45, xseed=405),
    "tiny_rnn_lstm_half7": dict(_F32, rnn_cell="LSTM", T=7, n_ts=2, place_adv=("N", "Y", "Y"), steps=1, wseed=46, xseed=406),
    # one step, one window of 5: weight_hh's gradient is exactly 0, weight decay and momentum still move it
    "tiny_rnn_lstm_ts1": dict(_F32, rnn_cell="LSTM", T=5, n_ts=1, place_adv=("N", "Y", "Y"), steps=2, wseed=47, xseed=407),
    # rows not 32-byte aligned; every slot past the third a repeat of the last frame
    "tiny_rnn_gru_odd": dict(arch="resnet18", fc_dim=20, T=3, n_ts=5, C=7, Bs=5, Bt=4, wscale="trained", lr=2e-3, rnn_cell="GRU",
                             place_adv=("N", "Y", "Y"), steps=2, wseed=48, xseed=408),
    # use_target none: no flag at all on the general builder
    "tiny_rnn_lstm_src": dict(_T5, rnn_cell="LSTM", steps=2, wseed=49, xseed=409),
    # the weighted and labelled loss paths
    "tiny_rnn_gru_sv_wcls": dict(_T5, rnn_cell="GRU", place_adv=("N", "Y", "Y"), steps=2, short_last=(5, 3), wseed=50, xseed=410,
                                 use_target="Sv", class_counts=(40, 2, 9, 21, 4)),
    # several tiles per launch; K = n_ts B = 320 in the recurrent weight gradients
    "mid_rnn_lstm": dict(arch="resnet18", fc_dim=128, T=5, n_ts=5, C=12, Bs=40, Bt=24, wscale="trained", lr=2e-3, rnn_cell="LSTM",
                         place_adv=("N", "Y", "Y"), steps=2, wseed=51, xseed=411),
    "mid_rnn_gru": dict(arch="resnet18", fc_dim=128, T=5, n_ts=5, C=12, Bs=40, Bt=24, wscale="trained", lr=2e-3, rnn_cell="GRU",
                        place_adv=("N", "Y", "Y"), steps=2, wseed=52, xseed=412),
    # validation on another segment count: a second plan, len_ts 5
    "tiny_rnn_eval": dict(_F32, rnn_cell="LSTM", T=5, n_ts=5, val_T=25, place_adv=("N", "Y", "Y"), steps=1, wseed=53, xseed=413),
}

if __name__ == "__main__":
    for nm in sys.argv[1:] or list(CASES) + ["rnn_init", "rnn_slots_golden"]:
        if nm == "rnn_init":
            run_init(nm)
        elif nm == "rnn_slots_golden":
            run_slots(nm)
        else:
            run_case(nm, CASES[nm])
