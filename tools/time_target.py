#!/usr/bin/env python
"""Per-step time of the fused step at the headline shape (resnet101 features, fc_dim 512, 128 + 74 videos x 5 segments, bf16 MFMA operands
read from bf16 twins) plain (uSv, attentive entropy), with --use_target Sv, with --add_loss_DA target_entropy and with both, in the same
run: one resident batch, 100 steps in one ta3n_train_steps call, timed with HIP events on the launch stream, best of 3 repeats.  One JSON
line per configuration.

    python tools/time_target.py [--steps 100] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd.engine import TrainEngine, flags_from_options  # noqa: E402
from ta3n_amd.synthetic import synth_batch, synth_state  # noqa: E402

CONFIGS = {"plain": ("uSv", "attentive_entropy"), "Sv": ("Sv", "attentive_entropy"), "target_entropy": ("uSv", "target_entropy"),
           "Sv+target_entropy": ("Sv", "target_entropy")}


def time_config(name: str, steps: int, repeats: int) -> dict:
    Bs, Bt, T, D, F, C = 128, 74, 5, 2048, 512, 12
    use_target, add_loss_DA = CONFIGS[name]
    eng = TrainEngine(Bs, Bt, T, D, F, C, bf16=True, bf16_store=True, flags=flags_from_options(add_loss_DA=add_loss_DA, use_target=use_target))
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    xs, xt, ys, yt = synth_batch(C, T, D, Bs, Bt, seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda(), target_label=yt.cuda() if eng.target_labels else None)
    eng.refresh_bf16(x=True)
    sched = [([0.75, 0.75, 0.5], 0.3 if eng.target_entropy else 0.003, 1e-4)] * steps
    eng.train_steps(sched[:10])                  # warm-up (code objects, caches)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.train_steps(sched)
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / steps)
    eng.flush()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.P).all()
    return dict(options=name, arithmetic="bf16", ms_per_step=round(best, 4), steps=steps, repeats=repeats, describe=eng.describe())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name in ("plain", "Sv", "target_entropy", "Sv+target_entropy", "plain"):      # (the plain step first and last: the drift of the run)
        print(json.dumps(time_config(name, a.steps, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
