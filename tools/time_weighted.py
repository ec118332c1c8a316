#!/usr/bin/env python
"""Per-step time of the fused step at the headline shape (resnet101 features, fc_dim 512, 128 + 74 videos x 5 segments, TA3N, bf16 MFMA
operands read from bf16 twins) with the weighted criteria (--weighted_class_loss Y --weighted_class_loss_DA Y: TrainEngine class_weights /
domain_weights) and without them, in the same run: one resident batch, 100 steps in one ta3n_train_steps call, timed with HIP events on
the launch stream, best of 3 repeats.  One JSON line per configuration.

    python tools/time_weighted.py [--steps 100] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd.engine import TrainEngine  # noqa: E402
from ta3n_amd.synthetic import synth_batch, synth_state  # noqa: E402


def time_config(weighted: str, steps: int, repeats: int) -> dict:
    Bs, Bt, T, D, F, C = 128, 74, 5, 2048, 512, 12
    class_w = [1.0 / ((1 + (5 * c) % C) / 78.0) for c in range(C)] if weighted in ("class", "both") else None      # 1 / freq of 1 .. 12 videos per class
    domain_w = (1.0 / 1438, 1.0 / 840) if weighted in ("domain", "both") else None
    eng = TrainEngine(Bs, Bt, T, D, F, C, bf16=True, bf16_store=True, class_weights=class_w, domain_weights=domain_w)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=7))
    xs, xt, ys, _ = synth_batch(C, T, D, Bs, Bt, seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.refresh_bf16(x=True)
    sched = [([0.75, 0.75, 0.5], 0.003, 1e-4)] * steps
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
    return dict(weights=weighted, arithmetic="bf16", ms_per_step=round(best, 4), steps=steps, repeats=repeats, describe=eng.describe())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for weighted in ("none", "both", "class", "domain", "none"):      # (the unweighted step first and last: the drift of the run)
        print(json.dumps(time_config(weighted, a.steps, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
