#!/usr/bin/env python
"""Cost of --optimizer Adam at the headline shape (resnet101 features, fc_dim 512, 128 + 74 videos x 5 segments, TA3N) in bf16 (MFMA
operands read from bf16 twins) on one resident batch, HIP events on the launch stream, best of 3 repeats:
 (a) the Adam update launch alone (ta3n_adam_range over the whole live prefix, norm from the fused step's partials) beside the SGD
     update launch alone (ta3n_sgd_step_fused), `--reps` back-to-back launches each;
 (b) ms per step of train_steps under Adam (ta3n_train_steps_adam: the update is a launch of its own in front of the step) beside SGD
     (ta3n_train_steps: all of the update but the shared frame FC rides in the step's first launch as side workgroups).
One JSON line per measurement.

    python tools/time_adam.py [--steps 100] [--reps 200] [--repeats 3]
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

SHAPE = dict(Bs=128, Bt=74, T=5, D=2048, F=512, C=12)
HYPER = ([0.75, 0.75, 0.5], 0.003, 1e-4)


def engine(optimizer: str) -> TrainEngine:
    s = SHAPE
    eng = TrainEngine(s["Bs"], s["Bt"], s["T"], s["D"], s["F"], s["C"], bf16=True, bf16_store=True, optimizer=optimizer)
    eng.load_state(synth_state({n: sh for n, _, sh, _ in eng.plan.params}, seed=7))
    xs, xt, ys, _ = synth_batch(s["C"], s["T"], s["D"], s["Bs"], s["Bt"], seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.refresh_bf16(x=True)
    return eng


def best_ms(fn, count: int, repeats: int) -> float:
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / count)
    return best


def time_update_launch(optimizer: str, reps: int, repeats: int) -> dict:
    eng = engine(optimizer)
    eng.train_step(*HYPER)                      # gradients and the fused step's norm partials of one real step
    if optimizer == "Adam":
        def launches():
            for k in range(reps):
                eng.adam_range(0, eng.plan.live_floats, HYPER[2], fused_norm=1, step=2 + k)
    else:
        def launches():
            for _ in range(reps):
                eng.sgd_step_fused()
    launches()                                  # warm-up
    torch.cuda.synchronize()
    us = 1e3 * best_ms(launches, reps, repeats)
    torch.cuda.synchronize()
    assert torch.isfinite(eng.P).all()
    n = eng.plan.live_floats
    per_param = 30 if optimizer == "Adam" else 22      # fp32 reads + writes + the 2-byte bf16 twin
    return dict(measurement="update_launch", optimizer=optimizer, us_per_launch=round(us, 2), live_floats=n, bytes_per_parameter=per_param,
                gb_per_s=round(n * per_param / us / 1e3, 1), reps=reps, repeats=repeats)


def time_steps(optimizer: str, steps: int, repeats: int) -> dict:
    eng = engine(optimizer)
    sched = [HYPER] * steps
    eng.train_steps(sched[:10])                 # warm-up (code objects, caches)
    torch.cuda.synchronize()
    ms = best_ms(lambda: eng.train_steps(sched), steps, repeats)
    eng.flush()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.P).all()
    return dict(measurement="train_steps", optimizer=optimizer, ms_per_step=round(ms, 4), steps=steps, repeats=repeats)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for opt in ("SGD", "Adam"):
        res[opt] = time_update_launch(opt, a.reps, a.repeats)
        print(json.dumps(res[opt]), flush=True)
    print(json.dumps(dict(measurement="update_launch_ratio", adam_over_sgd=round(res["Adam"]["us_per_launch"] / res["SGD"]["us_per_launch"], 3),
                          byte_ratio=round(30 / 22, 3), expectation_at_most=1.6)), flush=True)
    for opt in ("SGD", "Adam"):
        res[opt] = time_steps(opt, a.steps, a.repeats)
        print(json.dumps(res[opt]), flush=True)
    print(json.dumps(dict(measurement="train_steps_ratio", adam_over_sgd=round(res["Adam"]["ms_per_step"] / res["SGD"]["ms_per_step"], 3))), flush=True)


if __name__ == "__main__":
    main()
