#!/usr/bin/env python
"""Cost of the training meters (TrainEngine(train_meters=True), TA3N_FLAG_TRAIN_METERS) at the headline shape (resnet101 features, fc_dim
512, 128 + 74 videos x 5 segments, TA3N) in bf16 (MFMA operands read from bf16 twins) on one resident batch, HIP events on the launch stream:
 (a) ms per step of train_steps on an engine with the meters and on one without, `--steps` steps after `--warmup`, the two engines
     alternating in one process, best of `--repeats` each;
 (b) the meters launch alone (ta3n_time_phases: `--reps` back-to-back launches between two events), beside the step's other launches.
One JSON line per measurement, then a summary line.

    python tools/time_meters.py [--steps 200] [--warmup 20] [--reps 200] [--repeats 3]
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
PH_TRAIN_METERS = 23


def engine(train_meters: bool) -> TrainEngine:
    s = SHAPE
    eng = TrainEngine(s["Bs"], s["Bt"], s["T"], s["D"], s["F"], s["C"], bf16=True, bf16_store=True, train_meters=train_meters)
    eng.load_state(synth_state({n: sh for n, _, sh, _ in eng.plan.params}, seed=7))
    xs, xt, ys, _ = synth_batch(s["C"], s["T"], s["D"], s["Bs"], s["Bt"], seed=1234)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.refresh_bf16(x=True)
    return eng


def ms_per_step(eng: TrainEngine, steps: int) -> float:
    sched = [HYPER] * steps
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.train_steps(sched)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    engines = {False: engine(False), True: engine(True)}
    best = {False: float("inf"), True: float("inf")}
    runs = {False: [], True: []}
    for eng in engines.values():
        eng.train_steps([HYPER] * a.warmup)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for flagged in (False, True):      # alternating: both see the same clocks and the same neighbours
            ms = ms_per_step(engines[flagged], a.steps)
            runs[flagged].append(round(1e3 * ms, 2))
            best[flagged] = min(best[flagged], ms)
    for flagged in (False, True):
        engines[flagged].flush()
        torch.cuda.synchronize()
        assert torch.isfinite(engines[flagged].P).all()
        print(json.dumps(dict(measurement="train_steps", train_meters=flagged, us_per_step=round(1e3 * best[flagged], 2), runs_us=runs[flagged],
                              steps=a.steps, warmup=a.warmup, repeats=a.repeats)), flush=True)
    assert torch.equal(engines[False].P, engines[True].P)      # the same steps on the same state: the meters move nothing
    m = engines[True].meters()
    phases = engines[True].time_phases(reps=a.reps)
    meters_us = [1e3 * ms for kind, _, _, ms in phases if kind == PH_TRAIN_METERS]
    assert len(meters_us) == 1
    print(json.dumps(dict(measurement="launches", kinds=[k for k, _, _, _ in phases], us=[round(1e3 * ms, 2) for _, _, _, ms in phases],
                          reps=a.reps)), flush=True)
    print(json.dumps(dict(measurement="summary", us_per_step_without=round(1e3 * best[False], 2), us_per_step_with=round(1e3 * best[True], 2),
                          added_us=round(1e3 * (best[True] - best[False]), 2), meters_launch_alone_us=round(meters_us[0], 2),
                          window_steps=m["steps"], prec1=round(m["prec1"], 3), loss=round(m["loss"], 4), acc_domain=m["acc_domain"])), flush=True)


if __name__ == "__main__":
    main()
