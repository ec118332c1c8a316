#!/usr/bin/env python
"""What scoring costs at the headline shape: 202 videos x 5 segments, resnet101 features (D 2048), fc_dim 512, 12 classes, fp32, for the
four frame aggregations.  In one run, per aggregation:
  - ta3n_amd.Scorer.score() of the 202 videos on a score-only plan of capacity 202 (TA3N_FLAG_SCORE_ONLY), and the bare ta3n_score call;
  - the way to score them on a training engine: two TrainEngine(128, 74, ...).evaluate_batch calls (128 + 74 videos; trn-m and avgpool, the
    aggregations the engine is built for);
  - the loop body of test_models.py at --bS 64: VideoModel.forward on the clip fed to both halves, softmax, top-k and
    the confusion counts in torch with a copy to the host per batch (four batches, the last one padded).
One resident batch; warm-up, then `steps` calls between two HIP events (the test_models.py loop: a host clock around calls that end in a
copy to the host), best of `repeats`.  Reported: microseconds per 202 videos, videos per second, launches of the library per call (the
copies torch makes around them are not counted), workspace floats of the plans, and the score plan's launches each timed by itself
(ta3n_time_phases) with the score kernel as the difference to the bare call.  One JSON line per row, then the table.

    python tools/time_score.py [--steps 200] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ta3n_amd import _lib  # noqa: E402
from ta3n_amd.engine import TrainEngine  # noqa: E402
from ta3n_amd.models import VideoModel  # noqa: E402
from ta3n_amd.scoring import Scorer  # noqa: E402
from ta3n_amd.synthetic import synth_batch  # noqa: E402

Bs, Bt, T, D, FC, NC = 128, 74, 5, 2048, 512, 12
N = Bs + Bt
BS_TESTER = 64


def best_of_events(fn, steps, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / steps)
    return best * 1e3      # microseconds


def best_of_clock(fn, steps, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / steps)
    return best * 1e6


def model_of(agg):
    m = VideoModel(NC, "video", agg, "RGB", train_segments=T, val_segments=T, base_model="resnet101", fc_dim=FC, dropout_i=0.0, dropout_v=0.0,
                   use_attn="TransAttn" if agg == "trn-m" else "none", verbose=False).cuda()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():      # weights of a trained model's size (fan-in scaled), so that the logits are no near-ties
        for p in m.parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / float(p.shape[-1]) ** 0.5)
    m.eval()
    return m


def tester_loop(m, data, labels):
    """The loop body of test_models.py (lines :96-113 of this repository's) over the resident clips, in batches of BS_TESTER."""
    kmax = 5
    hits = torch.zeros(3, dtype=torch.long)
    confusion = torch.zeros(kmax, NC, NC, dtype=torch.long)
    for first in range(0, N, BS_TESTER):
        d, lab = data[first:first + BS_TESTER], labels[first:first + BS_TESTER]
        n = d.size(0)
        if n < BS_TESTER:
            d = torch.cat((d, torch.zeros(BS_TESTER - n, T, D, device=d.device)))
        with torch.no_grad():
            _, _, _, _, _, attn, out, _, _, _ = m(d, d, [0, 0, 0], 0, is_train=False, reverse=False)
        prob = torch.nn.Softmax(dim=1)(out[:n]).cpu()
        pred = prob.topk(kmax)[1]
        for j, t in enumerate((1, 3, 5)):
            hits[j] += (pred[:, :t] == lab[:, None]).sum()
        for k in range(kmax):
            confusion[k].index_put_((lab, pred[:, k]), torch.ones(n, dtype=torch.long), accumulate=True)
        attn[:n].detach().cpu()
    return hits


def rows_for(agg, steps, repeats):
    xs, xt, ys, yt = synth_batch(NC, T, D, Bs, Bt, seed=1234)
    data, labels = torch.cat((xs, xt)).cuda(), torch.cat((ys, yt))
    m = model_of(agg)
    rows = []
    # the scorer on the model's parameters
    s = Scorer.from_model(m, capacity=N)
    score = lambda: s.score(data, labels, reset=True)
    for _ in range(10):
        score()
    us = best_of_events(score, steps, repeats)
    P, L = s._params(), _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bare = lambda: _lib.check(L.ta3n_score(s.plan.handle, s.X.data_ptr(), P.data_ptr(), s.ws.data_ptr(), N, 1, st()), "ta3n_score")
    us_bare = best_of_events(bare, steps, repeats)
    cap = 64
    ms, kind, group = (C.c_float * cap)(), (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n_ph = _lib.check(L.ta3n_time_phases(s.plan.handle, s.X.data_ptr(), P.data_ptr(), None, None, s.ws.data_ptr(), st(), 50, ms, kind, group, cap),
                      "ta3n_time_phases")
    launches_us = [round(1e3 * ms[i], 2) for i in range(n_ph)]
    res = s.results()
    rows.append(dict(agg=agg, path="Scorer.score (score-only plan, capacity 202)", us=round(us, 1), videos_per_s=round(N / us * 1e6), launches=n_ph + 1,
                     ws_floats=s.plan.ws_floats, bare_ta3n_score_us=round(us_bare, 1), launch_kinds=[kind[i] for i in range(n_ph)] + ["score"],
                     launches_us=launches_us + [round(us_bare - sum(launches_us), 2)], prec1=round(res["prec1"], 3)))
    # the training engine's evaluate_batch (the engine is built for trn-m and avgpool)
    if agg in ("trn-m", "avgpool"):
        eng = TrainEngine(Bs, Bt, T, D, FC, NC, aggregation=agg)
        eng.load_state(m.state_dict())
        dl = labels.cuda()

        def evaluate():
            eng.evaluate_batch(data[:Bs], dl[:Bs], reset=True)
            eng.evaluate_batch(data[Bs:], dl[Bs:])
        for _ in range(10):
            evaluate()
        us_e = best_of_events(evaluate, steps, repeats)
        ev = eng.eval_results()
        rows.append(dict(agg=agg, path="TrainEngine(128, 74).evaluate_batch x 2", us=round(us_e, 1), videos_per_s=round(N / us_e * 1e6),
                         launches=2 * (L.ta3n_num_phases(eng.plan.handle, 0) + 2), ws_floats=eng.plan.ws_floats, prec1=round(ev["prec1"], 3)))
        del eng
    else:
        rows.append(dict(agg=agg, path="TrainEngine.evaluate_batch", us=None, note="the engine is not built for this aggregation"))
    # test_models.py's loop body
    for _ in range(3):
        hits = tester_loop(m, data, labels)
    us_t = best_of_clock(lambda: tester_loop(m, data, labels), max(steps // 8, 5), repeats)
    plan = m._plan(BS_TESTER, BS_TESTER, T)
    rows.append(dict(agg=agg, path="test_models.py loop (VideoModel.forward, --bS 64) x 4", us=round(us_t, 1), videos_per_s=round(N / us_t * 1e6),
                     launches=4 * L.ta3n_num_phases(plan.handle, 0), ws_floats=plan.ws_floats, prec1=round(100.0 * float(hits[0]) / N, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps(dict(shape=dict(videos=N, T=T, D=D, fc_dim=FC, C=NC), arithmetic="fp32", steps=a.steps, repeats=a.repeats,
                          library=_lib.lib().ta3n_version().decode())), flush=True)
    table = []
    for agg in ("trn-m", "avgpool", "rnn", "temconv"):
        for r in rows_for(agg, a.steps, a.repeats):
            print(json.dumps(r), flush=True)
            table.append(r)
    print(f"\n{'aggregation':<9} {'path':<54} {'us / 202 videos':>16} {'videos / s':>12} {'launches':>9} {'ws_floats':>11}")
    for r in table:
        if r["us"] is None:
            print(f"{r['agg']:<9} {r['path']:<54} {'-':>16} {'-':>12} {'-':>9} {'-':>11}   ({r['note']})")
            continue
        print(f"{r['agg']:<9} {r['path']:<54} {r['us']:>16.1f} {r['videos_per_s']:>12d} {r['launches']:>9d} {r['ws_floats']:>11d}")
    for r in table:
        if "launches_us" in r:
            print(f"{r['agg']}: bare ta3n_score {r['bare_ta3n_score_us']} us; its launches, each timed by itself (kind: us): " +
                  ", ".join(f"{k}: {u}" for k, u in zip(r["launch_kinds"], r["launches_us"])))


if __name__ == "__main__":
    main()
