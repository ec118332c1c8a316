"""GPU: the validation path - TrainEngine.evaluate_batch() -> ta3n_eval_metrics -> eval_results(), the numbers train_ddp.validate()
reports and selects its best checkpoint by (main.validate, main.py:669-761).

A1  eval_metrics_kernel alone, logits written straight into the "Y" region, against a float64 restatement with the explicit tie rule
    (the lower class index wins): every wave through one, two and three loop trips, ties, C = 63 / 64, wide logits, accumulation
    over calls, the argument checks.
A2  validation under use_bn on the reference's own recorded eval pass (model(xs0, xs0) scored on the target branch, main.py:707):
    all Bs rows of the fixtures' eval/out_t and eval/feat_t_v, and the metrics of those logits.
A3  the same against the float64 oracle with BatchNorm statistics / affine pairs that differ strongly between the domains, ragged
    batches larger than the target half, fp32 and bf16 arithmetic.
A4  evaluation neither disturbs a pipelined training run nor scores parameters one update behind it.

CE bound (A1, derived from fp32 rounding, not from the kernel): per video the kernel forms y - m, expf, a 64-lane sum, logf, two
subtractions and the running sum - about eight roundings on values up to max|y| + log C, plus the expf / logf error; with a margin
of 64 over those:  |got - ref| <= 64 * 2^-24 * n * (max|y| + log C).  A logit error of at most d per entry moves a video's
cross-entropy by at most 2 d (logsumexp and the label's logit are each 1-Lipschitz in the sup norm): + 2 n d where the logits
themselves are only known to d (A2, A3).

Rows left out of the exact count comparison (A2, A3: a row whose top-1 / top-5 / argmax decision hangs on a logit gap no larger than
the stated margin), measured on the CPU from the fixtures / the oracle for the seeds used here:
A2 (margin 1e-3): 0 of 6 (tiny_adabn), 0 of 4 (tiny_autodial), 0 of 6 (tiny_avgpool_adabn);
A3 (28 rows): 2 at the fp32 margin 2e-3 (7 %), 4 at the bf16 margin 1.19e-2 (14 %) - _A3_EXCLUDED below, asserted in the tests."""
import math

import numpy as np
import pytest
import torch

import oracle.ta3n_oracle as orc
from golden_util import Golden, case_config, step_schedule
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

TA3N_ERR_INVALID = -1      # include/ta3n_hip.h


# ---- the float64 reference (CPU) -------------------------------------------------------------------------------------------------
def ref_metrics(logits, labels):
    """main.validate's bookkeeping in float64 with the kernel's documented tie rule.  Returns per-row arrays and the sums:
    dict(ce [n], top1 [n] bool, top5 [n] bool, pred [n], ce_sum, hits1, hits5, confusion [C, C] int64)."""
    y = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    n, C = y.shape
    if n == 0:
        z = np.zeros(0)
        return dict(ce=z, top1=z.astype(bool), top5=z.astype(bool), pred=z.astype(np.int64), ce_sum=0.0, hits1=0, hits5=0,
                    confusion=np.zeros((C, C), np.int64))
    m = y.max(1)
    lse = m + np.log(np.exp(y - m[:, None]).sum(1))
    ylab = y[np.arange(n), lab]
    idx = np.arange(C)[None, :]
    ahead = ((y > ylab[:, None]) | ((y == ylab[:, None]) & (idx < lab[:, None]))).sum(1)      # the label's rank
    pred = y.argmax(1)                           # numpy: the FIRST index attaining the maximum
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (lab, pred), 1)
    ce = lse - ylab
    return dict(ce=ce, top1=ahead < 1, top5=ahead < 5, pred=pred, ce_sum=float(ce.sum()), hits1=int((ahead < 1).sum()),
                hits5=int((ahead < 5).sum()), confusion=conf)


def ce_bound(n, max_abs, C):
    return 64.0 * 2.0 ** -24 * n * (max_abs + math.log(C))


def decided_rows(logits, labels, margin):
    """Rows whose top-1 hit, top-5 hit and argmax cannot change when every logit moves by less than margin / 2: the label's logit is
    further than `margin` from the best and from the fifth-best of the other classes, and the two largest logits are further apart."""
    y = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    n, C = y.shape
    ylab = y[np.arange(n), lab]
    others = np.where(np.arange(C)[None, :] == lab[:, None], -np.inf, y)
    others = -np.sort(-others, 1)                # descending; the last column is the -inf that stands for the label itself
    ok = np.abs(ylab - others[:, 0]) > margin
    if C - 1 >= 5:                               # with fewer than six classes every row is a top-5 hit whatever the logits
        ok &= np.abs(ylab - others[:, 4]) > margin
    top = -np.sort(-y, 1)
    ok &= (top[:, 0] - top[:, 1]) > margin
    return ok


def check_results(res, logits, labels, ce_tol, margin=None, max_excluded=0.0, what=""):
    """eval_results() of the engine against ref_metrics(logits, labels).  margin None: counts and confusion matrix exactly; else only
    the decided rows are binding (every other row may fall either way) and at most max_excluded of the rows may be undecided."""
    ref = ref_metrics(logits, labels)
    n = len(labels)
    assert res["n"] == n, (what, res["n"], n)
    got_ce = res["loss"] * max(n, 1)
    print(f"{what}: n {n} CE sum got {got_ce:.9g} ref {ref['ce_sum']:.9g} |diff| {abs(got_ce - ref['ce_sum']):.3e} bound {ce_tol:.3e}")
    assert abs(got_ce - ref["ce_sum"]) <= ce_tol, (what, got_ce, ref["ce_sum"], ce_tol)
    got1, got5 = res["prec1"] * max(n, 1) / 100.0, res["prec5"] * max(n, 1) / 100.0
    conf = res["confusion"].numpy().astype(np.int64)
    assert conf.sum() == n, (what, conf.sum())
    if margin is None:
        assert abs(got1 - ref["hits1"]) < 1e-6 and abs(got5 - ref["hits5"]) < 1e-6, (what, got1, ref["hits1"], got5, ref["hits5"])
        assert np.array_equal(conf, ref["confusion"]), what
        return 0
    ok = decided_rows(logits, labels, margin)
    out = int((~ok).sum())
    print(f"{what}: {out} of {n} rows undecided at margin {margin:.3e}")
    assert out <= max_excluded * n, (what, out, n)
    lab = np.asarray(labels, dtype=np.int64)
    lo1, lo5 = int(ref["top1"][ok].sum()), int(ref["top5"][ok].sum())
    assert lo1 - 1e-6 <= got1 <= lo1 + out + 1e-6 and lo5 - 1e-6 <= got5 <= lo5 + out + 1e-6, (what, got1, lo1, got5, lo5, out)
    conf_ok = np.zeros_like(conf)
    np.add.at(conf_ok, (lab[ok], ref["pred"][ok]), 1)
    assert (conf - conf_ok).min() >= 0 and (conf - conf_ok).sum() == out, what
    return out


# ---- A1: the metrics kernel alone ------------------------------------------------------------------------------------------------
A1_BS = 40
_engines = {}


def _metrics_engine(C):
    if C not in _engines:
        _engines[C] = TrainEngine(A1_BS, 2, 3, 64, 32, C)
    return _engines[C]


def _tie_logits(C, seed, rows=A1_BS):
    """Integers of {-2 .. 2} as fp32 (for C >= 12 most rows tie at the label's value and at the maximum); row 0 all zero with label
    0, row 1 with its maximum attained at classes 0 and C - 1 and label C - 1, row 2 with label 0."""
    rng = np.random.default_rng(seed)
    y = rng.integers(-2, 3, size=(rows, C)).astype(np.float32)
    lab = rng.integers(0, C, size=(rows,))
    y[0] = 0.0; lab[0] = 0
    if rows > 1:
        y[1, 0] = y[1, C - 1] = 3.0; lab[1] = C - 1
    if rows > 2:
        lab[2] = 0
    return y, lab


def _wide_logits(C, seed, rows=A1_BS):
    rng = np.random.default_rng(seed)
    return rng.uniform(-80.0, 80.0, size=(rows, C)).astype(np.float32), rng.integers(0, C, size=(rows,))


def _run_metrics(eng, y, lab, n, reset):
    """Rows [0, n) of y / lab into the "Y" region and ws["labels"], rows [n, Bs) filled with what would move every metric if it were
    read (alternately: a huge logit at the label - a top-1 / top-5 hit and a diagonal confusion entry; a huge logit at another class -
    1e4 of cross-entropy, a top-5 hit, an off-diagonal entry), then ta3n_eval_metrics as evaluate_batch calls it."""
    C, Bs = eng.C, eng.Bs
    full = np.zeros((eng.B, C), np.float32)
    labels = np.zeros(eng.B, np.int64)
    full[:n] = y[:n]; labels[:n] = lab[:n]
    for r in range(n, Bs):
        labels[r] = r % C
        full[r] = -1e4
        full[r, labels[r] if (r & 1) else (labels[r] + 1) % C] = 1e4
        full[r, labels[r]] = max(full[r, labels[r]], 0.0)
    eng.region("Y", (eng.B, C)).copy_(torch.from_numpy(full))
    eng.region("labels").view(torch.int32).copy_(torch.from_numpy(labels.astype(np.int32)))
    return eng._L.ta3n_eval_metrics(eng.plan.handle, eng.ws.data_ptr(), int(n), int(reset), eng._stream())


@pytest.mark.parametrize("C", [5, 12, 63, 64])
def test_metrics_kernel_against_float64_reference(C):
    """n = 17 and 40 send waves through a second, 33 and 40 through a third trip of the per-wave loop; 0 and 1 leave waves idle."""
    eng = _metrics_engine(C)
    for n in (0, 1, 16, 17, 33, 40):
        for kind, make in (("ties", _tie_logits), ("wide", _wide_logits)):
            y, lab = make(C, seed=1000 * C + n)
            if kind == "ties" and C >= 12 and n >= 16:      # the case is about ties: most rows must have one at the label's value
                tied = sum(int((y[i] == y[i, lab[i]]).sum() > 1) for i in range(n))
                assert tied > n // 2, (C, n, tied)
            assert _run_metrics(eng, y, lab, n, reset=1) == 0
            max_abs = float(np.abs(y[:n]).max()) if n else 0.0
            check_results(eng.eval_results(), y[:n], lab[:n], ce_bound(n, max_abs, C), what=f"C {C} n {n} {kind}")


@pytest.mark.parametrize("C", [12, 64])
def test_metrics_kernel_accumulates_over_calls_and_resets(C):
    eng = _metrics_engine(C)
    parts = [(_tie_logits(C, 11), 33), (_wide_logits(C, 12), 5), (_tie_logits(C, 13), 17)]
    for i, ((y, lab), n) in enumerate(parts):
        assert _run_metrics(eng, y, lab, n, reset=int(i == 0)) == 0
    y = np.concatenate([p[0][0][:n] for p, n in zip(parts, (33, 5, 17))])
    lab = np.concatenate([p[0][1][:n] for p, n in zip(parts, (33, 5, 17))])
    check_results(eng.eval_results(), y, lab, ce_bound(len(lab), float(np.abs(y).max()), C), what=f"C {C} accumulated")
    assert _run_metrics(eng, parts[0][0][0], parts[0][0][1], 0, reset=1) == 0
    assert eng.region("metrics")[:4].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert int(eng.eval_results()["confusion"].abs().sum()) == 0


def test_metrics_entry_point_refuses_counts_outside_the_source_half():
    """ta3n_eval_metrics: n_videos in [0, batch_source]; anything else returns TA3N_ERR_INVALID and launches nothing."""
    eng = _metrics_engine(12)
    y, lab = _wide_logits(12, 5)
    assert _run_metrics(eng, y, lab, 7, reset=1) == 0
    torch.cuda.synchronize()
    before = eng.ws.clone()
    for bad in (A1_BS + 1, -1):
        assert eng._L.ta3n_eval_metrics(eng.plan.handle, eng.ws.data_ptr(), bad, 1, eng._stream()) == TA3N_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(eng.ws, before)


# ---- A2: the reference's recorded validation pass under use_bn ------------------------------------------------------------------
def _replay_bn_fixture(name):
    """The fixture's trajectory on a fresh engine: the plain train-mode forward, then its steps (as tests/test_gpu_engine_bn.py and
    tests/test_gpu_engine_avgpool_da.py run them).  Returns (engine, fixture, config, xs0, ys0)."""
    g = Golden(name)
    c = case_config(g)
    T, C = c["T"], c["C"]
    if c["agg"] == "avgpool":
        gamma = 0.0
        eng = TrainEngine(c["Bs"], c["Bt"], T, c["D"], c["fc_dim"], C, flags=flags_from_options(place_adv=c["place_adv"], add_loss_DA="none", use_attn="none"),
                          dropout_i=0.0, dropout_v=0.0, clip=c["clip"], aggregation="avgpool", use_bn=c["use_bn"])
    else:
        gamma = 0.003
        eng = TrainEngine(c["Bs"], c["Bt"], T, c["D"], c["fc_dim"], C, dropout_i=0.0, dropout_v=0.0, clip=c["clip"], use_bn=c["use_bn"])
    assert eng.use_bn == c["use_bn"] != "none"
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    xs0, xt0, ys0, _ = synth_batch(C, T, c["D"], c["Bs"], c["Bt"], seed=c["xseed"])
    eng.set_batch(xs0.cuda(), xt0.cuda(), ys0.cuda())
    eng.set_hyper([0.75, 0.75, 0.5], gamma, c["lr"], train=True)
    eng.forward()
    for st in step_schedule(c):
        xs, xt, ys, _ = synth_batch(C, T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step([0.75, 0.75, 0.5], gamma, st["lr"], valid_source=st["n_src"], valid_target=st["n_tgt"])
    return eng, g, c, xs0, ys0


@pytest.mark.parametrize("name", ["tiny_adabn", "tiny_autodial", "tiny_avgpool_adabn"])
def test_validation_under_domain_batchnorm_lands_on_the_reference(name):
    """evaluate_batch() on all Bs fixture videos in one call (tiny_adabn, tiny_avgpool_adabn: more than the target half holds) against
    what the reference recorded for model(xs0, xs0): its target branch, through bn_shared_T."""
    eng, g, c, xs0, ys0 = _replay_bn_fixture(name)
    Bs, C = c["Bs"], c["C"]
    torch.cuda.synchronize()
    run_before, batches_before = eng.bn_running.clone(), eng.bn_batches
    eng.evaluate_batch(xs0.cuda(), ys0.cuda(), reset=True)
    torch.cuda.synchronize()
    o = eng.outputs()
    for key, got in (("eval/out_t", o["out"][:Bs]), ("eval/feat_t_v", o["feat_v"][:Bs])):
        want = torch.from_numpy(g.z[key + "#full"]).float()
        assert want.shape[0] == Bs
        assert torch.allclose(got.cpu().reshape(want.shape), want, rtol=3e-4, atol=3e-4), (key, (got.cpu().reshape(want.shape) - want).abs().max())
    want = g.z["eval/out_t#full"]
    ce_tol = ce_bound(Bs, float(np.abs(want).max()), C) + Bs * 3e-4 * 2
    check_results(eng.eval_results(), want, ys0.numpy(), ce_tol, margin=1e-3, max_excluded=0.10, what=name)
    assert eng.bn_batches == batches_before and torch.equal(eng.bn_running, run_before)


# ---- A3: the float64 oracle, domains that cannot be confused --------------------------------------------------------------------
A3 = dict(Bs=20, Bt=3, T=3, D=64, Fc=32, C=7)
# rows left out of the exact count comparison, measured on the CPU for the seeds below (fp32: margin 2 x LOGIT_ATOL - either of two
# logits may move by LOGIT_ATOL; bf16: margin BF16_REF_LOGIT_REL_RMS x rms of the float64 logits); of 28 rows
_A3_EXCLUDED = {("AdaBN", False): 2, ("AutoDIAL", False): 2, ("AdaBN", True): 4}


def _a3_setup(use_bn):
    cfg = orc.Config(num_class=A3["C"], num_segments=A3["T"], feature_dim=A3["D"], fc_dim=A3["Fc"], dropout_i=0.0, dropout_v=0.0, use_bn=use_bn)
    params = synth_state(orc.param_shapes(cfg), seed=21, scale="trained")
    rng = np.random.default_rng(77)
    F = cfg.feat_dim

    def vec(centre, spread):
        return torch.tensor(centre + spread * rng.uniform(-1.0, 1.0, F), dtype=torch.float32)
    params["bn_shared_S.weight"], params["bn_shared_S.bias"] = vec(1.0, 0.1), vec(0.0, 0.05)
    params["bn_shared_T.weight"], params["bn_shared_T.bias"] = vec(0.5, 0.1), vec(0.2, 0.05)
    running = {"S": (vec(0.0, 0.1), vec(1.0, 0.2)), "T": (vec(0.5, 0.1), vec(4.0, 0.5))}
    state = dict(params)
    for d in "ST":
        state[f"bn_shared_{d}.running_mean"], state[f"bn_shared_{d}.running_var"] = running[d]
    batches = []
    for i, n in enumerate((20, 7, 1)):      # ragged; 20 and 7 are more than the target half (Bt = 3) holds
        xs, _, ys, _ = synth_batch(A3["C"], A3["T"], A3["D"], n, 1, seed=300 + i)
        batches.append((xs, ys))
    return cfg, params, running, state, batches


def _a3_oracle(cfg, params, running, x, domain):
    p64 = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        return orc.forward_domain(p64, x.double(), [0.0, 0.0, 0.0], cfg, domain=domain,
                                  bn_running=tuple(t.double() for t in running[domain]))["out"].numpy()


@pytest.mark.parametrize("use_bn,bf16", [("AdaBN", False), ("AutoDIAL", False), ("AdaBN", True)], ids=["AdaBN", "AutoDIAL", "AdaBN-bf16"])
def test_validation_goes_through_the_target_batchnorm_against_the_oracle(use_bn, bf16):
    cfg, params, running, state, batches = _a3_setup(use_bn)
    want_t = [_a3_oracle(cfg, params, running, x, "T") for x, _ in batches]
    want_s = [_a3_oracle(cfg, params, running, x, "S") for x, _ in batches]
    all_t = np.concatenate(want_t)
    rms = float(np.sqrt((all_t ** 2).mean()))
    logit_tol = tol.BF16_REF_LOGIT_REL_RMS * rms if bf16 else tol.LOGIT_ATOL
    # what the parent commit computed (the source domain's BatchNorm) is far outside the tolerance: this test tells the two apart
    for s, t in zip(want_s, want_t):
        assert np.abs(s - t).max() > 100 * tol.LOGIT_ATOL and np.abs(s - t).max() > 4 * logit_tol, (np.abs(s - t).max(), logit_tol)
    eng = TrainEngine(A3["Bs"], A3["Bt"], A3["T"], A3["D"], A3["Fc"], A3["C"], dropout_i=0.5, dropout_v=0.5, use_bn=use_bn,
                      **(dict(bf16=True, bf16_store=True) if bf16 else {}))
    eng.load_state(state)
    for i, ((x, y), want) in enumerate(zip(batches, want_t)):
        eng.evaluate_batch(x.cuda(), y.cuda(), reset=(i == 0))
        torch.cuda.synchronize()
        got = eng.outputs()["out"][:len(y)].cpu().double().numpy()
        err = np.abs(got - want).max()
        print(f"{use_bn} bf16 {bf16} n {len(y)}: max logit error {err:.3e} (tolerance {logit_tol:.3e}, rms {rms:.3e})")
        assert err <= logit_tol, (i, err, logit_tol)
    labels = np.concatenate([y.numpy() for _, y in batches])
    n = len(labels)
    margin = logit_tol if bf16 else 2 * logit_tol
    ce_tol = ce_bound(n, float(np.abs(all_t).max()), A3["C"]) + n * logit_tol * 2
    out = check_results(eng.eval_results(), all_t, labels, ce_tol, margin=margin, max_excluded=0.25 if bf16 else 0.10,
                        what=f"{use_bn} bf16 {bf16}")
    assert out == _A3_EXCLUDED[(use_bn, bf16)]
    assert eng.bn_batches == 0 and torch.equal(eng.bn_running.cpu(), torch.stack([torch.stack(running[d]) for d in "ST"]))


# ---- A4: evaluation beside a pipelined training run -------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bn", ["none", "AdaBN"])
def test_evaluation_neither_disturbs_nor_lags_pipelined_training(use_bn):
    """train_step_pipelined leaves its update pending.  An evaluation between two such steps must score the parameters WITH that update
    (what an explicit flush() in front of it gives, bit for bit) and leave the run where it would have been without it."""
    cfg = orc.Config(num_class=A3["C"], num_segments=A3["T"], feature_dim=A3["D"], fc_dim=A3["Fc"], use_bn=use_bn)
    params = synth_state(orc.param_shapes(cfg), seed=5, scale="trained")
    steps = [synth_batch(A3["C"], A3["T"], A3["D"], A3["Bs"], A3["Bt"], seed=40 + s) for s in range(3)]
    xv, _, yv, _ = synth_batch(A3["C"], A3["T"], A3["D"], 13, 1, seed=50)

    def run(evaluate, flush_first=False, stop_after_eval=False):
        eng = TrainEngine(A3["Bs"], A3["Bt"], A3["T"], A3["D"], A3["Fc"], A3["C"], use_bn=use_bn)
        assert eng.fused
        eng.load_state(params)
        logits = None
        for s, (xs, xt, ys, _) in enumerate(steps):
            if s == 2 and evaluate:
                if flush_first:
                    torch.cuda.synchronize()
                    before = eng.P.clone()
                    eng.flush()
                    torch.cuda.synchronize()
                    assert not torch.equal(before, eng.P)      # (the pending update is no no-op: the lag would show)
                eng.evaluate_batch(xv.cuda(), yv.cuda(), reset=True)
                torch.cuda.synchronize()
                logits = eng.outputs()["out"][:13].clone()
                if stop_after_eval:
                    return eng, logits
            eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
            eng.train_step_pipelined([0.75, 0.75, 0.5], 0.003, 1e-2)
        eng.flush()
        torch.cuda.synchronize()
        return eng, logits

    with_eval, logits = run(evaluate=True)
    without, _ = run(evaluate=False)
    assert torch.equal(with_eval.P, without.P) and torch.equal(with_eval.M, without.M)
    assert with_eval.step_count == without.step_count == 3
    if use_bn != "none":
        assert torch.equal(with_eval.bn_running, without.bn_running) and with_eval.bn_batches == without.bn_batches == 3
    _, logits_flushed = run(evaluate=True, flush_first=True, stop_after_eval=True)
    assert torch.equal(logits, logits_flushed)
