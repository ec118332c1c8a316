"""GPU: score-only plans (TA3N_FLAG_SCORE_ONLY), ta3n_score and ta3n_amd.Scorer.

S1  the score kernel alone: the V front end on an avgpool plan whose shared layer is the identity, so V, Wcv and bcv are the small
    integers the test writes and the logits are exact; rank, argmax, hits and the confusion matrix against the float64 restatement
    (tests/score_reference.py) exactly, ties included; the CE sum within the bound tests/test_gpu_validation.py derives from fp32
    rounding, 64 * 2^-24 * n * (max|y| + log C); accumulation over calls; the same call twice gives the same bits.
S2  rows at and past n of the input influence nothing.
S3  end to end against the forwards the reference recorded: source and target rows scored as one list, in one call and in two unequal
    calls.  Counts by the decided-rows method of tests/test_gpu_validation.py at margin 2 * LOGIT_ATOL with no row left out (0 rows are
    undecided at that margin in these fixtures: asserted).  trn-m without attention, which has no fixture, against the float64 oracle.
S4  sharing parameters with a TrainEngine (behind a pending pipelined update, without disturbing the run), a VideoModel (an in-place
    change is seen) and scoring straight from a FeatureStore.
S5  score_models.py (test_models.py's command line on the scorer) writes what test_models.py writes.
Every measured figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle.ta3n_oracle as orc
import score_reference as sr
from fixture_t7 import make_dataset
from test_gpu_validation import ce_bound, check_results, decided_rows
from ta3n_amd import Scorer, _lib, tolerances as tol
from ta3n_amd.engine import TrainEngine
from ta3n_amd.feature_store import FeatureStore
from ta3n_amd.models import VideoModel
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_VIDEO = ("V", "Y", "prob", "rank", "pred", "ce")


def _snapshot(s, n, names=PER_VIDEO + ("metrics", "confusion")):
    """Rows [0, n) of the per-video regions, and the accumulated ones, as raw bits."""
    torch.cuda.synchronize()
    out = {}
    for name in names + (("attn",) if "attn" in s.plan.regions else ()):
        t = s.region(name).view(torch.int32)
        out[name] = (t if name in ("metrics", "confusion") else t[: n * (t.numel() // s.capacity)]).cpu().clone()
    return out


def _check_counts(res, Y_ref, labels, ce_tol, what):
    want = sr.score_metrics(Y_ref, labels)
    n = len(labels)
    got_ce = res["loss"] * max(n, 1)
    print(f"{what}: n {n} CE sum got {got_ce:.9g} ref {want['ce_sum']:.9g} |diff| {abs(got_ce - want['ce_sum']):.3e} bound {ce_tol:.3e}")
    assert res["n"] == n
    assert abs(got_ce - want["ce_sum"]) <= ce_tol
    assert round(res["prec1"] * max(n, 1) / 100.0, 6) == want["hits1"] and round(res["prec5"] * max(n, 1) / 100.0, 6) == want["hits5"]
    assert np.array_equal(res["confusion"].numpy().astype(np.int64), want["confusion"])


# ---- S1: the kernel alone ---------------------------------------------------------------------------------------------------------
CAP = 9


def _integer_case(C, F, seed):
    """V [CAP, F] of {0..3}, Wcv [C, F] of {-1, 0, 1} with every third row repeated (ties between classes), bcv = 1.  Row 0 of V is zero:
    all classes tie, label 0; row 1 puts the maximum at classes 0 and C - 1 alone, label C - 1 (a label at a tie: rank 1, argmax 0);
    row 2's label is 0."""
    rng = np.random.default_rng(seed)
    V = rng.integers(0, 4, size=(CAP, F)).astype(np.float32)
    base = rng.integers(-1, 2, size=(3, F)).astype(np.float32)
    W = base[np.arange(C) % 3].copy()
    b = np.ones(C, np.float32)
    lab = rng.integers(0, C, size=CAP)
    V[0] = 0; lab[0] = 0
    W[:, 0] = -1; W[0, 0] = W[C - 1, 0] = 1
    W[C - 1, 1:] = W[0, 1:]
    V[1] = 0; V[1, 0] = 3; lab[1] = C - 1
    lab[2] = 0
    return V, W, b, lab


@pytest.mark.parametrize("F", [4, 36, 64, 516])
@pytest.mark.parametrize("C", [1, 5, 63, 64])
def test_score_kernel_against_the_float64_restatement(C, F):
    T, D = 2, max(F, 64)
    s = Scorer(T, D, F, C, capacity=CAP, aggregation="avgpool")
    V, W, b, lab = _integer_case(C, F, seed=100 * C + F)
    s.load_params({"fc_feature_shared_source.weight": torch.eye(F, D), "fc_feature_shared_source.bias": torch.zeros(F),
                   "fc_classifier_video_source.weight": torch.from_numpy(W), "fc_classifier_video_source.bias": torch.from_numpy(b)})
    x = torch.zeros(CAP, T, D)
    x[:, :, :F] = torch.from_numpy(V)[:, None, :]      # every segment the same row: F1 = relu(x I) = V and the mean is that row, exactly
    Y = sr.classify(V, W, b)
    assert np.array_equal(Y, Y.astype(np.float32)) and np.abs(Y).max() < 2 ** 20      # exact in fp32 whatever the summation order
    if C > 1:
        assert (Y[0] == Y[0, 0]).all() and Y[1, 0] == Y[1, C - 1] == Y[1].max() and (Y[1, 1:C - 1] < Y[1, 0]).all()
    for n in (0, 1, 4, 5, 9):
        s.score(x[:n], torch.from_numpy(lab[:n]), reset=True)
        first = _snapshot(s, n)
        want = sr.score_rows(Y[:n], lab[:n])
        pv = s.per_video()
        assert np.array_equal(pv["logits"].cpu().numpy().astype(np.float64), Y[:n])
        assert np.array_equal(pv["rank"].cpu().numpy(), want["rank"]) and np.array_equal(pv["pred"].cpu().numpy(), want["pred"])
        assert np.array_equal(pv["feat_v"].cpu().numpy(), V[:n])
        err = np.abs(pv["prob"].cpu().numpy().astype(np.float64) - want["prob"]).max() if n else 0.0
        print(f"C {C} F {F} n {n}: max prob error {err:.3e}")
        # expf within 2 ulp on the numerator and on every summand, six levels of rounding in the 64-lane sum, one divide: at most
        # 2 + 2 + 6 + 1 = 11 roundings of 2^-24 on a value <= 1
        assert err <= 16 * 2.0 ** -24
        _check_counts(s.results(), Y[:n], lab[:n], ce_bound(n, float(np.abs(Y[:n]).max()) if n else 0.0, C), f"C {C} F {F} n {n}")
        s.score(x[:n], torch.from_numpy(lab[:n]), reset=True)      # the same call again: the same bits everywhere
        again = _snapshot(s, n)
        assert all(torch.equal(first[k], again[k]) for k in first), [k for k in first if not torch.equal(first[k], again[k])]
    # three calls, reset on the first, count like one call over the union
    parts = [(0, 4), (4, 5), (2, 9)]
    for i, (lo, hi) in enumerate(parts):
        s.score(x[lo:hi], torch.from_numpy(lab[lo:hi]), reset=(i == 0))
    idx = np.concatenate([np.arange(lo, hi) for lo, hi in parts])
    _check_counts(s.results(), Y[idx], lab[idx], ce_bound(len(idx), float(np.abs(Y).max()), C), f"C {C} F {F} accumulated")
    assert s.per_video()["rank"].numel() == len(idx)
    s.score(x[:0], torch.from_numpy(lab[:0]), reset=True)
    assert s.region("metrics")[:4].tolist() == [0.0] * 4 and int(s.results()["confusion"].abs().sum()) == 0


# ---- S2: rows at and past n ---------------------------------------------------------------------------------------------------------
def _fixture_scorer(name, capacity=None, T=None, flags=None):
    g, c, kw, state_of = sr.case(name)
    agg = {v: k for k, v in sr.AGG.items()}[kw["aggregation"]]
    s = Scorer(c["T"] if T is None else T, c["D"], c["fc_dim"], c["C"], capacity=c["Bs"] + c["Bt"] if capacity is None else capacity,
               aggregation=agg, flags=c["flags"] if flags is None else flags, rnn_cell=c.get("rnn_cell", "LSTM"), n_ts=c.get("n_ts", 5))
    state = state_of({n: sh for n, _, sh, _ in s.plan.params})
    s.load_params(state)
    return g, c, s, state


@pytest.mark.parametrize("name,n", [("tiny_T5", 3), ("tiny_avgpool", 3)])
def test_rows_past_n_influence_nothing(name, n):
    g, c, s, _ = _fixture_scorer(name)
    assert s.capacity == 10
    x, labels = sr.first_batch(c)
    runs = []
    for fill in (0.0, float("nan"), 1e30):
        s.score(x[:1], labels[:1], reset=True)      # (allocates the buffers)
        s.X[n * s.T:] = fill
        s.score(x[:n], labels[:n], reset=True)
        runs.append(_snapshot(s, n))
        assert int(s.results()["n"]) == n
    for other in runs[1:]:
        assert all(torch.equal(runs[0][k], other[k]) for k in runs[0]), [k for k in runs[0] if not torch.equal(runs[0][k], other[k])]
    assert torch.isfinite(s.per_video()["logits"]).all()


# ---- S3: end to end against the reference's recorded forwards ------------------------------------------------------------------------
def _check_against_fixture(g, c, s, x, labels, what):
    B, Bs = c["Bs"] + c["Bt"], c["Bs"]
    ref_Y = np.concatenate([g.z["fwd/out_s#full"], g.z["fwd/out_t#full"]]).astype(np.float64)
    lab = labels.numpy()
    ok = decided_rows(ref_Y, lab, 2 * tol.LOGIT_ATOL)
    print(f"{what}: {int((~ok).sum())} of {B} rows undecided at margin {2 * tol.LOGIT_ATOL:.1e}")
    assert ok.all()
    want = sr.score_metrics(ref_Y, lab)
    for split in ((B,), (B // 3, B - B // 3)):      # one call; two unequal calls
        first = 0
        for i, m in enumerate(split):
            s.score(x[first:first + m], labels[first:first + m], reset=(i == 0))
            first += m
        pv = s.per_video()
        for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
            err = g.check(f"fwd/out_{dom}", pv["logits"][sl], 0, tol.LOGIT_ATOL)
            print(f"{what} {dom} calls {len(split)}: max logit error {err:.3e}")
            g.check(f"fwd/feat_{dom}_v", pv["feat_v"][sl], tol.F32_RTOL, tol.F32_ATOL)
            g.check(f"fwd/attn_{dom}", pv["attn"][sl] if pv["attn"] is not None else pv["feat_v"][sl][:, 0], tol.F32_RTOL, tol.F32_ATOL)
        res = s.results()
        n = B
        assert res["n"] == n and round(res["prec1"] * n / 100.0, 6) == want["hits1"] and round(res["prec5"] * n / 100.0, 6) == want["hits5"]
        assert np.array_equal(res["confusion"].numpy().astype(np.int64), want["confusion"])
        # per row, what the margin decides: the top-1 hit, the top-5 hit and the argmax (the exact rank of a label far from the top is not)
        rank, ref_rank = pv["rank"].cpu().numpy(), sr.score_rows(ref_Y, lab)["rank"]
        assert np.array_equal(rank < 1, ref_rank < 1) and np.array_equal(rank < 5, ref_rank < 5) and np.array_equal(pv["pred"].cpu().numpy(), ref_Y.argmax(1))
        ce_tol = ce_bound(n, float(np.abs(ref_Y).max()), c["C"]) + 2 * n * tol.LOGIT_ATOL      # (logits known to LOGIT_ATOL: test_gpu_validation.py)
        print(f"{what}: CE sum {res['loss'] * n:.9g} ref {want['ce_sum']:.9g} bound {ce_tol:.3e}")
        assert abs(res["loss"] * n - want["ce_sum"]) <= ce_tol


@pytest.mark.parametrize("name", ["tiny_T2", "tiny_T3", "tiny_T5", "tiny_T9", "mid_T12", "tiny_avgpool", "tiny_rnn_eval", "mid_rnn_gru"])
def test_scorer_lands_on_the_references_forward(name):
    g, c, s, _ = _fixture_scorer(name)
    x, labels = sr.first_batch(c)
    _check_against_fixture(g, c, s, x, labels, name)


@pytest.mark.parametrize("name", ["tiny_rnn_eval", "tiny_tc_eval"])
def test_scorer_at_the_validation_segment_count(name):
    """Trained on 5 segments, validated on 25: a plan of its own on the same parameters; logits only (tiny_tc_eval: 2 of 5 rows undecided)."""
    g, c, kw, _ = sr.case(name)
    xv, yv, val_T = sr.eval_batch(g, c)
    _, _, s, _ = _fixture_scorer(name, capacity=c["Bs"], T=val_T)
    s.score(xv, yv, reset=True)
    pv = s.per_video()
    err = g.check("eval/out_t", pv["logits"], 0, tol.LOGIT_ATOL)
    print(f"{name} val_T {val_T}: max logit error {err:.3e}")
    g.check("eval/feat_t_v", pv["feat_v"], tol.F32_RTOL, tol.F32_ATOL)


def test_trn_without_attention_lands_on_the_oracle():
    g, c, kw, state_of = sr.case("tiny_T5")
    flags = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
    _, _, s, state = _fixture_scorer("tiny_T5", flags=flags)
    assert "Hr" not in s.plan.regions
    x, labels = sr.first_batch(c)
    cfg = orc.Config(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc_dim"], dropout_i=0.0, dropout_v=0.0,
                     add_loss_DA="none", use_attn="none")
    with torch.no_grad():
        want = orc.forward_domain({k: v.double() for k, v in state.items()}, x.double(), [0.0, 0.0, 0.0], cfg)
    s.score(x, labels, reset=True)
    pv = s.per_video()
    err = float((pv["logits"].cpu().double() - want["out"]).abs().max())
    print(f"trn-m use_attn none: max logit error against the oracle {err:.3e}")
    assert err <= tol.LOGIT_ATOL
    assert float(pv["attn"].abs().max()) == 0.0
    s_attn = _fixture_scorer("tiny_T5")[2]
    s_attn.score(x, labels, reset=True)
    assert float((s_attn.per_video()["logits"] - pv["logits"]).abs().max()) > 100 * tol.LOGIT_ATOL      # the attention is no no-op here


# ---- S4: sharing ------------------------------------------------------------------------------------------------------------------
A = dict(Bs=24, Bt=8, T=4, D=96, Fc=64, C=7)


def test_scorer_on_an_engine_scores_the_updated_parameters_and_leaves_the_run_alone():
    cfg = orc.Config(num_class=A["C"], num_segments=A["T"], feature_dim=A["D"], fc_dim=A["Fc"])
    params = synth_state(orc.param_shapes(cfg), seed=5, scale="trained")
    steps = [synth_batch(A["C"], A["T"], A["D"], A["Bs"], A["Bt"], seed=40 + k) for k in range(2)]
    xv, _, yv, _ = synth_batch(A["C"], A["T"], A["D"], 13, 1, seed=50)

    def run(score):
        eng = TrainEngine(A["Bs"], A["Bt"], A["T"], A["D"], A["Fc"], A["C"])
        eng.load_state(params)
        got = None
        for k, (xs, xt, ys, _) in enumerate(steps):
            if k == 1 and score:
                s = Scorer.from_engine(eng)
                assert s.capacity == A["Bs"] + A["Bt"] and s.plan.params == eng.plan.params and s.plan.ws_floats < eng.plan.ws_floats
                before = eng.P.clone()
                s.score(xv, yv, reset=True)
                torch.cuda.synchronize()
                assert not torch.equal(before, eng.P)      # the pending update was applied first
                got = (s.per_video()["logits"].clone(), s.results())
            eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
            eng.train_step_pipelined([0.75, 0.75, 0.5], 0.003, 1e-2)
        eng.flush()
        torch.cuda.synchronize()
        return eng, got

    with_score, (logits, res) = run(True)
    without, _ = run(False)
    assert torch.equal(with_score.P, without.P) and torch.equal(with_score.M, without.M) and with_score.step_count == without.step_count == 2
    # the parent's path on the same videos and the same (updated) parameters
    eng = TrainEngine(A["Bs"], A["Bt"], A["T"], A["D"], A["Fc"], A["C"])
    eng.load_state(params)
    eng.set_batch(steps[0][0].cuda(), steps[0][1].cuda(), steps[0][2].cuda())
    eng.train_step_pipelined([0.75, 0.75, 0.5], 0.003, 1e-2)
    eng.evaluate_batch(xv.cuda(), yv.cuda(), reset=True)
    torch.cuda.synchronize()
    want = eng.outputs()["out"][:13]
    err = float((logits - want).abs().max())
    print(f"Scorer.from_engine against evaluate_batch: max logit difference {err:.3e}")
    assert err <= 2 * tol.LOGIT_ATOL
    # the scorer's counts against the float64 bookkeeping of the parent path's logits: rows whose decision hangs on a gap below twice the
    # logit bound may fall either way (their number is printed), every other row is binding; the CE sum moves by at most 2 d per row
    wl = want.cpu().double().numpy()
    ce_tol = ce_bound(13, float(np.abs(wl).max()), A["C"]) + 2 * 13 * 2 * tol.LOGIT_ATOL
    check_results(res, wl, yv.numpy(), ce_tol, margin=4 * tol.LOGIT_ATOL, max_excluded=1.0, what="Scorer.from_engine")
    assert eng.eval_results()["n"] == 13


def test_scorer_on_a_model_sees_an_in_place_parameter_change():
    m = VideoModel(A["C"], "video", "trn-m", "RGB", train_segments=A["T"], val_segments=A["T"], base_model="resnet18", fc_dim=A["Fc"],
                   dropout_i=0.0, dropout_v=0.0, verbose=False).cuda()
    sd = synth_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=9, scale="trained")
    m.load_state_dict(sd, strict=False)
    m.eval()
    xv, _, yv, _ = synth_batch(A["C"], A["T"], 512, 11, 1, seed=60)
    s = Scorer.from_model(m, capacity=4)
    s.score(xv, yv, reset=True)
    assert s._params().data_ptr() == m._flat.data_ptr()      # shared, not copied
    with torch.no_grad():
        want = m(xv.cuda(), xv.cuda(), [0, 0, 0], 0, False, False)[6]
    first = s.per_video()["logits"].clone()
    err = float((first - want).abs().max())
    print(f"Scorer.from_model against VideoModel.forward: max logit difference {err:.3e}")
    assert first.shape == (11, A["C"]) and err <= 2 * tol.LOGIT_ATOL
    with torch.no_grad():
        m.fc_classifier_video_source.bias.add_(1.0)
        m.fc_classifier_video_source.bias[0] += 2.0
    s.score(xv, yv, reset=True)
    moved = s.per_video()["logits"] - first
    assert torch.allclose(moved[:, 0], torch.full_like(moved[:, 0], 3.0), atol=1e-5) and torch.allclose(moved[:, 1:], torch.ones_like(moved[:, 1:]), atol=1e-5)


def test_score_store_equals_score_on_the_gathered_batch():
    g, c, s, _ = _fixture_scorer("tiny_T5", capacity=8)
    rng = np.random.default_rng(3)
    nf = torch.from_numpy(rng.integers(3, 12, size=23).astype(np.int32))
    rows = torch.from_numpy(np.abs(rng.standard_normal((int(nf.sum()), c["D"]))).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, c["C"], size=23).astype(np.int32))
    store = FeatureStore.from_tensors(rows, nf.cuda(), labels.cuda())
    ids = torch.from_numpy(rng.permutation(23).astype(np.int32))
    s.score_store(store, ids, reset=True)
    a, res_a = {k: (v.clone() if v is not None else None) for k, v in s.per_video().items()}, s.results()
    feats, lab = store.gather(ids.cuda(), c["T"])
    s.score(feats.cpu(), lab.cpu(), reset=True)
    b, res_b = s.per_video(), s.results()
    assert a["rank"].numel() == 23 and torch.equal(lab.cpu(), labels[ids.long()])
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    assert res_a["loss"] == res_b["loss"] and res_a["prec1"] == res_b["prec1"] and torch.equal(res_a["confusion"], res_b["confusion"]) and res_a["n"] == 23


# ---- S5: score_models.py -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg,use_attn", [("trn-m", "TransAttn"), ("avgpool", "none")])
def test_score_models_writes_what_test_models_writes(agg, use_attn, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import score_models
    import test_models
    data = make_dataset(str(tmp_path / "data"), videos=(1, 1, 12))
    m = VideoModel(5, "video", agg, "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, use_attn=use_attn, verbose=False)
    sd = m.state_dict()
    sd.update(synth_state({k: tuple(v.shape) for k, v in sd.items()}, seed=17, scale="trained"))
    weights = str(tmp_path / "w.pth.tar")
    torch.save({"epoch": 1, "prec1": 0.0, "state_dict": {"module." + k: v for k, v in sd.items()}}, weights)
    out = {}
    for mode in ("plain", "scorer"):
        pre = str(tmp_path / mode)
        argv = [data[0], "RGB", data[3], weights, "--arch", "resnet18", "--test_segments", "5", "--fc_dim", "64", "--baseline_type", "video",
                "--frame_aggregation", agg, "--use_attn", use_attn, "--bS", "5", "-j", "0", "--top", "1", "3", "--save_scores", pre + "_scores",
                "--save_confusion", pre + "_cm", "--save_attention", pre + "_attn"]
        acc = (score_models if mode == "scorer" else test_models).main(argv)
        lines = capsys.readouterr().out.splitlines()
        out[mode] = dict(acc=acc, final=[ln for ln in lines if ln.startswith("Pred@1 ") and "%" in ln][-1],
                         last=[ln for ln in lines if ln.startswith("Pred@1 ") and "sec/video" in ln][-1].split("average")[0],
                         top=open(pre + "_cm-top[1, 3].txt").read(), scores=np.load(pre + "_scores.npy"), attn=np.loadtxt(pre + "_attn.txt"))
        assert os.path.exists(pre + "_cm.png")
    a, b = out["plain"], out["scorer"]
    print(a["final"], "|", b["final"])
    assert a["final"] == b["final"] and a["last"] == b["last"] and a["top"] == b["top"] and a["acc"] == b["acc"]
    assert a["scores"].shape == b["scores"].shape == (12, 5)
    err_s, err_a = np.abs(a["scores"] - b["scores"]).max(), np.abs(a["attn"] - b["attn"]).max()
    print(f"{agg}: max score difference {err_s:.3e}, max attention difference {err_a:.3e}")
    assert err_s <= 1e-5 and a["attn"].shape == b["attn"].shape and err_a <= tol.F32_ATOL


def test_score_models_names_what_it_does_not_build(tmp_path):
    sys.path.insert(0, ROOT)
    import score_models
    data = make_dataset(str(tmp_path / "data"), videos=(1, 1, 2))
    m = VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, use_bn="AdaBN", verbose=False)
    weights = str(tmp_path / "w.pth.tar")
    torch.save({"epoch": 1, "prec1": 0.0, "state_dict": {"module." + k: v for k, v in m.state_dict().items()}}, weights)
    with pytest.raises(SystemExit, match=r"score_models.py: .*TA3N_FLAG_SCORE_ONLY with TA3N_FLAG_BN_SHARED \(use_bn\) is not built"):
        score_models.main([data[0], "RGB", data[3], weights, "--arch", "resnet18", "--test_segments", "5", "--fc_dim", "64", "--baseline_type", "video",
                           "--frame_aggregation", "trn-m", "--use_attn", "TransAttn", "--use_bn", "AdaBN", "--bS", "2", "-j", "0"])
