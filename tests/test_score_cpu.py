"""Score-only plans (TA3N_FLAG_SCORE_ONLY, include/ta3n_hip.h) on the CPU: the parameter layout is the training plan's, the launch list
holds only what the class logits depend on, the list executed with numpy plus the float64 restatement of the score kernel
(tests/score_reference.py) lands on the forwards the reference recorded, and everything that is not built is refused by name."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_reference as sr
from plan_interp import BASE_WS, EPI_DROP_I, EPI_DROP_V, PH_GEMM, PH_POOL_AVG_FWD, PH_RNN_CELL_FWD, PH_RNN_POOL_FWD, PH_TEMCONV_FWD, Interp, plan_arrays
from ta3n_amd import _lib, tolerances as tol

TA3N_ERR_INVALID = -1      # include/ta3n_hip.h
ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
# (fixture whose tiny shape is used, flags of the training configuration, plan keywords)
LAYOUT_CASES = {
    "trn-m TransAttn": ("tiny_T5", sr.ALL_FLAGS, {}),
    "trn-m no attention": ("tiny_T5", ADV, {}),
    "avgpool source-only": ("tiny_avgpool", 0, {}),
    "avgpool adversarial": ("tiny_avgpool", _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME, {}),
    "rnn LSTM": ("tiny_rnn_eval", None, dict(rnn_cell=0)),
    "rnn GRU": ("tiny_rnn_eval", None, dict(rnn_cell=1)),
    "temconv": ("tiny_tc_eval", None, {}),
}


def _plans(key):
    name, flags, over = LAYOUT_CASES[key]
    _, c, kw, _ = sr.case(name)
    kw = dict(kw, **over)
    return c, sr.train_plan(c, kw, flags=flags), sr.score_plan(c, kw, flags=flags)


@pytest.mark.parametrize("key", list(LAYOUT_CASES))
def test_score_plan_has_the_training_plans_parameter_layout_and_a_smaller_workspace(key):
    c, train, score = _plans(key)
    assert score.params == train.params                       # names, order, offsets, shapes, live
    assert score.param_floats == train.param_floats and score.live_floats == train.live_floats
    assert score.live_ranges == train.live_ranges
    assert score.ws_floats < train.ws_floats
    assert score.description["config"]["Bs"] + score.description["config"]["Bt"] == c["Bs"] + c["Bt"]      # the capacity
    assert not score.has_fused_step
    for name in ("Hf", "Pf", "Hv", "Pv", "Vd", "ones", "loss_part", "norm_part", "sumsq"):
        assert name not in score.regions, name
    assert not [r for r in score.regions if r.startswith("g")]      # no gradient region
    for name in ("F1", "V", "Y", "prob", "rank", "pred", "ce", "metrics", "confusion", "labels"):
        assert name in score.regions, name
    assert ("attn" in score.regions) == key.startswith("trn-m")


def _region_of(plan, off):
    return next(n for n, (o, size) in plan.regions.items() if o <= off < o + max(size, 1))


@pytest.mark.parametrize("key", list(LAYOUT_CASES))
def test_launch_list_holds_only_what_the_logits_depend_on(key):
    _, train, score = _plans(key)
    segs, tasks, phases, geom, _, _ = plan_arrays(score)
    assert all(ph.group == 0 for ph in phases)
    kinds = [ph.kind for ph in phases]
    assert set(kinds) <= set(Interp.LAUNCH)                    # launch kinds of today's enum only
    written = set()
    for ph in phases:
        if ph.kind != PH_GEMM:
            continue
        for t in tasks[ph.task_begin:ph.task_begin + ph.task_count]:
            if t.seg_count == 0:                               # (a filler of the tile order: computes nothing)
                continue
            assert t.c_base == BASE_WS
            assert not (t.epi & (EPI_DROP_I | EPI_DROP_V))     # no dropout epilogue
            written.add(_region_of(score, t.c_off))
    assert not written & {"Hf", "Pf", "Hv", "Pv"} and not [r for r in written if r.startswith("g")]
    if key == "trn-m TransAttn":
        assert kinds == [PH_GEMM] * 3 and written == {"F1", "Zr", "Hr"}
    elif key == "trn-m no attention":
        assert kinds == [PH_GEMM] * 2 and written == {"F1", "Zr"} and "Hr" not in score.regions
    elif key.startswith("avgpool"):
        assert kinds == [PH_GEMM, PH_POOL_AVG_FWD] and written == {"F1"}
    elif key.startswith("rnn"):
        assert kinds == [PH_GEMM, PH_RNN_POOL_FWD, PH_GEMM] + [PH_GEMM, PH_RNN_CELL_FWD] * 5 and written == {"F1", "rnn_Gx", "rnn_Gh"}
    else:
        assert kinds == [PH_GEMM, PH_TEMCONV_FWD] and written == {"F1"}
    n_train = sum(1 for ph in train.description["phases"] if ph["group"] == 0)
    assert len(phases) <= n_train and (len(phases) < n_train or key == "avgpool source-only")      # (that one's training forward is two launches too)


def _check_forward(g, out, Bs, B, prefix="fwd"):
    for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
        g.check(f"{prefix}/out_{dom}", out["Y"][sl], 0, tol.LOGIT_ATOL)
        g.check(f"{prefix}/feat_{dom}_v", out["V"][sl], tol.F32_RTOL, tol.F32_ATOL)
        attn = out["attn"][sl] if out["attn"] is not None else out["V"][sl][:, 0]      # (elsewhere the reference returns the placeholder V[:, 0], models.py:627-628)
        g.check(f"{prefix}/attn_{dom}", attn, tol.F32_RTOL, tol.F32_ATOL)


@pytest.mark.parametrize("name", ["tiny_T2", "tiny_T3", "tiny_T5", "tiny_T9", "tiny_avgpool"])
def test_score_plan_reproduces_the_references_forward_on_the_host(name):
    """Source and target rows as one list of videos on a plan of that capacity, against the recorded forward (dropout 0: the eval forward)."""
    g, c, kw, state_of = sr.case(name)
    plan = sr.score_plan(c, kw)
    x, labels = sr.first_batch(c)
    out = sr.run_plan(plan, state_of({n: s for n, _, s, _ in plan.params}), x, labels.numpy())
    _check_forward(g, out, c["Bs"], c["Bs"] + c["Bt"])
    assert np.allclose(out["prob"].sum(1), 1.0) and out["rank"].max() < c["C"]
    assert np.array_equal(out["rank"] == 0, out["pred"] == labels.numpy())      # nothing tied in these logits


@pytest.mark.parametrize("name", ["tiny_rnn_eval", "tiny_tc_eval"])
def test_score_plan_at_the_validation_segment_count_reproduces_the_recorded_eval_pass(name):
    """Trained on 5 segments, validated on 25: a score plan of its own on the same parameters (main.validate's call, main.py:707)."""
    g, c, kw, state_of = sr.case(name)
    xv, yv, val_T = sr.eval_batch(g, c)
    plan = sr.score_plan(c, kw, T=val_T, capacity=c["Bs"])
    assert plan.params == sr.train_plan(c, kw).params          # the training plan's layout at the training segment count
    out = sr.run_plan(plan, state_of({n: s for n, _, s, _ in plan.params}), xv, yv.numpy())
    g.check("eval/out_t", out["Y"], 0, tol.LOGIT_ATOL)
    g.check("eval/feat_t_v", out["V"], tol.F32_RTOL, tol.F32_ATOL)


def test_restatement_of_the_score_rules_orders_ties_by_class_index():
    y = np.array([[0, 0, 0, 0], [3, 1, 1, 3], [1, 2, 2, 0], [5, 5, 4, 4]], np.float64)
    lab = np.array([2, 3, 2, 0])
    r = sr.score_rows(y, lab)
    assert r["rank"].tolist() == [2, 1, 1, 0] and r["pred"].tolist() == [0, 0, 1, 0]
    want = torch.nn.functional.cross_entropy(torch.from_numpy(y), torch.from_numpy(lab), reduction="none").numpy()
    assert np.allclose(r["ce"], want, rtol=1e-12, atol=1e-12)
    assert np.allclose(r["prob"], torch.softmax(torch.from_numpy(y), 1).numpy(), rtol=1e-12, atol=1e-12)
    for i in range(4):      # torch.topk's own order agrees on rows without ties at the label
        if (y[i] == y[i, lab[i]]).sum() == 1:
            assert int((torch.from_numpy(y[i]).topk(4)[1] == lab[i]).nonzero()[0, 0]) == r["rank"][i]
    m = sr.score_metrics(y, lab)
    assert (m["hits1"], m["hits5"], m["n"]) == (1, 4, 4) and m["confusion"][2, 0] == 1 and m["confusion"][2, 1] == 1 and m["confusion"].sum() == 4


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(flags=sr.ALL_FLAGS, agg=_lib.AGG_TRN_M, **kw):
    with pytest.raises(ValueError) as e:
        _lib.Plan(6, 0, 5, 64, 32, 5, flags | _lib.FLAG_SCORE_ONLY, num_bottleneck=64, aggregation=agg, **kw)
    return str(e.value)


@pytest.mark.parametrize("flag,name", [(_lib.FLAG_BN_SHARED, "TA3N_FLAG_BN_SHARED"), (_lib.FLAG_BF16_MFMA, "TA3N_FLAG_BF16_MFMA"),
                                       (_lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, "TA3N_FLAG_BF16_MFMA"), (_lib.FLAG_BF16_STORE, "TA3N_FLAG_BF16_STORE"),
                                       (_lib.FLAG_F32_SPLIT, "TA3N_FLAG_F32_SPLIT"), (_lib.FLAG_FRAME_ATTN, "TA3N_FLAG_FRAME_ATTN"),
                                       (_lib.FLAG_CLASS_WEIGHTS, "TA3N_FLAG_CLASS_WEIGHTS")])
def test_flags_that_are_not_built_are_refused_by_name(flag, name):
    msg = _refused(sr.ALL_FLAGS | flag)
    assert f"TA3N_FLAG_SCORE_ONLY with {name}" in msg and msg.endswith("is not built")


def test_other_refusals_name_what_is_not_built():
    assert "TA3N_FLAG_SCORE_ONLY with TA3N_FLAG_GENERAL_ATTN (use_attn general) is not built" in _refused(ADV | _lib.FLAG_GENERAL_ATTN)
    assert "TA3N_FLAG_SCORE_ONLY with shared_fc_layers (--add_fc) 2 is not built" in _refused(shared_fc_layers=2)
    assert "TA3N_FLAG_SCORE_ONLY with wgrads_late is not built" in _refused(wgrads_late=1)
    assert "TA3N_FLAG_SCORE_ONLY with phase_tiles is not built" in _refused(phase_tiles=[114])
    assert "TA3N_FLAG_SCORE_ONLY with chain is not built" in _refused(chain=1)
    assert "TA3N_FLAG_SCORE_ONLY with split_k is not built" in _refused(split_k=2)
    assert "TA3N_FLAG_SCORE_ONLY with layout_flags is not built" in _refused(ADV, layout_flags=sr.ALL_FLAGS)
    for nb in (192, 1024):      # widths a training plan takes and the score kernel is not instantiated for
        with pytest.raises(ValueError, match=f"TA3N_FLAG_SCORE_ONLY with num_bottleneck {nb} is not built: 64, 128, 256 or 512"):
            _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS | _lib.FLAG_SCORE_ONLY, num_bottleneck=nb)
        _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS, num_bottleneck=nb)
    for nb in (64, 128, 256, 512):
        _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS | _lib.FLAG_SCORE_ONLY, num_bottleneck=nb)
    _lib.Plan(6, 0, 5, 64, 32, 5, _lib.FLAG_SCORE_ONLY, num_bottleneck=192, aggregation=_lib.AGG_AVGPOOL)      # (avgpool: the width is fc_dim)
    with pytest.raises(ValueError) as e:       # share_params N needs rows of both domains: the training plan's own check comes first
        _lib.Plan(6, 4, 5, 64, 32, 5, sr.ALL_FLAGS | _lib.FLAG_UNSHARED | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)
    assert "TA3N_FLAG_SCORE_ONLY with TA3N_FLAG_UNSHARED (share_params N) is not built" in str(e.value)


def test_the_training_plans_checks_come_first_with_their_own_messages():
    for flags, agg in ((sr.ALL_FLAGS, _lib.AGG_AVGPOOL), (_lib.FLAG_ATTN_ENTROPY, _lib.AGG_TRN_M), (_lib.FLAG_BF16_MFMA, _lib.AGG_RNN)):
        with pytest.raises(ValueError) as want:
            _lib.Plan(6, 0, 5, 64, 32, 5, flags, num_bottleneck=64, aggregation=agg)
        assert _refused(flags, agg) == str(want.value)
    assert "TA3N_FLAG_SCORE_ONLY" not in _refused(sr.ALL_FLAGS, _lib.AGG_AVGPOOL)


def test_accepted_flags_change_the_layout_only():
    base = _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)
    for extra in (_lib.FLAG_FEATURE_GRADS, _lib.FLAG_MCD, _lib.FLAG_MCD | _lib.FLAG_FEATURE_GRADS):
        p = _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS | extra | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)
        assert p.regions == base.regions and [ph["kind"] for ph in p.description["phases"]] == [ph["kind"] for ph in base.description["phases"]]
        assert p.params == _lib.Plan(6, 0, 5, 64, 32, 5, sr.ALL_FLAGS | extra, num_bottleneck=64).params
    both = _lib.Plan(6, 4, 5, 64, 32, 5, ADV | _lib.FLAG_TARGET_LABELS | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)      # (target labels need target rows)
    assert both.params == _lib.Plan(6, 4, 5, 64, 32, 5, ADV, num_bottleneck=64).params
    ent = _lib.Plan(6, 4, 5, 64, 32, 5, ADV | _lib.FLAG_TARGET_ENTROPY | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)
    assert ent.regions == both.regions


def test_entry_points_check_their_arguments_and_their_plan_without_a_device():
    L = _lib.lib()
    score = _lib.Plan(6, 4, 5, 64, 32, 5, sr.ALL_FLAGS | _lib.FLAG_SCORE_ONLY, num_bottleneck=64)
    train = _lib.Plan(6, 4, 5, 64, 32, 5, sr.ALL_FLAGS, num_bottleneck=64)
    buf = (C.c_float * 64)()
    a = C.addressof(buf)

    def call(plan=score, x=a, params=a, ws=a, n=3):
        return L.ta3n_score(plan.handle, x, params, ws, n, 0, None)
    assert call(x=None) == TA3N_ERR_INVALID and b"null" in L.ta3n_last_error()
    assert call(params=None) == TA3N_ERR_INVALID and call(ws=None) == TA3N_ERR_INVALID
    assert call(plan=train) == TA3N_ERR_INVALID and b"TA3N_FLAG_SCORE_ONLY" in L.ta3n_last_error()
    for bad in (-1, 11):      # the capacity is batch_source + batch_target = 10
        assert call(n=bad) == TA3N_ERR_INVALID and b"n_videos" in L.ta3n_last_error()
    assert call(x=a + 4) == TA3N_ERR_INVALID and b"aligned" in L.ta3n_last_error()
    hy = _lib.Hyper()
    refusals = [
        ("ta3n_set_hyper", L.ta3n_set_hyper(score.handle, a, C.byref(hy), None)),
        ("ta3n_loss", L.ta3n_loss(score.handle, a, None)),
        ("ta3n_backward", L.ta3n_backward(score.handle, a, a, a, a, None)),
        ("ta3n_train_step", L.ta3n_train_step(score.handle, a, a, a, a, None)),
        ("ta3n_train_step_range", L.ta3n_train_step_range(score.handle, a, a, a, a, 0, 1, None)),
        ("ta3n_train_step_after_update", L.ta3n_train_step_after_update(score.handle, a, a, a, a, a, 0, 1e-3, 0.9, 1e-4, 20.0, C.byref(hy), None)),
        ("ta3n_train_steps", L.ta3n_train_steps(score.handle, a, a, a, a, a, 0, 1e-3, 0.9, 1e-4, 20.0, C.byref(hy), 1, None, None, None, None, None)),
        ("ta3n_eval_metrics", L.ta3n_eval_metrics(score.handle, a, 1, 1, None)),
        ("ta3n_sgd_step", L.ta3n_sgd_step(score.handle, a, a, a, a, None)),
        ("ta3n_sgd_step_fused", L.ta3n_sgd_step_fused(score.handle, a, a, a, a, None)),
        ("ta3n_sgd_range", L.ta3n_sgd_range(score.handle, a, a, a, a, 0, 4, 0, 1e-3, 0.9, 1e-4, 20.0, None)),
        ("ta3n_sgd_live", L.ta3n_sgd_live(score.handle, a, a, a, a, 0, 1e-3, 0.9, 1e-4, 20.0, None)),
        ("ta3n_sgd_step_next", L.ta3n_sgd_step_next(score.handle, a, a, a, a, 0, 1e-3, 0.9, 1e-4, 20.0, C.byref(hy), None)),
        ("Adam", L.ta3n_adam_range(score.handle, a, a, a, a, a, 0, 4, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 20.0, 1, None)),
    ]
    for fn, rc in refusals:
        assert rc == TA3N_ERR_INVALID, fn
    assert L.ta3n_loss(score.handle, a, None) == TA3N_ERR_INVALID
    msg = L.ta3n_last_error().decode()
    assert msg.startswith("ta3n_loss") and "TA3N_FLAG_SCORE_ONLY" in msg
    assert L.ta3n_num_phases(score.handle, 0) > 0 and all(L.ta3n_num_phases(score.handle, k) == 0 for k in (1, 2, 3, 4, 5))


def test_scorer_refuses_what_is_not_built_with_the_librarys_sentence():
    from ta3n_amd import Scorer
    from ta3n_amd.models import VideoModel
    kw = dict(num_segments=5, feature_dim=64, fc_dim=32, num_class=5, capacity=4)
    for flags, what in ((sr.ALL_FLAGS | _lib.FLAG_BN_SHARED, "use_bn"), (sr.ALL_FLAGS | _lib.FLAG_UNSHARED, "share_params N"),
                        (sr.ALL_FLAGS | _lib.FLAG_FRAME_ATTN, "use_attn_frame"), (ADV | _lib.FLAG_GENERAL_ATTN, "use_attn general"),
                        (sr.ALL_FLAGS | _lib.FLAG_BF16_MFMA, "BF16_MFMA"), (sr.ALL_FLAGS | _lib.FLAG_F32_SPLIT, "F32_SPLIT"),
                        (sr.ALL_FLAGS | _lib.FLAG_CLASS_WEIGHTS, "weighted class loss")):
        with pytest.raises(NotImplementedError, match="TA3N_FLAG_SCORE_ONLY with .*is not built") as e:
            Scorer(flags=flags, **kw)
        assert what in str(e.value)
    with pytest.raises(NotImplementedError, match="use_attn general"):
        Scorer(use_attn="general", **kw)
    for add_fc in (2, 3):
        with pytest.raises(NotImplementedError, match=rf"shared_fc_layers \(--add_fc\) {add_fc} is not built"):
            Scorer(add_fc=add_fc, **kw)
    model = VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=32, use_bn="AdaBN", verbose=False)
    with pytest.raises(NotImplementedError, match="use_bn"):
        Scorer.from_model(model, capacity=4)
    model = VideoModel(5, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=32, verbose=False)
    with pytest.raises(ValueError, match="train_segments"):
        Scorer.from_model(model, capacity=4, num_segments=7)
    s = Scorer.from_model(model, capacity=4)      # built without a device; the plan lies on the model's layout
    assert s.plan.params == model._plan(1, 1).params and s.capacity == 4


def test_scorer_checks_labels_on_the_host():
    from ta3n_amd.scoring import Scorer
    s = Scorer(5, 64, 32, 5, capacity=4)
    x = torch.zeros(3, 5, 64)
    for bad in ([0, 5, 1], [-1, 0, 0]):
        with pytest.raises(ValueError, match=r"labels must be in \[0, 5\)"):
            s.score(x, torch.tensor(bad))
    with pytest.raises(ValueError, match="labels"):
        s.score(x, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="data must be"):
        s.score(torch.zeros(3, 4, 64), torch.tensor([0, 1, 2]))
