"""--frame_aggregation rnn (reference models.py:202-215, 392-422) on the CPU: the slot table against the reference's own pooling, the
TA3N_AGG_RNN plan executed with numpy against the fixtures the reference wrote (tests/golden/make_golden_rnn.py), every refusal by
message, the state_dict and a checkpoint round trip.  (tiny_rnn_gru_sv_wcls - class weights in the loss launch, which the interpreter
does not model - and tiny_rnn_eval's second plan run on the GPU: tests/test_gpu_rnn.py.)"""
import io

import numpy as np
import pytest
import torch

import rnn_reference as rr
from golden_util import GOLDEN_DIR, step_schedule
from plan_interp import (PH_GEMM, PH_POOL_AVG_BWD, PH_POOL_AVG_FWD, PH_RNN_CELL_BWD, PH_RNN_CELL_FWD, PH_RNN_POOL_BWD, PH_RNN_POOL_FWD, Interp,
                         plan_arrays)
from ta3n_amd import _lib, tolerances as tol
from ta3n_amd.models import VideoModel
from test_plan_cpu import make_hyper

INTERP_FIXTURES = [n for n in rr.FIXTURES if n != "tiny_rnn_gru_sv_wcls"]


def test_slot_table_is_the_reference_pooling():
    """ta3n_rnn_slots against the window maxima the reference's aggregate_frames produced on a ramp, for T 1..64 and n_ts 1..8, as
    integers; where the reference raised (len_ts == 0) the function refuses with a message that names n_ts."""
    want = np.load(GOLDEN_DIR + "/rnn_slots_golden.npz")["window_max"]
    refused = 0
    for T in range(1, 65):
        for n_ts in range(1, 9):
            if want[T, n_ts, 0] < 0:
                with pytest.raises(ValueError, match=f"n_ts {n_ts} with {T} segments"):
                    _lib.rnn_slots(T, n_ts)
                refused += 1
                continue
            len_ts, frames = _lib.rnn_slots(T, n_ts)
            assert len_ts == round(T / n_ts) and len(frames) == len_ts * n_ts
            got = [max(frames[j * len_ts:(j + 1) * len_ts]) + 1 for j in range(n_ts)]
            assert got == list(want[T, n_ts, :n_ts]), (T, n_ts)
            assert frames == [min(s, T - 1) for s in range(len_ts * n_ts)]
    assert refused == 16
    assert _lib.rnn_slots(5, 2)[0] == 2 and _lib.rnn_slots(7, 2)[0] == 4      # half to even
    for bad in ((0, 5), (65, 5), (5, 0), (5, 129)):
        with pytest.raises(ValueError):
            _lib.rnn_slots(*bad)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", INTERP_FIXTURES)
def test_plan_reproduces_reference_on_cpu(name, fused):
    g, c = rr.setup(name)
    T, B, Bs = c["T"], c["Bs"] + c["Bt"], c["Bs"]
    plan = rr.make_plan(c)
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(rr.state_of(shapes, c))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = rr.step_batch(c, st)
        it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:] = labels.numpy()
        it.hy = make_hyper(c, st, T, st["lr"])
        it.hy.update(rr.normalisers(c, st), beta=c["beta"], gamma=0.0)
        it.G[:] = 0
        if fused:
            it.run_group(4)
        else:
            it.run_group(0); it.run_group(1); it.run_group(2)
        if s == 0:
            geo = it.g
            outs = dict(out=it.r(geo.o_Y, (B, c["C"])), vid=it.r(geo.o_Pv, (B, 2)), frm=it.r(geo.o_Pf, (B, T, 2)), v=it.r(geo.o_V, (B, geo.F)),
                        f1=it.r(geo.o_F1, (B, T, geo.F)))
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", outs["out"][sl], 0, tol.LOGIT_ATOL)
                g.check(f"fwd/feat_{dom}_v", outs["v"][sl], tol.F32_RTOL, tol.F32_ATOL)
                g.check(f"fwd/feat_{dom}_f1", outs["f1"][sl], tol.F32_RTOL, tol.F32_ATOL)
                g.check(f"fwd/attn_{dom}", outs["v"][sl][:, 0], tol.F32_RTOL, tol.F32_ATOL)      # the placeholder V[:, 0] (models.py:628-629)
                if c["place_adv"] and (c["place_adv"][1] == "Y" or c["place_adv"][0] == "Y"):
                    g.check(f"fwd/pd_{dom}_vid", outs["vid"][sl], 0, tol.LOGIT_ATOL)
                    g.check(f"fwd/pd_{dom}_rel", outs["vid"][sl], 0, tol.LOGIT_ATOL)
                if c["place_adv"] and c["place_adv"][2] == "Y":
                    g.check(f"fwd/pd_{dom}_frm", outs["frm"][sl], 0, tol.LOGIT_ATOL)
        raw = it.get_params(it.G)
        if name == "tiny_rnn_lstm_ts1":
            assert not raw["rnn.weight_hh_l0"].any()                            # one step from the zero state: exactly 0, and live
        if c["rnn_cell"] == "LSTM":
            assert np.array_equal(raw["rnn.bias_ih_l0"], raw["rnn.bias_hh_l0"])
        if name == "tiny_rnn_gru_T7":                                           # frames 5 and 6 are in no window, no frame discriminator
            assert not it.r(it.g.o_gZ1, (B, T, it.g.F))[:, 5:, :].any()
        it.run_group(3, fused_norm=fused)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", new[k], tol.F32_RTOL, tol.F32_ATOL)
    if name == "tiny_rnn_lstm_ts1":                                             # ... weight decay and momentum still move it
        assert not np.array_equal(new["rnn.weight_hh_l0"], rr.state_of(shapes, c)["rnn.weight_hh_l0"].numpy())


def test_launch_list_is_the_tempooling_list_with_the_aggregator_replaced():
    g, c = rr.setup("tiny_rnn_lstm_T8")
    kinds = lambda plan, grp: [ph.kind for ph in plan_arrays(plan)[2] if ph.group == grp]
    rnn = rr.make_plan(c)
    avg = _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], c["flags"], aggregation=_lib.AGG_AVGPOOL)
    n = c["n_ts"]
    fwd = [PH_RNN_POOL_FWD, PH_GEMM] + [PH_GEMM, PH_RNN_CELL_FWD] * n
    bwd = [PH_RNN_CELL_BWD, PH_GEMM] * (n - 1) + [PH_RNN_CELL_BWD, PH_GEMM, PH_RNN_POOL_BWD]
    for grp in (0, 2, 4):
        want = []
        for k in kinds(avg, grp):
            want += fwd if k == PH_POOL_AVG_FWD else bwd if k == PH_POOL_AVG_BWD else [k]
        assert kinds(rnn, grp) == want
    steps = [ph.task_begin for ph in plan_arrays(rnn)[2] if ph.group == 4 and ph.kind in (PH_RNN_CELL_FWD, PH_RNN_CELL_BWD)]
    assert steps == list(range(n)) + list(range(n - 1, -1, -1))
    names = [p[0] for p in rnn.params]
    assert [p[0] for p in rnn.params if p[3]][-4:] == ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"]
    assert not any(nm.startswith("bn_") for nm in names)
    assert rr.make_plan(c, flags=0).live_floats > 0                              # no flag at all: the same builder


FLAG_REFUSALS = [(_lib.FLAG_BF16_MFMA, "TA3N_FLAG_BF16_MFMA"), (_lib.FLAG_BF16_STORE, "TA3N_FLAG_BF16_STORE"), (_lib.FLAG_F32_SPLIT, "TA3N_FLAG_F32_SPLIT"),
                 (_lib.FLAG_MCD, "TA3N_FLAG_MCD"), (_lib.FLAG_BN_SHARED, "TA3N_FLAG_BN_SHARED"), (_lib.FLAG_TRANS_ATTN, "TA3N_FLAG_TRANS_ATTN"),
                 (_lib.FLAG_ATTN_ENTROPY | _lib.FLAG_ADV_RELATION, "TA3N_FLAG_ATTN_ENTROPY"), (_lib.FLAG_TARGET_ENTROPY, "TA3N_FLAG_TARGET_ENTROPY"),
                 (_lib.FLAG_FRAME_ATTN, "TA3N_FLAG_FRAME_ATTN"), (_lib.FLAG_GENERAL_ATTN, "TA3N_FLAG_GENERAL_ATTN"), (_lib.FLAG_UNSHARED, "TA3N_FLAG_UNSHARED")]


def _plan(flags=_lib.FLAG_ADV_VIDEO, T=5, **kw):
    kw.setdefault("n_ts", 5)
    return _lib.Plan(6, 4, T, 512, 64, 5, flags, aggregation=_lib.AGG_RNN, **kw)


@pytest.mark.parametrize("flag,word", FLAG_REFUSALS)
def test_plan_create_refuses_flags_by_name(flag, word):
    with pytest.raises(ValueError, match=r"TA3N_AGG_RNN \(frame_aggregation rnn\) with " + word):
        _plan(_lib.FLAG_ADV_VIDEO | flag)


@pytest.mark.parametrize("kw,word", [(dict(shared_fc_layers=2), "shared_fc_layers"), (dict(chain=1), "chain"), (dict(split_k=2), "split_k"),
                                     (dict(wgrads_late=1), "wgrads_late"), (dict(phase_tiles=[222]), "phase_tiles"),
                                     (dict(layout_flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME), "layout_flags"),
                                     (dict(rnn_cell=2), "rnn_cell must be 0"), (dict(rnn_cell=-1), "rnn_cell must be 0"),
                                     (dict(n_ts=-1), "n_ts must not be negative"), (dict(T=2, n_ts=5), "n_ts 5 with 2 segments")])
def test_plan_create_refuses_options_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        _plan(**kw)


def test_plan_defaults_and_other_aggregations():
    assert _plan(n_ts=0).regions["rnn_Xp"][1] == 5 * 10 * 64                    # n_ts 0 means 5
    assert _plan(rnn_cell=1).regions["rnn_Gx"][1] == 5 * 10 * 3 * 64
    with pytest.raises(ValueError, match="aggregation must be TA3N_AGG_TRN_M or TA3N_AGG_AVGPOOL"):
        _lib.Plan(6, 4, 5, 512, 64, 5, 0, aggregation=3)
    plain = _lib.Plan(6, 4, 5, 512, 64, 5, _lib.FLAG_ADV_VIDEO, aggregation=_lib.AGG_AVGPOOL)
    same = _lib.Plan(6, 4, 5, 512, 64, 5, _lib.FLAG_ADV_VIDEO, aggregation=_lib.AGG_AVGPOOL, rnn_cell=1, n_ts=3)      # ignored elsewhere
    assert plain.description == same.description and not any(k.startswith("rnn_") for k in plain.regions)


def _model(cell="LSTM", **kw):
    kw = dict(dict(train_segments=5, val_segments=5, base_model="resnet18", fc_dim=32, use_attn="none", verbose=False, rnn_cell=cell), **kw)
    return VideoModel(7, "video", "rnn", "RGB", **kw)


@pytest.mark.parametrize("kw,word", [(dict(use_attn="TransAttn"), "frame_aggregation='rnn' with use_attn"), (dict(rnn_cell="RNN"), "rnn_cell='RNN'"),
                                     (dict(n_rnn=2), "n_rnn=2"), (dict(n_directions=2), "n_directions=2"), (dict(n_ts=0), "n_ts=0"),
                                     (dict(use_bn="AdaBN"), "use_bn='AdaBN' with frame_aggregation='rnn'"),
                                     (dict(ens_DA="MCD"), "ens_DA='MCD' with frame_aggregation='rnn'"), (dict(add_fc=2), "add_fc=2 with frame_aggregation='rnn'"),
                                     (dict(share_params="N"), "share_params='N' with frame_aggregation='rnn'"),
                                     (dict(use_attn_frame="TransAttn"), "use_attn_frame='TransAttn' with frame_aggregation='rnn'")])
def test_video_model_refuses_by_name(kw, word):
    with pytest.raises(NotImplementedError) as e:
        _model(**kw)
    assert word in str(e.value)


def _args(extra):
    from ta3n_amd.opts import parser
    return parser.parse_args(["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "rnn"] + extra)


def test_validate_options():
    import train_ddp
    ok = ["--use_attn", "none", "--add_loss_DA", "none"]
    train_ddp.validate_options(_args(ok), module_path=True)
    train_ddp.validate_options(_args(ok + ["--rnn_cell", "GRU", "--n_ts", "3", "--val_segments", "25"]), module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(_args(ok), module_path=False)
    assert "--frame_aggregation rnn (built: trn-m, avgpool) (built on main.py)" in str(e.value)
    for extra, word in ((["--use_attn", "TransAttn"], "--frame_aggregation rnn: frame_aggregation='rnn' with use_attn"),
                        (ok + ["--n_rnn", "2"], "--frame_aggregation rnn: n_rnn=2"), (ok + ["--n_directions", "2"], "--frame_aggregation rnn: n_directions=2"),
                        (ok + ["--use_bn", "AdaBN"], "--frame_aggregation rnn: use_bn='AdaBN'"), (ok + ["--ens_DA", "MCD"], "--frame_aggregation rnn: ens_DA='MCD'"),
                        (ok + ["--add_fc", "2"], "--frame_aggregation rnn: add_fc=2"), (ok + ["--share_params", "N"], "--frame_aggregation rnn: share_params='N'"),
                        (ok + ["--num_segments", "2", "--n_ts", "5"], "n_ts=5 with 2 segments"),
                        (ok + ["--n_ts", "7", "--val_segments", "3"], "n_ts=7 with 3 segments")):
        with pytest.raises(SystemExit) as e:
            train_ddp.validate_options(_args(extra), module_path=True)
        assert word in str(e.value), (extra, str(e.value))


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_state_dict_is_the_reference_one_after_construction(cell):
    """Keys in the reference's order - rnn.*, bn_before_rnn.*, bn_after_rnn.* between fc_classifier_domain.* and fc_feature_video_* - and,
    constructed under torch.manual_seed(1), every tensor bit for bit (rnn_init.npz: the reference's own state_dict)."""
    z = np.load(GOLDEN_DIR + "/rnn_init.npz")
    torch.manual_seed(1)
    sd = _model(cell).state_dict()
    keys = [str(k) for k in z[f"{cell}/keys"]]
    assert list(sd.keys()) == keys
    i = keys.index("fc_classifier_domain.bias")
    assert keys[i + 1:i + 5] == ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"]
    assert keys[i + 5:i + 15] == [f"{m}.{k}" for m in ("bn_before_rnn", "bn_after_rnn")
                                  for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert keys[i + 15].startswith("fc_feature_video_source")
    for k in keys:
        assert np.array_equal(sd[k].numpy(), z[f"{cell}/state/{k}"]), k
    g, _ = rr.setup("tiny_rnn_lstm_T5" if cell == "LSTM" else "tiny_rnn_gru_T5")
    assert list(sd.keys()) == [str(k) for k in g.meta("state_keys")]


def test_checkpoint_round_trip():
    """What torch.save writes from the model loads into a fresh one and into torch's own modules (the reference's checkpoint layout:
    {'state_dict': ...} with the reference's keys), and back."""
    torch.manual_seed(3)
    a = _model("GRU")
    buf = io.BytesIO()
    torch.save({"state_dict": a.state_dict()}, buf)
    buf.seek(0)
    sd = torch.load(buf)["state_dict"]
    b = _model("GRU")
    assert not torch.equal(b.rnn.weight_hh_l0, a.rnn.weight_hh_l0)
    b.load_state_dict(sd)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    ref = torch.nn.GRU(32, 32, 1, batch_first=True)
    ref.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")})
    bn = torch.nn.BatchNorm2d(1)
    bn.load_state_dict({k[len("bn_before_rnn."):]: v for k, v in sd.items() if k.startswith("bn_before_rnn.")})
    back = dict(sd)
    back.update({"rnn." + k: v + 1 for k, v in ref.state_dict().items()})
    b.load_state_dict(back)
    assert torch.equal(b.rnn.bias_hh_l0, a.rnn.bias_hh_l0 + 1)
    with pytest.raises(NotImplementedError):      # the default use_attn is TransAttn: still refused
        VideoModel(12, "video", "rnn", "RGB", verbose=False)


@pytest.mark.parametrize("name", ["tiny_rnn_lstm_T8", "tiny_rnn_gru_T5", "tiny_rnn_gru_sv_wcls", "tiny_rnn_lstm_src"])
def test_float64_restatement_matches_the_reference(name):
    """tests/rnn_reference.py (what the GPU tests compare with where no fixture exists) against the reference's first recorded step."""
    g, c = rr.setup(name)
    st = step_schedule(c)[0]
    xs, xt, labels = rr.step_batch(c, st)
    plan = rr.make_plan(c)
    state = rr.state_of({n: s for n, _, s, _ in plan.params}, c)
    fwd, grads, _ = rr.step(state, torch.cat((xs, xt)), labels, c["Bs"], st["n_src"], st["n_tgt"], c["rnn_cell"], c["n_ts"],
                            c["place_adv"] or ("N", "N", "N"), beta=c["beta"], class_w=c["class_w"], target_labels=c["use_target"] == "Sv")
    g.check("fwd/out_s", fwd["Y"][:c["Bs"]], 1e-5, 1e-6)
    g.check("fwd/feat_t_v", fwd["V"][c["Bs"]:], 1e-5, 1e-6)
    live = set(str(k) for k in g.meta("live"))
    assert {k for k, v in grads.items() if k in live or bool(v.any())} == live
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for k, v in grads.items() if k in live)))
    coef = min(c["clip"] / (total + 1e-6), 1.0)
    for k in sorted(live):
        assert g.rel_l2(f"step0/clipped_grad/{k}", grads[k] * coef) <= 1e-5, k
