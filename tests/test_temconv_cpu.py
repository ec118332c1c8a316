"""--frame_aggregation temconv (reference models.py:44-56, 228-243, 654-672) on the CPU: the TA3N_AGG_TEMCONV plan executed with numpy
against the fixtures the reference's own layers wrote (tests/golden/make_golden_temconv.py), every refusal by message, the state_dict
and a checkpoint round trip.  (tiny_tc_sv_wcls - class weights in the loss launch, which the interpreter does not model - and
tiny_tc_eval's second plan run on the GPU: tests/test_gpu_temconv.py.)"""
import io

import numpy as np
import pytest
import torch

import temconv_reference as tr
from golden_util import GOLDEN_DIR, step_schedule
from plan_interp import PH_POOL_AVG_BWD, PH_POOL_AVG_FWD, PH_TEMCONV_BWD, PH_TEMCONV_FWD, PH_TEMCONV_WGRAD, Interp, plan_arrays
from ta3n_amd import _lib, tolerances as tol
from ta3n_amd.models import VideoModel
from test_plan_cpu import make_hyper

INTERP_FIXTURES = [n for n in tr.FIXTURES if n != "tiny_tc_sv_wcls"]
DEAD = ("tcl_5_1.", "tcl_3_2.", "tcl_5_2.", "bn_1_S.", "bn_1_T.", "bn_2_S.", "bn_2_T.", "conv_fusion.")


def _like(ref_key, g, a):
    """a in the shape of the fixture's record (the plan knows tcl_3_1.conv2d.weight as 3 floats, the reference as [1, 1, 3, 1])."""
    k = ref_key + "#full"
    return np.asarray(a).reshape(g.z[k].shape) if k in g.z else a


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", INTERP_FIXTURES)
def test_plan_reproduces_reference_on_cpu(name, fused):
    g, c = tr.setup(name)
    T, B, Bs = c["T"], c["Bs"] + c["Bt"], c["Bs"]
    plan = tr.make_plan(c)
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(tr.state_of(shapes, c))
    live = [n for n, _, _, lv in plan.params if lv]
    assert set(live) == set(str(k) for k in g.meta("live"))
    assert live[-2:] == [tr.W, tr.C0]                                            # the last live parameters
    for s, st in enumerate(step_schedule(c)):
        xs, xt, labels = tr.step_batch(c, st)
        it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:] = labels.numpy()
        it.hy = make_hyper(c, st, T, st["lr"])
        it.hy.update(tr.normalisers(c, st), beta=c["beta"], gamma=0.0)
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
                g.check(f"fwd/attn_{dom}", outs["v"][sl][:, 0], tol.F32_RTOL, tol.F32_ATOL)      # the placeholder V[:, 0], as for avgpool / rnn
                if c["place_adv"] and (c["place_adv"][1] == "Y" or c["place_adv"][0] == "Y"):
                    g.check(f"fwd/pd_{dom}_vid", outs["vid"][sl], 0, tol.LOGIT_ATOL)
                    g.check(f"fwd/pd_{dom}_rel", outs["vid"][sl], 0, tol.LOGIT_ATOL)
                if c["place_adv"] and c["place_adv"][2] == "Y":
                    g.check(f"fwd/pd_{dom}_frm", outs["frm"][sl], 0, tol.LOGIT_ATOL)
        raw = it.get_params(it.G)
        assert raw[tr.W].any() and raw[tr.C0].any()
        it.run_group(3, fused_norm=fused)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", _like(f"step{s}/clipped_grad/{k}", g, raw[k] * coef), 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", _like(f"step{s}/param/{k}", g, new[k]), tol.F32_RTOL, tol.F32_ATOL)


def test_fused_norm_counts_the_temconv_gradients():
    """The fused optimiser's norm is the sum of the "sumsq" slots: the last one holds the four tcl_3_1 gradients' sum of squares."""
    g, c = tr.setup("tiny_tc_T5")
    plan = tr.make_plan(c)
    it = Interp(plan)
    it.set_params(tr.state_of({n: s for n, _, s, _ in plan.params}, c))
    st = step_schedule(c)[0]
    xs, xt, labels = tr.step_batch(c, st)
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:] = labels.numpy()
    it.hy = make_hyper(c, st, c["T"], st["lr"])
    it.hy.update(tr.normalisers(c, st), beta=c["beta"], gamma=0.0)
    it.run_group(4)
    geo = it.g
    slots = it.ws[geo.o_sumsq:geo.o_sumsq + geo.n_sumsq]
    mine = it.get_params(it.G)
    assert np.isclose(slots[-1], (mine[tr.W] ** 2).sum() + (mine[tr.C0] ** 2).sum(), rtol=1e-12) and slots[-1] > 0
    assert np.isclose(slots.sum(), (it.G[:geo.live_floats] ** 2).sum(), rtol=1e-9)


def test_launch_list_is_the_tempooling_list_with_the_aggregator_replaced():
    g, c = tr.setup("tiny_tc_T5")
    kinds = lambda plan, grp: [ph.kind for ph in plan_arrays(plan)[2] if ph.group == grp]
    tc = tr.make_plan(c)
    avg = _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], c["flags"], aggregation=_lib.AGG_AVGPOOL)
    for grp in (0, 1, 2, 3, 4):
        want = [PH_TEMCONV_FWD if k == PH_POOL_AVG_FWD else PH_TEMCONV_BWD if k == PH_POOL_AVG_BWD else k for k in kinds(avg, grp)]
        if grp in (2, 4):
            want.append(PH_TEMCONV_WGRAD)                                        # one small launch of its own, the last of the way back
        assert kinds(tc, grp) == want
    names = [p[0] for p in tc.params]
    assert [p[0] for p in tc.params if p[3]][-2:] == [tr.W, tr.C0]
    assert dict((p[0], p[2]) for p in tc.params)[tr.W] == (3,) and dict((p[0], p[2]) for p in tc.params)[tr.C0] == (1,)
    assert not any(nm.startswith(DEAD) for nm in names)
    assert tc.regions["tc_part"][1] == (c["Bs"] + c["Bt"]) * 4
    assert not any(k.startswith("tc_") for k in avg.regions)                     # an avgpool plan has no tc_* region
    assert tr.make_plan(c, flags=0).live_floats > 0                              # no flag at all: the same builder
    assert tc.live_floats == avg.live_floats + 16                                # two tensors, each padded to 8 floats


FLAG_REFUSALS = [(_lib.FLAG_BF16_MFMA, "TA3N_FLAG_BF16_MFMA"), (_lib.FLAG_BF16_STORE, "TA3N_FLAG_BF16_STORE"), (_lib.FLAG_F32_SPLIT, "TA3N_FLAG_F32_SPLIT"),
                 (_lib.FLAG_MCD, "TA3N_FLAG_MCD"), (_lib.FLAG_BN_SHARED, "TA3N_FLAG_BN_SHARED"), (_lib.FLAG_TRANS_ATTN, "TA3N_FLAG_TRANS_ATTN"),
                 (_lib.FLAG_ATTN_ENTROPY | _lib.FLAG_ADV_RELATION, "TA3N_FLAG_ATTN_ENTROPY"), (_lib.FLAG_TARGET_ENTROPY, "TA3N_FLAG_TARGET_ENTROPY"),
                 (_lib.FLAG_FRAME_ATTN, "TA3N_FLAG_FRAME_ATTN"), (_lib.FLAG_GENERAL_ATTN, "TA3N_FLAG_GENERAL_ATTN"), (_lib.FLAG_UNSHARED, "TA3N_FLAG_UNSHARED")]


def _plan(flags=_lib.FLAG_ADV_VIDEO, T=5, F=64, **kw):
    return _lib.Plan(6, 4, T, 512, F, 5, flags, aggregation=_lib.AGG_TEMCONV, **kw)


@pytest.mark.parametrize("flag,word", FLAG_REFUSALS)
def test_plan_create_refuses_flags_by_name(flag, word):
    with pytest.raises(ValueError, match=r"TA3N_AGG_TEMCONV \(frame_aggregation temconv\) with " + word):
        _plan(_lib.FLAG_ADV_VIDEO | flag)


@pytest.mark.parametrize("kw,word", [(dict(shared_fc_layers=2), "shared_fc_layers"), (dict(chain=1), "chain"), (dict(split_k=2), "split_k"),
                                     (dict(wgrads_late=1), "wgrads_late"), (dict(phase_tiles=[222]), "phase_tiles"),
                                     (dict(layout_flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME), "layout_flags")])
def test_plan_create_refuses_options_by_name(kw, word):
    with pytest.raises(ValueError, match=r"TA3N_AGG_TEMCONV \(frame_aggregation temconv\) with " + word):
        _plan(**kw)


def test_plan_dims_and_other_aggregations():
    assert _lib.AGG_TEMCONV == 4
    for bad in (dict(T=65), dict(F=30)):                                         # avgpool_dims_refusal applies as it is
        with pytest.raises(ValueError):
            _plan(**bad)
    for agg in (3, 7):
        with pytest.raises(ValueError, match="aggregation must be TA3N_AGG_TRN_M or TA3N_AGG_AVGPOOL"):
            _lib.Plan(6, 4, 5, 512, 64, 5, 0, aggregation=agg)
    assert _plan(_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ADV_RELATION | _lib.FLAG_FEATURE_GRADS | _lib.FLAG_TARGET_LABELS |
                 _lib.FLAG_CLASS_WEIGHTS).regions["gV_ext"][1] == 10 * 64


def _model(**kw):
    kw = dict(dict(train_segments=5, val_segments=5, base_model="resnet18", fc_dim=32, use_attn="none", verbose=False), **kw)
    return VideoModel(7, "video", "temconv", "RGB", **kw)


@pytest.mark.parametrize("kw,word", [(dict(use_attn="TransAttn"), "frame_aggregation='temconv' with use_attn"),
                                     (dict(use_attn="general"), "frame_aggregation='temconv' with use_attn"),
                                     (dict(use_bn="AdaBN"), "use_bn='AdaBN' with frame_aggregation='temconv' (the temconv_1 BatchNorm site is not built)"),
                                     (dict(ens_DA="MCD"), "ens_DA='MCD' with frame_aggregation='temconv'"),
                                     (dict(add_fc=2), "add_fc=2 with frame_aggregation='temconv'"),
                                     (dict(share_params="N"), "share_params='N' with frame_aggregation='temconv'"),
                                     (dict(use_attn_frame="TransAttn"), "use_attn_frame='TransAttn' with frame_aggregation='temconv'")])
def test_video_model_refuses_by_name(kw, word):
    with pytest.raises(NotImplementedError) as e:
        _model(**kw)
    assert word in str(e.value)


def test_video_model_refuses_the_frame_baseline_and_the_default_attention():
    with pytest.raises(NotImplementedError, match="baseline_type='frame'"):
        VideoModel(7, "frame", "temconv", "RGB", use_attn="none", verbose=False)
    with pytest.raises(NotImplementedError):      # the default use_attn is TransAttn: still refused
        VideoModel(12, "video", "temconv", "RGB", verbose=False)


def _args(extra):
    from ta3n_amd.opts import parser
    return parser.parse_args(["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "temconv"] + extra)


def test_validate_options():
    import train_ddp
    ok = ["--use_attn", "none", "--add_loss_DA", "none"]
    train_ddp.validate_options(_args(ok), module_path=True)
    train_ddp.validate_options(_args(ok + ["--val_segments", "25", "--use_target", "Sv"]), module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(_args(ok), module_path=False)
    assert "--frame_aggregation temconv (built: trn-m, avgpool) (built on main.py)" in str(e.value)
    for extra, word in ((["--use_attn", "TransAttn"], "--frame_aggregation temconv: frame_aggregation='temconv' with use_attn"),
                        (ok + ["--use_bn", "AdaBN"], "--frame_aggregation temconv: use_bn='AdaBN'"),
                        (ok + ["--ens_DA", "MCD"], "--frame_aggregation temconv: ens_DA='MCD'"),
                        (ok + ["--add_fc", "2"], "--frame_aggregation temconv: add_fc=2"),
                        (ok + ["--share_params", "N"], "--frame_aggregation temconv: share_params='N'"),
                        (ok + ["--use_attn_frame", "TransAttn"], "--frame_aggregation temconv: use_attn_frame='TransAttn'")):
        with pytest.raises(SystemExit) as e:
            train_ddp.validate_options(_args(extra), module_path=True)
        assert word in str(e.value), (extra, str(e.value))


def test_state_dict_is_the_reference_one_after_construction():
    """Keys in the reference's order - tcl_3_1, tcl_5_1, bn_1_S, bn_1_T, tcl_3_2, tcl_5_2, bn_2_S, bn_2_T, conv_fusion between
    fc_classifier_domain.* and fc_feature_video_* - and, constructed under torch.manual_seed(1), every tensor bit for bit
    (temconv_init.npz: the reference's own state_dict)."""
    z = np.load(GOLDEN_DIR + "/temconv_init.npz")
    torch.manual_seed(1)
    sd = _model().state_dict()
    keys = [str(k) for k in z["keys"]]
    assert list(sd.keys()) == keys
    i = keys.index("fc_classifier_domain.bias")
    assert keys[i + 1:i + 5] == ["tcl_3_1.conv2d.weight", "tcl_3_1.conv2d.bias", "tcl_5_1.conv2d.weight", "tcl_5_1.conv2d.bias"]
    assert keys[i + 5] == "bn_1_S.weight" and "conv_fusion.0.bias" in keys
    assert keys[keys.index("conv_fusion.0.bias") + 1].startswith("fc_feature_video_source")
    for k in keys:
        assert sd[k].dtype == torch.from_numpy(z[f"state/{k}"]).dtype and np.array_equal(sd[k].numpy(), z[f"state/{k}"]), k
    assert sd["tcl_3_1.conv2d.weight"].shape == (1, 1, 3, 1) and sd["tcl_5_2.conv2d.weight"].shape == (2, 2, 5, 1)
    for name in tr.FIXTURES:
        assert list(sd.keys()) == [str(k) for k in tr.setup(name)[0].meta("state_keys")]
    assert all(any(k.startswith(d) for k in keys) for d in DEAD)                 # the dead layers are present


def test_checkpoint_round_trip():
    """What torch.save writes from the model loads strictly into a fresh one and into torch's own modules (the reference's checkpoint
    layout: {'state_dict': ...} with the reference's keys), and back."""
    torch.manual_seed(3)
    a = _model()
    buf = io.BytesIO()
    torch.save({"state_dict": a.state_dict()}, buf)
    buf.seek(0)
    sd = torch.load(buf)["state_dict"]
    b = _model()
    assert not torch.equal(b.tcl_3_1.conv2d.weight, a.tcl_3_1.conv2d.weight)
    b.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    ref = torch.nn.Conv2d(1, 1, kernel_size=(3, 1), padding=(1, 0))
    ref.load_state_dict({k[len("tcl_3_1.conv2d."):]: v for k, v in sd.items() if k.startswith("tcl_3_1.conv2d.")})
    bn = torch.nn.BatchNorm1d(32)
    bn.load_state_dict({k[len("bn_1_S."):]: v for k, v in sd.items() if k.startswith("bn_1_S.")})
    back = dict(sd)
    back.update({"tcl_3_1.conv2d." + k: v + 1 for k, v in ref.state_dict().items()})
    b.load_state_dict(back)
    assert torch.equal(b.tcl_3_1.conv2d.bias, a.tcl_3_1.conv2d.bias + 1)
    # a reference-shaped checkpoint of another segment count: the parameters do not depend on T
    c = _model(train_segments=3, val_segments=25)
    c.load_state_dict(sd, strict=True)


def test_synth_temconv_state_scale():
    from ta3n_amd.synthetic import synth_temconv_state
    shapes = {tr.W: (1, 1, 3, 1), tr.C0: (1,), "tcl_5_1.conv2d.weight": (1, 1, 5, 1), "fc_feature_domain.weight": (4, 4)}
    st = synth_temconv_state(shapes, seed=5)
    assert set(st) == {tr.W, tr.C0} and st[tr.W].shape == (1, 1, 3, 1) and st[tr.C0].shape == (1,)
    taps = torch.cat([synth_temconv_state(shapes, seed=s)[tr.W].reshape(-1) for s in range(400)])
    bias = torch.cat([synth_temconv_state(shapes, seed=s)[tr.C0] for s in range(400)])
    assert abs(float(taps.var()) - 2 / 3) < 0.1 and abs(float(bias.var()) - 0.1) < 0.03      # N(0, 2/3): kaiming at fan-in 3; N(0, 0.1)
    assert torch.equal(synth_temconv_state(shapes, seed=5)[tr.W], st[tr.W])


@pytest.mark.parametrize("name", ["tiny_tc_T2", "tiny_tc_T3_direct", "tiny_tc_odd", "tiny_tc_sv_wcls", "tiny_tc_src"])
def test_float64_restatement_matches_the_reference(name):
    """tests/temconv_reference.py (what the GPU tests compare with where no fixture exists) against the reference's first recorded step."""
    g, c = tr.setup(name)
    st = step_schedule(c)[0]
    xs, xt, labels = tr.step_batch(c, st)
    plan = tr.make_plan(c)
    state = tr.state_of({n: s for n, _, s, _ in plan.params}, c)
    fwd, grads, _ = tr.step(state, torch.cat((xs, xt)), labels, c["Bs"], st["n_src"], st["n_tgt"], c["place_adv"] or ("N", "N", "N"),
                            beta=c["beta"], class_w=c["class_w"], target_labels=c["use_target"] == "Sv")
    g.check("fwd/out_s", fwd["Y"][:c["Bs"]], 1e-5, 1e-6)
    g.check("fwd/feat_t_v", fwd["V"][c["Bs"]:], 1e-5, 1e-6)
    live = set(str(k) for k in g.meta("live"))
    assert {k for k, v in grads.items() if k in live or bool(v.any())} == live
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for k, v in grads.items() if k in live)))
    coef = min(c["clip"] / (total + 1e-6), 1.0)
    for k in sorted(live):
        assert g.rel_l2(f"step0/clipped_grad/{k}", grads[k] * coef) <= 1e-5, k
