"""--use_attn_frame TransAttn (models.py:368-377, 612-614: every frame feature scaled by 1 + (1 - H(frame-discriminator softmax))
in front of the TRN, the weights not detached) on the CPU: the new plans executed with numpy (tests/plan_interp.py)
against fixtures the reference produced (tests/golden/make_golden_frame_attn.py), the launch order, the plans without the flag
left as they were, and the option handling at the plan, TrainEngine, VideoModel, train_ddp.py and main.py levels."""
import os
import sys

import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from plan_interp import PH_FRAME_ATTN_BWD, PH_FRAME_ATTN_FWD, Interp, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import flags_from_options, frame_attn_refusal
from ta3n_amd.synthetic import synth_batch, synth_state
from test_plan_cpu import make_hyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FAF_CASES = ["tiny_faf_T5", "tiny_faf_T2", "tiny_faf_odd", "tiny_faf_advN", "mid_faf", "tiny_faf_wide"]
ALL_FLAGS = (_lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN)
FAF = ALL_FLAGS | _lib.FLAG_FRAME_ATTN
TINY = dict(Bs=6, Bt=4, T=5, D=512, fc_dim=64, C=12)


def faf_flags(c):
    return flags_from_options(c["place_adv"] or ("Y", "Y", "Y"), "attentive_entropy", "TransAttn", "RevGrad", "uSv", use_attn_frame="TransAttn")


def _plan(c, flags, **kw):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags, **kw)


@pytest.mark.parametrize("extra", [0, _lib.FLAG_FEATURE_GRADS], ids=["engine", "module"])
@pytest.mark.parametrize("name", FAF_CASES)
def test_plan_reproduces_reference(name, extra):
    """ta3n_forward / ta3n_loss / ta3n_backward / ta3n_sgd_step of the frame-attention plan against the reference's run of the same
    command: forward tensors and the frame weights, clipped gradients and parameters after every step (the last step of tiny_faf_T5
    with padded videos).  extra = TA3N_FLAG_FEATURE_GRADS: the plan VideoModel builds (no outside gradient: the same numbers)."""
    g = Golden(name)
    c = case_config(g)
    T = c["T"]
    plan = _plan(c, faf_flags(c) | extra)
    assert not plan.has_fused_step
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    live = {n for n, _, _, lv in plan.params if lv}
    assert live == set(str(k) for k in g.meta("live"))
    assert {"fc_feature_domain.weight", "fc_classifier_domain.bias"} <= live      # also with place_adv Y Y N (tiny_faf_advN)
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, yt = synth_batch(c["C"], T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:c["Bs"]] = ys.numpy()
        it.hy = make_hyper(c, st, T, st["lr"])
        it.G[:] = 0
        it.run_group(0)
        if s == 0:
            B, Bs = c["Bs"] + c["Bt"], c["Bs"]
            geo = it.g
            outs = dict(out=it.r(geo.o_Y, (B, c["C"])), attn=it.r(geo.o_attn, (B, T - 1)),
                        rel=it.r(geo.o_Pr, (B, T - 1, 2)), vid=it.r(geo.o_Pv, (B, 2)), frm=it.r(geo.o_Pf, (B, T, 2)),
                        v=it.r(geo.o_V, (B, 256)), f1=it.r(geo.o_F1, (B, T, geo.F)),
                        attn_frame=it.r(plan.region("attn_frame")[0], (B, T)))
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", outs["out"][sl], 5e-5, 2e-5)
                g.check(f"fwd/attn_{dom}", outs["attn"][sl], 5e-5, 2e-5)
                g.check(f"fwd/attn_frame_{dom}", outs["attn_frame"][sl], 5e-5, 2e-5)
                for nm in ("rel", "vid", "frm"):
                    g.check(f"fwd/pd_{dom}_{nm}", outs[nm][sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_v", outs["v"][sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_f1", outs["f1"][sl], 5e-5, 2e-5)      # feat[2] stays un-attended
        it.run_group(1)
        it.run_group(2)
        raw = it.get_params(it.G)
        it.run_group(3)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", new[k], 1e-4, 2e-5)


def test_padded_rows_contribute_no_gradient():
    """Short last batch of tiny_faf_T5: the rows of the padded videos get a weight from whatever their logits hold, and zero in
    the TRN input gradient, the frame logit gradient and the gradient at F1."""
    g = Golden("tiny_faf_T5")
    c = case_config(g)
    T = c["T"]
    plan = _plan(c, FAF)
    it = Interp(plan)
    it.set_params(synth_state({n: s for n, _, s, _ in plan.params}, seed=c["wseed"], scale=c["wscale"]))
    st = step_schedule(c)[-1]
    assert (st["n_src"], st["n_tgt"]) == (5, 3)
    xs, xt, ys, yt = synth_batch(c["C"], T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:c["Bs"]] = ys.numpy()
    it.hy = make_hyper(c, st, T, st["lr"])
    for grp in (0, 1, 2):
        it.run_group(grp)
    B, F = c["Bs"] + c["Bt"], it.g.F
    pad = [5, 9]                                       # the padded source / target video
    assert (it.r(plan.region("attn_frame")[0], (B, T))[pad] != 0).all()
    for name, width in (("gF1a", F), ("gPfT", 2), ("gZ1", F)):
        assert (it.r(plan.region(name)[0], (B, T, width))[pad] == 0).all(), name
    assert (it.r(plan.region("gZ1")[0], (B, T, F))[:5] != 0).any()


def test_launch_order():
    """Forward: F1 | Hf | Pf | frame attention | tuples | Hr | pooling | {Y, Hv} | Pv.  Backward: ... | {TRN weight gradients, gF1a} |
    frame attention | {gHf, dWcd} | {dWfd, gZ1} | dWsh.  The tuple products and the TRN weight gradients read F1a."""
    plan = _plan(TINY, FAF)
    segs, tasks, phases, geo, _, _ = plan_arrays(plan)
    assert [ph.kind for ph in phases if ph.group == 0] == [0, 0, 0, PH_FRAME_ATTN_FWD, 0, 0, 1, 0, 0]
    assert [ph.kind for ph in phases if ph.group == 2] == [0, 0, 3, 0, 0, PH_FRAME_ATTN_BWD, 0, 0, 0]
    assert not any(ph.group in (4, 5) for ph in phases)
    F1, F1a = plan.region("F1"), plan.region("F1a")
    Zr = (geo.o_Zr, geo.o_Zr + plan.region("Zr")[1])

    def reads(t, reg):
        return [s for s in segs[t.seg_begin:t.seg_begin + t.seg_count] for base, off in ((s.a_base, s.a_off), (s.b_base, s.b_off))
                if base == 3 and reg[0] <= off < reg[0] + reg[1]]
    tuple_tasks = [t for t in tasks if t.seg_count and t.c_base == 3 and Zr[0] <= t.c_off < Zr[1]]
    assert tuple_tasks and all(reads(t, F1a) and not reads(t, F1) for t in tuple_tasks)
    fwd = [ph for ph in phases if ph.group == 0]
    first = {name: next(i for i, ph in enumerate(fwd) if ph.kind == 0 and any(tasks[k].c_off == off and tasks[k].c_base == 3
                        for k in range(ph.task_begin, ph.task_begin + ph.task_count)))
             for name, off in (("Pf", geo.o_Pf), ("Zr", geo.o_Zr))}
    assert first["Pf"] < 3 < first["Zr"]              # the logits before the attention launch, the tuples behind it
    # (1 + w) gF1a lands in gRa where it fits and in a region of its own where it does not (T F > (T - 1) 256)
    assert "gF1s" not in plan.regions
    wide = _plan(dict(TINY, T=3, fc_dim=512), FAF)
    assert wide.region("gF1s")[1] == 10 * 3 * 512


@pytest.mark.parametrize("flags", [ALL_FLAGS, ALL_FLAGS | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, ALL_FLAGS | _lib.FLAG_FEATURE_GRADS,
                                   _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_RELATION | _lib.FLAG_TRANS_ATTN])
def test_plans_without_the_flag_have_none_of_it(flags):
    """(that no recorded plan moved is tests/test_plan_fingerprints_cpu.py's; here: no new region, phase or live parameter leaks)"""
    plan = _plan(TINY, flags)
    assert not {"F1a", "attn_frame", "gF1a", "gPfT", "gF1s"} & set(plan.regions)
    assert not any(ph.kind in (PH_FRAME_ATTN_FWD, PH_FRAME_ATTN_BWD) for ph in plan_arrays(plan)[2])
    if not flags & _lib.FLAG_ADV_FRAME:
        assert "fc_feature_domain.weight" not in {n for n, _, _, lv in plan.params if lv}


def test_twin_plan_reads_the_twin_of_f1a():
    """bf16 + bf16_store: the tuple launch and the launch of the TRN weight gradients read twins (the frame-attention kernel keeps
    F1a's); fc_dim 20 (no 16-byte pieces of 8 elements): they keep rounding fp32 operands in registers."""
    tw = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
    for fc_dim, want in ((64, True), (20, False)):
        plan = _plan(dict(TINY, fc_dim=fc_dim), FAF | tw)
        _, tasks, phases, geo, _, _ = plan_arrays(plan)
        gF1a = plan.region("gF1a")[0]
        zr = [ph for ph in phases if ph.group == 0 and ph.kind == 0 and tasks[ph.task_begin].c_off == geo.o_Zr]
        gw = [ph for ph in phases if ph.group == 2 and ph.kind == 0 and
              any(tasks[k].c_off == gF1a for k in range(ph.task_begin, ph.task_begin + ph.task_count))]
        assert len(zr) == 1 and len(gw) == 1
        assert bool(zr[0].bf16 & 16) == want and bool(gw[0].bf16 & 16) == want


# ---- refusals and acceptance ----
@pytest.mark.parametrize("flags,kw,named", [
    (FAF & ~_lib.FLAG_TRANS_ATTN & ~_lib.FLAG_ATTN_ENTROPY, {}, "needs use_attn TransAttn"),
    (FAF, dict(aggregation=_lib.AGG_AVGPOOL), "on avgpool"),
    (FAF | _lib.FLAG_F32_SPLIT, {}, "F32_SPLIT"), (FAF | _lib.FLAG_MCD, {}, "MCD"), (FAF | _lib.FLAG_BN_SHARED, {}, "use_bn"),
    (FAF, dict(shared_fc_layers=2), "shared_fc_layers"), (FAF, dict(chain=1), "chain"), (FAF, dict(split_k=2), "split_k"),
    (FAF, dict(wgrads_late=1), "wgrads_late")])
def test_plan_refuses_unbuilt_combinations_by_name(flags, kw, named):
    with pytest.raises(ValueError, match="use_attn_frame.*" + named):
        _plan(TINY, flags, **kw)


@pytest.mark.parametrize("arith", [0, _lib.FLAG_BF16_MFMA, _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE])
def test_plan_accepts_the_supported_combination(arith):
    for extra in (0, _lib.FLAG_FEATURE_GRADS):
        plan = _plan(TINY, FAF | arith | extra)
        assert not plan.has_fused_step and _lib.lib().ta3n_has_pipelined_step(plan.handle) == 0
        assert plan.region("attn_frame")[1] == 50 and plan.region("F1a")[1] == 50 * 64


def test_refusal_text_names_the_combination():
    assert frame_attn_refusal("none", use_attn="none", frame_aggregation="avgpool", use_bn="AdaBN") == ""
    assert frame_attn_refusal("TransAttn") == ""
    assert "--use_attn_frame general" in frame_attn_refusal("general")
    assert "--use_attn none" in frame_attn_refusal("TransAttn", use_attn="none")
    assert "avgpool" in frame_attn_refusal("TransAttn", use_attn="none", frame_aggregation="avgpool")
    for kw, named in ((dict(add_fc=2), "--add_fc 2"), (dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(dis_DA="JAN"), "--dis_DA JAN"),
                      (dict(ens_DA="MCD"), "--ens_DA MCD"), (dict(f32_split=True), "f32_split"), (dict(chain=True), "chain"),
                      (dict(split_k=2), "split_k"), (dict(wgrads_late=True), "wgrads_late")):
        assert named in frame_attn_refusal("TransAttn", **kw)


def test_train_engine_refuses_before_it_needs_a_device(monkeypatch):
    """TrainEngine names the combination (the refusals come first; on a machine without a GPU the supported one then stops at the
    device check, which is how this test tells them apart)."""
    from ta3n_amd.engine import TrainEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for kw, named in ((dict(flags=FAF & ~_lib.FLAG_TRANS_ATTN & ~_lib.FLAG_ATTN_ENTROPY), "--use_attn none"),
                      (dict(flags=FAF, aggregation="avgpool"), "avgpool"), (dict(flags=FAF, use_bn="AdaBN"), "--use_bn AdaBN"),
                      (dict(flags=FAF, ens_DA="MCD"), "--ens_DA MCD"), (dict(flags=FAF, dis_DA="DAN"), "--dis_DA DAN"),
                      (dict(flags=FAF, f32_split=True), "f32_split")):
        with pytest.raises(NotImplementedError, match="use_attn_frame.*" + named):
            TrainEngine(6, 4, 5, 512, 64, 12, **kw)
    with pytest.raises(NotImplementedError, match="--add_fc 2"):
        TrainEngine(6, 4, 5, 512, 64, 12, flags=FAF, add_fc=2)


def _model(**kw):
    from ta3n_amd.models import VideoModel
    return VideoModel(12, "video", kw.pop("agg", "trn-m"), "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64,
                      verbose=False, **kw)


def test_video_model_accepts_frame_attention_and_adds_no_parameters():
    plain, m = _model(use_attn="TransAttn"), _model(use_attn="TransAttn", use_attn_frame="TransAttn")
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert m._flags() == plain._flags() | _lib.FLAG_FRAME_ATTN and m.use_attn_frame == "TransAttn"
    plan = m._plan(6, 4)
    assert "F1a" in plan.regions and not plan.has_fused_step


@pytest.mark.parametrize("kw,named", [(dict(use_attn="none", use_attn_frame="TransAttn"), "--use_attn none"),
                                      (dict(use_attn="TransAttn", use_attn_frame="general"), "--use_attn_frame general"),
                                      (dict(agg="avgpool", use_attn="none", use_attn_frame="TransAttn"), "avgpool"),
                                      (dict(use_attn="TransAttn", use_attn_frame="TransAttn", use_bn="AdaBN"), "--use_bn AdaBN"),
                                      (dict(use_attn="TransAttn", use_attn_frame="TransAttn", ens_DA="MCD"), "--ens_DA MCD"),
                                      (dict(use_attn="TransAttn", use_attn_frame="TransAttn", add_fc=2), "--add_fc 2")])
def test_video_model_refuses_unbuilt_combinations_by_name(kw, named):
    with pytest.raises(NotImplementedError, match="use_attn_frame.*" + named):
        _model(**kw)


BASE = ["classInd.txt", "RGB", "s.txt", "t.txt", "v.txt", "--baseline_type", "video", "--frame_aggregation", "trn-m",
        "--use_target", "uSv", "--adv_DA", "RevGrad", "--add_loss_DA", "attentive_entropy", "--lr_adaptive", "dann", "--fc_dim", "512"]


def test_validate_options_accepts_frame_attention():
    import train_ddp
    from ta3n_amd.opts import parser
    for extra in ([], ["--place_adv", "Y", "Y", "N"]):
        args = parser.parse_args(BASE + ["--use_attn", "TransAttn", "--use_attn_frame", "TransAttn"] + extra)
        train_ddp.validate_options(args)
        train_ddp.validate_options(args, module_path=True)


@pytest.mark.parametrize("extra,named", [
    (["--use_attn", "none", "--use_attn_frame", "TransAttn", "--add_loss_DA", "none"], "--use_attn none"),
    (["--use_attn", "TransAttn", "--use_attn_frame", "general"], "--use_attn_frame general"),
    (["--use_attn", "TransAttn", "--use_attn_frame", "TransAttn", "--use_bn", "AdaBN"], "--use_bn AdaBN"),
    (["--use_attn", "TransAttn", "--use_attn_frame", "TransAttn", "--ens_DA", "MCD", "--mu", "0.5"], "--ens_DA MCD"),
    (["--use_attn", "TransAttn", "--use_attn_frame", "TransAttn", "--dis_DA", "JAN"], "--dis_DA JAN"),
    (["--use_attn", "TransAttn", "--use_attn_frame", "TransAttn", "--add_fc", "2"], "--add_fc 2")])
def test_validate_options_refuses_unbuilt_combinations_by_name(extra, named):
    import train_ddp
    from ta3n_amd.opts import parser
    for module_path in (False, True):
        with pytest.raises(SystemExit) as e:
            train_ddp.validate_options(parser.parse_args(BASE + extra), module_path=module_path)
        assert "unsupported option" in str(e.value) and "use_attn_frame" in str(e.value) and named in str(e.value)


def test_validate_options_refuses_frame_attention_on_avgpool():
    import train_ddp
    from ta3n_amd.opts import parser
    argv = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "avgpool", "--use_attn", "none", "--add_loss_DA", "none",
            "--use_attn_frame", "TransAttn"]
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(parser.parse_args(argv))
    assert "--use_attn_frame TransAttn on --frame_aggregation avgpool" in str(e.value)


def test_flags_from_options_default_is_what_it_was():
    """Without the new keyword: the values the function returned before it existed, for the argument sets the other tests use."""
    R, V, Fr, E, A = (_lib.FLAG_ADV_RELATION, _lib.FLAG_ADV_VIDEO, _lib.FLAG_ADV_FRAME, _lib.FLAG_ATTN_ENTROPY, _lib.FLAG_TRANS_ATTN)
    assert flags_from_options() == R | V | Fr | E | A == 31
    assert flags_from_options(("N", "Y", "Y"), "none", "none", "RevGrad", "uSv") == V | Fr
    assert flags_from_options(place_adv=("Y", "Y", "Y"), add_loss_DA="none", use_attn="none") == R | V | Fr
    assert flags_from_options(("Y", "Y", "N"), "attentive_entropy", "TransAttn", "RevGrad", "uSv") == R | V | E | A
    assert flags_from_options(("Y", "Y", "Y"), "attentive_entropy", "TransAttn", "none", "uSv") == E | A
    assert flags_from_options(("Y", "Y", "Y"), "attentive_entropy", "TransAttn", "RevGrad", "none") == A
    assert flags_from_options(("Y", "Y", "Y"), "none", "TransAttn") == R | V | Fr | A
    assert flags_from_options(use_attn_frame="none") == 31
    assert flags_from_options(use_attn_frame="TransAttn") == 31 | _lib.FLAG_FRAME_ATTN == 31 | (1 << 11)


@pytest.mark.parametrize("kind", ["general", "DotProduct"])
def test_flags_from_options_refuses_other_kinds_by_name(kind):
    """The flag bit means TransAttn: no other kind of frame attention may turn into it on the way to TrainEngine(flags=...)."""
    with pytest.raises(ValueError, match="--use_attn_frame " + kind):
        flags_from_options(use_attn_frame=kind)
