"""--add_fc 2 / 3 (models.py:145-153, 581-603: one or two more Linear(F, F) -> ReLU -> dropout_i layers on the shared frame FC)
on the CPU: the plan's parameter table against the reference's, the launch structure, the single-layer plans left byte for byte
as they were, the descriptor lists executed with numpy (tests/plan_interp.py) against fixtures the reference produced
(tests/golden/make_golden_add_fc.py), and the option handling of train_ddp.py / VideoModel / test_models.py."""
import os
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden, case_config, step_schedule
from plan_interp import Interp, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state
from test_plan_cpu import make_hyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALL_FLAGS = (_lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN)
ADD_FC_CASES = ["tiny_addfc2", "tiny_addfc3_clip", "tiny_avgpool_addfc2_da", "tiny_avgpool_addfc2", "headline_addfc2"]
SMALL_CASES = [n for n in ADD_FC_CASES if n.startswith("tiny")]


def _setup(name):
    g = Golden(name)
    c = case_config(g)
    c["add_fc"] = int(g.meta("add_fc"))
    avg = c["agg"] == "avgpool"
    if not avg:
        flags = ALL_FLAGS
    elif c["place_adv"] is None:
        flags = 0                                             # TemPooling, source-only (use_target none)
    else:
        flags = flags_from_options(c["place_adv"], "none", "none", "RevGrad", "uSv")
    return g, c, flags, (_lib.AGG_AVGPOOL if avg else _lib.AGG_TRN_M)


def _plan(c, flags, agg, layers, **kw):
    return _lib.Plan(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags, aggregation=agg, shared_fc_layers=layers, **kw)


def _arrays(plan):
    segs, tasks, phases, geom, tup, tf = plan_arrays(plan)
    return bytes(segs), bytes(tasks), bytes(phases), bytes(geom), tup.tobytes(), tf.tobytes()


@pytest.mark.parametrize("name", ADD_FC_CASES)
def test_plan_parameters_are_the_references(name):
    """Every parameter of the reference model (names, shapes, total count from the fixture), the new layers live and directly
    behind fc_feature_shared_source (which stays first: the pipelined step updates it on its own)."""
    g, c, flags, agg = _setup(name)
    plan = _plan(c, flags, agg, c["add_fc"])
    want = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(g.meta("param_keys"), g.meta("param_shapes"))}
    got = {n: tuple(s) for n, _, s, _ in plan.params}
    assert set(got) >= set(want)
    assert {n: got[n] for n in want} == want
    assert sum(int(np.prod(s)) for n, s in got.items() if n in want) == int(g.meta("n_params"))
    assert {n for n, _, _, lv in plan.params if lv} == set(str(k) for k in g.meta("live"))
    names = [n for n, _, _, _ in plan.params]
    new = [f"fc_feature_shared_{k}_source.{w}" for k in range(2, c["add_fc"] + 1) for w in ("weight", "bias")]
    assert names[:2 + len(new)] == ["fc_feature_shared_source.weight", "fc_feature_shared_source.bias"] + new
    assert all(lv for n, _, _, lv in plan.params if n in new)


def _gemm_phases(plan, groups):
    _, _, phases, _, _, _ = plan_arrays(plan)
    return sum(1 for ph in phases if ph.group in groups and ph.kind == 0)


@pytest.mark.parametrize("agg,flags", [(_lib.AGG_TRN_M, ALL_FLAGS), (_lib.AGG_AVGPOOL, 0),
                                       (_lib.AGG_AVGPOOL, _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME)])
@pytest.mark.parametrize("layers", [2, 3])
def test_each_layer_adds_one_forward_and_one_backward_launch(agg, flags, layers):
    c = dict(Bs=128, Bt=74, T=5, D=2048, fc_dim=512, C=12)
    one, more = _plan(c, flags, agg, 1), _plan(c, flags, agg, layers)
    assert more.has_fused_step
    assert _gemm_phases(more, (4,)) == _gemm_phases(one, (4,)) + 2 * (layers - 1)
    assert _gemm_phases(more, (0, 2)) == _gemm_phases(one, (0, 2)) + 2 * (layers - 1)
    for k in range(1, layers):       # the earlier layers' activations and gradients are named regions
        assert more.region(f"F_l{k}")[1] == 202 * 5 * 512 and more.region(f"gZ_l{k}")[1] == 202 * 5 * 512
    if agg == _lib.AGG_TRN_M:        # 8 launches per step (7 + the update) at one layer, 8 + 2 (add_fc - 1) with more
        _, _, phases, _, _, _ = plan_arrays(more)
        assert sum(1 for ph in phases if ph.group == 4) + 1 == 8 + 2 * (layers - 1)


@pytest.mark.parametrize("agg,flags", [(_lib.AGG_TRN_M, ALL_FLAGS), (_lib.AGG_TRN_M, ALL_FLAGS | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE),
                                       (_lib.AGG_TRN_M, ALL_FLAGS | _lib.FLAG_FEATURE_GRADS), (_lib.AGG_AVGPOOL, 0),
                                       (_lib.AGG_AVGPOOL, _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE)])
def test_zero_and_one_layer_plans_are_byte_identical(agg, flags):
    """shared_fc_layers 0 (the field's value in every caller that predates it) and 1 build the same plan."""
    c = dict(Bs=128, Bt=74, T=5, D=2048, fc_dim=512, C=12)
    a, b = _plan(c, flags, agg, 0), _plan(c, flags, agg, 1)
    assert _arrays(a) == _arrays(b)
    assert a.params == b.params and a.regions == b.regions and (a.param_floats, a.ws_floats) == (b.param_floats, b.ws_floats)
    assert not any(k.startswith(("F_l", "gZ_l")) for k in a.regions)


def test_stacked_layers_carry_their_own_dropout_stream():
    """The k-th layer's forward tiles offset the dropout element id by (k - 1) B T F (Task.pad2); every other task keeps 0."""
    c = dict(Bs=6, Bt=4, T=5, D=512, fc_dim=64, C=12)
    plan = _plan(c, ALL_FLAGS, _lib.AGG_TRN_M, 3)
    _, tasks, _, _, _, _ = plan_arrays(plan)
    BTF = 10 * 5 * 64
    F = {plan.region("F_l1")[0]: 0, plan.region("F_l2")[0]: BTF, plan.region("F1")[0]: 2 * BTF}
    seen = set()
    for t in tasks:
        if t.epi & 16 and t.seg_count > 0:            # EPI_DROP_I
            assert t.c_off in F and t.pad2 == F[t.c_off]
            seen.add(t.c_off)
        else:
            assert t.pad2 == 0
    assert seen == set(F)
    one = _plan(c, ALL_FLAGS, _lib.AGG_TRN_M, 1)
    assert all(t.pad2 == 0 for t in plan_arrays(one)[1])


@pytest.mark.parametrize("what,kw", [("use_bn", dict(flags_extra=_lib.FLAG_BN_SHARED)), ("ens_DA MCD", dict(flags_extra=_lib.FLAG_MCD)),
                                     ("chain", dict(chain=1)), ("split_k", dict(split_k=2)), ("wgrads_late", dict(wgrads_late=1)),
                                     ("phase_tiles", dict(phase_tiles=[222] * 8))])
def test_plan_refuses_unbuilt_combinations_by_name(what, kw):
    c = dict(Bs=6, Bt=4, T=5, D=512, fc_dim=64, C=12)
    extra = kw.pop("flags_extra", 0)
    with pytest.raises(ValueError, match=what):
        _plan(c, ALL_FLAGS | extra, _lib.AGG_TRN_M, 2, **kw)
    _plan(c, ALL_FLAGS | extra, _lib.AGG_TRN_M, 1, **kw)      # (built at one layer)
    with pytest.raises(ValueError, match="shared_fc_layers"):
        _plan(c, ALL_FLAGS, _lib.AGG_TRN_M, 4)


def _run_interp(name, fused, bf16=False):
    g, c, flags, agg = _setup(name)
    T, L = c["T"], c["add_fc"]
    plan = _plan(c, flags | ((_lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE) if bf16 else 0), agg, L)
    it = Interp(plan)
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    live = {n for n, _, _, lv in plan.params if lv}
    avg = c["agg"] == "avgpool"
    return g, c, plan, it, shapes, live, avg, T, L


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_plan_reproduces_reference(name, fused):
    """fused=False: ta3n_forward / ta3n_loss / ta3n_backward; fused=True: ta3n_train_step.  Forward outputs (every shared layer's),
    losses, clipped gradients and parameters after every step, against the reference's run of the same command."""
    g, c, plan, it, shapes, live, avg, T, L = _run_interp(name, fused)
    log_losses = [float(line.split("Loss ")[1].split()[0]) for line in str(g.meta("log")).splitlines() if "Loss " in line]
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, yt = synth_batch(c["C"], T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:c["Bs"]] = ys.numpy()
        it.hy = make_hyper(c, st, T, st["lr"])
        if avg:
            it.hy["gamma"] = 0.0
            if c["place_adv"] is None:
                it.hy["beta"] = [0.0, 0.0, 0.0]
        it.G[:] = 0
        it.run_group(4 if fused else 0)
        if s == 0:
            B, Bs = c["Bs"] + c["Bt"], c["Bs"]
            geo = it.g
            F = geo.F
            outs = {f"l{k}": it.r(plan.region(f"F_l{k}")[0], (B, T, F)) for k in range(1, L)}
            outs[f"l{L}"] = it.r(geo.o_F1, (B, T, F))
            out = it.r(geo.o_Y, (B, c["C"]))
            v = it.r(geo.o_V, (B, geo.NB))
            for dom, sl in (("s", slice(0, Bs)), ("t", slice(Bs, B))):
                g.check(f"fwd/out_{dom}", out[sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_v", v[sl], 5e-5, 2e-5)
                g.check(f"fwd/feat_{dom}_f1", outs[f"l{L}"][sl], 5e-5, 2e-5)      # feat[2]: the LAST layer's output
                for k in range(1, L + 1):
                    g.check(f"fwd/feat_{dom}_l{k}", outs[f"l{k}"][sl], 5e-5, 2e-5)
                if not avg:
                    g.check(f"fwd/pd_{dom}_frm", it.r(geo.o_Pf, (B, T, 2))[sl], 5e-5, 2e-5)
                    g.check(f"fwd/attn_{dom}", it.r(geo.o_attn, (B, T - 1))[sl], 5e-5, 2e-5)
        if not fused:
            it.run_group(1)
            it.run_group(2)
        # the logged total loss of the step (the reference's `Loss` meter, main.py:597-605)
        assert abs(float(it.ws[it.g.o_losses]) - log_losses[s]) <= 1e-4 * max(1.0, abs(log_losses[s])), (s, it.ws[it.g.o_losses], log_losses[s])
        raw = it.get_params(it.G)
        it.run_group(3, fused_norm=fused)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in live:
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 1e-4, 2e-5)
            g.check(f"step{s}/param/{k}", new[k], 1e-4, 2e-5)
        if name == "tiny_addfc3_clip":
            assert coef < 1.0       # the clip branch was taken - with the new layers' Σg² in the fused norm (fused=True)


@pytest.mark.parametrize("name", ["tiny_addfc2", "tiny_avgpool_addfc2"])
def test_bf16_twin_plan_reads_twins_of_the_new_layers(name):
    """bf16 + bf16_store at add_fc 2: the new launches read twins, and the numpy execution of the twin plan stays within the bf16
    bounds of the reference's trajectory (step 0 parameters)."""
    g, c, plan, it, shapes, live, avg, T, L = _run_interp(name, True, bf16=True)
    _, tasks, phases, _, _, _ = plan_arrays(plan)
    F1l = plan.region("F_l1")[0]
    readers = [ph for ph in phases if ph.group == 4 and ph.kind == 0 and
               any(tasks[i].aux_off == F1l or tasks[i].c_off == plan.region("gZ_l1")[0] for i in range(ph.task_begin, ph.task_begin + ph.task_count))]
    assert readers and all(ph.bf16 & 16 for ph in readers)
    st = step_schedule(c)[0]
    xs, xt, ys, yt = synth_batch(c["C"], T, c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:c["Bs"]] = ys.numpy()
    it.hy = make_hyper(c, st, T, st["lr"])
    if avg:
        it.hy["gamma"] = 0.0
        it.hy["beta"] = [0.0, 0.0, 0.0]
    it.G[:] = 0
    it.run_group(4)
    it.run_group(3, fused_norm=True)
    new = it.get_params()
    for k in shapes:
        g.check(f"step0/param/{k}", new[k], 2e-2, 2e-4, rms_atol=0.02)


# ---- options ----
BASE = ["classInd.txt", "RGB", "s.txt", "t.txt", "v.txt", "--baseline_type", "video", "--frame_aggregation", "trn-m",
        "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn", "--add_loss_DA", "attentive_entropy",
        "--lr_adaptive", "dann", "--fc_dim", "512"]
AVG = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "avgpool", "--use_attn", "none", "--add_loss_DA", "none"]


@pytest.mark.parametrize("layers", ["2", "3"])
def test_validate_options_accepts_add_fc_2_and_3(layers):
    import train_ddp
    from ta3n_amd.opts import parser
    for argv in (BASE, AVG, AVG + ["--use_target", "none"], AVG + ["--place_adv", "N", "Y", "Y"]):
        train_ddp.validate_options(parser.parse_args(argv + ["--add_fc", layers]))
        train_ddp.validate_options(parser.parse_args(argv + ["--add_fc", layers]), module_path=True)


@pytest.mark.parametrize("extra,named", [(["--add_fc", "4"], "--add_fc 4"), (["--add_fc", "0"], "at least one fc layer"),
                                         (["--add_fc", "2", "--use_bn", "AdaBN"], "--use_bn AdaBN"),
                                         (["--add_fc", "2", "--use_bn", "AutoDIAL"], "--use_bn AutoDIAL"),
                                         (["--add_fc", "2", "--dis_DA", "DAN", "--place_dis", "N", "Y", "N", "N"], "--dis_DA DAN"),
                                         (["--add_fc", "3", "--dis_DA", "JAN"], "--dis_DA JAN"),
                                         (["--add_fc", "2", "--ens_DA", "MCD", "--mu", "0.5"], "--ens_DA MCD")])
def test_validate_options_refuses_unbuilt_add_fc_combinations_by_name(extra, named):
    import train_ddp
    from ta3n_amd.opts import parser
    for module_path in (False, True):
        with pytest.raises(SystemExit) as e:
            train_ddp.validate_options(parser.parse_args(BASE + extra), module_path=module_path)
        assert "unsupported option" in str(e.value) and named in str(e.value)


@pytest.mark.parametrize("name", ["tiny_addfc2", "tiny_addfc3_clip", "tiny_avgpool_addfc2_da"])
def test_video_model_has_the_reference_parameters(name):
    """VideoModel(add_fc=k): the reference's state_dict keys and parameters() order (the optimiser state indices of a checkpoint)."""
    from ta3n_amd.models import VideoModel
    g, c, _, _ = _setup(name)
    arch = {512: "resnet18", 2048: "resnet101"}[c["D"]]
    avg = c["agg"] == "avgpool"
    m = VideoModel(c["C"], "video", "avgpool" if avg else "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model=arch,
                   add_fc=c["add_fc"], fc_dim=c["fc_dim"], use_attn="none" if avg else "TransAttn", verbose=False)
    assert list(m.state_dict().keys()) == [str(k) for k in g.meta("state_keys")]
    assert [n for n, _ in m.named_parameters()] == [str(k) for k in g.meta("param_keys")]
    assert sum(p.numel() for p in m.parameters()) == int(g.meta("n_params"))
    sh = m.fc_feature_shared_2_source
    assert float(sh.bias.detach().abs().max()) == 0.0 and 0.0005 < float(sh.weight.detach().std()) < 0.002      # models.py:146-148: N(0, 0.001), zero bias


@pytest.mark.parametrize("kw,named", [(dict(add_fc=4), "add_fc=4"), (dict(add_fc=2, use_bn="AdaBN"), "use_bn='AdaBN'"),
                                      (dict(add_fc=3, ens_DA="MCD"), "ens_DA='MCD'")])
def test_video_model_refuses_unbuilt_add_fc_combinations_by_name(kw, named):
    from ta3n_amd.models import VideoModel
    with pytest.raises(NotImplementedError, match=named):
        VideoModel(12, "video", "trn-m", "RGB", train_segments=5, val_segments=5, base_model="resnet18", fc_dim=64, verbose=False, **kw)


def test_engine_refusal_names_the_combination():
    from ta3n_amd.engine import add_fc_refusal
    assert add_fc_refusal(1, use_bn="AdaBN", dis_DA="DAN", ens_DA="MCD", chain=True) == ""
    assert add_fc_refusal(2) == "" and add_fc_refusal(3) == ""
    for kw, named in ((dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(dis_DA="JAN"), "--dis_DA JAN"), (dict(ens_DA="MCD"), "--ens_DA MCD"),
                      (dict(chain=True), "chain"), (dict(split_k=2), "split_k"), (dict(wgrads_late=True), "wgrads_late"),
                      (dict(phase_tiles=True), "phase_tiles")):
        assert named in add_fc_refusal(2, **kw)
    assert "--add_fc 4" in add_fc_refusal(4)


def test_test_models_passes_add_fc_through():
    import test_models
    args = test_models.build_parser().parse_args(["classInd.txt", "RGB", "list.txt", "w.pth.tar", "--add_fc", "2",
                                                  "--frame_aggregation", "trn-m", "--baseline_type", "video", "--use_attn", "TransAttn"])
    assert args.add_fc == 2
