"""--pretrain_source and --lr_adaptive loss on the CPU: the shared parameter layout (ta3n_config.layout_flags), the live ranges of the
source-only plan, the two plans interpreted on ONE buffer (tests/plan_interp.py) against the fixtures the reference's own main.train wrote
(tests/golden/make_golden_pretrain.py), the refusals by name, validate_options on both programs and the loss-driven learning-rate rule."""
import math

import numpy as np
import pytest
import torch

import main as own_main
import train_ddp
from golden_util import Golden, case_config, step_schedule
from plan_interp import Interp
from test_plan_cpu import make_hyper
from ta3n_amd import _lib, tolerances as tol
from ta3n_amd.engine import PRETRAIN_DROPPED_FLAGS, flags_from_options, pretrain_refusal
from ta3n_amd.opts import parser
from ta3n_amd.synthetic import synth_batch, synth_state

ADV = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
TA3N = ADV | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN
SHAPE = (6, 4, 5, 512, 64, 12)
# the fixtures the plan interpreter can express (its loss has neither class weights nor target labels: tiny_pre_sv_wcls is the GPU test's)
INTERP_FIXTURES = ["tiny_pre_T5", "tiny_pre_T2", "tiny_pre_noattn", "tiny_pre_clip", "tiny_pre_short", "tiny_avgpool_pre"]


def fixture_flags(g, c):
    """(step flags, aggregation) of a pretrain fixture, as main.py composes them."""
    if c["agg"] == "avgpool":
        return flags_from_options(place_adv=c["place_adv"], add_loss_DA="none", use_attn="none"), _lib.AGG_AVGPOOL
    use_attn = str(g.meta("use_attn"))
    return flags_from_options(add_loss_DA="attentive_entropy" if use_attn != "none" else "none", use_attn=use_attn,
                              use_target=str(g.meta("use_target"))), _lib.AGG_TRN_M


def reached(plan):
    return {n for n, _, _, live in plan.params if live}


def expected_reached(T, attn):
    names = ["fc_feature_shared_source", "fc_classifier_video_source"] + [f"TRN.fc_fusion_scales.{j}.1" for j in range(T - 1)]
    if attn:
        names += [f"relation_domain_classifier_all.{j}.{k}" for j in range(T - 1) for k in (0, 2)]
    return {f"{n}.{w}" for n in names for w in ("weight", "bias")}


@pytest.mark.parametrize("flags,layout", [(_lib.FLAG_TRANS_ATTN, TA3N), (0, TA3N), (0, ADV), (_lib.FLAG_TRANS_ATTN | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE,
                                                                                       TA3N | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE)])
def test_layout_is_the_donors_entry_for_entry(flags, layout):
    donor = _lib.Plan(*SHAPE, layout)
    plan = _lib.Plan(*SHAPE, flags, layout_flags=layout)
    assert [p[:3] for p in plan.params] == [p[:3] for p in donor.params]      # name, offset, shape in the donor's order
    assert (plan.param_floats, plan.live_floats) == (donor.param_floats, donor.live_floats)
    own = _lib.Plan(*SHAPE, flags)
    assert reached(plan) == reached(own)                                      # which parameters are live stays the plan's own
    assert [ph["kind"] for ph in plan.description["phases"]] == [ph["kind"] for ph in own.description["phases"]]      # ... and so do its launches
    assert donor.live_ranges == [(0, donor.live_floats)] and own.live_ranges == [(0, own.live_floats)]


def test_avgpool_layout_crosses_the_two_builders():
    donor = _lib.Plan(6, 4, 5, 512, 64, 5, _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME, aggregation=_lib.AGG_AVGPOOL)
    plan = _lib.Plan(6, 4, 5, 512, 64, 5, 0, aggregation=_lib.AGG_AVGPOOL, layout_flags=_lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME)
    assert [p[:3] for p in plan.params] == [p[:3] for p in donor.params]
    assert reached(plan) == {f"{n}.{w}" for n in ("fc_feature_shared_source", "fc_classifier_video_source") for w in ("weight", "bias")}
    assert len(plan.live_ranges) == 2


@pytest.mark.parametrize("T", [2, 5, 9])
@pytest.mark.parametrize("attn", [True, False])
def test_live_ranges_cover_exactly_what_the_pass_reaches(T, attn):
    flags = _lib.FLAG_TRANS_ATTN if attn else 0
    plan = _lib.Plan(5, 3, T, 512, 32, 7, flags, layout_flags=ADV | _lib.FLAG_ATTN_ENTROPY | flags)
    assert reached(plan) == expected_reached(T, attn)
    rel = {n for n in reached(plan) if n.startswith("relation_domain_classifier_all")}
    assert bool(rel) == attn
    rng = plan.live_ranges
    assert all(b % 4 == 0 and e % 4 == 0 and b < e for b, e in rng)                       # float4 access
    assert all(rng[i][1] < rng[i + 1][0] for i in range(len(rng) - 1))                    # ascending, disjoint, maximal (no two touch)
    assert rng[0][0] == 0 and rng[-1][1] <= plan.live_floats
    covered = np.zeros(plan.param_floats, bool)
    for b, e in rng:
        covered[b:e] = True
    for name, off, shape, live in plan.params:
        n = int(np.prod(shape))
        assert covered[off:off + n].all() if live else not covered[off:off + n].any(), name
        covered[off:off + (n + 7) // 8 * 8] = False      # (the alignment padding behind a live parameter belongs to its range)
    assert not covered.any()


def test_plan_create_refuses_by_message():
    with pytest.raises(ValueError, match="fc_feature_domain.weight is live under flags and not under layout_flags"):
        _lib.Plan(*SHAPE, TA3N, layout_flags=_lib.FLAG_TRANS_ATTN)
    with pytest.raises(ValueError, match="fc_classifier_video_source_2.weight does not exist under layout_flags"):
        _lib.Plan(*SHAPE, _lib.FLAG_MCD, layout_flags=TA3N)
    with pytest.raises(ValueError, match="layout_flags: the donor configuration is refused: attentive_entropy requires"):
        _lib.Plan(*SHAPE, 0, layout_flags=_lib.FLAG_ATTN_ENTROPY)


def subset_update(it, ranges, h):
    """clip_grad_norm_ + Nesterov SGD over float ranges of the interpreter's flat buffers (torch's rule for the parameters with a grad)."""
    idx = np.concatenate([np.arange(b, e) for b, e in ranges])
    total = math.sqrt(float((it.G[idx] ** 2).sum()))
    coef = min(h["clip"] / (total + 1e-6), 1.0) if h["clip"] > 0 else 1.0
    d = it.G[idx] * coef + h["weight_decay"] * it.P[idx]
    it.M[idx] = h["momentum"] * it.M[idx] + d
    it.P[idx] -= h["lr"] * (d + h["momentum"] * it.M[idx])
    return total, coef


@pytest.mark.parametrize("name", INTERP_FIXTURES)
def test_two_plans_on_one_buffer_reproduce_the_reference(name):
    g = Golden(name)
    c = case_config(g)
    flags, agg = fixture_flags(g, c)
    pre_flags = flags & ~PRETRAIN_DROPPED_FLAGS
    dims = (c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"])
    plan, pre = _lib.Plan(*dims, flags, aggregation=agg), _lib.Plan(*dims, pre_flags, aggregation=agg, layout_flags=flags)
    assert reached(pre) == set(str(k) for k in g.meta("pre_live")) and reached(plan) == set(str(k) for k in g.meta("live"))
    it, ip = Interp(plan), Interp(pre)
    ip.P, ip.G, ip.M = it.P, it.G, it.M                                   # ONE params / grads / momentum buffer
    shapes = {n: s for n, _, s, _ in plan.params}
    it.set_params(synth_state(shapes, seed=c["wseed"], scale=c["wscale"]))
    outside = np.ones(plan.param_floats, bool)
    for b, e in pre.live_ranges:
        outside[b:e] = False
    for s, st in enumerate(step_schedule(c)):
        xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
        xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
        it.X = ip.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
        it.labels[:c["Bs"]] = ip.labels[:c["Bs"]] = ys.numpy()
        it.hy = ip.hy = make_hyper(c, st, c["T"], st["lr"])
        if c["agg"] == "avgpool":
            it.hy["gamma"] = 0.0
        p0, m0 = it.P.copy(), it.M.copy()
        it.G[:] = np.where(outside, 1e3, 0.0)                             # stale gradients of what the pass does not reach must not matter
        ip.run_group(4)
        subset_update(ip, pre.live_ranges, ip.hy)
        assert np.array_equal(it.P[outside], p0[outside]) and np.array_equal(it.M[outside], m0[outside])     # untouched: bit-equal
        after_pass = it.get_params()
        for k in reached(pre):
            g.check(f"step{s}/pre/param/{k}", after_pass[k], tol.F32_RTOL, tol.F32_ATOL)
        it.G[:] = 0
        it.run_group(4)
        raw = it.get_params(it.G)
        it.run_group(3, fused_norm=True)
        coef = it.ws[it.g.o_grad_norm + 1]
        new = it.get_params()
        for k in shapes:
            if k in reached(plan):
                g.check(f"step{s}/clipped_grad/{k}", raw[k] * coef, 1e-3, 2e-5, rms_atol=1e-2)
            g.check(f"step{s}/param/{k}", new[k], tol.F32_RTOL, tol.F32_ATOL)


@pytest.mark.parametrize("kw,named", [
    (dict(optimizer="Adam"), "optimizer Adam"), (dict(dis_DA="DAN"), "--dis_DA DAN"), (dict(dis_DA="JAN"), "--dis_DA JAN"),
    (dict(ens_DA="MCD"), "--ens_DA MCD"), (dict(use_attn_frame="TransAttn"), "--use_attn_frame TransAttn"),
    (dict(use_attn="general"), "--use_attn general"), (dict(share_params="N"), "--share_params N"), (dict(add_fc=2), "--add_fc 2"),
    (dict(add_fc=3), "--add_fc 3"), (dict(use_bn="AdaBN"), "--use_bn AdaBN"), (dict(f32_split=True), "f32x3"),
    (dict(feeds=True), "train_steps(feeds=...)"), (dict(capture=True), "capture()"), (dict(fused_update=True), "fused_update"),
    (dict(world=2), "world size 2"), (dict(process_group=True), "process group"), (dict(sharded_update=True), "shard"),
    (dict(peer_exchange=True), "peer"), (dict(ddp_selftest=True), "TA3N_DDP_SELFTEST")])
def test_refusals_name_what_is_not_built(kw, named):
    msg = pretrain_refusal(**kw)
    assert msg.startswith("pretrain_source together with ") and "is not built" in msg and named in msg, msg


def test_built_combinations_are_not_refused():
    assert pretrain_refusal() == "" and pretrain_refusal(use_attn="none") == "" and pretrain_refusal(optimizer="SGD", add_fc=1, world=1) == ""


BASE = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "trn-m"]


@pytest.mark.parametrize("opt,named", [(["--pretrain_source"], "--pretrain_source (built on main.py)"),
                                       (["--lr_adaptive", "loss"], "--lr_adaptive loss (built: dann, none with --lr_steps/--lr_decay; loss is built on main.py)")])
def test_validate_options_on_both_programs(opt, named):
    args = parser.parse_args(BASE + opt)
    train_ddp.validate_options(args, module_path=True)
    with pytest.raises(SystemExit) as e:
        train_ddp.validate_options(args)
    assert "unsupported option" in str(e.value) and named in str(e.value)
    train_ddp.validate_options(parser.parse_args(BASE + ["--pretrain_source", "--lr_adaptive", "loss", "--optimizer", "Adam", "--ens_DA", "MCD"]),
                               module_path=True)


def test_adjust_learning_rate_loss_on_a_scripted_sequence():
    lin = torch.nn.Linear(2, 2)
    opt = torch.optim.SGD(lin.parameters(), 0.08)
    current = previous = 999                         # main.py:221-222
    seen = []
    for loss_c in (2.0, 1.5, 1.7, 1.7, 1.6, 1.9, 3.0):
        own_main.adjust_learning_rate_loss(opt, 2.0, current, previous, ">")
        seen.append(opt.param_groups[0]["lr"])
        previous, current = current, loss_c
    # epoch 1: 999 > 999 no; 2: 2.0 > 999 no; 3: 1.5 > 2.0 no; 4: 1.7 > 1.5 YES; 5: 1.7 > 1.7 no; 6: 1.6 > 1.7 no; 7: 1.9 > 1.6 YES
    assert seen == [0.08, 0.08, 0.08, 0.04, 0.04, 0.04, 0.02]
    for op, cur, prev, moved in (("<", 1.0, 2.0, True), (">=", 2.0, 2.0, True), ("<=", 3.0, 2.0, False)):
        opt.param_groups[0]["lr"] = 1.0
        own_main.adjust_learning_rate_loss(opt, 4.0, cur, prev, op)
        assert opt.param_groups[0]["lr"] == (0.25 if moved else 1.0)
