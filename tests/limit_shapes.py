"""One table of shapes at the limits of what ta3n_plan_create accepts, shared by tests/test_limit_shapes_cpu.py (wiring of the plan and
conditioning of the inputs, no GPU) and tests/test_gpu_limit_shapes.py (the kernels), with the helpers both use.

Every case names the kernel instantiation or code path it exists for, and `plan_facts` / `assert_runs_what_it_claims` read from the
PLAN that the case really lands there: whether it has the fused step, how many videos a video workgroup of the heads kernel takes
(Geom.heads_vpw), the relation count (n_rel: the pipelined relation loops run where a wave handles more than one), FQ = ceil(F / 64) of
the heads kernel's frame workgroups, and how many GEMM operands cannot move 16 bytes at a time (the scalar loader of gemm_tiles).  A
case that silently lands on another variant is worth nothing.

Inputs are fixed: weights synth_state(seed=wseed, scale="trained"), batches synth_batch(seed=xseed + 7 * step), beta [0.75, 0.75, 0.5],
gamma 0.003, clip 20, no dropout.  The CPU tests check that the float64 oracle and its fp32 evaluation agree on them to a quarter of the
bounds the GPU tests assert (a near-cancelling sum in the inputs would otherwise be blamed on the kernels)."""
import functools

import numpy as np
import torch

from oracle import ta3n_oracle as orc
from plan_interp import PH_GEMM, PH_HEADS, Interp, plan_arrays
from ta3n_amd import _lib
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import ALL_FLAGS, flags_from_options
from ta3n_amd.synthetic import synth_batch, synth_state

BETA, GAMMA, CLIP, LR = [0.75, 0.75, 0.5], 0.003, 20.0, 2e-3
HEADS_MAX_F = 2048          # ta3n_heads.hip: heads_supported


def _case(Bs, Bt, T, D, F, C, why, agg="trn-m", place_adv=("Y", "Y", "Y"), wseed=11, xseed=21, scale="trained", ragged_second_step=False,
          unfused_too=False, arithmetics=False):
    return dict(Bs=Bs, Bt=Bt, T=T, D=D, F=F, C=C, why=why, agg=agg, place_adv=tuple(place_adv), wseed=wseed, xseed=xseed, scale=scale,
                ragged_second_step=ragged_second_step, unfused_too=unfused_too, arithmetics=arithmetics)


# Smallest instantiation first; the widest frame workgroups and the largest batches last (the order the GPU tests run in).
CASES = {
    "odd_D37_F30": _case(3, 2, 4, 37, 30, 7, "scalar loader paths of gemm_tiles (D, F no multiples of 4); FQ 1", unfused_too=True, arithmetics=True),
    "odd_D101_F67": _case(7, 6, 5, 101, 67, 9, "scalar loader paths; FQ 2 with a ragged last 64-column group", ragged_second_step=True),
    "T13_C63_F40": _case(9, 8, 13, 96, 40, 63, "C = 63: every class lane but one"),
    "T25_C33": _case(9, 8, 25, 128, 64, 33, "C just past half a wave; 24 relations", ragged_second_step=True),      # (9+8 videos: the ragged
                                                                                                                   # step leaves 6 and 3 valid)
    "T33_C5": _case(2, 1, 33, 36, 36, 5, "between the 12 segments tested before and the limit"),
    "T63_rows": _case(2, 1, 63, 64, 32, 12, "B T = 189: the last frame row group partly empty"),
    "T64_C64": _case(5, 3, 64, 64, 32, 64, "63 relations fill the relation-logit slots, every class lane valid, PIPE, FQ 1", unfused_too=True,
                     arithmetics=True),
    # (the same kernel variant on 190 videos, for the FREE-RUNNING comparison of the split arithmetic: with ~5e5 hidden units per step at 64
    # segments one of them sits within 2^-16 of zero and lands on the other side of its ReLU than in the oracle; that one unit is 3e-2 of
    # a relation discriminator's gradient at 8 videos, twice F32X3_GRAD_REL_L2, and 6e-3 at 190 - see test_gpu_limit_shapes.py)
    "T64_C64_b190": _case(100, 90, 64, 64, 32, 64, "T64_C64 with enough videos to dilute a flipped ReLU unit; frame rows in groups of 128",
                          xseed=24),      # (batch seeds 21, 23, 25 leave a relation discriminator's 2-element bias gradient a near-cancelling sum:
                                          # 5.0e-5 .. 3.6e-4 between ATen's fp32 and float64, over the conditioning bound; 22 and 24 give 2e-5)
    "C1": _case(3, 2, 2, 256, 256, 1, "a single class; FQ 4; one relation (no PIPE)"),
    "C2_F200": _case(6, 5, 4, 256, 200, 2, "two classes; FQ 4 with a ragged last 64-column group"),
    "F1000": _case(4, 3, 3, 1024, 1000, 12, "FQ 16, ragged", unfused_too=True, arithmetics=True),
    "F2048": _case(3, 2, 2, 2048, 2048, 12, "FQ 32: the widest fc_dim the fused step takes", arithmetics=True),
    "F2304_unfused": _case(3, 2, 3, 2304, 2304, 2, "fc_dim > 2048: no fused step, the engine falls back to the unfused launch lists"),
    "T64_two_per_wg": _case(120, 107, 64, 64, 32, 12, "two videos per video workgroup with an odd video count; 31-32 relations per wave",
                            ragged_second_step=True),
    "F2048_two_per_wg": _case(114, 113, 2, 2048, 2048, 12, "FQ 32 with two videos per video workgroup"),
    # TemPooling: the source-only builder and the general one (RevGrad on all three levels)
    "avg_T64_C64": _case(4, 3, 64, 64, 36, 64, "avgpool, source-only builder: 64 segments, 64 classes", agg="avgpool", place_adv=("N", "N", "N")),
    "avg_da_T33_F200": _case(5, 4, 33, 264, 200, 9, "avgpool, general builder: RevGrad at all three levels", agg="avgpool"),
}
TRN_CASES = [n for n, c in CASES.items() if c["agg"] == "trn-m"]
AVG_CASES = [n for n, c in CASES.items() if c["agg"] == "avgpool"]

# what each trn-m case must land on: (has_fused_step, heads_vpw, FQ, PIPE, scalar loader operands)
EXPECT = {
    "odd_D37_F30": (True, 1, 1, False, True), "odd_D101_F67": (True, 1, 2, False, True), "T13_C63_F40": (True, 1, 1, True, False),
    "T25_C33": (True, 1, 1, True, False), "T33_C5": (True, 1, 1, True, False), "T63_rows": (True, 1, 1, True, False),
    "T64_C64": (True, 1, 1, True, False), "T64_C64_b190": (True, 1, 1, True, False), "C1": (True, 1, 4, False, False), "C2_F200": (True, 1, 4, False, False),
    "F1000": (True, 1, 16, False, False), "F2048": (True, 1, 32, False, False), "F2304_unfused": (False, None, None, None, False),
    "T64_two_per_wg": (True, 2, 1, True, False), "F2048_two_per_wg": (True, 2, 32, False, False),
}
# ... and between them they cover every instantiation of the heads kernel and both loader paths
assert {e[2] for e in EXPECT.values() if e[0]} == {1, 2, 4, 16, 32}      # (FQ 8, F 257..512, is the headline shape's: tested before)
assert {(e[1], e[3]) for e in EXPECT.values() if e[0]} == {(1, False), (1, True), (2, False), (2, True)}


def flags_of(case):
    if case["agg"] == "trn-m":
        return ALL_FLAGS
    return flags_from_options(case["place_adv"], "none", "none", "RevGrad", "uSv")


def make_plan(case, extra_flags=0):
    return _lib.Plan(case["Bs"], case["Bt"], case["T"], case["D"], case["F"], case["C"], flags_of(case) | extra_flags,
                     aggregation=_lib.AGG_AVGPOOL if case["agg"] == "avgpool" else _lib.AGG_TRN_M)


def plan_facts(plan):
    """What the plan says about the launches a case runs (see the module docstring)."""
    segs, tasks, phases, geom, _, _ = plan_arrays(plan)
    fused = [ph for ph in phases if ph.group == 4]
    facts = dict(has_fused_step=bool(plan.has_fused_step), n_rel=int(geom.n_rel), F=int(geom.F), C=int(geom.C),
                 heads_launches=sum(1 for ph in fused if ph.kind == PH_HEADS))
    if facts["heads_launches"]:
        vpw = int(geom.heads_vpw) or 1
        facts.update(vpw=vpw, fq=next(q for q in (1, 2, 4, 8, 16, 32) if q >= (geom.F + 63) // 64), pipe=geom.n_rel > 4 // vpw,
                     n_vid_wg=int(geom.n_vid_wg), n_frm_wg=int(geom.n_frm_wg), heads_rpw=int(geom.heads_rpw))
    # operands the fp32 loader of gemm_tiles moves element by element (ta3n_gemm_kernel.h, Loader::setup: 16-byte movability), per
    # GEMM launch of the step the engine runs (group 4 where the plan has it, else the forward and backward lists)
    scalar = []
    for ph in phases:
        if ph.kind != PH_GEMM or ph.group not in ((4,) if plan.has_fused_step else (0, 1, 2)):
            continue
        n = 0
        for ti in range(ph.task_begin, ph.task_begin + ph.task_count):
            t = tasks[ti]
            for si in range(t.seg_begin, t.seg_begin + t.seg_count):
                s = segs[si]
                for off, ld, km in ((s.a_off, s.a_ld, s.a_kmajor), (s.b_off, s.b_ld, s.b_kmajor)):
                    n += bool((off | ld | (0 if km else s.klen)) & 3)
        scalar.append(n)
    facts["scalar_operands_per_gemm_launch"] = scalar
    return facts


def assert_runs_what_it_claims(name, plan, check_loader=True):
    """check_loader=False: plans with bf16 twins, whose Segs address the twins in units of two elements."""
    case, (fused, vpw, fq, pipe, scalar) = CASES[name], EXPECT[name]
    f = plan_facts(plan)
    assert f["has_fused_step"] == fused == (case["F"] <= HEADS_MAX_F), (name, f)
    assert f["n_rel"] == case["T"] - 1 and f["F"] == min(case["F"], case["D"]) and f["C"] == case["C"], (name, f)
    if fused:
        assert f["heads_launches"] == 1 and (f["vpw"], f["fq"], f["pipe"]) == (vpw, fq, pipe), (name, f)
        assert f["vpw"] == (2 if case["Bs"] + case["Bt"] > 224 else 1)
        assert f["n_vid_wg"] == -(-(case["Bs"] + case["Bt"]) // vpw)
    # the scalar loader: in the shared-FC product (the step's first GEMM launch), the tuple products (its second) and the shared-FC weight
    # gradient (its last) at once - or in neither of the two forward products (a launch with the small head weight gradients has
    # operands with odd leading dimensions, C or 2, at any shape)
    per = f["scalar_operands_per_gemm_launch"]
    if not check_loader:
        return f
    assert len(per) >= 3, (name, f)
    assert (per[0] > 0 and per[1] > 0 and per[-1] > 0) if scalar else (per[0] == 0 and per[1] == 0), (name, f)
    return f


# ---- inputs ----
def oracle_cfg(case, arithmetic="fp32"):
    kw = dict(num_class=case["C"], num_segments=case["T"], feature_dim=case["D"], fc_dim=case["F"], dropout_i=0.0, dropout_v=0.0,
              arithmetic=arithmetic)
    if case["agg"] == "avgpool":      # as tests/test_gpu_adam.py: _oracle_cfg("avgpool"), with the case's adversarial levels
        kw.update(frame_aggregation="avgpool", place_adv=case["place_adv"], add_loss_DA="none", use_attn="none")
    return orc.Config(**kw)


def initial_params(case):
    return synth_state(orc.param_shapes(oracle_cfg(case)), seed=case["wseed"], scale=case["scale"])


def gamma_of(case):
    return GAMMA if case["agg"] == "trn-m" else 0.0


def batch(case, step):
    """(xs, xt, ys, n_src, n_tgt) of a step: the second step of a ragged case has dummy rows (zeros) behind the valid ones."""
    xs, xt, ys, _ = synth_batch(case["C"], case["T"], case["D"], case["Bs"], case["Bt"], seed=case["xseed"] + 7 * step)
    ns, nt = case["Bs"], case["Bt"]
    if step == 1 and case["ragged_second_step"]:
        ns, nt = ns - 3, nt - 5
        assert ns > 0 and nt > 0
    xs[ns:] = 0; xt[nt:] = 0
    return xs, xt, ys, ns, nt


def oracle_step(case, params, momentum, xs, xt, ys, ns, nt, dtype, masks=None, arithmetic="fp32"):
    """One oracle train step in `dtype` on the given fp32 parameters and inputs: (result, state after the step)."""
    cast = lambda t: t.detach().cpu().to(dtype).clone()
    state = orc.TrainState(params={k: cast(v) for k, v in params.items()}, lr=LR)
    state.momentum = {k: cast(v) for k, v in (momentum or {}).items()}
    res = orc.train_step(state, cast(xs), cast(xt), ys, BETA, gamma_of(case), oracle_cfg(case, arithmetic), clip=CLIP, n_src=ns, n_tgt=nt,
                         masks=masks)
    return res, state


def relu_patterns(res):
    """The on/off patterns of a run's ReLUs, in the form train_step(masks=...) takes."""
    return tuple({k: v.detach() > 0 for k, v in res[dom]["hidden"].items()} for dom in ("src", "tgt"))


@functools.lru_cache(maxsize=None)
def float64_reference(name, step=0):
    """The float64 oracle on the case's fp32 inputs, free-running (its own ReLU patterns).  Computed once per process and shared: treat
    the result as read-only.  Step 1 starts from the parameters and momentum step 0 left, rounded to fp32 as an engine would hold them."""
    case = CASES[name]
    torch.set_num_threads(min(8, torch.get_num_threads()))
    if step == 0:
        params, momentum = initial_params(case), {}
    else:
        _, st = float64_reference(name, step - 1)
        params, momentum = {k: v.float() for k, v in st.params.items()}, {k: v.float() for k, v in st.momentum.items()}
    xs, xt, ys, ns, nt = batch(case, step)
    res, state = oracle_step(case, params, momentum, xs, xt, ys, ns, nt, torch.float64)
    return dict(res=res, params=params, momentum=momentum, batch=(xs, xt, ys, ns, nt)), state


# ---- comparisons ----
LOGIT_KEYS = (("out", lambda r: r["out"]), ("pred_rel", lambda r: r["pred_domain"][0]), ("pred_vid", lambda r: r["pred_domain"][1]),
              ("pred_frm", lambda r: r["pred_domain"][2]))


def oracle_logits(res, ns, nt, keys=LOGIT_KEYS):
    """{key: [valid source rows; valid target rows]} in float64."""
    return {k: torch.cat((pick(res["src"])[:ns], pick(res["tgt"])[:nt]), 0).detach().double() for k, pick in keys}


def oracle_loss_scalars(case, res, ns, nt):
    """The six scalars the step logs - total, classification, the adversarial cross-entropy per level (relation, video, frame),
    attentive entropy - from an oracle result (which keeps the three adversarial terms as one sum)."""
    import torch.nn.functional as F
    parts = {k: float(v) for k, v in res["parts"].items()}
    out = dict(loss=parts["loss"], loss_c=parts["loss_c"], loss_e=parts.get("loss_e", 0.0))
    for l, key in enumerate(("loss_adv_rel", "loss_adv_vid", "loss_adv_frm")):
        out[key] = 0.0
        if case["place_adv"][l] == "Y":
            ps, pt = res["src"]["pred_domain"][l][:ns].reshape(-1, 2), res["tgt"]["pred_domain"][l][:nt].reshape(-1, 2)
            lab = torch.cat((torch.zeros(ps.size(0)), torch.ones(pt.size(0)))).long()
            out[key] = float(F.cross_entropy(torch.cat((ps, pt), 0).detach(), lab))
    total_adv = out["loss_adv_rel"] + out["loss_adv_vid"] + out["loss_adv_frm"]
    assert abs(total_adv - parts.get("loss_a", 0.0)) <= 1e-6 * max(1.0, abs(total_adv))
    return out


def logit_bound(want):
    """tolerances.py states LOGIT_ATOL as "1e-3 at O(1..10) logits": read relatively, since the logits grow with the relation count
    (about 230 at 64 segments on trained-scale weights, where 1e-3 is below fp32 resolution of a K = 2048 sum)."""
    return tol.LOGIT_ATOL * max(1.0, float(want.abs().max()) / 10.0)


def rel_l2_per_tensor(got, want):
    """{name: relative L2} over the tensors of `want`; where the reference tensor is exactly zero (the classifier gradients of a
    single-class model) the entry is None and the caller bounds max |got| by F32_ATOL instead."""
    out = {}
    for k, w in want.items():
        w = w.detach().double().cpu()
        g = got[k].detach().double().cpu().reshape(w.shape)
        out[k] = None if not bool(w.any()) else ((g - w).pow(2).sum().sqrt() / w.pow(2).sum().sqrt()).item()
    return out


def assert_gradients(name, step, got, want, bound, median_bound=None):
    """Every tensor within `bound` (exactly-zero reference tensors: max |got| <= F32_ATOL), the median within `median_bound`.
    Returns (worst, median, {tensor: rel. L2}) over the tensors with a non-zero reference."""
    per = rel_l2_per_tensor(got, want)
    for k, v in per.items():
        if v is None:
            assert float(got[k].detach().double().abs().max()) <= tol.F32_ATOL, (name, step, k)
        else:
            assert v <= bound, (name, step, k, v)
    vals = {k: v for k, v in per.items() if v is not None}
    med = float(np.median(list(vals.values())))
    if median_bound is not None:
        assert med <= median_bound, (name, step, med)
    return max(vals.values()), med, vals


# ---- the plan interpreter on a case ----
def interp_hyper(case, ns, nt):
    T = case["T"]
    return dict(beta=BETA, gamma=gamma_of(case), lr=LR, momentum=0.9, weight_decay=1e-4, clip=CLIP, p_drop_i=0.0, p_drop_v=0.0, seed_i=1,
                seed_v=2, inv_n_cls=1.0 / ns, inv_n_rel=1.0 / ((ns + nt) * max(T - 1, 1)), inv_n_vid=1.0 / (ns + nt),
                inv_n_frm=1.0 / ((ns + nt) * T), inv_n_ent=1.0 / (ns + nt), valid_source=ns, valid_target=nt, train=1)


def interp_step(case, plan, params, xs, xt, ys, ns, nt, fused):
    """The plan's launch lists executed in float64 numpy: (gradients by name, interpreter)."""
    it = Interp(plan)
    it.set_params(params)
    it.X = torch.cat((xs, xt), 0).double().numpy().reshape(-1)
    it.labels[:case["Bs"]] = ys.numpy()
    it.hy = interp_hyper(case, ns, nt)
    it.G[:] = 0
    for group in ((4,) if fused else (0, 1, 2)):
        it.run_group(group)
    return it.get_params(it.G), it
