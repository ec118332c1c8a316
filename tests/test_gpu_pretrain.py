"""GPU: --pretrain_source (reference main.py:388-414) - ta3n_sgd_live, the engine's source-only pass on the step's parameter layout against
the fixtures the reference's own main.train wrote (tests/golden/make_golden_pretrain.py), bf16 twins across the two workspaces, and
main.py with --pretrain_source / --lr_adaptive loss on the fast path and on the module path.

bf16 twins against fp32 (test_bf16_twins_*; profiles/pretrain_parity.txt), one iteration from the same parameters at the tiny_pre_T5 shape,
deviation = ||dP_bf16 - dP_fp32||_2 / ||dP_fp32||_2 over the flat live prefix, measured on one MI355X: the plain bf16 step 2.22e-2, pass + step
2.78e-2, under the bound of 2 x the plain step's, 4.44e-2."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fixture_t7 import make_dataset
from golden_util import Golden, case_config, step_schedule
from test_pretrain_cpu import TA3N, fixture_flags, reached
from ta3n_amd import _lib, tolerances as tol
from ta3n_amd.engine import PRETRAIN_DROPPED_FLAGS
from ta3n_amd.synthetic import synth_batch, synth_state
from weighted_loss_cases import log_numbers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 4, 5, 512, 64, 12)                     # the fixtures' shape
FIXTURES = ["tiny_pre_T5", "tiny_pre_T2", "tiny_pre_noattn", "tiny_pre_clip", "tiny_pre_short", "tiny_pre_sv_wcls", "tiny_avgpool_pre"]
TWINS = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
LR, MU, WD = 3e-3, 0.9, 1e-4


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buffers:
    """Flat buffers of one plan with reproducible contents: parameters, gradients, momentum (all param_floats long), workspace."""

    def __init__(self, plan, seed=5):
        gen = torch.Generator().manual_seed(seed)
        n = plan.param_floats
        self.plan = plan
        self.P, self.G, self.M = (torch.randn(n, generator=gen).mul_(s).cuda() for s in (0.1, 0.02, 0.05))
        self.ws = torch.zeros(plan.ws_floats, device="cuda")
        _lib.check(_lib.lib().ta3n_init_workspace(plan.handle, self.ws.data_ptr(), _stream()))
        if "sumsq" in plan.regions:                # what a fused step would leave: one partial per gradient tile
            off, k = plan.region("sumsq")
            self.ws[off:off + k] = torch.rand(k, generator=gen).mul_(0.3).cuda()

    def region(self, name):
        off, n = self.plan.region(name)
        return self.ws[off:off + n]

    def live(self, fused_norm, clip):
        _lib.check(_lib.lib().ta3n_sgd_live(self.plan.handle, self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.ws.data_ptr(),
                                            int(fused_norm), LR, MU, WD, float(clip), _stream()), "ta3n_sgd_live")

    def range(self, fused_norm, clip):
        _lib.check(_lib.lib().ta3n_sgd_range(self.plan.handle, self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.ws.data_ptr(),
                                             0, self.plan.live_floats, int(fused_norm), LR, MU, WD, float(clip), _stream()), "ta3n_sgd_range")


def _twin_bits(b):
    n = b.plan.param_floats
    return b.region("p16").view(torch.int16)[:n]


@pytest.mark.parametrize("flags", [TA3N, TA3N | TWINS])
@pytest.mark.parametrize("fused_norm", [0, 1])
@pytest.mark.parametrize("clip", [0.0, 0.05])
def test_sgd_live_is_sgd_range_over_the_prefix_on_a_plain_plan(flags, fused_norm, clip):
    plan = _lib.Plan(*SHAPE, flags)
    assert plan.live_ranges == [(0, plan.live_floats)]
    a, b = Buffers(plan), Buffers(plan)
    a.live(fused_norm, clip)
    b.range(fused_norm, clip)
    torch.cuda.synchronize()
    assert torch.equal(a.P, b.P) and torch.equal(a.M, b.M) and torch.equal(a.region("grad_norm")[:2], b.region("grad_norm")[:2])
    assert bool((a.P != Buffers(plan).P)[:plan.live_floats].any()) and (clip == 0.0 or float(a.region("grad_norm")[1]) < 1.0)
    if flags & TWINS:
        assert torch.equal(_twin_bits(a), _twin_bits(b))


def _fma(a, b, c):
    """a b + c with one rounding to fp32 (a fused multiply-add): the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


@pytest.mark.parametrize("flags,layout", [(_lib.FLAG_TRANS_ATTN, TA3N), (0, TA3N), (_lib.FLAG_TRANS_ATTN | TWINS, TA3N | TWINS)])
@pytest.mark.parametrize("fused_norm", [0, 1])
@pytest.mark.parametrize("clip", [0.0, 0.05])
def test_sgd_live_on_a_source_only_plan(flags, layout, fused_norm, clip):
    """Bit-equal to clip + Nesterov restated in torch over the ranges (fp32 values, every multiply-add of the rule rounded once, as the kernel's
    fmaf; the coefficient from the recorded norm by the kernel's expression), nothing outside the ranges touched, the norm blind to what
    the gradient buffer holds outside them."""
    plan = _lib.Plan(*SHAPE, flags, layout_flags=layout)
    b = Buffers(plan)
    inside = torch.zeros(plan.param_floats, dtype=torch.bool, device="cuda")
    for lo, hi in plan.live_ranges:
        inside[lo:hi] = True
    assert 2 < len(plan.live_ranges) and int(inside.sum()) < plan.live_floats
    b.G[~inside] = 1e6                                   # garbage where the pass does not reach
    p0, m0, g = b.P.clone(), b.M.clone(), b.G.clone()
    tw0 = _twin_bits(b).clone() if flags & TWINS else None
    b.live(fused_norm, clip)
    torch.cuda.synchronize()
    norm, coef = (float(v) for v in b.region("grad_norm")[:2])
    want_norm = (float(b.region("sumsq").double().sum().sqrt()) if fused_norm else float(g[inside].double().norm()))
    assert abs(norm - want_norm) <= 1e-5 * want_norm, (norm, want_norm)
    want_coef = float(min(np.float32(clip) / (np.float32(norm) + np.float32(1e-6)), np.float32(1.0))) if clip > 0 else 1.0
    assert coef == want_coef and (clip == 0.0 or coef < 1.0)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")      # noqa: E731
    gs = g * f(coef)
    d = _fma(f(WD), p0, gs)
    m = _fma(f(MU), m0, d)
    d = _fma(f(MU), m, d)
    p = _fma(-f(LR), d, p0)
    assert torch.equal(b.P[inside], p[inside]) and torch.equal(b.M[inside], m[inside])
    assert torch.equal(b.P[~inside], p0[~inside]) and torch.equal(b.M[~inside], m0[~inside]) and torch.equal(b.G, g)
    if flags & TWINS:      # the twins of the new values, and only of those
        tw = _twin_bits(b)
        assert torch.equal(tw[inside], b.P[inside].to(torch.bfloat16).view(torch.int16)) and torch.equal(tw[~inside], tw0[~inside])


def test_prefix_updates_refuse_a_plan_on_another_layout():
    plan = _lib.Plan(*SHAPE, _lib.FLAG_TRANS_ATTN, layout_flags=TA3N)
    b = Buffers(plan)
    p0 = b.P.clone()
    with pytest.raises(ValueError, match="ta3n_sgd_range: this plan lies on another plan's parameter layout"):
        b.range(0, 0.0)
    L = _lib.lib()
    assert L.ta3n_has_pipelined_step(plan.handle) == 0 and L.ta3n_has_fused_step(plan.handle) == 1
    assert L.ta3n_sgd_step(plan.handle, b.P.data_ptr(), b.G.data_ptr(), b.M.data_ptr(), b.ws.data_ptr(), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(b.P, p0)


def _engine(g, c, **kw):
    from ta3n_amd.engine import TrainEngine
    flags, agg = fixture_flags(g, c)
    cw = g.meta("class_w")
    cw = None if np.all(cw == cw[0]) else [float(v) for v in cw]
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc_dim"], c["C"], flags=flags, dropout_i=0.0, dropout_v=0.0, clip=c["clip"],
                      aggregation=c["agg"], class_weights=cw, **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=c["wseed"], scale=c["wscale"]))
    return eng


def _set_batch(eng, c, st):
    xs, xt, ys, yt = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=st["xseed"])
    xs[st["n_src"]:] = 0; xt[st["n_tgt"]:] = 0
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda(), **(dict(target_label=yt.cuda()) if eng.target_labels else {}))


class _StopAfterPass(Exception):
    pass


@pytest.mark.parametrize("name", FIXTURES)
def test_engine_follows_the_reference_trajectory(name):
    """Three iterations of pass + step in fp32: the parameters after every pass and after every step, the step's logged losses and clipped
    gradients, at the bounds of ta3n_amd/tolerances.py; what the pass does not reach is bit-unchanged across it, momentum included."""
    g = Golden(name)
    c = case_config(g)
    eng = _engine(g, c, pretrain_source=True)
    assert "pretrain_source" in eng.describe() and eng.plan_pre.cfg.flags == eng._flags & ~PRETRAIN_DROPPED_FLAGS
    pre_live, live = set(str(k) for k in g.meta("pre_live")), set(eng.live_names())
    assert reached(eng.plan_pre) == pre_live and live == set(str(k) for k in g.meta("live"))
    inside = torch.zeros(eng.plan.param_floats, dtype=torch.bool, device="cuda")
    for lo, hi in eng.plan_pre.live_ranges:
        inside[lo:hi] = True
    gamma = 0.0 if c["agg"] == "avgpool" else 0.003
    log = str(g.meta("log")).strip().splitlines()
    enqueue = eng._enqueue_step
    for s, st in enumerate(step_schedule(c)):
        _set_batch(eng, c, st)
        p0, m0 = eng.P.clone(), eng.M.clone()
        kw = dict(valid_source=st["n_src"], valid_target=st["n_tgt"])

        def stop():
            raise _StopAfterPass
        eng._enqueue_step = stop                         # the pass alone first: train_step runs it, then would enqueue the step
        with pytest.raises(_StopAfterPass):
            eng.train_step([0.75, 0.75, 0.5], gamma, st["lr"], **kw)
        torch.cuda.synchronize()
        assert torch.equal(eng.P[~inside], p0[~inside]) and torch.equal(eng.M[~inside[:eng.M.numel()]], m0[~inside[:eng.M.numel()]])
        assert not torch.equal(eng.P[inside], p0[inside])
        for k, v in eng.param_views().items():
            if k in pre_live:
                g.check(f"step{s}/pre/param/{k}", v.cpu(), tol.F32_RTOL, tol.F32_ATOL)
        assert eng.pretrain_losses()["loss_c"] > 0 and eng.pretrain_losses()["loss"] == eng.pretrain_losses()["loss_c"]
        eng._enqueue_step = enqueue                      # ... then the step proper on the parameters the pass left
        eng.pretrain_source = False
        try:
            eng.train_step([0.75, 0.75, 0.5], gamma, st["lr"], **kw)
        finally:
            eng.pretrain_source = True
        torch.cuda.synchronize()
        Lg = eng.losses()
        got = dict(Loss=Lg["loss"], loss_c=Lg["loss_c"], loss_a=Lg["loss_adv_rel"] + Lg["loss_adv_vid"] + Lg["loss_adv_frm"], loss_e=Lg["loss_e"])
        for k, w in log_numbers(log[s]).items():
            assert abs(got[k] - w) <= 2e-4 * max(1.0, abs(w)), (name, s, k, got[k], w)
        coef = eng.region("grad_norm")[1].item()
        grads = eng.param_views(eng.G)
        for k, v in eng.param_views().items():
            if k in live:
                assert g.rel_l2(f"step{s}/clipped_grad/{k}", grads[k].cpu() * coef) <= tol.F32_GRAD_REL_L2 * tol.GOLDEN_DRIFT_FACTOR, (name, s, k)
            g.check(f"step{s}/param/{k}", v.cpu(), tol.F32_RTOL, tol.F32_ATOL)


def test_one_call_runs_pass_then_step():
    """train_step() with the pass = the pass alone followed by the plain step, bit for bit (what the trajectory test takes apart)."""
    g = Golden("tiny_pre_T5")
    c = case_config(g)
    st = step_schedule(c)[0]
    whole, parts = _engine(g, c, pretrain_source=True), _engine(g, c, pretrain_source=True)
    for eng in (whole, parts):
        _set_batch(eng, c, st)
    whole.train_step([0.75, 0.75, 0.5], 0.003, st["lr"])
    parts.set_hyper([0.75, 0.75, 0.5], 0.003, st["lr"])
    parts._pretrain_pass(st["lr"], None)
    parts._enqueue_step()
    torch.cuda.synchronize()
    assert torch.equal(whole.P, parts.P) and torch.equal(whole.M, parts.M)
    for call in (lambda: whole.capture(), lambda: whole.train_steps([([0.75, 0.75, 0.5], 0.003, 1e-3)]),
                 lambda: whole.train_step_pipelined([0.75, 0.75, 0.5], 0.003, 1e-3)):
        with pytest.raises(NotImplementedError, match="pretrain_source together with"):
            call()


def _one_iteration(g, c, st, pretrain, bf16, force_refresh=False):
    eng = _engine(g, c, pretrain_source=pretrain, **(dict(bf16=True, bf16_store=True) if bf16 else {}))
    _set_batch(eng, c, st)
    p0 = eng.P.clone()
    if force_refresh:      # ta3n_refresh_bf16 of parameters AND input in front of each pass, in the workspace that pass reads
        L, X, P = eng._L, eng.X.data_ptr(), eng.P.data_ptr()
        eng.set_hyper([0.75, 0.75, 0.5], 0.003, st["lr"])
        _lib.check(L.ta3n_refresh_bf16(eng.plan_pre.handle, X, P, eng.ws_pre.data_ptr(), _stream()))
        eng._pretrain_pass(st["lr"], None)
        _lib.check(L.ta3n_refresh_bf16(eng.plan.handle, X, P, eng.ws.data_ptr(), _stream()))
        eng._enqueue_step()
    else:
        eng.train_step([0.75, 0.75, 0.5], 0.003, st["lr"])
    torch.cuda.synchronize()
    return eng, (eng.P - p0)[:eng.plan.live_floats].double()


def test_bf16_twins_across_the_two_workspaces():
    g = Golden("tiny_pre_T5")
    c = case_config(g)
    st = step_schedule(c)[0]
    eng, d16 = _one_iteration(g, c, st, True, True)
    forced, _ = _one_iteration(g, c, st, True, True, force_refresh=True)
    assert torch.equal(eng.P, forced.P) and torch.equal(eng.M, forced.M)                  # every pass read twins of the current values
    n = eng.plan.param_floats
    assert torch.equal(eng.region("p16").view(torch.int16)[:n], eng.P.to(torch.bfloat16).view(torch.int16))      # ... and the step's are current after it
    _, d32 = _one_iteration(g, c, st, True, False)
    _, plain16 = _one_iteration(g, c, st, False, True)
    _, plain32 = _one_iteration(g, c, st, False, False)
    dev_plain = float((plain16 - plain32).norm() / plain32.norm())
    dev_pre = float((d16 - d32).norm() / d32.norm())
    print(f"[pretrain parity] bf16 twins against fp32, one iteration at {SHAPE}: plain step {dev_plain:.2e}, pass + step {dev_pre:.2e} "
          f"(bound 2 x plain = {2 * dev_plain:.2e})")
    # (profiles/pretrain_parity.txt is this, as one MI355X printed it)
    print(f"bf16 twins against fp32, one iteration from the same parameters, shape {SHAPE}, ||dP_bf16 - dP_fp32|| / ||dP_fp32|| over the live prefix\n"
          f"plain step {dev_plain:.3e}\npass + step {dev_pre:.3e}\nbound (2 x plain step: two updates per iteration) {2 * dev_plain:.3e}")
    assert 0 < dev_plain and dev_pre <= 2 * dev_plain, (dev_pre, dev_plain)


OPTS = ["--baseline_type", "video", "--frame_aggregation", "trn-m", "--use_target", "uSv", "--adv_DA", "RevGrad", "--use_attn", "TransAttn",
        "--add_loss_DA", "attentive_entropy", "--beta", "0.75", "0.75", "0.5", "--gamma", "0.003"]
COMMON = ["--arch", "resnet18", "--num_segments", "5", "--fc_dim", "64", "-b", "8", "6", "8", "-j", "0", "--print_freq", "1", "--no_partialbn"]
NUM = re.compile(r"(Prec@1|Prec@5|Loss|loss_c|loss_a|loss_e|lr:) (-?[0-9.]+)")


def _main(data, exp, tmp_path, fast, extra):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), data[0], "RGB", data[1], data[2], data[3], "--exp_path", exp + "/", *OPTS, *COMMON,
           *extra, "--save_best_log", str(tmp_path / f"best{fast}.log")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, TA3N_MAIN_FAST=fast))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_own_main_pretrain_source_fast_path_logs_what_the_module_path_logs(tmp_path):
    data = make_dataset(str(tmp_path / "data"))
    extra = ["--pretrain_source", "--lr_adaptive", "dann", "--lr", "0.03", "--epochs", "2", "--dropout_i", "0.5", "--dropout_v", "0.5", "--save_model"]
    outs, cks = [], []
    for fast in ("1", "0"):
        exp = str(tmp_path / f"exp{fast}")
        r = _main(data, exp, tmp_path, fast, extra)
        said = [ln for ln in r.stdout.splitlines() if ln.startswith("[ta3n]") and "pretrain_source" in ln]
        assert bool(said) == (fast == "1"), r.stdout[-2000:]
        outs.append([ln for ln in open(exp + "/RGB/train.log") if ln.startswith("Train:")])
        cks.append(torch.load(exp + "/RGB/checkpoint.pth.tar", map_location="cpu", weights_only=False))
    print("# train.log of main.py --pretrain_source with the engine's pass (TA3N_MAIN_FAST=1), then on the module path (=0)\n" +
          "".join(outs[0]) + "# ----\n" + "".join(outs[1]))
    assert len(outs[0]) == len(outs[1]) == 6      # 2 epochs x ceil(24 / 8) steps, print_freq 1
    for a, b in zip(*outs):
        fa, fb = NUM.findall(a), NUM.findall(b)
        assert [k for k, _ in fa] == [k for k, _ in fb] and {"Prec@1", "Loss", "loss_c", "loss_a", "loss_e"} <= {k for k, _ in fa}
        for (k, x), (_, y) in zip(fa, fb):
            assert abs(float(x) - float(y)) <= 2e-4 * max(1.0, abs(float(y))), (k, x, y, a, b)
    sds = [{k: v.double() for k, v in ck["state_dict"].items() if v.dtype.is_floating_point} for ck in cks]
    assert set(sds[0]) == set(sds[1])
    for k in sds[0]:
        err = (sds[0][k] - sds[1][k]).abs()
        assert bool((err <= tol.F32_ATOL + tol.F32_RTOL * sds[1][k].abs()).all()), (k, float(err.max()))
    for ck in cks:      # the momentum buffers travel: every parameter either path trained has one
        assert len(ck["optimizer"]["state"]) == len(cks[1]["optimizer"]["state"])


def test_own_main_lr_adaptive_loss_follows_the_logged_class_loss(tmp_path):
    """Four epochs; train_short.log holds each epoch's last line, whose loss_c is the epoch's losses_c.avg - the statistic of the rule
    (reference main.py:233-234, 246-248, 794-798) - and whose lr is the epoch's: lr /= lr_decay exactly where the epoch before raised it."""
    data = make_dataset(str(tmp_path / "data"))
    extra = ["--lr_adaptive", "loss", "--lr", "0.5", "--lr_decay", "2", "--epochs", "4", "--dropout_i", "0", "--dropout_v", "0"]
    _main(data, str(tmp_path / "exp"), tmp_path, "1", extra)
    lines = [ln for ln in open(str(tmp_path / "exp") + "/RGB/train_short.log") if ln.startswith("Train:")]
    print("".join(lines))
    assert len(lines) == 4
    lr, current, previous = 0.5, 999.0, 999.0
    for ln in lines:
        num = dict(NUM.findall(ln))
        if current > previous:
            lr /= 2
        assert abs(float(num["lr:"]) - lr) <= 5.1e-6, (ln, lr)      # (logged to five decimals)
        previous, current = current, float(num["loss_c"])
