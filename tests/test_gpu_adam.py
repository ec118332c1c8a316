"""GPU: --optimizer Adam on the engine (include/ta3n_hip.h: ta3n_adam_range / ta3n_adam_step_next / ta3n_train_steps_adam).

The yardstick of the arithmetic tests is the reference's own fp32 error: clip_grad_norm_ + torch.optim.Adam on the CPU, once in fp32
and once in float64, on the SAME gradients the kernel sees.  For each of P, exp_avg, exp_avg_sq
    max |gpu - f64|  <=  4 x max |torch fp32 - f64|.
Why 4: two legitimate fp32 evaluation orders of this recurrence (200 k elements, 10 steps, gradients spanning 1e-9 .. 1) sat at 1.0 x,
2.6 x and 0.94 x of torch's distance for the three buffers on a CPU; 4 leaves room above 2.6.  The measured ratios are printed.
Parameters are never compared element by element against a free-running second implementation: Adam's first steps move every element
by about lr * sign(g), so an element whose gradient is below the fp32 summation-order floor differs by 2 lr between any two correct
implementations (gradient parity itself: test_gpu_gradients.py).  The loss trajectory is compared against the oracle instead."""
import os

import numpy as np
import pytest
import torch

from oracle import ta3n_oracle as orc
from ta3n_amd import tolerances as tol
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

CFG = dict(C=12, T=5, D=512, fc=128, Bs=12, Bt=8)      # the small shape of test_gpu_ddp_engine.py
LR, WD, BOUND = 1e-3, 1e-4, 4.0
BETA, GAMMA = [0.75, 0.75, 0.5], 0.003


def _engine(optimizer="Adam", **kw):
    from ta3n_amd.engine import TrainEngine
    c = CFG
    kw.setdefault("weight_decay", WD)
    eng = TrainEngine(c["Bs"], c["Bt"], c["T"], c["D"], c["fc"], c["C"], dropout_i=0.0, dropout_v=0.0, optimizer=optimizer, **kw)
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=3))
    return eng


def _batch(eng, seed=9):
    c = CFG
    xs, xt, ys, _ = synth_batch(c["C"], c["T"], c["D"], c["Bs"], c["Bt"], seed=seed)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    return xs, xt, ys


def _real_mask(eng):
    """True at the floats of the live prefix that belong to a parameter (the rest is alignment padding)."""
    mask = torch.zeros(eng.plan.live_floats, dtype=torch.bool)
    for _, off, shape, live in eng.plan.params:
        if live:
            mask[off:off + int(np.prod(shape))] = True
    return mask


def _cpu_adam(p0, grads, lrs, wd, clip, dtype, betas=(0.9, 0.999), eps=1e-8):
    """clip_grad_norm_ + torch.optim.Adam (main.py:86, 578-583) over the flat prefix in `dtype`: (P, exp_avg, exp_avg_sq, [norms])."""
    p = torch.nn.Parameter(p0.detach().cpu().to(dtype).clone())
    opt = torch.optim.Adam([p], lrs[0], betas=betas, eps=eps, weight_decay=wd)
    norms = []
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.detach().cpu().to(dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], clip if clip > 0 else float("inf"))))
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], norms


def _assert_within_torch_fp32_error(eng, p0, grads, lrs, clip, what):
    n = eng.plan.live_floats
    r32 = _cpu_adam(p0, grads, lrs, eng.weight_decay, clip, torch.float32, eng.betas, eng.eps)
    r64 = _cpu_adam(p0, grads, lrs, eng.weight_decay, clip, torch.float64, eng.betas, eng.eps)
    torch.cuda.synchronize()
    ratios = {}
    for name, gpu, a32, a64 in zip(("P", "exp_avg", "exp_avg_sq"), (eng.P[:n], eng.M, eng.V), r32, r64):
        ours = (gpu.detach().cpu().double() - a64).abs().max().item()
        torchs = (a32.double() - a64).abs().max().item()
        ratios[name] = ours / torchs
        print(f"[adam {what}] {name}: max|gpu - f64| = {ours:.3e}, max|torch fp32 - f64| = {torchs:.3e}, ratio {ours / torchs:.2f}")
    assert eng.adam_step_count == len(grads)
    for name, r in ratios.items():
        assert r <= BOUND, (what, name, ratios)
    return r32, ratios


# ---- 1. the update arithmetic, every element ----
@pytest.mark.parametrize("clipped", [False, True])
def test_update_matches_torch_adam_within_its_own_fp32_error(clipped):
    steps = 10
    eng = _engine(clip=0.0)
    n, mask = eng.plan.live_floats, _real_mask(eng)
    assert (n // 4) % 256 != 0 and n // 4 > 256      # several workgroups, the last one partly idle: the tail path runs
    gen = torch.Generator().manual_seed(11)
    scale = torch.logspace(-9, 0, n)[torch.randperm(n, generator=gen)]
    grads = []
    for k in range(steps):
        g = torch.randn(n, generator=gen) * scale * mask
        if k == 3:
            g[::7] = 0.0
        grads.append(g)
    clip = 0.5 * float(grads[0].norm()) if clipped else 0.0
    eng.clip = clip
    p0 = eng.P[:n].detach().cpu().clone()
    norms_gpu = []
    for g in grads:
        eng.G[:n].copy_(g.cuda())
        eng.adam_step(LR, fused_norm=0)
        norms_gpu.append(eng.region("grad_norm")[:2].tolist())
    (_, _, _, norms), _ = _assert_within_torch_fp32_error(eng, p0, grads, [LR] * steps, clip, f"synthetic clipped={clipped}")
    for (gn, coef), want in zip(norms_gpu, norms):
        assert abs(gn - want) <= tol.F32_RTOL * want
        assert (coef < 1.0) == clipped and (not clipped or abs(coef - clip / (want + 1e-6)) <= tol.F32_RTOL)
    pad = ~mask
    for buf in (eng.P[:n], eng.M, eng.V):
        assert not bool(buf.detach().cpu()[pad].any())      # alignment padding inside the prefix stays exactly 0
    assert float(eng.V.min()) >= 0.0 and bool(torch.isfinite(eng.P).all())


# ---- 2. composition is bit-exact ----
def _synthetic_grad(eng, seed=5):
    n = eng.plan.live_floats
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * _real_mask(eng)
    eng.G[:n].copy_(g.cuda())


def test_two_ranges_equal_one_whole_prefix_call():
    whole, split = _engine(clip=1.0), _engine(clip=1.0)
    n, first = whole.plan.live_floats, whole._n_first
    assert 0 < first < n and first % 4 == 0
    for step in (1, 2):
        for eng in (whole, split):
            _synthetic_grad(eng, seed=step)
        whole.adam_range(0, n, LR, fused_norm=0, step=step)
        split.adam_range(0, first, LR, fused_norm=0, step=step)
        split.adam_range(first, n, LR, fused_norm=0, step=step)
    torch.cuda.synchronize()
    assert torch.equal(whole.P, split.P) and torch.equal(whole.M, split.M) and torch.equal(whole.V, split.V)
    assert torch.equal(whole.region("grad_norm")[:2], split.region("grad_norm")[:2]) and float(whole.region("grad_norm")[1]) < 1.0
    assert float(whole.M.abs().max()) > 0


def _state(eng):
    eng.flush()
    torch.cuda.synchronize()
    return eng.P.clone(), eng.M.clone(), eng.V.clone(), eng.adam_step_count


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("n_steps", [3, 6])      # 6: train_steps splits its schedule into pieces, each opening with the pending update
def test_train_steps_equal_pipelined_steps_equal_single_steps(n_steps):
    sched = [(BETA, GAMMA, LR * (1.0 - 0.1 * k)) for k in range(n_steps)]

    def run(how, unfused_norm):
        eng = _engine(clip=0.05)      # below the gradient norm of this batch: coef < 1 on every step
        eng.force_unfused_norm = unfused_norm
        _batch(eng)
        if how == "steps":
            assert eng.can_batch_steps()
            eng.train_steps(sched)
        else:
            for b, g, lr in sched:
                (eng.train_step_pipelined if how == "pipelined" else eng.train_step)(b, g, lr)
        out = _state(eng)
        assert float(eng.region("grad_norm")[1]) < 1.0 and out[3] == n_steps
        return out
    assert _same(run("steps", False), run("pipelined", False))      # the norm from the fused step's partials on both sides
    assert _same(run("pipelined", True), run("single", True))       # the norm from the gradient-norm pass on both sides
    assert _same(run("steps", True), run("single", True))


def test_deferred_steps_equal_single_steps():
    def run(deferred):
        eng = _engine()
        eng.force_unfused_norm = True
        _batch(eng)
        for k in range(3):
            (eng.train_step_deferred if deferred else eng.train_step)(BETA, GAMMA, LR)
        return _state(eng)
    assert _same(run(True), run(False))


def test_checkpoint_resume_continues_the_uninterrupted_run(tmp_path):
    from ta3n_amd import checkpoint as ckpt
    from ta3n_amd.models import VideoModel
    c = CFG
    model = VideoModel(c["C"], "video", "trn-m", "RGB", train_segments=c["T"], val_segments=c["T"], base_model="resnet18", fc_dim=c["fc"],
                       verbose=False)
    full, first = _engine(), _engine()
    for eng in (full, first):
        _batch(eng)
    for k in range(4):
        full.train_step(BETA, GAMMA, LR)
    for k in range(2):
        first.train_step(BETA, GAMMA, LR)
    path = ckpt.save_checkpoint(ckpt.engine_checkpoint(first, model, 1, "resnet18", LR, 0.0, 0.0), False, str(tmp_path))
    ck = torch.load(path, map_location="cpu", weights_only=False)
    opt = torch.optim.Adam(model.parameters(), 0.1)
    opt.load_state_dict(ck["optimizer"])      # main.py:104
    live = set(first.live_names())
    for name, p in model.named_parameters():
        assert (name in live) == (p in opt.state and len(opt.state[p]) > 0)
        if name in live:
            assert float(opt.state[p]["step"]) == 2.0
    second = _engine()
    second.M.fill_(1.0); second.V.fill_(1.0)      # whatever was there is replaced, the alignment padding included
    st = ckpt.load_into_engine(second, model, ck, resume_hp=True)
    assert st["lr"] == LR and second.adam_step_count == 2
    _batch(second)
    second.step_count = 2
    for k in range(2):
        second.train_step(BETA, GAMMA, LR)
    assert _same(_state(second), _state(full))
    sgd = _engine(optimizer="SGD")
    with pytest.raises(ValueError, match="Adam"):
        ckpt.load_into_engine(sgd, model, ck, resume_hp=True)


# ---- 3. bf16 twins ----
@pytest.mark.parametrize("mode", ["bf16", "f32x3"])
def test_update_keeps_the_parameter_twins_current(mode):
    eng = _engine(bf16=True, bf16_store=True) if mode == "bf16" else _engine(f32_split=True, bf16_store=True)
    names = ["p16"] + (["p16_lo"] if mode == "f32x3" else [])
    assert all(k in eng.plan.regions for k in names)
    for step in (1, 2):
        _synthetic_grad(eng, seed=step)
        eng.adam_step(LR, fused_norm=0)
    before = {k: eng.region(k).clone() for k in names}
    eng.refresh_bf16(params=True)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(before[k].view(torch.int32), eng.region(k).view(torch.int32)), k
    lo, n = eng.plan.region("p16")
    hi16 = eng.ws[lo:lo + n].view(torch.bfloat16)[: eng.plan.live_floats]
    assert torch.equal(hi16, eng.P[: eng.plan.live_floats].to(torch.bfloat16))      # and the twin IS the rounded parameter


# ---- 4. / 5. the step through the engine ----
def _oracle_cfg(aggregation="trn-m"):
    c = CFG
    kw = dict(num_class=c["C"], num_segments=c["T"], feature_dim=c["D"], fc_dim=c["fc"], dropout_i=0.0, dropout_v=0.0)
    if aggregation == "avgpool":      # TemPooling, source only (the engine's default flags for avgpool: none)
        kw.update(frame_aggregation="avgpool", place_adv=("N", "N", "N"), add_loss_DA="none", use_attn="none")
    return orc.Config(**kw)


def _engine_against_torch_adam_and_oracle(eng, n_steps, cfg, beta, gamma, what):
    n = eng.plan.live_floats
    p0 = eng.P[:n].detach().cpu().clone()
    # the oracle's trajectory: its own gradients at its own parameters, clip_grad_norm_ + torch.optim.Adam applied to them
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    o_params = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in eng.param_views().items()}
    o_opt = torch.optim.Adam([o_params[k] for k in eng.live_names()], LR, weight_decay=eng.weight_decay)
    grads, losses = [], []
    for i in range(n_steps):
        xs, xt, ys = _batch(eng, seed=100 + i)
        eng.train_step(beta, gamma, LR)
        loss = eng.losses()["loss"]
        grads.append(eng.G[:n].detach().cpu().clone())      # the update does not touch the gradients (the clip coefficient is applied in flight)
        res = orc.train_step(orc.TrainState(params={k: v.detach() for k, v in o_params.items()}), xs, xt, ys, beta, gamma, cfg,
                             weight_decay=eng.weight_decay, clip=None)
        for k in eng.live_names():
            o_params[k].grad = res["grads"][k].clone()
        torch.nn.utils.clip_grad_norm_([o_params[k] for k in eng.live_names()], float(eng.clip))
        o_opt.step()
        losses.append((loss, float(res["loss"])))
    _assert_within_torch_fp32_error(eng, p0, grads, [LR] * n_steps, float(eng.clip), what)
    for i, (ours, oracle) in enumerate(losses):
        print(f"[adam {what}] step {i}: loss {ours:.6f}, oracle {oracle:.6f}")
        assert abs(ours - oracle) <= tol.TRAIN_EARLY_REL_F32 * abs(oracle), (what, i, losses)
    assert n_steps == 1 or losses[-1][0] != losses[0][0]


def test_five_steps_match_torch_adam_on_the_engines_gradients_and_the_oracles_losses():
    eng = _engine()
    assert eng.fused
    _engine_against_torch_adam_and_oracle(eng, 5, _oracle_cfg(), BETA, GAMMA, "fused trn-m")


@pytest.mark.parametrize("family", ["unfused", "avgpool"])
def test_other_launch_families_run_the_adam_update(family):
    eng = _engine(fused=False) if family == "unfused" else _engine(aggregation="avgpool")
    assert eng.fused == (family == "avgpool")
    beta, gamma = (BETA, GAMMA) if family == "unfused" else ([0.0, 0.0, 0.0], 0.0)
    _engine_against_torch_adam_and_oracle(eng, 1, _oracle_cfg("trn-m" if family == "unfused" else "avgpool"), beta, gamma, family)
    assert eng.adam_step_count == 1 and float(eng.V.max()) > 0


# ---- 6. refusals on the device ----
def test_sgd_only_schedules_are_refused_by_name():
    from ta3n_amd.two_stream import TwoStreamEngine
    eng = _engine()
    _batch(eng)
    with pytest.raises(NotImplementedError, match="Adam.*capture"):
        eng.capture()
    with pytest.raises(NotImplementedError, match="Adam.*fused_update"):
        eng.train_steps([(BETA, GAMMA, LR)] * 2, fused_update=True)
    with pytest.raises(NotImplementedError, match="Adam.*TA3N_SIDE_UPDATE"):
        eng.time_update_launches()
    assert eng.adam_step_count == 0 and not bool(eng.M.any())
    c = CFG
    two = TwoStreamEngine(c["Bs"], c["Bt"], c["T"], (256, 256), c["fc"], c["C"], dropout_i=0.0, dropout_v=0.0, optimizer="Adam")
    with pytest.raises(NotImplementedError, match="Adam.*two-stream"):
        two.train_steps([(BETA, GAMMA, LR)] * 2)
    sgd = _engine(optimizer="SGD")
    assert sgd.V is None
    with pytest.raises(Exception, match="SGD"):
        sgd.adam_views()
