"""Inputs and CPU references of the SGD update tests (test_gpu_sgd_update.py, test_sgd_shards_cpu.py); importable without a GPU.

The update under test is clip_grad_norm_ + torch.optim.SGD(nesterov=True, weight_decay) on the flat live prefix (reference main.py:83,
578-583), one element:   d = coef g + wd p;   m = mu m + d;   d += mu m;   p -= lr d.

`python tests/sgd_update_cases.py` prints the CPU-side ratios from which the bound K of the general-arithmetic test was chosen
(profiles/sgd_update_floors.txt)."""
import numpy as np
import torch

SHAPES = {      # Bs, Bt, T, D, fc_dim, C
    "small": (12, 8, 5, 512, 128, 12),       # the small shape of test_gpu_adam.py
    "odd": (3, 2, 4, 100, 36, 7),            # test_gpu_bf16.py: parameter sizes that are no multiples of 8 - padding floats inside the prefix
    "headline": (128, 74, 5, 2048, 512, 12),
}
MU, WD = 0.9, 1e-4                            # the general case (main.py's defaults)
GENERAL_STEPS = 10


def real_mask(plan):
    """True at the floats of the live prefix that belong to a parameter (the rest is alignment padding)."""
    mask = torch.zeros(plan.live_floats, dtype=torch.bool)
    for _, off, shape, live in plan.params:
        if live:
            mask[off:off + int(np.prod(shape))] = True
    return mask


def n_first(plan):
    """Floats of the shared frame FC at the head of the prefix: region A of the sharded update, the first range of the deferred one."""
    return next(off for name, off, _, _ in plan.params if not name.startswith("fc_feature_shared_source"))


def cpu_sgd(p0, m0, grads, lrs, mu, wd, clip, dtype):
    """clip_grad_norm_ + torch.optim.SGD(nesterov=True) over the flat prefix in `dtype`, the momentum buffer pre-seeded with m0:
    (P, M, [total norms])."""
    p = torch.nn.Parameter(p0.detach().cpu().to(dtype).clone())
    opt = torch.optim.SGD([p], lrs[0], momentum=mu, weight_decay=wd, nesterov=True)
    opt.state[p]["momentum_buffer"] = m0.detach().cpu().to(dtype).clone()
    norms = []
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.detach().cpu().to(dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], clip if clip > 0 else float("inf"))))
        opt.step()
    return p.detach(), opt.state[p]["momentum_buffer"], norms


def cpu_sgd_fma(p0, m0, grads, lrs, mu, wd, clip):
    """The same recurrence a second legitimate way in fp32: every a b + c formed in float64 and rounded to fp32 once (a fused multiply-add),
    the norm taken in float64 and rounded once.  Used only to measure how far two correct fp32 evaluations lie apart (the bound K)."""
    f32 = lambda t: t.to(torch.float32).to(torch.float64)      # noqa: E731 - one rounding to fp32, kept in a float64 container
    s32 = lambda x: float(np.float32(x))                       # noqa: E731
    p, m = f32(p0.detach().cpu()), f32(m0.detach().cpu())
    mu_, wd_ = s32(mu), s32(wd)
    for g, lr in zip(grads, lrs):
        g = f32(g.detach().cpu())
        coef = 1.0
        if clip > 0:
            total = s32(float(g.norm()))
            coef = min(s32(s32(clip) / s32(total + s32(1e-6))), 1.0)
        gs = f32(g * coef)
        d = f32(wd_ * p + gs)
        m = f32(mu_ * m + d)
        d = f32(mu_ * m + d)
        p = f32(-s32(lr) * d + p)
    return p.to(torch.float32), m.to(torch.float32)


def exact_case(n, mask, seed):
    """Inputs on which three updates are exact in fp32: p0, m0 and three gradients are integers in [-8, 8] (zero on the padding),
    lr = 0.25, mu = 0.5, wd = 0.25, no clipping.  Every intermediate of the recurrence is then a small dyadic rational, so ANY correct fp32
    evaluation - fused multiply-adds or not - gives the float64 values bit for bit; a fourth step would not be exact.
    Returns dict(p0, m0, grads, lr, mu, wd, clip, P=[3 x fp32], M=[3 x fp32]): P[k], M[k] is the state after update k + 1.
    The exactness is asserted here, so a changed recipe fails on the CPU side of the test, not silently."""
    gen = torch.Generator().manual_seed(seed)
    draw = lambda: (torch.randint(-8, 9, (n,), generator=gen).to(torch.float64) * mask)      # noqa: E731
    p0, m0, grads = draw(), draw(), [draw() for _ in range(3)]
    lr, mu, wd = 0.25, 0.5, 0.25
    exact = lambda t: torch.equal(t.to(torch.float32).to(torch.float64), t)      # noqa: E731
    p, m, P, M = p0.clone(), m0.clone(), [], []
    for k, g in enumerate(grads):      # the recurrence itself in float64, every intermediate checked
        d = g + wd * p
        m = mu * m + d
        d2 = d + mu * m
        p = p - lr * d2
        assert exact(d) and exact(m) and exact(d2) and exact(p), f"update {k + 1} of exact_case is not exact in fp32"
        assert float(p.abs().max()) < 16.0
        P.append(p.to(torch.float32)); M.append(m.to(torch.float32))
        for dtype in (torch.float64, torch.float32):      # and torch's own SGD walks the same values in both precisions
            tp, tm, _ = cpu_sgd(p0, m0, grads[:k + 1], [lr] * (k + 1), mu, wd, 0.0, dtype)
            assert torch.equal(tp.to(torch.float64), p) and torch.equal(tm.to(torch.float64), m), (k, dtype)
    f = lambda t: t.to(torch.float32)      # noqa: E731
    return dict(p0=f(p0), m0=f(m0), grads=[f(g) for g in grads], lr=lr, mu=mu, wd=wd, clip=0.0, P=P, M=M)


def general_case(p0, mask, clipped, seed=11):
    """The inputs of the general-arithmetic test: 10 updates, gradients randn x logspace(-9, 0) (permuted; every 7th zero at step 3), a
    non-zero momentum buffer, a learning rate that changes every step, clip = half the first gradient's norm when `clipped`."""
    n = mask.numel()
    gen = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-9, 0, n)[torch.randperm(n, generator=gen)]
    grads = []
    for k in range(GENERAL_STEPS):
        g = torch.randn(n, generator=gen) * scale * mask
        if k == 3:
            g[::7] = 0.0
        grads.append(g)
    m0 = torch.randn(n, generator=gen) * scale[torch.randperm(n, generator=gen)] * mask
    lrs = [1e-3 * (1.0 - 0.07 * k) for k in range(GENERAL_STEPS)]
    clip = 0.5 * float(grads[0].double().norm()) if clipped else 0.0
    return dict(p0=p0.detach().cpu().float().clone(), m0=m0, grads=grads, lrs=lrs, mu=MU, wd=WD, clip=clip)


def general_references(case):
    """((P, M, norms) of torch in fp32, the same in float64) for a general_case."""
    args = (case["p0"], case["m0"], case["grads"], case["lrs"], case["mu"], case["wd"], case["clip"])
    return cpu_sgd(*args, torch.float32), cpu_sgd(*args, torch.float64)


def flat_state(plan, seed=3):
    """The flat parameter prefix an engine holds after load_state(synth_state(..., seed)), built on the CPU."""
    from ta3n_amd.synthetic import synth_state
    state = synth_state({n: s for n, _, s, _ in plan.params}, seed=seed)
    flat = torch.zeros(plan.param_floats)
    for name, off, shape, _ in plan.params:
        flat[off:off + int(np.prod(shape))] = state[name].reshape(-1).float()
    return flat[:plan.live_floats].clone()


def shard_layout(live, first, world):
    """(a_chunk, a_end, b_chunk, b_end) of include/ta3n_hip.h's sharded update, restated: region A = [0, a_end) with a_end the first multiple
    of 4 world at or past `first`, region B = the rest of the live prefix in `world` equal 4-aligned chunks."""
    q = 4 * world
    a_end = -(-first // q) * q
    rest = max(live - a_end, 0)
    b_chunk = -(-rest // q) * 4
    return a_end // world, a_end, b_chunk, a_end + b_chunk * world


def shard_own(live, first, world, rank):
    a_chunk, a_end, b_chunk, _ = shard_layout(live, first, world)
    return [min(a_chunk * rank, live), min(a_chunk * (rank + 1), live), min(a_end + b_chunk * rank, live), min(a_end + b_chunk * (rank + 1), live)]


def _measure():
    from ta3n_amd import _lib
    from ta3n_amd.engine import ALL_FLAGS
    worst = 0.0
    for shape in ("small", "odd"):
        plan = _lib.Plan(*SHAPES[shape], ALL_FLAGS)
        mask, p0 = real_mask(plan), flat_state(plan)
        for clipped in (False, True):
            case = general_case(p0, mask, clipped)
            r32, r64 = general_references(case)
            fp, fm = cpu_sgd_fma(case["p0"], case["m0"], case["grads"], case["lrs"], case["mu"], case["wd"], case["clip"])
            for name, ours, a32, a64 in (("P", fp, r32[0], r64[0]), ("M", fm, r32[1], r64[1])):
                mine = (ours.double() - a64).abs().max().item()
                torchs = (a32.double() - a64).abs().max().item()
                worst = max(worst, mine / torchs)
                print(f"{shape} clipped={clipped} {name}: max|fma fp32 - f64| = {mine:.3e}, max|torch fp32 - f64| = {torchs:.3e}, ratio {mine / torchs:.3f}")
            print(f"{shape} clipped={clipped} norm: max rel |torch fp32 - f64| = {max(abs(a - b) / b for a, b in zip(r32[2], r64[2])):.3e}")
    k = 1.0
    while k < 2.0 * worst:
        k *= 2.0
    print(f"worst ratio {worst:.3f} -> K = {k:g} (the next power of two at or above twice the worst ratio)")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _measure()
