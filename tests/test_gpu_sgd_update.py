"""GPU: the clip + Nesterov SGD update (nesterov_sgd / clip_coef of csrc/ta3n_kernels.h, update_range<SgdRule>) against float64, through
every entry of include/ta3n_hip.h that reaches it directly - ta3n_sgd_step, ta3n_sgd_range, ta3n_sgd_step_next, ta3n_sgd_shard,
ta3n_sgd_step_fused - and the shard split at worlds 2, 3, 5 and 8 with one process playing every rank.  The other schedules (deferred,
pipelined, train_steps, fused update, the multi-process sharded step) are held bit-identical to these by their own tests.

Three yardsticks, none taken from the code under test (inputs and CPU references: sgd_update_cases.py):
  exact    integer inputs with lr = 0.25, mu = 0.5, wd = 0.25: three updates are exact in fp32, so the result must equal the float64
           recurrence bit for bit on every element, whatever the evaluation order or contraction.
  general  max |gpu - f64| <= K x max |torch fp32 - f64| for P and for the momentum buffer, K = 2.  The kernel contracts each line of
           the recurrence into one fma, torch does not; a CPU evaluation with every a b + c rounded once (sgd_update_cases.cpu_sgd_fma)
           sat at 1.000 / 0.655 (P / M, small shape) and 1.000 / 0.743 (odd shape) of torch's distance unclipped and at 0.195 / 0.009 and
           0.681 / 0.022 clipped (torch's fp32 norm is off by 2e-5 relative there); worst ratio 1.000, twice that is 2.  The GPU's own
           ratios are printed (profiles/sgd_update_floors.txt).
  norm     |norm - norm64| <= L 2^-24 norm64 with L the longest chain of fp32 additions one square passes through on its way to the
           total (a sum of non-negative terms through L roundings is off by at most L 2^-24 relative, the root halves that and adds one
           rounding).  The gradient-norm pass: 256 workgroups of 256 threads stride live / 4 float4 - 4 float4 = 16 fused adds per thread
           at the small shape, 2 at the odd one (14 = 56 adds at the headline shape); 6 + 4 in the block sum; 8 in the strided sum of
           the 256 partials; 6 + 4 in the block sum of the update's prologue: L = 44 here (84 at the headline shape).  A rank's shard
           partial (two strided loops, block sum, one more block sum over the 256 workgroups) and the sum over the slots stay below 60.
           The fixed 1e-5 used below is this bound at L = 167.  For the fused step's partials L is counted from the plan's tile lists."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import plan_interp as pi
import sgd_update_cases as sc
from ta3n_amd import _lib
from ta3n_amd.synthetic import synth_batch, synth_state

pytestmark = pytest.mark.gpu

K_BOUND = 2.0
NORM_RTOL = 1e-5
BETA, GAMMA = [0.75, 0.75, 0.5], 0.003
SENTINEL = 3.0        # behind the live prefix: no update may touch it, no norm may read it
WORLDS = [2, 3, 5, 8]

_ENGINES = {}


def _engine(shape, which="a", cache=True, **kw):
    """A TrainEngine of one of sgd_update_cases.SHAPES.  Cached: every test writes P, G, M and its scalars itself."""
    from ta3n_amd.engine import TrainEngine
    key = (shape, which, tuple(sorted(kw.items())))
    if not cache or key not in _ENGINES:
        eng = TrainEngine(*sc.SHAPES[shape], dropout_i=0.0, dropout_v=0.0, **kw)
        if not cache:
            return eng
        _ENGINES[key] = eng
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def _mask(shape):
    return sc.real_mask(_engine(shape).plan)


@functools.lru_cache(maxsize=None)
def _exact(shape):
    m = _mask(shape)
    return sc.exact_case(m.numel(), m, seed=17)


@functools.lru_cache(maxsize=None)
def _general(shape, clipped):
    p0 = sc.flat_state(_engine(shape).plan)
    case = sc.general_case(p0, _mask(shape), clipped)
    return case, sc.general_references(case)


def _fill(eng, p, m, g=None):
    n = eng.plan.live_floats
    eng.P.fill_(SENTINEL); eng.G[n:].fill_(SENTINEL)
    eng.P[:n].copy_(p); eng.M.copy_(m)
    if g is not None:
        eng.G[:n].copy_(g)
    if eng.bf16_store:
        eng.refresh_bf16(params=True)


def _ptrs(eng):
    return (eng.plan.handle, eng.P.data_ptr(), eng.G.data_ptr(), eng.M.data_ptr(), eng.ws.data_ptr())


def _sgd_range(eng, lo, hi, lr, mu, wd, clip, fused_norm=0):
    _lib.check(eng._L.ta3n_sgd_range(*_ptrs(eng), lo, hi, fused_norm, lr, mu, wd, clip, eng._stream()), "ta3n_sgd_range")


def _update(eng, entry, lr, mu, wd, clip, nxt=None):
    n, first = eng.plan.live_floats, sc.n_first(eng.plan)
    if entry == "step":              # the scalars travel through ws["hyper"]
        eng.momentum, eng.weight_decay, eng.clip = mu, wd, clip
        eng.set_hyper(BETA, GAMMA, lr)
        eng.sgd_step()
    elif entry == "range":
        _sgd_range(eng, 0, n, lr, mu, wd, clip)
    elif entry == "two_ranges":
        _sgd_range(eng, 0, first, lr, mu, wd, clip)
        _sgd_range(eng, first, n, lr, mu, wd, clip)
    elif entry == "step_next":
        _lib.check(eng._L.ta3n_sgd_step_next(*_ptrs(eng), 0, lr, mu, wd, clip, C.byref(nxt), eng._stream()), "ta3n_sgd_step_next")
    else:
        raise AssertionError(entry)


def _hyper_words(eng):
    return eng.region("hyper").view(torch.int32)[: C.sizeof(_lib.Hyper) // 4].cpu().numpy()


def _next_hyper(eng, k):
    """A ta3n_hyper no other call of the test leaves in the workspace."""
    return eng.hyper_for([0.1 + k, 0.2, 0.3], 0.5 + k, 0.125 * (k + 1), step=1000 + k)


def _twin_is_rounded_parameter(eng):
    n = eng.plan.live_floats
    lo, size = eng.plan.region("p16")
    p16 = eng.ws[lo:lo + size].view(torch.bfloat16)[:n]
    return torch.equal(p16.view(torch.int16), eng.P[:n].to(torch.bfloat16).view(torch.int16))


def _within_torch_fp32_error(eng, r32, r64, what):
    n = eng.plan.live_floats
    ratios = {}
    for name, gpu, a32, a64 in (("P", eng.P[:n], r32[0], r64[0]), ("M", eng.M, r32[1], r64[1])):
        ours = (gpu.detach().cpu().double() - a64).abs().max().item()
        torchs = (a32.double() - a64).abs().max().item()
        ratios[name] = ours / torchs
        print(f"[sgd {what}] {name}: max|gpu - f64| = {ours:.3e}, max|torch fp32 - f64| = {torchs:.3e}, ratio {ours / torchs:.3f}")
    for name, r in ratios.items():
        assert r <= K_BOUND, (what, name, ratios)


# ---- (a) exact arithmetic, every element ----
@pytest.mark.parametrize("clip", [0.0, 1e30])      # 1e30: fminf(clip / (norm + 1e-6), 1) must be exactly 1
@pytest.mark.parametrize("entry", ["step", "range", "two_ranges", "step_next"])
@pytest.mark.parametrize("shape,twins", [("small", False), ("odd", False), ("small", True)])
def test_three_exact_updates_equal_the_float64_recurrence_bit_for_bit(shape, twins, entry, clip):
    eng = _engine(shape, bf16=True, bf16_store=True) if twins else _engine(shape)
    case, mask = _exact(shape), _mask(shape)
    n = eng.plan.live_floats
    assert not bool(mask.all())                          # alignment padding inside the prefix
    assert (n // 4) % 256 != 0 and n // 4 > 256          # several workgroups, the last one partly idle
    _fill(eng, case["p0"], case["m0"])
    for k, g in enumerate(case["grads"]):
        eng.G[:n].copy_(g)
        nxt = _next_hyper(eng, k) if entry == "step_next" else None
        _update(eng, entry, case["lr"], case["mu"], case["wd"], clip, nxt)
        torch.cuda.synchronize()
        P, M = eng.P.detach().cpu(), eng.M.detach().cpu()
        assert torch.equal(P[:n], case["P"][k]), (k, int((P[:n] != case["P"][k]).sum()))
        assert torch.equal(M, case["M"][k]), (k, int((M != case["M"][k]).sum()))
        assert not bool(P[:n][~mask].any()) and not bool(M[~mask].any())      # alignment padding stays exactly 0
        assert bool((P[n:] == SENTINEL).all())
        assert float(eng.region("grad_norm")[1]) == 1.0
        if entry == "step_next":
            assert np.array_equal(_hyper_words(eng), np.frombuffer(nxt, dtype=np.int32))
        if twins:
            assert _twin_is_rounded_parameter(eng)


# ---- (b) general arithmetic within torch's own fp32 error ----
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("shape", ["small", "odd"])
def test_ten_updates_match_torch_sgd_within_its_own_fp32_error(shape, clipped):
    eng = _engine(shape)
    case, (r32, r64) = _general(shape, clipped)
    n, mask = eng.plan.live_floats, _mask(shape)
    _fill(eng, case["p0"], case["m0"])
    seen = []
    for k, (g, lr) in enumerate(zip(case["grads"], case["lrs"])):
        eng.G[:n].copy_(g)
        clip = case["clip"] if clipped else (0.0, -1.0)[k % 2]      # clip = 0 and clip < 0 both mean: no clipping
        _sgd_range(eng, 0, n, lr, case["mu"], case["wd"], clip)
        seen.append(eng.region("grad_norm")[:2].tolist())
    torch.cuda.synchronize()
    _within_torch_fp32_error(eng, r32, r64, f"{shape} clipped={clipped}")
    for (gn, coef), norm64 in zip(seen, r64[2]):
        assert abs(gn - norm64) <= NORM_RTOL * norm64, (gn, norm64)
        if clipped:
            assert coef < 1.0 and abs(coef - case["clip"] / (norm64 + 1e-6)) <= 1e-5
        else:
            assert coef == 1.0
    P, M = eng.P.detach().cpu(), eng.M.detach().cpu()
    assert not bool(P[:n][~mask].any()) and not bool(M[~mask].any()) and bool((P[n:] == SENTINEL).all())
    assert bool(torch.isfinite(P).all()) and float(M.abs().max()) > 0


# ---- (c) ranges compose; argument checks ----
def _random_grad(eng, shape, seed):
    n = eng.plan.live_floats
    eng.G[:n].copy_(torch.randn(n, generator=torch.Generator().manual_seed(seed)) * _mask(shape))


@pytest.mark.parametrize("shape", ["small", "odd"])
def test_three_ranges_equal_one_whole_prefix_call(shape):
    whole, split = _engine(shape), _engine(shape, "b")
    n, first = whole.plan.live_floats, sc.n_first(whole.plan)
    edges = {off for _, off, _, _ in whole.plan.params} | {off + int(np.prod(s)) for _, off, s, _ in whole.plan.params}
    cut = first + 4 * ((n - first) // 12)
    while cut in edges:
        cut += 4
    assert 0 < first < cut < n and first % 4 == 0 and cut % 4 == 0
    case, _ = _general(shape, False)
    for eng in (whole, split):
        _fill(eng, case["p0"], case["m0"])
    for step in (1, 2):
        for eng in (whole, split):
            _random_grad(eng, shape, seed=step)
        args = (1e-3 * step, sc.MU, sc.WD, 1.0)      # clip 1.0 is far below the norm of n standard normals
        _sgd_range(whole, 0, n, *args)
        for lo, hi in ((0, first), (first, cut), (cut, n)):
            _sgd_range(split, lo, hi, *args)
    torch.cuda.synchronize()
    assert torch.equal(whole.P, split.P) and torch.equal(whole.M, split.M)
    assert torch.equal(whole.region("grad_norm")[:2], split.region("grad_norm")[:2]) and float(whole.region("grad_norm")[1]) < 1.0
    assert not torch.equal(whole.P[:n].cpu(), case["p0"])


def test_bad_ranges_are_refused_and_change_nothing():
    eng = _engine("small")
    n = eng.plan.live_floats
    case, _ = _general("small", False)
    _fill(eng, case["p0"], case["m0"], case["grads"][0])
    msg = "range must be 4-float aligned and inside the live parameter prefix"
    for lo, hi in ((2, n), (0, n + 4), (8, 4), (0, n - 2), (-4, n)):
        with pytest.raises(ValueError, match=msg):
            _sgd_range(eng, lo, hi, 1e-3, sc.MU, sc.WD, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(eng.P[:n].cpu(), case["p0"]) and torch.equal(eng.M.cpu(), case["m0"])
    from ta3n_amd.engine import TrainEngine
    wide = TrainEngine(2, 2, 3, 2304, 2304, 4, dropout_i=0.0, dropout_v=0.0)      # fc_dim 2304: no fused step, so no norm partials to take
    assert not wide.plan.has_fused_step
    with pytest.raises(ValueError, match="no fused step for this configuration"):
        _sgd_range(wide, 0, wide.plan.live_floats, 1e-3, sc.MU, sc.WD, 0.0, fused_norm=1)
    torch.cuda.synchronize()
    assert not bool(wide.P.any()) and not bool(wide.M.any())


# ---- (d) every rank of a sharded update, played by one process ----
def _own(eng, rank, world):
    own = (C.c_int64 * 4)()
    _lib.check(eng._L.ta3n_shard_ranges(eng.plan.handle, rank, world, own, None), "ta3n_shard_ranges")
    return list(own)


def _shard_slots(eng, world):
    """ta3n_shard_sumsq as every rank in turn: [the value rank r leaves in slot r]; every other slot must be zero."""
    slots = []
    for r in range(world):
        _lib.check(eng._L.ta3n_shard_sumsq(eng.plan.handle, eng.G.data_ptr(), eng.ws.data_ptr(), r, world, eng._stream()), "ta3n_shard_sumsq")
        part = eng.region("norm_part").cpu()
        assert part.numel() == 256
        slots.append(float(part[r]))
        part[r] = 0.0
        assert not bool(part.any()), (r, world)
    return slots


def _sharded_update(eng, world, lr, mu, wd, clip, nxt=None):
    """The update of all `world` ranks on one stream; the host plays the all-gather of one float per rank.  Returns the slots."""
    slots = _shard_slots(eng, world)
    gathered = torch.zeros(256)
    gathered[:world] = torch.tensor(slots)
    eng.region("norm_part").copy_(gathered)
    for r in range(world):
        _lib.check(eng._L.ta3n_sgd_shard(*_ptrs(eng), r, world, lr, mu, wd, clip, C.byref(nxt) if nxt is not None else None, eng._stream()),
                   "ta3n_sgd_shard")
    return slots


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape", ["small", "odd"])
def test_all_ranks_of_an_unclipped_sharded_update_equal_the_whole_prefix_update(shape, world):
    """Every float of the prefix is updated exactly once: bitwise the whole-prefix update, two steps (the second on a momentum buffer the
    first one left).  The second step carries the next step's scalars on every rank."""
    whole, sharded = _engine(shape), _engine(shape, "b")
    n = whole.plan.live_floats
    case, _ = _general(shape, False)
    for eng in (whole, sharded):
        _fill(eng, case["p0"], case["m0"])
    nxt = _next_hyper(sharded, world)
    for k in (0, 1):
        for eng in (whole, sharded):
            eng.G[:n].copy_(case["grads"][k])
        _sgd_range(whole, 0, n, case["lrs"][k], sc.MU, sc.WD, 0.0)
        _sharded_update(sharded, world, case["lrs"][k], sc.MU, sc.WD, 0.0, nxt if k == 1 else None)
    torch.cuda.synchronize()
    assert torch.equal(whole.P, sharded.P) and torch.equal(whole.M, sharded.M)
    assert bool((sharded.P[n:] == SENTINEL).all()) and float(sharded.region("grad_norm")[1]) == 1.0
    assert np.array_equal(_hyper_words(sharded), np.frombuffer(nxt, dtype=np.int32))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape", ["small", "odd"])
def test_all_ranks_of_a_clipped_sharded_update_stay_within_torchs_fp32_error(shape, world):
    """The norm is the sum of the ranks' partials - another summation order than the whole-prefix pass, so not the same bits: both engines
    against float64 under the bound of the general test, the partials and the recorded norm against the float64 norm."""
    whole, sharded = _engine(shape), _engine(shape, "b")
    n = whole.plan.live_floats
    case, _ = _general(shape, True)
    steps = 2
    args = (case["p0"], case["m0"], case["grads"][:steps], case["lrs"][:steps], sc.MU, sc.WD, case["clip"])
    r32, r64 = sc.cpu_sgd(*args, torch.float32), sc.cpu_sgd(*args, torch.float64)
    for eng in (whole, sharded):
        _fill(eng, case["p0"], case["m0"])
    for k in range(steps):
        for eng in (whole, sharded):
            eng.G[:n].copy_(case["grads"][k])
        _sgd_range(whole, 0, n, case["lrs"][k], sc.MU, sc.WD, case["clip"])
        slots = _sharded_update(sharded, world, case["lrs"][k], sc.MU, sc.WD, case["clip"])
        norm64 = r64[2][k]
        gn, coef = sharded.region("grad_norm")[:2].tolist()
        print(f"[sgd shards {shape} world {world}] step {k}: sum of slots {sum(slots):.9e}, norm64^2 {norm64 ** 2:.9e}, norm {gn:.9e} vs {norm64:.9e}")
        assert abs(math.fsum(slots) - norm64 ** 2) <= 2.0 * NORM_RTOL * norm64 ** 2
        assert abs(gn - norm64) <= NORM_RTOL * norm64 and coef < 1.0 and abs(coef - case["clip"] / (norm64 + 1e-6)) <= 1e-5
    torch.cuda.synchronize()
    _within_torch_fp32_error(whole, r32, r64, f"{shape} whole prefix, clipped")
    _within_torch_fp32_error(sharded, r32, r64, f"{shape} world {world}, clipped")
    assert bool((sharded.P[n:] == SENTINEL).all())


def test_sharded_update_keeps_the_parameter_twins_current():
    whole, sharded = _engine("small"), _engine("small", bf16=True, bf16_store=True)
    n = whole.plan.live_floats
    case, _ = _general("small", True)
    for eng in (whole, sharded):
        _fill(eng, case["p0"], case["m0"], case["grads"][0])
    _sgd_range(whole, 0, n, 1e-3, sc.MU, sc.WD, 0.0)
    _sharded_update(sharded, 3, 1e-3, sc.MU, sc.WD, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(whole.P[:n], sharded.P[:n]) and torch.equal(whole.M, sharded.M)
    assert _twin_is_rounded_parameter(sharded)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape", ["small", "odd"])
def test_shard_partials_count_exactly_the_own_floats(shape, world):
    """G = 1 at the first and the last float of each own range of each rank, 0 elsewhere: slot r must be exactly the number of ones inside
    rank r's ranges - a bound off by one float4 changes an integer."""
    eng = _engine(shape)
    n, first = eng.plan.live_floats, sc.n_first(eng.plan)
    g = torch.zeros(n)
    want = []
    for r in range(world):
        own = _own(eng, r, world)
        assert own == sc.shard_own(n, first, world, r)
        count = 0
        for lo, hi in ((own[0], own[1]), (own[2], own[3])):
            if hi > lo:
                g[lo] = 1.0; g[hi - 1] = 1.0
                count += 2
        want.append(float(count))
    eng.G.fill_(SENTINEL)
    eng.G[:n].copy_(g)
    slots = _shard_slots(eng, world)
    assert slots == want and sum(slots) == float(g.sum())


def test_a_rank_without_a_share_only_delivers_the_next_steps_scalars():
    """ta3n_sgd_shard itself accepts any world the flat buffers can hold: at one chunk of 4 floats per rank and more ranks than float4s in the
    prefix, rank 10 owns floats [40, 44) and nothing else, and the ranks past the prefix own nothing: they only leave `next` in ws["hyper"]."""
    eng = _engine("odd")
    n, first = eng.plan.live_floats, sc.n_first(eng.plan)
    world = n // 4 + 1000
    a_chunk, a_end, b_chunk, b_end = sc.shard_layout(n, first, world)
    assert a_chunk == 4 and a_end > n and b_chunk == 0 and b_end <= eng.plan.param_floats
    case = _exact("odd")
    _fill(eng, case["p0"], case["m0"], case["grads"][0])
    eng.region("norm_part").zero_()
    assert _own(eng, 10, world) == [40, 44, n, n] and _own(eng, world - 1, world) == [n, n, n, n]
    nxt = _next_hyper(eng, 7)
    for rank, nx in ((world - 1, nxt), (10, None)):
        _lib.check(eng._L.ta3n_sgd_shard(*_ptrs(eng), rank, world, case["lr"], case["mu"], case["wd"], 0.0,
                                         C.byref(nx) if nx is not None else None, eng._stream()), "ta3n_sgd_shard")
    torch.cuda.synchronize()
    assert np.array_equal(_hyper_words(eng), np.frombuffer(nxt, dtype=np.int32))
    want_p, want_m = case["p0"].clone(), case["m0"].clone()
    want_p[40:44], want_m[40:44] = case["P"][0][40:44], case["M"][0][40:44]
    assert torch.equal(eng.P[:n].cpu(), want_p) and torch.equal(eng.M.cpu(), want_m) and bool((eng.P[n:] == SENTINEL).all())


# ---- (f) the fused step's norm partials ----
def _norm_chain_length(plan, bn_shared):
    """The longest chain of fp32 additions between one squared gradient and the total of ta3n_sgd_step_fused, from the plan's own lists:
      1. in a gradient tile every thread adds the squares of 4 x ITER outputs, ITER = ceil(BM BN / 4 / threads), plus one for a bias
         gradient (EPI_ROWSUM_A); in a column-sum task those of ceil(columns / threads) outputs; in a BatchNorm workgroup 2 per column;
      2. 6 steps of the wave reduction and one addition per wave of the workgroup;
      3. strided_partial_sum over the n_sumsq slots on 256 threads, 8 additions per round;
      4. block_sum of the update's prologue: 6 steps in the wave, 4 waves."""
    _, tasks, phases, geom, _, _ = pi.plan_arrays(plan)
    in_thread = in_block = 0
    for ph in phases:
        if ph.group != 4 or ph.kind != pi.PH_GEMM:
            continue
        waves = ph.wm * ph.wn * ph.wk
        bm, bn = 32 * ph.wm * max(ph.rm, 1), 32 * ph.wn * max(ph.rn, 1)
        for t in tasks[ph.task_begin: ph.task_begin + ph.task_count]:
            if not t.epi & pi.EPI_SUMSQ:
                continue
            if t.epi & pi.EPI_COLSUM:
                mine = -(-(t.n_valid - t.n0) // (64 * waves))
            else:
                mine = 4 * -(-(bm * bn // 4) // (64 * waves)) + (1 if t.epi & pi.EPI_ROWSUM_A else 0)
            in_thread, in_block = max(in_thread, mine), max(in_block, 6 + waves)
    if bn_shared:
        in_thread = max(in_thread, 2 * pi.BN_COLS)
    assert in_thread > 0 and geom.n_sumsq > 0
    return in_thread + in_block + 8 * -(-geom.n_sumsq // (8 * 256)) + (6 + 4)


FUSED_CASES = {
    "fp32": {},
    "bf16_twins": dict(bf16=True, bf16_store=True),
    "f32x3_pair_twins": dict(f32_split=True, bf16_store=True),
    "AdaBN": dict(use_bn="AdaBN"),
    "add_fc_2": dict(add_fc=2),
    "avgpool": dict(aggregation="avgpool"),
    "wgrads_late": dict(wgrads_late=True),
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
@pytest.mark.parametrize("shape", ["small", "odd"])
def test_fused_step_partials_add_up_to_the_norm_of_the_gradients_it_wrote(shape, case):
    """ta3n_sgd_step_fused takes the clip norm from ws["sumsq"], one slot per gradient tile, instead of reading the gradients: after one
    fused step on real data the recorded norm against the float64 norm of G, within the counted summation depth (lr = 0: nothing moves)."""
    kw = FUSED_CASES[case]
    eng = _engine(shape, cache=False, clip=0.0, **kw)
    assert eng.fused and eng.plan.has_fused_step
    Bs, Bt, T, D, _, Cn = sc.SHAPES[shape]
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=3))
    xs, xt, ys, _ = synth_batch(Cn, T, D, Bs, Bt, seed=9)
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    n = eng.plan.live_floats
    beta, gamma = (([0.0, 0.0, 0.0], 0.0) if case == "avgpool" else (BETA, GAMMA))
    eng.set_hyper(beta, gamma, 0.0)
    eng.fused_step()
    torch.cuda.synchronize()
    before = eng.P.clone()
    norm64 = float(eng.G[:n].double().norm())
    eng.sgd_step_fused()
    torch.cuda.synchronize()
    gn, coef = eng.region("grad_norm")[:2].tolist()
    chain = _norm_chain_length(eng.plan, bn_shared="use_bn" in kw)
    bound = chain * 2.0 ** -24
    print(f"[sgd fused norm {shape} {case}] norm {gn:.9e}, float64 {norm64:.9e}, rel {abs(gn - norm64) / norm64:.2e}; chain {chain}, bound {bound:.2e}, "
          f"{eng.plan.region('sumsq')[1]} slots")
    assert bound <= NORM_RTOL
    assert norm64 > 0 and abs(gn - norm64) <= bound * norm64
    assert coef == 1.0 and torch.equal(eng.P, before)
