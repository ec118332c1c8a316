"""The kind-specialised backward GEMM kernels request a tile's residual (EPI_ADD), mask (EPI_MASK) and fan-out masks at the head of the K loop
and consume them from registers in the store loop (ta3n_gemm_kernel.h: EPI_EARLY).  Fused train steps through TrainEngine at the smallest
shapes that reach every path of that request (tests/epilogue_operand_cases.py: the table, shared with tests/test_epilogue_operands_cpu.py,
and what each case must land on - asserted from the plan before anything runs), dropout 0.5 / 0.5 throughout:

 (1) EXACT: every twin case with the kind-specialised kernels (early requests) against the same case on the general kernels (requests inside
     the store loop; TA3N_KIND_KERNELS=0, read once per process: two child processes, as tests/test_gpu_kind_kernels.py does at the headline) -
     parameters, gradients, momentum and the whole workspace (losses, every activation and gradient region, their bf16 twins: with twins the
     masked and the fan-out tiles store gZ1 / gZ as twins only) after two steps, byte for byte.  The loads only move, so any difference - a mask dropped or misread at nrem 1 - 3, at m_valid < 32 or on
     the scalar path - is an error, whatever the size of the tensor it lands in.
 (2) against the float64 / mask-synchronised oracle on the kernels' own dropout masks (the recipe and helpers of
     tests/test_gpu_dropout_parity.py) with the bounds of ta3n_amd/tolerances.py - nothing new: fp32 (general kernels), bf16 twins against the
     bf16-operand oracle, f32x3 on pair twins, and use_bn AdaBN, whose launches use add / aux differently.

Chained, split-K and fused-update tiles exist in the experiments build only and keep the old sequence by construction (EPI_EARLY is false
there): nothing here needs that build."""
import os
import subprocess
import sys

import pytest
import torch

import epilogue_operand_cases as eoc
from dropout_masks import BETA, GAMMA, LR, batch, dropout_masks, rel_l2, summary
from oracle import ta3n_oracle as orc
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, dropout_seeds
from ta3n_amd.synthetic import synth_state
from test_gpu_dropout_parity import ADABN_SMALL, _engine_masks, _grad_parity, _oracle

pytestmark = pytest.mark.gpu

P_I = P_V = 0.5

# ---- (1) early requests against requests inside the store loop, byte for byte ----
CHILD = r"""
import hashlib, sys, torch
sys.path.insert(0, "tests")
import epilogue_operand_cases as eoc
from dropout_masks import BETA, GAMMA, LR, batch
from ta3n_amd.engine import TrainEngine
from ta3n_amd.synthetic import synth_state
for case in eoc.TWIN_CASES:
    sh = eoc.SHAPES[eoc.CASES[case][0]]
    eng = TrainEngine(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], dropout_i=0.5, dropout_v=0.5, clip=20.0, **eoc.engine_kw(case))
    assert eng.fused
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=11, scale="trained"))
    for step in range(2):
        xs, xt, ys = batch(sh, 21, step, sh["Bs"], sh["Bt"])
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step(BETA, GAMMA, LR, seed=step)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (eng.P, eng.G, eng.M, eng.ws):      # the WHOLE workspace (zero-filled at construction): fp32 regions and their bf16 twins alike
        h.update(t.cpu().numpy().tobytes())
    nz = float((eng.G[:eng.plan.live_floats] != 0).float().mean())
    print("HASH", case, h.hexdigest(), float(eng.region("losses")[0]), nz)
"""


def test_early_requests_are_bit_identical_to_requests_in_the_store_loop():
    for case in eoc.TWIN_CASES:      # the default process runs what this is about
        eoc.assert_lands_on_early_kernels(case, eoc.early_request_launches(eoc.make_plan(case)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=dict(os.environ, TA3N_KIND_KERNELS=flag), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        out[flag] = {l.split()[1]: l.split()[2:] for l in r.stdout.splitlines() if l.startswith("HASH")}
    assert set(out["0"]) == set(out["1"]) == set(eoc.TWIN_CASES)
    for case in eoc.TWIN_CASES:
        digest, loss, nonzero = out["1"][case]
        assert float(loss) == float(loss) and float(loss) > 0 and float(nonzero) > 0.05, (case, loss, nonzero)      # a finite loss, gradients that are there
        assert out["0"][case][0] == digest, case
    assert len({v[0] for v in out["1"].values()}) == len(eoc.TWIN_CASES)      # (the cases are different computations)


# ---- (2) against the oracle ----
def _cfg(shape, arithmetic="fp32", **kw):
    return orc.Config(num_class=shape["C"], num_segments=shape["T"], feature_dim=shape["D"], fc_dim=shape["F"], dropout_i=P_I, dropout_v=P_V,
                      **({} if arithmetic == "fp32" else dict(arithmetic="bf16", bf16_twins=True)), **kw)


def _cfg_kw(case):
    return dict(use_bn="AdaBN") if eoc.CASES[case][3] else {}


def _step(case):
    """One fused train step of a case; returns (engine, shape, state before the step, batch, host masks, engine ReLU patterns, activations)."""
    shape = eoc.SHAPES[eoc.CASES[case][0]]
    Bs, Bt, T, D, Fc, Cn = (shape[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=P_I, dropout_v=P_V, clip=20.0, **eoc.engine_kw(case))
    assert eng.fused
    early = eoc.early_request_launches(eng.plan)
    if case in eoc.TWIN_CASES:
        eoc.assert_lands_on_early_kernels(case, early)
    else:
        assert early == []      # fp32 MFMA: general kernels
    eng.load_state(synth_state(orc.param_shapes(_cfg(shape, **_cfg_kw(case))), seed=11, scale="trained"))
    xs, xt, ys = batch(shape, 21, 0, Bs, Bt)
    state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
    state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(BETA, GAMMA, LR, seed=0)
    torch.cuda.synchronize()
    mk = dropout_masks(*dropout_seeds(0, 0), P_I, P_V, Bs, Bt, T, eng.F, 256)
    masks, act = _engine_masks(eng, False)
    return eng, shape, state, (xs, xt, ys), mk, masks, act


@pytest.mark.parametrize("case", [c for c in eoc.CASES if c not in eoc.TWIN_CASES])
def test_fp32_against_the_float64_oracle(case, capsys):
    """tests/test_gpu_dropout_parity.py (b): hidden activations, loss and every gradient tensor against the float64 oracle on the host's
    dropout masks and the engine's ReLU patterns, F32_MASKED_GRAD_REL_L2 per tensor and F32_MASKED_GRAD_REL_L2_MEDIAN in the median (AdaBN:
    the two tensors that file names are held to 1e-5 of the largest gradient norm)."""
    eng, shape, state, (xs, xt, ys), mk, masks, act = _step(case)
    res = _oracle(_cfg(shape, **_cfg_kw(case)), state, xs, xt, ys, GAMMA, shape["Bs"], shape["Bt"], mk, masks)
    for d, dom in enumerate(("src", "tgt")):
        for k, a in act[d].items():
            want = res[dom]["hidden"][k].detach()
            err = (a.double() - want).abs().max().item()
            assert err <= 2e-4 * max(1.0, want.abs().max().item()), (case, dom, k, err)
    loss = eng.losses()["loss"]
    assert abs(loss - res["loss"].item()) <= 2e-4 * max(1.0, abs(res["loss"].item())), (case, loss, res["loss"].item())
    lines = []
    _grad_parity(eng, res, f"epilogue operands {case}", lines, ADABN_SMALL if eoc.CASES[case][3] else ())
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("case", [c for c in eoc.TWIN_CASES if eoc.CASES[c][1] == "bf16"])
def test_bf16_twins_against_the_bf16_operand_oracle(case, capsys):
    """Gradients and logits against the oracle's bf16-operand mode on the SAME masks, held to the BF16_REF_* bounds the way
    tests/test_gpu_dropout_parity.py::test_bf16_twins_carry_the_dropped_zeros applies them (per tensor from 4096 elements on, the median over
    all; the small tensors behind the masked tiles are held exactly by the byte comparison above)."""
    eng, shape, state, (xs, xt, ys), mk, masks, _ = _step(case)
    kw = _cfg_kw(case)
    res16 = _oracle(_cfg(shape, "bf16", **kw), state, xs, xt, ys, GAMMA, shape["Bs"], shape["Bt"], mk, masks, dtype=torch.float32)
    res32 = _oracle(_cfg(shape, **kw), state, xs, xt, ys, GAMMA, shape["Bs"], shape["Bt"], mk, masks, dtype=torch.float32)
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res16["grads"]}
    assert all(torch.isfinite(v).all() for v in got.values())
    per, contract = rel_l2(got, res16["grads"]), rel_l2(res16["grads"], res32["grads"])
    med, worst, line = summary(per, f"epilogue operands {case} vs the bf16-operand oracle")
    with capsys.disabled():
        print("\n" + line)
    for k, v in per.items():
        if res16["grads"][k].numel() >= 4096:
            bound = min(tol.BF16_REF_GRAD_REL_L2, tol.BF16_REF_GRAD_CONTRACT_FACTOR * contract[k] + tol.BF16_REF_GRAD_FLOOR)
            assert v <= bound, (case, k, v, bound)
    assert med <= tol.BF16_REF_GRAD_REL_L2_MEDIAN, (case, med)
    o = eng.outputs()
    for key, pick in (("out", lambda r: r["out"]), ("pred_rel", lambda r: r["pred_domain"][0]), ("pred_vid", lambda r: r["pred_domain"][1]),
                      ("pred_frm", lambda r: r["pred_domain"][2])):
        want = torch.cat((pick(res16["src"]), pick(res16["tgt"])), 0).detach()
        err = (o[key].cpu().reshape(want.shape) - want).abs().max().item()
        assert err <= tol.BF16_REF_LOGIT_REL_RMS * want.pow(2).mean().sqrt().item() + 1e-7, (case, key, err)


def test_pair_twins_against_the_float64_oracle(capsys):
    """f32x3 on pair twins (hi + lo planes), headline tile list, ragged shape: fp32-grade, so the float64 comparison of the fp32 cases with
    the split arithmetic's own bounds F32X3_GRAD_REL_L2 (every tensor) / F32X3_GRAD_REL_L2_MEDIAN."""
    eng, shape, state, (xs, xt, ys), mk, masks, _ = _step("ragged_f32x3p")
    res = _oracle(_cfg(shape), state, xs, xt, ys, GAMMA, shape["Bs"], shape["Bt"], mk, masks)
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res["grads"]}
    med, worst, line = summary(rel_l2(got, res["grads"]), "epilogue operands ragged_f32x3p vs float64")
    with capsys.disabled():
        print("\n" + line)
    assert worst <= tol.F32X3_GRAD_REL_L2 and med <= tol.F32X3_GRAD_REL_L2_MEDIAN, (worst, med)
