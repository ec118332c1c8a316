"""Seg boundaries of the GEMM tiles' K loops in the kind-specialised twin kernels on two stages (ta3n_gemm_kernel.h: SEG_EARLY): the issue cursor
prepares the next Seg's per-lane stream state one chunk before it is used, and a Seg's full chunks all run the body without skip tests.  Fused train steps through TrainEngine at the smallest
shapes at which that code can go wrong (tests/seg_boundary_cases.py: the table, shared with tests/test_seg_boundary_cpu.py, which asserts
from the plans that the table contains what it claims), dropout 0.5 / 0.5 throughout:

 (1) EXACT: every case on the kind-specialised kernels against the same case on the general kernels, which keep the old sequence
     (TA3N_KIND_KERNELS=0, read once per process: two child processes, as tests/test_gpu_epilogue_operands.py does) - parameters, gradients,
     momentum and the whole workspace after two steps, byte for byte.  The arithmetic does not change - the same MFMAs on the same operands in
     the same order - so any difference (a Seg opened with the wrong length or scale, a stale row limit, a chunk computed from the wrong buffer) is
     an error, whatever the size of the tensor it lands in.
 (2) the `tails` and `T12` cases against the mask-synchronised oracle in its bf16-operand mode, with the bounds of ta3n_amd/tolerances.py as
     tests/test_gpu_dropout_parity.py and tests/test_gpu_epilogue_operands.py apply them - nothing new."""
import os
import subprocess
import sys

import pytest
import torch

import seg_boundary_cases as sbc
from dropout_masks import BETA, GAMMA, LR, batch, dropout_masks, rel_l2, summary
from oracle import ta3n_oracle as orc
from ta3n_amd import tolerances as tol
from ta3n_amd.engine import TrainEngine, dropout_seeds
from ta3n_amd.synthetic import synth_state
from test_gpu_dropout_parity import _engine_masks, _oracle

pytestmark = pytest.mark.gpu

P_I = P_V = 0.5

# ---- (1) kind-specialised kernels against the general kernels (old sequence), byte for byte ----
CHILD = r"""
import hashlib, sys, torch
sys.path.insert(0, "tests")
import seg_boundary_cases as sbc
from dropout_masks import BETA, GAMMA, LR, batch
from ta3n_amd.engine import TrainEngine
from ta3n_amd.synthetic import synth_state
for case in sbc.CASES:
    sh = sbc.SHAPES[sbc.CASES[case][0]]
    eng = TrainEngine(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], dropout_i=0.5, dropout_v=0.5, clip=20.0, **sbc.engine_kw(case))
    assert eng.fused
    eng.load_state(synth_state({n: s for n, _, s, _ in eng.plan.params}, seed=11, scale="trained"))
    losses = []
    for step in range(2):
        xs, xt, ys = batch(sh, 21, step, sh["Bs"], sh["Bt"])
        eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
        eng.train_step(BETA, GAMMA, LR, seed=step)
        torch.cuda.synchronize()
        losses.append(float(eng.region("losses")[0]))
    h = hashlib.sha256()
    for t in (eng.P, eng.G, eng.M, eng.ws):      # the WHOLE workspace (zero-filled at construction): fp32 regions and their bf16 twins alike
        h.update(t.cpu().numpy().tobytes())
    print("HASH", case, h.hexdigest(), *losses)
"""


def _kernels_of(case):
    return [k for _, k, _ in sbc.gemm_launches(sbc.make_plan(case))]


def test_kind_kernels_are_bit_identical_to_the_general_kernels():
    for case in sbc.CASES:      # the default process runs what this is about
        ks = _kernels_of(case)
        assert all(k is not None for k in ks[2:]) and (sbc.CASES[case][0] == "odd" or None not in ks), (case, ks)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=dict(os.environ, TA3N_KIND_KERNELS=flag), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        out[flag] = {l.split()[1]: l.split()[2:] for l in r.stdout.splitlines() if l.startswith("HASH")}
    assert set(out["0"]) == set(out["1"]) == set(sbc.CASES)
    for case in sbc.CASES:
        digest, *losses = out["1"][case]
        assert len(losses) == 2 and all(float(l) == float(l) and 0 < float(l) < float("inf") for l in losses), (case, losses)
        assert out["0"][case][0] == digest, case
    assert len({v[0] for v in out["1"].values()}) == len(sbc.CASES)      # (the cases are different computations)


# ---- (2) against the oracle ----
def _cfg(shape, arithmetic="fp32"):
    return orc.Config(num_class=shape["C"], num_segments=shape["T"], feature_dim=shape["D"], fc_dim=shape["F"], dropout_i=P_I, dropout_v=P_V,
                      **({} if arithmetic == "fp32" else dict(arithmetic="bf16", bf16_twins=True)))


@pytest.mark.parametrize("case", sbc.ORACLE_CASES)
def test_bf16_twins_against_the_bf16_operand_oracle(case, capsys):
    """Gradients and logits of one fused step against the oracle's bf16-operand mode on the SAME masks, held to the BF16_REF_* bounds the way
    tests/test_gpu_dropout_parity.py::test_bf16_twins_carry_the_dropped_zeros applies them (per tensor from 4096 elements on, the median
    over all)."""
    shape = sbc.SHAPES[sbc.CASES[case][0]]
    Bs, Bt, T, D, Fc, Cn = (shape[k] for k in ("Bs", "Bt", "T", "D", "F", "C"))
    eng = TrainEngine(Bs, Bt, T, D, Fc, Cn, dropout_i=P_I, dropout_v=P_V, clip=20.0, **sbc.engine_kw(case))
    assert eng.fused and None not in [k for _, k, _ in sbc.gemm_launches(eng.plan)]
    eng.load_state(synth_state(orc.param_shapes(_cfg(shape)), seed=11, scale="trained"))
    xs, xt, ys = batch(shape, 21, 0, Bs, Bt)
    state = orc.TrainState(params={k: v.detach().cpu().clone() for k, v in eng.param_views().items()}, lr=LR)
    state.momentum = {k: v.detach().cpu().clone() for k, v in eng.momentum_views().items()}
    eng.set_batch(xs.cuda(), xt.cuda(), ys.cuda())
    eng.train_step(BETA, GAMMA, LR, seed=0)
    torch.cuda.synchronize()
    mk = dropout_masks(*dropout_seeds(0, 0), P_I, P_V, Bs, Bt, T, eng.F, 256)
    masks, _ = _engine_masks(eng, False)
    res16 = _oracle(_cfg(shape, "bf16"), state, xs, xt, ys, GAMMA, Bs, Bt, mk, masks, dtype=torch.float32)
    res32 = _oracle(_cfg(shape), state, xs, xt, ys, GAMMA, Bs, Bt, mk, masks, dtype=torch.float32)
    got = {k: v.detach().cpu() for k, v in eng.param_views(eng.G).items() if k in res16["grads"]}
    assert all(torch.isfinite(v).all() for v in got.values())
    per, contract = rel_l2(got, res16["grads"]), rel_l2(res16["grads"], res32["grads"])
    med, worst, line = summary(per, f"seg boundary {case} vs the bf16-operand oracle")
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
