"""The GEMM tiles' descriptor in lanes (ta3n_gemm_kernel.h: TASK_LANES): the kind-specialised kernels fetch their Task with one vector load -
lane i holds dword i - and the first 20 dwords of Hyper with a second one, and take every field by a lane select at its use, in the front,
between Segs and in the epilogue.  Fused train steps through TrainEngine at
the smallest shapes that put every such field to use (tests/task_front_cases.py: the table, shared with tests/test_task_front_cpu.py, which
asserts from the plans that the table contains what it claims), dropout 0.5 / 0.5 throughout:

 EXACT: every case on the kind-specialised kernels against the same case on the general kernels, which read the descriptor field by field
 from memory as before (TA3N_KIND_KERNELS=0, read once per process: two child processes, as tests/test_gpu_seg_boundary.py does) -
 parameters, gradients, momentum and the whole workspace after two steps, byte for byte.  The arithmetic does not change - the same DMAs,
 MFMAs and epilogue operations in the same order - so any difference (a field taken from the wrong lane, a scalar of the wrong step, a
 bias of the wrong column group) is an error, whatever the size of the tensor it lands in.

 No oracle test is added here.  The two cases that are new in the table are --add_fc 2 plans, and the oracle has no stacked shared layers
 (tests/test_gpu_dropout_parity.py::test_add_fc_2_layers_draw_the_offset_streams holds that option against the float64 interpreter of its
 plan); a tile whose row panel Seg.pad[0] cuts exists in no plan (tests/test_task_front_cpu.py).  The cases taken over from
 tests/epilogue_operand_cases.py and tests/seg_boundary_cases.py are held against the oracle by the GPU tests of those tables, which run
 the same kernels."""
import os
import subprocess
import sys

import pytest

import task_front_cases as tfc

pytestmark = pytest.mark.gpu

CHILD = r"""
import hashlib, sys, torch
sys.path.insert(0, "tests")
import task_front_cases as tfc
from dropout_masks import BETA, GAMMA, LR, batch
from ta3n_amd.engine import TrainEngine
from ta3n_amd.synthetic import synth_state
for case in tfc.CASES:
    sh = tfc.SHAPES[tfc.CASES[case][0]]
    eng = TrainEngine(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], dropout_i=0.5, dropout_v=0.5, clip=20.0, **tfc.engine_kw(case))
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


def test_kind_kernels_are_bit_identical_to_the_general_kernels():
    for case in tfc.CASES:      # the default process runs what this is about: kind kernels, but for the launches the table names
        launches = tfc.kind_launch_tasks(tfc.make_plan(case))
        general = {(ph.wm, ph.wn, ph.wk, ph.bf16) for ph, kernel, _ in launches if kernel is None}
        assert general == tfc.GENERAL_KERNEL_LAUNCHES.get(case, set()) and sum(k is not None for _, k, _ in launches) >= 2, (case, general)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=dict(os.environ, TA3N_KIND_KERNELS=flag), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        out[flag] = {l.split()[1]: l.split()[2:] for l in r.stdout.splitlines() if l.startswith("HASH")}
    assert set(out["0"]) == set(out["1"]) == set(tfc.CASES)
    for case in tfc.CASES:
        digest, *losses = out["1"][case]
        assert len(losses) == 2 and all(float(l) == float(l) and 0 < float(l) < float("inf") for l in losses), (case, losses)
        assert out["0"][case][0] == digest, case
    assert len({v[0] for v in out["1"].values()}) == len(tfc.CASES)      # (the cases are different computations)
