"""One table of the smallest fused-step shapes that put to use every descriptor field the kind-specialised GEMM kernels take from lanes
(ta3n_gemm_kernel.h: TASK_LANES - the Task is fetched once per tile, lane i of a register holding its dword i, and so are the first 20
dwords of Hyper), shared by tests/test_task_front_cpu.py (the plans contain what the table claims: no GPU) and tests/test_gpu_task_front.py
(the kernels).  The twin cases of tests/epilogue_operand_cases.py and the cases of tests/seg_boundary_cases.py are taken over as they are:
between them bias, residual, ReLU / dropout mask, three fan-outs, twin-only stores, EPI_ROWSUM_A, EPI_SUMSQ slots, the EPI_COLSUM and
EPI_SUMROWS8 side jobs, padding tasks, tiles of one Seg and of many, ragged D 40 / D 36, F 42, T 3, AdaBN and pair twins.  New here:

  ragged_addfc2_bf16   --add_fc 2 at the `ragged` shape, every launch on the 32x64 tile with three stages (tile_config 3124; a plan of
                       stacked layers takes no per-launch tile list): the second shared layer's forward launch lands on the forward
                       kind kernel, and its tiles are the only ones whose Task.pad2 - the dropout stream offset - is not zero
  odd_addfc2_bf16      --add_fc 2 at the `odd` shape (tile_config 2124).  F 42 rounds fp32 operands in registers, and the library holds
                       no forward kind kernel of that mode: the forward launches, the one that reads pad2 among them, run the general
                       kernels at every tile this plan can be given (the known exception, as `odd` is in tests/seg_boundary_cases.py);
                       the four backward launches land on the mode-1 kind kernel with its 4-byte path

No plan builder sets Seg.pad[0] (readable A rows beyond the task's m_valid: the block of ones of the bias-gradient column sums, which the
row sums of EPI_ROWSUM_A replaced), so no fused step has a row panel cut by it - tests/test_task_front_cpu.py asserts that over the
table; the row panels these cases cut are cut by m_valid (`tails`: 140 and 700 rows in panels of 32)."""
import epilogue_operand_cases as eoc
import seg_boundary_cases as sbc
from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS

# case -> (shape, TrainEngine keywords beside the shape and the dropout rates)
NEW_CASES = {
    "ragged_addfc2_bf16": ("ragged", dict(bf16=True, bf16_store=True, add_fc=2, tile_config=3124)),
    "odd_addfc2_bf16": ("odd", dict(bf16=True, bf16_store=True, add_fc=2, tile_config=2124)),
}
SHAPES = dict(eoc.SHAPES, **sbc.SHAPES)
assert all(eoc.SHAPES[s] == sbc.SHAPES[s] for s in set(eoc.SHAPES) & set(sbc.SHAPES))
assert all(eoc.engine_kw(c) == sbc.engine_kw(c) and eoc.CASES[c][0] == sbc.CASES[c][0] for c in set(eoc.TWIN_CASES) & set(sbc.CASES))
CASES = {}
for _c in eoc.TWIN_CASES:
    CASES[_c] = (eoc.CASES[_c][0], eoc.engine_kw(_c))
for _c in sbc.CASES:
    CASES.setdefault(_c, (sbc.CASES[_c][0], sbc.engine_kw(_c)))
CASES.update(NEW_CASES)

# cases with a launch that no kind kernel takes, and the (wm, wn, wk, Phase.bf16) of those launches
GENERAL_KERNEL_LAUNCHES = {
    "odd_bf16": {(1, 2, 4, 3)},              # forward launches that round fp32 operands in registers on three stages
    "odd_addfc2_bf16": {(1, 2, 4, 2), (1, 2, 4, 18)},      # ... on two stages (tile 2124), and the TRN launch on twins of two stages
    "ragged_D36_bf16": {(1, 2, 4, 3), (2, 2, 2, 2)},      # D 36: the shared FC rounds in registers, the gradient-at-F1 launch leaves the twins
    "ragged_addfc2_bf16": {(1, 2, 4, 3), (1, 2, 4, 19)},   # backward launches on three stages: the backward kind kernels have two
}


def engine_kw(case):
    return dict(CASES[case][1])


def make_plan(case):
    """The plan TrainEngine builds for the case."""
    if case in eoc.CASES:
        return eoc.make_plan(case)
    if case in sbc.CASES:
        return sbc.make_plan(case)
    shape, kw = CASES[case]
    sh = SHAPES[shape]
    return _lib.Plan(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], ALL_FLAGS | _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE,
                     tile_config=kw["tile_config"], shared_fc_layers=kw["add_fc"])


def kind_launch_tasks(plan):
    """[(phase, kernel or None, [every task of the launch: tiles, side jobs and padding tasks])] of the fused step's GEMM launches."""
    _, tasks, _, _, _, _ = sbc.plan_arrays(plan)
    return [(ph, kernel, [tasks[i] for i in range(ph.task_begin, ph.task_begin + ph.task_count)]) for ph, kernel, _ in sbc.gemm_launches(plan)]
