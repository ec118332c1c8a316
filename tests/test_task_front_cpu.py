"""The case table of tests/task_front_cases.py contains what it claims (no GPU: the plans are read with plan_interp.plan_arrays).  The
kind-specialised GEMM kernels take every field of their Task from the lanes of one register (ta3n_gemm_kernel.h: TASK_LANES), so a lane
select that is off by one shows only on a tile that USES the field: here, from the plans alone, every field those kernels read is put to
use - holds a value that changes the result - by a task that runs on one of them."""
import ctypes as C

import pytest

import plan_interp
import seg_boundary_cases as sbc
import task_front_cases as tfc
from plan_interp import EPI_ADD, EPI_BIAS, EPI_COLSUM, EPI_DROP_I, EPI_DROP_V, EPI_MASK, EPI_ROWSUM_A, EPI_SGD, EPI_SUMROWS8, EPI_SUMSQ, plan_arrays

BASE_G, BASE_WS = plan_interp.BASE_G, plan_interp.BASE_WS


@pytest.fixture(scope="module")
def plans():
    out = {}
    for case in tfc.CASES:
        plan = tfc.make_plan(case)
        out[case] = (plan_arrays(plan)[0], tfc.kind_launch_tasks(plan), plan)      # (the arrays live in the plan)
    return out


def test_a_task_is_fifty_dwords():
    """One dword per lane of a wave (static_assert in gemm_tile), and the mirror the tests read plans with agrees with the library."""
    assert C.sizeof(plan_interp.Task) == 200 and C.sizeof(plan_interp.Task) // 4 <= 64
    assert plan_interp.struct_sizes_ok()
    # the per-step scalars the tiles use are the first 20 dwords of Hyper, `train` the last of them
    from ta3n_amd import _lib
    assert _lib.Hyper.train.offset == 19 * 4 and _lib.Hyper.beta.offset == 0


def test_the_table_takes_over_both_case_lists():
    assert set(tfc.CASES) == set(tfc.eoc.TWIN_CASES) | set(sbc.CASES) | set(tfc.NEW_CASES) and len(tfc.NEW_CASES) == 2


@pytest.mark.parametrize("case", list(tfc.CASES))
def test_every_gemm_launch_lands_on_a_kind_kernel_or_is_a_known_exception(plans, case):
    _, launches, _ = plans[case]
    assert len(launches) >= 6
    general = {(ph.wm, ph.wn, ph.wk, ph.bf16) for ph, kernel, _ in launches if kernel is None}
    assert general == tfc.GENERAL_KERNEL_LAUNCHES.get(case, set()), (case, general)
    assert all(kernel in sbc.KIND_KERNELS for _, kernel, _ in launches if kernel is not None)
    assert sum(kernel is not None for _, kernel, _ in launches) >= 2, case


def _kind_tasks(plans, cases=None):
    """(case, phase, kernel, task) of every task - tile, side job, padding - that runs on a kind-specialised kernel."""
    for case in (cases or tfc.CASES):
        for ph, kernel, tasks in plans[case][1]:
            if kernel is not None:
                for t in tasks:
                    yield case, ph, kernel, t


def _is_tile(t):
    return t.seg_count > 0 and not (t.epi & (EPI_SGD | EPI_COLSUM))


# field(s) of Task -> "a task that runs on a kind kernel puts them to use" (ph: its launch)
USES = {
    "m0": lambda ph, t: _is_tile(t) and t.m0 > 0,
    "n0": lambda ph, t: _is_tile(t) and t.n0 > 0,
    "m_valid": lambda ph, t: _is_tile(t) and t.m0 + 32 * ph.wm > t.m_valid,                 # cuts the tile's rows
    "n_valid": lambda ph, t: _is_tile(t) and t.n0 + 32 * ph.wn > t.n_valid,                 # ... its columns
    "seg_begin": lambda ph, t: _is_tile(t) and t.seg_count > 1 and t.seg_begin > 0,
    "seg_count == 0": lambda ph, t: t.seg_count == 0 and not (t.epi & (EPI_SGD | EPI_COLSUM)),      # padding task
    "seg_count > 1": lambda ph, t: _is_tile(t) and t.seg_count > 1,
    "epi": lambda ph, t: _is_tile(t) and t.epi != 0,
    "alpha_kind": lambda ph, t: _is_tile(t) and t.alpha_kind != 0,
    "gamma_kind": lambda ph, t: _is_tile(t) and t.gamma_kind != 0,
    "c_base == G": lambda ph, t: _is_tile(t) and t.c_base == BASE_G,
    "c_base == WS": lambda ph, t: _is_tile(t) and t.c_base == BASE_WS,
    "c_off, c_ld": lambda ph, t: _is_tile(t) and t.c_off > 0 and t.c_ld > 0 and t.m0 > 0,
    "bias_base, bias_off (bias)": lambda ph, t: _is_tile(t) and (t.epi & EPI_BIAS) and t.bias_off > 0,
    "bias_base, bias_off (row sums)": lambda ph, t: _is_tile(t) and (t.epi & EPI_ROWSUM_A) and t.bias_off > 0,
    "aux_base, aux_off, aux_ld": lambda ph, t: _is_tile(t) and (t.epi & EPI_MASK) and t.aux_off > 0 and t.m0 > 0,
    "add_base, add_off, add_ld": lambda ph, t: _is_tile(t) and (t.epi & EPI_ADD) and t.add_off > 0 and t.m0 > 0,
    # (dropout_i: no GEMM tile of a fused step draws dropout_v - the heads kernel does; asserted below)
    "drop_ld": lambda ph, t: _is_tile(t) and (t.epi & EPI_DROP_I) and t.drop_ld > 0 and t.m0 > 0,
    "fan_count == 1": lambda ph, t: _is_tile(t) and t.fan_count == 1,
    "fan_count == 3, fan_ld, fan_mask_off[0..2], fan_out_off[0..2]": lambda ph, t: _is_tile(t) and t.fan_count == 3 and t.fan_ld > 0 and
        len(set(t.fan_mask_off)) == 3 and len(set(t.fan_out_off)) == 3,
    "seg0 (K-contiguous x K-contiguous)": lambda ph, t: _is_tile(t) and (t.seg0.a_kmajor, t.seg0.b_kmajor) == (0, 0),
    "seg0 (K-contiguous x k-major)": lambda ph, t: _is_tile(t) and (t.seg0.a_kmajor, t.seg0.b_kmajor) == (0, 1),
    "seg0 (k-major x k-major)": lambda ph, t: _is_tile(t) and (t.seg0.a_kmajor, t.seg0.b_kmajor) == (1, 1),
    "seg0.scale_kind": lambda ph, t: _is_tile(t) and t.seg0.scale_kind != 0,
    "seg0.a_base != seg0.b_base": lambda ph, t: _is_tile(t) and t.seg0.a_base != t.seg0.b_base,
    "seg0.a_ld != seg0.b_ld": lambda ph, t: _is_tile(t) and t.seg0.a_ld != t.seg0.b_ld,
    "pad[0..2] (EPI_SUMROWS8)": lambda ph, t: bool(t.epi & EPI_SUMROWS8) and t.seg_count > 0 and t.pad[2] > 0,
    "pad[0..2] (EPI_COLSUM)": lambda ph, t: bool(t.epi & EPI_COLSUM) and t.pad[1] > 0 and t.pad[2] > 0,
    "pad[3] (EPI_SUMSQ)": lambda ph, t: _is_tile(t) and (t.epi & EPI_SUMSQ) and t.pad[3] > 0,
    "pad[3] (EPI_COLSUM | EPI_SUMSQ)": lambda ph, t: (t.epi & EPI_COLSUM) and (t.epi & EPI_SUMSQ) and t.pad[3] > 0,
    "pad2": lambda ph, t: _is_tile(t) and (t.epi & (EPI_DROP_I | EPI_DROP_V)) and t.pad2 > 0,
}
# the fields of Task that the kind kernels of the default library never read: the chained-launch fields (launch_gemm refuses a chained
# launch on it) and `cost` (the plan builder's own; the stamps build records it)
NOT_READ = {"sig", "wait_begin", "wait_count", "cost"}


def test_the_uses_name_every_field_the_kernels_read():
    named = " ".join(USES)
    for f, _ in plan_interp.Task._fields_:
        assert (f in NOT_READ) != (f in named), f


def test_every_field_is_put_to_use_on_a_kind_kernel(plans):
    found = {u: set() for u in USES}
    for case, ph, kernel, t in _kind_tasks(plans):
        for u, pred in USES.items():
            if pred(ph, t):
                found[u].add((case, kernel))
    assert not [u for u, f in found.items() if not f], [u for u, f in found.items() if not f]
    # both K loops (three stages: forward kernels; two: backward kernels), plain twins and pair twins, see descriptors with Segs, edges and epilogue operands
    for u in ("m0", "n0", "m_valid", "n_valid", "seg_count > 1"):
        assert {k[4] for _, k in found[u]} == {2, 3}, (u, found[u])
        assert {(2, 1, 4, 4, 3, 1), (1, 2, 4, 3, 2, 26), (1, 2, 2, 4, 2, 26)} & {k for _, k in found[u]}, (u, found[u])
    # the dropout stream offset is not zero in one place only: the second shared layer of --add_fc 2, on the forward kind kernel
    assert found["pad2"] == {("ragged_addfc2_bf16", (1, 2, 4, 2, 3, 1))}
    assert not any(t.epi & EPI_DROP_V for _, _, _, t in _kind_tasks(plans))
    # the side jobs ride in launches of kind kernels
    for u in ("pad[0..2] (EPI_SUMROWS8)", "pad[0..2] (EPI_COLSUM)", "seg_count == 0"):
        assert len({c for c, _ in found[u]}) >= 8, (u, found[u])


def test_the_pad2_tile_of_the_odd_shape_runs_a_general_kernel(plans):
    """--add_fc 2 at F 42: the launch whose tiles carry pad2 rounds fp32 operands in registers, and no forward kind kernel of that mode exists."""
    seen = [(kernel, t.pad2) for ph, kernel, tasks in plans["odd_addfc2_bf16"][1] for t in tasks if t.pad2 > 0]
    assert seen and all(kernel is None for kernel, _ in seen)
    sh = tfc.SHAPES["odd"]
    assert {p for _, p in seen} == {(sh["Bs"] + sh["Bt"]) * sh["T"] * sh["F"]}      # (k - 1) B T F, k = 2
    assert sum(kernel == (1, 2, 4, 1, 2, 26) for _, kernel, _ in plans["odd_addfc2_bf16"][1]) == 4


def test_no_plan_sets_the_row_limit_of_a_seg(plans):
    """Seg.pad[0] > 0 would give the A operand more readable rows than the task's m_valid.  Nothing builds such a Seg any more, so the table
    can hold no tile whose row panel it cuts; the kernels keep the test (`sg.pad[0] > 0 ? sg.pad[0] : m_valid`).  A plan builder that sets it
    again makes this fail - and then a case with such a tile belongs into the table."""
    for case in tfc.CASES:
        segs, launches, _ = plans[case]
        assert max(s.pad[0] for s in segs) == 0 and max(s.pad[1] for s in segs) == 0, case
        assert all(t.seg0.pad[0] == 0 for _, _, tasks in launches for t in tasks), case


def test_row_panels_cut_by_m_valid(plans):
    """... the last row panels of `tails` are cut by m_valid: 140 and 700 rows in panels of 32, m_valid inside the fifth and the twenty-second."""
    rows = {(t.m0, t.m_valid) for _, ph, kernel, t in _kind_tasks(plans, ["tails_bf16"]) if kernel == (1, 2, 4, 2, 3, 1) and _is_tile(t)}
    assert {(128, 140), (672, 700)} <= rows, sorted(rows)
