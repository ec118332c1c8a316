"""gemm_tile requests a tile's residual (EPI_ADD), mask (EPI_MASK) and fan-out masks BEFORE its K loop in the kind-specialised kernels
(ta3n_gemm_kernel.h, EPI_EARLY).  That is only sound if no other task of the same launch writes what such a request reads: here, from
the plan alone, for every un-chained GEMM launch of the benchmarked plans and of every plan tests/test_gpu_epilogue_operands.py runs
(tests/epilogue_operand_cases.py: the one table of both files) - the same element intervals Builder::end_chain lays out for chained
launches.  A task may read what it writes itself only in place (same offset and leading dimension: every thread then reads exactly
the elements it stores later).  The same table's claim about which launches land on an early-request kernel is checked here too."""
import numpy as np
import pytest

import epilogue_operand_cases as eoc
from plan_interp import (BASE_G, BASE_P, BASE_WS, BASE_X, EPI_ADD, EPI_COLSUM, EPI_MASK, EPI_ROWSUM_A, EPI_SGD, PH_GEMM, plan_arrays)
from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS
from ta3n_amd.tuning import tuned_phase_tiles

BF16 = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
PLANS = {
    # the benchmarked plans; name: (Bs, Bt, T, D, F, C, extra flags, phase tiles)
    "headline_bf16": (128, 74, 5, 2048, 512, 12, BF16, eoc.HEADLINE_TILES),
    "headline_f32": (128, 74, 5, 2048, 512, 12, 0, tuned_phase_tiles(202, 5, 2048, 512, False, False)),
    "headline_f32x3p": (128, 74, 5, 2048, 512, 12, _lib.FLAG_F32_SPLIT | _lib.FLAG_BF16_STORE, eoc.HEADLINE_TILES_PAIR),
    "two_stream_bf16": (128, 128, 12, 1024, 512, 12, BF16, None),
}


def _make(name):
    if name in eoc.CASES:
        return eoc.make_plan(name)
    Bs, Bt, T, D, F, C, extra, tiles = PLANS[name]
    return _lib.Plan(Bs, Bt, T, D, F, C, ALL_FLAGS | extra, phase_tiles=tiles)


def _rows(off, ld, r0, nr, c0, nc):
    return [(off + r * ld + c0, off + r * ld + c0 + nc) for r in range(r0, r0 + nr)]


def epilogue_hazards(plan):
    """[(phase, reader task, writer task, what)] over the un-chained GEMM launches of every launch list of the plan."""
    segs, tasks, phases, geom, _, _ = plan_arrays(plan)
    size = {BASE_X: geom.B * geom.T * geom.D, BASE_P: plan.param_floats, BASE_G: plan.param_floats, BASE_WS: plan.ws_floats}
    owner = {b: np.full(n, -1, np.int32) for b, n in size.items()}
    found, n_reads = [], 0
    for pi, ph in enumerate(phases):
        if ph.kind != PH_GEMM or ph.chain_off >= 0:
            continue
        BM, BN = 32 * ph.wm * max(ph.rm, 1), 32 * ph.wn * max(ph.rn, 1)
        writes, reads = [], []
        for ti in range(ph.task_begin, ph.task_begin + ph.task_count):
            t = tasks[ti]
            if t.epi & EPI_SGD:
                writes.append((BASE_P, 4 * t.pad[0], 4 * t.pad[1], ti)); continue
            if t.epi & EPI_COLSUM:
                writes.append((t.c_base, t.c_off + t.n0, t.c_off + t.n_valid, ti)); continue
            if t.seg_count == 0:
                continue
            nr, nc = min(BM, t.m_valid - t.m0), min(BN, t.n_valid - t.n0)
            for lo, hi in _rows(t.c_off, t.c_ld, t.m0, nr, t.n0, nc):
                writes.append((t.c_base, lo, hi, ti))
            if t.epi & EPI_ROWSUM_A:
                writes.append((t.bias_base, t.bias_off + t.m0, t.bias_off + t.m0 + nr, ti))
            for f in range(t.fan_count):
                for lo, hi in _rows(t.fan_out_off[f], t.fan_ld, t.m0, nr, t.n0, nc):
                    writes.append((BASE_WS, lo, hi, ti))
                for lo, hi in _rows(t.fan_mask_off[f], t.fan_ld, t.m0, nr, t.n0, nc):
                    reads.append((BASE_WS, lo, hi, ti, "fan mask", False))
            if t.epi & EPI_MASK:
                in_place = (t.aux_base, t.aux_off, t.aux_ld) == (t.c_base, t.c_off, t.c_ld)
                reads += [(t.aux_base, lo, hi, ti, "aux", in_place) for lo, hi in _rows(t.aux_off, t.aux_ld, t.m0, nr, t.n0, nc)]
            if t.epi & EPI_ADD:
                in_place = (t.add_base, t.add_off, t.add_ld) == (t.c_base, t.c_off, t.c_ld)
                reads += [(t.add_base, lo, hi, ti, "add", in_place) for lo, hi in _rows(t.add_off, t.add_ld, t.m0, nr, t.n0, nc)]
        for b, lo, hi, ti in writes:
            if b in owner:
                owner[b][lo:hi] = ti
        for b, lo, hi, ti, what, in_place in reads:
            n_reads += 1
            w = owner[b][lo:hi]
            bad = w[(w >= 0) & ((w != ti) | (not in_place))]
            if bad.size:
                found.append((pi, ti, int(bad[0]), what))
        for b, lo, hi, ti in writes:
            if b in owner:
                owner[b][lo:hi] = -1
    return found, n_reads


@pytest.mark.parametrize("name", sorted(PLANS) + sorted(eoc.CASES))
def test_no_launch_writes_what_its_tiles_request_early(name):
    found, n_reads = epilogue_hazards(_make(name))
    assert n_reads > 0, "the plan has masked, residual and fan-out tiles"
    assert not found, found[:5]


@pytest.mark.parametrize("name", sorted(eoc.CASES))
def test_cases_land_on_the_kernels_they_are_for(name):
    """The twin cases reach the early-request kernels with the operands the table says (relation-level backward: residual + fan-out masks;
    gradient-at-F1 launch: mask, aligned / unaligned / on the general kernel at D 36); the fp32 cases run general kernels only."""
    early = eoc.early_request_launches(eoc.make_plan(name))
    if name in eoc.TWIN_CASES:
        eoc.assert_lands_on_early_kernels(name, early)
    else:
        assert early == []


def test_headline_backward_launches_request_early():
    early = eoc.early_request_launches(_make("headline_bf16"))
    assert eoc.has(early, (1, 2, 4, 1, 2, 26), add=True, fans={1, 3}) and eoc.has(early, (2, 2, 2, 2, 2, 26), aux=True, unaligned=False), early


def test_the_check_sees_a_hazard():
    """A launch whose tile reads another tile's output as its mask is reported: the relation-level backward's fan-out masks against
    that launch's own fan-out stores, after pointing one task's mask at them."""
    plan = _lib.Plan(3, 2, 5, 36, 40, 5, ALL_FLAGS, phase_tiles=None)
    _, tasks, phases, _, _, _ = plan_arrays(plan)
    fan = [ti for ph in phases if ph.kind == PH_GEMM and ph.group == 4 for ti in range(ph.task_begin, ph.task_begin + ph.task_count)
           if tasks[ti].fan_count > 0]
    assert len(fan) >= 2
    a, b = tasks[fan[0]], tasks[fan[1]]
    keep = a.fan_mask_off[0]
    a.fan_mask_off[0] = b.fan_out_off[0] + (b.m0 - a.m0) * b.fan_ld + (b.n0 - a.n0)      # (the arrays are views of the plan's own)
    try:
        found, _ = epilogue_hazards(plan)
    finally:
        a.fan_mask_off[0] = keep
    assert any(w == "fan mask" and r == fan[0] and wr == fan[1] for _, r, wr, w in found), found[:5]
