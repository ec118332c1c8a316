"""The case table of tests/seg_boundary_cases.py contains what it claims (no GPU: the plans are read with plan_interp.plan_arrays): Seg lists
whose consecutive Segs have equal geometry (only the offsets change) and ones whose geometry changes (leading dimension, row limit),
Segs of one chunk, of two full chunks and of a full chunk plus a tail, a scaled Seg in front of further Segs, and launches that
land on the kind-specialised kernels, among them the ones that treat a Seg boundary differently (ta3n_gemm_kernel.h: SEG_EARLY)."""
import pytest

import seg_boundary_cases as sbc
from plan_interp import plan_arrays

SK_ONE = 0


@pytest.fixture(scope="module")
def plans():
    out = {}
    for case in sbc.CASES:
        plan = sbc.make_plan(case)
        out[case] = (plan, plan_arrays(plan)[0], sbc.gemm_launches(plan))
    return out


def _tiles(plans, case):
    _, segs, launches = plans[case]
    for ph, kernel, tiles in launches:
        for t in tiles:
            yield ph, kernel, t, sbc.task_segs(segs, t)


def _pairs(plans, case):
    """(task, Seg, next Seg) of every Seg boundary of the case's kind-kernel tiles."""
    for _, kernel, t, ss in _tiles(plans, case):
        if kernel is not None:
            for a, b in zip(ss, ss[1:]):
                yield kernel, t, a, b


@pytest.mark.parametrize("case", list(sbc.CASES))
def test_every_gemm_launch_lands_on_a_kind_kernel(plans, case):
    _, _, launches = plans[case]
    assert len(launches) >= 6
    for ph, kernel, tiles in launches:
        if sbc.CASES[case][0] == "odd" and ph.bf16 == 3:
            # The two forward launches whose operands have leading dimension 42 or 44 round fp32 operands in registers on three stages, and
            # TA3N_KIND_CONFIGS holds no forward kernel of that mode: they run the general kernel (old sequence) at every tile list.  The
            # case is about the backward launches, which must land on the mode-1 kind kernel with its 4-byte path.
            assert kernel is None
            continue
        assert kernel in sbc.KIND_KERNELS, (case, ph.wm, ph.wn, ph.wk, ph.bf16)
    kernels = {k for _, k, _ in launches}
    if sbc.CASES[case][1] == "f32x3p":
        assert {(2, 1, 4, 4, 3, 1), (1, 2, 4, 3, 2, 26), (1, 2, 2, 4, 2, 26)} <= kernels
    elif sbc.CASES[case][0] == "odd":
        assert [k for _, k, _ in launches[-2:]] == [(1, 2, 4, 1, 2, 26)] * 2
    else:
        assert {(1, 2, 4, 2, 3, 1), (1, 2, 4, 1, 2, 26), (2, 2, 2, 2, 2, 26)} <= kernels      # both K loops: three stages and two


@pytest.mark.parametrize("case", list(sbc.CASES))
def test_equal_and_changing_geometry(plans, case):
    same = [(k, t) for k, t, a, b in _pairs(plans, case) if sbc.seg_geometry(t, a) == sbc.seg_geometry(t, b)]
    diff = [(k, t) for k, t, a, b in _pairs(plans, case) if sbc.seg_geometry(t, a) != sbc.seg_geometry(t, b)]
    if sbc.CASES[case][0] == "T2":
        assert {k[4] for k, _ in same} == {3} and diff      # one tuple per scale: the two-stage kernels see changing geometry only
        return
    assert {k[4] for k, _ in same} == {2, 3}, case      # only the offsets change, in both K loops (two and three stages)
    assert diff, case                                   # ... and the leading dimension or the row limit changes inside a Seg list
    assert any(a.a_ld != b.a_ld or a.b_ld != b.b_ld for _, _, a, b in _pairs(plans, case))


def test_ragged_gradient_at_f1_tiles(plans):
    """Up to 12 Segs of exactly two full chunks beside the frame-discriminator Seg, whose leading dimensions, length and scale differ."""
    ch = sbc.chunk_k("bf16")
    best = 0
    for _, kernel, t, ss in _tiles(plans, "ragged_bf16"):
        if kernel == (2, 2, 2, 2, 2, 26) and len(ss) > 3:
            two = [s for s in ss if s.klen == 2 * ch]
            other = [s for s in ss if s.klen != 2 * ch]
            assert len(other) == 1 and other[0].scale_kind != SK_ONE and other[0].klen < ch
            assert (other[0].a_ld, other[0].b_ld) != (two[0].a_ld, two[0].b_ld)
            best = max(best, len(two))
    assert 8 <= best <= 12


def test_seg_counts_of_the_small_segment_numbers(plans):
    def counts(case, ns):
        return {len(ss) for _, kernel, t, ss in _tiles(plans, case) if kernel is not None and kernel[4] == ns}
    assert counts("T2_bf16", 3) == {1, 2} and counts("T2_bf16", 2) == {1, 2}
    assert {1, 2, 3} <= counts("T3_bf16", 3) and {1, 3, 4} <= counts("T3_bf16", 2)
    # one-Seg tiles beside multi-Seg tiles in one launch
    for case in ("T2_bf16", "T3_bf16"):
        _, _, launches = plans[case]
        assert any(len({t.seg_count for t in tiles}) > 1 and min(t.seg_count for t in tiles) == 1 for _, _, tiles in launches)
    # more Segs than either loop has stages
    assert max(counts("T12_bf16", 3)) == 12 and max(counts("T12_bf16", 2)) >= 20


def test_chunk_patterns(plans):
    ch = sbc.chunk_k("bf16")
    def klens(case, ns):
        return {s.klen for _, kernel, t, ss in _tiles(plans, case) if kernel is not None and kernel[4] == ns for s in ss}
    assert all(k < ch for k in klens("ragged_bf16", 3) if k != 2 * ch)       # every forward Seg of the first launches: one partial chunk
    assert 2 * ch in klens("ragged_bf16", 2)                                  # two full chunks
    assert {200, 264} <= klens("tails_bf16", 3)                               # a full chunk + 72, two full chunks + 8
    assert {140, 200, 2 * ch} <= klens("tails_bf16", 2)                       # 128 + 12 rows of a weight gradient, 128 + 72
    # seven row panels of 32, m_valid inside the last one
    rows = {(t.m0, t.m_valid) for _, kernel, t, _ in _tiles(plans, "tails_bf16") if kernel == (1, 2, 4, 2, 3, 1)}
    assert any(m0 + 32 > mv > m0 for m0, mv in rows)
    # the pair-twin chunk holds 64 k
    assert 256 in {s.klen for _, kernel, t, ss in _tiles(plans, "ragged_f32x3p") if kernel is not None for s in ss}


@pytest.mark.parametrize("case", list(sbc.CASES))
def test_a_scaled_seg_that_is_not_the_last(plans, case):
    assert any(s.scale_kind != SK_ONE for _, kernel, t, ss in _tiles(plans, case) if kernel is not None for s in ss[:-1]), case


def test_odd_runs_the_four_byte_path(plans):
    """No operand of the multi-Seg backward tiles can move 16 bytes at a time (OperandStream: vec false) on some Seg, and can on another."""
    vecs = set()
    for kernel, t, a, b in _pairs(plans, "odd_bf16"):
        if kernel == (1, 2, 4, 1, 2, 26):
            for s in (a, b):
                vecs.add(((s.a_off | s.a_ld | (s.klen if not s.a_kmajor else (t.m0 | (s.pad[0] if s.pad[0] > 0 else t.m_valid)))) & 3) == 0)
    assert False in vecs
