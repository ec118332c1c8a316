"""One table of the shapes, tile lists and engine options at which the early request of a GEMM tile's epilogue operands (ta3n_gemm_kernel.h:
EPI_EARLY) is tested, shared by tests/test_epilogue_operands_cpu.py (no launch writes what its tiles request early: the plans, no GPU) and
tests/test_gpu_epilogue_operands.py (the kernels), with `early_request_launches`, which reads from a PLAN which launches land on a kernel
that requests early and what their tiles carry.

  ragged      Bs 3, Bt 2, T 5, D 40, F 40, C 5: 5 / 25 valid rows in tiles of 32 or 64 (m_valid < 32), 40 of 64 columns (mostly padding)
  ragged_D36  the same with D 36 (fc_dim becomes min(F, D) = 36): 36 bf16 elements are no multiple of 16 bytes, so the gradient-at-F1 launch
              leaves the bf16 twins and with them the 64x64 kind kernel - its masked tiles run the general kernel (old order), the relation-level
              backward still requests early
  odd         D 44, F 42: leading dimension 42, so no float4 of F1 / gZ1 is 16-byte aligned (aux_vec false, the scalar path) and the last one
              of a row has two valid columns (nrem 2)
  T3          T 3: two scales, of one tuple and of three"""
from plan_interp import EPI_ADD, EPI_COLSUM, EPI_MASK, EPI_ROWSUM_A, EPI_SGD, EPI_SPLITK, PH_GEMM, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS
from ta3n_amd.tuning import tuned_phase_tiles

SHAPES = {
    "ragged": dict(Bs=3, Bt=2, T=5, D=40, F=40, C=5),
    "ragged_D36": dict(Bs=3, Bt=2, T=5, D=36, F=40, C=5),
    "odd": dict(Bs=3, Bt=2, T=5, D=44, F=42, C=5),
    "T3": dict(Bs=3, Bt=2, T=3, D=40, F=40, C=5),
}
HEADLINE_TILES = tuned_phase_tiles(202, 5, 2048, 512, True, True)
HEADLINE_TILES_PAIR = tuned_phase_tiles(202, 5, 2048, 512, False, True, split=True)
# "odd": no operand of an F = 42 plan moves 16 bytes at a time, so its launches round fp32 operands in registers (mode 1) and the
# 64x64 twin kernel is out of reach; the 32x64 tile on the last two launches puts the masked tiles on the mode-1 kind kernel instead
ODD_TILES = HEADLINE_TILES[:14] + [2124, 2124]

# case -> (shape, arithmetic, per-launch tile list (None: the plan's own choice), use_bn).  The twin cases take the headline's tile lists, which
# put the backward launches on the kind-specialised kernels; fp32 runs the general kernels.
CASES = {
    "ragged_f32": ("ragged", "f32", None, False),
    "ragged_D36_f32": ("ragged_D36", "f32", None, False),
    "odd_f32": ("odd", "f32", None, False),
    "T3_f32": ("T3", "f32", None, False),
    "ragged_adabn_f32": ("ragged", "f32", None, True),
    "ragged_bf16": ("ragged", "bf16", HEADLINE_TILES, False),
    "ragged_D36_bf16": ("ragged_D36", "bf16", HEADLINE_TILES, False),
    "odd_bf16": ("odd", "bf16", ODD_TILES, False),
    "T3_bf16": ("T3", "bf16", HEADLINE_TILES, False),
    "ragged_f32x3p": ("ragged", "f32x3p", HEADLINE_TILES_PAIR, False),
    "ragged_adabn_bf16": ("ragged", "bf16", HEADLINE_TILES, True),
}
TWIN_CASES = [n for n, c in CASES.items() if c[1] != "f32"]


def engine_kw(case):
    """TrainEngine keywords of a case (beside the shape and the dropout rates)."""
    _, arith, tiles, bn = CASES[case]
    kw = dict(bf16=True, bf16_store=True) if arith == "bf16" else dict(f32_split=True, bf16_store=True) if arith == "f32x3p" else {}
    if tiles is not None:
        kw["phase_tiles"] = list(tiles)
    if bn:
        kw["use_bn"] = "AdaBN"
    return kw


def make_plan(case):
    """The plan TrainEngine builds for the case."""
    shape, arith, tiles, bn = CASES[case]
    sh = SHAPES[shape]
    flags = ALL_FLAGS | (_lib.FLAG_BN_SHARED if bn else 0)
    flags |= {"f32": 0, "bf16": _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, "f32x3p": _lib.FLAG_F32_SPLIT | _lib.FLAG_BF16_STORE}[arith]
    return _lib.Plan(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], flags, phase_tiles=list(tiles) if tiles is not None else None)


# TA3N_KIND_CONFIGS without the two forward kernels (KV = 1), which keep the old order (EPI_EARLY); launch_gemm tries them in this order
KIND_KERNELS = ((1, 2, 4, 1, 2, 26), (2, 2, 2, 2, 2, 26), (1, 2, 4, 3, 2, 26), (1, 2, 2, 4, 2, 26))


def early_request_launches(plan):
    """[(kernel, facts)] of the fused step's GEMM launches that launch_gemm puts on a kind-specialised backward kernel (ta3n_gemm.hip: tile,
    mode, stages and operand kinds of the launch), with what their tiles carry: add / aux / the fan_counts that occur / an operand whose
    float4s are not 16-byte aligned."""
    _, tasks, phases, _, _, _ = plan_arrays(plan)
    out = []
    for ph in phases:
        if ph.kind != PH_GEMM or ph.group != 4 or ph.chain_off >= 0 or max(ph.rm, 1) * max(ph.rn, 1) > 1 or (ph.bf16 & 64):
            continue
        mode = 0 if ph.bf16 == 0 else ((4 if ph.bf16 & 32 else 2) if ph.bf16 & 16 else (3 if ph.bf16 & 32 else 1))
        ns = 2 if ph.bf16 == 0 else (3 if (ph.bf16 & 15) == 3 else 2)
        kinds, facts = 0, dict(add=False, aux=False, fans=set(), unaligned=False)
        for ti in range(ph.task_begin, ph.task_begin + ph.task_count):
            t = tasks[ti]
            if t.epi & EPI_SPLITK:
                kinds |= 32
            if t.seg_count == 0 or (t.epi & (EPI_SGD | EPI_COLSUM)):
                continue
            kind = t.seg0.a_kmajor * 2 + t.seg0.b_kmajor
            kinds |= (1 << kind) if kind < 3 else (16 if t.epi & EPI_ROWSUM_A else 8)
            facts["add"] |= bool(t.epi & EPI_ADD)
            facts["aux"] |= bool(t.epi & EPI_MASK)
            if t.fan_count:
                facts["fans"].add(int(t.fan_count))
            facts["unaligned"] |= bool((t.epi & EPI_MASK) and ((t.aux_off | t.aux_ld) & 3)) or bool((t.epi & EPI_ADD) and ((t.add_off | t.add_ld) & 3))
        for k in KIND_KERNELS:
            if (ph.wm, ph.wn, ph.wk, mode, ns) == k[:5] and kinds and not (kinds & ~k[5]):
                out.append((k, facts))
                break
    return out


def has(early, kernel, **want):
    """True if a launch of `early` runs `kernel` with the given facts."""
    return any(k == kernel and all(f[n] == v for n, v in want.items()) for k, f in early)


# what every twin case must land on (asserted from the plan on the CPU and again before the GPU steps): the relation-level backward - residual +
# fan-out masks, one store pass per thread - and the gradient-at-F1 launch with its masked tiles
def assert_lands_on_early_kernels(case, early):
    shape, arith, _, _ = CASES[case]
    l5 = (1, 2, 4, 3, 2, 26) if arith == "f32x3p" else (1, 2, 4, 1, 2, 26)
    assert has(early, l5, add=True, fans={1, 3}), (case, early)
    if arith == "f32x3p":
        assert has(early, (1, 2, 2, 4, 2, 26), aux=True, unaligned=False), (case, early)      # 32x64 on four waves: two passes per thread
    elif shape == "odd":
        assert has(early, (1, 2, 4, 1, 2, 26), aux=True, unaligned=True), (case, early)       # one pass, scalar path
    elif shape == "ragged_D36":
        assert not any(f["aux"] for _, f in early), (case, early)                              # masked tiles on the general kernel
    else:
        assert has(early, (2, 2, 2, 2, 2, 26), aux=True, unaligned=False), (case, early)      # 64x64 twin kernel: two passes per thread
