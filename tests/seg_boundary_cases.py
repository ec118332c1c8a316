"""One table of the shapes, tile lists and engine options at which the Seg boundaries of the GEMM tiles' K loops (ta3n_gemm_kernel.h:
SEG_EARLY - the two-stage loop of the twin kind kernels prepares the next Seg's stream state one chunk early, and a Seg's full chunks all
run the FULL body, its last one included) are tested, shared by tests/test_seg_boundary_cpu.py (the plans contain what the
table claims: no GPU) and tests/test_gpu_seg_boundary.py (the kernels).

  ragged   Bs 3, Bt 2, T 5, D 40, F 40, C 5: every forward Seg is one partial chunk; the gradient-at-F1 tiles carry up to 12 Segs of exactly
           two full chunks (NB 256 = 2 x 128 bf16) behind the frame-discriminator Seg (the tile's first), whose operands, leading dimensions and scale differ
  T2, T3   the same with 2 and 3 segments: one scale of one tuple / two scales of one and three tuples - tiles of one, two and three Segs,
           one-Seg tiles beside multi-Seg tiles in one launch
  T12      12 segments: the longest Seg lists the plan builds at a small shape, more Segs than either loop has stages
  tails    Bs 70, Bt 70, T 5, D 264, F 200, C 5: forward Segs of 128 + 72 k (a full chunk and a tail in every Seg), shared-FC K 264 (two
           full chunks + 8), weight-gradient Segs of 140 rows (128 + 12), seven row panels with m_valid past the last panel's rows
  odd      D 44, F 42: no operand moves 16 bytes at a time - the launches run the mode-1 kernels and the 4-byte path (vec false)"""
from plan_interp import EPI_COLSUM, EPI_ROWSUM_A, EPI_SGD, EPI_SPLITK, PH_GEMM, plan_arrays
from ta3n_amd import _lib
from ta3n_amd.engine import ALL_FLAGS
from ta3n_amd.tuning import tuned_phase_tiles

SHAPES = {
    "ragged": dict(Bs=3, Bt=2, T=5, D=40, F=40, C=5),
    "T2": dict(Bs=3, Bt=2, T=2, D=40, F=40, C=5),
    "T3": dict(Bs=3, Bt=2, T=3, D=40, F=40, C=5),
    "T12": dict(Bs=3, Bt=2, T=12, D=40, F=40, C=5),
    "tails": dict(Bs=70, Bt=70, T=5, D=264, F=200, C=5),
    "odd": dict(Bs=3, Bt=2, T=5, D=44, F=42, C=5),
}
HEADLINE_TILES = tuned_phase_tiles(202, 5, 2048, 512, True, True)
HEADLINE_TILES_PAIR = tuned_phase_tiles(202, 5, 2048, 512, False, True, split=True)
# "odd": an F = 42 plan rounds fp32 operands in registers (mode 1), so the 64x64 twin kernel is out of reach; the 32x64 tile on the last
# two launches puts them on the mode-1 kind kernel (tests/epilogue_operand_cases.py: the same list)
ODD_TILES = HEADLINE_TILES[:14] + [2124, 2124]

# case -> (shape, arithmetic, per-launch tile list).  All are twin cases on the headline's tile lists: every GEMM launch of the fused step
# lands on a kernel of TA3N_KIND_CONFIGS.
CASES = {
    "ragged_bf16": ("ragged", "bf16", HEADLINE_TILES),
    "T2_bf16": ("T2", "bf16", HEADLINE_TILES),
    "T3_bf16": ("T3", "bf16", HEADLINE_TILES),
    "T12_bf16": ("T12", "bf16", HEADLINE_TILES),
    "tails_bf16": ("tails", "bf16", HEADLINE_TILES),
    "odd_bf16": ("odd", "bf16", ODD_TILES),
    "ragged_f32x3p": ("ragged", "f32x3p", HEADLINE_TILES_PAIR),
}
ORACLE_CASES = ("tails_bf16", "T12_bf16")


def chunk_k(arith):
    """K elements per stage of the twin kernels (ta3n_gemm_kernel.h: CH) - 128 bf16, or 64 as a hi and a lo plane."""
    return 64 if arith == "f32x3p" else 128


def engine_kw(case):
    """TrainEngine keywords of a case (beside the shape and the dropout rates)."""
    _, arith, tiles = CASES[case]
    kw = dict(bf16=True, bf16_store=True) if arith == "bf16" else dict(f32_split=True, bf16_store=True)
    kw["phase_tiles"] = list(tiles)
    return kw


def make_plan(case):
    """The plan TrainEngine builds for the case."""
    shape, arith, tiles = CASES[case]
    sh = SHAPES[shape]
    flags = ALL_FLAGS | {"bf16": _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE, "f32x3p": _lib.FLAG_F32_SPLIT | _lib.FLAG_BF16_STORE}[arith]
    return _lib.Plan(sh["Bs"], sh["Bt"], sh["T"], sh["D"], sh["F"], sh["C"], flags, phase_tiles=list(tiles))


# TA3N_KIND_CONFIGS (wm, wn, wk, mode, stages, KV), in the order launch_gemm tries them
KIND_KERNELS = ((1, 2, 4, 2, 3, 1), (1, 2, 4, 1, 2, 26), (2, 2, 2, 2, 2, 26), (2, 1, 4, 4, 3, 1), (1, 2, 4, 3, 2, 26), (1, 2, 2, 4, 2, 26))


def gemm_launches(plan):
    """[(phase, kernel or None, [task])] of the fused step's GEMM launches: the kind-specialised kernel launch_gemm puts the launch on
    (ta3n_gemm.hip: tile, mode, stages and operand kinds of the launch), and its tiles that run a K loop."""
    _, tasks, phases, _, _, _ = plan_arrays(plan)
    out = []
    for ph in phases:
        if ph.kind != PH_GEMM or ph.group != 4:
            continue
        mode = 0 if ph.bf16 == 0 else ((4 if ph.bf16 & 32 else 2) if ph.bf16 & 16 else (3 if ph.bf16 & 32 else 1))
        ns = 2 if ph.bf16 == 0 else (3 if (ph.bf16 & 15) == 3 else 2)
        kinds, tiles = 0, []
        for ti in range(ph.task_begin, ph.task_begin + ph.task_count):
            t = tasks[ti]
            if t.epi & EPI_SPLITK:
                kinds |= 32
            if t.seg_count == 0 or (t.epi & (EPI_SGD | EPI_COLSUM)):
                continue
            kind = t.seg0.a_kmajor * 2 + t.seg0.b_kmajor
            kinds |= (1 << kind) if kind < 3 else (16 if t.epi & EPI_ROWSUM_A else 8)
            tiles.append(t)
        kernel = None
        if ph.chain_off < 0 and max(ph.rm, 1) * max(ph.rn, 1) == 1 and not (ph.bf16 & 64) and kinds:
            for k in KIND_KERNELS:
                if (ph.wm, ph.wn, ph.wk, mode, ns) == k[:5] and not (kinds & ~k[5]):
                    kernel = k
                    break
        out.append((ph, kernel, tiles))
    return out


def seg_geometry(task, sg):
    """What the per-lane stream state of a Seg depends on beside its offsets (OperandStream::setup): leading dimensions and the A row limit."""
    return (sg.a_ld, sg.b_ld, sg.pad[0] if sg.pad[0] > 0 else task.m_valid)


def task_segs(segs, task):
    return [segs[i] for i in range(task.seg_begin, task.seg_begin + task.seg_count)]
