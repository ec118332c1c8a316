"""Pure-Python restatement of the device segment samplers (include/ta3n_hip.h "sampler key"), for tests/test_sampler_cpu.py and
tests/test_gpu_sampler.py.  It shares no code with the library and never touches ta3n_amd._lib: the hash is written from the header's
description, the test-mode frames come from the oracle's restatement of the reference (gather_cases.segment_frames), the val-mode
arithmetic is the reference's float64 expression in Python floats.

    frames(sampler, nf, T, seed, step, slot)  1-based frame numbers of the T segments of a clip of nf frames (new_length 1)
    reference(case, ids, sampler, seed, step, bf16_store)  what a gather of `ids` from a gather_cases.Case must leave, like Case.reference
"""
import torch

TEST, VAL, TRAIN = 0, 1, 2
CODES = {"test": TEST, "val": VAL, "train": TRAIN}
M32 = 0xFFFFFFFF


def mix32(v: int) -> int:
    v &= M32
    v ^= v >> 16
    v = (v * 0x7FEB352D) & M32
    v ^= v >> 15
    v = (v * 0x846CA68B) & M32
    v ^= v >> 16
    return v


def draw(seed: int, step: int, slot: int, x: int, avg: int) -> int:
    """r in [0, avg): the high half of the 64-bit product of the key's hash and avg."""
    h = mix32(mix32(mix32(mix32((seed & M32) ^ 0x9E3779B9) ^ (step & M32)) ^ (slot & M32)) ^ (x & M32))
    return (h * avg) >> 32


def frames(sampler, nf: int, T: int, seed: int = 0, step: int = 0, slot: int = 0):
    sampler = CODES.get(sampler, sampler)
    if sampler == TEST:
        from gather_cases import segment_frames
        return segment_frames(nf, T)
    if sampler == VAL:
        if nf < T:
            return [1] * T
        tick = float(nf) / float(T)
        return [int(tick / 2.0 + tick * float(x)) + 1 for x in range(T)]
    assert sampler == TRAIN
    avg = nf // T
    if avg == 0:
        return [1] * T
    return [x * avg + draw(seed, step, slot, x, avg) + 1 for x in range(T)]


def reference(case, ids, sampler, seed: int = 0, step: int = 0, bf16_store: bool = False):
    """gather_cases.Case.reference for a sampler: x, hi, lo, labels, seg of a gather of `ids` whose slot s is ids[s]."""
    from gather_cases import split
    ids = [int(v) for v in (ids.tolist() if torch.is_tensor(ids) else ids)]
    seg = [f for s, v in enumerate(ids) for f in frames(sampler, case.num_frames[v], case.T, seed, step, s)]
    rows = torch.tensor([int(case.first_row[v]) + f - 1 for v, f in zip([v for v in ids for _ in range(case.T)], seg)], dtype=torch.int64)
    x = case.rows[rows].view(len(ids) * case.T, case.D)
    if bf16_store:
        hi = x.to(torch.bfloat16)
        x, hi, lo = hi.to(torch.float32), hi.view(torch.int16), torch.zeros(x.shape, dtype=torch.int16)
    else:
        hi, lo = split(x)
    return dict(x=x, hi=hi, lo=lo, seg=torch.tensor(seg, dtype=torch.int32),
                labels=case.labels[torch.tensor(ids, dtype=torch.int64)].view(-1) if ids else case.labels[:0])
