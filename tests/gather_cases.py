"""Shared table and CPU reference of the device batch assembly tests (tests/test_gather_cases_cpu.py, tests/test_gpu_gather_widths.py):
synthetic packed stores, the rows / labels / segment ids / twin planes a gather of given video ids must produce, and the widths, segment
counts and id lists the tests run.

The reference is plain torch / numpy on the CPU and shares no code with the library: the frames of a video come from the oracle's pure
Python restatement of TSNDataSet._get_test_indices (oracle.ta3n_oracle.segment_indices_test_mode), never from ta3n_amd._lib; the twin
planes are torch's own round-to-nearest-even conversion, hi = x.to(bfloat16), lo = (x - hi).to(bfloat16); a bf16 store holds
x.to(bfloat16) and its lo plane is all zero.  Every comparison against it is bit for bit (int32 / int16 views: -0.0 is not +0.0).

Row values (row_values): every element is a seeded random fp32 bit pattern - random sign, exponent 2^-100 .. 2^125, random 23-bit
mantissa - so a wrong row, column or plane changes bits; one element in eight is replaced by an entry of VALUE_TABLE: the powers
2^e, e in [-100, 126], both signs, +-0.0, and the fp32 patterns of TIE_BITS (and their negatives), whose bf16 rounding is a tie to even,
a tie to odd, just above a tie, or a carry into the exponent.
Excluded on purpose: NaN (the payload a converter leaves is unspecified); subnormals and anything above 2^126 (the project does not
specify the converter's denormal and overflow behaviour, and real features are ReLU outputs).  Over this range the split stays finite,
no plane is subnormal (the smallest non-zero lo is one fp32 ulp of 2^-100 = 2^-123) and hi + lo reconstructs x to within 2^-17 relative
(7.61e-6 measured over 2^20 samples) - checked on the CPU in tests/test_gather_cases_cpu.py."""
import functools

import numpy as np
import torch

from oracle.ta3n_oracle import segment_indices_test_mode

# fp32 patterns around the bf16 rounding boundary: a tie that goes down to even, a tie that goes up to even, above a tie, one fp32 ulp
# above a tie, a carry through the whole mantissa, a tie that goes up with that carry, and at the top of the range one ulp below a tie and
# the carry into the exponent (2^126)
TIE_BITS = (0x3F808000, 0x3F818000, 0x3F80C000, 0x3F808001, 0x3F7FFFFF, 0x3F7F8000, 0x7E7F7FFF, 0x7E7FFFFF)
EXP_MIN, EXP_MAX = -100, 126

F32_VECTOR_WIDTHS = (4, 36, 1020, 1024, 1028, 2048, 4096)      # D / 4 = 255, 256, 257 around the 256-thread row loop; 2 and 4 trips
F32_SCALAR_WIDTHS = (1, 37, 257, 1030)                         # D % 4 != 0: the element-wise copy of gather_row's fp32 body (ta3n_gather_segments only)
BF16_WIDTHS = (8, 2040, 2048, 2056, 4096)                      # D / 8 = 255, 256, 257; 2 trips
INDEX_SEGMENTS = (2, 7, 16, 33, 64)                            # segment counts beside the golden file's 3, 5, 9, 12, 25
LONG_CLIPS = (1000, 9999, 100003)


def _from_bits(bits) -> torch.Tensor:
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


@functools.lru_cache(maxsize=None)
def value_table() -> torch.Tensor:
    """The special values, fp32 [472]: +-2^e for e in [EXP_MIN, EXP_MAX], +-0.0, TIE_BITS and their negatives."""
    pw = torch.tensor([2.0 ** e for e in range(EXP_MIN, EXP_MAX + 1)], dtype=torch.float64).to(torch.float32)
    ties = _from_bits(TIE_BITS)
    return torch.cat([pw, -pw, torch.tensor([0.0, -0.0]), ties, -ties])


def row_values(n_rows: int, D: int, seed: int, exps=(EXP_MIN, EXP_MAX - 1), specials: bool = True) -> torch.Tensor:
    """fp32 [n_rows, D]: seeded random bit patterns with exponents in `exps` (inclusive; the random mantissa keeps every value below
    2^(exps[1] + 1)), one element in eight replaced by a VALUE_TABLE entry when `specials`."""
    rng = np.random.default_rng(seed)
    n = n_rows * D
    bits = (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) | \
           (rng.integers(exps[0] + 127, exps[1] + 128, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    if specials:
        tab = value_table().numpy().view(np.uint32)
        take = rng.integers(0, 8, n) == 0
        bits[take] = tab[rng.integers(0, tab.size, int(take.sum()))]
    return torch.from_numpy(bits.view(np.float32).copy()).view(n_rows, D)


def frame_counts(T: int):
    """A dozen videos: clips shorter than, equal to and just above T and 2T, and three lengths of real datasets."""
    return [max(1, v) for v in (T + 1, 400, 1, 2 * T - 1, 47, T, 2 * T, 101, T - 1, 13, 2 * T + 1, 64)]


def segment_frames(nf: int, T: int):
    """1-based frame numbers of a clip of nf frames in test mode: the oracle's Python restatement of the reference's sampler."""
    return [int(v) for v in segment_indices_test_mode(int(nf), int(T), 1)]


def split(x: torch.Tensor):
    """(hi, lo) bit patterns (int16) of the pair-twin split of fp32 x."""
    x = x.to(torch.float32)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def id_list(n_videos: int, n: int, seed: int):
    """n video ids, unsorted; from three ids on the list holds the first and the last video of the store and one id twice."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n_videos, (n,), generator=g).tolist()
    if n >= 3:
        ids[0], ids[1], ids[n - 1] = n_videos - 1, 0, n_videos - 1
    return ids


def id_table(n_videos: int, steps: int, n: int, seed: int) -> torch.Tensor:
    """int32 [steps, n]: one id_list per step."""
    return torch.tensor([id_list(n_videos, n, seed + 131 * k) for k in range(steps)], dtype=torch.int32).view(steps, n)


def other_ids(table: torch.Tensor, n_videos: int) -> torch.Tensor:
    """A table of the same shape and dtype whose every entry is another valid id."""
    return ((table.to(torch.int64) + 1 + (torch.arange(table.numel()).view(table.shape) % max(n_videos - 1, 1))) % n_videos).to(table.dtype)


class Case:
    """A synthetic packed dataset on the CPU and the reference of any gather from it."""

    def __init__(self, T: int, D: int, seed: int = 0, num_frames=None, num_class: int = 5, **values):
        self.T, self.D = int(T), int(D)
        self.num_frames = [int(v) for v in (num_frames if num_frames is not None else frame_counts(T))]
        self.first_row = np.concatenate(([0], np.cumsum(self.num_frames)[:-1])).astype(np.int64)
        self.rows = row_values(sum(self.num_frames), D, seed=1000 * seed + 7 * D + T, **values)
        self.labels = torch.randint(0, num_class, (len(self.num_frames),), generator=torch.Generator().manual_seed(seed + 17), dtype=torch.int32)

    def __len__(self):
        return len(self.num_frames)

    # ---- the reference ----
    def segment_ids(self, ids) -> torch.Tensor:
        """int32 [len(ids) * T]: the 1-based frame numbers, video by video."""
        return torch.tensor([f for v in ids for f in segment_frames(self.num_frames[int(v)], self.T)], dtype=torch.int32).view(-1)

    def store_rows(self, ids) -> torch.Tensor:
        """int64 [len(ids) * T]: the rows of the packed store a gather of `ids` reads, in output order."""
        first = torch.tensor([int(self.first_row[int(v)]) for v in ids for _ in range(self.T)], dtype=torch.int64).view(-1)
        return first + self.segment_ids(ids).to(torch.int64) - 1

    def reference(self, ids, bf16_store: bool = False):
        """dict of what a gather of `ids` must leave: x fp32 [n T, D] (a bf16 store: its rows widened), hi / lo int16 [n T, D] twin
        planes (a bf16 store: the stored bits and zeros), labels int32 [n], seg int32 [n T]."""
        ids = [int(v) for v in (ids.tolist() if torch.is_tensor(ids) else ids)]
        x = self.rows[self.store_rows(ids)].view(len(ids) * self.T, self.D)
        if bf16_store:
            hi = x.to(torch.bfloat16)
            x, hi, lo = hi.to(torch.float32), hi.view(torch.int16), torch.zeros(x.shape, dtype=torch.int16)
        else:
            hi, lo = split(x)
        return dict(x=x, hi=hi, lo=lo, seg=self.segment_ids(ids),
                    labels=self.labels[torch.tensor(ids, dtype=torch.int64)].view(-1) if ids else self.labels[:0])

    # ---- the stores on the device ----
    def store(self, bf16: bool = False):
        """FeatureStore.from_tensors over the rows (bf16: their RNE roundings as int16 bit patterns) on the current device."""
        from ta3n_amd.feature_store import FeatureStore
        rows = self.rows.to(torch.bfloat16).view(torch.int16) if bf16 else self.rows
        return FeatureStore.from_tensors(rows.cuda().contiguous(), torch.tensor(self.num_frames), self.labels)

    # ---- the same dataset as per-frame files (the host mirror's input) ----
    def write_frames(self, directory) -> str:
        """One torch-saved 1-D tensor per frame + the list file, as the reference's datasets are laid out; returns the list file."""
        lines = []
        for v, (first, n) in enumerate(zip(self.first_row.tolist(), self.num_frames)):
            d = directory / f"vid{v}"
            d.mkdir()
            for f in range(n):
                torch.save(self.rows[first + f].clone(), str(d / f"img_{f + 1:05d}.t7"))
            lines.append(f"{d}/ {n} {int(self.labels[v])}")
        lst = directory / "list.txt"
        lst.write_text("\n".join(lines) + "\n")
        return str(lst)


@functools.lru_cache(maxsize=None)
def case(T: int, D: int, seed: int = 0, train: bool = False) -> Case:
    """Cached Case (treat as read-only).  train: tame values (2^-6 .. 1, no table entries) a train step stays finite on - still one
    random mantissa per element."""
    return Case(T, D, seed, num_class=5, **(dict(exps=(-6, -1), specials=False) if train else {}))
