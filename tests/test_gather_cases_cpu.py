"""The reference of the device batch assembly tests (tests/gather_cases.py), checked without a GPU: against the host mirror of the
reference's TSNDataSet, against the indices the reference itself produced, and the properties of its value table that
tests/test_gpu_gather_widths.py relies on."""
import os

import numpy as np
import pytest
import torch

import gather_cases as gc
from oracle import ta3n_oracle as orc
from ta3n_amd import _lib
from ta3n_amd.dataset import TSNDataSet

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_golden.npz"))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("D", [36, 1028])
def test_reference_builder_equals_the_host_dataset(tmp_path, D):
    """Rows, labels and frame numbers of the builder against ta3n_amd.dataset.TSNDataSet in test mode reading per-frame files."""
    T = 5
    c = gc.Case(T, D, seed=3, num_frames=(1, 2, 3, 4, 5, 6, 9, 17, 40, 101, 250), num_class=7)
    lst = c.write_frames(tmp_path)
    ds = TSNDataSet("", lst, num_dataload=len(c), num_segments=T, new_length=1, modality="RGB", test_mode=True)
    ids = [10, 0, 3, 3, 9, 1, 2, 4, 5, 6, 7, 8]
    ref = c.reference(ids)
    for k, vid in enumerate(ids):
        x, y = ds[vid]
        assert torch.equal(_bits(ref["x"][k * T:(k + 1) * T]), _bits(x)), (vid, D)
        assert int(ref["labels"][k]) == y
        assert ref["seg"][k * T:(k + 1) * T].tolist() == [int(v) for v in ds._get_test_indices(ds.video_list[vid])]
    # the bf16 store's reference: the same rows rounded, widened again; lo plane zero
    r16 = c.reference(ids, bf16_store=True)
    assert torch.equal(r16["hi"], ref["hi"]) and not r16["lo"].any()
    assert torch.equal(_bits(r16["x"]), _bits(ref["hi"].view(torch.bfloat16).to(torch.float32)))


@pytest.mark.parametrize("T", [3, 5, 9, 12, 25])
def test_reference_builder_indices_equal_the_reference_dataset(T):
    """segment_frames against tests/golden/index_golden.npz: what the REFERENCE's TSNDataSet._get_test_indices returned for 1..400 frames."""
    rows = GOLD[f"segidx_S{T}_L1"]
    assert rows.shape == (400, T + 1)
    for r in rows:
        assert gc.segment_frames(int(r[0]), T) == [int(v) for v in r[1:]], (T, int(r[0]))
    c = gc.Case(T, 1, num_frames=[int(r[0]) for r in rows[:60]])
    ids = list(range(59, -1, -1))
    assert c.segment_ids(ids).view(-1, T).tolist() == [[int(v) for v in rows[i, 1:]] for i in ids]
    assert c.store_rows(ids).view(-1, T).tolist() == [[int(c.first_row[i]) + int(v) - 1 for v in rows[i, 1:]] for i in ids]


@pytest.mark.parametrize("T", gc.INDEX_SEGMENTS)
def test_library_segment_indices_equal_the_oracle_at_other_segment_counts(T):
    for nf in list(range(1, 401)) + list(gc.LONG_CLIPS):
        want = [int(v) for v in orc.segment_indices_test_mode(nf, T, 1)]
        assert _lib.segment_indices(nf, T) == want, (T, nf)
        assert all(1 <= v <= nf for v in want) and want == sorted(want)


def test_value_table_is_what_the_gpu_tests_assume():
    tab = gc.value_table()
    bits = tab.view(torch.int32)
    assert tab.numel() == 2 * (gc.EXP_MAX - gc.EXP_MIN + 1) + 2 + 2 * len(gc.TIE_BITS)
    assert torch.isfinite(tab).all() and (tab > 0).any() and (tab < 0).any()
    have = set((bits.to(torch.int64) & 0xFFFFFFFF).tolist())
    for b in gc.TIE_BITS:
        assert b in have and (b | 0x80000000) in have, hex(b)
    assert 0x00000000 in have and 0x80000000 in have                        # +0.0 and -0.0
    for e in (gc.EXP_MIN, 0, gc.EXP_MAX):
        assert ((e + 127) << 23) in have and (((e + 127) << 23) | 0x80000000) in have
    expo = (bits >> 23) & 0xFF
    assert not ((expo == 0) & ((bits & 0x7FFFFF) != 0)).any(), "subnormal in the table"
    assert tab.abs().max().item() == 2.0 ** 126
    # the roundings the tie block is there for (RNE to 16 bits, worked out by hand): tie down to even, tie up to even, up, up, carry
    # through the mantissa, tie up with that carry, down just below a tie, carry into the exponent
    hi = torch.from_numpy(np.asarray(gc.TIE_BITS, dtype=np.uint32).view(np.float32).copy()).to(torch.bfloat16).view(torch.int16)
    assert [int(v) & 0xFFFF for v in hi.tolist()] == [0x3F80, 0x3F82, 0x3F81, 0x3F81, 0x3F80, 0x3F80, 0x7E7F, 0x7E80]


def test_row_values_stay_inside_the_range_the_split_is_specified_on():
    x = gc.row_values(1 << 10, 1 << 10, seed=5).reshape(-1)                    # 2^20 samples, table entries among them
    bits = x.view(torch.int32)
    assert torch.isfinite(x).all() and x.abs().max().item() <= 2.0 ** 126
    nz = x != 0
    assert x[nz].abs().min().item() >= 2.0 ** gc.EXP_MIN
    assert bits.unique().numel() > 0.85 * x.numel()                           # seven in eight are one-off patterns
    assert set(gc.value_table().view(torch.int32).tolist()) <= set(bits.tolist())     # every table entry occurs
    hi, lo = gc.split(x)
    hi_f, lo_f = hi.view(torch.bfloat16).to(torch.float64), lo.view(torch.bfloat16).to(torch.float64)
    assert torch.isfinite(hi_f).all() and torch.isfinite(lo_f).all()
    for plane in (hi, lo):      # no subnormal bf16 in either plane
        assert not ((((plane >> 7) & 0xFF) == 0) & ((plane & 0x7F) != 0)).any()
    rel = ((hi_f + lo_f - x.to(torch.float64)).abs()[nz] / x.to(torch.float64).abs()[nz]).max().item()
    assert rel <= 2.0 ** -17, rel
    assert torch.equal((hi_f + lo_f)[~nz], torch.zeros(int((~nz).sum()), dtype=torch.float64))
    # the tame values of the training cases
    t = gc.row_values(64, 64, seed=5, exps=(-6, -1), specials=False)
    assert t.abs().max().item() < 1.0 and t.abs().min().item() >= 2.0 ** -6


def test_id_lists_are_unsorted_with_duplicates_and_both_ends():
    for n_videos, n in ((12, 3), (12, 6), (12, 12), (403, 9)):
        ids = gc.id_list(n_videos, n, seed=n)
        assert len(ids) == n and all(0 <= v < n_videos for v in ids)
        assert 0 in ids and n_videos - 1 in ids and len(set(ids)) < n and ids != sorted(ids)
    tab = gc.id_table(12, 7, 5, seed=2)
    assert tab.shape == (7, 5) and tab.dtype == torch.int32 and len({tuple(r) for r in tab.tolist()}) > 1
    oth = gc.other_ids(tab, 12)
    assert oth.shape == tab.shape and oth.dtype == tab.dtype and (oth != tab).all() and oth.min() >= 0 and oth.max() < 12
