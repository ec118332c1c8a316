"""The train- and val-mode segment samplers on the host: ta3n_amd.dataset.TSNDataSet(test_mode=False) against the reference's own indices
(tests/golden/sampler_golden.npz, written by tests/golden/make_sampler_golden.py from the unmodified reference), and the rule the device
kernels share with ta3n_sample_segments against the fixture (val), against ta3n_segment_indices (test) and against the pure-Python
restatement of tests/sampler_reference.py (train) - bit for bit - plus what a sampler has to be: inside the reference's interval,
uniform, keyed by (seed, step, slot) and by nothing else.  No GPU."""
import ctypes as C
import functools
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import gather_cases as gc
import sampler_reference as sr
from ta3n_amd import _lib
from ta3n_amd.dataset import TSNDataSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "sampler_golden.npz"))
NEW_LENGTHS, SEGMENTS, SEEDS, DRAWS = (1, 2, 5), (2, 3, 5, 9, 25, 64), (0, 1, 2), 8


def _counts(T):
    return [int(v) for v in GOLDEN[f"nf_T{T}"]]


def test_fixture_holds_the_cases():
    for T in SEGMENTS:
        want = []
        for v in (1, T - 1, T, T + 1, T + 3, 2 * T - 1, 2 * T, 2 * T + 1, 47, 400):
            if v >= 1 and v not in want:
                want.append(v)
        assert _counts(T) == want
        for L in NEW_LENGTHS:
            assert GOLDEN[f"val_L{L}_T{T}"].shape == (len(want), T)
            assert GOLDEN[f"train_L{L}_T{T}"].shape == (len(SEEDS), len(want), DRAWS, T)
        assert (GOLDEN[f"train_L1_T{T}"] >= 1).all() and (GOLDEN[f"train_L2_T{T}"] >= 1).all()      # the reference raises for new_length 5 only


# ---- 1. the host dataset, through __getitem__ on per-frame files ----
def _expected_item(case, v, indices, L):
    """Rows TSNDataSet.get (dataset.py:128-144) stacks for 1-based `indices`: new_length consecutive frames, stopping at the clip's end."""
    nf, first = case.num_frames[v], int(case.first_row[v])
    rows = []
    for p in indices:
        p = int(p)
        for _ in range(L):
            rows.append(first + p - 1)
            if p < nf:
                p += 1
    return case.rows[torch.tensor(rows, dtype=torch.int64)]


@pytest.mark.parametrize("T", SEGMENTS)
def test_dataset_reproduces_the_reference_indices_through_getitem(T, tmp_path, monkeypatch):
    counts = _counts(T)
    case = gc.Case(T, 2, seed=3, num_frames=counts)
    assert len(set(case.rows.contiguous().view(torch.int64).view(-1).tolist())) == case.rows.shape[0]      # a row names its frame
    lst = case.write_frames(tmp_path)
    # every frame file is read once: the items of this test read each of them hundreds of times (a memo in front of torch.load - the
    # dataset still builds every path and walks every frame itself)
    monkeypatch.setattr(torch, "load", functools.lru_cache(maxsize=None)(torch.load))
    for L in NEW_LENGTHS:
        val = TSNDataSet("", lst, num_dataload=len(counts), num_segments=T, new_length=L, random_shift=False, test_mode=False)
        train = TSNDataSet("", lst, num_dataload=len(counts), num_segments=T, new_length=L)      # the class's own defaults
        assert train.random_shift and not train.test_mode and len(train) == len(counts)
        for v in range(len(counts)):
            x, y = val[v]
            assert y == int(case.labels[v]) and x.shape == (T * L, 2)
            assert torch.equal(x.view(torch.int32), _expected_item(case, v, GOLDEN[f"val_L{L}_T{T}"][v], L).view(torch.int32)), (L, counts[v])
            assert np.array_equal(np.asarray(val.segment_indices(val.video_list[v])).astype(np.int64), GOLDEN[f"val_L{L}_T{T}"][v])
            for s in SEEDS:
                np.random.seed(s)
                for d in range(DRAWS):
                    want = GOLDEN[f"train_L{L}_T{T}"][s, v, d]
                    if (want < 0).all():                     # the reference raises here (numpy refuses randint's bound)
                        with pytest.raises(ValueError):
                            train[v]
                        continue
                    x, y = train[v]
                    assert y == int(case.labels[v])
                    assert torch.equal(x.view(torch.int32), _expected_item(case, v, want, L).view(torch.int32)), (L, counts[v], s, d)


def test_dataset_keeps_test_mode_and_refuses_flow(tmp_path):
    case = gc.Case(3, 2, seed=4, num_frames=[1, 2, 7])
    lst = case.write_frames(tmp_path)
    ds = TSNDataSet("", lst, num_dataload=3, num_segments=3, random_shift=False, test_mode=True)
    for v in range(3):
        assert torch.equal(ds[v][0], case.reference([v])["x"])
    with pytest.raises(NotImplementedError, match="Flow"):
        TSNDataSet("", lst, num_dataload=3, num_segments=3, modality="Flow")


# ---- 2. VAL and TEST of the shared rule ----
def test_val_rule_equals_the_reference_and_test_rule_equals_segment_indices():
    for T in SEGMENTS:
        for i, nf in enumerate(_counts(T)):
            for key in ((0, 0, 0), (7, 3, 2)):             # neither sampler reads the key
                assert _lib.sample_segments("val", nf, T, *key) == GOLDEN[f"val_L1_T{T}"][i].tolist() == sr.frames("val", nf, T)
                assert _lib.sample_segments("test", nf, T, *key) == _lib.segment_indices(nf, T) == sr.frames("test", nf, T)
    out = (C.c_int64 * 4)()
    L = _lib.lib()
    assert L.ta3n_sample_segments(3, 10, 4, 0, 0, 0, out) != 0 and L.ta3n_sample_segments(-1, 10, 4, 0, 0, 0, out) != 0
    assert L.ta3n_sample_segments(2, 0, 4, 0, 0, 0, out) != 0 and L.ta3n_sample_segments(2, 10, 4, 0, 0, 0, None) != 0


# ---- 3. TRAIN against the pure-Python restatement ----
TRAIN_SEEDS = (0, 1, 0x9E3779B9, 0xFFFFFFFF)


def test_train_rule_equals_the_python_restatement():
    L = _lib.lib()
    n = 0
    for T in SEGMENTS:
        out = (C.c_int64 * T)()
        for nf in _counts(T):
            for seed in TRAIN_SEEDS:
                for step in (0, 1, 2 ** 32 - 1):
                    for slot in (0, 1, 255):
                        assert L.ta3n_sample_segments(2, nf, T, seed, step, slot, out) == 0
                        assert list(out) == sr.frames("train", nf, T, seed, step, slot), (nf, T, seed, step, slot)
                        n += 1
    assert n == sum(len(_counts(T)) for T in SEGMENTS) * 36


# ---- 4. structure: the reference's interval ----
def test_train_draws_lie_in_the_interval_of_the_reference():
    for T in SEGMENTS:
        x = np.arange(T)
        for i, nf in enumerate(_counts(T)):
            avg = nf // T
            ours = np.array([_lib.sample_segments("train", nf, T, seed, step, slot) for seed in (0, 5) for step in range(8) for slot in (0, 3)])
            theirs = GOLDEN[f"train_L1_T{T}"][:, i].reshape(-1, T)
            for name, draws in (("library", ours), ("reference", theirs)):
                if nf >= T:
                    assert (draws >= x * avg + 1).all() and (draws <= (x + 1) * avg).all(), (name, nf, T)
                else:
                    assert (draws == 1).all(), (name, nf, T)


# ---- 5. uniformity ----
@functools.lru_cache(maxsize=None)
def _residues(seed=20240229):
    """int [70000, 5]: the residues r of 1000 steps x 70 slots at nf = 35, T = 5 (avg = 7), one fixed seed."""
    L = _lib.lib()
    out = (C.c_int64 * 5)()
    rows = np.empty((70000, 5), dtype=np.int64)
    k = 0
    for step in range(1000):
        for slot in range(70):
            assert L.ta3n_sample_segments(2, 35, 5, seed, step, slot, out) == 0
            rows[k] = out
            k += 1
    return rows - 1 - 7 * np.arange(5)


def test_train_draw_is_uniform_per_segment_and_pairwise():
    r = _residues()
    assert r.min() == 0 and r.max() == 6
    bound = 5.0 * math.sqrt(70000 * (1 / 7) * (6 / 7))      # 5 binomial standard deviations: 463
    assert 462 < bound < 464
    for x in range(5):
        counts = np.bincount(r[:, x], minlength=7)
        print("segment", x, counts.tolist())
        assert np.abs(counts - 10000).max() <= bound, (x, counts)
    pair_bound = 5.0 * math.sqrt(70000 * (1 / 49) * (48 / 49))
    pairs = np.bincount(r[:, 0] * 7 + r[:, 1], minlength=49)
    print("pairs", pairs.tolist())
    assert np.abs(pairs - 70000 / 49).max() <= pair_bound, pairs


# ---- 6. the key ----
def test_every_key_changes_the_draw_and_nothing_else_does():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 2 ** 32, size=(1000, 3), dtype=np.uint64)
    for which in range(3):                                    # seed, step, slot
        changed = 0
        for k, (seed, step, slot) in enumerate(base.tolist()):
            other = [seed, step, slot]
            other[which] = (other[which] + 1 + k % 5) % 2 ** 32
            changed += _lib.sample_segments("train", 35, 5, seed, step, slot) != _lib.sample_segments("train", 35, 5, *other)
        print(("seed", "step", "slot")[which], changed)
        assert changed >= 900, (which, changed)
    # the rule has no other input: its signature is (sampler, num_frames, num_segments, seed, step, slot) - the video id and first_video
    # never reach it (on the device: tests/test_gpu_sampler.py gathers the same video at two slots and at two first_video)
    assert _lib.lib().ta3n_sample_segments.argtypes[:6] == [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    case = gc.case(5, 4)
    for ids in ([1, 1, 4, 1], [4, 1, 1, 1]):
        ref = sr.reference(case, ids, "train", seed=9, step=2)
        for s, v in enumerate(ids):
            assert ref["seg"][s * 5:(s + 1) * 5].tolist() == _lib.sample_segments("train", case.num_frames[v], 5, 9, 2, s)


# ---- 7. the ABI ----
def test_feed_layout_and_sampler_names(tmp_path):
    f = _lib.Feed()
    assert (f.sampler, f.seed, f.step0) == (0, 0, 0)
    assert [n for n, _ in _lib.Feed._fields_[-3:]] == ["sampler", "seed", "step0"]
    src = tmp_path / "feed_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ta3n_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ta3n_feed), offsetof(ta3n_feed, sampler), offsetof(ta3n_feed, seed), '
                   'offsetof(ta3n_feed, step0)); return 0; }\n')
    exe = tmp_path / "feed_size"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(_lib.Feed), _lib.Feed.sampler.offset, _lib.Feed.seed.offset, _lib.Feed.step0.offset], sizes
    assert [_lib.sampler_code(n) for n in ("test", "val", "train")] == [0, 1, 2] and _lib.sampler_code(2) == 2
    for bad in ("jitter", 3, None, True):
        with pytest.raises(ValueError, match="'test', 'val', 'train'"):
            _lib.sampler_code(bad)


def test_feature_store_refuses_an_unknown_sampler():
    """FeatureStore.gather / gather_into / sampled name the three samplers before anything reaches the device (a store needs one to be
    built, so the methods are called on a bare instance: the sampler is checked first)."""
    from ta3n_amd.feature_store import FeatureStore
    store = object.__new__(FeatureStore)
    ids = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: store.gather(ids, 3, sampler="jitter"), lambda: store.gather_into(types.SimpleNamespace(), ids, 0, sampler="jitter"),
                 lambda: store.sampled("jitter", 1)):
        with pytest.raises(ValueError, match="'test', 'val', 'train'"):
            call()
    view = FeatureStore.sampled(store, "train", 5)
    assert (view.sampler, view.seed) == (2, 5) and (FeatureStore.sampler, FeatureStore.seed) == (0, 0)


# ---- 8. train_ddp's option ----
def test_train_ddp_segment_sampler_option():
    import train_ddp
    from ta3n_amd.opts import parser
    base = ["c", "RGB", "s", "t", "v", "--baseline_type", "video", "--frame_aggregation", "trn-m"]
    args = parser.parse_args(base)
    assert not hasattr(args, "segment_sampler")
    train_ddp.validate_options(args)                          # every command line accepted so far carries no such attribute
    for sampler in ("val", "train"):
        args = parser.parse_args(base)
        args.segment_sampler, args.feature_store = sampler, None
        with pytest.raises(SystemExit, match=f"--segment_sampler {sampler} without --feature_store"):
            train_ddp.validate_options(args)
        args.feature_store = ["src", "tgt", "val"]
        train_ddp.validate_options(args)
    args.segment_sampler = "jitter"
    with pytest.raises(SystemExit, match="--segment_sampler jitter"):
        train_ddp.validate_options(args)
    args.segment_sampler, args.feature_store = "test", None
    train_ddp.validate_options(args)
    seeds = {train_ddp.sampler_seed(d, r) for d in (0, 1) for r in range(8)}
    assert len(seeds) == 16
