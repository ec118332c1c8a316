"""Train- and val-mode segment indices produced by the REFERENCE ITSELF: TSNDataSet._sample_indices (dataset.py:76-90) and
TSNDataSet._get_val_indices (dataset.py:92-101), unmodified, imported through tests/golden/ref_shim.py.

Run in the build container only:

    python tests/golden/make_sampler_golden.py        # writes tests/golden/sampler_golden.npz

Cases: new_length L in {1, 2, 5} x num_segments T in {2, 3, 5, 9, 25, 64} x num_frames in frame_counts(T) =
{1, T-1, T, T+1, T+3, 2T-1, 2T, 2T+1, 47, 400} (duplicates dropped, order kept).  Per (L, T):

* ``nf_T{T}``          int64 [n]: the frame counts.
* ``val_L{L}_T{T}``    int64 [n, T]: _get_val_indices of each frame count.
* ``train_L{L}_T{T}``  int64 [3, n, 8, T]: for seed s in {0, 1, 2} and each frame count, np.random.seed(s) followed by eight consecutive
  _sample_indices calls.  A row of -1 where the reference raises (numpy refuses randint's bound: num_frames - new_length + 1 <= 0 in
  the sorted branch).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()
import dataset as ref_dataset  # noqa: E402  (the reference's, /root/reference/dataset.py)

assert os.path.realpath(ref_dataset.__file__).startswith("/root/reference/"), ref_dataset.__file__

NEW_LENGTHS, SEGMENTS, SEEDS, DRAWS = (1, 2, 5), (2, 3, 5, 9, 25, 64), (0, 1, 2), 8


def frame_counts(T):
    out = []
    for v in (1, T - 1, T, T + 1, T + 3, 2 * T - 1, 2 * T, 2 * T + 1, 47, 400):
        if v >= 1 and v not in out:
            out.append(v)
    return out


def main():
    store = {}
    for T in SEGMENTS:
        counts = frame_counts(T)
        store[f"nf_T{T}"] = np.asarray(counts, dtype=np.int64)
        for L in NEW_LENGTHS:
            ds = object.__new__(ref_dataset.TSNDataSet)          # the methods read two attributes only; __init__ wants list files
            ds.num_segments, ds.new_length = T, L
            val = np.zeros((len(counts), T), dtype=np.int64)
            train = np.full((len(SEEDS), len(counts), DRAWS, T), -1, dtype=np.int64)
            for i, nf in enumerate(counts):
                rec = types.SimpleNamespace(num_frames=nf)
                v = np.asarray(ref_dataset.TSNDataSet._get_val_indices(ds, rec))
                assert (v == v.astype(np.int64)).all()
                val[i] = v.astype(np.int64)
                for s in SEEDS:
                    np.random.seed(s)
                    for d in range(DRAWS):
                        try:
                            t = np.asarray(ref_dataset.TSNDataSet._sample_indices(ds, rec))
                        except ValueError:
                            continue                              # the reference raises: row stays -1
                        assert (t == t.astype(np.int64)).all() and (t >= 1).all()
                        train[s, i, d] = t.astype(np.int64)
            store[f"val_L{L}_T{T}"], store[f"train_L{L}_T{T}"] = val, train
    path = os.path.join(HERE, "sampler_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes;", len(store), "arrays")


if __name__ == "__main__":
    main()
