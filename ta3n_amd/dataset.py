"""TSNDataSet with the reference's constructor and item format (dataset.py:31-144):
a list file of `<dir> <num_frames> <label>` lines and one torch-saved 1-D feature
tensor per frame (`img_{:05d}.t7`).  All three segment samplers of the reference are
here, selected as dataset.py:118-126 selects them: the deterministic test-mode selection
(dataset.py:103-116 - the one main.py uses, main.py:171-197) comes from the C library and
is bit-exact; the val-mode selection (dataset.py:92-101) and the train mode's temporal
jitter (dataset.py:76-90) are the reference's arithmetic, the jitter drawing from
numpy.random with the reference's arguments in the reference's order, so that after
np.random.seed(s) the indices are the reference's.  (On the device the jitter draws from a
counter-based hash instead: ta3n_amd/feature_store.py.)  The file loading itself is outside
the timed path."""
import os

import numpy as np
import torch
import torch.utils.data as data

from . import _lib


class VideoRecord(object):
    def __init__(self, row):
        self._data = row

    @property
    def path(self):
        return self._data[0]

    @property
    def num_frames(self):
        return int(self._data[1])

    @property
    def label(self):
        return int(self._data[2])


class TSNDataSet(data.Dataset):
    def __init__(self, root_path, list_file, num_dataload, num_segments=3, new_length=1, modality='RGB',
                 image_tmpl='img_{:05d}.t7', transform=None, force_grayscale=False, random_shift=True,
                 test_mode=False):
        self.root_path, self.list_file = root_path, list_file
        self.num_segments, self.new_length, self.modality = num_segments, new_length, modality
        self.image_tmpl, self.transform = image_tmpl, transform
        self.random_shift, self.test_mode, self.num_dataload = random_shift, test_mode, num_dataload
        if modality in ('RGBDiff', 'RGBDiff2', 'RGBDiffplus'):
            self.new_length += 1                                         # dataset.py:47-48
        if modality == 'Flow':
            raise NotImplementedError("Flow features (x/y file pairs, dataset.py:62-66) are outside the TA3N hot path")
        self._parse_list()

    def _parse_list(self):
        """dataset.py:69-74: the list is repeated and truncated to num_dataload entries."""
        rows = [VideoRecord(x.strip().split(' ')) for x in open(self.list_file)]
        n_repeat = self.num_dataload // len(rows)
        n_left = self.num_dataload % len(rows)
        self.video_list = rows * n_repeat + rows[:n_left]

    def _sample_indices(self, record):
        """dataset.py:76-90: a uniform draw inside each segment's stretch; a sorted draw over the clip where the stretch is empty but
        the clip longer than num_segments (new_length >= 3 only); frame 1 otherwise."""
        T, selectable = self.num_segments, record.num_frames - self.new_length + 1
        stretch = selectable // T
        if stretch > 0:
            return np.arange(T) * stretch + np.random.randint(stretch, size=T) + 1
        if record.num_frames > T:
            return np.sort(np.random.randint(selectable, size=T)) + 1
        return np.ones((T,))

    def _get_val_indices(self, record):
        """dataset.py:92-101: the centre of each segment in float64; frame 1 for every segment of a clip that is too short."""
        T, selectable = self.num_segments, record.num_frames - self.new_length + 1
        if selectable < T:
            return np.ones((T,))
        tick = float(selectable) / float(T)
        return np.array([int(tick / 2.0 + tick * float(x)) for x in range(T)]) + 1

    def _get_test_indices(self, record):
        return _lib.segment_indices(record.num_frames, self.num_segments, self.new_length)

    def segment_indices(self, record):
        """The 1-based frame ids of `record`'s segments by the sampler the constructor selected (dataset.py:118-126)."""
        if not self.test_mode:
            return self._sample_indices(record) if self.random_shift else self._get_val_indices(record)
        return self._get_test_indices(record)

    def _load_feature(self, directory, idx):
        return [torch.load(os.path.join(directory, self.image_tmpl.format(idx)))]

    def __getitem__(self, index):
        record = self.video_list[index]
        frames = []
        for seg_ind in self.segment_indices(record):                     # dataset.py:128-144
            p = int(seg_ind)
            for _ in range(self.new_length):
                frames.extend(self._load_feature(record.path, p))
                if p < record.num_frames:
                    p += 1
        return torch.stack(frames), record.label

    def __len__(self):
        return len(self.video_list)
