"""Scoring without the training step: `Scorer` classifies videos on a score-only plan (TA3N_FLAG_SCORE_ONLY, include/ta3n_hip.h).

What main.validate (reference main.py:707-735) and test_models.py (:155-198) need from the model is the class logits of an eval-mode
forward and the bookkeeping on them.  A score-only plan holds exactly that: the launches the logits depend on, over `capacity` rows that
are all alike, and one kernel from the aggregated feature to probabilities, ranks, top-k hits and the confusion matrix.  Its parameter
layout is the training plan's of the same options, so a `TrainEngine`'s or a `VideoModel`'s flat parameter buffer is scored as it is.

    scorer = Scorer.from_engine(engine)               # or Scorer.from_model(model, capacity=64), or Scorer(...) + load_params(...)
    scorer.score(data, labels, reset=True)            # any number of videos, in chunks of `capacity`
    scorer.results()                                  # dict(loss, prec1, prec5, n, confusion): the shape of TrainEngine.eval_results()
    scorer.per_video()                                # dict(logits, prob, rank, pred, feat_v, attn) of the videos scored since the reset
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib

_AGGREGATIONS = {"trn-m": _lib.AGG_TRN_M, "avgpool": _lib.AGG_AVGPOOL, "rnn": _lib.AGG_RNN, "temconv": _lib.AGG_TEMCONV}
# flags that change neither the parameter layout nor the logits (and that a plan without target rows refuses)
_NO_EFFECT = _lib.FLAG_TARGET_LABELS | _lib.FLAG_TARGET_ENTROPY


def default_flags(aggregation: str, use_attn: str) -> int:
    """The flags of the training configuration whose parameters are scored when the caller names none: TrainEngine's defaults for trn-m
    and avgpool, VideoModel's for rnn and temconv."""
    if aggregation == "trn-m":
        adv = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME
        return adv | (_lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN if use_attn == "TransAttn" else 0)
    if aggregation == "avgpool":
        return 0
    return _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_FEATURE_GRADS


class Scorer:
    def __init__(self, num_segments: int, feature_dim: int, fc_dim: int, num_class: int, capacity: int, aggregation: str = "trn-m",
                 use_attn: str = "TransAttn", flags: Optional[int] = None, rnn_cell: str = "LSTM", n_ts: int = 5,
                 device: Optional[torch.device] = None, add_fc: int = 1):
        """flags: the TA3N_FLAG_* of the training configuration whose parameters are scored (None: default_flags).  add_fc: the model's
        --add_fc, which from_model / from_engine pass on so that 2 and 3 are refused here with the library's sentence (only 1 is built)."""
        if aggregation not in _AGGREGATIONS:
            raise NotImplementedError(f"frame_aggregation {aggregation!r} (built: {', '.join(_AGGREGATIONS)})")
        if use_attn not in ("TransAttn", "none", "general"):
            raise NotImplementedError(f"use_attn {use_attn!r}")
        if capacity < 1:
            raise ValueError("capacity must be positive")
        if flags is None:
            flags = default_flags(aggregation, use_attn) | (_lib.FLAG_GENERAL_ATTN if use_attn == "general" else 0)
        self.flags = (int(flags) & ~_NO_EFFECT) | _lib.FLAG_SCORE_ONLY
        self.aggregation, self.capacity = aggregation, int(capacity)
        self.T, self.D, self.C = int(num_segments), int(feature_dim), int(num_class)
        # (share_params N is refused whatever the rows; with target rows the refusal is the score-only one, not the training plan's about rows)
        target_rows = 1 if self.flags & _lib.FLAG_UNSHARED else 0
        try:      # what is not built is refused by the plan builder, by name; its sentence is the message
            self.plan = _lib.Plan(self.capacity, target_rows, self.T, self.D, int(fc_dim), self.C, self.flags, aggregation=_AGGREGATIONS[aggregation],
                                  shared_fc_layers=int(add_fc), rnn_cell=_lib.RNN_CELLS[rnn_cell] if aggregation == "rnn" else 0,
                                  n_ts=int(n_ts) if aggregation == "rnn" else 0)
        except ValueError as e:
            if "TA3N_FLAG_SCORE_ONLY with" in str(e):
                raise NotImplementedError(str(e)) from None
            raise
        self._engine = None
        self._model = None
        self.P: Optional[torch.Tensor] = None
        self._kept: list = []
        self._L = None
        self.device = torch.device(device) if device is not None else None
        self.ws: Optional[torch.Tensor] = None

    # ---- where the parameters come from ----
    @classmethod
    def from_model(cls, model, capacity: int, num_segments: Optional[int] = None) -> "Scorer":
        """A scorer on a VideoModel's flat parameter buffer (model._flat: shared, not copied - an in-place change of a parameter is seen by
        the next score()).  num_segments defaults to the model's val_segments; a count other than the training one is a plan of its own
        where the aggregation allows it (not trn-m: its relation module is built for train_segments)."""
        T = int(model.val_segments if num_segments is None else num_segments)
        if T != model.train_segments and not model._avg:
            raise ValueError("num_segments must equal train_segments for frame_aggregation 'trn-m' (the relation module is built for train_segments)")
        device = next(model.parameters()).device
        if device.type != "cuda":
            device = None      # (the current HIP device, at the first score())
        self = cls(T, model.feature_dim, model._feat_dim_F, model.num_class, capacity, aggregation=model.frame_aggregation,
                   use_attn=model.use_attn, flags=model._flags(), rnn_cell=model.rnn_cell, n_ts=model.n_ts, device=device, add_fc=model.add_fc)
        self._model = model
        return self

    @classmethod
    def from_engine(cls, engine, capacity: Optional[int] = None) -> "Scorer":
        """A scorer on a TrainEngine's parameter buffer (engine.P: shared).  Every score() first calls engine.flush(), so an update that a
        pipelined step left pending is applied before the parameters are read."""
        self = cls(engine.T, engine.D, engine.F, engine.C, engine.B if capacity is None else capacity, aggregation=engine.aggregation,
                   flags=engine._flags, device=engine.device, add_fc=engine.add_fc)
        self._engine = engine
        return self

    def load_params(self, params) -> None:
        """A flat tensor laid out as the plan's parameters (plan.params), or a state_dict under the reference's names."""
        self._engine = self._model = None
        self._ensure_buffers()
        if self.P is None:
            self.P = torch.zeros(self.plan.param_floats, dtype=torch.float32, device=self.device)
        if isinstance(params, torch.Tensor):
            if params.numel() != self.plan.param_floats:
                raise ValueError(f"flat parameters: {params.numel()} floats, the plan has {self.plan.param_floats}")
            self.P.copy_(params.reshape(-1).to(device=self.device, dtype=torch.float32))
            return
        for name, off, shape, _ in self.plan.params:
            if name in params:
                n = 1
                for s in shape:
                    n *= s
                self.P[off:off + n].copy_(params[name].reshape(-1).to(device=self.device, dtype=torch.float32))

    # ---- plumbing ----
    def _ensure_buffers(self) -> None:
        if self.ws is not None:
            return
        if not torch.cuda.is_available():
            raise _lib.Ta3nError("Scorer needs a HIP device; there is no CPU fallback")
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._L = _lib.lib()
        with torch.cuda.device(self.device):
            self.ws = torch.zeros(self.plan.ws_floats, dtype=torch.float32, device=self.device)
            self.X = torch.zeros(self.capacity * self.T, self.D, dtype=torch.float32, device=self.device)
            _lib.check(self._L.ta3n_init_workspace(self.plan.handle, self.ws.data_ptr(), self._stream()), "ta3n_init_workspace")
        off, n = self.plan.region("labels")
        self._labels = self.ws[off:off + n].view(torch.int32)
        # the per-video results lie back to back in the workspace: one copy per call keeps them for per_video()
        first = "attn" if "attn" in self.plan.regions else "V"
        self._kept_span = (self.plan.region(first)[0], sum(self.plan.region("ce")))

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _params(self) -> torch.Tensor:
        if self._engine is not None:
            self._engine.flush()
            return self._engine.P
        if self._model is not None:
            self._model._ensure_flat(self.plan, self.device)
            return self._model._flat
        if self.P is None:
            raise _lib.Ta3nError("Scorer has no parameters: load_params(), Scorer.from_model() or Scorer.from_engine()")
        return self.P

    def region(self, name: str, shape=None, dtype=torch.float32) -> torch.Tensor:
        off, n = self.plan.region(name)
        t = self.ws[off:off + n]
        if dtype != torch.float32:
            t = t.view(dtype)
        return t.view(*shape) if shape is not None else t

    def _score_chunk(self, n: int, reset: bool) -> None:
        P = self._params()
        with torch.cuda.device(self.device):
            _lib.check(self._L.ta3n_score(self.plan.handle, self.X.data_ptr(), P.data_ptr(), self.ws.data_ptr(), int(n), int(bool(reset)),
                                          self._stream()), "ta3n_score")
            if n > 0:
                self._kept.append((n, self.ws[self._kept_span[0]:self._kept_span[1]].clone()))

    # ---- scoring ----
    def score(self, data: torch.Tensor, labels: torch.Tensor, reset: bool = False) -> None:
        """data [n, T, D], labels [n]: any n, in chunks of `capacity`.  Accumulates into results() / per_video(); reset clears both first."""
        if data.dim() != 3 or data.size(1) != self.T or data.size(2) != self.D:
            raise ValueError(f"data must be [n, {self.T}, {self.D}]")
        n = data.size(0)
        lab = torch.as_tensor(labels).reshape(-1).to(device="cpu", dtype=torch.int64)
        if lab.numel() != n:
            raise ValueError(f"{n} videos, {lab.numel()} labels")
        if n and (int(lab.min()) < 0 or int(lab.max()) >= self.C):
            raise ValueError(f"labels must be in [0, {self.C})")
        self._ensure_buffers()
        if reset:
            self._kept = []
        lab = lab.to(torch.int32)
        for first in range(0, max(n, 1), self.capacity):
            m = min(self.capacity, n - first)
            if m > 0:
                self.X[:m * self.T].copy_(data[first:first + m].reshape(-1, self.D), non_blocking=True)
                self._labels[:m].copy_(lab[first:first + m], non_blocking=True)
            self._score_chunk(m, reset and first == 0)

    def score_store(self, store, video_ids: torch.Tensor, reset: bool = False) -> None:
        """The videos `video_ids` of a FeatureStore, gathered on the device in chunks of `capacity`: no host copy of the features."""
        if store.feature_dim != self.D:
            raise ValueError(f"the store holds {store.feature_dim}-wide rows, the scorer takes {self.D}")
        self._ensure_buffers()
        if len(store) and (int(store.labels.min()) < 0 or int(store.labels.max()) >= self.C):      # the store's labels: one min / max per call
            raise ValueError(f"labels must be in [0, {self.C})")
        ids = torch.as_tensor(video_ids).reshape(-1).to(device=self.device, dtype=torch.int32)
        n = ids.numel()
        if reset:
            self._kept = []
        for first in range(0, max(n, 1), self.capacity):
            m = min(self.capacity, n - first)
            if m > 0:
                store.gather(ids[first:first + m], self.T, out=self.X, labels_out=self._labels)
            self._score_chunk(m, reset and first == 0)

    # ---- results ----
    def results(self) -> Dict[str, object]:
        self._ensure_buffers()
        m = self.region("metrics")[:4].tolist()
        n = max(m[3], 1.0)
        conf = self.region("confusion", dtype=torch.int32)[: self.C * self.C].view(self.C, self.C).cpu()
        return dict(loss=m[0] / n, prec1=100.0 * m[1] / n, prec5=100.0 * m[2] / n, n=int(m[3]), confusion=conf)

    def per_video(self) -> Dict[str, Optional[torch.Tensor]]:
        """logits, prob [n, C]; rank, pred int32 [n]; feat_v [n, NB or F]; attn [n, T - 1] (trn-m; None elsewhere) of the videos scored
        since the last reset, in the order they were given.  Every call keeps one copy of its per-video results (capacity rows) on the device
        until the next reset, and this method concatenates them all: a long run without reset holds every result, and calling this after every
        batch costs time quadratic in the number of batches."""
        self._ensure_buffers()
        base = self._kept_span[0]
        width = self.plan.region("V")[1] // self.capacity

        def take(name, cols, dtype=torch.float32):
            off = self.plan.region(name)[0] - base
            parts = [span[off:off + n * cols] for n, span in self._kept] or [torch.zeros(0, dtype=torch.float32, device=self.device)]
            return torch.cat(parts).view(dtype)
        return dict(logits=take("Y", self.C).view(-1, self.C), prob=take("prob", self.C).view(-1, self.C), rank=take("rank", 1, torch.int32),
                    pred=take("pred", 1, torch.int32), feat_v=take("V", width).view(-1, width),
                    attn=take("attn", self.T - 1).view(-1, self.T - 1) if "attn" in self.plan.regions else None)
