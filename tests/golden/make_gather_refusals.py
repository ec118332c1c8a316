"""What the batch-assembly entry points refuse, with which status and which ta3n_last_error() text: every exported
ta3n_gather_segments* function (seven: ENTRIES) for a fixed table of (entry point, violated conditions), and the ta3n_feed checks of ta3n_train_steps /
ta3n_train_steps_adam.

    python tests/golden/make_gather_refusals.py        # writes tests/golden/gather_refusals.json

Run it on the commit whose behaviour is the REFERENCE (the parent of a restructuring of these checks), never on the code under test:
the JSON is the evidence; tests/test_gather_refusals_cpu.py asks every row of "gather" again and compares for equality, and
tests/test_gpu_gather_widths.py does the same for "feeds".  Deterministic: no commit, date, path or address enters the file.

"gather" needs no device.  Every pointer is real host memory (a numpy array, each buffer 16-byte aligned or deliberately 4 bytes off)
that the host code compares and never dereferences, and every row asks for n_videos = 0 (or -1): a row that wrongly passed every check
would end at the launcher's early return with TA3N_OK and no launch.  The _into rows use plans of ta3n_plan_create (host only).
A row is [entry point, case, status, text (null where status is 0)]; a case names what differs from an accepted call:
  "null": pointers passed as NULL, "off4": pointers moved 4 bytes off their alignment, "plan": the plan of an _into call (PLANS),
  and the integer arguments n_videos, num_segments, feature_dim, first_video, sampler by name.

"feeds" is reachable only behind the plan's upload, so it is recorded where a device is present (and kept as it stands where none is):
[entry point, violation of the source feed (FEED_CASES), status, text]."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ta3n_amd import _lib  # noqa: E402

JSON_PATH = os.path.join(HERE, "gather_refusals.json")
TINY = (6, 4, 5, 64, 32, 7)      # Bs, Bt, T, D, fc_dim, C
FLAGS = _lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN
TWINS = _lib.FLAG_BF16_MFMA | _lib.FLAG_BF16_STORE
# name -> (feature_dim, flags): TINY with and without bf16 twins of the input, and the widths the % 4 / % 8 rules refuse
PLANS = {"f32": (64, FLAGS), "bf16": (64, FLAGS | TWINS), "f32_d6": (6, FLAGS), "f32_d12": (12, FLAGS), "bf16_d12": (12, FLAGS | TWINS)}

# entry point -> (into a plan, bf16 store, takes a sampler key)
ENTRIES = {
    "ta3n_gather_segments": (False, False, False),
    "ta3n_gather_segments_sampled": (False, False, True),
    "ta3n_gather_segments_bf16": (False, True, True),
    "ta3n_gather_segments_into": (True, False, False),
    "ta3n_gather_segments_sampled_into": (True, False, True),
    "ta3n_gather_segments_bf16_into": (True, True, False),
    "ta3n_gather_segments_bf16_sampled_into": (True, True, True),
}
assert sorted(ENTRIES) == sorted(s for s in _lib.SYMBOLS if s.startswith("ta3n_gather_segments"))

_POINTERS = ("store", "first_row", "num_frames", "labels", "video_ids", "out", "x", "ws", "labels_out", "segment_ids_out")
_ARENA = np.zeros(64 * len(_POINTERS) + 16, dtype=np.uint8)
_BASE = (_ARENA.ctypes.data + 15) & ~15
_PLAN_CACHE = {}


def plan(name):
    if name not in _PLAN_CACHE:
        D, flags = PLANS[name]
        _PLAN_CACHE[name] = _lib.Plan(*TINY[:3], D, *TINY[4:], flags)
    return _PLAN_CACHE[name]


def cases(fn):
    """The cases of one entry point, in a fixed order."""
    into, bf16, sampled = ENTRIES[fn]
    checked = ["store", "first_row", "num_frames", "video_ids"] + ((["ws"] if bf16 else ["x", "ws"]) if into else ["out"])
    aligned = ["store"] + (["x", "ws"] if into else ["out"])
    out = [{}]
    out += [{"null": ["plan"]}] if into else []
    out += [{"null": [p]} for p in checked]
    out += [{"null": ["labels"]}, {"null": ["labels", "labels_out"]}, {"null": ["labels_out"]}, {"n_videos": -1}]
    if into:
        out += [{"first_video": -1}, {"first_video": TINY[0] + TINY[1]}, {"first_video": TINY[0] + TINY[1] + 1},
                {"plan": "bf16_d12" if bf16 else "f32_d6"}, {"plan": "f32_d12"}]
    else:
        out += [{"null": ["segment_ids_out"]}, {"num_segments": 0}, {"num_segments": -1}, {"feature_dim": 0}, {"feature_dim": -4},
                {"feature_dim": 12}, {"feature_dim": 6}, {"feature_dim": 6, "off4": aligned}]
    if sampled:
        out += [{"sampler": -1}, {"sampler": 3}, {"sampler": 1}, {"sampler": 2}]
    out += [{"off4": [p]} for p in aligned]
    if into and bf16:      # x may be null where the plan keeps bf16 twins of the input
        out += [{"null": ["x"]}, {"null": ["x"], "plan": "f32"}, {"plan": "f32"}]
    # two conditions at once: which message wins
    out += [{"null": ["store", "labels"]}, {"null": ["labels"], "n_videos": -1}, {"n_videos": -1, "off4": ["store"]}]
    if sampled:
        out += [{"n_videos": -1, "sampler": 3}, {"sampler": 3, "off4": ["store"]}]
    if into:
        out += [{"first_video": -1, "off4": ["ws"]}, {"null": ["plan", "store"]}]
    else:
        out += [{"num_segments": 0, "feature_dim": 6}, {"feature_dim": 0, "off4": ["out"]}]
    if into and bf16:
        out += [{"null": ["x"], "plan": "f32", "off4": ["ws"]}, {"null": ["x"], "plan": "f32_d12"}]
    return out


def ask(fn, case):
    """(status, ta3n_last_error() text or None) of one call."""
    into, bf16, sampled = ENTRIES[fn]
    L = _lib.lib()

    def ptr(name):
        if name in case.get("null", ()):
            return None
        return C.c_void_p(_BASE + 64 * _POINTERS.index(name) + (4 if name in case.get("off4", ()) else 0))
    n = case.get("n_videos", 0)
    assert n <= 0
    head = [ptr(p) for p in ("store", "first_row", "num_frames", "labels", "video_ids")]
    if into:
        p = plan(case.get("plan", "bf16" if bf16 else "f32"))
        args = [None if "plan" in case.get("null", ()) else p.handle] + head + [n, case.get("first_video", 0), ptr("x"), ptr("ws"),
                                                                               ptr("labels_out"), None]
    else:
        args = head + [n, case.get("num_segments", TINY[2]), case.get("feature_dim", TINY[3]), ptr("out"), ptr("labels_out"),
                       ptr("segment_ids_out"), None]
    if sampled:
        args += [case.get("sampler", 0), 7, 3]
    else:
        assert "sampler" not in case
    rc = getattr(L, fn)(*args)
    return rc, (L.ta3n_last_error().decode() if rc != 0 else None)


# ---- the ta3n_feed checks (device needed: they sit behind the plan's upload) ----
FEED_ENTRIES = ("ta3n_train_steps", "ta3n_train_steps_adam")
FEED_CASES = ("ids_per_step", "first_row", "labels", "sampler")      # ids_per_step > Bs, null first_row, no labels, sampler 3


def ask_feed(eng, stores, tables, entry, violation):
    """One n_steps = 1 call of `entry` on the engine's buffers with both feeds, the SOURCE feed carrying `violation` (None: none).
    stores / tables: (source, target) FeatureStores and int32 device id tables [1, n].  Returns (status, text or None)."""
    import torch
    feeds = []
    for st, ids in zip(stores, tables):
        f = _lib.Feed()
        f.store, f.bf16, f.ids_per_step = st.store.data_ptr(), int(st.bf16), ids.shape[1]
        f.first_row, f.num_frames, f.labels, f.video_ids = st.first_row.data_ptr(), st.num_frames.data_ptr(), st.labels.data_ptr(), ids.data_ptr()
        feeds.append(f)
    src = feeds[0]
    if violation == "ids_per_step":
        src.ids_per_step = eng.Bs + 1
    elif violation == "first_row":
        src.first_row = None
    elif violation == "labels":
        src.labels = None
    elif violation == "sampler":
        src.sampler = 3
    else:
        assert violation is None
    hy = eng.hyper_array([([0.75, 0.75, 0.5], 0.003, 2e-3)], 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    if entry == "ta3n_train_steps":
        rc = L.ta3n_train_steps(eng.plan.handle, p(eng.X), p(eng.P), p(eng.G), p(eng.M), p(eng.ws), 0, 2e-3, 0.9, 1e-4, 20.0, hy, 1,
                                C.byref(feeds[0]), C.byref(feeds[1]), None, None, stream)
    else:
        rc = L.ta3n_train_steps_adam(eng.plan.handle, p(eng.X), p(eng.P), p(eng.G), p(eng.M), p(eng.V), p(eng.ws), 0, 2e-3, 0.9, 0.999, 1e-8,
                                     1e-4, 20.0, 1, hy, 1, C.byref(feeds[0]), C.byref(feeds[1]), stream)
    return rc, (L.ta3n_last_error().decode() if rc != 0 else None)


def record_feeds():
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    import gather_cases as gc
    from ta3n_amd.engine import TrainEngine
    rows = []
    for entry in FEED_ENTRIES:
        eng = TrainEngine(*TINY, dropout_i=0.5, dropout_v=0.5, f32_split=True, bf16_store=True,
                          optimizer="Adam" if entry.endswith("adam") else "SGD")
        case = gc.case(TINY[2], TINY[3], seed=1, train=True)
        stores = (case.store(), case.store())
        tables = tuple(gc.id_table(len(case), 1, n, seed=11 + i).cuda() for i, n in enumerate(TINY[:2]))
        for violation in FEED_CASES:
            rows.append([entry, violation, *ask_feed(eng, stores, tables, entry, violation)])
        torch.cuda.synchronize()
    return rows


def record():
    import torch
    rec = {"gather": [[fn, case, *ask(fn, case)] for fn in ENTRIES for case in cases(fn)]}
    if torch.cuda.is_available():
        rec["feeds"] = record_feeds()
    else:
        try:
            with open(JSON_PATH) as f:
                rec["feeds"] = json.load(f)["feeds"]
        except OSError:
            rec["feeds"] = []
    return rec


def dumps(rec):
    """One line per row."""
    return "{" + ",\n".join('"%s": [\n%s]' % (k, ",\n".join(json.dumps(r) for r in rec[k])) for k in ("gather", "feeds")) + "}\n"


def main():
    rec = record()
    with open(JSON_PATH, "w") as f:
        f.write(dumps(rec))
    print("wrote", JSON_PATH, len(rec["gather"]), "gather rows,", len(rec["feeds"]), "feed rows")


if __name__ == "__main__":
    main()
