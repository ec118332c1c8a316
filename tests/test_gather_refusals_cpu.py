"""The refusals of every exported ta3n_gather_segments* function - status and exact ta3n_last_error() text, one at a time and two at once
(which message wins) - against tests/golden/gather_refusals.json, recorded by tests/golden/make_gather_refusals.py before the entry
points' checks were merged into one routine and never on the code under test.  No GPU: the buffers are host memory the checks only
compare, and every row asks for no videos, so a row that passed every check by mistake would return TA3N_OK without a launch and fail
the comparison here."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gather_refusals as mg  # noqa: E402

with open(mg.JSON_PATH) as _f:
    GOLDEN = json.load(_f)


def test_table_covers_every_entry_point_and_condition():
    rows = GOLDEN["gather"]
    assert [(fn, case) for fn, case, _, _ in rows] == [(fn, case) for fn in mg.ENTRIES for case in mg.cases(fn)]
    for fn, (into, bf16, sampled) in mg.ENTRIES.items():
        mine = [(case, rc, text) for f, case, rc, text in rows if f == fn]
        texts = {text for _, rc, text in mine if rc != 0}
        assert all(rc == -1 for _, rc, _ in mine if rc != 0) and (({}, 0, None) in mine)
        want = {"null argument", "labels_out needs labels", "videos outside the batch" if into else "bad sizes"}
        if sampled:
            want.add("sampler must be TA3N_SAMPLER_TEST, _VAL or _TRAIN")
        if into or bf16:
            want.add(f"feature_dim % {8 if bf16 else 4} and 16-byte alignment required")
        else:
            want.add("buffers must be 16-byte aligned")
        if into and bf16:
            want.add("a plan without bf16 twins needs the fp32 input rows (x)")
        assert texts == want, fn
        n_edits = lambda case: sum(len(v) if isinstance(v, list) else 1 for v in case.values())
        assert any(n_edits(case) > 1 and rc != 0 for case, rc, _ in mine)      # two at once
        assert all(case.get("n_videos", 0) <= 0 for case, _, _ in mine)
    assert [(e, v) for e, v, _, _ in GOLDEN["feeds"]] == [(e, v) for e in mg.FEED_ENTRIES for v in mg.FEED_CASES]
    assert all(rc == -1 and text.startswith("ta3n_feed: ") for _, _, rc, text in GOLDEN["feeds"])


@pytest.mark.parametrize("fn", list(mg.ENTRIES))
def test_every_refusal_keeps_its_status_and_text(fn):
    for f, case, rc, text in GOLDEN["gather"]:
        if f == fn:
            assert mg.ask(fn, case) == (rc, text), (fn, case)
