"""The shard split of the sharded optimiser step (include/ta3n_hip.h: ta3n_shard_ranges) at any world size; no device is touched.

Every rank owns one chunk of region A (the shared frame FC, padded to a multiple of 4 world) and one of region B (the rest of the live
prefix): the own ranges of all ranks must be 4-float aligned, disjoint, and cover [0, live) exactly - a float outside every range is never
updated, one inside two is updated twice.  The GPU side (every rank's kernels played by one process): test_gpu_sgd_update.py."""
import ctypes as C

import pytest

import sgd_update_cases as sc
from ta3n_amd import _lib

ALL_FLAGS = (_lib.FLAG_ADV_RELATION | _lib.FLAG_ADV_VIDEO | _lib.FLAG_ADV_FRAME | _lib.FLAG_ATTN_ENTROPY | _lib.FLAG_TRANS_ATTN)
WORLDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 64]
TOO_SHORT = "the flat buffers are too short to shard over this many ranks"

_PLANS = {}


def _plan(shape):
    if shape not in _PLANS:
        _PLANS[shape] = _lib.Plan(*sc.SHAPES[shape], ALL_FLAGS)
    return _PLANS[shape]


def _ranges(plan, rank, world):
    own, lay = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    _lib.check(_lib.lib().ta3n_shard_ranges(plan.handle, rank, world, own, lay), "ta3n_shard_ranges")
    return list(own), list(lay)


def test_engine_flags_are_the_full_ta3n_configuration():
    from ta3n_amd.engine import ALL_FLAGS as engine_flags
    assert engine_flags == ALL_FLAGS


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape", ["small", "odd", "headline"])
def test_own_ranges_tile_the_live_prefix(shape, world):
    plan = _plan(shape)
    live, first = plan.live_floats, sc.n_first(plan)
    assert 0 < first < live and live % 4 == 0
    _, (a_chunk, a_end, b_chunk, b_end) = _ranges(plan, 0, world)
    q = 4 * world
    assert a_end % q == 0 and first <= a_end < first + q           # the first multiple of 4 world at or past n_first
    assert a_chunk * world == a_end and a_chunk % 4 == 0
    assert b_chunk % 4 == 0 and b_end == a_end + b_chunk * world
    assert live <= b_end < live + q and b_end <= plan.param_floats   # B's padding stays below one chunk quantum and inside the buffers
    assert (a_chunk, a_end, b_chunk, b_end) == sc.shard_layout(live, first, world)
    pieces = []
    for rank in range(world):
        own, lay = _ranges(plan, rank, world)
        assert lay == [a_chunk, a_end, b_chunk, b_end]
        assert own == sc.shard_own(live, first, world, rank)
        assert all(v % 4 == 0 and 0 <= v <= live for v in own)
        assert own[0] <= own[1] <= min(a_end, live) <= own[2] <= own[3]
        pieces += [(own[0], own[1]), (own[2], own[3])]
    pieces = sorted(p for p in pieces if p[1] > p[0])
    assert pieces[0][0] == 0 and pieces[-1][1] == live
    for (_, hi), (lo, _) in zip(pieces, pieces[1:]):
        assert hi == lo                                              # no gap, no overlap
    assert sum(hi - lo for lo, hi in pieces) == live


def test_the_last_rank_of_a_padded_region_b_owns_less_than_a_chunk():
    """The clamp of a_end + b_chunk (rank + 1) to the live prefix: region B's padding comes off the last rank's range."""
    plan = _plan("odd")
    live = plan.live_floats
    own, (a_chunk, a_end, b_chunk, b_end) = _ranges(plan, 63, 64)
    assert b_end > live and own[3] == live and own[3] - own[2] == b_chunk - (b_end - live) and own[1] - own[0] == a_chunk


def test_a_split_past_the_flat_buffers_is_refused():
    """a_end may pass n_first, and b_end the live prefix, by up to 4 world - 4 floats each; a split that ends behind the flat buffers must
    be refused.  Searched, not assumed: every plan with a pipelined step carries at least the source-only heads behind its live prefix (tens
    of thousands of floats), so no world up to the 256 slots of ws["norm_part"] gets there - only a world in the ten thousands does."""
    L = _lib.lib()
    found = []
    for shape in ("odd", "small", (2, 2, 3, 64, 8, 3)):
        plan = _plan(shape) if isinstance(shape, str) else _lib.Plan(*shape, ALL_FLAGS)
        assert L.ta3n_has_pipelined_step(plan.handle) == 1
        live, first = plan.live_floats, sc.n_first(plan)
        for world in list(range(1, 257)) + [1 << k for k in range(9, 22)]:
            want_refused = sc.shard_layout(live, first, world)[3] > plan.param_floats
            own, lay = (C.c_int64 * 4)(), (C.c_int64 * 4)()
            rc = L.ta3n_shard_ranges(plan.handle, 0, world, own, lay)
            assert (rc != 0) == want_refused, (shape, world)
            if rc != 0:
                assert rc == -1 and L.ta3n_last_error().decode() == TOO_SHORT and world > 256
                found.append((shape, world))
    assert found, "no searched plan ends close enough behind its live prefix"
    with pytest.raises(ValueError, match=TOO_SHORT):
        _ranges(_plan(found[0][0]), 0, found[0][1])


def test_bad_ranks_and_worlds_are_refused():
    plan = _plan("small")
    with pytest.raises(ValueError, match="rank outside the group"):
        _ranges(plan, 3, 3)
    with pytest.raises(ValueError, match="rank outside the group"):
        _ranges(plan, -1, 3)
    with pytest.raises(ValueError, match="bad shard arguments"):
        _ranges(plan, 0, 0)
    # more ranks than slots of ws["norm_part"]: refused before the plan is uploaded to a device (the dummy buffers are never read)
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    slots = plan.region("norm_part")[1]
    assert slots == 256
    rc = L.ta3n_shard_sumsq(plan.handle, C.addressof(dummy), C.addressof(dummy), 0, slots + 1, None)
    assert rc == -1 and L.ta3n_last_error().decode() == "rank outside the group"
