"""Fingerprints of the plans the host-side plan builder produces (ta3n_amd/csrc/ta3n_plan*.cpp), for a fixed matrix of
configurations: what "the plan did not change by a byte" means for a restructuring of the builder.

    python tests/golden/make_plan_fingerprints.py        # writes tests/golden/plan_fingerprints.json

Run it on the commit whose plans are the REFERENCE (the parent of a builder refactor), never on the code under test: the JSON is the
evidence, tests/test_plan_fingerprints_cpu.py rebuilds every plan and compares.  Host-only: no GPU is touched.

Per configuration, a SHA-256 over, in this order: the raw bytes of the Seg, Task and Phase arrays and of Geom (ta3n_debug_arrays;
every field is 32 bits wide, so there is no padding), the wait list (ta3n_debug_waits), the tuple table and tuple_first, every
ta3n_param_info row, ta3n_param_floats / ta3n_live_param_floats / ta3n_workspace_floats, the ta3n_plan_describe string (every
region's name, offset and size; every phase), ta3n_num_phases of the five groups and the three ta3n_has_* answers.  A configuration
the builder refuses is recorded as [return code, exact ta3n_last_error() text] instead.  The configurations themselves are not in
the JSON: matrix() below is their definition, the JSON maps its names to the fingerprints.

The builder reads TA3N_THIRD_STAGE (once per process), TA3N_UNFUSED_TWINS and TA3N_HEADS_VPW from the environment: clean_env()
removes them and must run before the first plan of the process is created.
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

JSON_PATH = os.path.join(HERE, "plan_fingerprints.json")
ENV_KNOBS = ("TA3N_THIRD_STAGE", "TA3N_UNFUSED_TWINS", "TA3N_HEADS_VPW")

REL, VID, FRM, ENT, ATT, MCD, FG, BN = (1 << i for i in range(8))
BF16, STORE, SPLIT = 1 << 8, 1 << 9, 1 << 10
ADV = REL | VID | FRM
ALL = ADV | ENT | ATT
ARITH = {"f32": 0, "bf16": BF16, "twins": BF16 | STORE, "split": SPLIT, "pair": SPLIT | STORE}
MAIN = ("f32", "twins", "pair")      # the arithmetics the wider sweeps use ("bf16" and "split" ride on the headline shape)
TRN, AVG = 0, 1

# (Bs, Bt, T, D, fc_dim, C, NB)
HEAD = dict(Bs=128, Bt=74, T=5, D=2048, F=512, C=12, NB=256)       # the headline shape
BIG = dict(Bs=512, Bt=512, T=9, D=2048, F=512, C=30, NB=256)       # 512+512 x 9
TWO = dict(Bs=128, Bt=128, T=12, D=1024, F=512, C=12, NB=256)      # 128+128 x 12
MID = dict(Bs=6, Bt=5, T=5, D=64, F=32, C=8, NB=256)               # small, with a fused step
TINY = dict(Bs=3, Bt=2, T=3, D=40, F=16, C=5, NB=64)               # heads_supported says no: no fused step
ODD = dict(Bs=5, Bt=4, T=4, D=52, F=20, C=6, NB=256)               # D no multiple of 8, C no multiple of 4
CH = dict(Bs=40, Bt=24, T=5, D=256, F=128, C=12, NB=256)           # several tiles per launch, small enough for many chained plans
SHAPES = {"head": HEAD, "big": BIG, "two": TWO, "mid": MID, "tiny": TINY, "odd": ODD, "ch": CH}
# (7222, 46221 and 56221 name kernels that only the experiments build has: the default library refuses them, by text)
TILE_CODES = (0, 114, 118, 222, 3222, 6222, 7222, 10222, 30222, 30221, 36222, 35221, 46221, 56221)


def clean_env():
    for k in ENV_KNOBS:
        os.environ.pop(k, None)


def matrix():
    """name -> configuration (shape keys of SHAPES + flags, agg and the knobs of ta3n_config)."""
    out = {}

    def add(name, shape, flags=0, **knobs):
        assert name not in out, name
        out[name] = dict(shape, flags=flags, **knobs)

    trn_flags = {"none": 0, "rel": REL, "vid": VID, "frm": FRM, "adv": ADV, "all": ALL, "mcd": ADV | MCD, "fg": ADV | FG,
                 "bn": ALL | BN, "bn_only": BN, "att": ATT}
    # ---- trn-m: shapes x arithmetics x flag sets ----
    for sn in ("head", "mid", "tiny", "odd"):
        for an, a in ARITH.items():
            for fn, f in trn_flags.items():
                if sn == "head" or (an in MAIN and fn in ("none", "all", "mcd", "fg", "bn")):
                    add(f"trn/{sn}/{an}/{fn}", SHAPES[sn], f | a)
    for an in MAIN:
        for sn in ("big", "two"):
            add(f"trn/{sn}/{an}/all", SHAPES[sn], ALL | ARITH[an])
        add(f"trn/big/{an}/bn", BIG, ALL | BN | ARITH[an])
        for T in (2, 3, 9, 12):
            add(f"trn/mid_T{T}/{an}/all", dict(MID, T=T), ALL | ARITH[an])
        add(f"trn/tiny_T2/{an}/all", dict(TINY, T=2), ALL | ARITH[an])
        add(f"trn/head_Bt0/{an}/none", dict(HEAD, Bt=0), ARITH[an])
        add(f"trn/head_Bt0/{an}/all", dict(HEAD, Bt=0), ALL | ARITH[an])
        add(f"trn/vpw2/{an}/all", dict(HEAD, Bs=128, Bt=128), ALL | ARITH[an])          # 225 videos or more: two per video workgroup
        add(f"trn/vpw2_edge/{an}/all", dict(MID, Bs=113, Bt=112), ALL | ARITH[an])
        add(f"trn/vpw1_edge/{an}/all", dict(MID, Bs=112, Bt=112), ALL | ARITH[an])
    add("trn/head/store_only/all", HEAD, ALL | STORE)
    # ---- knobs (trn-m, all DA flags).  Chained plans of the headline shape take ~0.4 s each to build (the interval analysis of
    # Builder::end_chain): the sweeps with chain = 1 run on the "ch" shape, a few entries on the large ones ----
    for an, a in ARITH.items():
        for tc in TILE_CODES:
            add(f"tile/head/{an}/{tc}", HEAD, ALL | a, tile_config=tc)
    for an in MAIN:
        a = ARITH[an]
        for tc in TILE_CODES:
            add(f"tile/ch/{an}/{tc}/chain", CH, ALL | a, tile_config=tc, chain=1)
        for tc in (0, 30222):
            add(f"tile/big/{an}/{tc}", BIG, ALL | a, tile_config=tc)
            add(f"tile/two/{an}/{tc}", TWO, ALL | a, tile_config=tc)
        for sk in (2, 4, 6):
            add(f"split_k/head/{an}/{sk}", HEAD, ALL | a, split_k=sk)
            add(f"split_k/ch/{an}/{sk}/chain", CH, ALL | a, split_k=sk, chain=1)
        add(f"split_k/head/{an}/6/bn", HEAD, ALL | BN | a, split_k=6)
        add(f"split_k/head/{an}/6/xcd3", HEAD, ALL | a, split_k=6, xcd_aware=3, cost_model=1)
        for late in (1, 6):
            add(f"late/head/{an}/{late}", HEAD, ALL | a, wgrads_late=late)
            add(f"late/ch/{an}/{late}/chain", CH, ALL | a, wgrads_late=late, chain=1)
            add(f"late/odd/{an}/{late}", ODD, ALL | a, wgrads_late=late)
        add(f"xcd/head/{an}/1", HEAD, ALL | a, xcd_aware=1)
        for x in (2, 3):
            for cm in (0, 1):
                add(f"xcd/head/{an}/{x}/cost{cm}", HEAD, ALL | a, xcd_aware=x, cost_model=cm)
            add(f"xcd/odd/{an}/{x}", ODD, ALL | a, xcd_aware=x)
            add(f"xcd/ch/{an}/{x}/chain", CH, ALL | a, xcd_aware=x, chain=1)
        add(f"xcd/two/{an}/3", TWO, ALL | a, xcd_aware=3)
        add(f"xcd/big/{an}/3", BIG, ALL | a, xcd_aware=3, cost_model=1)
        add(f"cost/head/{an}", HEAD, ALL | a, cost_model=1)
        add(f"chain/ch/{an}/bn", CH, ALL | BN | a, chain=1)                          # (use_bn: no fused step with chain)
        add(f"chain/tiny/{an}", TINY, ALL | a, chain=1)
        add(f"chain/odd/{an}", ODD, ALL | a, chain=1)
        add(f"chain/mid/{an}", MID, ALL | a, chain=1)
        add(f"phase_tiles/head/{an}", HEAD, ALL | a, tile_config=222,
            phase_tiles=[114, 0, 118, 30222, 0, 0, 0, 222, 3222, 0, 6222, 30221, 0, 114, 0, 10222])
        add(f"phase_tiles/ch/{an}/chain", CH, ALL | a, phase_tiles=[30221, 118, 114, 0, 36222, 222], chain=1)
        add(f"phase_tiles/avg/{an}", HEAD, a, agg=AVG, phase_tiles=[30222, 114, 118, 222])
        add(f"add_fc/head/{an}/1/trn", HEAD, ALL | a, shared_fc_layers=1)
        for L in (2, 3):
            add(f"add_fc/head/{an}/{L}/trn", HEAD, ALL | a, shared_fc_layers=L)
            add(f"add_fc/odd/{an}/{L}/trn", ODD, ALL | a, shared_fc_layers=L)
            add(f"add_fc/head/{an}/{L}/avg", HEAD, a, agg=AVG, shared_fc_layers=L)
            add(f"add_fc/head/{an}/{L}/avg_da", HEAD, ADV | a, agg=AVG, shared_fc_layers=L)
            add(f"add_fc/odd/{an}/{L}/avg_da", ODD, ADV | a, agg=AVG, shared_fc_layers=L)
            add(f"add_fc/tiny/{an}/{L}/trn", TINY, ALL | a, shared_fc_layers=L)
            add(f"add_fc/head/{an}/{L}/trn_fg", HEAD, ADV | FG | a, shared_fc_layers=L)
            add(f"add_fc/head/{an}/{L}/tile30222_xcd3", HEAD, ALL | a, shared_fc_layers=L, tile_config=30222, xcd_aware=3, cost_model=1)
    for an in MAIN:      # chained plans at the large shapes: the tile heuristics with a settled chain shape
        add(f"chain/head/{an}", HEAD, ALL | ARITH[an], chain=1)
    add("chain/head/twins/30222", HEAD, ALL | BF16 | STORE, chain=1, tile_config=30222)
    add("chain/head/twins/36222_xcd3", HEAD, ALL | BF16 | STORE, chain=1, tile_config=36222, xcd_aware=3)
    add("chain/two/twins", TWO, ALL | BF16 | STORE, chain=1)
    add("chain/head/twins/bn", HEAD, ALL | BN | BF16 | STORE, chain=1)
    # ---- avgpool: source-only fast path and the general builder through each of its doors ----
    avg_flags = {"src": 0, "frm": FRM, "vid": VID, "rel": REL, "mcd": MCD, "fg": FG, "bn": BN, "adv": ADV,
                 "every": ADV | MCD | FG | BN}
    for sn in ("head", "big", "two", "tiny", "odd"):
        for an, a in ARITH.items():
            for fn, f in avg_flags.items():
                if sn == "head" or (an in MAIN and fn in (("src", "frm", "every") if sn == "odd" else ("src", "every"))):
                    add(f"avg/{sn}/{an}/{fn}", SHAPES[sn], f | a, agg=AVG)
    for an in MAIN:
        add(f"avg/head_Bt0/{an}/src", dict(HEAD, Bt=0), ARITH[an], agg=AVG)
        add(f"avg/head_Bt0/{an}/every", dict(HEAD, Bt=0), ADV | MCD | FG | BN | ARITH[an], agg=AVG)
        for tc in (222, 30222, 35221):
            add(f"avg/head/{an}/src/tile{tc}", HEAD, ARITH[an], agg=AVG, tile_config=tc)
            add(f"avg/head/{an}/every/tile{tc}", HEAD, ADV | MCD | FG | BN | ARITH[an], agg=AVG, tile_config=tc, xcd_aware=3)
        add(f"avg/head/{an}/src/knobs", HEAD, ARITH[an], agg=AVG, chain=1, split_k=6, wgrads_late=1, xcd_aware=2, cost_model=1)
        add(f"avg/head/{an}/adv/knobs", HEAD, ADV | ARITH[an], agg=AVG, chain=1, split_k=6, wgrads_late=1, xcd_aware=2, cost_model=1)
    # ---- refusals ----
    add("refuse/batch_negative", dict(MID, Bs=-1), ALL)
    add("refuse/batch_zero", dict(MID, Bs=0, Bt=0), ALL)
    add("refuse/aggregation", MID, ALL, agg=7)
    add("refuse/T1", dict(MID, T=1), ALL)
    add("refuse/T65", dict(MID, T=65), ALL)
    add("refuse/T1_avg", dict(MID, T=1), 0, agg=AVG)
    add("refuse/D0", dict(MID, D=0), ALL)
    add("refuse/C0", dict(MID, C=0), ALL)
    add("refuse/F0", dict(MID, F=0), ALL)
    add("refuse/NB100", dict(MID, NB=100), ALL)
    add("refuse/NB0", dict(MID, NB=0), ALL)
    add("refuse/NB2048", dict(MID, NB=2048), ALL)
    add("refuse/C65", dict(MID, C=65), ALL)
    add("refuse/entropy_without_video", MID, REL | FRM | ENT)
    add("refuse/entropy_alone_avg", MID, ENT, agg=AVG)
    add("refuse/split_and_bf16", MID, ALL | SPLIT | BF16)
    add("refuse/tile_config_333", MID, ALL, tile_config=333)
    add("refuse/tile_config_40222", MID, ALL | BF16 | STORE, tile_config=40222)
    add("refuse/tile_config_4222", MID, ALL, tile_config=4222)
    add("refuse/phase_tiles_bad", MID, ALL, phase_tiles=[0, 0, 223])
    add("refuse/xcd_negative", MID, ALL, xcd_aware=-1)
    add("refuse/xcd_4", MID, ALL, xcd_aware=4)
    add("refuse/too_large_x", dict(MID, Bs=20000, Bt=0, T=64, D=2048, F=16), ALL)
    add("refuse/too_large_f1", dict(MID, Bs=20000, Bt=20000, T=64, D=1024, F=1024), 0, agg=AVG)
    add("refuse/workspace_too_large", dict(MID, Bs=2048, Bt=2048, T=64, D=2048, F=2048), ALL)
    add("refuse/add_fc_negative", MID, ALL, shared_fc_layers=-1)
    add("refuse/add_fc_4", MID, ALL, shared_fc_layers=4)
    add("refuse/add_fc_4_avg", MID, 0, agg=AVG, shared_fc_layers=4)
    add("refuse/add_fc_bn", MID, ALL | BN, shared_fc_layers=2)
    add("refuse/add_fc_mcd", MID, ADV | MCD, shared_fc_layers=2)
    add("refuse/add_fc_bn_and_mcd", MID, ADV | MCD | BN, shared_fc_layers=3)
    add("refuse/add_fc_chain", MID, ALL, shared_fc_layers=2, chain=1)
    add("refuse/add_fc_split_k", MID, ALL, shared_fc_layers=2, split_k=2)
    add("refuse/add_fc_wgrads_late", MID, ALL, shared_fc_layers=3, wgrads_late=1)
    add("refuse/add_fc_phase_tiles", MID, ALL, shared_fc_layers=2, phase_tiles=[0, 222])
    add("refuse/add_fc_avg_mcd", MID, MCD, agg=AVG, shared_fc_layers=2)
    add("refuse/avg_src_attention", MID, ATT, agg=AVG)
    add("refuse/avg_da_attention", MID, FRM | ATT, agg=AVG)
    add("refuse/avg_da_entropy", MID, ALL, agg=AVG)
    add("refuse/avg_src_F18", dict(MID, F=18), 0, agg=AVG)
    add("refuse/avg_da_F18", dict(MID, F=18), FRM, agg=AVG)
    add("refuse/avg_bn_F18", dict(MID, F=18), BN, agg=AVG)
    add("refuse/trn_bn_F18", dict(MID, F=18), ALL | BN)
    add("refuse/trn_bn_F18_twins", dict(MID, F=18), BN | BF16 | STORE)
    return out


def _config(c):
    from ta3n_amd import _lib
    cfg = _lib.Config(c["Bs"], c["Bt"], c["T"], c["D"], c["F"], c["NB"], c["C"], c["flags"], c.get("tile_config", 0))
    for i, t in enumerate(c.get("phase_tiles", [])):
        cfg.phase_tiles[i] = t
    cfg.xcd_aware = c.get("xcd_aware", 0)
    cfg.aggregation = c.get("agg", TRN)
    cfg.wgrads_late = c.get("wgrads_late", 0)
    cfg.chain = c.get("chain", 0)
    cfg.cost_model = c.get("cost_model", 0)
    cfg.split_k = c.get("split_k", 0)
    cfg.shared_fc_layers = c.get("shared_fc_layers", 0)
    return cfg


def fingerprint(c):
    """SHA-256 (hex) of the plan of configuration c, or [return code, error text] when the builder refuses it."""
    from ta3n_amd import _lib
    import plan_interp as pi
    L = _lib.lib()
    cfg = _config(c)
    h = C.c_void_p()
    rc = L.ta3n_plan_create(C.byref(cfg), C.byref(h))
    if rc != 0:
        return [rc, L.ta3n_last_error().decode()]
    try:
        ptrs = [C.c_void_p() for _ in range(6)]
        ns = [C.c_int64() for _ in range(3)]
        L.ta3n_debug_arrays(h, C.byref(ptrs[0]), C.byref(ns[0]), C.byref(ptrs[1]), C.byref(ns[1]), C.byref(ptrs[2]), C.byref(ns[2]),
                            C.byref(ptrs[3]), C.byref(ptrs[4]), C.byref(ptrs[5]))
        geom = C.cast(ptrs[3], C.POINTER(pi.Geom)).contents
        parts = []

        def raw(name, ptr, nbytes):
            parts.append((name, C.string_at(ptr, nbytes) if nbytes else b""))

        raw("segs", ptrs[0], ns[0].value * C.sizeof(pi.Seg))
        raw("tasks", ptrs[1], ns[1].value * C.sizeof(pi.Task))
        raw("phases", ptrs[2], ns[2].value * C.sizeof(pi.Phase))
        raw("geom", ptrs[3], C.sizeof(pi.Geom))
        w = C.c_void_p(); nw = C.c_int64()
        L.ta3n_debug_waits(h, C.byref(w), C.byref(nw))
        raw("waits", w, nw.value * 8)
        raw("tuples", ptrs[4], geom.n_tuples * geom.T * 4)
        raw("tuple_first", ptrs[5], (geom.n_rel + 1) * 4)
        rows = []
        for i in range(L.ta3n_num_params(h)):
            name = C.c_char_p(); off = C.c_int64(); r = C.c_int32(); cc = C.c_int32(); live = C.c_int32()
            assert L.ta3n_param_info(h, i, C.byref(name), C.byref(off), C.byref(r), C.byref(cc), C.byref(live)) == 0
            rows.append(f"{name.value.decode()} {off.value} {r.value} {cc.value} {live.value}")
        parts.append(("params", "\n".join(rows).encode()))
        parts.append(("floats", f"{L.ta3n_param_floats(h)} {L.ta3n_live_param_floats(h)} {L.ta3n_workspace_floats(h)}".encode()))
        n = L.ta3n_plan_describe(h, None, 0)
        buf = C.create_string_buffer(n + 1)
        L.ta3n_plan_describe(h, buf, n + 1)
        parts.append(("describe", buf.value))
        parts.append(("num_phases", " ".join(str(L.ta3n_num_phases(h, g)) for g in range(5)).encode()))
        parts.append(("has", f"{L.ta3n_has_fused_step(h)} {L.ta3n_has_pipelined_step(h)} {L.ta3n_has_fused_update(h)}".encode()))
        total = hashlib.sha256()
        for name, data in parts:
            total.update(name.encode() + b":" + str(len(data)).encode() + b":")
            total.update(data)
        return total.hexdigest()
    finally:
        L.ta3n_plan_destroy(h)


def main():
    clean_env()
    import subprocess
    import plan_interp as pi
    assert pi.struct_sizes_ok(), "ctypes mirrors out of date with ta3n_types.h"
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "ta3n_amd/csrc", "include"], text=True).strip()
        if dirty:
            commit += " + local changes under ta3n_amd/csrc or include"
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    from ta3n_amd.build import source_hash
    entries = {name: fingerprint(c) for name, c in matrix().items()}
    with open(JSON_PATH, "w") as f:      # one line per configuration
        f.write('{"generated_from": %s,\n"entries": {\n' % json.dumps({"commit": commit, "source_hash": source_hash()}))
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(entries.items())))
        f.write("\n}}\n")
    refused = sum(1 for e in entries.values() if isinstance(e, list))
    print("wrote", JSON_PATH, os.path.getsize(JSON_PATH), "bytes;", len(entries), "entries,", refused, "refused")


if __name__ == "__main__":
    main()
