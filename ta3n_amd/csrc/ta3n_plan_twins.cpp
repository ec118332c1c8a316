// Plan builder, bf16 twins (TA3N_FLAG_BF16_STORE): the twin regions, which launches read twins, which producers store them.
#include "ta3n_plan_builder.h"

#include <cstdlib>

namespace ta3n {
namespace {

// what a task covers in the workspace: its output, its fan-out copies and their masks, its epilogue operands
Span out_span(const Task &t) { return span_of(t.c_off, t.m_valid, t.c_ld, t.n_valid); }
Span fan_out_span(const Task &t, int f) { return span_of(t.fan_out_off[f], t.m_valid, t.fan_ld, t.n_valid); }
Span fan_mask_span(const Task &t, int f) { return span_of(t.fan_mask_off[f], t.m_valid, t.fan_ld, t.n_valid); }
Span aux_span(const Task &t) { return span_of(t.aux_off, t.m_valid, t.aux_ld, t.n_valid); }
Span add_span(const Task &t) { return span_of(t.add_off, t.m_valid, t.add_ld, t.n_valid); }
// one side (0: A, 1: B) of a Seg, rows = the operand's readable rows
Span operand_span(const Seg &sg, int side, int rows) {
    const int off = side ? sg.b_off : sg.a_off, ld = side ? sg.b_ld : sg.a_ld;
    return (side ? sg.b_kmajor : sg.a_kmajor) ? span_of(off, sg.klen, ld, rows) : span_of(off, rows, ld, sg.klen);
}
int a_rows_of(const Seg &sg, const Task &t) { return sg.pad[0] > 0 ? sg.pad[0] : t.m_valid; }

// Two launch sequences share the workspace and its twin regions: the FUSED step (groups 4 / 5) and - round 6 - the UNFUSED lists
// (groups 0 / 2: ta3n_forward / ta3n_backward, what the DA options with a loss term between forward and backward run; their GEMM launches
// were twice as long on fp32 stages rounded in registers as the fused step's on twins).  Each family is analysed on its own: who keeps a
// twin up to date, which launch may read twins, which producers store them.  (TA3N_FLAG_MCD: the second pass runs on a second workspace -
// its caller copies the parameter / input twins over from the first before it, TrainEngine.mcd_second_forward.)
bool fused_family(int group) { return group == 4 || group == 5; }
bool unfused_family(int group) { return group == 0 || group == 2; }
bool gemm_of(const Phase &ph, bool (*in_family)(int)) { return in_family(ph.group) && ph.kind == PH_GEMM; }

// the Seg's side can be read from its twin: 16-byte pieces, and (workspace) a producer that keeps the twin current
bool side_ok(const Seg &sg, int side, int rows, const std::vector<Span> &produced, std::vector<Span> &reads) {
    const int base = side ? sg.b_base : sg.a_base, off = side ? sg.b_off : sg.a_off, ld = side ? sg.b_ld : sg.a_ld;
    const int kmajor = side ? sg.b_kmajor : sg.a_kmajor;
    if (base == BASE_G) return false;
    if (((off | ld) & 7) != 0) return false;
    if ((kmajor ? rows : sg.klen) & 7) return false;      // the 16-byte pieces run along rows (k-major) or k
    if (base == BASE_WS) {
        const Span rd = operand_span(sg, side, rows);
        bool covered = false;
        for (auto &pr : produced) covered = covered || overlaps(rd, pr);
        if (!covered) return false;
        reads.push_back(rd);
    }
    return true;
}

void twin(const Geom &g, int32_t &base, int32_t &off) {
    if (base == BASE_P) { base = BASE_P16; off = off / 2; return; }      // relative to the twin region the launch is handed
    const int32_t origin = base == BASE_WS ? g.o_ws16 : g.o_x16;
    off = origin + off / 2;
    base = BASE_WS;
}

void analyse(ta3n_plan &p, const Geom &g, bool (*in_family)(int), const std::vector<Span> &extra) {
    // who keeps a twin up to date: GEMM tiles of the family (their C and their fan-out copies) and - fused step - the heads
    // kernel for gHf.  A launch may read twins only of such data (plus parameters and the input).
    std::vector<Span> produced;   // (Span = [first, last) in ws floats)
    for (auto &sp : extra) produced.push_back(sp);
    for (const Phase &ph : p.phases) {
        if (!gemm_of(ph, in_family)) continue;
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
            const Task &t = p.tasks[i];
            if (t.seg_count == 0) continue;
            if (t.c_base == BASE_WS) produced.push_back(out_span(t));
            for (int f = 0; f < t.fan_count; ++f) produced.push_back(fan_out_span(t, f));
        }
    }
    std::vector<Span> read16;   // ws spans some twin-reading Seg covers
    for (Phase &ph : p.phases) {
        if (!gemm_of(ph, in_family)) continue;
        bool ok = true;
        std::vector<Span> reads;
        std::vector<char> seen(p.segs.size(), 0);
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count && ok; ++i) {
            const Task &t = p.tasks[i];
            for (int k = t.seg_begin; k < t.seg_begin + t.seg_count && ok; ++k) {
                if (seen[k]) continue;
                seen[k] = 1;
                const Seg &sg = p.segs[k];
                ok = side_ok(sg, 0, a_rows_of(sg, t), produced, reads) && side_ok(sg, 1, t.n_valid, produced, reads);
            }
        }
        if (!ok) continue;
        ph.bf16 |= 16;
        read16.insert(read16.end(), reads.begin(), reads.end());
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
            const Task &t = p.tasks[i];
            for (int k = t.seg_begin; k < t.seg_begin + t.seg_count; ++k) {
                if (seen[k]) continue;
                seen[k] = 1;
                twin(g, p.segs[k].a_base, p.segs[k].a_off);
                twin(g, p.segs[k].b_base, p.segs[k].b_off);
            }
        }
    }
    // producers whose output some twin-reading Seg covers store the twin as well
    auto read_as_twin = [&](const Span &out) {
        for (auto &rd : read16)
            if (overlaps(out, rd)) return true;
        return false;
    };
    for (const Phase &ph : p.phases) {
        if (!gemm_of(ph, in_family)) continue;
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
            Task &t = p.tasks[i];
            if (t.seg_count == 0) continue;
            if (t.c_base == BASE_WS && read_as_twin(out_span(t))) t.epi |= EPI_TWIN16;
            for (int f = 0; f < t.fan_count; ++f)
                if (read_as_twin(fan_out_span(t, f))) t.epi |= EPI_TWIN16_FAN;
        }
    }
}

// some launch of the fused step reads reg in fp32: a launch that does not read twins through a Seg, any launch through its
// epilogue operands (masks / residuals are read in fp32 by twin launches too)
bool has_fp32_reader(const ta3n_plan &p, const Span &reg) {
    for (const Phase &ph : p.phases) {
        if (!gemm_of(ph, fused_family)) continue;
        const bool reads_twins = (ph.bf16 & 16) != 0;
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
            const Task &t = p.tasks[i];
            if (!reads_twins)
                for (int k = t.seg_begin; k < t.seg_begin + t.seg_count; ++k) {
                    const Seg &sg = p.segs[k];
                    if (sg.a_base == BASE_WS && overlaps(operand_span(sg, 0, a_rows_of(sg, t)), reg)) return true;
                    if (sg.b_base == BASE_WS && overlaps(operand_span(sg, 1, t.n_valid), reg)) return true;
                }
            if (t.seg_count == 0) continue;
            if ((t.epi & EPI_MASK) && t.aux_base == BASE_WS && overlaps(aux_span(t), reg)) return true;
            if ((t.epi & EPI_ADD) && t.add_base == BASE_WS && overlaps(add_span(t), reg)) return true;
            if (reads_twins)
                for (int f = 0; f < t.fan_count; ++f)
                    if (overlaps(fan_mask_span(t, f), reg)) return true;
        }
    }
    return false;
}

}  // namespace

void add_bf16_twins(ta3n_plan &p, Builder &b, Geom &g, int BT, int D, const std::vector<Span> &extra_produced,
                    const std::vector<Span> &gemm_only, const std::vector<Span> &unfused_produced) {
    const ta3n_config &c = p.cfg;
    if (!stored_twins(c)) return;
    // bf16 twins.  A launch of the fused step reads twins when every one of its operands can be moved 16 bytes (8
    // elements) at a time and has a producer that keeps the twin current; its Segs are then re-addressed into the
    // twin regions.  Launches with odd-shaped operands (the small head weight gradients) keep rounding fp32
    // operands in registers.
    g.ws16_span = (int32_t)p.ws_floats;
    p.ws_floats_before_twins = p.ws_floats;
    g.o_ws16 = (int32_t)b.add_region("ws16", (p.ws_floats + 1) / 2);
    g.o_p16 = (int32_t)b.add_region("p16", (p.param_floats + 1) / 2);
    g.o_x16 = (int32_t)b.add_region("x16", ((int64_t)BT * D + 1) / 2);
    g.o_p16b = (int32_t)b.add_region("p16b", (p.param_floats + 1) / 2);      // (fused-update step: twins of the second parameter buffer)
    if (c.flags & TA3N_FLAG_F32_SPLIT) {
        // the lo planes: the same four regions again, so ONE displacement leads from any twin element to its lo half
        const int32_t lo_ws = (int32_t)b.add_region("ws16_lo", (p.ws_floats_before_twins + 1) / 2);
        const int32_t lo_p = (int32_t)b.add_region("p16_lo", (p.param_floats + 1) / 2);
        const int32_t lo_x = (int32_t)b.add_region("x16_lo", ((int64_t)BT * D + 1) / 2);
        const int32_t lo_pb = (int32_t)b.add_region("p16b_lo", (p.param_floats + 1) / 2);
        g.pair_delta = lo_ws - g.o_ws16;
        if (lo_p - g.o_p16 != g.pair_delta || lo_x - g.o_x16 != g.pair_delta || lo_pb - g.o_p16b != g.pair_delta || (g.pair_delta & 3))
            g.pair_delta = -1;      // (cannot happen: equal sizes, 64-float alignment; build_plan reports it)
    }
    analyse(p, g, fused_family, extra_produced);
    const char *ue = std::getenv("TA3N_UNFUSED_TWINS");      // (=0: the unfused lists on fp32 stages rounded in registers, as before round 6 - A/B aid)
    if (!(ue && std::atoi(ue) == 0)) analyse(p, g, unfused_family, unfused_produced);
    // gemm_only: workspace regions that only GEMM launches read (no pointwise kernel, no API output).  If every launch
    // that reads such a region reads its twin, the producers skip the fp32 store (EPI_TWIN_ONLY): the fp32 region then
    // holds nothing meaningful in this configuration.
    for (const Span &reg : gemm_only) {
        if (has_fp32_reader(p, reg)) continue;
        for (const Phase &ph : p.phases) {
            if (!gemm_of(ph, fused_family)) continue;
            for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
                Task &t = p.tasks[i];
                if (t.seg_count == 0) continue;
                if ((t.epi & EPI_TWIN16) && t.c_base == BASE_WS && overlaps(out_span(t), reg)) t.epi |= EPI_TWIN_ONLY;
                if (t.epi & EPI_TWIN16_FAN) {
                    bool all_in = t.fan_count > 0;
                    for (int f = 0; f < t.fan_count; ++f) all_in = all_in && overlaps(fan_out_span(t, f), reg);
                    if (all_in) t.epi |= EPI_TWIN_ONLY_FAN;
                }
            }
        }
    }
}

}  // namespace ta3n
