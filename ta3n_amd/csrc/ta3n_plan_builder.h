// Plan builder internals shared by ta3n_plan.cpp (models), ta3n_plan_tiles.cpp (specs -> tile tasks) and ta3n_plan_twins.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ta3n_plan.h"
#include "ta3n_kernels.h"

namespace ta3n {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct Ref {  // operand reference
    int32_t base, off, ld, kmajor;
};
inline Ref KC(int32_t base, int64_t off, int32_t ld) { return Ref{base, (int32_t)off, ld, 0}; }  // element (r,k) at off + r*ld + k
inline Ref KM(int32_t base, int64_t off, int32_t ld) { return Ref{base, (int32_t)off, ld, 1}; }  // element (r,k) at off + k*ld + r

// a_rows > 0: number of readable rows of the A operand when it exceeds the task's output rows (the [K][4] block of
// ones behind the bias-gradient column sums: four identical rows are multiplied, one is stored)
inline Seg mkseg(Ref a, Ref b, int klen, int scale_kind = SK_ONE, int a_rows = 0) {
    Seg s;
    std::memset(&s, 0, sizeof(s));
    s.pad[0] = a_rows;
    s.a_base = a.base; s.a_off = a.off; s.a_ld = a.ld; s.a_kmajor = a.kmajor;
    s.b_base = b.base; s.b_off = b.off; s.b_ld = b.ld; s.b_kmajor = b.kmajor;
    s.klen = klen;
    s.scale_kind = scale_kind;
    return s;
}

struct GemmSpec {
    int M, N;
    std::vector<Seg> segs;
    Task proto;   // epilogue fields; m0/n0/seg range filled on expansion
    int split = 0;   // 2: two tasks per tile, each over part of the Segs (EPI_SPLITK; the Segs' order is kept: a Seg with a scale stays first)
    int affinity = -1;   // >= 0: specs with the same value read (mostly) the same operand slabs - xcd_aware 3 keeps their tiles on one XCD, back to back
};

inline Task proto(int32_t c_base, int64_t c_off, int32_t c_ld) {
    Task t;
    std::memset(&t, 0, sizeof(t));
    t.c_base = c_base; t.c_off = (int32_t)c_off; t.c_ld = c_ld;
    t.bias_base = BASE_NONE; t.aux_base = BASE_NONE; t.add_base = BASE_NONE;
    t.alpha_kind = SK_ONE; t.gamma_kind = SK_ONE;
    return t;
}
inline void with_bias(Task &t, int64_t off) { t.epi |= EPI_BIAS; t.bias_base = BASE_P; t.bias_off = (int32_t)off; }
inline void with_mask(Task &t, int64_t off, int32_t ld) { t.epi |= EPI_MASK; t.aux_base = BASE_WS; t.aux_off = (int32_t)off; t.aux_ld = ld; }
inline void with_add(Task &t, int64_t off, int32_t ld) { t.epi |= EPI_ADD; t.add_base = BASE_WS; t.add_off = (int32_t)off; t.add_ld = ld; }
// the tiles of the first column block also write the row sums of their own A operand: db beside dW = G^T X (EPI_ROWSUM_A)
inline void with_bias_grad(Task &t, int64_t off) { t.epi |= EPI_ROWSUM_A; t.bias_base = BASE_G; t.bias_off = (int32_t)off; }

// "Twins are on": bf16_twins = plain bf16 twins, what register-blocked tiles and half stages need (tile selection); stored_twins =
// plain or pair twins (TA3N_FLAG_F32_SPLIT | _BF16_STORE: every twin has a hi and a lo plane, x = hi + lo to 16 mantissa bits),
// what the twin layout and the fused step's placement of dWfd go by.
inline bool bf16_twins(const ta3n_config &c) { return (c.flags & TA3N_FLAG_BF16_MFMA) && (c.flags & TA3N_FLAG_BF16_STORE); }
inline bool stored_twins(const ta3n_config &c) { return (c.flags & (TA3N_FLAG_BF16_MFMA | TA3N_FLAG_F32_SPLIT)) && (c.flags & TA3N_FLAG_BF16_STORE); }

typedef std::pair<int64_t, int64_t> Span;   // [first, last) in ws floats
// rows x cols elements at off, row stride ld
inline Span span_of(int64_t off, int rows, int ld, int cols) { return Span{off, off + (int64_t)(rows - 1) * ld + cols}; }
inline bool overlaps(const Span &a, const Span &b) { return a.first < b.second && b.first < a.second; }

// Tile code (ta3n_config.tile_config) of an existing launch's shape.  Two encodings, on purpose: a later level of a chained
// launch repeats the chain's first level (its bf16 digit holds the stages as chosen; blocking as the 0..3 bit pair), the group-5
// launch mirrors the step's first launch including the half-stage offset and the tall tiles' blocking codes.
inline int tile_code_of_chain(const Phase &ph) {
    return ph.wm * 100 + ph.wn * 10 + ph.wk + 1000 * (ph.bf16 & 15) + 10000 * ((ph.rm > 1 ? 1 : 0) + (ph.rn > 1 ? 2 : 0));
}
inline int tile_code_mirroring(const Phase &ph) {
    return ph.wm * 100 + ph.wn * 10 + ph.wk + 1000 * ((ph.bf16 & 15) + ((ph.bf16 & 64) ? 3 : 0)) + 10000 * blk_code(ph.rm, ph.rn);
}

// A "panel" is the set of tiles of one GEMM that share an operand slab: all column tiles of one row tile when the A side (M*K) is
// the larger operand, all row tiles of one column tile otherwise.  Panels are dealt to 8 queues (one per XCD: workgroup b runs on
// XCD b % 8 - a speed assumption only) so the larger operand is partitioned across the private L2s and only the smaller one is replicated.
struct Panel { std::vector<Task> tiles; int64_t cost; int group; };

struct Builder {
    ta3n_plan &p;
    explicit Builder(ta3n_plan &pl) : p(pl) {}

    void add_param(const std::string &name, int rows, int cols, bool live) {
        ParamInfo pi;
        pi.name = name; pi.rows = rows; pi.cols = cols; pi.live = live;
        pi.off = p.param_floats;
        if (!p.layout.empty()) {   // ta3n_config.layout_flags: where the donor plan has it
            const ParamInfo *at = nullptr;
            for (const ParamInfo &d : p.layout) if (d.name == name) at = &d;
            if (!at || at->rows != rows || at->cols != cols) {
                if (p.layout_error.empty()) p.layout_error = "parameter " + name + " does not exist under layout_flags";
            } else {
                if (live && !at->live && p.layout_error.empty()) p.layout_error = "parameter " + name + " is live under flags and not under layout_flags";
                pi.off = at->off;
            }
            p.params.push_back(pi);
            p.param_floats = std::max(p.param_floats, align_up(pi.off + (int64_t)rows * (cols ? cols : 1), 8));
            return;
        }
        p.params.push_back(pi);
        p.param_floats = align_up(p.param_floats + (int64_t)rows * (cols ? cols : 1), 8);   // 8: a bf16 twin row starts 16-byte aligned too
    }
    void add_linear(const std::string &name, int out, int in, bool live) {
        add_param(name + ".weight", out, in, live);
        add_param(name + ".bias", out, 0, live);
    }
    int64_t add_region(const std::string &name, int64_t size) {
        Region r;
        r.name = name; r.off = p.ws_floats; r.size = size;
        p.regions.push_back(r);
        p.ws_floats = align_up(p.ws_floats + size, 64);
        return r.off;
    }

    // a Linear that receives no gradient in this configuration is laid out behind the live prefix (add_dead_linears), in the order it was named
    struct Lin { std::string name; int out, in; };
    std::vector<Lin> dead;
    void lin(const std::string &name, int out, int in, bool live) { if (live) add_linear(name, out, in, true); else dead.push_back(Lin{name, out, in}); }
    void add_dead_linears() { for (auto &d : dead) add_linear(d.name, d.out, d.in, false); }

    int n_split_pairs = 0;      // split-K tile pairs handed out so far (EPI_SPLITK)
    int gemm_phase_index = 0;
    int force_next = 0;         // tile code for the next add_gemm_phase only (a launch that mirrors an earlier one)
    // chained launch under construction (begin_chain .. end_chain): the levels' task lists are concatenated into ONE phase whose tile shape is the first level's
    bool chaining = false;
    int chain_levels = 0;
    Phase chain_ph;
    std::vector<Task> chain_tasks;
    void begin_chain() { chaining = true; chain_levels = 0; chain_tasks.clear(); }
    void chain_append(std::vector<Task> extra) {
        for (auto &t : extra) { t.sig = -1; t.wait_begin = t.wait_count = 0; chain_tasks.push_back(t); }
    }
    std::string end_chain();    // ta3n_plan_tiles.cpp; returns an error message or ""
    bool mixed_kinds = false;   // a GEMM spec whose Segs differ in operand kinds (not supported by the kernel)
    int sum8[3] = {-1, 0, 0};   // {dst, src, rows}: when dst >= 0 the first workgroup of the next GEMM phase also sums an [rows][8] table
    std::vector<Task> side_tasks;   // non-tile tasks (EPI_COLSUM) appended to the next GEMM phase

    // exact fp32 column sums of a [rows][ld] table of per-workgroup partials -> gradient entries dst[0 .. n): one task per 256 columns
    void colsum_pending(int64_t src, int rows, int ld, int n, int64_t dst) {
        for (int n0 = 0; n0 < n; n0 += 256) {
            Task t;
            std::memset(&t, 0, sizeof(t));
            t.epi = EPI_COLSUM;
            t.c_base = BASE_G; t.c_off = (int32_t)dst; t.c_ld = n;
            t.bias_base = BASE_NONE; t.aux_base = BASE_NONE; t.add_base = BASE_NONE;
            t.m_valid = 1; t.n0 = n0; t.n_valid = std::min(n, n0 + 256);
            t.pad[0] = (int32_t)src; t.pad[1] = rows; t.pad[2] = ld;
            side_tasks.push_back(t);
        }
    }
    void sum8_pending(int dst, int src, int rows) { sum8[0] = dst; sum8[1] = src; sum8[2] = rows; }
    void add_simple_phase(int kind, int group) {
        Phase ph;
        std::memset(&ph, 0, sizeof(ph));
        ph.kind = kind; ph.group = group;
        p.phases.push_back(ph);
    }

    // expand GEMM specs into tile tasks of one phase (ta3n_plan_tiles.cpp)
    void add_gemm_phase(int group, std::vector<GemmSpec> &specs);
    void add_gemm_phase(int group, GemmSpec spec) { std::vector<GemmSpec> s{std::move(spec)}; add_gemm_phase(group, s); }

private:
    // the steps of add_gemm_phase
    bool blocking_denied() const { return (p.deny_blocking >> (p.phases.size() & 63)) & 1; }   // build_plan's retry loop, for the phase being added
    int next_tile_code();
    Phase choose_tiles(int group, int code, const std::vector<GemmSpec> &specs) const;
    std::vector<Panel> expand_panels(const std::vector<GemmSpec> &specs, int BM, int BN);
    std::vector<Task> order_tiles(std::vector<Panel> &panels) const;
    void attach_side_jobs(std::vector<Task> &tiles);
};

// bf16 twins (TA3N_FLAG_BF16_STORE; ta3n_plan_twins.cpp).  extra_produced: ws spans whose twin a non-GEMM kernel of the fused step
// keeps current (unfused_produced: the same for the unfused lists); gemm_only: ws regions that only GEMM launches read.
void add_bf16_twins(ta3n_plan &p, Builder &b, Geom &g, int BT, int D, const std::vector<Span> &extra_produced,
                    const std::vector<Span> &gemm_only = {}, const std::vector<Span> &unfused_produced = {});

}  // namespace ta3n
