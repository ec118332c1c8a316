// Host-side launch plan: parameter layout, workspace regions, phases and GEMM
// tile tasks for one (Bs, Bt, T, D, F, C) configuration.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/ta3n_hip.h"
#include "ta3n_types.h"

struct ParamInfo {
    std::string name;
    int64_t off;
    int32_t rows, cols;   // cols == 0 for 1-D parameters
    bool live;
};

struct Region {
    std::string name;
    int64_t off, size;
};

struct ta3n_plan {
    ta3n_config cfg;
    ta3n::Geom geom;
    std::vector<ParamInfo> params;
    int64_t param_floats = 0, live_floats = 0;
    // ta3n_config.layout_flags: the donor plan's parameter table (empty without it) - Builder::add_param places every parameter where the
    // donor has it - what went wrong doing so, and the maximal runs of this plan's live parameters in the flat buffer (every plan has them)
    std::vector<ParamInfo> layout;
    std::string layout_error;
    std::vector<std::pair<int64_t, int64_t>> live_ranges;
    int64_t first_floats = 0;   // size of the leading parameter block the step's first launch reads (shared frame FC weight + bias)
    std::vector<Region> regions;
    int64_t ws_floats = 0;
    int64_t ws_floats_before_twins = 0;   // (size of the region the ws twins mirror)
    std::vector<ta3n::Seg> segs;
    std::vector<ta3n::Task> tasks;
    std::vector<ta3n::Phase> phases;
    std::vector<ta3n::Wait> waits;      // wait lists of the chained launches (Task.wait_begin / wait_count)
    std::vector<int32_t> tuples, scale_len, scale_id, tuple_first;  // tuple_first[j..j+1) = tuples of scale j
    int n_tuples = 0;
    std::vector<int32_t> phase_kinds;   // per phase: which operand-kind combinations its GEMM tasks use (gemm_tiles' KV bits; filled at upload)
    // workspace offsets of the two frame-attention launches (TA3N_FLAG_FRAME_ATTN; -1 without it).  Kept here and not in Geom, whose
    // layout is fixed; resolved once by the builder and passed to the kernels as launch arguments.
    struct FrameAttn { int32_t F1a = -1, attn = -1, gF1a = -1, gFs = -1, gPfT = -1; } frame_attn;
    // ... and of the two general-attention launches (TA3N_FLAG_GENERAL_ATTN): regions "Ua" (U, then A = tanh(U) in place), "gUa", "gs" and the
    // parameter offsets of attn_layer.2 (weight [1][NB], bias [1])
    struct GeneralAttn { int32_t Ua = -1, gUa = -1, gs = -1, p_wa2 = -1, p_ba2 = -1; } general_attn;
    // TA3N_AGG_RNN: the launch argument of the four recurrent kernels (n_ts == 0 on every other plan)
    ta3n::RnnArgs rnn = {};
    // TA3N_AGG_TEMCONV: the launch argument of the three temporal-convolution kernels (p_w < 0 on every other plan)
    ta3n::TemconvArgs temconv = {-1, -1, -1, -1};
    // TA3N_FLAG_SCORE_ONLY: the launch argument of the score kernel (o_prob < 0 on every other plan)
    ta3n::ScoreArgs score = {0, 0, -1, -1, -1, -1, -1};
    // TA3N_FLAG_TRAIN_METERS: the launch argument of the meters kernel (o_counts < 0 on every other plan)
    ta3n::MetersArgs meters = {-1, -1, 0};
    int64_t class_w_off = 0;    // ws offset of region "class_w" (TA3N_FLAG_CLASS_WEIGHTS; 0 without it): what the launchers put into Hyper::class_w_off
    uint64_t deny_blocking = 0;   // bit i: phase i must not use register-blocked tiles (it does not read bf16 twins; build_plan's retry)
    // device copies (created lazily by the launcher)
    void *d_segs = nullptr;
    void *d_tasks = nullptr;
    void *d_waits = nullptr;
    bool uploaded = false;
    int device = -1;

    int64_t poff(const std::string &name) const;
    int64_t woff(const std::string &name) const;
};

namespace ta3n {
int build_plan(ta3n_plan &p, std::string &err);
void set_error(const std::string &msg);
}
