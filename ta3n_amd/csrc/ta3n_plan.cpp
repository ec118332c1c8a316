// Plan builder: turns a ta3n_config into parameter/workspace layouts and the
// per-launch GEMM tile lists.  Pure host code (no HIP calls) so that the CPU
// test-suite can validate the whole wiring against the oracle.
// Here: the GEMM spec vocabulary, the layout pieces the models share, the three models and build_plan; specs -> tile tasks:
// ta3n_plan_tiles.cpp; bf16 twins: ta3n_plan_twins.cpp.
//
// Math being wired (reference file:line in SURVEY.md Appendix A):
//   F1 = drop_i(relu(X Wsh^T + bsh))                           models.py:565-575
//   Pf = Wcd relu(Wfd GRL(F1) + bfd) + bcd                     models.py:456-462
//   Z_t = relu(W_j concat_{f in tau_t} F1[:,f] + b_j)          TRNmodule.py:58-82
//   R_j = sum_{t in scale j} Z_t
//   Pr_j = W2_j relu(W1_j GRL(R_j) + b1_j) + b2_j              models.py:472-488
//   w = 1 - H(softmax Pr);  V = sum_j (1+w_j) R_j;  Vd = drop_v(V)   models.py:351-357, 379-388, 651, 679
//   Y = Wcv Vd + bcv;  Pv = Wcdv relu(Wdv GRL(Vd) + bdv) + bcdv      models.py:686, 464-470
//   TA3N_FLAG_FRAME_ATTN: wf = 1 - H(softmax Pf);  F1a = (1 + wf) F1 replaces F1 in Z_t             models.py:368-377, 612-614
//   TA3N_FLAG_GENERAL_ATTN: w = softmax_j(<tanh(Wa1 R_j + ba1), wa2> + ba2) replaces w = 1 - H(softmax Pr)   models.py:320-325, 359-366
//   TA3N_FLAG_UNSHARED: the target rows of F1 come from Wsh_t / bsh_t, the target rows of Y from Wcv_t / bcv_t   models.py:174-192, 296-305, 565-566, 686-687
#include "ta3n_plan_builder.h"

#include <cstdlib>

using namespace ta3n;

int64_t ta3n_plan::poff(const std::string &name) const {
    for (const auto &p : params)
        if (p.name == name) return p.off;
    return -1;
}
int64_t ta3n_plan::woff(const std::string &name) const {
    for (const auto &r : regions)
        if (r.name == name) return r.off;
    return -1;
}

namespace {

struct Dims { int Bs, Bt, B, T, D, F, NB, C, BT; };

Dims dims_of(const ta3n_config &c) {
    const int B = c.batch_source + c.batch_target, F = std::min(c.fc_dim, c.feature_dim);   // models.py:129
    return Dims{c.batch_source, c.batch_target, B, c.num_segments, c.feature_dim, F, c.num_bottleneck, c.num_class, B * c.num_segments};
}

// ---------------------------------------------------------------------------------------------------------------------
// GEMM specs: one per affine contraction of a step.  Offsets and dimensions are explicit; x_base is BASE_X or BASE_WS.

// Y = act(X W^T + b), W [N][K]
GemmSpec spec_linear(int M, int N, int K, int x_base, int64_t x_off, int x_ld, int64_t w, int64_t bias, int64_t y_off, int y_ld, bool relu) {
    GemmSpec s;
    s.M = M; s.N = N;
    s.segs.push_back(mkseg(KC(x_base, x_off, x_ld), KC(BASE_P, w, K), K));
    s.proto = proto(BASE_WS, y_off, y_ld);
    with_bias(s.proto, bias);
    if (relu) s.proto.epi |= EPI_RELU;
    return s;
}

// (G W) * [H > 0], G two logits wide: the way back through a discriminator's second layer and its ReLU
GemmSpec spec_masked_back(int M, int N, int64_t g_off, int64_t w, int64_t mask_off, int64_t out_off) {
    GemmSpec s;
    s.M = M; s.N = N;
    s.segs.push_back(mkseg(KC(BASE_WS, g_off, 2), KM(BASE_P, w, N), 2));
    s.proto = proto(BASE_WS, out_off, N);
    with_mask(s.proto, mask_off, N);
    return s;
}

// dW = G^T X; bias_dst >= 0: the tiles of the first column block also write db = column sums of G, i.e. the row sums of
// their own A operand (EPI_ROWSUM_A) - no separate ones^T G tasks, which were as long as a weight-gradient tile each
GemmSpec spec_wgrad(int M, int N, int K, int64_t g_off, int g_ld, int x_base, int64_t x_off, int x_ld, int64_t dst, int64_t bias_dst = -1) {
    GemmSpec gw;
    gw.M = M; gw.N = N;
    gw.segs.push_back(mkseg(KM(BASE_WS, g_off, g_ld), KM(x_base, x_off, x_ld), K));
    gw.proto = proto(BASE_G, dst, N);
    if (bias_dst >= 0) with_bias_grad(gw.proto, bias_dst);
    return gw;
}

// shared frame FC (models.py:565-575) into out_off: + ReLU + dropout_i, or - bn_shared - the linear output only (BatchNorm, ReLU
// and dropout follow in the PH_BN_FWD launch)
// (TA3N_FLAG_UNSHARED: the rows [r0, r0 + nr) alone, through the layer at Wsh / bsh.  A spec's rows count from its own first row, so
// the dropout_i element id - the GLOBAL row * F + n - gets the range's first element as its stream offset: the masks of the target
// half do not restart at row 0)
GemmSpec spec_shared_fc(const Dims &d, int64_t Wsh, int64_t bsh, int64_t out_off, bool bn_shared, int split, int r0 = 0, int nr = -1) {
    const int D = d.D, F = d.F;
    GemmSpec s;
    s.M = nr < 0 ? d.BT : nr; s.N = F;
    if (nr >= 0) {
        s.segs.push_back(mkseg(KC(BASE_X, (int64_t)r0 * D, D), KC(BASE_P, Wsh, D), D));
        s.proto = proto(BASE_WS, out_off + (int64_t)r0 * F, F);
        with_bias(s.proto, bsh);
        s.proto.epi |= EPI_RELU | EPI_DROP_I;
        s.proto.gamma_kind = SK_INV_KEEP_I;
        s.proto.drop_ld = F;
        s.proto.pad2 = (int32_t)(uint32_t)((uint64_t)r0 * (uint64_t)F);
        return s;
    }
    if (split && D >= 512 && (D / 2) % 128 == 0) {
        // split_k bit 2 (round 6 experiment): the launch has ONE tile per compute unit at the headline shape - one resident workgroup
        // pulls its stages at ~15 B/clk where two pull ~21 - so every tile becomes two workgroups over the two halves of K
        // (EPI_SPLITK: partial tile through L2 + ticket, the second to arrive adds and runs the epilogue)
        s.segs.push_back(mkseg(KC(BASE_X, 0, D), KC(BASE_P, Wsh, D), D / 2));
        s.segs.push_back(mkseg(KC(BASE_X, D / 2, D), KC(BASE_P, Wsh + D / 2, D), D / 2));
        s.split = 2;
    } else s.segs.push_back(mkseg(KC(BASE_X, 0, D), KC(BASE_P, Wsh, D), D));
    s.proto = proto(BASE_WS, out_off, F);
    with_bias(s.proto, bsh);
    if (bn_shared) return s;
    s.proto.epi |= EPI_RELU | EPI_DROP_I;
    s.proto.gamma_kind = SK_INV_KEEP_I;
    s.proto.drop_ld = F;
    return s;
}

// parameter offsets of the layers every model has (by their state_dict names)
struct HeadParams {
    int64_t Wsh, bsh, Wfd, bfd, Wcd, bcd, Wdv, bdv, Wcv, bcv, Wcdv, bcdv, Wcv2 = 0, bcv2 = 0;
};

HeadParams head_params(const ta3n_plan &p, bool mcd) {
    HeadParams w;
    w.Wsh = p.poff("fc_feature_shared_source.weight"); w.bsh = p.poff("fc_feature_shared_source.bias");
    w.Wfd = p.poff("fc_feature_domain.weight"); w.bfd = p.poff("fc_feature_domain.bias");
    w.Wcd = p.poff("fc_classifier_domain.weight"); w.bcd = p.poff("fc_classifier_domain.bias");
    w.Wdv = p.poff("fc_feature_domain_video.weight"); w.bdv = p.poff("fc_feature_domain_video.bias");
    w.Wcv = p.poff("fc_classifier_video_source.weight"); w.bcv = p.poff("fc_classifier_video_source.bias");
    w.Wcdv = p.poff("fc_classifier_domain_video.weight"); w.bcdv = p.poff("fc_classifier_domain_video.bias");
    if (mcd) { w.Wcv2 = p.poff("fc_classifier_video_source_2.weight"); w.bcv2 = p.poff("fc_classifier_video_source_2.bias"); }
    return w;
}

// gVt = drop_v'( -beta1 * gHv Wdv + gY Wcv [+ gY2 Wcv2] ), N = width of the video feature
// (TA3N_FLAG_UNSHARED: the videos [b0, b0 + nb) alone, through the classifier at Wcv - a spec's rows count from its own first row, so the
// dropout_v element id, which is the GLOBAL b * N + n, gets the range's first element as its stream offset)
GemmSpec spec_gVt(const Geom &g, int N, const HeadParams &w, bool live_vid, bool mcd, int b0 = 0, int nb = -1, int64_t Wcv = -1) {
    GemmSpec gv;
    gv.M = nb < 0 ? g.B : nb; gv.N = N;
    if (live_vid) gv.segs.push_back(mkseg(KC(BASE_WS, g.o_gHv + (int64_t)b0 * N, N), KM(BASE_P, w.Wdv, N), N, SK_NEG_BETA_VID));
    gv.segs.push_back(mkseg(KC(BASE_WS, g.o_gY + (int64_t)b0 * g.C, g.C), KM(BASE_P, Wcv < 0 ? w.Wcv : Wcv, N), g.C));
    if (mcd) gv.segs.push_back(mkseg(KC(BASE_WS, g.o_gY2, g.C), KM(BASE_P, w.Wcv2, N), g.C));
    gv.proto = proto(BASE_WS, g.o_gVt + (int64_t)b0 * N, N);
    gv.proto.alpha_kind = SK_REVERSE_MU;      // forward(..., reverse=True): everything behind the video feature sees GradReverse(mu) (models.py:682-684)
    gv.proto.epi |= EPI_DROP_V; gv.proto.gamma_kind = SK_INV_KEEP_V; gv.proto.drop_ld = N;
    gv.proto.pad2 = (int32_t)(uint32_t)((uint64_t)b0 * (uint64_t)N);
    return gv;
}

// ---------------------------------------------------------------------------------------------------------------------
// --add_fc (ta3n_config.shared_fc_layers; models.py:145-153, 581-603): L - 1 more Linear(F, F) -> ReLU -> dropout_i layers on the
// shared frame FC.  Layer k's output is F_k, the gradient at its pre-activation gZ_k; F_L / gZ_L are Geom's o_F1 / o_gZ1 (what the
// heads, the pooling kernels and the frame discriminator read), the earlier ones the regions "F_l<k>" / "gZ_l<k>" that only GEMM
// specs address.  Forward: one launch per layer, F_k = drop_i(relu(F_{k-1} W_k^T + b_k)).  Backward: one launch per layer,
// gZ_{k-1} = (gZ_k W_k) * [F_{k-1} > 0] / keep_i beside dW_k = gZ_k^T F_{k-1}, db_k = column sums of gZ_k; dWsh = gZ_1^T X stays last.
struct SharedStack {
    int L = 1;
    int64_t W[4] = {0, 0, 0, 0}, bias[4] = {0, 0, 0, 0};   // parameter offsets of layer k = 2 .. L
    int64_t o_F[4] = {0, 0, 0, 0}, o_gZ[4] = {0, 0, 0, 0}; // ws offsets, k = 1 .. L
};

int shared_layers(const ta3n_config &c) { return c.shared_fc_layers <= 1 ? 1 : c.shared_fc_layers; }

// "" when the configuration's shared_fc_layers is built, otherwise the refusal (naming the option)
std::string shared_layers_refusal(const ta3n_config &c) {
    if (c.shared_fc_layers < 0 || c.shared_fc_layers > 3)
        return "shared_fc_layers (--add_fc) " + std::to_string(c.shared_fc_layers) + " is not built: 1, 2 or 3 (add_fc >= 4 shifts the "
               "reference's place_dis slicing, main.py:368-378)";
    if (c.shared_fc_layers <= 1) return "";
    std::string what;
    if (c.flags & TA3N_FLAG_BN_SHARED) what = "use_bn (TA3N_FLAG_BN_SHARED)";
    else if (c.flags & TA3N_FLAG_MCD) what = "ens_DA MCD (TA3N_FLAG_MCD)";
    else if (c.chain) what = "chain";
    else if (c.split_k) what = "split_k";
    else if (c.wgrads_late) what = "wgrads_late";
    else
        for (int i = 0; i < 16; ++i)
            if (c.phase_tiles[i]) what = "phase_tiles (indexed by the single-layer launch order)";
    return what.empty() ? "" : "shared_fc_layers (--add_fc) " + std::to_string(c.shared_fc_layers) + " with " + what + " is not built";
}

// parameter offsets and the earlier layers' regions; o_F1 / o_gZ1: Geom's (layer L)
void lay_out_stack(ta3n_plan &p, Builder &b, SharedStack &st, int BT, int F, int64_t o_F1, int64_t o_gZ1) {
    st.L = shared_layers(p.cfg);
    for (int k = 2; k <= st.L; ++k) {
        st.W[k] = p.poff("fc_feature_shared_" + std::to_string(k) + "_source.weight");
        st.bias[k] = p.poff("fc_feature_shared_" + std::to_string(k) + "_source.bias");
    }
    for (int k = 1; k < st.L; ++k) st.o_F[k] = b.add_region("F_l" + std::to_string(k), (int64_t)BT * F);
    for (int k = 1; k < st.L; ++k) st.o_gZ[k] = b.add_region("gZ_l" + std::to_string(k), (int64_t)BT * F);
    st.o_F[st.L] = o_F1;
    st.o_gZ[st.L] = o_gZ1;
}

GemmSpec spec_shared_layer(const SharedStack &st, int k, int BT, int F) {   // F_k = drop_i(relu(F_{k-1} W_k^T + b_k))  (models.py:581-603)
    GemmSpec s = spec_linear(BT, F, F, BASE_WS, st.o_F[k - 1], F, st.W[k], st.bias[k], st.o_F[k], F, true);
    s.proto.epi |= EPI_DROP_I;
    s.proto.gamma_kind = SK_INV_KEEP_I;
    s.proto.drop_ld = F;
    s.proto.pad2 = (int32_t)(uint32_t)((uint64_t)(k - 1) * (uint64_t)BT * (uint64_t)F);   // a dropout stream of its own (ta3n_types.h)
    return s;
}

void push_shared_layer_back(std::vector<GemmSpec> &s, const SharedStack &st, int k, int BT, int F) {
    GemmSpec gz;                 // gZ_{k-1} = (gZ_k W_k) * [F_{k-1} > 0] / keep_i
    gz.M = BT; gz.N = F;
    gz.segs.push_back(mkseg(KC(BASE_WS, st.o_gZ[k], F), KM(BASE_P, st.W[k], F), F));
    gz.proto = proto(BASE_WS, st.o_gZ[k - 1], F);
    with_mask(gz.proto, st.o_F[k - 1], F);
    gz.proto.gamma_kind = SK_INV_KEEP_I;
    s.push_back(gz);
    // dW_k = gZ_k^T F_{k-1}, db_k = column sums of gZ_k
    s.push_back(spec_wgrad(F, F, BT, st.o_gZ[k], F, BASE_WS, st.o_F[k - 1], F, st.W[k], st.bias[k]));
}

void add_stack_forward(Builder &b, const SharedStack &st, int group, int BT, int F) {
    for (int k = 2; k <= st.L; ++k) b.add_gemm_phase(group, spec_shared_layer(st, k, BT, F));
}

void add_stack_backward(Builder &b, const SharedStack &st, int group, int BT, int F) {
    for (int k = st.L; k >= 2; --k) { std::vector<GemmSpec> s; push_shared_layer_back(s, st, k, BT, F); b.add_gemm_phase(group, s); }
}

// ---------------------------------------------------------------------------------------------------------------------
// Layout pieces every model uses, in the order the models call them.

// the parameters every model starts with: the shared frame FC (first: ta3n_train_step_after_update relies on it; first_floats:
// its update rides in the step's first launch) and, live and directly behind it, layers 2 .. L of --add_fc (models.py:141, 145-153)
void add_shared_fc_params(ta3n_plan &p, Builder &b, const Dims &d) {
    b.add_linear("fc_feature_shared_source", d.F, d.D, true);
    p.first_floats = p.param_floats;
    for (int k = 2; k <= shared_layers(p.cfg); ++k) b.add_linear("fc_feature_shared_" + std::to_string(k) + "_source", d.F, d.F, true);
}

const char *bn_shared_refusal(const ta3n_config &c, const Dims &d) {
    return ((c.flags & TA3N_FLAG_BN_SHARED) && d.F % BN_COLS != 0)
               ? "use_bn: fc_dim must be a multiple of 4 (the BatchNorm launches move a row's four columns as one 16-byte access)" : nullptr;
}

void add_bn_shared_params(Builder &b, int F) {   // models.py:195-196 (nn.BatchNorm1d(feat_shared_dim) x 2): weight and bias are trained
    b.add_param("bn_shared_S.weight", F, 0, true); b.add_param("bn_shared_S.bias", F, 0, true);
    b.add_param("bn_shared_T.weight", F, 0, true); b.add_param("bn_shared_T.bias", F, 0, true);
}

void init_geom(Geom &g, const Dims &d, int NB, uint32_t flags) {
    std::memset(&g, 0, sizeof(g));
    g.Bs = d.Bs; g.Bt = d.Bt; g.B = d.B; g.T = d.T; g.D = d.D; g.F = d.F; g.NB = NB; g.C = d.C;
    g.flags = flags;
    g.o_ws16 = g.o_p16 = g.o_x16 = g.o_p16b = -1; g.pair_delta = 0;
}

void add_bn_regions(const ta3n_plan &p, Builder &b, Geom &g, const Dims &d) {
    g.o_Z0 = (int32_t)b.add_region("Z0", (int64_t)d.BT * d.F);
    g.o_gZ0 = (int32_t)b.add_region("gZ0", (int64_t)d.BT * d.F);
    g.o_bn_batch = (int32_t)b.add_region("bn_batch", (int64_t)2 * 3 * d.F);
    g.o_bn_run = (int32_t)b.add_region("bn_run", (int64_t)2 * 2 * d.F);
    g.p_bn_w[0] = (int32_t)p.poff("bn_shared_S.weight"); g.p_bn_b[0] = (int32_t)p.poff("bn_shared_S.bias");
    g.p_bn_w[1] = (int32_t)p.poff("bn_shared_T.weight"); g.p_bn_b[1] = (int32_t)p.poff("bn_shared_T.bias");
}

void add_mcd_regions(Builder &b, Geom &g, const Dims &d) {
    g.o_Y2 = (int32_t)b.add_region("Y2", (int64_t)d.B * d.C);
    g.o_gY2 = (int32_t)b.add_region("gY2", (int64_t)d.B * d.C);
}

// The workspace tail, first part: zeros .. tuple_first.  The model's own partial-sum regions follow, then add_tail_end.
bool add_tail_begin(Builder &b, Geom &g, const Dims &d, int n_tuple_first, std::string &err) {
    g.o_zeros = (int32_t)b.add_region("zeros", 64);   // never written: source of out-of-range operand elements
    g.o_ones = (int32_t)b.add_region("ones", (int64_t)d.BT * 4);   // [BT][4] block of ones (k-major A operand of the column sums)
    if (g.o_ones != g.o_zeros + 64) { err = "internal: ones must follow zeros"; return false; }
    g.o_losses = (int32_t)b.add_region("losses", 8);
    g.n_norm_blocks = 256;
    g.o_norm_part = (int32_t)b.add_region("norm_part", g.n_norm_blocks);
    g.o_grad_norm = (int32_t)b.add_region("grad_norm", 4);
    g.o_hyper = (int32_t)b.add_region("hyper", 32);
    g.o_labels = (int32_t)b.add_region("labels", d.B);
    g.o_tuple_first = (int32_t)b.add_region("tuple_first", n_tuple_first);
    return true;
}

void add_tail_end(const ta3n_plan &p, Builder &b, Geom &g, const Dims &d, int64_t loss_part_floats, const HeadParams &w) {
    g.o_loss_part = (int32_t)b.add_region("loss_part", loss_part_floats);
    g.o_metrics = (int32_t)b.add_region("metrics", 8);
    g.o_confusion = (int32_t)b.add_region("confusion", (int64_t)d.C * d.C);
    g.live_floats = (int32_t)p.live_floats;
    g.p_Wcv = (int32_t)w.Wcv; g.p_bcv = (int32_t)w.bcv;
}

// every gradient tile (and column-sum task) of the fused step leaves the sum of its squares in its own slot: the optimiser
// (ta3n_sgd_step_fused) adds the slots in a fixed order instead of re-reading the gradient buffer.  extra_slots: see bn_sumsq_slots
void assign_sumsq_slots(ta3n_plan &p, Builder &b, Geom &g, int extra_slots) {
    std::vector<size_t> grad_tasks;
    for (const Phase &ph : p.phases)
        if (ph.group == 4 && ph.kind == PH_GEMM)
            for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i)
                if ((p.tasks[i].seg_count > 0 || (p.tasks[i].epi & EPI_COLSUM)) && p.tasks[i].c_base == BASE_G) grad_tasks.push_back((size_t)i);
    g.n_sumsq = (int32_t)grad_tasks.size() + extra_slots;
    g.o_sumsq = (int32_t)b.add_region("sumsq", g.n_sumsq);
    for (size_t k = 0; k < grad_tasks.size(); ++k) {
        p.tasks[grad_tasks[k]].epi |= EPI_SUMSQ;
        p.tasks[grad_tasks[k]].pad[3] = g.o_sumsq + (int32_t)k;
    }
}

// use_bn: the BatchNorm weight / bias gradients come from the PH_BN_BWD launch, not from a tile - its workgroups ((F + BN_COLS - 1) / BN_COLS
// column blocks x 2 domains) leave their sums of squares in the LAST slots of the sumsq region (bn_shared_bwd_kernel)
int bn_sumsq_slots(bool bn_shared, int F) { return bn_shared ? 2 * ((F + BN_COLS - 1) / BN_COLS) : 0; }

// split-K pairs: partial tiles and tickets behind everything else (outside the span the twins mirror)
void lay_out_split_pairs(ta3n_plan &p, Builder &b) {
    std::vector<int64_t> pair_off(b.n_split_pairs, -1);
    int64_t floats = 0;
    for (const Phase &ph : p.phases) {
        if (ph.kind != PH_GEMM) continue;
        const int64_t tile = (int64_t)(32 * ph.wm * std::max(ph.rm, 1)) * (32 * ph.wn * std::max(ph.rn, 1));
        for (int i = ph.task_begin; i < ph.task_begin + ph.task_count; ++i) {
            const Task &t = p.tasks[i];
            if ((t.epi & EPI_SPLITK) && pair_off[t.pad[0]] < 0) { pair_off[t.pad[0]] = floats; floats += 2 * tile; }
        }
    }
    const int64_t o_part = b.add_region("splitk_part", floats);
    const int64_t o_tick = b.add_region("splitk_ticket", b.n_split_pairs);
    for (auto &t : p.tasks)
        if (t.epi & EPI_SPLITK) {
            const int pair = t.pad[0];
            t.pad[0] = (int32_t)(o_part + pair_off[pair]);
            t.pad[1] = (int32_t)(o_tick + pair);
        }
}

bool workspace_fits(const ta3n_plan &p, std::string &err) {
    if (p.ws_floats >= (1ll << 31)) { err = "workspace too large for 32-bit offsets"; return false; }
    return true;
}

// what closes every model, behind add_bf16_twins
int finish_plan(ta3n_plan &p, Builder &b, std::string &err) {
    if (!workspace_fits(p, err)) return TA3N_ERR_INVALID;
    if (b.mixed_kinds) { err = "internal: a GEMM spec mixes operand kinds across its K segments"; return TA3N_ERR_INVALID; }
    if (b.n_split_pairs > 0) {
        lay_out_split_pairs(p, b);
        if (!workspace_fits(p, err)) return TA3N_ERR_INVALID;
    }
    for (auto &t : p.tasks)      // (after the twin re-addressing: the copies must be the final Segs)
        if (t.seg_count > 0) t.seg0 = p.segs[t.seg_begin];
    // TA3N_FLAG_CLASS_WEIGHTS: the per-class weights of the class cross-entropy, written by the caller.  Behind everything else and only
    // under the flag: no other plan changes by a byte.  Reached through Hyper::class_w_off (Geom's layout is fixed).
    if (p.cfg.flags & TA3N_FLAG_CLASS_WEIGHTS) {
        p.class_w_off = b.add_region("class_w", 64);
        if (!workspace_fits(p, err)) return TA3N_ERR_INVALID;
    }
    // TA3N_FLAG_TRAIN_METERS: one launch behind the fused step list (group 4, where the plan has one) and behind the loss list (group 1),
    // two regions behind everything else.  Only under the flag: no other plan changes by a byte.  A level is counted when its ADV flag is
    // set and the plan has its logits row by row (no relation rows outside trn-m: region "Pr" is a stub there).
    if (p.cfg.flags & TA3N_FLAG_TRAIN_METERS) {
        const Geom &g = p.geom;
        auto rows_of = [&p](const char *name) { for (const auto &r : p.regions) if (r.name == name) return r.size / 2; return (int64_t)0; };
        p.meters.levels = ((p.cfg.flags & TA3N_FLAG_ADV_RELATION) && g.n_rel > 0 && rows_of("Pr") == (int64_t)g.B * g.n_rel ? 1 : 0) |
                          ((p.cfg.flags & TA3N_FLAG_ADV_VIDEO) && rows_of("Pv") == g.B ? 2 : 0) |
                          ((p.cfg.flags & TA3N_FLAG_ADV_FRAME) && rows_of("Pf") == (int64_t)g.B * g.T ? 4 : 0);
        p.meters.o_counts = (int32_t)b.add_region("meter_counts", MT_WORDS);
        p.meters.o_sums = (int32_t)b.add_region("meter_sums", 2 * METER_SUMS);      // (regions start on multiples of 64 floats: 8-byte aligned)
        if (!workspace_fits(p, err)) return TA3N_ERR_INVALID;
        bool fused = false;
        for (const Phase &ph : p.phases) fused = fused || ph.group == 4;
        if (fused) b.add_simple_phase(PH_TRAIN_METERS, 4);
        b.add_simple_phase(PH_TRAIN_METERS, 1);
    }
    return TA3N_OK;
}

const char *avgpool_dims_refusal(const Dims &d) {
    if (d.T < 1 || d.T > 64) return "num_segments must be in [1,64]";
    if (d.F % 4 != 0) return "avgpool: fc_dim must be a multiple of 4";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// TA3N_AGG_AVGPOOL: BASELINE configs[0] (TemPooling, source-only).  Reference: models.py:557-579 (shared frame FC),
// 421-433 (aggregate_frames, "1. averaging"), 679-687 (dropout_v, classifier), main.py:439-451 (CE on the source rows),
// 574-583 (backward, clip, SGD).  Launches: F1 GEMM, pool_cls kernel, {dWsh, dWcv} GEMM, SGD.  ta3n_forward runs the first
// two, ta3n_loss nothing, ta3n_backward the third; ta3n_train_step all three.
int build_plan_avgpool(ta3n_plan &p, std::string &err) {
    const ta3n_config &c = p.cfg;
    const Dims d = dims_of(c);
    const int B = d.B, BT = d.BT, D = d.D, F = d.F, C = d.C;
    const uint32_t da_flags = TA3N_FLAG_ADV_RELATION | TA3N_FLAG_ADV_VIDEO | TA3N_FLAG_ADV_FRAME | TA3N_FLAG_ATTN_ENTROPY | TA3N_FLAG_TRANS_ATTN;
    if (c.flags & da_flags) { err = "avgpool is built for the source-only configuration: no adversarial / attention flags (SURVEY 8f rank 4)"; return TA3N_ERR_INVALID; }
    if (c.flags & TA3N_FLAG_TARGET_ENTROPY) { err = "avgpool: TA3N_FLAG_TARGET_ENTROPY (add_loss_DA target_entropy) is not built"; return TA3N_ERR_INVALID; }
    if (c.flags & TA3N_FLAG_TARGET_LABELS) {
        err = "TA3N_FLAG_TARGET_LABELS (use_target Sv) on the source-only avgpool plan: built on the general avgpool plan (an adversarial flag) and on trn-m";
        return TA3N_ERR_INVALID;
    }
    if (const char *e = avgpool_dims_refusal(d)) { err = e; return TA3N_ERR_INVALID; }
    Builder b(p);
    // live parameters first (the all-reduce / optimiser operand), then the rest of the reference's state_dict for this configuration
    add_shared_fc_params(p, b, d);
    b.add_linear("fc_classifier_video_source", C, F, true);            // :272 (feat_aggregated_dim = F, :246-247)
    p.live_floats = p.param_floats;
    const std::pair<const char *, int> rest[] = {{"fc_feature_source", F}, {"fc_feature_domain", F}, {"fc_classifier_source", C}, {"fc_classifier_domain", 2},
                                                 {"fc_feature_video_source", F}, {"fc_feature_video_source_2", F}, {"fc_feature_domain_video", F}, {"fc_classifier_domain_video", 2}};
    for (auto &r : rest) b.add_linear(r.first, r.second, F, false);
    const HeadParams w = head_params(p, false);

    Geom &g = p.geom;
    init_geom(g, d, F, c.flags);
    g.o_F1 = (int32_t)b.add_region("F1", (int64_t)BT * F);
    g.o_V = (int32_t)b.add_region("V", (int64_t)B * F);
    g.o_Vd = (int32_t)b.add_region("Vd", (int64_t)B * F);
    g.o_Y = (int32_t)b.add_region("Y", (int64_t)B * C);
    g.o_gY = (int32_t)b.add_region("gY", (int64_t)B * C);
    g.o_gZ1 = (int32_t)b.add_region("gZ1", (int64_t)BT * F);
    SharedStack st;
    lay_out_stack(p, b, st, BT, F, g.o_F1, g.o_gZ1);
    if (!add_tail_begin(b, g, d, 1, err)) return TA3N_ERR_INVALID;
    g.n_vid_wg = B; g.n_frm_wg = 0;
    add_tail_end(p, b, g, d, (int64_t)B * 8, w);

    auto grads = [&]() {
        std::vector<GemmSpec> s;
        s.push_back(spec_wgrad(F, D, BT, st.o_gZ[1], F, BASE_X, 0, D, w.Wsh, w.bsh));   // dWsh = gZ1^T X, dbsh = column sums of gZ1 (of the first layer's gradient with --add_fc > 1)
        s.push_back(spec_wgrad(C, F, B, g.o_gY, C, BASE_WS, g.o_Vd, F, w.Wcv, w.bcv));   // dWcv = gY^T Vd, dbcv = column sums of gY
        return s;
    };
    for (int group : {0, 4}) {           // ta3n_forward / first part of ta3n_train_step
        b.add_gemm_phase(group, spec_shared_fc(d, w.Wsh, w.bsh, st.o_F[1], false, 0));      // (--add_fc > 1: into the first of the stacked layers' outputs)
        add_stack_forward(b, st, group, BT, F);
        b.add_simple_phase(PH_POOL_CLS, group);
        if (group == 4) { b.sum8_pending(g.o_losses, g.o_loss_part, B); add_stack_backward(b, st, 4, BT, F); auto q = grads(); b.add_gemm_phase(4, q); }
    }
    b.sum8_pending(g.o_losses, g.o_loss_part, B);
    add_stack_backward(b, st, 2, BT, F);
    { auto q = grads(); b.add_gemm_phase(2, q); }   // ta3n_backward (also adds up the loss partials for logging)
    b.add_simple_phase(PH_GRAD_NORM, 3);
    b.add_simple_phase(PH_SGD, 3);
    assign_sumsq_slots(p, b, g, 0);      // fused grad-norm partials, as in the trn-m step
    add_bf16_twins(p, b, g, BT, D, {Span{g.o_gZ1, g.o_gZ1 + (int64_t)BT * F}});   // pool_cls keeps the twin of gZ1
    return finish_plan(p, b, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// TA3N_AGG_AVGPOOL, general: TemPooling with the adversarial branches (the "RevGrad" rows of the paper's TemPooling table;
// also what the module path uses for every avgpool model, because there the caller assembles the loss).  Reference:
// models.py:557-579 (shared frame FC), 456-462 (frame discriminator), 421-433 (averaging), 679-687 (dropout_v, classifier),
// 464-470 (video discriminator; feat_aggregated_dim = F, :246-247), 697-708 (pred_domain = [video again, video, frame]),
// main.py:439-451, 508-538 (losses), 574-583.  Every Linear is a tile-list GEMM; the three small kernels are the
// averaging, the losses (the trn-m loss kernel with zero relation rows) and the way back through the averaging.
// Launches of one step (ta3n_forward / ta3n_loss / ta3n_backward, or all of them as ta3n_train_step): F1 | Hf | mean |
// {Y, Hv} | {Pv, Pf} | losses | {gHv, gHf, small weight gradients} | {gVt, dWdv, dWfd} | spread | gZ1 | dWsh.
struct AvgpoolDa {
    Builder &b;
    const Geom &g;
    const Dims d;
    HeadParams w;
    SharedStack st;
    bool live_frm, live_vid, mcd, bn_shared;
    // TA3N_AGG_RNN (models.py:202-215, 392-422): the two aggregator launches become the recurrence; nullptr: TemPooling
    const RnnArgs *rnn = nullptr;
    int64_t Wih = -1, bih = -1, Whh = -1, bhh = -1;
    // TA3N_AGG_TEMCONV (models.py:228-243, 654-672): the two aggregator launches become the filter's, and one more launch at the end of the
    // way back sums the per-video parts of the four parameter gradients
    bool temconv = false;

    void add_step_phase(int kind, int group, int t) { b.add_simple_phase(kind, group); b.p.phases.back().task_begin = t; }

    // Xp | Gx = Xp W_ih^T + b_ih over all n_ts B rows | per step { Gh_t = h_{t-1} W_hh^T + b_hh | cell }.  h keeps n_ts + 1 slabs with
    // slab 0 zero, so every step has the same shape (and dW_hh is one weight gradient over all the rows)
    void rnn_forward(int group) {
        const int B = d.B, F = d.F, GF = (rnn->cell ? 3 : 4) * F;
        b.add_simple_phase(PH_RNN_POOL_FWD, group);
        b.add_gemm_phase(group, spec_linear(rnn->n_ts * B, GF, F, BASE_WS, rnn->o_Xp, F, Wih, bih, rnn->o_Gx, GF, false));
        for (int t = 0; t < rnn->n_ts; ++t) {
            b.add_gemm_phase(group, spec_linear(B, GF, F, BASE_WS, rnn->o_h + (int64_t)t * B * F, F, Whh, bhh, rnn->o_Gh + (int64_t)t * B * GF, GF, false));
            add_step_phase(PH_RNN_CELL_FWD, group, t);
        }
    }

    // t descending { cell backward | gh_{t-1} = gGh_t W_hh + its direct part } | {dW_ih, db_ih, dW_hh, db_hh, gXp} | route gXp to the frames
    void rnn_backward(int group) {
        const int B = d.B, F = d.F, GF = (rnn->cell ? 3 : 4) * F, rows = rnn->n_ts * B;
        for (int t = rnn->n_ts - 1; t >= 0; --t) {
            add_step_phase(PH_RNN_CELL_BWD, group, t);
            if (t == 0) break;                                    // (nobody reads the gradient at the zero initial state)
            GemmSpec gh;
            gh.M = B; gh.N = F;
            gh.segs.push_back(mkseg(KC(BASE_WS, rnn->o_gGh + (int64_t)t * B * GF, GF), KM(BASE_P, Whh, F), GF));
            gh.proto = proto(BASE_WS, rnn->o_gh, F);
            with_add(gh.proto, rnn->o_ghd, F);
            b.add_gemm_phase(group, gh);
        }
        std::vector<GemmSpec> s;
        s.push_back(spec_wgrad(GF, F, rows, rnn->o_gGx, GF, BASE_WS, rnn->o_Xp, F, Wih, bih));   // dW_ih = gGx^T Xp, db_ih
        s.push_back(spec_wgrad(GF, F, rows, rnn->o_gGh, GF, BASE_WS, rnn->o_h, F, Whh, bhh));    // dW_hh = gGh^T h_prev (slabs 0 .. n_ts - 1), db_hh
        GemmSpec gx;                                                                              // gXp = gGx W_ih
        gx.M = rows; gx.N = F;
        gx.segs.push_back(mkseg(KC(BASE_WS, rnn->o_gGx, GF), KM(BASE_P, Wih, F), GF));
        gx.proto = proto(BASE_WS, rnn->o_gXp, F);
        s.push_back(gx);
        b.add_gemm_phase(group, s);
        b.add_simple_phase(PH_RNN_POOL_BWD, group);
    }

    void forward(int group) {
        const int B = d.B, BT = d.BT, F = d.F, C = d.C;
        b.add_gemm_phase(group, spec_shared_fc(d, w.Wsh, w.bsh, bn_shared ? g.o_Z0 : st.o_F[1], bn_shared, 0));
        if (bn_shared) b.add_simple_phase(PH_BN_FWD, group);
        add_stack_forward(b, st, group, BT, F);
        if (live_frm) b.add_gemm_phase(group, spec_linear(BT, F, F, BASE_WS, g.o_F1, F, w.Wfd, w.bfd, g.o_Hf, F, true));   // models.py:458-459
        if (rnn) rnn_forward(group); else b.add_simple_phase(temconv ? PH_TEMCONV_FWD : PH_POOL_AVG_FWD, group);
        {
            std::vector<GemmSpec> s{spec_linear(B, C, F, BASE_WS, g.o_Vd, F, w.Wcv, w.bcv, g.o_Y, C, false)};                     // :686
            if (mcd) s.push_back(spec_linear(B, C, F, BASE_WS, g.o_Vd, F, w.Wcv2, w.bcv2, g.o_Y2, C, false));                     // :717-718
            if (live_vid) s.push_back(spec_linear(B, F, F, BASE_WS, g.o_Vd, F, w.Wdv, w.bdv, g.o_Hv, F, true));                   // :466-467
            b.add_gemm_phase(group, s);
        }
        if (live_vid || live_frm) {
            std::vector<GemmSpec> s;
            if (live_vid) s.push_back(spec_linear(B, 2, F, BASE_WS, g.o_Hv, F, w.Wcdv, w.bcdv, g.o_Pv, 2, false));                // :468
            if (live_frm) s.push_back(spec_linear(BT, 2, F, BASE_WS, g.o_Hf, F, w.Wcd, w.bcd, g.o_Pf, 2, false));                 // :460
            b.add_gemm_phase(group, s);
        }
    }

    void backward(int group) {
        const int B = d.B, BT = d.BT, D = d.D, F = d.F, C = d.C;
        {   // what depends only on the logit gradients
            std::vector<GemmSpec> s;
            if (live_vid) {
                s.push_back(spec_masked_back(B, F, g.o_gPv, w.Wcdv, g.o_Hv, g.o_gHv));
                s.push_back(spec_wgrad(2, F, B, g.o_gPv, 2, BASE_WS, g.o_Hv, F, w.Wcdv, w.bcdv));
            }
            if (live_frm) {
                s.push_back(spec_masked_back(BT, F, g.o_gPf, w.Wcd, g.o_Hf, g.o_gHf));
                s.push_back(spec_wgrad(2, F, BT, g.o_gPf, 2, BASE_WS, g.o_Hf, F, w.Wcd, w.bcd));
            }
            s.push_back(spec_wgrad(C, F, B, g.o_gY, C, BASE_WS, g.o_Vd, F, w.Wcv, w.bcv));
            if (mcd) s.push_back(spec_wgrad(C, F, B, g.o_gY2, C, BASE_WS, g.o_Vd, F, w.Wcv2, w.bcv2));
            b.add_gemm_phase(group, s);
        }
        {   // gVt = dropout_v'( -beta1 * gHv Wdv + gY Wcv ), first-layer weight gradients of the discriminators
            std::vector<GemmSpec> s{spec_gVt(g, F, w, live_vid, mcd)};
            if (live_vid) s.push_back(spec_wgrad(F, F, B, g.o_gHv, F, BASE_WS, g.o_Vd, F, w.Wdv, w.bdv));
            if (live_frm) s.push_back(spec_wgrad(F, F, BT, g.o_gHf, F, BASE_WS, g.o_F1, F, w.Wfd, w.bfd));
            b.add_gemm_phase(group, s);
        }
        if (rnn) rnn_backward(group); else b.add_simple_phase(temconv ? PH_TEMCONV_BWD : PH_POOL_AVG_BWD, group);
        if (live_frm) {   // gZ1 = ( -beta2 gHf Wfd + gVt / T ) * [F1 > 0] / keep_i
            GemmSpec gz;
            gz.M = BT; gz.N = F;
            gz.segs.push_back(mkseg(KC(BASE_WS, g.o_gHf, F), KM(BASE_P, w.Wfd, F), F, SK_NEG_BETA_FRM));
            gz.proto = proto(BASE_WS, g.o_gZ1, F);
            with_add(gz.proto, g.o_gRa, F);
            with_mask(gz.proto, g.o_F1, F);
            gz.proto.gamma_kind = SK_INV_KEEP_I;
            b.add_gemm_phase(group, gz);
        }
        add_stack_backward(b, st, group, BT, F);
        if (bn_shared) b.add_simple_phase(PH_BN_BWD, group);
        b.add_gemm_phase(group, spec_wgrad(F, D, BT, bn_shared ? g.o_gZ0 : st.o_gZ[1], F, BASE_X, 0, D, w.Wsh, w.bsh));
        if (temconv) b.add_simple_phase(PH_TEMCONV_WGRAD, group);      // (the last launch of the way back: in front of PH_GRAD_NORM)
    }
};

// What neither TA3N_AGG_RNN nor TA3N_AGG_TEMCONV is built with: "" when the configuration has none of it, otherwise the refusal, which
// begins with `head` (the aggregation) and names the option
std::string new_aggregation_refusal(const ta3n_config &c, const std::string &head) {
    const std::pair<uint32_t, const char *> flags[] = {
        {TA3N_FLAG_BF16_MFMA, "TA3N_FLAG_BF16_MFMA"}, {TA3N_FLAG_BF16_STORE, "TA3N_FLAG_BF16_STORE"}, {TA3N_FLAG_F32_SPLIT, "TA3N_FLAG_F32_SPLIT"},
        {TA3N_FLAG_MCD, "TA3N_FLAG_MCD (ens_DA MCD)"}, {TA3N_FLAG_BN_SHARED, "TA3N_FLAG_BN_SHARED (use_bn)"},
        {TA3N_FLAG_TRANS_ATTN, "TA3N_FLAG_TRANS_ATTN (use_attn TransAttn)"}, {TA3N_FLAG_ATTN_ENTROPY, "TA3N_FLAG_ATTN_ENTROPY (add_loss_DA attentive_entropy)"},
        {TA3N_FLAG_TARGET_ENTROPY, "TA3N_FLAG_TARGET_ENTROPY (add_loss_DA target_entropy)"}, {TA3N_FLAG_FRAME_ATTN, "TA3N_FLAG_FRAME_ATTN (use_attn_frame)"},
        {TA3N_FLAG_GENERAL_ATTN, "TA3N_FLAG_GENERAL_ATTN (use_attn general)"}, {TA3N_FLAG_UNSHARED, "TA3N_FLAG_UNSHARED (share_params N)"}};
    for (const auto &f : flags)
        if (c.flags & f.first) return head + f.second + " is not built";
    if (c.shared_fc_layers > 1) return head + "shared_fc_layers (--add_fc) " + std::to_string(c.shared_fc_layers) + " is not built";
    if (c.chain) return head + "chain is not built";
    if (c.split_k) return head + "split_k is not built";
    if (c.wgrads_late) return head + "wgrads_late is not built";
    for (int i = 0; i < 16; ++i)
        if (c.phase_tiles[i]) return head + "phase_tiles is not built";
    if (c.layout_flags) return head + "layout_flags is not built";
    return "";
}

// "" when the configuration is built on TA3N_AGG_TEMCONV, otherwise the refusal, naming what is not built there
std::string temconv_refusal(const ta3n_config &c) {
    return new_aggregation_refusal(c, "TA3N_AGG_TEMCONV (frame_aggregation temconv) with ");
}

// "" when the configuration is built on TA3N_AGG_RNN, otherwise the refusal, naming what is not built there
std::string rnn_refusal(const ta3n_config &c) {
    const std::string e = new_aggregation_refusal(c, "TA3N_AGG_RNN (frame_aggregation rnn) with ");
    if (!e.empty()) return e;
    if (c.rnn_cell != 0 && c.rnn_cell != 1) return "rnn_cell must be 0 (LSTM) or 1 (GRU), not " + std::to_string(c.rnn_cell);
    if (c.n_ts < 0) return "n_ts must not be negative (0 means 5), not " + std::to_string(c.n_ts);
    return "";
}

int build_plan_avgpool_general(ta3n_plan &p, std::string &err) {
    const ta3n_config &c = p.cfg;
    const Dims d = dims_of(c);
    const int B = d.B, BT = d.BT, F = d.F, C = d.C;
    const bool is_rnn = c.aggregation == TA3N_AGG_RNN, is_temconv = c.aggregation == TA3N_AGG_TEMCONV;
    if (c.flags & (TA3N_FLAG_ATTN_ENTROPY | TA3N_FLAG_TRANS_ATTN)) {
        err = "avgpool: attention / attentive entropy are not built (the reference's script switches them off with use_attn none)";
        return TA3N_ERR_INVALID;
    }
    if (c.flags & TA3N_FLAG_TARGET_ENTROPY) { err = "avgpool: TA3N_FLAG_TARGET_ENTROPY (add_loss_DA target_entropy) is not built"; return TA3N_ERR_INVALID; }
    if (const char *e = avgpool_dims_refusal(d)) { err = e; return TA3N_ERR_INVALID; }
    if (const char *e = bn_shared_refusal(c, d)) { err = e; return TA3N_ERR_INVALID; }
    const bool live_frm = (c.flags & TA3N_FLAG_ADV_FRAME) != 0;
    // the video discriminator also serves the relation slot (models.py:707-708), see loss_kernel
    const bool live_vid = (c.flags & (TA3N_FLAG_ADV_VIDEO | TA3N_FLAG_ADV_RELATION)) != 0;
    const bool mcd = (c.flags & TA3N_FLAG_MCD) != 0;                   // the DA options of the TemPooling rows (module path)
    const bool feat_grads = (c.flags & TA3N_FLAG_FEATURE_GRADS) != 0;
    const bool bn_shared = (c.flags & TA3N_FLAG_BN_SHARED) != 0;
    Builder b(p);
    add_shared_fc_params(p, b, d);
    b.lin("fc_feature_domain", F, F, live_frm);                        // :161
    b.lin("fc_classifier_domain", 2, F, live_frm);                     // :170
    b.lin("fc_feature_domain_video", F, F, live_vid);                  // :267 (feat_aggregated_dim = F)
    b.add_linear("fc_classifier_video_source", C, F, true);            // :272
    if (mcd) b.add_linear("fc_classifier_video_source_2", C, F, true); // :276-279
    if (bn_shared) add_bn_shared_params(b, F);                         // :195-196
    b.lin("fc_classifier_domain_video", 2, F, live_vid);               // :281
    const int GF = (c.rnn_cell ? 3 : 4) * F;                           // TA3N_AGG_RNN: nn.LSTM / nn.GRU(F, F), one layer (:202-207)
    if (is_rnn) {                                                      // (bn_before_rnn / bn_after_rnn, :213-214, are never called: no parameters of the plan)
        b.add_param("rnn.weight_ih_l0", GF, F, true); b.add_param("rnn.weight_hh_l0", GF, F, true);
        b.add_param("rnn.bias_ih_l0", GF, 0, true); b.add_param("rnn.bias_hh_l0", GF, 0, true);
    }
    if (is_temconv) {      // TA3N_AGG_TEMCONV: tcl_3_1 = Conv2d(1, 1, (3, 1)) (:230); tcl_5_1, tcl_3_2, tcl_5_2, bn_1_*, bn_2_*, conv_fusion (:231-243) are
        b.add_param("tcl_3_1.conv2d.weight", 3, 0, true);      // never called: no parameters of the plan
        b.add_param("tcl_3_1.conv2d.bias", 1, 0, true);
    }
    p.live_floats = p.param_floats;
    b.add_dead_linears();
    b.add_linear("fc_feature_source", F, F, false);
    b.add_linear("fc_classifier_source", C, F, false);
    b.add_linear("fc_feature_video_source", F, F, false);
    b.add_linear("fc_feature_video_source_2", F, F, false);
    const HeadParams w = head_params(p, mcd);

    Geom &g = p.geom;
    init_geom(g, d, F, c.flags);
    g.o_F1 = (int32_t)b.add_region("F1", (int64_t)BT * F);
    g.o_Hf = (int32_t)b.add_region("Hf", live_frm ? (int64_t)BT * F : 4);
    g.o_Pf = (int32_t)b.add_region("Pf", (int64_t)BT * 2);
    g.o_V = (int32_t)b.add_region("V", (int64_t)B * F);
    g.o_Vd = (int32_t)b.add_region("Vd", (int64_t)B * F);
    g.o_Y = (int32_t)b.add_region("Y", (int64_t)B * C);
    g.o_Hv = (int32_t)b.add_region("Hv", live_vid ? (int64_t)B * F : 4);
    g.o_Pv = (int32_t)b.add_region("Pv", (int64_t)B * 2);
    g.o_Pr = (int32_t)b.add_region("Pr", 4);            // no relation rows
    g.o_gY = (int32_t)b.add_region("gY", (int64_t)B * C);
    g.o_gPv = (int32_t)b.add_region("gPv", (int64_t)B * 2);
    g.o_gPr = (int32_t)b.add_region("gPr", 4);
    g.o_gPf = (int32_t)b.add_region("gPf", (int64_t)BT * 2);
    g.o_gHv = (int32_t)b.add_region("gHv", live_vid ? (int64_t)B * F : 4);
    const int64_t o_gHf = b.add_region("gHf", live_frm ? (int64_t)BT * F : 4);
    g.o_gHf = live_frm ? (int32_t)o_gHf : -1;           // -1: pool_avg_bwd writes gZ1 directly
    g.o_gVt = (int32_t)b.add_region("gVt", (int64_t)B * F);
    g.o_gRa = (int32_t)b.add_region("gRa", live_frm ? (int64_t)BT * F : 4);   // gVt / T spread over the segments
    g.o_gZ1 = (int32_t)b.add_region("gZ1", (int64_t)BT * F);
    AvgpoolDa m{b, g, d, w, SharedStack(), live_frm, live_vid, mcd, bn_shared};
    lay_out_stack(p, b, m.st, BT, F, g.o_F1, g.o_gZ1);
    if (is_rnn) {
        RnnArgs &r = p.rnn;
        int32_t len_ts = 0, frames[RNN_MAX_SLOTS + 64];
        r.cell = c.rnn_cell; r.n_ts = c.n_ts ? c.n_ts : 5;
        if (ta3n_rnn_slots(d.T, r.n_ts, &len_ts, frames) != TA3N_OK) { err = ta3n_last_error(); return TA3N_ERR_INVALID; }
        if (len_ts * r.n_ts > RNN_MAX_SLOTS) { err = "n_ts: more than 128 pooling slots"; return TA3N_ERR_INVALID; }
        r.len_ts = len_ts;
        for (int i = 0; i < len_ts * r.n_ts; ++i) r.frames[i] = (uint8_t)frames[i];
        const int64_t rows = (int64_t)r.n_ts * B;
        if (rows * GF >= (1ll << 31)) { err = "problem too large for 32-bit offsets"; return TA3N_ERR_INVALID; }
        r.o_Xp = (int32_t)b.add_region("rnn_Xp", rows * F);
        r.o_Gx = (int32_t)b.add_region("rnn_Gx", rows * GF);
        r.o_Gh = (int32_t)b.add_region("rnn_Gh", rows * GF);
        r.o_gates = (int32_t)b.add_region("rnn_gates", rows * GF);
        r.o_c = (int32_t)b.add_region("rnn_c", (rows + B) * F);
        r.o_h = (int32_t)b.add_region("rnn_h", (rows + B) * F);
        r.o_gGx = (int32_t)b.add_region("rnn_gGx", rows * GF);
        r.o_gGh = (int32_t)b.add_region("rnn_gGh", rows * GF);
        r.o_gc = (int32_t)b.add_region("rnn_gc", rows * F);
        r.o_gh = (int32_t)b.add_region("rnn_gh", (int64_t)B * F);
        r.o_ghd = (int32_t)b.add_region("rnn_ghd", (int64_t)B * F);
        r.o_gXp = (int32_t)b.add_region("rnn_gXp", rows * F);
        m.rnn = &p.rnn;
        m.Wih = p.poff("rnn.weight_ih_l0"); m.Whh = p.poff("rnn.weight_hh_l0");
        m.bih = p.poff("rnn.bias_ih_l0"); m.bhh = p.poff("rnn.bias_hh_l0");
    }
    if (is_temconv) {
        p.temconv.p_w = (int32_t)p.poff("tcl_3_1.conv2d.weight"); p.temconv.p_b = (int32_t)p.poff("tcl_3_1.conv2d.bias");
        p.temconv.o_part = (int32_t)b.add_region("tc_part", (int64_t)B * 4);
        m.temconv = true;
    }
    g.o_attn = (int32_t)b.add_region("attn", 4); g.o_gattn = (int32_t)b.add_region("g_attn", 4);
    if (feat_grads) g.o_gV_ext = (int32_t)b.add_region("gV_ext", (int64_t)B * F);
    if (mcd) add_mcd_regions(b, g, d);
    if (bn_shared) add_bn_regions(p, b, g, d);
    if (!add_tail_begin(b, g, d, 1, err)) return TA3N_ERR_INVALID;
    add_tail_end(p, b, g, d, 8, w);

    m.forward(0);
    b.add_simple_phase(PH_LOSS, 1);
    m.backward(2);
    b.add_simple_phase(PH_GRAD_NORM, 3);
    b.add_simple_phase(PH_SGD, 3);
    m.forward(4);                           // ta3n_train_step: the same launches as one sequence
    b.add_simple_phase(PH_LOSS, 4);
    m.backward(4);
    // (TA3N_AGG_TEMCONV - never with bn_shared - : the four tcl_3_1 gradients come from PH_TEMCONV_WGRAD, which leaves their sum of squares in the last slot)
    assign_sumsq_slots(p, b, g, bn_sumsq_slots(bn_shared, F) + (is_temconv ? 1 : 0));
    if (is_temconv) p.temconv.o_sumsq = g.o_sumsq + g.n_sumsq - 1;
    // (no bf16 twins on this path: the small kernels between the launches do not maintain them; the contractions still
    // round their operands in registers with TA3N_FLAG_BF16_MFMA)
    return finish_plan(p, b, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// TA3N_AGG_TRN_M: the TA3N model.  What the spec builders and the launch lists share lives here.
struct TrnModel {
    ta3n_plan &p;
    Builder b;
    Geom &g;
    const ta3n_config &c;
    const Dims d;
    const int NR, NT;
    // Which discriminators receive a gradient depends on the options, as in the reference, where a parameter whose output feeds no loss
    // keeps grad None and is skipped by SGD (no weight decay either): the frame discriminator is live only with its adversarial loss
    // (place_adv[2], main.py:508-538), the video discriminator with its loss (attentive entropy needs it too, and the plan requires ADV_VIDEO
    // for it), the relation discriminators with their loss OR the transferable attention, whose weights are not detached (models.py:351-357, 379-388).
    // TA3N_FLAG_FRAME_ATTN (models.py:368-377, 612-614): the TRN reads F1a = (1 + wf) F1, wf from the frame discriminator's logits and not
    // detached - so that discriminator is live whatever place_adv[2] says, its logits come BEFORE the tuple products and its backward
    // AFTER the TRN input gradient (add_unfused_lists)
    // TA3N_FLAG_GENERAL_ATTN (models.py:320-325, 359-366, 379-388): w = softmax over the relations of attn_layer(R_j), a learned layer
    // (Wa1, ba1, wa2, ba2: always live) in place of the relation discriminators' entropy - those stay computed, and live only with their loss
    // TA3N_FLAG_UNSHARED (models.py:174-192, 296-305, 565-566, 686-687): the target rows have a first frame layer (Wsh_t, bsh_t) and a video
    // classifier (Wcv_t, bcv_t) of their own; everything between is one set of weights.  Five specs become a source and a target spec
    // each, cut at row Bs T / video Bs, in the launch the whole one sat in.  The first layer is live when some loss reads a target row
    // (any adversarial level, an entropy term, target labels), the classifier when some loss reads the target class logits (an entropy
    // term, target labels) - both with TA3N_FLAG_FEATURE_GRADS, where the caller assembles the loss
    const bool frame_attn, general_attn, unshared;
    const bool live_frm, live_vid, live_rel, mcd, feat_grads, bn_shared;
    const bool live_cv_t, live_sh_t;
    int64_t Wsh_t = -1, bsh_t = -1, Wcv_t = -1, bcv_t = -1;
    const int ldZ, ldR, ldF;
    int64_t o_F1a = -1, o_gF1a = -1, o_gFs = -1, o_gPfT = -1;   // frame attention: attended features, TRN input gradient, (1 + wf) gF1a, gPf + attention term
    int64_t o_Ua = -1, o_gUa = -1, o_gs = -1, Wa1 = -1, ba1 = -1, wa2 = -1, ba2 = -1;   // general attention: U / A = tanh(U), gradient at U, gradient at the scores; attn_layer.0 / .2
    HeadParams w;
    std::vector<int64_t> trnW, trnB, W1, B1, W2, B2;   // per scale j
    SharedStack st;
    int split_shared_fc = 0;    // (set for the fused step's first launch: ta3n_config.split_k bit 2)
    int split_f1_grad = 0;      // (set for the fused step's launches: ta3n_config.split_k)

    TrnModel(ta3n_plan &pl, const Dims &dm)
        : p(pl), b(pl), g(pl.geom), c(pl.cfg), d(dm), NR(dm.T - 1), NT(pl.n_tuples), frame_attn(c.flags & TA3N_FLAG_FRAME_ATTN),
          general_attn(c.flags & TA3N_FLAG_GENERAL_ATTN), unshared(c.flags & TA3N_FLAG_UNSHARED),
          live_frm(c.flags & (TA3N_FLAG_ADV_FRAME | TA3N_FLAG_FRAME_ATTN)),
          live_vid(c.flags & TA3N_FLAG_ADV_VIDEO), live_rel(c.flags & (TA3N_FLAG_ADV_RELATION | TA3N_FLAG_TRANS_ATTN)), mcd(c.flags & TA3N_FLAG_MCD),
          feat_grads(c.flags & TA3N_FLAG_FEATURE_GRADS), bn_shared(c.flags & TA3N_FLAG_BN_SHARED),
          live_cv_t(unshared && (c.flags & (TA3N_FLAG_ATTN_ENTROPY | TA3N_FLAG_TARGET_ENTROPY | TA3N_FLAG_TARGET_LABELS | TA3N_FLAG_FEATURE_GRADS))),
          live_sh_t(unshared && (live_cv_t || (c.flags & (TA3N_FLAG_ADV_RELATION | TA3N_FLAG_ADV_VIDEO | TA3N_FLAG_ADV_FRAME)))), ldZ(NT * dm.NB), ldR(NR * dm.NB), ldF(dm.T * dm.F) {}

    int tau(int t, int pos) const { return p.tuples[(size_t)t * d.T + pos]; }

    void add_params();
    void resolve_params();
    bool lay_out_workspace(std::string &err);
    void add_unfused_lists();
    void add_frame_attn_lists();
    void add_general_attn_lists();
    int64_t trn_input() const { return frame_attn ? o_F1a : g.o_F1; }   // what the tuple products and the TRN weight gradients read
    bool add_fused_step(std::string &err);
    void forward_levels(int group, const std::vector<Task> *side, std::string &cerr);
    std::vector<Task> update_side_tasks() const;

    // ---- GEMM specs (one per affine contraction of the step) ----
    GemmSpec spec_F1() const { return spec_shared_fc(d, w.Wsh, w.bsh, bn_shared ? g.o_Z0 : st.o_F[1], bn_shared, split_shared_fc); }
    GemmSpec spec_Hf() const { return spec_linear(d.BT, d.F, d.F, BASE_WS, g.o_F1, d.F, w.Wfd, w.bfd, g.o_Hf, d.F, true); }   // frame-discriminator hidden layer (models.py:458-459)
    GemmSpec spec_Pf() const { return spec_linear(d.BT, 2, d.F, BASE_WS, g.o_Hf, d.F, w.Wcd, w.bcd, g.o_Pf, 2, false); }      // frame domain logits (:460)
    GemmSpec spec_Y() const { return spec_linear(d.B, d.C, d.NB, BASE_WS, g.o_Vd, d.NB, w.Wcv, w.bcv, g.o_Y, d.C, false); }   // video classifier (:686)
    GemmSpec spec_Y2() const { return spec_linear(d.B, d.C, d.NB, BASE_WS, g.o_Vd, d.NB, w.Wcv2, w.bcv2, g.o_Y2, d.C, false); }   // ens_DA MCD: the second video classifier on the same feature (:717-718)
    GemmSpec spec_Hv() const { return spec_linear(d.B, d.NB, d.NB, BASE_WS, g.o_Vd, d.NB, w.Wdv, w.bdv, g.o_Hv, d.NB, true); }    // video-discriminator hidden layer (:466-467)
    GemmSpec spec_Pv() const { return spec_linear(d.B, 2, d.NB, BASE_WS, g.o_Hv, d.NB, w.Wcdv, w.bcdv, g.o_Pv, 2, false); }   // video domain logits (:468)
    GemmSpec spec_gHv() const { return spec_masked_back(d.B, d.NB, g.o_gPv, w.Wcdv, g.o_Hv, g.o_gHv); }   // gHv = (gPv Wcdv) * [Hv>0]
    GemmSpec spec_gHf() const { return spec_masked_back(d.BT, d.F, frame_attn ? o_gPfT : g.o_gPf, w.Wcd, g.o_Hf, g.o_gHf); }     // gHf = (gPf Wcd) * [Hf>0]
    GemmSpec spec_dWcd() const { return wgrad(2, d.F, d.BT, frame_attn ? o_gPfT : g.o_gPf, 2, g.o_Hf, d.F, w.Wcd, w.bcd); }              // dWcd = gPf^T Hf, dbcd
    GemmSpec wgrad(int M, int N, int K, int64_t g_off, int g_ld, int64_t x_off, int x_ld, int64_t dst, int64_t bias_dst) const {
        return spec_wgrad(M, N, K, g_off, g_ld, BASE_WS, x_off, x_ld, dst, bias_dst);
    }
    GemmSpec spec_Z(int t) const;
    GemmSpec spec_Hr(int j) const;
    GemmSpec spec_Ua(int j) const;
    GemmSpec spec_gR(int j) const;
    // ---- TA3N_FLAG_UNSHARED: the specs that exist once per domain (rows [0, Bs T) / videos [0, Bs): the source layer; the rest: the target's) ----
    void push_F1(std::vector<GemmSpec> &s) const {
        if (!unshared) { s.push_back(spec_F1()); return; }
        s.push_back(spec_shared_fc(d, w.Wsh, w.bsh, g.o_F1, false, 0, 0, d.Bs * d.T));
        s.push_back(spec_shared_fc(d, Wsh_t, bsh_t, g.o_F1, false, 0, d.Bs * d.T, d.Bt * d.T));
    }
    void push_Y(std::vector<GemmSpec> &s) const {
        if (!unshared) { s.push_back(spec_Y()); return; }
        s.push_back(spec_linear(d.Bs, d.C, d.NB, BASE_WS, g.o_Vd, d.NB, w.Wcv, w.bcv, g.o_Y, d.C, false));
        s.push_back(spec_linear(d.Bt, d.C, d.NB, BASE_WS, g.o_Vd + (int64_t)d.Bs * d.NB, d.NB, Wcv_t, bcv_t, g.o_Y + (int64_t)d.Bs * d.C, d.C, false));
    }
    void push_gVt(std::vector<GemmSpec> &s) const {
        if (!unshared) { s.push_back(spec_gVt(g, d.NB, w, true, mcd)); return; }
        s.push_back(spec_gVt(g, d.NB, w, true, false, 0, d.Bs, w.Wcv));
        s.push_back(spec_gVt(g, d.NB, w, true, false, d.Bs, d.Bt, Wcv_t));
    }
    void push_video_head_wgrads(std::vector<GemmSpec> &s) const {   // dWcdv, dbcdv, dWcv, dbcv
        s.push_back(wgrad(2, d.NB, d.B, g.o_gPv, 2, g.o_Hv, d.NB, w.Wcdv, w.bcdv));
        if (unshared) {   // K over the source videos into the source classifier's gradient, over the target videos into the target's (when it is live)
            s.push_back(wgrad(d.C, d.NB, d.Bs, g.o_gY, d.C, g.o_Vd, d.NB, w.Wcv, w.bcv));
            if (live_cv_t)
                s.push_back(wgrad(d.C, d.NB, d.Bt, g.o_gY + (int64_t)d.Bs * d.C, d.C, g.o_Vd + (int64_t)d.Bs * d.NB, d.NB, Wcv_t, bcv_t));
            return;
        }
        s.push_back(wgrad(d.C, d.NB, d.B, g.o_gY, d.C, g.o_Vd, d.NB, w.Wcv, w.bcv));
        if (mcd) s.push_back(wgrad(d.C, d.NB, d.B, g.o_gY2, d.C, g.o_Vd, d.NB, w.Wcv2, w.bcv2));
    }
    void push_video_disc_wgrads(std::vector<GemmSpec> &s) const { s.push_back(wgrad(d.NB, d.NB, d.B, g.o_gHv, d.NB, g.o_Vd, d.NB, w.Wdv, w.bdv)); }   // dWdv, dbdv
    void push_frame_disc_wgrads(std::vector<GemmSpec> &s) const { s.push_back(wgrad(d.F, d.F, d.BT, g.o_gHf, d.F, g.o_F1, d.F, w.Wfd, w.bfd)); }       // dWfd, dbfd
    void push_relation_level(std::vector<GemmSpec> &s) const {   // gR_j (+ fan-out to gZ), dW1_j, db1_j, dW2_j, db2_j
        const int NB = d.NB;
        for (int j = 0; j < NR; ++j) {
            s.push_back(spec_gR(j));
            s.push_back(wgrad(NB, NB, d.B, g.o_gHr + (int64_t)j * NB, ldR, g.o_R + (int64_t)j * NB, ldR, W1[j], B1[j]));
            s.push_back(wgrad(2, NB, d.B, g.o_gPrT + (int64_t)j * 2, NR * 2, g.o_Hr + (int64_t)j * NB, ldR, W2[j], B2[j]));
        }
        if (general_attn) {   // the attention layer, rows flat over (b, j): dWa1 = gUa^T R, dba1; dwa2 = gs^T A, dba2 = sum gs
            s.push_back(wgrad(NB, NB, d.B * NR, o_gUa, NB, g.o_R, NB, Wa1, ba1));
            s.push_back(wgrad(1, NB, d.B * NR, o_gs, 1, o_Ua, NB, wa2, ba2));
        }
    }
    void push_trn_wgrads(std::vector<GemmSpec> &s, unsigned scale_mask = ~0u) const;
    void push_f1_grad(std::vector<GemmSpec> &s) const;
    GemmSpec spec_gZ1_behind_frame_attn() const;
    void push_shared_fc_wgrad(std::vector<GemmSpec> &s) const {   // shared frame FC weight grad (no input gradient: the features are data); behind the BatchNorm with use_bn
        if (unshared) {   // dWsh_s = gZ1[0 : Bs T]^T X[0 : Bs T], dWsh_t over the other rows (when it is live), with their bias gradients
            const int rs = d.Bs * d.T;
            s.push_back(spec_wgrad(d.F, d.D, rs, g.o_gZ1, d.F, BASE_X, 0, d.D, w.Wsh, w.bsh));
            if (live_sh_t) s.push_back(spec_wgrad(d.F, d.D, d.Bt * d.T, g.o_gZ1 + (int64_t)rs * d.F, d.F, BASE_X, (int64_t)rs * d.D, d.D, Wsh_t, bsh_t));
            return;
        }
        s.push_back(spec_wgrad(d.F, d.D, d.BT, bn_shared ? g.o_gZ0 : st.o_gZ[1], d.F, BASE_X, 0, d.D, w.Wsh, w.bsh));   // + dbsh
    }
};

GemmSpec TrnModel::spec_Z(int t) const {   // TRN tuple GEMM (TRNmodule.py:60-79): gather+concat folded into the A-operand addressing
    const int j = p.scale_id[t], sl = p.scale_len[t], F = d.F, NB = d.NB;
    GemmSpec z;
    z.M = d.B; z.N = NB;
    z.affinity = 300 + j;               // the tuples of scale j read the same W_j
    for (int pos = 0; pos < sl; ++pos)
        z.segs.push_back(mkseg(KC(BASE_WS, trn_input() + (int64_t)tau(t, pos) * F, ldF),
                               KC(BASE_P, trnW[j] + (int64_t)pos * F, sl * F), F));
    z.proto = proto(BASE_WS, g.o_Zr + (int64_t)t * NB, ldZ);
    with_bias(z.proto, trnB[j]); z.proto.epi |= EPI_RELU;
    return z;
}

GemmSpec TrnModel::spec_Hr(int j) const {   // relation-discriminator hidden layer on R_j = sum_t Z_t (models.py:475-479)
    const int NB = d.NB;
    GemmSpec h;
    h.M = d.B; h.N = NB;
    for (int t = p.tuple_first[j]; t < p.tuple_first[j + 1]; ++t)
        h.segs.push_back(mkseg(KC(BASE_WS, g.o_Zr + (int64_t)t * NB, ldZ), KC(BASE_P, W1[j], NB), NB));
    h.proto = proto(BASE_WS, g.o_Hr + (int64_t)j * NB, ldR);
    with_bias(h.proto, B1[j]); h.proto.epi |= EPI_RELU;
    return h;
}

// relation-attention layer's first product on R_j = sum_t Z_t: U_j = Wa1 R_j + ba1 (models.py:321-322, 362), the K segments of spec_Hr(j)
GemmSpec TrnModel::spec_Ua(int j) const {
    const int NB = d.NB;
    GemmSpec u;
    u.M = d.B; u.N = NB;
    for (int t = p.tuple_first[j]; t < p.tuple_first[j + 1]; ++t)
        u.segs.push_back(mkseg(KC(BASE_WS, g.o_Zr + (int64_t)t * NB, ldZ), KC(BASE_P, Wa1, NB), NB));
    u.proto = proto(BASE_WS, o_Ua + (int64_t)j * NB, ldR);
    with_bias(u.proto, ba1);
    return u;
}

GemmSpec TrnModel::spec_gR(int j) const {   // gR_j = gRa_j - beta0 * gHr_j W1_j, fanned out through the TRN ReLU masks
    const int NB = d.NB;
    GemmSpec gr;
    gr.M = d.B; gr.N = NB;
    // (general attention: + gUa_j Wa1, a second K segment behind the scaled one - the scale then sits on the first Seg, as in push_f1_grad)
    gr.segs.push_back(mkseg(KC(BASE_WS, g.o_gHr + (int64_t)j * NB, ldR), KM(BASE_P, W1[j], NB), NB, general_attn ? SK_NEG_BETA_REL : SK_ONE));
    if (general_attn) gr.segs.push_back(mkseg(KC(BASE_WS, o_gUa + (int64_t)j * NB, ldR), KM(BASE_P, Wa1, NB), NB));
    gr.proto = proto(BASE_WS, g.o_gR + (int64_t)j * NB, ldR);
    gr.proto.alpha_kind = general_attn ? SK_ONE : SK_NEG_BETA_REL;
    with_add(gr.proto, g.o_gRa + (int64_t)j * NB, ldR);
    const int nt = p.tuple_first[j + 1] - p.tuple_first[j];
    gr.proto.fan_count = nt; gr.proto.fan_ld = ldZ;
    for (int k = 0; k < nt; ++k) {
        const int t = p.tuple_first[j] + k;
        gr.proto.fan_mask_off[k] = g.o_Zr + t * NB;
        gr.proto.fan_out_off[k] = g.o_gZ + t * NB;
    }
    return gr;
}

void TrnModel::push_trn_wgrads(std::vector<GemmSpec> &s, unsigned scale_mask) const {   // TRN weight (and bias) gradients of the scales in the mask
    const int F = d.F, NB = d.NB;
    for (int j = 0; j < NR; ++j) {
        if (!((scale_mask >> (j & 31)) & 1)) continue;
        const int sl = d.T - j;
        for (int pos = 0; pos < sl; ++pos) {   // dW_j[:, pos*F:(pos+1)*F] = sum_t gZ_t^T F1[:, tau_t[pos]]
            GemmSpec gw;
            gw.M = NB; gw.N = F;
            gw.affinity = 100 + j;      // every position of scale j reads the same gZ_t
            for (int t = p.tuple_first[j]; t < p.tuple_first[j + 1]; ++t)
                gw.segs.push_back(mkseg(KM(BASE_WS, g.o_gZ + (int64_t)t * NB, ldZ),
                                        KM(BASE_WS, trn_input() + (int64_t)tau(t, pos) * F, ldF), d.B));
            gw.proto = proto(BASE_G, trnW[j] + (int64_t)pos * F, sl * F);
            if (pos == 0) with_bias_grad(gw.proto, trnB[j]);   // db_j = sum_t column sums of gZ_t
            s.push_back(gw);
        }
    }
}

void TrnModel::push_f1_grad(std::vector<GemmSpec> &s) const {   // gradient at the frame features (TRN input gradient + frame discriminator's, reversed)
    const int F = d.F, NB = d.NB;
    for (int f = 0; f < d.T; ++f) {   // gZ1[:, f] = ( -beta2 gHf[:, f] Wfd + sum_{(t,pos): tau_t[pos]==f} gZ_t W_j[:, pos] ) * [F1>0] / keep
        GemmSpec gz;
        gz.M = d.B; gz.N = F;
        gz.affinity = 200 + f;          // the row panels of frame f read the same weight slabs (Wfd, W_j[:, pos] of every tuple that holds f)
        // (frame attention: the TRN input gradient alone, gF1a[:, f] = sum gZ_t W_j[:, pos] - the frame discriminator's share, the
        // ReLU / dropout mask and the attention scale follow behind PH_FRAME_ATTN_BWD: spec_gZ1_behind_frame_attn)
        if (!frame_attn) gz.segs.push_back(mkseg(KC(BASE_WS, g.o_gHf + (int64_t)f * F, ldF), KM(BASE_P, w.Wfd, F), F, SK_NEG_BETA_FRM));
        for (int t = 0; t < NT; ++t) {
            const int j = p.scale_id[t], sl = p.scale_len[t];
            for (int pos = 0; pos < sl; ++pos)
                if (tau(t, pos) == f)
                    gz.segs.push_back(mkseg(KC(BASE_WS, g.o_gZ + (int64_t)t * NB, ldZ),
                                            KM(BASE_P, trnW[j] + (int64_t)pos * F, sl * F), NB));
        }
        if (frame_attn) {
            gz.proto = proto(BASE_WS, o_gF1a + (int64_t)f * F, ldF);
            s.push_back(gz);
            continue;
        }
        gz.proto = proto(BASE_WS, g.o_gZ1 + (int64_t)f * F, ldF);
        with_mask(gz.proto, g.o_F1 + (int64_t)f * F, ldF);
        gz.proto.gamma_kind = SK_INV_KEEP_I;
        gz.split = split_f1_grad;
        s.push_back(gz);
    }
}

// frame attention: gZ1 = ( -beta2 gHf Wfd + (1 + wf) gF1a ) * [F1 > 0] / keep_i - the spec the avgpool model uses behind its pooling
GemmSpec TrnModel::spec_gZ1_behind_frame_attn() const {
    const int F = d.F;
    GemmSpec gz;
    gz.M = d.BT; gz.N = F;
    gz.segs.push_back(mkseg(KC(BASE_WS, g.o_gHf, F), KM(BASE_P, w.Wfd, F), F, SK_NEG_BETA_FRM));
    gz.proto = proto(BASE_WS, g.o_gZ1, F);
    with_add(gz.proto, o_gFs, F);
    with_mask(gz.proto, g.o_F1, F);
    gz.proto.gamma_kind = SK_INV_KEEP_I;
    return gz;
}

// ---- parameters: live first (they form the all-reduce / optimiser operand) ----
void TrnModel::add_params() {
    const int T = d.T, F = d.F, NB = d.NB, C = d.C;
    add_shared_fc_params(p, b, d);                                       // (--add_fc: updated by the first launch's side workgroups)
    if (unshared) b.lin("fc_feature_shared_target", F, d.D, live_sh_t);  // :175
    b.lin("fc_feature_domain", F, F, live_frm);                          // :161
    b.lin("fc_classifier_domain", 2, F, live_frm);                       // :170
    for (int j = 0; j < NR; ++j)                                         // TRNmodule.py:44-54
        b.add_linear("TRN.fc_fusion_scales." + std::to_string(j) + ".1", NB, (T - j) * F, true);
    for (int j = 0; j < NR; ++j) {                                       // models.py:286-294
        b.lin("relation_domain_classifier_all." + std::to_string(j) + ".0", NB, NB, live_rel);
        b.lin("relation_domain_classifier_all." + std::to_string(j) + ".2", 2, NB, live_rel);
    }
    b.lin("fc_feature_domain_video", NB, NB, live_vid);                  // :267
    b.add_linear("fc_classifier_video_source", C, NB, true);             // :272
    if (unshared) b.lin("fc_classifier_video_target", C, NB, live_cv_t); // :303
    if (bn_shared) add_bn_shared_params(b, F);
    if (mcd) b.add_linear("fc_classifier_video_source_2", C, NB, true);  // :276-279 (ens_DA MCD)
    b.lin("fc_classifier_domain_video", 2, NB, live_vid);                // :281
    if (general_attn) {                                                  // :320-325 (last in the reference's state_dict; here: inside the live prefix)
        b.add_linear("attn_layer.0", NB, NB, true);
        b.add_linear("attn_layer.2", 1, NB, true);
    }
    p.live_floats = p.param_floats;
    b.add_dead_linears();                                                // computed (zero or unused) gradients land past the live prefix
    // never receive a gradient in this configuration: kept for state_dict compatibility
    b.add_linear("fc_feature_source", F, F, false);                      // :156
    b.add_linear("fc_classifier_source", C, F, false);                   // :166 (dead for baseline_type 'video')
    b.add_param("bn_trn_S.weight", NB, 0, false); b.add_param("bn_trn_S.bias", NB, 0, false);   // :225-226
    b.add_param("bn_trn_T.weight", NB, 0, false); b.add_param("bn_trn_T.bias", NB, 0, false);
    b.add_linear("fc_feature_video_source", NB, NB, false);              // :258
    b.add_linear("fc_feature_video_source_2", NB, NB, false);            // :262
    if (unshared) {                                                      // computed by the reference (fc_classifier_target, :618) or not at all: feed no loss
        b.add_linear("fc_feature_target", F, F, false);                  // :187
        b.add_linear("fc_classifier_target", C, F, false);               // :190
        b.add_linear("fc_feature_video_target", NB, NB, false);          // :297
        b.add_linear("fc_feature_video_target_2", NB, NB, false);        // :300
        Wsh_t = p.poff("fc_feature_shared_target.weight"); bsh_t = p.poff("fc_feature_shared_target.bias");
        Wcv_t = p.poff("fc_classifier_video_target.weight"); bcv_t = p.poff("fc_classifier_video_target.bias");
    }
    resolve_params();
}

// the offsets the spec builders address, from the parameter table (add_params' own, or - TA3N_FLAG_SCORE_ONLY - the training plan's)
void TrnModel::resolve_params() {
    w = head_params(p, mcd);
    for (int j = 0; j < NR; ++j) {
        const std::string trn = "TRN.fc_fusion_scales." + std::to_string(j) + ".1", rel = "relation_domain_classifier_all." + std::to_string(j);
        trnW.push_back(p.poff(trn + ".weight")); trnB.push_back(p.poff(trn + ".bias"));
        W1.push_back(p.poff(rel + ".0.weight")); B1.push_back(p.poff(rel + ".0.bias"));
        W2.push_back(p.poff(rel + ".2.weight")); B2.push_back(p.poff(rel + ".2.bias"));
    }
    if (general_attn) {
        Wa1 = p.poff("attn_layer.0.weight"); ba1 = p.poff("attn_layer.0.bias");
        wa2 = p.poff("attn_layer.2.weight"); ba2 = p.poff("attn_layer.2.bias");
    }
}

// ---- workspace ----
bool TrnModel::lay_out_workspace(std::string &err) {
    const int B = d.B, BT = d.BT, F = d.F, NB = d.NB, C = d.C;
    init_geom(g, d, NB, c.flags);
    g.n_tuples = NT; g.n_rel = NR;
    g.o_F1 = (int32_t)b.add_region("F1", (int64_t)BT * F);
    g.o_Hf = (int32_t)b.add_region("Hf", (int64_t)BT * F);
    g.o_Pf = (int32_t)b.add_region("Pf", (int64_t)BT * 2);
    g.o_Zr = (int32_t)b.add_region("Zr", (int64_t)B * NT * NB);
    g.o_Hr = (int32_t)b.add_region("Hr", (int64_t)B * NR * NB);
    g.o_Pr = (int32_t)b.add_region("Pr", (int64_t)B * NR * 2);
    g.o_R = (int32_t)b.add_region("R", (int64_t)B * NR * NB);
    g.o_attn = (int32_t)b.add_region("attn", (int64_t)B * NR);
    g.o_V = (int32_t)b.add_region("V", (int64_t)B * NB);
    g.o_Vd = (int32_t)b.add_region("Vd", (int64_t)B * NB);
    g.o_Y = (int32_t)b.add_region("Y", (int64_t)B * C);
    g.o_Hv = (int32_t)b.add_region("Hv", (int64_t)B * NB);
    g.o_Pv = (int32_t)b.add_region("Pv", (int64_t)B * 2);
    g.o_gY = (int32_t)b.add_region("gY", (int64_t)B * C);
    g.o_gPv = (int32_t)b.add_region("gPv", (int64_t)B * 2);
    g.o_gPr = (int32_t)b.add_region("gPr", (int64_t)B * NR * 2);
    g.o_gPf = (int32_t)b.add_region("gPf", (int64_t)BT * 2);
    g.o_gattn = (int32_t)b.add_region("g_attn", (int64_t)B * NR);
    g.o_gHv = (int32_t)b.add_region("gHv", (int64_t)B * NB);
    g.o_gHf = (int32_t)b.add_region("gHf", (int64_t)BT * F);
    g.o_gVt = (int32_t)b.add_region("gVt", (int64_t)B * NB);
    g.o_gPrT = (int32_t)b.add_region("gPrT", (int64_t)B * NR * 2);
    g.o_gRa = (int32_t)b.add_region("gRa", (int64_t)B * NR * NB);
    g.o_gHr = (int32_t)b.add_region("gHr", (int64_t)B * NR * NB);
    g.o_gR = (int32_t)b.add_region("gR", (int64_t)B * NR * NB);
    g.o_gZ = (int32_t)b.add_region("gZ", (int64_t)B * NT * NB);
    g.o_gZ1 = (int32_t)b.add_region("gZ1", (int64_t)BT * F);
    lay_out_stack(p, b, st, BT, F, g.o_F1, g.o_gZ1);
    if (feat_grads) g.o_gV_ext = (int32_t)b.add_region("gV_ext", (int64_t)B * NB);
    if (bn_shared) add_bn_regions(p, b, g, d);
    if (mcd) add_mcd_regions(b, g, d);
    if (frame_attn) {
        o_F1a = b.add_region("F1a", (int64_t)BT * F);
        const int64_t o_attn = b.add_region("attn_frame", BT);
        o_gF1a = b.add_region("gF1a", (int64_t)BT * F);
        o_gPfT = b.add_region("gPfT", (int64_t)BT * 2);
        // (1 + wf) gF1a, the additive base of the gradient at F1: in gRa - free once the relation level has read it - when it fits
        o_gFs = (int64_t)B * NR * NB >= (int64_t)BT * F ? (int64_t)g.o_gRa : b.add_region("gF1s", (int64_t)BT * F);
        p.frame_attn = {(int32_t)o_F1a, (int32_t)o_attn, (int32_t)o_gF1a, (int32_t)o_gFs, (int32_t)o_gPfT};
    }
    if (general_attn) {
        o_Ua = b.add_region("Ua", (int64_t)B * NR * NB);      // U from the GEMM launch, A = tanh(U) in place from the attention launch
        o_gUa = b.add_region("gUa", (int64_t)B * NR * NB);
        o_gs = b.add_region("gs", (int64_t)B * NR);
        p.general_attn = {(int32_t)o_Ua, (int32_t)o_gUa, (int32_t)o_gs, (int32_t)wa2, (int32_t)ba2};
    }
#ifdef TA3N_GEMM_STAMPS
    b.add_region("stamps", 8192 * 16 * 2);            // (debug build: per-workgroup cycle stamps of the GEMM launches, directly in front of "zeros")
#endif
    if (!add_tail_begin(b, g, d, NR + 1, err)) return false;
    // Videos per video workgroup (ta3n_heads.hip; TA3N_HEADS_VPW in the environment forces 1 / 2 for A/B runs).  A video workgroup owns
    // its compute unit, so what matters is how many ROUNDS the launch needs and how long a workgroup lives - and a workgroup's life is
    // dominated by the relation stages, whose per-wave chain grows with the relations a wave handles.  Measured (profiles/r04_heads_vpw_ab.txt):
    // 128+128 videos x 12 segments (configs[4]): 2 per workgroup turns 1.2 rounds into one, launch 40.6 -> 29.1 us, two-stream step 477 -> 470;
    // 512+512 x 9 (configs[3]): the video workgroups alone fill the chip whatever the packing - 4 per workgroup 79.5 -> 79.5 us on one box and
    // +40 us per step on another, 2 per workgroup -7 us on the launch and +6 on the step: left at one; 128+74 x 5 (headline): 2 per
    // workgroup 15.5 -> 20.1 us (every video has a compute unit already).
    // Round 5: with the relation loops pipelined (heads_kernel PIPE: a wave requests its next relation's operands while it reduces the current
    // one) a wave that handles twice the relations no longer takes twice as long: 512+512 x 9 on two videos per workgroup 81.0 -> 65.8 us on
    // the launch, 0.457 -> 0.441 ms on the step (two alternating repeats, profiles/r05_heads_vpw_tune.txt) - two per workgroup from 225 videos up.
    g.heads_vpw = B > 224 ? 2 : 1;
    // (A/B override: 1 or 2.  Four per workgroup - never a plan's choice - faulted on the round-5 build at 512+512 x 9 ("memory access fault",
    // gpurun_out of call 5) and is no longer accepted; the kernel template keeps the case.)
    if (const char *e = std::getenv("TA3N_HEADS_VPW")) { const int v = std::atoi(e); if (v == 1 || v == 2) g.heads_vpw = v; }
    g.n_vid_wg = (B + g.heads_vpw - 1) / g.heads_vpw;
    g.heads_rpw = HEADS_RPW;      // all workgroups of the heads kernel resident at once if the chip (256 CUs) can hold them
    while (g.n_vid_wg + (BT + g.heads_rpw - 1) / g.heads_rpw > 256 && g.heads_rpw < 8 * HEADS_RPW) g.heads_rpw *= 2;
    g.n_frm_wg = (BT + g.heads_rpw - 1) / g.heads_rpw;
    g.o_fh_part = (int32_t)b.add_region("fh_part", (int64_t)g.n_frm_wg * 2 * F);
    g.o_fh_bpart = (int32_t)b.add_region("fh_bpart", (int64_t)g.n_frm_wg * 2);
    add_tail_end(p, b, g, d, (int64_t)(g.n_vid_wg + g.n_frm_wg) * 8, w);
    g.p_Wcd = (int32_t)w.Wcd; g.p_bcd = (int32_t)w.bcd; g.p_Wdv = (int32_t)w.Wdv; g.p_bdv = (int32_t)w.bdv;
    g.p_Wcdv = (int32_t)w.Wcdv; g.p_bcdv = (int32_t)w.bcdv;
    g.p_W2_0 = (int32_t)W2[0]; g.p_b2_0 = (int32_t)B2[0];
    g.p_W2_stride = NR > 1 ? (int32_t)(W2[1] - W2[0]) : 0;
    g.p_b2_stride = NR > 1 ? (int32_t)(B2[1] - B2[0]) : 0;
    return workspace_fits(p, err);
}

// ---- the unfused lists: forward (group 0), loss (1), backward (2), optimiser (3) ----
void TrnModel::add_unfused_lists() {
    const int BT = d.BT, F = d.F;
    if (frame_attn) { add_frame_attn_lists(); return; }
    if (general_attn) { add_general_attn_lists(); return; }
    { std::vector<GemmSpec> s; push_F1(s); b.add_gemm_phase(0, s); }
    if (bn_shared) b.add_simple_phase(PH_BN_FWD, 0);
    add_stack_forward(b, st, 0, BT, F);
    {   // F2
        std::vector<GemmSpec> s{spec_Hf()};
        for (int t = 0; t < NT; ++t) s.push_back(spec_Z(t));
        b.add_gemm_phase(0, s);
    }
    {   // F3
        std::vector<GemmSpec> s;
        for (int j = 0; j < NR; ++j) s.push_back(spec_Hr(j));
        s.push_back(spec_Pf());
        b.add_gemm_phase(0, s);
    }
    b.add_simple_phase(PH_POOL_FWD, 0);   // Pr, attention weights, R, V, Vd
    { std::vector<GemmSpec> s; push_Y(s); s.push_back(spec_Hv()); if (mcd) s.push_back(spec_Y2()); b.add_gemm_phase(0, s); }   // F6
    b.add_gemm_phase(0, spec_Pv());       // F7
    b.add_simple_phase(PH_LOSS, 1);
    {   // Q1: heads that depend only on the logit gradients
        std::vector<GemmSpec> s{spec_gHv(), spec_gHf()};
        push_video_head_wgrads(s);
        s.push_back(spec_dWcd());
        b.add_gemm_phase(2, s);
    }
    {   // Q2: gradient at the pooled video feature + first-layer weight grads of the video/frame discriminators
        std::vector<GemmSpec> s;
        push_gVt(s);
        push_video_disc_wgrads(s);
        push_frame_disc_wgrads(s);
        b.add_gemm_phase(2, s);
    }
    b.add_simple_phase(PH_POOL_BWD, 2);   // gPrT (attention path), gRa = (1+w) gVt, gHr
    { std::vector<GemmSpec> s; push_relation_level(s); b.add_gemm_phase(2, s); }                       // Q5
    { std::vector<GemmSpec> s; push_trn_wgrads(s); push_f1_grad(s); b.add_gemm_phase(2, s); }          // Q6
    add_stack_backward(b, st, 2, BT, F);
    if (bn_shared) b.add_simple_phase(PH_BN_BWD, 2);
    { std::vector<GemmSpec> s; push_shared_fc_wgrad(s); b.add_gemm_phase(2, s); }                      // Q7
    b.add_simple_phase(PH_GRAD_NORM, 3);
    b.add_simple_phase(PH_SGD, 3);
}

// TA3N_FLAG_FRAME_ATTN: the same lists re-ordered around the two frame-attention launches.  Forward: the frame discriminator runs to
// its logits before the tuple products (which read F1a); backward: its two layers follow the TRN input gradient, whose inner product
// with F1 is the gradient at the attention weight.  Two more GEMM launches in the forward (Hf and Pf no longer share a launch with
// the tuples / Hr), two more in the backward, and the two pointwise launches.
void TrnModel::add_frame_attn_lists() {
    b.add_gemm_phase(0, spec_F1());
    b.add_gemm_phase(0, spec_Hf());
    b.add_gemm_phase(0, spec_Pf());
    b.add_simple_phase(PH_FRAME_ATTN_FWD, 0);   // attn_frame, F1a (+ its twin)
    { std::vector<GemmSpec> s; for (int t = 0; t < NT; ++t) s.push_back(spec_Z(t)); b.add_gemm_phase(0, s); }
    { std::vector<GemmSpec> s; for (int j = 0; j < NR; ++j) s.push_back(spec_Hr(j)); b.add_gemm_phase(0, s); }
    b.add_simple_phase(PH_POOL_FWD, 0);
    { std::vector<GemmSpec> s{spec_Y(), spec_Hv()}; b.add_gemm_phase(0, s); }
    b.add_gemm_phase(0, spec_Pv());
    b.add_simple_phase(PH_LOSS, 1);
    { std::vector<GemmSpec> s{spec_gHv()}; push_video_head_wgrads(s); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s{spec_gVt(g, d.NB, w, true, false)}; push_video_disc_wgrads(s); b.add_gemm_phase(2, s); }
    b.add_simple_phase(PH_POOL_BWD, 2);
    { std::vector<GemmSpec> s; push_relation_level(s); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s; push_trn_wgrads(s); push_f1_grad(s); b.add_gemm_phase(2, s); }          // TRN weight gradients (on F1a), gF1a
    b.add_simple_phase(PH_FRAME_ATTN_BWD, 2);   // gPfT, (1 + wf) gF1a
    { std::vector<GemmSpec> s{spec_gHf(), spec_dWcd()}; b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s; push_frame_disc_wgrads(s); s.push_back(spec_gZ1_behind_frame_attn()); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s; push_shared_fc_wgrad(s); b.add_gemm_phase(2, s); }
    b.add_simple_phase(PH_GRAD_NORM, 3);
    b.add_simple_phase(PH_SGD, 3);
}

// TA3N_FLAG_GENERAL_ATTN: the plain lists (add_fc 1, no BatchNorm, no MCD: general_attn_refusal) in their order, with U_j = Wa1 R_j + ba1
// riding in the launch of Hr_j and Pf, the general-attention launches in place of the two pooling launches, and the relation-level
// launch carrying gUa_j Wa1 in gR_j and the attention layer's two weight gradients (push_relation_level).  No launch more than the
// plain lists have.
void TrnModel::add_general_attn_lists() {
    b.add_gemm_phase(0, spec_F1());
    { std::vector<GemmSpec> s{spec_Hf()}; for (int t = 0; t < NT; ++t) s.push_back(spec_Z(t)); b.add_gemm_phase(0, s); }
    {
        std::vector<GemmSpec> s;
        for (int j = 0; j < NR; ++j) s.push_back(spec_Hr(j));
        s.push_back(spec_Pf());
        for (int j = 0; j < NR; ++j) s.push_back(spec_Ua(j));
        b.add_gemm_phase(0, s);
    }
    b.add_simple_phase(PH_GENERAL_ATTN_FWD, 0);   // Pr, R, A, attention weights, V, Vd
    { std::vector<GemmSpec> s{spec_Y(), spec_Hv()}; b.add_gemm_phase(0, s); }
    b.add_gemm_phase(0, spec_Pv());
    b.add_simple_phase(PH_LOSS, 1);
    { std::vector<GemmSpec> s{spec_gHv(), spec_gHf()}; push_video_head_wgrads(s); s.push_back(spec_dWcd()); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s{spec_gVt(g, d.NB, w, true, false)}; push_video_disc_wgrads(s); push_frame_disc_wgrads(s); b.add_gemm_phase(2, s); }
    b.add_simple_phase(PH_GENERAL_ATTN_BWD, 2);   // gs, gUa, gRa = (1 + w) gv, gPrT = gPr, gHr
    { std::vector<GemmSpec> s; push_relation_level(s); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s; push_trn_wgrads(s); push_f1_grad(s); b.add_gemm_phase(2, s); }
    { std::vector<GemmSpec> s; push_shared_fc_wgrad(s); b.add_gemm_phase(2, s); }
    b.add_simple_phase(PH_GRAD_NORM, 3);
    b.add_simple_phase(PH_SGD, 3);
}

// chain: the three forward GEMM levels are ONE launch (tile-level hand-offs inside it, Builder::end_chain), likewise the
// last two backward levels: 5 launches per step instead of 8 (north_star's "gather+concat and the
// relation MLP as one grouped GEMM launch")
void TrnModel::forward_levels(int group, const std::vector<Task> *side, std::string &cerr) {
    const bool chain = c.chain != 0;
    if (chain) b.begin_chain();
    b.add_gemm_phase(group, spec_F1());
    if (side) {
        if (chain) b.chain_append(*side);
        else { for (auto &t : *side) p.tasks.push_back(t); p.phases.back().task_count += (int32_t)side->size(); }
    }
    if (!chain && group == 5) return;      // unchained: the pipelined variant only mirrors the first launch
    if (bn_shared) b.add_simple_phase(PH_BN_FWD, group);      // F1 = dropout_i(relu(BatchNorm_domain(Z0))), batch statistics
    add_stack_forward(b, st, group, d.BT, d.F);      // --add_fc: behind the first launch, whose side workgroups update W_2 / W_3
    {
        std::vector<GemmSpec> s{spec_Hf()};
        for (int t = 0; t < NT; ++t) s.push_back(spec_Z(t));
        b.add_gemm_phase(group, s);
    }
    {
        std::vector<GemmSpec> s;
        for (int j = 0; j < NR; ++j) s.push_back(spec_Hr(j));
        b.add_gemm_phase(group, s);
    }
    if (chain) { const std::string e = b.end_chain(); if (!e.empty()) cerr = e; }
}

// the PREVIOUS step's optimiser update of every parameter the step's first launch does not read itself (all but the shared
// frame FC), as EPI_SGD side tasks of that launch (ta3n_train_step_after_update)
std::vector<Task> TrnModel::update_side_tasks() const {
    const int64_t i0 = p.first_floats / 4, i1 = p.live_floats / 4;
    const int n_side = 256;
    const int64_t per = (i1 - i0 + n_side - 1) / n_side;
    std::vector<Task> side;
    for (int k = 0; k < n_side; ++k) {
        Task t;
        std::memset(&t, 0, sizeof(t));
        t.epi = EPI_SGD;
        t.sig = -1;
        t.c_base = BASE_NONE; t.bias_base = BASE_NONE; t.aux_base = BASE_NONE; t.add_base = BASE_NONE;
        t.pad[0] = (int32_t)std::min(i0 + per * k, i1);
        t.pad[1] = (int32_t)std::min(i0 + per * (k + 1), i1);
        side.push_back(t);
    }
    return side;
}

// ---- fused forward + loss + backward (group 4, ta3n_train_step), the group-5 mirror of its first launch, and the twins ----
// Same arithmetic in 7 launches instead of 15: everything between (Hr, Hf) and (gHr, gHf) - both
// discriminator heads, the attention pooling, the classifier, the losses and their backward - is one
// kernel (ta3n_heads.hip); its small weight gradients ride along with the relation level.
bool TrnModel::add_fused_step(std::string &err) {
    const int B = d.B, BT = d.BT, F = d.F, NB = d.NB;
    const bool chain = c.chain != 0;
    const bool twins = stored_twins(c);
    std::string cerr;
    split_shared_fc = ((c.split_k & 4) && !chain && !bn_shared) ? 1 : 0;
    forward_levels(4, nullptr, cerr);
    b.add_simple_phase(PH_HEADS, 4);
    b.sum8_pending(g.o_losses, g.o_loss_part, g.n_vid_wg + g.n_frm_wg);   // logging scalars
    {
        std::vector<GemmSpec> s;
        push_relation_level(s);
        push_video_head_wgrads(s);
        push_video_disc_wgrads(s);
        // dWcd, dbcd = sums over the frame workgroups of their partial sums: exact fp32 column sums in a fixed order
        b.colsum_pending(g.o_fh_part, g.n_frm_wg, 2 * F, 2 * F, w.Wcd);
        b.colsum_pending(g.o_fh_bpart, g.n_frm_wg, 2, 2, w.bcd);
        // dWfd: gHf is ready after the heads kernel, so it can fill the CUs this short level leaves idle - unless the
        // next launch reads bf16 twins and this one cannot (odd-shaped head gradients): then it is cheaper there
        if (!twins) push_frame_disc_wgrads(s);
        b.add_gemm_phase(4, s);
    }
    // The critical path of the backward pass is  relation level -> gradient at F1 -> shared-FC weight gradient; the TRN
    // weight gradients and dWfd feed nothing but the optimiser, so they may ride with either of the last two launches
    // (ta3n_config.wgrads_late, default 0 = with the gradient at F1: measured faster at the headline shape, ta3n_hip.h).
    // wgrads_late: 0 = all with the gradient at F1, 1 = all with the shared-FC weight gradient, otherwise a mask:
    // bit 1 = the frame discriminator's first layer, bit 2 + j = TRN scale j (j = 0: all T frames)
    const unsigned late_mask = c.wgrads_late == 0 ? 0u : c.wgrads_late == 1 ? ~0u : (unsigned)c.wgrads_late;
    const bool late_fd = (late_mask >> 1) & 1;
    const unsigned late_trn = late_mask >> 2;
    if (chain) b.begin_chain();
    split_f1_grad = ((c.split_k & 2) && !chain) ? 2 : 0;
    {
        std::vector<GemmSpec> s;
        if (chain) {      // one launch: the tiles everything else waits for (the gradient at F1) are dispatched first
            push_f1_grad(s);
            if (twins && !late_fd) push_frame_disc_wgrads(s);
            push_trn_wgrads(s, ~late_trn);
        } else {
            if (twins && !late_fd) push_frame_disc_wgrads(s);
            push_trn_wgrads(s, ~late_trn);
            push_f1_grad(s);
        }
        b.add_gemm_phase(4, s);
    }
    add_stack_backward(b, st, 4, BT, F);
    if (bn_shared) b.add_simple_phase(PH_BN_BWD, 4);      // gZ0 + the BatchNorm weight / bias gradients from gZ1
    {
        std::vector<GemmSpec> s;
        push_shared_fc_wgrad(s);
        push_trn_wgrads(s, late_trn);
        if (twins && late_fd) push_frame_disc_wgrads(s);
        b.add_gemm_phase(4, s);
    }
    if (chain) { const std::string e = b.end_chain(); if (!e.empty()) cerr = e; }
    {   // group 5: the step's first launch once more, carrying the previous step's optimiser update
        const Phase *f1 = nullptr;
        for (const Phase &ph : p.phases)
            if (ph.group == 4 && ph.kind == PH_GEMM) { f1 = &ph; break; }
        b.force_next = tile_code_mirroring(*f1);
        const std::vector<Task> side = update_side_tasks();
        forward_levels(5, &side, cerr);
    }
    if (!cerr.empty()) { err = cerr; return false; }
    assign_sumsq_slots(p, b, g, bn_sumsq_slots(bn_shared, F));
    // (the heads kernel keeps the twin of gHf; gZ and gZ1 are read by GEMM launches only: twin-only when those read twins.
    // use_bn: the BatchNorm launches keep the twins of what they produce - F1 and gZ0 - and READ gZ1 in fp32)
    std::vector<Span> kept{Span{g.o_gHf, g.o_gHf + (int64_t)BT * F}};
    std::vector<Span> gemm_only{Span{g.o_gZ, g.o_gZ + (int64_t)B * NT * NB}};
    if (bn_shared) {
        kept.push_back(Span{g.o_F1, g.o_F1 + (int64_t)BT * F});
        kept.push_back(Span{g.o_gZ0, g.o_gZ0 + (int64_t)BT * F});
    } else {
        gemm_only.push_back(Span{g.o_gZ1, g.o_gZ1 + (int64_t)BT * F});
        for (int k = 1; k < st.L; ++k) gemm_only.push_back(Span{st.o_gZ[k], st.o_gZ[k] + (int64_t)BT * F});   // (--add_fc)
    }
    add_bf16_twins(p, b, g, BT, d.D, kept, gemm_only);
    return true;
}

// "" when the configuration's frame attention is built, otherwise the refusal (naming the combination)
std::string frame_attn_refusal(const ta3n_config &c) {
    if (!(c.flags & TA3N_FLAG_FRAME_ATTN)) return "";
    const std::string what = "use_attn_frame TransAttn (TA3N_FLAG_FRAME_ATTN)";
    if (c.aggregation != TA3N_AGG_TRN_M) return what + " on avgpool is not built: frame attention feeds the TRN of trn-m";
    if (!(c.flags & TA3N_FLAG_TRANS_ATTN))
        return what + " needs use_attn TransAttn (TA3N_FLAG_TRANS_ATTN): the reference takes the kind of frame attention from use_attn "
               "(models.py:369-372) and fails with use_attn none";
    const char *with = nullptr;
    if (c.flags & TA3N_FLAG_F32_SPLIT) with = "TA3N_FLAG_F32_SPLIT";
    else if (c.flags & TA3N_FLAG_MCD) with = "ens_DA MCD (TA3N_FLAG_MCD)";
    else if (c.flags & TA3N_FLAG_BN_SHARED) with = "use_bn (TA3N_FLAG_BN_SHARED)";
    else if (c.shared_fc_layers > 1) with = "shared_fc_layers (--add_fc) > 1";
    else if (c.chain) with = "chain";
    else if (c.split_k) with = "split_k";
    else if (c.wgrads_late) with = "wgrads_late";
    return with ? what + " with " + with + " is not built" : "";
}

// "" when the configuration's general attention is built, otherwise the refusal (naming the combination)
std::string general_attn_refusal(const ta3n_config &c) {
    if (!(c.flags & TA3N_FLAG_GENERAL_ATTN)) return "";
    const std::string what = "use_attn general (TA3N_FLAG_GENERAL_ATTN)";
    if (c.aggregation != TA3N_AGG_TRN_M) return what + " on avgpool is not built: the reference's aggregate_frames ignores use_attn there";
    const char *with = nullptr;
    if (c.flags & TA3N_FLAG_TRANS_ATTN) with = "use_attn TransAttn (TA3N_FLAG_TRANS_ATTN): two values of one option";
    else if (c.flags & TA3N_FLAG_FRAME_ATTN) with = "use_attn_frame (TA3N_FLAG_FRAME_ATTN): the reference sends 'general' frame attention to a 256-wide layer on fc_dim-wide rows";
    else if (c.flags & TA3N_FLAG_F32_SPLIT) with = "TA3N_FLAG_F32_SPLIT";
    else if (c.flags & TA3N_FLAG_MCD) with = "ens_DA MCD (TA3N_FLAG_MCD)";
    else if (c.flags & TA3N_FLAG_BN_SHARED) with = "use_bn (TA3N_FLAG_BN_SHARED)";
    else if (c.shared_fc_layers > 1) with = "shared_fc_layers (--add_fc) > 1";
    else if (c.chain) with = "chain";
    else if (c.split_k) with = "split_k";
    else if (c.wgrads_late) with = "wgrads_late";
    else
        for (int i = 0; i < 16; ++i)
            if (c.phase_tiles[i]) with = "phase_tiles (indexed by the plain launch order)";
    return with ? what + " with " + with + " is not built" : "";
}

// "" when the configuration's unshared target layers are built, otherwise the refusal (naming the combination)
std::string share_params_refusal(const ta3n_config &c) {
    if (!(c.flags & TA3N_FLAG_UNSHARED)) return "";
    const std::string what = "share_params N (TA3N_FLAG_UNSHARED)";
    if (c.aggregation != TA3N_AGG_TRN_M) return what + " on avgpool is not built: the unshared target layers are built on the unfused trn-m lists";
    if (c.batch_source <= 0 || c.batch_target <= 0)
        return what + " with batch_source == 0 or batch_target == 0 is not built: each domain's layers need rows of their own";
    const char *with = nullptr;
    if (c.flags & TA3N_FLAG_MCD) with = "ens_DA MCD (TA3N_FLAG_MCD)";
    else if (c.flags & TA3N_FLAG_BN_SHARED) with = "use_bn (TA3N_FLAG_BN_SHARED)";
    else if (c.flags & TA3N_FLAG_FRAME_ATTN) with = "use_attn_frame (TA3N_FLAG_FRAME_ATTN)";
    else if (c.flags & TA3N_FLAG_GENERAL_ATTN) with = "use_attn general (TA3N_FLAG_GENERAL_ATTN)";
    else if (c.flags & TA3N_FLAG_F32_SPLIT) with = "TA3N_FLAG_F32_SPLIT";
    else if (c.shared_fc_layers > 1) with = "shared_fc_layers (--add_fc) > 1";
    else if (c.chain) with = "chain";
    else if (c.split_k) with = "split_k";
    else if (c.wgrads_late) with = "wgrads_late";
    else
        for (int i = 0; i < 16; ++i)
            if (c.phase_tiles[i]) with = "phase_tiles (indexed by the plain launch order)";
    return with ? what + " with " + with + " is not built" : "";
}

int build_plan_trn(ta3n_plan &p, std::string &err) {
    const Dims d = dims_of(p.cfg);
    if (const char *e = bn_shared_refusal(p.cfg, d)) { err = e; return TA3N_ERR_INVALID; }
    // ---- relation tuples ----
    const int T = d.T, NR = T - 1;
    p.n_tuples = ta3n_num_relation_tuples(T);
    p.tuples.assign((size_t)p.n_tuples * T, -1);
    p.scale_len.assign(p.n_tuples, 0);
    p.scale_id.assign(p.n_tuples, 0);
    ta3n_relation_table(T, p.tuples.data(), p.scale_len.data(), p.scale_id.data());
    p.tuple_first.assign(NR + 1, 0);
    for (int t = 0; t < p.n_tuples; ++t) p.tuple_first[p.scale_id[t] + 1] = t + 1;
    for (int j = 1; j <= NR; ++j) p.tuple_first[j] = std::max(p.tuple_first[j], p.tuple_first[j - 1]);

    TrnModel m(p, d);
    m.add_params();
    if (!m.lay_out_workspace(err)) return TA3N_ERR_INVALID;
    m.add_unfused_lists();
    // (The fused heads kernel knows neither the second classifier nor an outside gradient.  use_bn - round 6 - IS part of the fused
    // step: the two BatchNorm launches sit where the unfused lists have them, behind the shared-FC product and in front of its weight
    // gradient: 10 launches instead of 17, models.py:490-543, 569-570; chained launches stay without it.)
    if (m.frame_attn) {
        // frame attention: the unfused lists only (the fused heads kernel computes Pf behind the tuple products); the frame-attention
        // launch keeps the twin of F1a, which the tuple products and the TRN weight gradients read
        add_bf16_twins(p, m.b, m.g, d.BT, d.D, {}, {}, {Span{m.o_F1a, m.o_F1a + (int64_t)d.BT * d.F}});
    } else if (m.general_attn) {
        // general attention: the unfused lists only (the fused heads kernel computes the entropy attention); its two launches keep no twin -
        // what they write (R, A, gUa, gRa, gHr, gs) is read by the relation-level launch, which reads no twins in the plain lists either
        add_bf16_twins(p, m.b, m.g, d.BT, d.D, {}, {});
    } else if (heads_supported(d.NB, d.C, d.F) && !m.mcd && !m.feat_grads && !m.unshared && !(m.bn_shared && p.cfg.chain != 0)) {
        if (!m.add_fused_step(err)) return TA3N_ERR_INVALID;
    } else {
        // no fused step (TA3N_FLAG_FEATURE_GRADS: dis_DA DAN / JAN put a gradient between forward and backward; TA3N_FLAG_MCD; TA3N_FLAG_UNSHARED:
        // the heads kernel keeps one classifier per workgroup; a shape the heads kernel does not cover): the unfused lists are all there is - round 6: they read twins too (add_bf16_twins: the unfused family)
        add_bf16_twins(p, m.b, m.g, d.BT, d.D, {}, {});
    }
    return finish_plan(p, m.b, err);
}

const char *const TILE_CODES_TEXT = "0 or one of 114, 118, 212, 122, 214, 124, 221, 222 (+ 2000 / 3000: bf16 stages; + 10000 / 20000 / 30000: "
                                    "2 row / 2 column / 2 x 2 blocks per wave with 222 or 221, bf16 twins)";

// what every aggregation requires, in this order (the first failing check decides the message), then the model's builder
int build_plan_once(ta3n_plan &p, std::string &err) {
    const ta3n_config &c = p.cfg;
    const Dims d = dims_of(c);
    if (d.Bs < 0 || d.Bt < 0 || d.Bs + d.Bt <= 0) { err = "batch sizes must be non-negative and not both zero"; return TA3N_ERR_INVALID; }
    if (c.aggregation != TA3N_AGG_TRN_M && c.aggregation != TA3N_AGG_AVGPOOL && c.aggregation != TA3N_AGG_RNN && c.aggregation != TA3N_AGG_TEMCONV) {
        err = "aggregation must be TA3N_AGG_TRN_M or TA3N_AGG_AVGPOOL";      // (the text tests/golden/plan_fingerprints.json pins; TA3N_AGG_RNN and _TEMCONV are the others)
        return TA3N_ERR_INVALID;
    }
    if (c.aggregation == TA3N_AGG_TEMCONV) { const std::string e = temconv_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    if (c.aggregation == TA3N_AGG_RNN) { const std::string e = rnn_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    if (d.T < 2 || d.T > 64) { err = "num_segments must be in [2,64] for trn-m"; return TA3N_ERR_INVALID; }
    if (d.D <= 0 || d.F <= 0 || d.C <= 0) { err = "feature_dim, fc_dim and num_class must be positive"; return TA3N_ERR_INVALID; }
    if (d.NB <= 0 || d.NB % 64 != 0 || d.NB > 1024) { err = "num_bottleneck must be a multiple of 64 (<= 1024)"; return TA3N_ERR_INVALID; }
    if (d.C > 64) { err = "num_class > 64 not supported by the loss kernel"; return TA3N_ERR_INVALID; }
    if ((c.flags & TA3N_FLAG_CLASS_WEIGHTS) && d.Bs <= 0) {
        err = "TA3N_FLAG_CLASS_WEIGHTS (weighted class loss) without source rows: batch_source must be positive";
        return TA3N_ERR_INVALID;
    }
    // TA3N_FLAG_TARGET_LABELS (--use_target Sv) / TA3N_FLAG_TARGET_ENTROPY (--add_loss_DA target_entropy): what is not built, by name
    if ((c.flags & TA3N_FLAG_TARGET_LABELS) && (c.flags & TA3N_FLAG_MCD)) {
        err = "TA3N_FLAG_TARGET_LABELS (use_target Sv) with TA3N_FLAG_MCD: the reference itself fails there (main.py:448: out_source_2 has n_s rows against n_s + n_t labels)";
        return TA3N_ERR_INVALID;
    }
    if ((c.flags & TA3N_FLAG_TARGET_ENTROPY) && (c.flags & TA3N_FLAG_MCD)) {
        err = "TA3N_FLAG_TARGET_ENTROPY (add_loss_DA target_entropy) with TA3N_FLAG_MCD is not built (MCD rebinds out_target to the second pass's logits)";
        return TA3N_ERR_INVALID;
    }
    if ((c.flags & TA3N_FLAG_TARGET_LABELS) && d.Bt <= 0) {
        err = "TA3N_FLAG_TARGET_LABELS (use_target Sv) without target rows: batch_target must be positive";
        return TA3N_ERR_INVALID;
    }
    if ((c.flags & TA3N_FLAG_TARGET_ENTROPY) && (c.flags & TA3N_FLAG_ATTN_ENTROPY)) {
        err = "TA3N_FLAG_TARGET_ENTROPY and TA3N_FLAG_ATTN_ENTROPY are two values of one option (add_loss_DA target_entropy / attentive_entropy): set one";
        return TA3N_ERR_INVALID;
    }
    if ((c.flags & TA3N_FLAG_ATTN_ENTROPY) &&
        !((c.flags & TA3N_FLAG_ADV_RELATION) && (c.flags & TA3N_FLAG_ADV_VIDEO))) {
        // main.py:559-562 indexes pred_domain_all[1]; that is the video entry only when
        // place_adv[0] and place_adv[1] are both 'Y' (otherwise the reference fails on a shape mismatch)
        err = "attentive_entropy requires place_adv[0]=='Y' and place_adv[1]=='Y'";
        return TA3N_ERR_INVALID;
    }
    if ((c.flags & TA3N_FLAG_F32_SPLIT) && (c.flags & TA3N_FLAG_BF16_MFMA)) {
        err = "TA3N_FLAG_F32_SPLIT and TA3N_FLAG_BF16_MFMA are different arithmetics: set one";
        return TA3N_ERR_INVALID;
    }
    auto tile_ok = [](int t) { return t == 0 || tile_config_ok(t); };
    if (!tile_ok(c.tile_config)) { err = std::string("tile_config must be ") + TILE_CODES_TEXT; return TA3N_ERR_INVALID; }
    for (int i = 0; i < 16; ++i)
        if (!tile_ok(c.phase_tiles[i])) { err = std::string("phase_tiles entries must be ") + TILE_CODES_TEXT; return TA3N_ERR_INVALID; }
    if (c.xcd_aware < 0 || c.xcd_aware > 3) { err = "xcd_aware must be 0, 1, 2 or 3"; return TA3N_ERR_INVALID; }
    if ((int64_t)d.BT * d.D >= (1ll << 31) || (int64_t)d.BT * d.F >= (1ll << 31)) { err = "problem too large for 32-bit offsets"; return TA3N_ERR_INVALID; }
    { const std::string e = shared_layers_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    { const std::string e = share_params_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    { const std::string e = general_attn_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    { const std::string e = frame_attn_refusal(c); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    if (c.aggregation == TA3N_AGG_TRN_M) return build_plan_trn(p, err);
    p.n_tuples = 0;      // (no relation tuples)
    p.tuple_first.assign(1, 0);
    if (c.aggregation == TA3N_AGG_RNN || c.aggregation == TA3N_AGG_TEMCONV) return build_plan_avgpool_general(p, err);      // (also with no flag at all: there is no source-only fast path)
    // avgpool, source-only: the fused fast path (BASELINE configs[0]); with adversarial branches or a module-path option: the general one
    const uint32_t general = TA3N_FLAG_ADV_RELATION | TA3N_FLAG_ADV_VIDEO | TA3N_FLAG_ADV_FRAME | TA3N_FLAG_MCD | TA3N_FLAG_FEATURE_GRADS |
                             TA3N_FLAG_BN_SHARED;
    return (c.flags & general) ? build_plan_avgpool_general(p, err) : build_plan_avgpool(p, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// TA3N_FLAG_SCORE_ONLY: the forward to the class logits and nothing else (main.validate / test_models.py score out_target of an eval-mode
// forward, main.py:707-735).  The parameter table is the training plan's of the same configuration (`donor`, built first: its checks
// come first, and a training plan's params buffer is passed as it is); every row of batch_source + batch_target is alike.  One launch
// list, group 0, of launch kinds the training plans have, up to the aggregated feature:
//   trn-m    F1 | tuple products [+ Hr_j with TA3N_FLAG_TRANS_ATTN]                (the score kernel pools: no PH_POOL_FWD)
//   avgpool  F1 | PH_POOL_AVG_FWD          temconv  F1 | PH_TEMCONV_FWD          rnn  F1 | slot pooling | Gx | per step { Gh | cell }
// behind which ta3n_score runs the score kernel (ta3n_score.hip): classifier, softmax, rank, metrics.  No dropout epilogue (eval mode:
// the scalars ta3n_init_workspace leaves), no discriminator, no gradient / partial-sum / twin / optimiser region.
std::string score_refusal(const ta3n_config &c) {
    const std::string head = "TA3N_FLAG_SCORE_ONLY with ";
    const std::pair<uint32_t, const char *> flags[] = {
        {TA3N_FLAG_BN_SHARED, "TA3N_FLAG_BN_SHARED (use_bn)"}, {TA3N_FLAG_BF16_MFMA, "TA3N_FLAG_BF16_MFMA"}, {TA3N_FLAG_BF16_STORE, "TA3N_FLAG_BF16_STORE"},
        {TA3N_FLAG_F32_SPLIT, "TA3N_FLAG_F32_SPLIT"}, {TA3N_FLAG_FRAME_ATTN, "TA3N_FLAG_FRAME_ATTN (use_attn_frame)"},
        {TA3N_FLAG_GENERAL_ATTN, "TA3N_FLAG_GENERAL_ATTN (use_attn general)"}, {TA3N_FLAG_UNSHARED, "TA3N_FLAG_UNSHARED (share_params N)"},
        {TA3N_FLAG_CLASS_WEIGHTS, "TA3N_FLAG_CLASS_WEIGHTS (weighted class loss)"}};
    for (const auto &f : flags)
        if (c.flags & f.first) return head + f.second + " is not built";
    if (c.shared_fc_layers > 1) return head + "shared_fc_layers (--add_fc) " + std::to_string(c.shared_fc_layers) + " is not built";
    if (c.chain) return head + "chain is not built";
    if (c.split_k) return head + "split_k is not built";
    if (c.wgrads_late) return head + "wgrads_late is not built";
    for (int i = 0; i < 16; ++i)
        if (c.phase_tiles[i]) return head + "phase_tiles is not built";
    if (c.layout_flags) return head + "layout_flags is not built";
    // (trn-m: the score kernel keeps a video's pooled feature lane-resident, num_bottleneck / 64 channels per lane, in the widths it is instantiated for)
    const int q = c.num_bottleneck / 64;
    if (c.aggregation == TA3N_AGG_TRN_M && q != 1 && q != 2 && q != 4 && q != 8)
        return head + "num_bottleneck " + std::to_string(c.num_bottleneck) + " is not built: 64, 128, 256 or 512";
    return "";
}

int build_plan_score(ta3n_plan &p, std::string &err) {
    const ta3n_config cfg = p.cfg;
    ta3n_plan donor;
    donor.cfg = cfg;
    donor.cfg.flags = cfg.flags & ~TA3N_FLAG_SCORE_ONLY;
    const int rc = ta3n::build_plan(donor, err);
    if (rc != TA3N_OK) return rc;
    { const std::string e = score_refusal(cfg); if (!e.empty()) { err = e; return TA3N_ERR_INVALID; } }
    p = ta3n_plan();
    p.cfg = cfg;
    p.params = donor.params; p.param_floats = donor.param_floats; p.live_floats = donor.live_floats; p.first_floats = donor.first_floats;
    p.live_ranges = donor.live_ranges;
    p.n_tuples = donor.n_tuples; p.tuples = donor.tuples; p.scale_len = donor.scale_len; p.scale_id = donor.scale_id; p.tuple_first = donor.tuple_first;

    const ta3n_config &c = p.cfg;
    const Dims d = dims_of(c);
    const int B = d.B, BT = d.BT, D = d.D, F = d.F, C = d.C;
    const bool trn = c.aggregation == TA3N_AGG_TRN_M, attn = trn && (c.flags & TA3N_FLAG_TRANS_ATTN);
    const int NB = trn ? d.NB : F, NR = trn ? d.T - 1 : 0, NT = p.n_tuples;
    TrnModel m(p, d);                  // (its builder serves every aggregation; its specs trn-m)
    Builder &b = m.b;
    Geom &g = p.geom;
    init_geom(g, d, NB, c.flags);
    g.n_tuples = NT; g.n_rel = NR;
    g.o_F1 = (int32_t)b.add_region("F1", (int64_t)BT * F);
    if (trn) {
        m.resolve_params();
        g.o_Zr = (int32_t)b.add_region("Zr", (int64_t)B * NT * NB);
        if (attn) g.o_Hr = (int32_t)b.add_region("Hr", (int64_t)B * NR * NB);
        g.o_attn = (int32_t)b.add_region("attn", (int64_t)B * NR);
        g.p_W2_0 = (int32_t)m.W2[0]; g.p_b2_0 = (int32_t)m.B2[0];
        g.p_W2_stride = NR > 1 ? (int32_t)(m.W2[1] - m.W2[0]) : 0;
        g.p_b2_stride = NR > 1 ? (int32_t)(m.B2[1] - m.B2[0]) : 0;
    }
    const HeadParams w = head_params(p, false);      // (TA3N_FLAG_MCD: classifier 1 is the one scored, test_models.py)
    g.o_V = g.o_Vd = (int32_t)b.add_region("V", (int64_t)B * NB);      // eval mode: dropout_v is the identity, the aggregator launches write one region twice
    g.o_Y = (int32_t)b.add_region("Y", (int64_t)B * C);
    p.score.trn = trn ? 1 : 0; p.score.width = NB;      // (the per-video results lie back to back, "attn" .. "ce": one copy takes them all)
    p.score.o_prob = (int32_t)b.add_region("prob", (int64_t)B * C);
    p.score.o_rank = (int32_t)b.add_region("rank", B);
    p.score.o_pred = (int32_t)b.add_region("pred", B);
    p.score.o_ce = (int32_t)b.add_region("ce", B);
    AvgpoolDa a{b, g, d, w, SharedStack(), false, false, false, false};
    if (c.aggregation == TA3N_AGG_RNN) {
        RnnArgs &r = p.rnn;
        r = donor.rnn;                 // cell, n_ts, len_ts and the slot table
        const int GF = (r.cell ? 3 : 4) * F;
        const int64_t rows = (int64_t)r.n_ts * B;
        r.o_Xp = (int32_t)b.add_region("rnn_Xp", rows * F);
        r.o_Gx = (int32_t)b.add_region("rnn_Gx", rows * GF);
        r.o_Gh = (int32_t)b.add_region("rnn_Gh", rows * GF);
        r.o_gates = (int32_t)b.add_region("rnn_gates", rows * GF);
        r.o_c = (int32_t)b.add_region("rnn_c", (rows + B) * F);
        r.o_h = (int32_t)b.add_region("rnn_h", (rows + B) * F);
        r.o_gGx = r.o_gGh = r.o_gc = r.o_gh = r.o_ghd = r.o_gXp = -1;
        a.rnn = &p.rnn;
        a.Wih = p.poff("rnn.weight_ih_l0"); a.Whh = p.poff("rnn.weight_hh_l0");
        a.bih = p.poff("rnn.bias_ih_l0"); a.bhh = p.poff("rnn.bias_hh_l0");
    }
    if (c.aggregation == TA3N_AGG_TEMCONV)
        p.temconv = {(int32_t)p.poff("tcl_3_1.conv2d.weight"), (int32_t)p.poff("tcl_3_1.conv2d.bias"), -1, -1};
    p.score.o_ticket = (int32_t)b.add_region("score_ticket", 1);
    g.o_zeros = (int32_t)b.add_region("zeros", 64);   // never written: source of out-of-range operand elements
    g.o_ones = -1;                                    // (the column sums of the weight gradients read it: no such launch here)
    g.o_losses = (int32_t)b.add_region("losses", 8);  // (cleared by the aggregator launches, read by nobody)
    g.o_hyper = (int32_t)b.add_region("hyper", 32);
    g.o_labels = (int32_t)b.add_region("labels", B);
    g.o_tuple_first = (int32_t)b.add_region("tuple_first", NR + 1);
    g.o_metrics = (int32_t)b.add_region("metrics", 8);
    g.o_confusion = (int32_t)b.add_region("confusion", (int64_t)C * C);
    g.live_floats = (int32_t)p.live_floats;
    g.p_Wcv = (int32_t)w.Wcv; g.p_bcv = (int32_t)w.bcv;

    // the shared frame FC without its dropout epilogue (models.py:565-575 in eval mode)
    b.add_gemm_phase(0, spec_linear(BT, F, D, BASE_X, 0, D, w.Wsh, w.bsh, g.o_F1, F, true));
    if (trn) {
        std::vector<GemmSpec> s;
        for (int t = 0; t < NT; ++t) s.push_back(m.spec_Z(t));
        b.add_gemm_phase(0, s);
        if (attn) {
            std::vector<GemmSpec> h;
            for (int j = 0; j < NR; ++j) h.push_back(m.spec_Hr(j));
            b.add_gemm_phase(0, h);
        }
    } else if (a.rnn) a.rnn_forward(0);
    else b.add_simple_phase(c.aggregation == TA3N_AGG_TEMCONV ? PH_TEMCONV_FWD : PH_POOL_AVG_FWD, 0);
    return finish_plan(p, b, err);
}

}  // namespace

// models.py:397-409.  Python's round(T / n_ts) is half-to-even on the float quotient; T <= 64 and n_ts <= 128 make every quotient with
// fraction 1/2 exact in binary and keep every other one away from it, so the integer rule below is that rounding.
extern "C" int ta3n_rnn_slots(int num_segments, int n_ts, int32_t *len_ts, int32_t *frames) {
    if (num_segments < 1 || num_segments > 64) { ta3n::set_error("ta3n_rnn_slots: num_segments must be in [1,64]"); return TA3N_ERR_INVALID; }
    if (n_ts < 1 || n_ts > 128) { ta3n::set_error("ta3n_rnn_slots: n_ts must be in [1,128]"); return TA3N_ERR_INVALID; }
    const int q = num_segments / n_ts, r = num_segments % n_ts;
    const int len = 2 * r < n_ts ? q : 2 * r > n_ts ? q + 1 : q + (q & 1);
    if (len == 0) {
        ta3n::set_error("n_ts " + std::to_string(n_ts) + " with " + std::to_string(num_segments) + " segments: len_ts = round(num_segments / n_ts) is 0 "
                        "(the reference fails there, models.py:397-409)");
        return TA3N_ERR_INVALID;
    }
    if (len_ts) *len_ts = len;
    if (frames)
        for (int s = 0; s < len * n_ts; ++s) frames[s] = std::min(s, num_segments - 1);
    return TA3N_OK;
}

// Register-blocked tiles exist for launches that read bf16 twins only, and whether a launch does is known once the whole
// plan is laid out (add_bf16_twins): build, look, and rebuild without the blocking where it cannot be used.
int ta3n::build_plan(ta3n_plan &p, std::string &err) {
    const ta3n_config cfg = p.cfg;
    // TA3N_FLAG_TRAIN_METERS: a score-only plan has no step to meter; a chained step list is an experiments build's
    if ((cfg.flags & TA3N_FLAG_TRAIN_METERS) && (cfg.flags & TA3N_FLAG_SCORE_ONLY)) { err = "TA3N_FLAG_TRAIN_METERS with TA3N_FLAG_SCORE_ONLY is not built"; return TA3N_ERR_INVALID; }
    if ((cfg.flags & TA3N_FLAG_TRAIN_METERS) && cfg.chain) { err = "TA3N_FLAG_TRAIN_METERS with chain is not built"; return TA3N_ERR_INVALID; }
    if (cfg.flags & TA3N_FLAG_SCORE_ONLY) return build_plan_score(p, err);
    // ta3n_config.layout_flags: build the donor first and place this plan's parameters where the donor has them
    std::vector<ParamInfo> layout;
    int64_t donor_live = 0;
    if (cfg.layout_flags) {
        ta3n_plan donor;
        donor.cfg = cfg;
        donor.cfg.flags = cfg.layout_flags;
        donor.cfg.layout_flags = 0;
        const int rc = build_plan(donor, err);
        if (rc != TA3N_OK) { err = "layout_flags: the donor configuration is refused: " + err; return rc; }
        layout = donor.params;
        donor_live = donor.live_floats;
    }
    uint64_t deny = 0;
    for (int attempt = 0; attempt < 16; ++attempt) {
        p = ta3n_plan();
        p.cfg = cfg;
        p.deny_blocking = deny;
        p.layout = layout;
        const int rc = build_plan_once(p, err);
        if (rc != TA3N_OK) return rc;
        if (!layout.empty()) {
            if (p.layout_error.empty() && p.params.size() != layout.size()) p.layout_error = "the two configurations differ in their parameters";
            if (!p.layout_error.empty()) { err = "layout_flags: " + p.layout_error; return TA3N_ERR_INVALID; }
            std::stable_sort(p.params.begin(), p.params.end(), [](const ParamInfo &a, const ParamInfo &b) { return a.off < b.off; });   // the donor's order
            p.live_floats = donor_live;
            p.geom.live_floats = (int32_t)donor_live;
        }
        // the maximal runs of live parameters (8-float aligned slots: adjacent parameters touch)
        p.live_ranges.clear();
        if (layout.empty()) {
            p.live_ranges.push_back({0, p.live_floats});
        } else {
            for (const ParamInfo &pi : p.params) {
                if (!pi.live) continue;
                const int64_t b0 = pi.off, e0 = align_up(pi.off + (int64_t)pi.rows * (pi.cols ? pi.cols : 1), 8);
                if (!p.live_ranges.empty() && p.live_ranges.back().second == b0) p.live_ranges.back().second = e0;
                else p.live_ranges.push_back({b0, e0});
            }
        }
        uint64_t bad = 0;
        for (size_t i = 0; i < p.phases.size(); ++i) {
            const Phase &ph = p.phases[i];
            if (ph.kind == PH_GEMM && (ph.rm * ph.rn > 1 || (ph.bf16 & 64)) && !(ph.bf16 & 16)) bad |= 1ull << (i & 63);
        }
        if (bad == 0) return TA3N_OK;
        deny |= bad;
    }
    err = "internal: register-blocked tile selection did not settle";
    return TA3N_ERR_INVALID;
}
