// Device-side helpers and launcher declarations shared by the .hip files.
#pragma once
// -DTA3N_EXPERIMENTS=1 (the A/B build: TA3N_LIBDIR=ta3n_amd/lib_ab TA3N_EXTRA_FLAGS=-DTA3N_EXPERIMENTS=1 python -m ta3n_amd.build; tests:
// `pytest -m gpu_ab` with the same TA3N_LIBDIR) keeps the step-level variants that were built, measured and rejected - chained launches
// (ta3n_config.chain), split-K tiles (split_k), time-based tile order (cost_model), the optimiser inside the gradient tiles
// (ta3n_train_steps_fused_update), the four-wave 192x128 / 256x128 and four-half-stage kernels.  The default library carries only what a
// plan can select by default.  ta3n_plan_create still BUILDS such launch lists (host code, checked on the CPU by tests/plan_interp.py); launching one
// on the default library fails with TA3N_ERR_INVALID and a message naming the flag (launch_gemm returns -5, every caller maps it).  History: docs/history/.
#ifndef TA3N_EXPERIMENTS
#define TA3N_EXPERIMENTS 0
#endif
#include <hip/hip_runtime.h>

#include "../../include/ta3n_hip.h"
#include "ta3n_types.h"

namespace ta3n {

struct Ptrs {
    const float *x;   // BASE_X  input features [B*T, D]
    const float *p;   // BASE_P  flat parameters
    float *g;         // BASE_G  flat gradients
    float *ws;        // BASE_WS workspace
    const float *p16; // BASE_P16 bf16 twins of the parameters this launch reads (inside ws; nullptr: no twins)
};

// Side job of a GEMM launch (EPI_SGD tasks): the optimiser update of a parameter range, with its scalars by value.
// ta3n_train_step_after_update puts the update of everything but the shared frame FC into the first launch of the
// next step, whose own tiles only read the shared frame FC.
struct SgdSide {
    float *params, *momentum;
    float lr, mu, wd, clip;
    int32_t norm_off, norm_n;    // ws offsets of the squared-norm partials (fused per-tile slots or the grad_norm kernel's)
    int32_t p16_off;             // ws offset of the parameter twins, -1: none
    // Fused update (ta3n_train_steps_fused_update): every gradient tile applies the Nesterov step to its own block of parameters in
    // its epilogue - reads the parameters the step computes with (Ptrs.p) and the momentum, writes the NEW parameters (and their
    // twins) into the other buffer, so launches of the same step that still read the old values are not disturbed.  The clip
    // coefficient is taken as 1; sgd_fixup_kernel corrects the rare step whose gradient norm exceeds the clip value.
    float *p_new;                // nullptr: no fused update
    float *p16_new;              // twin region of p_new (floats), nullptr: no twins
};

__device__ __forceinline__ float hyper_scale(const Hyper *__restrict__ hy, int kind) {
    switch (kind) {
        case SK_NEG_BETA_REL: return -hy->beta[0];
        case SK_NEG_BETA_VID: return -hy->beta[1];
        case SK_NEG_BETA_FRM: return -hy->beta[2];
        case SK_INV_KEEP_I: return (hy->train && hy->p_drop_i > 0.f) ? (hy->p_drop_i < 1.f ? 1.f / (1.f - hy->p_drop_i) : 0.f) : 1.f;
        case SK_INV_KEEP_V: return (hy->train && hy->p_drop_v > 0.f) ? (hy->p_drop_v < 1.f ? 1.f / (1.f - hy->p_drop_v) : 0.f) : 1.f;
        case SK_REVERSE_MU: return hy->reverse ? -hy->mu : 1.f;
        default: return 1.f;
    }
}

// Stateless dropout stream: keep(seed, element) is recomputed in the backward
// pass instead of storing a mask (nn.Dropout, reference models.py:131-132,
// 574-575, 679-680; bit-matching torch's Philox/MT streams is not possible nor
// required - SURVEY.md 7 "Dropout").
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {      // (host too: ta3n_sample_segments draws with the device's own code)
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float keep_mask(uint32_t seed, uint32_t idx, float p) {
    const uint32_t h = mix32(mix32(idx + 0x9E3779B9U * (seed | 1u)) ^ seed);
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);   // [0,1)
    return u >= p ? 1.f : 0.f;
}

// Wave64 all-reduce on the DPP network (row-local butterflies, then row_bcast 15 / 31, then a readlane of lane 63):
// ~13 VALU instructions.  The __shfl_xor form compiles to six dependent ds_bpermute_b32 round trips through
// the LDS crossbar, which dominated the latency of the per-video stages of the heads kernel.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float identity, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v),
                                                                  CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_allreduce_sum(float v) {
    v += dpp_move<0xB1, 0xF>(0.f, v);    // quad_perm [1,0,3,2]
    v += dpp_move<0x4E, 0xF>(0.f, v);    // quad_perm [2,3,0,1]
    v += dpp_move<0x141, 0xF>(0.f, v);   // row_half_mirror
    v += dpp_move<0x140, 0xF>(0.f, v);   // row_mirror: every lane of a 16-lane row holds the row sum
    v += dpp_move<0x142, 0xA>(0.f, v);   // row_bcast:15 into rows 1 and 3
    v += dpp_move<0x143, 0xC>(0.f, v);   // row_bcast:31 into rows 2 and 3: lanes 48-63 hold the total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// This thread's share of  sum_{k < n} src[k]  (elements tid, tid + stride, ...), added in exactly the order of the plain loop
//     for (k = tid; k < n; k += stride) acc += src[k];
// but with EIGHT loads in flight per round trip: the plain loop compiled to load - s_waitcnt vmcnt(0) - add per iteration, i.e. n / stride
// dependent L2 round trips (five to twelve for the ~1 200 - 3 000 gradient-norm partials of a step) at the top of the optimiser launch
// that opens every step and of each of the update's side workgroups (ISA pass of round 5).  Elements past n are added as + 0.f:
// the partial sums are sums of squares (>= +0), so acc + 0 = acc bit for bit.
__device__ __forceinline__ float strided_partial_sum(const float *__restrict__ src, int n, int tid, int stride) {
    float acc = 0.f;
#pragma unroll 1
    for (int k0 = tid; k0 < n; k0 += 8 * stride) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + i * stride;
            v[i] = k < n ? src[k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += v[i];
    }
    return acc;
}

__device__ __forceinline__ float wave_allreduce_max(float v) {
    const float ninf = -INFINITY;
    v = fmaxf(v, dpp_move<0xB1, 0xF>(ninf, v));
    v = fmaxf(v, dpp_move<0x4E, 0xF>(ninf, v));
    v = fmaxf(v, dpp_move<0x141, 0xF>(ninf, v));
    v = fmaxf(v, dpp_move<0x140, 0xF>(ninf, v));
    v = fmaxf(v, dpp_move<0x142, 0xA>(ninf, v));
    v = fmaxf(v, dpp_move<0x143, 0xC>(ninf, v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

struct Soft2 {
    float p0, p1, lp0, lp1, H;
};
// softmax / log_softmax / entropy of a 2-vector, same formulas as torch
// (x - max, exp, sum; log_softmax = x - max - log(sum)).
__device__ __forceinline__ Soft2 soft2(float z0, float z1) {
    Soft2 s;
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float sum = e0 + e1;
    s.p0 = e0 / sum; s.p1 = e1 / sum;
    const float ls = logf(sum);
    s.lp0 = z0 - m - ls; s.lp1 = z1 - m - ls;
    s.H = -(s.p0 * s.lp0 + s.p1 * s.lp1);
    return s;
}

bool tile_config_ok(int cfg);   // WM*100 + WN*10 + WK of an instantiated gemm_tiles<WM, WN, WK>
int launch_gemm(const Phase &ph, const Task *d_tasks, const Seg *d_segs, const Ptrs &ptrs, int hyper_off,
                int zeros_off, int twin_off, hipStream_t stream, const SgdSide *side = nullptr, const Wait *d_waits = nullptr,
                int pair_delta = 0, int kinds = 0);
#if defined(__HIPCC__)
// two floats -> one dword of two bf16 (round to nearest even: v_cvt_pk_bf16_f32), low half = first argument
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// the lo halves of the split x = hi + lo (pair twins, Geom::pair_delta): lo = bf16(x - float(hi)); the subtraction is exact in fp32
__device__ __forceinline__ unsigned pack_bf16_lo(float x0, float x1, unsigned hi) {
    return pack_bf16(x0 - __builtin_bit_cast(float, hi << 16), x1 - __builtin_bit_cast(float, hi & 0xFFFF0000u));
}

// The optimiser arithmetic, written ONCE: every training path (plain, deferred, pipelined, sharded, the EPI_SGD side job of gemm_tile, the
// fused-update tiles) must produce the same bits, so each of them calls these (the Adam rule, adam_update, is beside its kernel).  Device code is compiled with contraction on: the fmaf
// forms below are the arithmetic, keep every expression as written.
// clip_grad_norm_: coef = clip / (total_norm + 1e-6) clamped to 1; clip <= 0: no clipping
__device__ __forceinline__ float clip_coef(float total, float clip) {
    float coef = 1.f;
    if (clip > 0.f) coef = fminf(clip / (total + 1e-6f), 1.f);
    return coef;
}
// torch.optim.SGD(nesterov=True) on one element, g_scaled = g * coef:  d = g_scaled + wd p;  m = mu m + d;  d += mu m;  p -= lr d
__device__ __forceinline__ void nesterov_sgd(float &p, float &m, float g_scaled, float lr, float mu, float wd) {
    float d = fmaf(wd, p, g_scaled);
    m = fmaf(mu, m, d);
    d = fmaf(mu, m, d);
    p = fmaf(-lr, d, p);
}

// The loss and attention rules, written ONCE under the same contract (keep every expression as written, association included): the fused heads
// kernel, the unfused lists (pool_fwd / loss / pool_bwd, frame_attn_*, pool_cls), the MCD glue and the validation metrics call these, and every new variant does.
// Is video b of the batch [Bs source | Bt target] a real row, not the padding of a ragged batch (source-only steps pass valid_target = 0)
__device__ __forceinline__ bool video_valid(int Bs, int valid_source, int valid_target, int b) { return b < Bs ? (b < valid_source) : (b - Bs < valid_target); }
// Is the class cross-entropy of video b on: a valid source row, or - TA3N_FLAG_TARGET_LABELS - any valid row (main.py:442-446)
__device__ __forceinline__ bool class_ce_on(uint32_t flags, int Bs, bool valid, int b) { return valid && (b < Bs || (flags & TA3N_FLAG_TARGET_LABELS)); }
// Domain cross-entropy of a 2-logit row (source: label 0, target: 1), mean over 1 / inv_n rows (main.py:508-538): loss term and logit gradient
struct DomainCe { float l, g0, g1; };
__device__ __forceinline__ DomainCe domain_ce(const Soft2 &s, bool is_src, float inv_n) {
    const int d = is_src ? 0 : 1;
    return {-(d ? s.lp1 : s.lp0) * inv_n, (s.p0 - (d == 0 ? 1.f : 0.f)) * inv_n, (s.p1 - (d == 1 ? 1.f : 0.f)) * inv_n};
}
__device__ __forceinline__ float dH_dz(float p, float lp, float H) { return -p * (lp + H); }   // of the entropy H of softmax(z) (loss.py:20-24)
// Plain target entropy (TA3N_FLAG_TARGET_ENTROPY, --add_loss_DA target_entropy; main.py:542-545, loss.py:8-12): gamma * mean over the valid target
// rows of H(softmax y).  Per valid target row: the loss term, and the logit gradient with ce = gamma * inv_n_ent.  No (1 + H_d) factor, nothing
// to the domain logits, nothing on source rows.
__device__ __forceinline__ bool target_ent_on(uint32_t flags, int Bs, bool valid, int b) { return (flags & TA3N_FLAG_TARGET_ENTROPY) && valid && b >= Bs; }
__device__ __forceinline__ float target_ent_loss(float Hc, float inv_n_ent) { return Hc * inv_n_ent; }
__device__ __forceinline__ float target_ent_grad(float ce, float p, float lp, float Hc) { return ce * dH_dz(p, lp, Hc); }
// Transferable attention (models.py:351-357): w = 1 - H(softmax z) and the features scaled by 1 + w.  The weights are not detached: with
// dot = dL/dw, dot dw/dz_i = dot p_i (log p_i + H) joins the logit gradients; the gradient behind the scale is 1 + (1 - H) times the one in front.
__device__ __forceinline__ float attn_weight(const Soft2 &s) { return 1.f - s.H; }
__device__ __forceinline__ float attn_scale(const Soft2 &s) { return 1.f + (1.f - s.H); }
__device__ __forceinline__ void attn_back(const Soft2 &s, float dot, float &g0, float &g1) {
    g0 += dot * s.p0 * (s.lp0 + s.H);
    g1 += dot * s.p1 * (s.lp1 + s.H);
}
// log_softmax of <= 64 logits over the lanes of a wave (lane c = class c where `on`) as torch takes it: m = max, e = exp(y - m), sum, ls = log sum,
// lp = y - m - ls (0 off).  The softmax stays at the site: expf(lp) in the step's kernels, e / sum (torch's) in row_soft - they differ in the last bit.
struct LaneSoft { float m, e, sum, ls, lp; };
__device__ __forceinline__ LaneSoft lane_log_softmax(float y, bool on) {
    const float m = wave_allreduce_max(on ? y : -INFINITY), e = on ? expf(y - m) : 0.f;
    const float sum = wave_allreduce_sum(e), ls = logf(sum);
    return {m, e, sum, ls, on ? y - m - ls : 0.f};
}
// gH = (ga wa + gb wb) [h > 0]: the way back through a 2-wide output layer and the ReLU in front of it.  The fmaf is written out (gb wb is rounded on its own): left to contraction, which product that is changes with the code around the sum.
__device__ __forceinline__ float relu_back2(float h, float ga, float wa, float gb, float wb) { return h > 0.f ? fmaf(ga, wa, gb * wb) : 0.f; }
__device__ __forceinline__ float class_ce_grad(float p, bool is_label, float inv_n_cls) { return (p - (is_label ? 1.f : 0.f)) * inv_n_cls; }   // main.py:446
// Weighted criteria (main.py:160-167, 205-206: CrossEntropyLoss(weight = w), mean reduction = sum_i w[y_i] ce_i / sum_i w[y_i]).
// Class CE (TA3N_FLAG_CLASS_WEIGHTS): the coefficient of a row, handed to class_ce_grad and the loss term in place of inv_n_cls, is
// w[label] / sum_j w[label_j] over the valid source rows of the step.  Every wave that needs it forms the sum itself, from ws["labels"] and
// ws["class_w"]: lane l adds rows l, l + 64, ... in order, then wave_allreduce_sum - the same bits in every workgroup of every launch of
// the step, with no launch of its own and nothing from the host (device-gathered batches: the labels arrive in the step's opening launch).
// Rows at and past valid_source (padding) never enter; a label outside [0, C) adds nothing.  All 64 lanes must be active at the call.
// TA3N_FLAG_TARGET_LABELS (--use_target Sv, main.py:442-446: criterion(cat(out_source, out_target), cat(label_source, label_target))): the valid
// target rows carry labels too (ws["labels"][Bs + j]) and enter the class CE and the sum of the weights; callers whose rows are all source
// rows (validation, the source-only pool_cls) pass valid_target = 0.
struct ClassRule { const float *w; float inv; int C; };      // w == nullptr: unweighted, inv = inv_n_cls; otherwise inv = 1 / sum_j w[label_j]
__device__ __forceinline__ ClassRule class_rule(const Geom &g, const float *__restrict__ ws, int class_w_off, int valid_source, int valid_target, float inv_n_cls, int lane) {
    if (!(g.flags & TA3N_FLAG_CLASS_WEIGHTS) || class_w_off <= 0) return {nullptr, inv_n_cls, g.C};
    const float *__restrict__ w = ws + class_w_off;
    const int *__restrict__ labels = reinterpret_cast<const int *>(ws + g.o_labels);
    const int n = valid_source < g.Bs ? valid_source : g.Bs;
    float acc = 0.f;
    for (int j = lane; j < n; j += 64) {
        const int l = labels[j];
        acc += (unsigned)l < (unsigned)g.C ? w[l] : 0.f;
    }
    if (g.flags & TA3N_FLAG_TARGET_LABELS) {      // the second range, [Bs, Bs + valid_target), behind the first in every lane: one order at every call site
        const int nt = valid_target < g.B - g.Bs ? valid_target : g.B - g.Bs;
        for (int j = lane; j < nt; j += 64) {
            const int l = labels[g.Bs + j];
            acc += (unsigned)l < (unsigned)g.C ? w[l] : 0.f;
        }
    }
    const float sum = wave_allreduce_sum(acc);
    return {w, sum > 0.f ? 1.f / sum : 0.f, g.C};
}
__device__ __forceinline__ float class_coef(const ClassRule &r, int label) { return r.w ? ((unsigned)label < (unsigned)r.C ? r.w[label] * r.inv : 0.f) : r.inv; }
// Domain CE: 1 / n of the level times the step's factor for the row's domain (ta3n_hyper.dom_k; 0 is read as 1: unweighted, and x * 1.f = x bit for bit)
__device__ __forceinline__ float domain_factor(float k) { return k != 0.f ? k : 1.f; }
__device__ __forceinline__ float domain_coef(float inv_n, bool is_src, float k_src, float k_tgt) { return inv_n * (is_src ? k_src : k_tgt); }
// One value / four values to the bf16 twin (TA3N_FLAG_BF16_STORE): the hi plane and, with pair twins (Geom::pair_delta floats further on), the lo plane
__device__ __forceinline__ void twin1(unsigned short *__restrict__ tw, int64_t pair_delta, float v) {
    const unsigned h = pack_bf16(v, 0.f);
    *tw = (unsigned short)h;
    if (pair_delta) tw[2 * (size_t)pair_delta] = (unsigned short)pack_bf16_lo(v, 0.f, h);
}
struct Twin4 { uint2 hi, lo; };
__device__ __forceinline__ Twin4 twin4(const float4 v) {
    const unsigned h0 = pack_bf16(v.x, v.y), h1 = pack_bf16(v.z, v.w);
    return {make_uint2(h0, h1), make_uint2(pack_bf16_lo(v.x, v.y, h0), pack_bf16_lo(v.z, v.w, h1))};
}
#endif

// Where an update finds the squared-norm partials of its step: the per-tile slots the fused step's gradient tiles left behind, or the
// per-block partials of grad_norm_kernel (also the sharded update's per-rank slots)
struct NormSource {
    int32_t off, n;      // ws offset, count
};
inline NormSource norm_source(const Geom &g, bool fused_norm) {
    return fused_norm ? NormSource{g.o_sumsq, g.n_sumsq} : NormSource{g.o_norm_part, g.n_norm_blocks};
}

int launch_to_bf16(const float *src, float *dst_twin, int64_t n, hipStream_t stream);   // n fp32 -> n bf16 (RNE), n % 4 == 0
int launch_to_bf16_pair(const float *src, float *dst_hi, float *dst_lo, int64_t n, hipStream_t stream);   // ... and the lo plane
bool heads_supported(int NB, int C, int F);   // configurations the fused heads kernel (ta3n_heads.hip) covers
int launch_heads(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int set_heads_waves(int waves);               // 0 automatic / 4 / 8 waves per workgroup of the heads kernel, where a shape has both; -1: no such value
int heads_waves(const Geom &g);               // what launch_heads would launch for this geometry now (0: no heads kernel)
int launch_pool_cls(const Geom &g, const Ptrs &ptrs, hipStream_t stream);   // TA3N_AGG_AVGPOOL: between F1 and gZ1
int launch_pool_avg_fwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int launch_pool_avg_bwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int launch_bn_shared_fwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int launch_mcd_source_loss(const Geom &g, float *ws, float *part, float *out, hipStream_t stream);                            // ens_DA MCD glue (ta3n_mcd_*)
int launch_mcd_second_loss(const Geom &g, float *ws, float *ws2, float inv_count, float *part, float *out, hipStream_t stream);
int launch_bn_shared_bwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int launch_pool_fwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
int launch_loss(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
// TA3N_FLAG_FRAME_ATTN: ws offsets of regions "F1a", "attn_frame" / "gF1a", the additive base ("gF1s" or "gRa"), "gPfT"
int launch_frame_attn_fwd(const Geom &g, const Ptrs &ptrs, int o_F1a, int o_attn_frame, hipStream_t stream);
int launch_frame_attn_bwd(const Geom &g, const Ptrs &ptrs, int o_gF1a, int o_gFs, int o_gPfT, hipStream_t stream);
// TA3N_FLAG_GENERAL_ATTN: ws offsets of regions "Ua" / "gUa", "gs"; parameter offsets of attn_layer.2.weight / .bias
int launch_general_attn_fwd(const Geom &g, const Ptrs &ptrs, int o_Ua, int p_wa2, int p_ba2, hipStream_t stream);
int launch_general_attn_bwd(const Geom &g, const Ptrs &ptrs, int o_Ua, int o_gUa, int o_gs, int p_wa2, hipStream_t stream);
int launch_pool_bwd(const Geom &g, const Ptrs &ptrs, hipStream_t stream);
// TA3N_AGG_RNN (ta3n_rnn.hip): slot max-pooling and one cell step t, forward and backward
int launch_rnn_pool_fwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, hipStream_t stream);
int launch_rnn_cell_fwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, int t, hipStream_t stream);
int launch_rnn_cell_bwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, int t, hipStream_t stream);
int launch_rnn_pool_bwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, hipStream_t stream);
// TA3N_AGG_TEMCONV (ta3n_temconv.hip): the 3-tap filter over the segments + ReLU + mean, its way back, the parameter-gradient sum
int launch_temconv_fwd(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream);
int launch_temconv_bwd(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream);
int launch_temconv_wgrad(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream);
int launch_grad_norm(const Geom &g, const float *grads, float *ws, hipStream_t stream);
int launch_sgd(const Geom &g, float *params, const float *grads, float *momentum, float *ws, hipStream_t stream,
               bool fused_norm = false);
int launch_fill(float *dst, float value, int64_t n, hipStream_t stream);
int launch_set_hyper(float *ws_hyper, const Hyper &h, hipStream_t stream);   // scalars by kernel argument (no staging copy)
int launch_sgd_fixup(const Geom &g, float *params, const float *grads, float *momentum, float *ws, float *p16, float lr, float mu,
                     float clip, const Hyper *next, hipStream_t stream);
int launch_sgd_range(const Geom &g, float *params, const float *grads, float *momentum, float *ws, int64_t begin, int64_t end,
                     bool fused_norm, float lr, float mu, float wd, float clip, const Hyper *next, hipStream_t stream, bool write_norm = false);
// The live ranges of a plan (ta3n_live_range) in float4 units, as a launch argument of ta3n_sgd_live's two kernels: ascending, disjoint,
// none empty.  block0: first workgroup of each range in the update launch (filled by launch_sgd_live; block0[n] = the grid).
struct LiveRanges {
    static constexpr int MAX = 32;
    int32_t n;
    int32_t i0[MAX], i1[MAX], block0[MAX + 1];
};
int launch_live_norm(const Geom &g, const float *grads, float *ws, const LiveRanges &ranges, hipStream_t stream);
int launch_sgd_live(const Geom &g, float *params, const float *grads, float *momentum, float *ws, LiveRanges ranges, bool fused_norm,
                    float lr, float mu, float wd, float clip, hipStream_t stream);
// clip + Adam over floats [begin, end) of the live prefix (adam_range_kernel): step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t)
// already formed by the host (ta3n_adam_scalars); the betas in double so that 1 - beta reaches the kernel as torch's fp32 value of it
int launch_adam_range(const Geom &g, float *params, const float *grads, float *exp_avg, float *exp_avg_sq, float *ws, int64_t begin,
                      int64_t end, bool fused_norm, float step_size, float bc2_sqrt, double beta1, double beta2, float eps, float wd,
                      float clip, const Hyper *next, hipStream_t stream);
// One gather of the device batch assembly - a ta3n_gather_segments* call, or one batch half of a step's feed: device pointers of a packed
// feature store (fp32 rows, or bf16 rows where bf16 != 0), the video ids, where the rows go (fp32 rows / bf16 twin rows, either may be
// null; labels and 1-based frame numbers where asked for), and the sampler with the key of its draw.  n_videos = 0: nothing to assemble
struct FeedJob {
    const void *store;
    const int64_t *first_row;
    const int32_t *num_frames, *labels, *video_ids;
    float *out, *twin;
    int32_t *labels_out, *seg_out;
    int32_t n_videos, bf16;
    int32_t sampler;             // TA3N_SAMPLER_*; seed and step key the train sampler's draw (sample_offset)
    uint32_t seed, step;
};
__host__ __device__ inline int feed_rows(const FeedJob &job, int T) { return job.n_videos > 0 ? job.n_videos * T : 0; }
// one workgroup per output row (gather_kernel); pair_delta: the plan's distance from a twin's hi plane to its lo plane, 0 for none
int launch_gather(const FeedJob &job, int T, int D, int64_t pair_delta, hipStream_t stream);
// the launch that opens a pipelined step together with its batch assembly (sgd_open_feed_kernel): the update's workgroups, then the rows of feeds[0], feeds[1]
int launch_sgd_open_feed(const Geom &g, float *params, const float *grads, float *momentum, float *ws, int64_t begin, int64_t end,
                         bool fused_norm, float lr, float mu, float wd, float clip, const Hyper *next, const FeedJob feeds[2], hipStream_t stream);
int launch_shard_sumsq(const Geom &g, const float *grads, float *ws, int64_t a0, int64_t a1, int64_t b0, int64_t b1, int rank, hipStream_t stream);
int launch_eval_metrics(const Geom &g, float *ws, int n, int reset, hipStream_t stream);
// TA3N_FLAG_SCORE_ONLY (ta3n_score.hip): classifier, softmax, rank and metrics of the first n videos, behind the plan's launch list
int launch_score(const Geom &g, const Ptrs &ptrs, const ScoreArgs &a, int n, int reset, hipStream_t stream);
// TA3N_FLAG_TRAIN_METERS (ta3n_meters.hip): one step's loss slots, source accuracy and domain accuracy added to the two meter regions
int launch_train_meters(const Geom &g, const Ptrs &ptrs, const MetersArgs &a, hipStream_t stream);

}  // namespace ta3n

// pieces of the sharded update that live beside the RCCL binding (csrc/ta3n_comm.hip)
struct ta3n_comm;
namespace ta3n {
int comm_rank(const ta3n_comm *c);
int comm_world_size(const ta3n_comm *c);
hipEvent_t comm_event(ta3n_comm *c, int which);      // 0 fork, 1 join, 2 fork2, 3 join2 (created on first use)
int comm_reduce_scatter_sum(ta3n_comm *c, float *buf, int64_t begin, int64_t chunk, void *scratch_bf16, hipStream_t s);
int comm_all_gather(ta3n_comm *c, float *buf, int64_t begin, int64_t chunk, hipStream_t s);
}  // namespace ta3n
