// TA3N_AGG_RNN: the pointwise kernels of the recurrent frame aggregator (reference models.py:202-215, 392-422) - temporal slot
// max-pooling, one LSTM / GRU cell step, and both ways back.  The contractions between them (Gx = Xp W_ih^T + b_ih, Gh_t = h_{t-1} W_hh^T
// + b_hh, gh_{t-1} += gGh_t W_hh, the weight gradients, gXp = gGx W_ih) are tile-list GEMM launches of the plan (ta3n_plan.cpp: AvgpoolDa).
// All four are bandwidth-bound: a thread moves four columns as one 16-byte access (F % 4 == 0: avgpool_dims_refusal) and owns every
// gate of its hidden units, so nothing crosses lanes; sigmoid and tanh are expf-based fp32.  Tensors are time-major (row t * B + b).
#include "ta3n_kernels.h"

namespace ta3n {
namespace {

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
// 1 - 2 / (e^{2x} + 1): exact limits at +-inf (expf overflows to inf -> 1, underflows to 0 -> -1), no cancellation blow-up inside
__device__ __forceinline__ float tanh_f(float x) { return 1.f - 2.f / (expf(2.f * x) + 1.f); }

__device__ __forceinline__ float4 ld4(const float *__restrict__ p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *__restrict__ p, const float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
template <typename Fn> __device__ __forceinline__ float4 map4(Fn f, const float4 a) { return make_float4(f(a.x), f(a.y), f(a.z), f(a.w)); }
template <typename Fn> __device__ __forceinline__ float4 map4(Fn f, const float4 a, const float4 b) {
    return make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w));
}
template <typename Fn> __device__ __forceinline__ float4 map4(Fn f, const float4 a, const float4 b, const float4 c) {
    return make_float4(f(a.x, b.x, c.x), f(a.y, b.y, c.y), f(a.z, b.z, c.z), f(a.w, b.w, c.w));
}

// Temporal segments and pooling (models.py:397-409): window j of video b holds the frames of slots j * len_ts .. (j + 1) * len_ts - 1
// (ta3n_rnn_slots: frames past the last slot are dropped, the last frame repeats where there are too few).  One workgroup per video;
// it also clears the zero initial state (slab 0 of h and c).
__global__ __launch_bounds__(256) void rnn_pool_fwd_kernel(Geom g, Ptrs ptrs, RnnArgs a) {
    float *__restrict__ ws = ptrs.ws;
    const int b = blockIdx.x, F = g.F, T = g.T, B = g.B;
    for (int k = threadIdx.x * 4; k < F; k += 1024) {
        const float *__restrict__ f1 = ws + g.o_F1 + (size_t)b * T * F + k;
        for (int j = 0; j < a.n_ts; ++j) {
            float4 m = ld4(f1 + (size_t)a.frames[j * a.len_ts] * F);
            for (int i = 1; i < a.len_ts; ++i) m = map4(fmaxf, m, ld4(f1 + (size_t)a.frames[j * a.len_ts + i] * F));
            st4(ws + a.o_Xp + ((size_t)j * B + b) * F + k, m);
        }
        st4(ws + a.o_h + (size_t)b * F + k, make_float4(0.f, 0.f, 0.f, 0.f));
        if (a.cell == 0) st4(ws + a.o_c + (size_t)b * F + k, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// One step of nn.LSTM / nn.GRU (one layer, one direction) for every (video, four hidden units): the activated gates go to "rnn_gates"
// for the backward pass.
//   LSTM (gates i, f, g, o):  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
//   GRU  (gates r, z, n):     n = tanh(Gx_n + r Gh_n)  (Gh_n = W_hn h + b_hn: b_hh stays on the recurrent side),  h_t = (1 - z) n + z h_{t-1}
// The last step also writes the video feature V = h_t and Vd = dropout_v(V) - element id b * F + k, as pool_avg_fwd_kernel - and clears
// the eight loss slots the loss kernel accumulates into.
__global__ __launch_bounds__(256) void rnn_cell_fwd_kernel(Geom g, Ptrs ptrs, RnnArgs a, int t) {
    float *__restrict__ ws = ptrs.ws;
    const Hyper *__restrict__ hy = reinterpret_cast<const Hyper *>(ws + g.o_hyper);
    const int F = g.F, B = g.B, F4 = F / 4, GF = (a.cell ? 3 : 4) * F;
    const bool last = t == a.n_ts - 1;
    if (last && blockIdx.x == 0 && threadIdx.x < 8) ws[g.o_losses + threadIdx.x] = 0.f;
    const bool drop_v = hy->train != 0 && hy->p_drop_v > 0.f;
    const float inv_keep_v = hyper_scale(hy, SK_INV_KEEP_V), p_v = hy->p_drop_v;
    const uint32_t seed_v = hy->seed_v;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < B * F4; e += gridDim.x * 256) {
        const int b = e / F4, k = (e - b * F4) * 4;
        const size_t row = (size_t)t * B + b;
        const float *__restrict__ gx = ws + a.o_Gx + row * GF + k;
        const float *__restrict__ gh = ws + a.o_Gh + row * GF + k;
        float *__restrict__ act = ws + a.o_gates + row * GF + k;
        const float4 hp = ld4(ws + a.o_h + row * F + k);      // slab t = h_{t-1}
        float4 h;
        if (a.cell == 0) {
            const float4 gi = map4(sigmoidf, add4(ld4(gx), ld4(gh))), gf = map4(sigmoidf, add4(ld4(gx + F), ld4(gh + F)));
            const float4 gg = map4(tanh_f, add4(ld4(gx + 2 * F), ld4(gh + 2 * F))), go = map4(sigmoidf, add4(ld4(gx + 3 * F), ld4(gh + 3 * F)));
            const float4 cp = ld4(ws + a.o_c + row * F + k);
            const float4 c = add4(map4([](float x, float y) { return x * y; }, gf, cp), map4([](float x, float y) { return x * y; }, gi, gg));
            h = map4([](float o, float cc) { return o * tanh_f(cc); }, go, c);
            st4(act, gi); st4(act + F, gf); st4(act + 2 * F, gg); st4(act + 3 * F, go);
            st4(ws + a.o_c + (row + B) * F + k, c);
        } else {
            const float4 gr = map4(sigmoidf, add4(ld4(gx), ld4(gh))), gz = map4(sigmoidf, add4(ld4(gx + F), ld4(gh + F)));
            const float4 gn = map4([](float x, float r, float hn) { return tanh_f(x + r * hn); }, ld4(gx + 2 * F), gr, ld4(gh + 2 * F));
            h = map4([](float z, float n, float p) { return (1.f - z) * n + z * p; }, gz, gn, hp);
            st4(act, gr); st4(act + F, gz); st4(act + 2 * F, gn);
        }
        st4(ws + a.o_h + (row + B) * F + k, h);
        if (last) {
            st4(ws + g.o_V + (size_t)b * F + k, h);
            float4 vd = h;
            if (drop_v) {
                const uint32_t id = (uint32_t)(b * F + k);
                vd.x *= keep_mask(seed_v, id, p_v) * inv_keep_v; vd.y *= keep_mask(seed_v, id + 1, p_v) * inv_keep_v;
                vd.z *= keep_mask(seed_v, id + 2, p_v) * inv_keep_v; vd.w *= keep_mask(seed_v, id + 3, p_v) * inv_keep_v;
            }
            st4(ws + g.o_Vd + (size_t)b * F + k, vd);
        }
    }
}

// Step t of the way back.  gh_t: at the last step the gradient at V - gVt (it carries dropout_v's mask and scale already) plus, with
// TA3N_FLAG_FEATURE_GRADS, the caller's - otherwise "rnn_gh", which the GEMM launch after step t + 1 completed.  gc_t: slab t + 1 of
// "rnn_gc" (zero at the last step).  Out: gGx_t and gGh_t (gradients at the two pre-activation projections; they differ only in the
// GRU's n gate, where the recurrent part sits behind r), gc_{t-1} into slab t, and the part of gh_{t-1} that does not go through W_hh
// ("rnn_ghd": z gh_t for the GRU, zero for the LSTM).
__global__ __launch_bounds__(256) void rnn_cell_bwd_kernel(Geom g, Ptrs ptrs, RnnArgs a, int t) {
    float *__restrict__ ws = ptrs.ws;
    const int F = g.F, B = g.B, F4 = F / 4, GF = (a.cell ? 3 : 4) * F;
    const bool last = t == a.n_ts - 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < B * F4; e += gridDim.x * 256) {
        const int b = e / F4, k = (e - b * F4) * 4;
        const size_t row = (size_t)t * B + b, vid = (size_t)b * F + k;
        float4 gh;
        if (last) {
            gh = ld4(ws + g.o_gVt + vid);
            if (g.o_gV_ext > 0) gh = add4(gh, ld4(ws + g.o_gV_ext + vid));
        } else gh = ld4(ws + a.o_gh + vid);
        const float *__restrict__ act = ws + a.o_gates + row * GF + k;
        float *__restrict__ ggx = ws + a.o_gGx + row * GF + k;
        float *__restrict__ ggh = ws + a.o_gGh + row * GF + k;
        if (a.cell == 0) {
            const float4 gi = ld4(act), gf = ld4(act + F), gg = ld4(act + 2 * F), go = ld4(act + 3 * F);
            const float4 cp = ld4(ws + a.o_c + row * F + k), c = ld4(ws + a.o_c + (row + B) * F + k);
            const float4 tc = map4(tanh_f, c);
            float4 gc = map4([](float h, float o, float tt) { return h * o * (1.f - tt * tt); }, gh, go, tc);
            if (!last) gc = add4(gc, ld4(ws + a.o_gc + (row + B) * F + k));
            const float4 di = map4([](float q, float x, float i) { return q * x * i * (1.f - i); }, gc, gg, gi);
            const float4 df = map4([](float q, float x, float f) { return q * x * f * (1.f - f); }, gc, cp, gf);
            const float4 dg = map4([](float q, float i, float x) { return q * i * (1.f - x * x); }, gc, gi, gg);
            const float4 dq = map4([](float h, float tt, float o) { return h * tt * o * (1.f - o); }, gh, tc, go);
            st4(ggx, di); st4(ggx + F, df); st4(ggx + 2 * F, dg); st4(ggx + 3 * F, dq);
            st4(ggh, di); st4(ggh + F, df); st4(ggh + 2 * F, dg); st4(ggh + 3 * F, dq);
            st4(ws + a.o_gc + row * F + k, map4([](float q, float f) { return q * f; }, gc, gf));
            st4(ws + a.o_ghd + vid, make_float4(0.f, 0.f, 0.f, 0.f));
        } else {
            const float4 gr = ld4(act), gz = ld4(act + F), gn = ld4(act + 2 * F);
            const float4 hp = ld4(ws + a.o_h + row * F + k), hn = ld4(ws + a.o_Gh + row * GF + 2 * F + k);
            const float4 dn = map4([](float h, float z, float n) { return h * (1.f - z) * (1.f - n * n); }, gh, gz, gn);
            const float4 dz = map4([](float h, float d, float z) { return h * d * z * (1.f - z); }, gh,
                                   map4([](float p, float n) { return p - n; }, hp, gn), gz);
            const float4 dr = map4([](float d, float x, float r) { return d * x * r * (1.f - r); }, dn, hn, gr);
            st4(ggx, dr); st4(ggx + F, dz); st4(ggx + 2 * F, dn);
            st4(ggh, dr); st4(ggh + F, dz); st4(ggh + 2 * F, map4([](float d, float r) { return d * r; }, dn, gr));
            st4(ws + a.o_ghd + vid, map4([](float h, float z) { return h * z; }, gh, gz));
        }
    }
}

// Backward of the slot max-pooling: gXp[j][b] goes to the frame that held the window's maximum - the LOWEST frame index among equal
// candidates.  (Ties need no rule of their own: F1 = dropout_i(relu(.)) has exact zeros, but where a window's maximum is 0 every
// candidate is 0 and the [F1 > 0] mask of gZ1 removes the gradient; the only other exact tie is the last frame against its repeats,
// and those land on the same frame.)  Frames are visited in slot order; only the last frame can serve several slots, so every other
// frame is written exactly once and the last one collects its sum in a register: no atomics, one workgroup owns a video's rows.
// Frames in no window receive zero.  direct: no live frame discriminator - the result IS gZ1 after the ReLU / dropout_i mask;
// otherwise it is the additive base ("gRa") of the launch that forms gZ1.  The two modes of pool_avg_bwd_kernel.
__global__ __launch_bounds__(256) void rnn_pool_bwd_kernel(Geom g, Ptrs ptrs, RnnArgs a, int direct) {
    float *__restrict__ ws = ptrs.ws;
    const Hyper *__restrict__ hy = reinterpret_cast<const Hyper *>(ws + g.o_hyper);
    const int b = blockIdx.x, F = g.F, T = g.T, B = g.B, L = a.n_ts * a.len_ts;
    const float inv_keep_i = hyper_scale(hy, SK_INV_KEEP_I);
    float *__restrict__ out = ws + (direct ? g.o_gZ1 : g.o_gRa) + (size_t)b * T * F;
    const auto put = [&](int f, int k, const float4 f1, const float4 v) {
        st4(out + (size_t)f * F + k, direct ? map4([=](float x, float y) { return x > 0.f ? y * inv_keep_i : 0.f; }, f1, v) : v);
    };
    for (int k = threadIdx.x * 4; k < F; k += 1024) {
        const float *__restrict__ f1 = ws + g.o_F1 + (size_t)b * T * F + k;
        float4 acc_last = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < a.n_ts; ++j) {
            const float4 xp = ld4(ws + a.o_Xp + ((size_t)j * B + b) * F + k), gx = ld4(ws + a.o_gXp + ((size_t)j * B + b) * F + k);
            float4 open = make_float4(1.f, 1.f, 1.f, 1.f);      // 1 until the window's maximum has been met
            for (int i = 0; i < a.len_ts; ++i) {
                const int f = a.frames[j * a.len_ts + i];
                const float4 v = ld4(f1 + (size_t)f * F);
                const float4 hit = map4([](float o, float x, float m) { return (o != 0.f && x == m) ? 1.f : 0.f; }, open, v, xp);
                open = map4([](float o, float h) { return h != 0.f ? 0.f : o; }, open, hit);
                const float4 val = map4([](float h, float q) { return h != 0.f ? q : 0.f; }, hit, gx);
                if (f == T - 1) acc_last = add4(acc_last, val);
                else put(f, k, v, val);
            }
        }
        for (int f = L; f < T - 1; ++f) put(f, k, ld4(f1 + (size_t)f * F), make_float4(0.f, 0.f, 0.f, 0.f));
        put(T - 1, k, ld4(f1 + (size_t)(T - 1) * F), acc_last);
    }
}

int cell_grid(const Geom &g) { return std::max(1, std::min(2048, (g.B * (g.F / 4) + 255) / 256)); }

}  // namespace

int launch_rnn_pool_fwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(rnn_pool_fwd_kernel, dim3(g.B), dim3(256), 0, stream, g, ptrs, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_rnn_cell_fwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, int t, hipStream_t stream) {
    if (t < 0 || t >= a.n_ts) return -1;
    hipLaunchKernelGGL(rnn_cell_fwd_kernel, dim3(cell_grid(g)), dim3(256), 0, stream, g, ptrs, a, t);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_rnn_cell_bwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, int t, hipStream_t stream) {
    if (t < 0 || t >= a.n_ts) return -1;
    hipLaunchKernelGGL(rnn_cell_bwd_kernel, dim3(cell_grid(g)), dim3(256), 0, stream, g, ptrs, a, t);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_rnn_pool_bwd(const Geom &g, const Ptrs &ptrs, const RnnArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(rnn_pool_bwd_kernel, dim3(g.B), dim3(256), 0, stream, g, ptrs, a, g.o_gHf < 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace ta3n
