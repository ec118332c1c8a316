// TA3N_AGG_TEMCONV: the temporal-convolution frame aggregator (reference models.py:44-56, 228-243, 654-672).  tcl_3_1 is a
// Conv2d(1, 1, (3, 1), padding (1, 0)) over the segment axis of the frame features - three scalar taps w0 w1 w2 and one scalar bias c,
// shared by every channel, zero rows outside 0 .. T-1 - followed by ReLU and the mean over the segments:
//     Z_t = w0 F1[t-1] + w1 F1[t] + w2 F1[t+1] + c,   V = (1/T) sum_t relu(Z_t),   Vd = dropout_v(V)
// Three kernels, all fp32 and bandwidth-bound.  A thread moves four channels as one 16-byte access (F % 4 == 0: avgpool_dims_refusal)
// and walks the segments with a sliding window in registers, so every F1 row is read once per pass and Z is never stored: the way
// back recomputes it, by the same tc_z - the same fused multiply-adds in the same order - so both passes see the same ReLU mask.
// The four parameter gradients are sums over every video, segment and channel: each workgroup reduces its video's share in a fixed
// order (lanes, then the four waves through LDS) into "tc_part", and a one-workgroup launch adds the videos in a fixed order.  No
// floating-point atomics: the same step twice gives the same bits.
#include "ta3n_kernels.h"

namespace ta3n {
namespace {

__device__ __forceinline__ float4 ld4(const float *__restrict__ p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *__restrict__ p, const float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

struct Taps { float w0, w1, w2, c; };
__device__ __forceinline__ Taps load_taps(const float *__restrict__ P, const TemconvArgs &a) {
    return Taps{P[a.p_w], P[a.p_w + 1], P[a.p_w + 2], P[a.p_b]};
}
// the one place Z is formed (forward and backward must agree on its sign bit for bit)
__device__ __forceinline__ float tc_z(const Taps &w, float lo, float mid, float hi) { return fmaf(w.w2, hi, fmaf(w.w1, mid, fmaf(w.w0, lo, w.c))); }
__device__ __forceinline__ float relu(float z) { return z > 0.f ? z : 0.f; }

// One workgroup per video.  Window: F1[t-1], F1[t], F1[t+1].  Also clears the eight loss slots the loss kernel accumulates into, as
// pool_avg_fwd_kernel (the launch this one replaces) does; dropout_v's element id is b * F + k, the same mask stream.
__global__ __launch_bounds__(256) void temconv_fwd_kernel(Geom g, Ptrs ptrs, TemconvArgs a) {
    float *__restrict__ ws = ptrs.ws;
    const Hyper *__restrict__ hy = reinterpret_cast<const Hyper *>(ws + g.o_hyper);
    const int b = blockIdx.x, F = g.F, T = g.T;
    const Taps w = load_taps(ptrs.p, a);
    const bool drop_v = hy->train != 0 && hy->p_drop_v > 0.f;
    const float inv_keep_v = hyper_scale(hy, SK_INV_KEEP_V), inv_T = 1.f / (float)T, p_v = hy->p_drop_v;
    const uint32_t seed_v = hy->seed_v;
    if (blockIdx.x == 0 && threadIdx.x < 8) ws[g.o_losses + threadIdx.x] = 0.f;
    for (int k = threadIdx.x * 4; k < F; k += 1024) {
        const float *__restrict__ f1 = ws + g.o_F1 + (size_t)b * T * F + k;
        float4 lo = zero4(), mid = ld4(f1), acc = zero4();
        for (int t = 0; t < T; ++t) {
            const float4 hi = t + 1 < T ? ld4(f1 + (size_t)(t + 1) * F) : zero4();
            acc.x += relu(tc_z(w, lo.x, mid.x, hi.x)); acc.y += relu(tc_z(w, lo.y, mid.y, hi.y));
            acc.z += relu(tc_z(w, lo.z, mid.z, hi.z)); acc.w += relu(tc_z(w, lo.w, mid.w, hi.w));
            lo = mid; mid = hi;
        }
        const float4 v = make_float4(acc.x * inv_T, acc.y * inv_T, acc.z * inv_T, acc.w * inv_T);
        st4(ws + g.o_V + (size_t)b * F + k, v);
        float4 vd = v;
        if (drop_v) {
            const uint32_t id = (uint32_t)(b * F + k);
            vd.x *= keep_mask(seed_v, id, p_v) * inv_keep_v; vd.y *= keep_mask(seed_v, id + 1, p_v) * inv_keep_v;
            vd.z *= keep_mask(seed_v, id + 2, p_v) * inv_keep_v; vd.w *= keep_mask(seed_v, id + 3, p_v) * inv_keep_v;
        }
        st4(ws + g.o_Vd + (size_t)b * F + k, vd);
    }
}

// one channel of one step s of the way back: gR_s from the window (F1[s-1], F1[s], F1[s+1]) and its share of the four parameter sums
__device__ __forceinline__ float tc_back(const Taps &w, float gs, float lo, float mid, float hi, float (&sum)[4]) {
    const float gr = tc_z(w, lo, mid, hi) > 0.f ? gs : 0.f;
    sum[0] = fmaf(gr, lo, sum[0]); sum[1] = fmaf(gr, mid, sum[1]); sum[2] = fmaf(gr, hi, sum[2]); sum[3] += gr;
    return gr;
}
__device__ __forceinline__ float tc_gf(const Taps &w, float gr_next, float gr, float gr_prev) { return fmaf(w.w2, gr_prev, fmaf(w.w1, gr, w.w0 * gr_next)); }

// One workgroup per video.  gV = gVt (it carries dropout_v's mask and scale already) plus, with TA3N_FLAG_FEATURE_GRADS, the caller's;
// gR_t = gV / T [Z_t > 0];  gF1[t] = w0 gR[t+1] + w1 gR[t] + w2 gR[t-1], zeros outside 0 .. T-1.  Step s forms gR_s from F1[s-1 .. s+1]
// and writes row s - 1, which needs gR[s-2 .. s]: five rows of F1 stand behind every output row, three of them and two gR rows are
// in registers.  direct: no live frame discriminator - the result IS gZ1 = gF1 [F1 > 0] / keep_i; otherwise it is the additive base
// ("gRa") of the launch that forms gZ1.  The two modes of pool_avg_bwd_kernel.
__global__ __launch_bounds__(256) void temconv_bwd_kernel(Geom g, Ptrs ptrs, TemconvArgs a, int direct) {
    __shared__ float red[4][4];
    float *__restrict__ ws = ptrs.ws;
    const Hyper *__restrict__ hy = reinterpret_cast<const Hyper *>(ws + g.o_hyper);
    const int b = blockIdx.x, F = g.F, T = g.T;
    const Taps w = load_taps(ptrs.p, a);
    const float inv_T = 1.f / (float)T, inv_keep_i = hyper_scale(hy, SK_INV_KEEP_I);
    float *__restrict__ out = ws + (direct ? g.o_gZ1 : g.o_gRa) + (size_t)b * T * F;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = threadIdx.x * 4; k < F; k += 1024) {
        const float *__restrict__ f1 = ws + g.o_F1 + (size_t)b * T * F + k;
        float4 gv = ld4(ws + g.o_gVt + (size_t)b * F + k);
        if (g.o_gV_ext > 0) {
            const float4 e = ld4(ws + g.o_gV_ext + (size_t)b * F + k);
            gv.x += e.x; gv.y += e.y; gv.z += e.z; gv.w += e.w;
        }
        const float4 gs = make_float4(gv.x * inv_T, gv.y * inv_T, gv.z * inv_T, gv.w * inv_T);
        float4 lo = zero4(), mid = ld4(f1), hi = T > 1 ? ld4(f1 + F) : zero4();
        float4 gr_pp = zero4(), gr_p = zero4();      // gR[s-2], gR[s-1]
        for (int s = 0; s <= T; ++s) {
            float4 gr = zero4();
            if (s < T) {
                gr.x = tc_back(w, gs.x, lo.x, mid.x, hi.x, sum); gr.y = tc_back(w, gs.y, lo.y, mid.y, hi.y, sum);
                gr.z = tc_back(w, gs.z, lo.z, mid.z, hi.z, sum); gr.w = tc_back(w, gs.w, lo.w, mid.w, hi.w, sum);
            }
            if (s >= 1) {                            // row s - 1; lo = F1[s-1]
                float4 gf = make_float4(tc_gf(w, gr.x, gr_p.x, gr_pp.x), tc_gf(w, gr.y, gr_p.y, gr_pp.y),
                                        tc_gf(w, gr.z, gr_p.z, gr_pp.z), tc_gf(w, gr.w, gr_p.w, gr_pp.w));
                if (direct) {
                    gf.x = lo.x > 0.f ? gf.x * inv_keep_i : 0.f; gf.y = lo.y > 0.f ? gf.y * inv_keep_i : 0.f;
                    gf.z = lo.z > 0.f ? gf.z * inv_keep_i : 0.f; gf.w = lo.w > 0.f ? gf.w * inv_keep_i : 0.f;
                }
                st4(out + (size_t)(s - 1) * F + k, gf);
            }
            gr_pp = gr_p; gr_p = gr;
            lo = mid; mid = hi;
            hi = s + 2 < T ? ld4(f1 + (size_t)(s + 2) * F) : zero4();
        }
    }
    // this video's share of d w0, d w1, d w2, d c: lanes, then the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s = wave_allreduce_sum(sum[j]);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) ws[a.o_part + (size_t)b * 4 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// d tcl_3_1.conv2d.weight[j] = sum_b tc_part[b][j], d bias = sum_b tc_part[b][3].  One workgroup: thread i adds rows i, i + 256, ... in
// order (in double: B terms of either sign), then a fixed tree over the 256 threads.  Thread 0 also leaves the four gradients' sum of
// squares in the plan's last "sumsq" slot, where the fused optimiser's norm expects every gradient that no tile wrote.
__global__ __launch_bounds__(256) void temconv_wgrad_kernel(Geom g, Ptrs ptrs, TemconvArgs a) {
    __shared__ double red[4][256];
    const float *__restrict__ part = ptrs.ws + a.o_part;
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < g.B; b += 256) {
        const float4 v = ld4(part + (size_t)b * 4);
        acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[j][tid] += red[j][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float d0 = (float)red[0][0], d1 = (float)red[1][0], d2 = (float)red[2][0], dc = (float)red[3][0];
        ptrs.g[a.p_w] = d0; ptrs.g[a.p_w + 1] = d1; ptrs.g[a.p_w + 2] = d2; ptrs.g[a.p_b] = dc;
        if (a.o_sumsq >= 0) ptrs.ws[a.o_sumsq] = fmaf(dc, dc, fmaf(d2, d2, fmaf(d1, d1, d0 * d0)));
    }
}

}  // namespace

int launch_temconv_fwd(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(temconv_fwd_kernel, dim3(g.B), dim3(256), 0, stream, g, ptrs, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_temconv_bwd(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(temconv_bwd_kernel, dim3(g.B), dim3(256), 0, stream, g, ptrs, a, g.o_gHf < 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_temconv_wgrad(const Geom &g, const Ptrs &ptrs, const TemconvArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(temconv_wgrad_kernel, dim3(1), dim3(256), 0, stream, g, ptrs, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace ta3n
