// The score kernel of TA3N_FLAG_SCORE_ONLY plans (gfx950, wave64): from the aggregated feature to class probabilities, ranks and the
// validation metrics of main.validate / test_models.py (reference main.py:707-735, 809-822; test_models.py:155-198) in ONE launch behind
// the plan's launch list (ta3n_score).
//
// One wave per video, four videos per workgroup, a grid over the n videos of the call.
//   front end, trn-m: R_j = sum of scale j's tuple activations (lane-resident, as pool_fwd_kernel forms it), with TA3N_FLAG_TRANS_ATTN
//     Pr_j = W2_j Hr_j + b2_j and w_j = 1 - H(softmax(Pr_j)) (attn_weight: the one copy of the rule), without it w_j = 0 and Hr is never
//     read; V = sum_j (1 + w_j) R_j.  Other aggregations: V is what their last launch left in region "V", any width.
//   body: Y = Wcv V + bcv (C <= 64, lane c = class c), lane_log_softmax, prob = e / sum, ce = -log_softmax[label], rank and argmax in
//     torch.topk order (ties: the lower class index is ahead) - eval_metrics_kernel's rules.
//   ending: lane 0 of every wave publishes {ce, rank, pred} of its video, the workgroup takes a ticket, and the workgroup that draws the last
//     one adds the n values in video order to "metrics" and counts "confusion": no float atomics, no dependence on which workgroup is
//     last or when.  Rows at and past n are never touched.
#include <hip/hip_runtime.h>

#include "ta3n_kernels.h"
#include "../../include/ta3n_hip.h"

using namespace ta3n;

namespace {

constexpr int SCORE_WAVES = 4;

// Q > 0: trn-m with NB = 64 Q (V in registers, channel q * 64 + lane); Q == 0: V from region "V", a.width floats per row
template <int Q>
__global__ __launch_bounds__(64 * SCORE_WAVES) void score_kernel(Geom g, Ptrs ptrs, ScoreArgs a, int n, int reset) {
    __shared__ int last_flag;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * SCORE_WAVES + wv;
    float *__restrict__ ws = ptrs.ws;
    const int C = g.C, W = a.width;
    const int *__restrict__ labels = reinterpret_cast<const int *>(ws + g.o_labels);
    float *__restrict__ ce_out = ws + a.o_ce;
    int *__restrict__ rank_out = reinterpret_cast<int *>(ws + a.o_rank);
    int *__restrict__ pred_out = reinterpret_cast<int *>(ws + a.o_pred);
    if (b < n) {      // (uniform per wave)
        float *__restrict__ vrow = ws + g.o_V + (size_t)b * W;
        float vacc[Q > 0 ? Q : 1];
        if (Q > 0) {
            const int *__restrict__ tf = reinterpret_cast<const int *>(ws + g.o_tuple_first);
            const int NB = 64 * Q, NR = g.n_rel, NT = g.n_tuples;
            const bool attn_on = (g.flags & TA3N_FLAG_TRANS_ATTN) != 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) vacc[q] = 0.f;
            for (int j = 0; j < NR; ++j) {
                float w = 0.f;
                if (attn_on) {
                    const float *__restrict__ W2 = ptrs.p + g.p_W2_0 + (size_t)j * g.p_W2_stride;
                    const float *__restrict__ b2 = ptrs.p + g.p_b2_0 + (size_t)j * g.p_b2_stride;
                    const float *__restrict__ hr = ws + g.o_Hr + ((size_t)b * NR + j) * NB;
                    float d0 = 0.f, d1 = 0.f;
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const int c = q * 64 + lane;
                        const float h = hr[c];
                        d0 = fmaf(h, W2[c], d0);
                        d1 = fmaf(h, W2[NB + c], d1);
                    }
                    d0 = wave_allreduce_sum(d0) + b2[0];
                    d1 = wave_allreduce_sum(d1) + b2[1];
                    w = attn_weight(soft2(d0, d1));
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int c = q * 64 + lane;
                    float r = 0.f;
                    for (int t = tf[j]; t < tf[j + 1]; ++t) r += ws[g.o_Zr + ((size_t)b * NT + t) * NB + c];
                    vacc[q] += attn_on ? (w + 1.f) * r : r;
                }
                if (lane == 0) ws[g.o_attn + (size_t)b * NR + j] = w;
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) vrow[q * 64 + lane] = vacc[q];
        }
        // Y = Wcv V + bcv, the lanes over the channels, lane c keeps class c.  A chunk of V (NV channels per lane) is held in registers and
        // the classifier rows of CB classes are requested together: one round trip per CB classes and chunk, not one per class and 64 channels
        constexpr int NV = Q > 0 ? Q : 8, CB = 4;
        const float *__restrict__ Wcv = ptrs.p + g.p_Wcv;
        float y = 0.f;
        for (int k0 = 0; k0 < W; k0 += 64 * NV) {      // (trn-m: one chunk, W = 64 Q)
            float v[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int k = k0 + i * 64 + lane;
                v[i] = Q > 0 ? vacc[Q > 0 ? i : 0] : (k < W ? vrow[k] : 0.f);
            }
            for (int c0 = 0; c0 < C; c0 += CB) {
                float w[CB][NV];
#pragma unroll
                for (int j = 0; j < CB; ++j)
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const int k = k0 + i * 64 + lane;
                        w[j][i] = (c0 + j < C && k < W) ? Wcv[(size_t)(c0 + j) * W + k] : 0.f;
                    }
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    float acc = 0.f;
#pragma unroll
                    for (int i = 0; i < NV; ++i) acc = fmaf(v[i], w[j][i], acc);
                    acc = wave_allreduce_sum(acc);
                    if (lane == c0 + j) y += acc;
                }
            }
        }
        if (lane < C) y += ptrs.p[g.p_bcv + lane];
        const bool on = lane < C;
        const int lab = labels[b];
        const LaneSoft sm = lane_log_softmax(on ? y : -INFINITY, on);
        const float ylab = wave_allreduce_sum(lane == lab ? y : 0.f);
        // rank of the label among the logits, torch.topk order; argmax with the same tie rule: the lowest class that attains the maximum
        const float ahead = wave_allreduce_sum((on && (y > ylab || (y == ylab && lane < lab))) ? 1.f : 0.f);
        float amin = (on && y == sm.m) ? (float)lane : 1e9f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) amin = fminf(amin, __shfl_xor(amin, off, 64));
        if (on) {
            ws[g.o_Y + (size_t)b * C + lane] = y;
            ws[a.o_prob + (size_t)b * C + lane] = sm.e / sm.sum;
        }
        if (lane == 0) {      // what the last workgroup reads: written through to memory (agent-scope atomic stores)
            __hip_atomic_store(ce_out + b, -(ylab - sm.m - sm.ls), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(rank_out + b, (int)ahead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(pred_out + b, amin < (float)C ? (int)amin : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ticket: stores done -> barrier -> one agent-scope release -> fetch_add; the workgroup that draws the last ticket acquires and sums
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int *ticket = reinterpret_cast<int *>(ws + a.o_ticket);
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = drawn == (int)gridDim.x - 1 ? 1 : 0;
        if (last_flag) {
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last_flag) return;
    int *__restrict__ conf = reinterpret_cast<int *>(ws + g.o_confusion);
    if (reset)
        for (int i = threadIdx.x; i < C * C; i += 64 * SCORE_WAVES) conf[i] = 0;
    __syncthreads();
    for (int v = threadIdx.x; v < n; v += 64 * SCORE_WAVES) {
        const int lab = labels[v], pred = __hip_atomic_load(pred_out + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)lab < (unsigned)C && (unsigned)pred < (unsigned)C) atomicAdd(&conf[lab * C + pred], 1);
    }
    if (wv == 0) {      // lane l adds videos l, l + 64, ... in order, then the lanes in the order of the DPP network: one order, whoever is last
        float ce = 0.f, t1 = 0.f, t5 = 0.f;
        for (int v = lane; v < n; v += 64) {
            ce += __hip_atomic_load(ce_out + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int r = __hip_atomic_load(rank_out + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t1 += r < 1 ? 1.f : 0.f;
            t5 += r < 5 ? 1.f : 0.f;
        }
        ce = wave_allreduce_sum(ce); t1 = wave_allreduce_sum(t1); t5 = wave_allreduce_sum(t5);
        if (lane < 4) {
            const float add = lane == 0 ? ce : lane == 1 ? t1 : lane == 2 ? t5 : (float)n;
            ws[g.o_metrics + lane] = (reset ? 0.f : ws[g.o_metrics + lane]) + add;
        }
    }
}

}  // namespace

namespace ta3n {

int launch_score(const Geom &g, const Ptrs &ptrs, const ScoreArgs &a, int n, int reset, hipStream_t stream) {
    if (g.C < 1 || g.C > 64 || a.o_prob < 0 || a.width < 1 || n < 0 || n > g.B) return -1;
    const dim3 grid(n > 0 ? (n + SCORE_WAVES - 1) / SCORE_WAVES : 1), block(64 * SCORE_WAVES);      // (n == 0: one workgroup, for `reset`)
    if (!a.trn) hipLaunchKernelGGL((score_kernel<0>), grid, block, 0, stream, g, ptrs, a, n, reset);
    else {
        if (a.width != g.NB) return -1;
        switch (g.NB / 64) {
            case 1: hipLaunchKernelGGL((score_kernel<1>), grid, block, 0, stream, g, ptrs, a, n, reset); break;
            case 2: hipLaunchKernelGGL((score_kernel<2>), grid, block, 0, stream, g, ptrs, a, n, reset); break;
            case 4: hipLaunchKernelGGL((score_kernel<4>), grid, block, 0, stream, g, ptrs, a, n, reset); break;
            case 8: hipLaunchKernelGGL((score_kernel<8>), grid, block, 0, stream, g, ptrs, a, n, reset); break;
            default: return -1;
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace ta3n
