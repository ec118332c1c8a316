// The training meters of TA3N_FLAG_TRAIN_METERS plans (gfx950, wave64): what main.train logs every print_freq steps (reference
// main.py:564-617: Prec@1 / Prec@5 of the source batch and the running averages of the loss terms) kept on the device, in ONE launch
// behind the step's launch list, accumulated across steps in regions "meter_counts" (int32) and "meter_sums" (float64).
//
// A bandwidth-bound reduction over Bs x C class logits and at most B (T - 1) + B + B T rows of two domain logits.  Work items are waves:
//   source videos: one wave per video, lane c = class c (C <= 64): rank of the label in torch.topk order, eval_metrics_kernel's rule;
//   domain rows:   per counted level 64 rows per wave, one lane per row; the prediction is target iff logit[1] > logit[0].
// A grid of up to METER_MAX_WG workgroups of four waves walks the items with a grid stride, every wave keeps its counts in registers
// (wave-uniform: ballots and wave sums), the workgroup adds them up in LDS and issues one integer atomic per non-zero count.
// Integer atomics commute: the result does not depend on their order, and no float is added by an atomic.
//   ending: the workgroup takes a ticket; the one that draws the last counts the step, adds the six loss slots to their float64 sums (one
//     thread, slot order) and moves the step's own three accuracy numbers from the scratch words to the last-step words.  Every word that
//     crosses workgroups inside the launch (scratch, ticket) is touched by agent-scope read-modify-write atomics only, and a workgroup's
//     adds have returned (vmcnt(0), barrier) before its ticket add is issued - no plain load ever reads another workgroup's data.
//   a step whose total loss is not finite counts as a step and as a non-finite step and adds nothing else: every workgroup sees that from
//     losses[0] (written by an earlier launch) and skips its items.
// The launch writes its two regions and nothing else.
#include <hip/hip_runtime.h>

#include "ta3n_kernels.h"
#include "../../include/ta3n_hip.h"

using namespace ta3n;

namespace {

constexpr int METER_WAVES = 4;
constexpr int METER_MAX_WG = 512;
constexpr int N_ACC = 3 + 12;      // source rows, top-1, top-5; then [level][domain]{rows, correct}

struct MeterItems { int n_src, n_lv[3], total; };      // wave items: source videos, then 64-row groups of each counted level

__host__ __device__ inline MeterItems meter_items(const Geom &g, const MetersArgs &a) {
    MeterItems it;
    it.n_src = g.Bs;
    const int64_t rows[3] = {(int64_t)g.B * g.n_rel, (int64_t)g.B, (int64_t)g.B * g.T};
    it.total = it.n_src;
    for (int l = 0; l < 3; ++l) {
        it.n_lv[l] = ((a.levels >> l) & 1) ? (int)((rows[l] + 63) / 64) : 0;
        it.total += it.n_lv[l];
    }
    return it;
}

__global__ __launch_bounds__(64 * METER_WAVES) void train_meters_kernel(Geom g, Ptrs ptrs, MetersArgs a) {
    __shared__ int acc[N_ACC];
    __shared__ int last_flag;
    float *__restrict__ ws = ptrs.ws;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const Hyper *__restrict__ hy = reinterpret_cast<const Hyper *>(ws + g.o_hyper);
    const int *__restrict__ labels = reinterpret_cast<const int *>(ws + g.o_labels);
    int *__restrict__ cnt = reinterpret_cast<int *>(ws + a.o_counts);
    const float *__restrict__ L = ws + g.o_losses;
    const bool finite = isfinite(L[0]);
    const int vs = hy->valid_source, vt = hy->valid_target;
    if (threadIdx.x < N_ACC) acc[threadIdx.x] = 0;
    __syncthreads();
    if (finite) {
        const MeterItems it = meter_items(g, a);
        const int C = g.C;
        int mine[N_ACC];      // (wave-uniform)
#pragma unroll
        for (int i = 0; i < N_ACC; ++i) mine[i] = 0;
        for (int item = blockIdx.x * METER_WAVES + wv; item < it.total; item += gridDim.x * METER_WAVES) {
            if (item < it.n_src) {
                const int b = item;
                if (b >= vs) continue;      // (the reference's dummy rows)
                const bool on = lane < C;
                const float y = on ? ws[g.o_Y + (size_t)b * C + lane] : -INFINITY;
                const int lab = labels[b];
                const float ylab = wave_allreduce_sum(lane == lab ? y : 0.f);
                const int ahead = __popcll(__ballot(on && (y > ylab || (y == ylab && lane < lab))));
                mine[0] += 1;
                mine[1] += ahead < 1 ? 1 : 0;
                mine[2] += ahead < 5 ? 1 : 0;
                continue;
            }
            int k = item - it.n_src, l = 0;
            if (k >= it.n_lv[0]) { k -= it.n_lv[0]; l = 1; if (k >= it.n_lv[1]) { k -= it.n_lv[1]; l = 2; } }      // (item < total: k ends inside level l)
            const int per = l == 0 ? g.n_rel : l == 1 ? 1 : g.T;   // rows per video
            const int64_t n_rows = (int64_t)g.B * per, row = (int64_t)k * 64 + lane;
            const int o = l == 0 ? g.o_Pr : l == 1 ? g.o_Pv : g.o_Pf;
            bool src = false, valid = false, tgt_pred = false;
            if (row < n_rows) {
                const int b = (int)(row / per);
                src = b < g.Bs;
                valid = video_valid(g.Bs, vs, vt, b);
                const float2 z = *reinterpret_cast<const float2 *>(ws + o + row * 2);
                tgt_pred = z.y > z.x;      // (a tie predicts source)
            }
            const int c[4] = {(int)__popcll(__ballot(valid && src)), (int)__popcll(__ballot(valid && src && !tgt_pred)),
                              (int)__popcll(__ballot(valid && !src)), (int)__popcll(__ballot(valid && !src && tgt_pred))};
#pragma unroll
            for (int ll = 0; ll < 3; ++ll)      // (constant indices: the counts stay in registers)
#pragma unroll
                for (int j = 0; j < 4; ++j) mine[3 + ll * 4 + j] += ll == l ? c[j] : 0;
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < N_ACC; ++i)
                if (mine[i]) atomicAdd(&acc[i], mine[i]);
        }
        __syncthreads();
        if (threadIdx.x < N_ACC) {
            const int v = acc[threadIdx.x];
            if (v) {
                const int i = threadIdx.x;
                __hip_atomic_fetch_add(cnt + (i < 3 ? MT_ROWS + i : MT_DOMAIN + (i - 3)), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (i < 3) __hip_atomic_fetch_add(cnt + MT_CUR + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // ticket: this workgroup's adds have returned -> barrier -> fetch_add; the workgroup that draws the last ticket closes the step
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int drawn = __hip_atomic_fetch_add(cnt + MT_TICKET, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = drawn == (int)gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!last_flag || threadIdx.x != 0) return;
    __hip_atomic_exchange(cnt + MT_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    cnt[MT_STEPS] += 1;
    if (!finite) { cnt[MT_NONFINITE] += 1; return; }
    for (int i = 0; i < 3; ++i) cnt[MT_LAST_ROWS + i] = __hip_atomic_exchange(cnt + MT_CUR + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double *__restrict__ sums = reinterpret_cast<double *>(ws + a.o_sums);
    for (int i = 0; i < 6; ++i) sums[i] += (double)L[i];
}

}  // namespace

namespace ta3n {

int launch_train_meters(const Geom &g, const Ptrs &ptrs, const MetersArgs &a, hipStream_t stream) {
    if (a.o_counts < 0 || a.o_sums < 0 || (a.o_sums & 1) || g.C < 1 || g.C > 64) return -1;
    const int items = meter_items(g, a).total;
    const dim3 grid(std::max(1, std::min(METER_MAX_WG, (items + METER_WAVES - 1) / METER_WAVES))), block(64 * METER_WAVES);
    hipLaunchKernelGGL(train_meters_kernel, grid, block, 0, stream, g, ptrs, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace ta3n
