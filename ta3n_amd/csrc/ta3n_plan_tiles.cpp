// Plan builder, GEMM launches: Builder::add_gemm_phase turns the GEMM specs of one launch into its tile tasks (tile code -> tile shape
// and stages -> panels -> order over the XCD queues -> side jobs), Builder::end_chain derives the hand-offs of a chained launch.
#include "ta3n_plan_builder.h"

#include <cstdlib>

namespace ta3n {

static int64_t tiles_at(const std::vector<GemmSpec> &specs, int bm, int bn) {
    int64_t n = 0;
    for (auto &g : specs) n += (int64_t)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
    return n;
}

// the tile code this launch is built with: the chain's, the one forced for this launch, its phase_tiles entry or tile_config
int Builder::next_tile_code() {
    if (chaining && chain_levels > 0) { ++gemm_phase_index; return tile_code_of_chain(chain_ph); }   // later level of a chained launch: the tile shape is settled
    if (force_next != 0) { const int code = force_next; force_next = 0; return code; }
    const int i = gemm_phase_index++;
    return i < 16 && p.cfg.phase_tiles[i] != 0 ? p.cfg.phase_tiles[i] : p.cfg.tile_config;
}

// tile shape (waves and blocks per wave) and LDS stages of the launch: decoded from the tile code, or the plan's own choice
Phase Builder::choose_tiles(int group, int forced, const std::vector<GemmSpec> &specs) const {
    int wm = 1, wn = 1, wk = 4;
    // ten-thousands digit: register blocking (bf16 twins only; dropped again for launches that turn out not to read twins,
    // build_plan's retry loop - deny_blocking)
    int blk = forced / 10000;
    forced %= 10000;
    const bool twins_flags = bf16_twins(p.cfg);
    if (!twins_flags || blocking_denied()) blk = 0;
    int forced_stages = forced / 1000;
    forced %= 1000;
    // thousands digit 5 / 6 / 7: HALF stages (64 k per stage: gemm_tiles MODE 5), 2 / 3 / 4 of them - for launches that read plain bf16 twins;
    // dropped again (with the blocking) where a launch turns out not to (build_plan's retry loop)
    bool half_stages = false;
    if (forced_stages >= 5 && forced_stages <= 7) {
        half_stages = twins_flags && !(p.cfg.flags & TA3N_FLAG_F32_SPLIT) && !blocking_denied();
        forced_stages = half_stages ? forced_stages - 3 : 0;
    }
    if (forced != 0) {
        wm = forced / 100; wn = (forced / 10) % 10; wk = forced % 10;
    } else {
        // heuristic from MI355X measurements (tools/proto_gemm.hip, bench.py --autotune):
        // 64x64 tiles with an 8-wave workgroup once they still give every CU a workgroup,
        // otherwise 32x32 tiles, K split 8 ways when there are fewer than two tiles per CU
        // bf16 twins: 128x128 tiles (2 x 2 blocks per wave) once they still give every CU two workgroups - half the operand
        // bytes per flop through the LDS-DMA (measured at the 512+512-video, 9-segment shape: 153 -> 132 us and 89 -> 73 us
        // for the two long launches; with fewer tiles the 64x64 tile's better balance wins)
        if (twins_flags && !blocking_denied() && tiles_at(specs, 128, 128) >= 512) { wm = 2; wn = 2; wk = 2; blk = 3; }
        else if (tiles_at(specs, 64, 64) >= 256) { wm = 2; wn = 2; wk = 2; }
        else if (tiles_at(specs, 32, 32) >= 512) { wm = 1; wn = 1; wk = 4; }
        else { wm = 1; wn = 1; wk = 8; }
    }
    if (blk >= 4) {
        // 192x128 / 256x128 tiles: half-stage kernels of four waves, and only where every A operand is K-contiguous (forward levels,
        // gradients at activations); anywhere else the launch falls back to the plan's own choice
        bool a_kcontig = true;
        for (auto &g : specs) for (auto &sg : g.segs) a_kcontig = a_kcontig && !sg.a_kmajor;
        if (!(half_stages && forced == 221 && forced_stages == 3 && a_kcontig)) {
            half_stages = false; forced_stages = 0;
            if (twins_flags && !blocking_denied() && tiles_at(specs, 128, 128) >= 256) { wm = 2; wn = 2; wk = 2; blk = 3; }
            else { wm = 2; wn = 2; wk = 2; blk = 0; }
        }
    }
    const int rm = blk_rm(blk), rn = blk_rn(blk);
    if (forced_stages == 3 && rm * rn == 4 && !half_stages) forced_stages = 2;   // three 64 KiB stages do not fit
    const int BM = 32 * wm * rm, BN = 32 * wn * rn;
    Phase ph;
    std::memset(&ph, 0, sizeof(ph));
    ph.kind = PH_GEMM; ph.group = group; ph.wm = wm; ph.wn = wn; ph.wk = wk; ph.rm = rm; ph.rn = rn;
    if (p.cfg.flags & (TA3N_FLAG_BF16_MFMA | TA3N_FLAG_F32_SPLIT)) {
        // a third stage pays once every tile streams a long K; short-K launches keep the extra resident workgroup
        int min_k = 1 << 30;
        for (auto &g : specs) {
            int k = 0;
            for (auto &sg : g.segs) k += sg.klen;
            min_k = std::min(min_k, k);
        }
        // ... and the twin kernel's third 128-k stage of a 64x64 tile (3 x 32 KB) costs the CU its second resident workgroup.  For the
        // launches of the UNFUSED sequence (ta3n_forward / ta3n_backward: what the module path runs, each launch on its own) two
        // workgroups on two stages each are faster once there is more than one tile per CU (512+512 videos x 9 segments, shared-FC
        // product, 1 152 tiles: 113 -> 86 us; TRN gradient level: 391 -> 260 us; 128+128 x 12, 384 tiles: 29.5 -> 19.7 us), with at
        // most one tile per CU the third stage is (shared-FC weight gradient, 256 tiles: 46.8 vs 53.5 us).  The launches of the
        // pipelined fused step keep the third stage: the same change measured SLOWER there under bench.py's protocol (configs[4]
        // two-stream 0.497 -> 0.504 ms, three alternating processes each: profiles/r04_half_stage_ab.txt) - a launch timed alone
        // and the same launch between its neighbours with the update's side workgroups aboard are different experiments.
        // TA3N_THIRD_STAGE=always / =residency applies one rule to every launch (A/B).
        const int64_t n_tiles = tiles_at(specs, BM, BN);
        const int64_t twin_stage = (int64_t)(BM + BN) * 256;
        const bool third_costs_a_workgroup = twins_flags && !(p.cfg.flags & TA3N_FLAG_F32_SPLIT) &&
                                             2 * 3 * twin_stage > 160 * 1024 && 2 * 2 * twin_stage <= 160 * 1024;
        static const int third_rule = [] { const char *e = getenv("TA3N_THIRD_STAGE"); return !e ? 0 : std::strcmp(e, "always") == 0 ? 1 : std::strcmp(e, "residency") == 0 ? 2 : 0; }();
        const bool by_residency = third_rule == 2 || (third_rule == 0 && group < 4);
        const bool third = min_k >= 1024 && rm * rn < 4 && !(by_residency && third_costs_a_workgroup && n_tiles > 256);
        ph.bf16 = forced_stages ? forced_stages : (third ? 3 : 2);
        if (p.cfg.flags & TA3N_FLAG_F32_SPLIT) ph.bf16 |= 32;      // split (hi + lo) operands, three MFMAs per product block
        if (half_stages) ph.bf16 |= 64;
    }
    // (fp32 MFMA kernel: two LDS stages only.  A third stage for the launches with one tile per compute unit - shared-FC product and its
    // weight gradient, 256 tiles at the headline shape - was built and measured in round 5: 257.6 -> 260.3 us per step, 265.7 with
    // three stages everywhere; profiles/r05_persistent_ab.txt.  The thousands digit of a tile code is ignored in the fp32 arithmetic.)
    ph.chain_off = -1; ph.chain_n = 0;
    return ph;
}

// split-K: the Segs [0, cut) and [cut, n) of a tile go to two tasks; cut = the boundary that balances the two K sums best
static void push_split_pair(Panel &pn, const GemmSpec &g, const Task &t, int seg_begin, int cost, int pair) {
    int total = 0, best_cut = 1, acc_k = 0, best_diff = 1 << 30;
    for (auto &sg : g.segs) total += sg.klen;
    for (size_t k = 0; k + 1 < g.segs.size(); ++k) {
        acc_k += g.segs[k].klen;
        const int diff = std::abs(2 * acc_k - total);
        if (diff < best_diff) { best_diff = diff; best_cut = (int)k + 1; }
    }
    int k0 = 0;
    for (int k = 0; k < best_cut; ++k) k0 += g.segs[k].klen;
    Task h0 = t, h1 = t;
    h0.epi |= EPI_SPLITK; h1.epi |= EPI_SPLITK;
    h0.seg_count = best_cut; h1.seg_begin = seg_begin + best_cut; h1.seg_count = (int)g.segs.size() - best_cut;
    h0.pad[2] = 1; h1.pad[2] = 2;
    h0.pad[0] = h1.pad[0] = pair;         // (pair id; the ws offsets are assigned once the workspace is laid out)
    h0.cost = cost * k0 / std::max(total, 1); h1.cost = cost - h0.cost;
    pn.tiles.push_back(h0); pn.tiles.push_back(h1);
}

// the specs' Segs go into the plan, their tiles into panels (struct Panel)
std::vector<Panel> Builder::expand_panels(const std::vector<GemmSpec> &specs, int BM, int BN) {
    std::vector<Panel> panels;
    int spec_index = -1;
    for (auto &g : specs) {
        ++spec_index;
        const int seg_begin = (int)p.segs.size();
        int cost = 0;
        for (auto &s : g.segs)   // the kernel selects its K loop by the operand kinds of the task's first Seg
            if (s.a_kmajor != g.segs[0].a_kmajor || s.b_kmajor != g.segs[0].b_kmajor ||
                ((g.proto.epi & EPI_ROWSUM_A) && !(s.a_kmajor && s.b_kmajor)))   // row sums exist in the k-major/k-major loop only
                mixed_kinds = true;
        for (auto &s : g.segs) {
            p.segs.push_back(s);
            // operands the kernel cannot move 16 bytes at a time take the 4-byte LDS-DMA path: such tiles are
            // several times slower per chunk, so they are weighted up and therefore scheduled first
            const int a_rows = s.pad[0] > 0 ? s.pad[0] : g.M;
            const bool a_vec = s.a_kmajor ? ((s.a_off | s.a_ld | a_rows) & 3) == 0 : ((s.a_off | s.a_ld | s.klen) & 3) == 0;
            const bool b_vec = s.b_kmajor ? ((s.b_off | s.b_ld | g.N) & 3) == 0 : ((s.b_off | s.b_ld | s.klen) & 3) == 0;
            int seg_cost = (s.klen + 63) / 64 * 64 * ((a_vec ? 1 : 3) + (b_vec ? 1 : 3)) / 2;
            // cost_model 1 (measured, profiles/r03_chain_handoff_ab.txt: a weight-gradient tile - both operands k-major - streams
            // a k in ~9 ns, the other kinds in ~5.5 ns; every tile pays ~3 us of descriptor fetch + epilogue whatever its K):
            // the XCD queues are balanced on time, not on K
            if (p.cfg.cost_model == 1 && s.a_kmajor && s.b_kmajor) seg_cost = seg_cost * 17 / 10;
            cost += seg_cost;
        }
        if (p.cfg.cost_model == 1) cost += 576;
        // split-K - not for tiles with a bias gradient or a later Seg that rescales the accumulator: that scale would have to
        // apply to the other half's contributions too
        bool spec_can_split = g.split == 2 && g.segs.size() >= 2 && !chaining;
        for (size_t k = 1; k < g.segs.size(); ++k) spec_can_split = spec_can_split && g.segs[k].scale_kind == SK_ONE;
        const bool split_m = g.M >= g.N;
        const int outer = split_m ? g.M : g.N, inner = split_m ? g.N : g.M;
        const int bo = split_m ? BM : BN, bi = split_m ? BN : BM;
        for (int o0 = 0; o0 < outer; o0 += bo) {
            Panel pn;
            pn.cost = 0;
            pn.group = g.affinity >= 0 ? g.affinity : -1 - spec_index;      // (no affinity given: the spec's own panels form a group)
            for (int i0 = 0; i0 < inner; i0 += bi) {
                Task t = g.proto;
                t.m0 = split_m ? o0 : i0; t.n0 = split_m ? i0 : o0;
                t.m_valid = g.M; t.n_valid = g.N;
                t.seg_begin = seg_begin; t.seg_count = (int)g.segs.size();
                if (t.n0 != 0) t.epi &= ~(uint32_t)EPI_ROWSUM_A;   // the bias gradient is written once per row block
                t.cost = cost;
                if (spec_can_split && !(t.epi & (EPI_ROWSUM_A | EPI_SUMSQ))) push_split_pair(pn, g, t, seg_begin, cost, n_split_pairs++);
                else pn.tiles.push_back(t);
                pn.cost += cost;
            }
            panels.push_back(pn);
        }
    }
    return panels;
}

constexpr int NX = 8;      // XCD queues

// xcd_aware 3.  Affinity groups (round 6): the panels of specs that share operand slabs - the row panels of one frame's
// gradient-at-F1 GEMM (same TRN weight slabs), the (scale, position) weight-gradient GEMMs of one scale (same gZ_t), the
// tuple GEMMs of one scale (same W_j) - stay on ONE XCD and run back to back, so that XCD's L2 fetches the shared slab once
// for all of them instead of once per panel wherever it landed.  A group heavier than ~0.45 of an XCD's fair share is cut into
// chunks of consecutive panels; chunks go heaviest first onto the least loaded queue, preferring a queue that already holds
// a chunk of the same group when that costs less than half a chunk of balance.
static void deal_affinity_groups(const std::vector<Panel> &panels, std::vector<std::vector<Task>> &q) {
    std::vector<int64_t> load(NX, 0);
    int64_t total = 0;
    for (auto &pn : panels) total += pn.cost;
    const int64_t limit = std::max<int64_t>(1, total * 45 / (100 * NX));
    struct Chunk { std::vector<int> panels; int64_t cost; int group; int64_t tile_cost; };
    std::vector<Chunk> chunks;
    std::vector<int> order;                       // group ids in order of first appearance
    for (auto &pn : panels) if (std::find(order.begin(), order.end(), pn.group) == order.end()) order.push_back(pn.group);
    for (int gid : order) {
        Chunk ck{{}, 0, gid, 0};
        for (int i = 0; i < (int)panels.size(); ++i) {
            if (panels[i].group != gid) continue;
            if (!ck.panels.empty() && ck.cost + panels[i].cost > limit) { chunks.push_back(ck); ck = Chunk{{}, 0, gid, 0}; }
            ck.panels.push_back(i);
            ck.cost += panels[i].cost;
            for (auto &t : panels[i].tiles) ck.tile_cost = std::max<int64_t>(ck.tile_cost, t.cost);
        }
        if (!ck.panels.empty()) chunks.push_back(ck);
    }
    std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &a, const Chunk &b) { return a.cost > b.cost; });
    std::vector<std::vector<int>> held(NX);       // chunk indices per queue
    for (int ci = 0; ci < (int)chunks.size(); ++ci) {
        int best = 0;
        for (int x = 1; x < NX; ++x) if (load[x] < load[best]) best = x;
        for (int x = 0; x < NX; ++x) {
            bool same = false;
            for (int h : held[x]) same = same || chunks[h].group == chunks[ci].group;
            if (same && load[x] <= load[best] + chunks[ci].cost / 2) { best = x; break; }
        }
        held[best].push_back(ci);
        load[best] += chunks[ci].cost;
    }
    for (int x = 0; x < NX; ++x) {                // per queue: chunks with the longest tiles first, a group's chunks adjacent
        std::stable_sort(held[x].begin(), held[x].end(), [&](int a, int b) {
            if (chunks[a].tile_cost != chunks[b].tile_cost) return chunks[a].tile_cost > chunks[b].tile_cost;
            return chunks[a].group < chunks[b].group;
        });
        for (int h : held[x]) for (int i : chunks[h].panels) for (auto &t : panels[i].tiles) q[x].push_back(t);
    }
}

// the launch's task order: workgroup b runs on XCD b % 8, so the queues are interleaved
std::vector<Task> Builder::order_tiles(std::vector<Panel> &panels) const {
    std::vector<Task> local;
    if (p.cfg.xcd_aware == 2) {
        for (auto &pn : panels) for (auto &t : pn.tiles) local.push_back(t);
        std::stable_sort(local.begin(), local.end(), [](const Task &a, const Task &b) { return a.cost > b.cost; });
        return local;
    }
    std::vector<std::vector<Task>> q(NX);
    if (p.cfg.xcd_aware == 3) {
        deal_affinity_groups(panels, q);
    } else {
        std::vector<int64_t> load(NX, 0);
        std::stable_sort(panels.begin(), panels.end(), [](const Panel &a, const Panel &b) { return a.cost > b.cost; });
        for (auto &pn : panels) {   // heaviest panel first onto the least loaded XCD queue
            int best = 0;
            for (int x = 1; x < NX; ++x) if (load[x] < load[best]) best = x;
            for (auto &t : pn.tiles) q[best].push_back(t);
            load[best] += pn.cost;
        }
        for (auto &v : q) std::stable_sort(v.begin(), v.end(), [](const Task &a, const Task &b) { return a.cost > b.cost; });
    }
    size_t depth = 0;
    for (auto &v : q) depth = std::max(depth, v.size());
    Task nop;
    std::memset(&nop, 0, sizeof(nop));   // seg_count == 0: the workgroup exits immediately
    nop.c_base = BASE_NONE; nop.bias_base = BASE_NONE; nop.aux_base = BASE_NONE; nop.add_base = BASE_NONE;
    // (affinity groups leave queues of very different LENGTH - one of many short tiles beside seven of few long ones.  Padding the
    // short queues with empty workgroups keeps "workgroup b runs on XCD b % 8" exact, but only pays while most queues still have
    // tiles: once fewer than half do, the rest is appended unpadded and spreads over all XCDs - short tiles, balance over locality.)
    size_t padded_depth = depth;
    if (p.cfg.xcd_aware == 3) {
        std::vector<size_t> sizes;
        for (auto &v : q) sizes.push_back(v.size());
        std::sort(sizes.begin(), sizes.end());
        padded_depth = sizes[NX / 2];      // depth at which half of the queues have run out
    }
    for (size_t d = 0; d < padded_depth; ++d)
        for (int x = 0; x < NX; ++x) local.push_back(d < q[x].size() ? q[x][d] : nop);
    while (!local.empty() && local.back().seg_count == 0) local.pop_back();
    for (size_t d = padded_depth; d < depth; ++d)
        for (int x = 0; x < NX; ++x) if (d < q[x].size()) local.push_back(q[x][d]);
    return local;
}

// the pending 8-column sum and the pending non-tile tasks ride with this launch
void Builder::attach_side_jobs(std::vector<Task> &local) {
    if (sum8[0] >= 0 && !local.empty()) {
        // on the LAST task of the list - a real tile (trailing padding was popped) and the launch's lightest, so the side job's
        // dependent loads sit under the other tiles.  (Until round 5 it rode on local[0], the HEAVIEST tile: ~1.5 us on the critical
        // path of the relation-level backward launch.)
        Task &host = local.back();
        host.epi |= EPI_SUMROWS8;
        host.pad[0] = sum8[0]; host.pad[1] = sum8[1]; host.pad[2] = sum8[2];
        sum8[0] = -1;
    }
    // the short side tasks go right behind the first tile: they finish under the tiles instead of extending the launch's tail
    local.insert(local.begin() + (local.empty() ? 0 : 1), side_tasks.begin(), side_tasks.end());
    side_tasks.clear();
}

void Builder::add_gemm_phase(int group, std::vector<GemmSpec> &specs) {
    Phase ph = choose_tiles(group, next_tile_code(), specs);
    ph.task_begin = (int32_t)p.tasks.size();
    std::vector<Panel> panels = expand_panels(specs, 32 * ph.wm * ph.rm, 32 * ph.wn * ph.rn);
    std::vector<Task> local = order_tiles(panels);
    attach_side_jobs(local);
    if (chaining) {
        if (chain_levels == 0) { chain_ph = ph; chain_ph.group = group; }
        ++chain_levels;
        for (auto &t : local) { t.sig = -1; chain_tasks.push_back(t); }
        return;
    }
    for (auto &t : local) { t.sig = -1; p.tasks.push_back(t); }
    ph.task_count = (int32_t)local.size();
    p.phases.push_back(ph);
}

// ---------------------------------------------------------------------------------------------------------------------
// Chained launches: who waits for whom.  Every task's writes and reads are laid out as element intervals per buffer (the
// twins mirror their originals element for element, so this runs on the original offsets, before add_bf16_twins); a task
// depends on every EARLIER task of the launch whose writes overlap its reads.  Producers with the same set of consumers share
// one counter (target = their number), a consumer's wait list names the counters of its producers.  A later task overwriting
// what an earlier one reads or writes would be a race inside one launch: reported as an error (such levels must stay launches).
struct Ival { int64_t lo, hi; int task; };

static void tile_rows(std::vector<Ival> &out, int64_t off, int64_t ld, int r0, int nr, int c0, int nc, int task) {
    for (int r = r0; r < r0 + nr; ++r) out.push_back(Ival{off + (int64_t)r * ld + c0, off + (int64_t)r * ld + c0 + nc, task});
}

std::string Builder::end_chain() {
    chaining = false;
    Phase ph = chain_ph;
    const int BM = 32 * ph.wm * std::max(ph.rm, 1), BN = 32 * ph.wn * std::max(ph.rn, 1);
    const int n = (int)chain_tasks.size();
    std::vector<Ival> wr[BASE_COUNT], rd[BASE_COUNT];
    auto operand = [&](std::vector<Ival> &out, int off, int ld, int kmajor, int r0, int rows_valid, int tile_rows_n, int klen, int task) {
        const int nr = std::min(tile_rows_n, rows_valid - r0);
        if (nr <= 0) return;
        if (!kmajor) tile_rows(out, off, ld, r0, nr, 0, klen, task);
        else for (int k = 0; k < klen; ++k) out.push_back(Ival{off + (int64_t)k * ld + r0, off + (int64_t)k * ld + r0 + nr, task});
    };
    for (int i = 0; i < n; ++i) {
        const Task &t = chain_tasks[i];
        if (t.epi & EPI_SGD) {            // optimiser side job: writes the parameters [4 pad0, 4 pad1) (reads gradients / norm partials of earlier launches)
            wr[BASE_P].push_back(Ival{4ll * t.pad[0], 4ll * t.pad[1], i});
            continue;
        }
        if (t.epi & EPI_COLSUM) {
            tile_rows(rd[BASE_WS], t.pad[0], t.pad[2], 0, t.pad[1], t.n0, t.n_valid - t.n0, i);
            wr[t.c_base].push_back(Ival{(int64_t)t.c_off + t.n0, (int64_t)t.c_off + t.n_valid, i});
            if (t.epi & EPI_SUMSQ) wr[BASE_WS].push_back(Ival{t.pad[3], t.pad[3] + 1, i});
            continue;
        }
        if (t.seg_count == 0) continue;
        if (t.epi & EPI_SUMROWS8) {
            rd[BASE_WS].push_back(Ival{t.pad[1], t.pad[1] + 8ll * t.pad[2], i});
            wr[BASE_WS].push_back(Ival{t.pad[0], t.pad[0] + 8, i});
        }
        const int nr = std::min(BM, t.m_valid - t.m0), nc = std::min(BN, t.n_valid - t.n0);
        for (int k = t.seg_begin; k < t.seg_begin + t.seg_count; ++k) {
            const Seg &sg = p.segs[k];
            operand(rd[sg.a_base], sg.a_off, sg.a_ld, sg.a_kmajor, t.m0, sg.pad[0] > 0 ? sg.pad[0] : t.m_valid, BM, sg.klen, i);
            operand(rd[sg.b_base], sg.b_off, sg.b_ld, sg.b_kmajor, t.n0, t.n_valid, BN, sg.klen, i);
        }
        if (t.epi & EPI_BIAS) rd[t.bias_base].push_back(Ival{(int64_t)t.bias_off + t.n0, (int64_t)t.bias_off + t.n0 + nc, i});
        if (t.epi & EPI_MASK) tile_rows(rd[t.aux_base], t.aux_off, t.aux_ld, t.m0, nr, t.n0, nc, i);
        if (t.epi & EPI_ADD) tile_rows(rd[t.add_base], t.add_off, t.add_ld, t.m0, nr, t.n0, nc, i);
        for (int f = 0; f < t.fan_count; ++f) {
            tile_rows(rd[BASE_WS], t.fan_mask_off[f], t.fan_ld, t.m0, nr, t.n0, nc, i);
            tile_rows(wr[BASE_WS], t.fan_out_off[f], t.fan_ld, t.m0, nr, t.n0, nc, i);
        }
        tile_rows(wr[t.c_base], t.c_off, t.c_ld, t.m0, nr, t.n0, nc, i);
        if (t.epi & EPI_ROWSUM_A) wr[t.bias_base].push_back(Ival{(int64_t)t.bias_off + t.m0, (int64_t)t.bias_off + t.m0 + nr, i});
        if (t.epi & EPI_SUMSQ) wr[BASE_WS].push_back(Ival{t.pad[3], t.pad[3] + 1, i});
    }
    std::vector<std::vector<int>> consumers(n), producers(n);
    for (int b = 0; b < BASE_COUNT; ++b) {
        auto &w = wr[b];
        std::sort(w.begin(), w.end(), [](const Ival &a, const Ival &c) { return a.lo < c.lo; });
        for (size_t k = 1; k < w.size(); ++k)
            if (w[k].lo < w[k - 1].hi && w[k].task != w[k - 1].task)
                return "chained launch: tasks " + std::to_string(w[k - 1].task) + " and " + std::to_string(w[k].task) + " write the same elements";
        for (const Ival &r : rd[b]) {
            // writers are sorted and disjoint: the first one that can overlap ends after r.lo
            size_t k = std::lower_bound(w.begin(), w.end(), r.lo, [](const Ival &a, int64_t v) { return a.hi <= v; }) - w.begin();
            for (; k < w.size() && w[k].lo < r.hi; ++k) {
                if (w[k].task == r.task) continue;
                if (w[k].task > r.task)
                    return "chained launch: task " + std::to_string(w[k].task) + " overwrites what the earlier task " + std::to_string(r.task) + " reads";
                producers[r.task].push_back(w[k].task);
            }
        }
    }
    for (int i = 0; i < n; ++i) {
        auto &v = producers[i];
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        for (int j : v) consumers[j].push_back(i);      // (i ascending: the lists come out sorted)
    }
    std::vector<std::pair<std::vector<int>, int>> groups;   // (consumer set, counter)
    std::vector<int> target;
    for (int j = 0; j < n; ++j) {
        if (consumers[j].empty()) continue;
        int c = -1;
        for (auto &gp : groups)
            if (gp.first == consumers[j]) { c = gp.second; break; }
        if (c < 0) { c = (int)target.size(); groups.push_back({consumers[j], c}); target.push_back(0); }
        ++target[c];
        chain_tasks[j].sig = c;
    }
    for (int i = 0; i < n; ++i) {
        std::vector<int> cs;
        for (int j : producers[i]) cs.push_back(chain_tasks[j].sig);
        std::sort(cs.begin(), cs.end());
        cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
        chain_tasks[i].wait_begin = (int32_t)p.waits.size();
        chain_tasks[i].wait_count = (int32_t)cs.size();
        for (int c : cs) p.waits.push_back(Wait{c, target[c]});
    }
    ph.chain_n = (int32_t)target.size();
    ph.chain_off = (int32_t)add_region("chain" + std::to_string(p.phases.size()), 2 + ph.chain_n);
    ph.task_begin = (int32_t)p.tasks.size();
    ph.task_count = n;
    for (auto &t : chain_tasks) p.tasks.push_back(t);
    p.phases.push_back(ph);
    chain_tasks.clear();
    return "";
}

}  // namespace ta3n
