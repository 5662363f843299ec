// Classic MCTS for a batch, the tree itself (planning/mcts_mission.py of the reference: Node.uct / select_child :24-66, progressive
// widening :263-272, simulate :274-304, select_best_child :341-351) in device tables: all roots advance one simulation at a time in
// lock step, with no host read between the first simulation and the chosen waypoints (ipp_ctree_search, ipp_engine.hip).
// Tables per root, cap = simulations + 1 node slots, slot 0 = the root; a simulation adds at most one node, in ascending slot order, so
// the children of a node are the slots with parent == node in ascending order = creation order.  The kernels:
//   k_ctree_descend  one wave per root: _simulate / _widen / select_child iteratively from slot 0 -- ends at a terminal node, at a node
//                    never visited (its row of the rollout state is written) or at a node that widens (its row of the expansion state)
//   k_ctree_attach   one thread per root: the expansion's recorded step becomes slot count++, then simulate(child, ..) = terminal or the
//                    child's rollout row
//   k_ctree_backup   one thread per root: the rollout's value into the leaf, then up the recorded path as simulate unwinds (undiscounted,
//                    the double increment of every traversed non-root node kept)
//   k_ctree_best     one wave per root: the first child of slot 0 with the largest value_sum / visits
// fp64 without fused multiply-adds, no atomics, sums in a stated order, lowest index wins (k_rollout.h); the geometry and the cost are
// k_rollout.h's device functions.  Every loop is bounded by a launch constant (horizon, cap, kmax); every slot index read from a table
// is range-checked before it is used as an address, an out-of-range value sets err and ends that root's search; a root with err != 0
// is skipped by every kernel (descend still clears the `live` of its two state rows, so that nothing rolls on for it).
#pragma once
#include "k_rollout.h"

namespace ipp {

__device__ __forceinline__ double ctree_wp(const ipp_ctree& ct, int i, int node, int q) {
    return node == 0 ? ct.root_wp[3 * i + q] : ct.action[((size_t)i * ct.cap + node) * 3 + q];
}

// a row of an ipp_rollout state at the tree node `node` (MCTSMission.rollout / the expansion policy start there, charging from its waypoint)
__device__ __forceinline__ void ctree_write_row(const ipp_ctree& ct, const ipp_rollout& st, int i, int node, int plen, double budget,
                                                int depth_left) {
    st.root[i] = ct.root_slot[i];
    for (int d = 0; d < kTreeDepth; ++d) st.path[(size_t)i * kTreeDepth + d] = d < plen ? ct.path[((size_t)i * ct.cap + node) * kTreeDepth + d] : -1;
    st.plen[i] = plen;
    for (int q = 0; q < 3; ++q) {
        const double w = ctree_wp(ct, i, node, q);
        st.cur[3 * i + q] = w;
        st.charge_from[3 * i + q] = w;
    }
    st.budget[i] = budget;
    st.depth_left[i] = depth_left;
    st.value[i] = 0.0;
    st.disc[i] = 1.0;
    st.live[i] = 1;
    st.flag[i] = IPP_ROLLOUT_RUNNING;
}

// Node.uct + the cost bar of select_child for child slot s of `node` (visits v > 0), children's values in [lo, hi]
__device__ __forceinline__ double ctree_uct(const ipp_ctree& ct, int i, int s, double logv, double lo, double hi, double nx, double ny, double nz,
                                            double budget, bool flight, double vmax, double amax) {
#pragma clang fp contract(off)
    const size_t o = (size_t)i * ct.cap + s;
    const int cv = ct.visits[o];
    double u;
    if (cv == 0) {
        u = INFINITY;
    } else {
        const double value = ct.value_sum[o] / (double)cv;
        const double expl = ct.c * sqrt(logv / (double)cv);
        if (hi == 0.0) u = value + expl;
        else if (hi == lo) u = value / hi + expl;
        else u = (value - lo / (hi - lo)) + expl;  // (the reference's precedence, :52)
    }
    const double cost = rollout_cost(ct.action[3 * o + 0], ct.action[3 * o + 1], ct.action[3 * o + 2], nx, ny, nz, flight, vmax, amax);
    if (cost == 0.0 || cost >= budget) u = -INFINITY;
    return u;
}

__global__ __launch_bounds__(64) void k_ctree_descend(ipp_ctree ct, ipp_rollout ex, ipp_rollout ro) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= ct.roots) return;
    if (ct.err[i] != 0) {
        if (lane == 0) { ex.live[i] = 0; ro.live[i] = 0; }
        return;
    }
    const int cap = ct.cap, horizon = ct.horizon, kmax = ro.kmax;
    const size_t base = (size_t)i * cap;
    const int* parent = ct.parent + base;
    const int* visits = ct.visits + base;
    const double* value_sum = ct.value_sum + base;
    const bool flight = (ro.flags & IPP_USE_FLIGHT_TIME) != 0;
    const int count = ct.count[i];
    int fail = (count < 1 || count > cap) ? IPP_CTREE_ERR_RANGE : 0;
    double budget = ct.root_budget[i];
    int depth = horizon, node = 0, kind = IPP_CTREE_TERMINAL, tlen = 0;
    if (lane == 0 && !fail)
        for (int q = 0; q < 3; ++q) ct.action[base * 3 + q] = ct.root_wp[3 * i + q];  // (the table's record of the root; read through ctree_wp)
    for (int lvl = 0; lvl <= horizon && !fail; ++lvl) {
        if (lane == 0) ct.t_slot[(size_t)i * (horizon + 1) + lvl] = node;
        tlen = lvl + 1;
        if (depth == 0 || budget < ro.resolution) { kind = IPP_CTREE_TERMINAL; break; }
        const int v = visits[node];
        if (v == 0) { kind = IPP_CTREE_ROLLOUT; break; }
        if (v < 0 || v >= ct.thr_len) { fail = IPP_CTREE_ERR_RANGE; break; }
        const double nx = ctree_wp(ct, i, node, 0), ny = ctree_wp(ct, i, node, 1), nz = ctree_wp(ct, i, node, 2);
        // get_next_actions_mask(node.action, budget).sum() (:167-173) over the candidate square
        int n_av = 0;
        for (int k0 = 0; k0 < kmax; k0 += 64) {
            const int j = k0 + lane;
            bool av = false;
            if (j < kmax) {
                double x, y, z;
                if (rollout_candidate(ro, j, nx, ny, nz, x, y, z)) {
                    const double c = rollout_cost(x, y, z, nx, ny, nz, flight, ro.vmax, ro.amax);
                    av = c > 0.0 && c <= budget;
                }
            }
            n_av += __popcll(__ballot(av));
        }
        // the node's children and the range of their values
        int nch = 0;
        double lo = INFINITY, hi = -INFINITY;
        for (int k0 = 0; k0 < count; k0 += 64) {
            const int s = k0 + lane;
            const bool ch = s >= 1 && s < count && parent[s] == node;
            if (ch && visits[s] > 0) {
                const double val = value_sum[s] / (double)visits[s];
                lo = fmin(lo, val);
                hi = fmax(hi, val);
            }
            nch += __popcll(__ballot(ch));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, o, 64));
            hi = fmax(hi, __shfl_xor(hi, o, 64));
        }
        // RolloutPolicy.widen; thr[v] = k v^alpha from the host's fp64 table
        if (nch == 0 || ((double)nch <= ct.thr[v] && nch < n_av)) { kind = IPP_CTREE_EXPAND; break; }
        // select_child: the children whose UCT equals the largest one (a NaN never does), child number min(floor(u ties), ties - 1) of them
        const double logv = log((double)v);
        double m = -INFINITY;
        bool has = false;
        for (int k0 = 0; k0 < count; k0 += 64) {
            const int s = k0 + lane;
            if (s >= 1 && s < count && parent[s] == node) {
                const double u = ctree_uct(ct, i, s, logv, lo, hi, nx, ny, nz, budget, flight, ro.vmax, ro.amax);
                if (u == u) { has = true; m = u > m ? u : m; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        if (!__any(has)) { fail = IPP_CTREE_ERR_SELECT; break; }
        int ties = 0;
        for (int k0 = 0; k0 < count; k0 += 64) {
            const int s = k0 + lane;
            const bool tie = s >= 1 && s < count && parent[s] == node &&
                             ctree_uct(ct, i, s, logv, lo, hi, nx, ny, nz, budget, flight, ro.vmax, ro.amax) == m;
            ties += __popcll(__ballot(tie));
        }
        long long pick = (long long)(ct.tie_u[(size_t)i * horizon + lvl] * (double)ties);
        pick = pick < ties - 1 ? pick : ties - 1;
        pick = pick < 0 ? 0 : pick;
        int chosen = -1, seen = 0;
        for (int k0 = 0; k0 < count && chosen < 0; k0 += 64) {
            const int s = k0 + lane;
            const bool tie = s >= 1 && s < count && parent[s] == node &&
                             ctree_uct(ct, i, s, logv, lo, hi, nx, ny, nz, budget, flight, ro.vmax, ro.amax) == m;
            unsigned long long b = __ballot(tie);
            const int c = __popcll(b);
            if (pick < seen + c) {
                for (int r = (int)pick - seen; r > 0; --r) b &= b - 1;  // drop the r lowest ties
                chosen = k0 + (int)__ffsll((long long)b) - 1;
            }
            seen += c;
        }
        if (chosen < 1 || chosen >= count) { fail = IPP_CTREE_ERR_SELECT; break; }
        budget = budget - rollout_cost(ctree_wp(ct, i, chosen, 0), ctree_wp(ct, i, chosen, 1), ctree_wp(ct, i, chosen, 2), nx, ny, nz, flight,
                                       ro.vmax, ro.amax);
        depth -= 1;
        node = chosen;
    }
    if (lane != 0) return;
    int plen = 0;
    if (!fail && kind != IPP_CTREE_TERMINAL) {
        plen = ct.plen[base + node];
        if (plen < 0 || plen > kTreeDepth) fail = IPP_CTREE_ERR_RANGE;
    }
    ex.live[i] = 0;
    ro.live[i] = 0;
    if (fail) { ct.err[i] = fail; return; }
    ct.t_len[i] = tlen;
    ct.leaf_kind[i] = kind;
    ct.leaf_budget[i] = budget;
    ct.leaf_depth[i] = depth;
    if (kind == IPP_CTREE_ROLLOUT) ctree_write_row(ct, ro, i, node, plen, budget, depth);
    else if (kind == IPP_CTREE_EXPAND) ctree_write_row(ct, ex, i, node, plen, budget, 1);
}

__global__ __launch_bounds__(64) void k_ctree_attach(ipp_ctree ct, ipp_rollout ex, ipp_rollout ro) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ct.roots || ct.err[i] != 0 || ct.leaf_kind[i] != IPP_CTREE_EXPAND) return;
    const int cap = ct.cap, horizon = ct.horizon;
    const size_t base = (size_t)i * cap;
    const int L = ct.t_len[i], count = ct.count[i];
    if (L < 1 || L > horizon || count < 1 || count > cap) { ct.err[i] = IPP_CTREE_ERR_RANGE; return; }
    const int node = ct.t_slot[(size_t)i * (horizon + 1) + L - 1];
    if (node < 0 || node >= count) { ct.err[i] = IPP_CTREE_ERR_RANGE; return; }
    if (ex.live[i] == 0) {
        // nothing reachable where the reference raises inside np.random.choice(0): no child, the node counts as the terminal case
        if (ex.flag[i] == IPP_ROLLOUT_NO_ACTION) ct.leaf_kind[i] = IPP_CTREE_TERMINAL;
        else ct.err[i] = IPP_CTREE_ERR_PICK | (ex.flag[i] << 8);
        return;
    }
    const int st = ex.step_status[i];
    if (st != IPP_STATUS_OK) { ct.err[i] = IPP_CTREE_ERR_STEP | (st << 8); return; }  // (RANK_FULL included: the host path raises there)
    if (count >= cap) { ct.err[i] = IPP_CTREE_ERR_FULL; return; }
    const int pl = ct.plen[base + node];
    if (pl < 0 || pl >= kTreeDepth) { ct.err[i] = IPP_CTREE_ERR_RANGE; return; }
    const int c = count, new_id = ex.new_id[i];
    ct.parent[base + c] = node;
    ct.dev[base + c] = new_id;
    for (int d = 0; d < kTreeDepth; ++d) ct.path[(base + c) * kTreeDepth + d] = d < pl ? ct.path[(base + node) * kTreeDepth + d] : d == pl ? new_id : -1;
    ct.plen[base + c] = pl + 1;
    const double ax = ex.action[3 * i + 0], ay = ex.action[3 * i + 1], az = ex.action[3 * i + 2];
    ct.action[(base + c) * 3 + 0] = ax; ct.action[(base + c) * 3 + 1] = ay; ct.action[(base + c) * 3 + 2] = az;
    ct.visits[base + c] = 0;
    ct.value_sum[base + c] = 0.0;
    ct.edge_reward[base + c] = (double)ex.step_reward[i];
    ct.count[i] = c + 1;
    ct.t_slot[(size_t)i * (horizon + 1) + L] = c;
    ct.t_len[i] = L + 1;
    // simulate(child, budget - cost(child.action, node.action), depth - 1)
    const double budget = ct.leaf_budget[i] - rollout_cost(ax, ay, az, ctree_wp(ct, i, node, 0), ctree_wp(ct, i, node, 1), ctree_wp(ct, i, node, 2),
                                                           (ro.flags & IPP_USE_FLIGHT_TIME) != 0, ro.vmax, ro.amax);
    const int depth = ct.leaf_depth[i] - 1;
    ct.leaf_budget[i] = budget;
    ct.leaf_depth[i] = depth;
    if (depth <= 0 || budget < ro.resolution) { ct.leaf_kind[i] = IPP_CTREE_TERMINAL; return; }
    ct.leaf_kind[i] = IPP_CTREE_ROLLOUT;
    ctree_write_row(ct, ro, i, c, pl + 1, budget, depth);
}

__global__ __launch_bounds__(64) void k_ctree_backup(ipp_ctree ct, ipp_rollout ro) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ct.roots || ct.err[i] != 0) return;
    const int cap = ct.cap, horizon = ct.horizon;
    const size_t base = (size_t)i * cap;
    const int L = ct.t_len[i], count = ct.count[i], kind = ct.leaf_kind[i];
    if (L < 1 || L > horizon + 1 || count < 1 || count > cap || (kind != IPP_CTREE_TERMINAL && kind != IPP_CTREE_ROLLOUT)) {
        ct.err[i] = IPP_CTREE_ERR_RANGE;
        ro.live[i] = 0;
        return;
    }
    const int* trace = ct.t_slot + (size_t)i * (horizon + 1);
    for (int j = 0; j < L; ++j)
        if (trace[j] < 0 || trace[j] >= count) { ct.err[i] = IPP_CTREE_ERR_RANGE; ro.live[i] = 0; return; }
    double value = 0.0;
    if (kind == IPP_CTREE_ROLLOUT) {
        const int flag = ro.flag[i];
        if (flag == IPP_ROLLOUT_ERR_FOOTPRINT || flag == IPP_ROLLOUT_ERR_NAN || flag == IPP_ROLLOUT_ERR_STEP) {
            ct.err[i] = IPP_CTREE_ERR_ROLLOUT | (flag << 8);
            ro.live[i] = 0;
            return;
        }
        const int leaf = trace[L - 1];
        value = ro.value[i];
        ct.visits[base + leaf] = ct.visits[base + leaf] + 1;
        ct.value_sum[base + leaf] = ct.value_sum[base + leaf] + value;
    }
    for (int j = L - 2; j >= 0; --j) {  // simulate unwinding (:286-301)
        const int node = trace[j], child = trace[j + 1];
        value = ct.edge_reward[base + child] + value;
        ct.visits[base + node] = ct.visits[base + node] + 1;
        ct.visits[base + child] = ct.visits[base + child] + 1;
        ct.value_sum[base + node] = ct.value_sum[base + node] + value;
    }
}

__global__ __launch_bounds__(64) void k_ctree_best(ipp_ctree ct, double* __restrict__ out_action, int* __restrict__ out_has) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= ct.roots) return;
    const size_t base = (size_t)i * ct.cap;
    const int count = ct.count[i];
    int best = -1;
    if (ct.err[i] == 0 && count >= 1 && count <= ct.cap) {
        double bv = -INFINITY;  // this lane's first maximiser over its slots, ascending
        int bi = 0x7fffffff;
        for (int k0 = 0; k0 < count; k0 += 64) {
            const int s = k0 + lane;
            if (s >= 1 && s < count && ct.parent[base + s] == 0 && ct.visits[base + s] > 0) {  // (no search leaves a child unvisited)
                const double val = ct.value_sum[base + s] / (double)ct.visits[base + s];
                if (val > bv || (bi == 0x7fffffff && val == bv)) { bv = val; bi = s; }
            }
        }
        double m = bv;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        int idx = (bi != 0x7fffffff && bv == m) ? bi : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) idx = min(idx, __shfl_xor(idx, o, 64));
        best = idx != 0x7fffffff ? idx : -1;
    }
    if (lane != 0) return;
    for (int q = 0; q < 3; ++q) out_action[3 * i + q] = best >= 0 ? ct.action[(base + best) * 3 + q] : ct.root_wp[3 * i + q];
    out_has[i] = best >= 0 ? 1 : 0;
}

}  // namespace ipp
