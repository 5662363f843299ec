// The compact self-play replay ring (include/ipp_engine.h, ipp_replay_compact): a ring row keeps what its network input is a function
// of -- the H history entries, the map mean at record time, the episode it belongs to -- instead of the planes [C][N][N] themselves
// (replay_buffers.py:48-101 loads them from a pickle; episode_generators.py:157-192 writes them), and an ended episode's factor columns are
// kept ONCE, in a spare engine slot behind the envs, for all of its rows.  The planes are built when a minibatch is drawn.  The kernels:
//   k_rc_record    one workgroup per env, before the search: the env's history entries into its ring row (entry 0's rank made explicit,
//                  every valid entry's slot replaced by the archive slot the running episode will get), its current mean, the episode tag
//   k_rc_archive   after the budget step, before the commit: workgroups of envs whose episode did not end exit at once; the others copy
//                  the columns [0, r_last) of the env slot, their spans and rectangles and the ENDED episode's prior pair into the archive slot, rank
//                  r_last + 1 (every sample of the episode is a strict prefix: k_feature_planes.h, plane_diag).  What makes the copy
//                  valid AFTER the step's reset: wave_reset_env (ipp_common.h) leaves the column storage alone.
//   k_rc_evict     the archive slot of episode p held episode p - E: the env's ring rows still tagged p - E lose their flag (counted),
//                  then the env's episode counter moves on
//   k_rc_entries   a minibatch's ring rows -> n x H plane entries + mask means [n][N] for one ipp_feature_planes call
//   k_rc_crop      the augmented copies c >= 1 from the originals states[0:n] (ReplicationPad2d(4) + the crop: k_selfplay.h)
// Copy and crop are bandwidth kernels: 16-byte accesses, vector stores only.
#pragma once
#include "ipp_common.h"
#include "ipp_host.h"
#include "k_selfplay.h"

namespace ipp {

// archive slot of episode p of env e on an engine whose slots [0, B) are the envs
__device__ __forceinline__ int rc_archive_slot(int B, int E, int e, long long p) { return B + e * E + (int)(p % E); }

__device__ __forceinline__ bool rc_ended(const ipp_selfplay& sp, int e) { return sp.done[e] != 0 || sp.forced[e] != 0; }

__global__ __launch_bounds__(256) void k_rc_record(ipp_selfplay sp, ipp_replay_compact rc, FactorSlots fs, long long step,
                                                   const ipp_plane_entry* __restrict__ entries) {
    const int e = blockIdx.x, B = sp.num_envs, H = rc.history, N = fs.N;
    if (e >= B) return;
    const size_t row = (size_t)(step % sp.slots) * B + e;
    const long long p = rc.episodes[e];
    const int r_now = fs.rank[e];
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
        ipp_plane_entry x = entries[(size_t)e * H + h];
        if (x.valid) {
            x.root_env = rc_archive_slot(B, rc.archive_episodes, e, p);
            if (h == 0) x.rank = r_now;  // (-1 = "the slot's current rank" would name the archive's)
        }
        rc.r_entries[row * H + h] = x;
    }
    const float* src = fs.mean + (size_t)e * fs.Npad;  // (the slab's rows are 16-byte aligned: wave_reset_env stores them as float4)
    float* dst = rc.r_mean + row * N;
    if ((N & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int c = threadIdx.x; c < N / 4; c += blockDim.x) d4[c] = s4[c];
    } else {
        for (int c = threadIdx.x; c < N; c += blockDim.x) dst[c] = src[c];
    }
    if (threadIdx.x == 0) {
        rc.r_episode[row] = p;
        rc.last_rank[e] = r_now;
    }
}

// grid (chunks, B): the columns of env blockIdx.y in float4 strides over the chunks; chunk 0 also the metadata
__global__ __launch_bounds__(256) void k_rc_archive(ipp_selfplay sp, ipp_replay_compact rc, FactorSlots fs) {
    const int e = blockIdx.y, B = sp.num_envs;
    if (e >= B || !rc_ended(sp, e)) return;
    const int dst = rc_archive_slot(B, rc.archive_episodes, e, rc.episodes[e]);
    if (dst >= fs.cap) return;
    int r = rc.last_rank[e];
    r = r < 0 ? 0 : (r > fs.rank_cap ? fs.rank_cap : r);
    const size_t n4 = (size_t)r * fs.pstride / 4;  // (a stored column is pstride floats, a multiple of 16)
    const float4* cs = reinterpret_cast<const float4*>(fs.cov + (size_t)e * fs.cov_slot);
    float4* cd = reinterpret_cast<float4*>(fs.cov + (size_t)dst * fs.cov_slot);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) cd[i] = cs[i];
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < r; k += blockDim.x) {
            fs.colspan[(size_t)dst * fs.rank_cap + k] = fs.colspan[(size_t)e * fs.rank_cap + k];
            fs.colrect[(size_t)dst * fs.rank_cap + k] = fs.colrect[(size_t)e * fs.rank_cap + k];
        }
        if (threadIdx.x == 0) {
            // the prior of the episode that ENDED.  With the config's prior in every episode that is the slot's pair.  With per-episode
            // priors (ipp_set_budget_prior) the step's reset has already installed the next episode's pair in the slot (depth 0, the episode
            // counter advanced: ledger_close), and the ended episode's is drawn again from its index -- the same number, prior_start
            double sv = fs.prior[2 * e + 0], ls = fs.prior[2 * e + 1];
            if (fs.prior_shuffle && fs.led_depth[e] == 0)
                prior_start(fs.sv0, fs.ls0, fs.prior_seed, fs.prior_row_offset, e, fs.led_episode[e] - 1, sv, ls);
            fs.prior[2 * dst + 0] = sv;
            fs.prior[2 * dst + 1] = ls;
            fs.rank[dst] = r + 1;  // never stepped: the field only bounds the prefixes, and keeps every sample off the slot's stored diag
        }
    }
}

// one wave per env, behind k_rc_archive
__global__ __launch_bounds__(64) void k_rc_evict(ipp_selfplay sp, ipp_replay_compact rc) {
    const int e = blockIdx.x, lane = threadIdx.x, B = sp.num_envs, S = sp.slots;
    if (e >= B || !rc_ended(sp, e)) return;
    const long long p = rc.episodes[e], old = p - rc.archive_episodes;
    int n = 0;
    if (old >= 0) {
        for (int s = lane; s < S; s += 64) {
            const size_t row = (size_t)s * B + e;
            if (sp.r_flags[row] != 0 && rc.r_episode[row] == old) {
                sp.r_flags[row] = 0;
                ++n;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __syncthreads();  // (every lane has read the counter)
    if (lane == 0) {
        if (n) atomicAdd(reinterpret_cast<unsigned long long*>(rc.evicted), (unsigned long long)n);
        rc.episodes[e] = p + 1;
    }
}

// output row o: the entries and the mean of ring row index[o]; outside the ring (-1: an empty draw) an entry no engine can evaluate
// (NaN planes, like the dense gather's)
__global__ __launch_bounds__(256) void k_rc_entries(ipp_replay_compact rc, long long cap, int N, int n, const int64_t* __restrict__ index,
                                                    ipp_plane_entry* __restrict__ ent, float* __restrict__ mean) {
    const int o = blockIdx.x, H = rc.history;
    if (o >= n) return;
    long long row = index[o];
    if (row < 0 || row >= cap) row = -1;
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
        ipp_plane_entry x;
        if (row >= 0) {
            x = rc.r_entries[(size_t)row * H + h];
        } else {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            x.root_env = -1; x.rank = 0; x.valid = 1; x.reserved = 0;
            for (int j = 0; j < IPP_TREE_DEPTH; ++j) x.path[j] = -1;
            for (int q = 0; q < 3; ++q) x.position[q] = nan;
            x.budget = nan;
        }
        ent[(size_t)o * H + h] = x;
    }
    float* dst = mean + (size_t)o * N;
    if (row >= 0 && (N & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(rc.r_mean + (size_t)row * N);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int c = threadIdx.x; c < N / 4; c += blockDim.x) d4[c] = s4[c];
    } else {
        for (int c = threadIdx.x; c < N; c += blockDim.x) dst[c] = row >= 0 ? rc.r_mean[(size_t)row * N + c] : 0.f;
    }
}

// block b: channel b % C of output row n + b / C = copy c >= 1 of draw i, from states[i] (g.planes == g.states: rows [0, n) are read,
// rows [n, n copies) written), shifted by the copy's offsets as ipp_replay_gather drew them
__global__ __launch_bounds__(256) void k_rc_crop(SpGather g, const int32_t* __restrict__ offsets) {
    const long long b = blockIdx.x;
    const int o = g.n + (int)(b / g.C), ch = (int)(b % g.C);
    const int copy = o / g.n, i = o % g.n;
    const int oi = min(max(offsets[2 * copy], 0), 8), oj = min(max(offsets[2 * copy + 1], 0), 8);
    sp_gather_plane(g, i, o, ch, oi, oj);
}

}  // namespace ipp
