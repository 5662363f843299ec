// Episode reset, ground-truth generation, state copies, materialisation, metrics and RNG kernels.
#pragma once
#include "ipp_common.h"

namespace ipp {

// mean <- 0.5, diag <- sigma^2, rank <- 0, prior <- (sigma^2, l); optional ground-truth install.
// mapping/mappings.py:235-240,259-261.
struct InitAction { double p[3]; };  // Mission.init_action (planning/missions.py:69), by value

__global__ void k_reset_small(View v, const int* __restrict__ env_ids, int n_items,
                              const double* __restrict__ prior_scale, const float* __restrict__ gt_in,
                              double* __restrict__ prev_out, InitAction init) {
    const int item = blockIdx.y;
    if (item >= n_items) return;
    const int env = env_ids ? env_ids[item] : item;
    if (env < 0 || env >= v.cap) return;
    double sv = prior_scale ? prior_scale[2 * item + 0] : v.sv0;
    double ls = prior_scale ? prior_scale[2 * item + 1] : v.ls0;
    // a length scale the column window was not sized for (ipp_config.fixed_prior): fail loudly, not inaccurately
    if (v.ls_max > 0.0 && ls > v.ls_max * (1.0 + 1e-12)) sv = ls = NAN;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell == 0) {
        v.rank[env] = 0;
        v.prior[2 * env + 0] = sv;
        v.prior[2 * env + 1] = ls;
        if (prev_out)
            for (int k = 0; k < 3; ++k) prev_out[3 * env + k] = init.p[k];
    }
    if (cell >= v.Npad) return;
    const bool valid = cell < v.N;
    v.mean[(size_t)env * v.Npad + cell] = valid ? (isnan(sv) ? NAN : 0.5f) : 0.f;
    v.diag[(size_t)env * v.Npad + cell] = valid ? (float)sv : 0.f;
    if (gt_in) gt_plane(v, env)[cell] = valid ? gt_in[(size_t)item * v.N + cell] : 0.f;
}

// ipp_step_autoreset behind the step kernels that do not reset in-kernel: item i resets its env when ar.src[i] >= 0.
__global__ void k_reset_flagged(View v, const int* __restrict__ env_ids, int n_items, AutoReset ar) {
    const int item = blockIdx.y;
    if (item >= n_items) return;
    const int k = ar.src[item];
    if (k < 0) return;
    const int env = env_ids ? env_ids[item] : item;
    if (env < 0 || env >= v.cap) return;
    double sv = ar.prior ? ar.prior[2 * k + 0] : v.sv0, ls = ar.prior ? ar.prior[2 * k + 1] : v.ls0;
    if (v.ls_max > 0.0 && ls > v.ls_max * (1.0 + 1e-12)) sv = ls = NAN;  // (like k_reset_small)
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell == 0) {
        v.rank[env] = 0;
        // a flip without a staged field (only this thread looks at / takes the flag): the env's prior becomes NaN -- every later
        // step of the episode then reports IPP_STATUS_NOT_PD and a NaN reward instead of observing a stale plane
        const bool stale = !ar.gt && v.gt_slot[v.cap + env] == 0;
        v.prior[2 * env + 0] = stale ? NAN : sv;
        v.prior[2 * env + 1] = stale ? NAN : ls;
        if (ar.prev)
            for (int j = 0; j < 3; ++j) ar.prev[3 * env + j] = ar.init[j];
        if (!ar.gt) {  // (the new ground truth was staged into the alternate plane: no other thread reads the slot here)
            v.gt_slot[env] = gt_alt_slot(v, env);
            v.gt_slot[v.cap + env] = 0;
        }
    }
    if (cell >= v.Npad) return;
    const bool valid = cell < v.N;
    v.mean[(size_t)env * v.Npad + cell] = valid ? (isnan(sv) ? NAN : 0.5f) : 0.f;
    v.diag[(size_t)env * v.Npad + cell] = valid ? (float)sv : 0.f;
    if (ar.gt) gt_plane(v, env)[cell] = valid ? ar.gt[(size_t)k * v.N + cell] : 0.f;
}

// ipp_read_prior: the (sigma^2, l) pairs of n slots as one 16-byte vector store each; a slot outside the engine reads NaN
__global__ __launch_bounds__(256) void k_read_prior(View v, const int* __restrict__ env_ids, int n, double2* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int env = env_ids ? env_ids[i] : i;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    out[i] = (env >= 0 && env < v.cap) ? make_double2(v.prior[2 * env + 0], v.prior[2 * env + 1]) : make_double2(nan, nan);
}

// ipp_read_gt / ipp_write_gt: the env's CURRENT ground-truth plane (the slot lives on the device)
__global__ void k_copy_gt(View v, int env, float* __restrict__ out, const float* __restrict__ in) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.N) return;
    if (out) out[i] = gt_plane(v, env)[i];
    else gt_plane(v, env)[i] = in[i];
}

__global__ void k_init_gt_slots(View v) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.cap) { v.gt_slot[e] = e; v.gt_slot[v.cap + e] = 0; }
}

// Dense state: P <- Matern prior (mapping/mappings.py:242-261).  Workgroup = kBandRows rows x 1024 columns.
__global__ __launch_bounds__(256) void k_reset_dense(View v, const int* __restrict__ env_ids, int n_items, int n_bands,
                                                     int n_ctiles) {
    int item, part;
    if (!decode_block(blockIdx.x, n_items, n_bands * n_ctiles, item, part)) return;
    const int env = env_ids ? env_ids[item] : item;
    if (env < 0 || env >= v.cap) return;
    const int band = part / n_ctiles, tile = part - band * n_ctiles;
    const int cell0 = tile * 1024 + 4 * threadIdx.x;
    if (cell0 >= v.Npad) return;
    const double sv = v.prior[2 * env + 0], ls = v.prior[2 * env + 1];
    int cr[4], cc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { cr[c] = (cell0 + c) / v.W; cc[c] = (cell0 + c) - cr[c] * v.W; }
    float* P = v.cov + (size_t)env * v.cov_slot;
    const int row0 = band * kBandRows, nrows = min(kBandRows, v.N - row0);
    with_prior_kind(v.prior_kind, [&](auto kind) {
    for (int rr = 0; rr < nrows; ++rr) {
        const int i = row0 + rr, ri = i / v.W, ci = i - ri * v.W;
        float out[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            out[c] = (cell0 + c < v.N) ? (float)prior_d<decltype(kind)::value>(ri - cr[c], ci - cc[c], v.res, sv, ls) : 0.f;
        *reinterpret_cast<float4*>(P + (size_t)i * v.Npad + cell0) = make_float4(out[0], out[1], out[2], out[3]);
    }
    });
}

// GRF as a circular convolution: field = white (*) h, h = Re ifft2(amp) (simulations/ground_truths.py:14-31;
// amp is real and even so Re ifft2(fft2(white) * amp) is exactly this convolution).  fp64 accumulate.
// One workgroup per env: the tap table h (fp64) and the white noise (fp32) are staged in LDS once; a thread
// owns OT consecutive outputs of one row and keeps the OT taps they share in a rotating register window, so
// each step costs one 8-byte LDS tap read and one broadcast white value for OT fp64 FMAs; the taps of the
// next OT steps are read while the current ones are consumed.  Grids whose tables exceed LDS read them
// through L1/L2 instead (LDS_TABLES = false).
template <int OT, bool LDS_TABLES>
__global__ __launch_bounds__(256) void k_grf_conv(View v, int n_items, const float* __restrict__ white, int tpr,
                                                  float* __restrict__ raw_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_grf[];
    const int item = blockIdx.y;
    if (item >= n_items) return;
    const int W = v.W, H = v.H, N = v.N;
    const float* __restrict__ wn = white + (size_t)item * N;
    const double* hk = v.grf_h;
    const float* wk = wn;
    if (LDS_TABLES) {
        double* hs = reinterpret_cast<double*>(smem_grf);
        float* ws = reinterpret_cast<float*>(hs + N);
        for (int i = threadIdx.x; i < N; i += blockDim.x) { hs[i] = v.grf_h[i]; ws[i] = wn[i]; }
        __syncthreads();
        hk = hs;
        wk = ws;
    }
    const int n_groups = H * tpr;
    for (int tix = blockIdx.x * blockDim.x + threadIdx.x; tix < n_groups; tix += gridDim.x * blockDim.x) {
        const int y = tix / tpr;
        const int x0 = (tix - y * tpr) * OT;
        double acc[OT], win[OT], nxt[OT];
#pragma unroll
        for (int j = 0; j < OT; ++j) acc[j] = 0.0;
        const int wsteps = (W + OT - 1) / OT * OT;
        for (int yp = 0; yp < H; ++yp) {
            int hy = y - yp;
            if (hy < 0) hy += H;
            const double* hrow = hk + (size_t)hy * W;
            const float* wrow = wk + (size_t)yp * W;
            // window holds h[(x0 + j - xp) mod W] at win[(j - xp) mod OT]; preload j = 1..OT-1 for xp = 0
#pragma unroll
            for (int j = 1; j < OT; ++j) {
                int idx = x0 + j;
                idx -= (idx >= W) ? W : 0;
                win[j] = hrow[idx];
            }
            int hi = x0;  // (x0 - xp) mod W, decremented each step
#pragma unroll
            for (int u = 0; u < OT; ++u) { nxt[u] = hrow[hi]; hi = (hi == 0) ? W - 1 : hi - 1; }
            for (int xb = 0; xb < wsteps; xb += OT) {
                double cur[OT];
                float wv[OT];
#pragma unroll
                for (int u = 0; u < OT; ++u) { cur[u] = nxt[u]; wv[u] = (xb + u < W) ? wrow[xb + u] : 0.f; }
#pragma unroll
                for (int u = 0; u < OT; ++u) { nxt[u] = hrow[hi]; hi = (hi == 0) ? W - 1 : hi - 1; }  // taps of the next block
#pragma unroll
                for (int u = 0; u < OT; ++u) {
                    win[(OT - u) % OT] = cur[u];  // new tap h[(x0 - xp) mod W] replaces the one that left
                    const double w = (double)wv[u];
#pragma unroll
                    for (int j = 0; j < OT; ++j) acc[j] = fma(w, win[(j + OT - u) % OT], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < OT; ++j)
            if (x0 + j < W) raw_out[(size_t)item * v.Npad + y * W + x0 + j] = (float)acc[j];
    }
}

// min-max normalisation to [0, 1] (simulations/ground_truths.py:31).
// gt_out == nullptr: write into the env slots (ipp_reset); else into the caller buffer [n][N] (ipp_generate_grf).
__global__ __launch_bounds__(256) void k_grf_norm(View v, const int* __restrict__ env_ids, int n_items,
                                                  const float* __restrict__ raw_all, float* __restrict__ gt_out) {
    __shared__ float smin[4], smax[4];
    const int item = blockIdx.x;
    const int env = gt_out ? 0 : (env_ids ? env_ids[item] : item);
    if (env < 0 || env >= v.cap) return;
    const float* raw = raw_all + (size_t)item * v.Npad;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < v.N; i += blockDim.x) { lo = fminf(lo, raw[i]); hi = fmaxf(hi, raw[i]); }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    hi = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const double dlo = lo, span = (double)hi - (double)lo;
    if (gt_out) {
        float* gt = gt_out + (size_t)item * v.N;
        for (int i = threadIdx.x; i < v.N; i += blockDim.x) gt[i] = (float)(((double)raw[i] - dlo) / span);
        return;
    }
    float* gt = gt_plane(v, env);
    for (int i = threadIdx.x; i < v.Npad; i += blockDim.x) gt[i] = (i < v.N) ? (float)(((double)raw[i] - dlo) / span) : 0.f;
}

// State slot copy (tree-search children).  grid = (chunks, n); float4 grid-stride over the covariance slab.
__global__ __launch_bounds__(256) void k_fork(View v, const int* __restrict__ src_ids, const int* __restrict__ dst_ids,
                                              int n_items) {
    const int item = blockIdx.y;
    if (item >= n_items) return;
    const int s = src_ids[item], d = dst_ids[item];
    if (s < 0 || s >= v.cap || d < 0 || d >= v.cap || s == d) return;
    const int r = (v.mode == IPP_FACTOR) ? v.rank[s] : v.N;
    const size_t n4 = (size_t)r * (v.patch ? (size_t)v.pstride : (size_t)v.Npad) / 4;  // (patch layout: a column is pstride floats)
    const float4* cs = reinterpret_cast<const float4*>(v.cov + (size_t)s * v.cov_slot);
    float4* cd = reinterpret_cast<float4*>(v.cov + (size_t)d * v.cov_slot);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) cd[i] = cs[i];
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < v.Npad; i += blockDim.x) {
            v.mean[(size_t)d * v.Npad + i] = v.mean[(size_t)s * v.Npad + i];
            v.diag[(size_t)d * v.Npad + i] = v.diag[(size_t)s * v.Npad + i];
            gt_plane(v, d)[i] = gt_plane(v, s)[i];
        }
        if (threadIdx.x == 0) {
            v.prior[2 * d + 0] = v.prior[2 * s + 0];
            v.prior[2 * d + 1] = v.prior[2 * s + 1];
        }
        if (v.mode == IPP_FACTOR)
            for (int i = threadIdx.x; i < r; i += blockDim.x)
            {
                v.colspan[(size_t)d * v.rank_cap + i] = v.colspan[(size_t)s * v.rank_cap + i];
                v.colrect[(size_t)d * v.rank_cap + i] = v.colrect[(size_t)s * v.rank_cap + i];
            }
    }
}
// rank is written by a second tiny launch so that k_fork never reads a rank another block already replaced
__global__ void k_fork_rank(View v, const int* __restrict__ src_ids, const int* __restrict__ dst_ids, int n_items) {
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= n_items) return;
    const int s = src_ids[item], d = dst_ids[item];
    if (s < 0 || s >= v.cap || d < 0 || d >= v.cap) return;
    v.rank[d] = v.rank[s];
}

// Factor state -> dense P = P0 - U U^T for callers that need the matrix (np.diag(state), feature planes).
__global__ __launch_bounds__(256) void k_read_cov_factor(View v, int env, float* __restrict__ out) {
    const int i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.N || j >= v.N) return;
    const double sv = v.prior[2 * env + 0], ls = v.prior[2 * env + 1];
    const int ri = i / v.W, ci = i - ri * v.W, rj = j / v.W, cj = j - rj * v.W;
    double acc = prior_d(v.prior_kind, ri - rj, ci - cj, v.res, sv, ls);
    const float* U = v.cov + (size_t)env * v.cov_slot;
    const int r = v.rank[env];
    const int ti = i / v.tile_cells, tj = j / v.tile_cells;
    const int* span = v.colspan + (size_t)env * v.rank_cap;
    for (int k = 0; k < r; ++k) {
        const int lo = span[k] & 0xffff, hi = span[k] >> 16;  // a column is zero outside its stored tiles
        if (ti < lo || ti > hi || tj < lo || tj > hi) continue;
        if (v.rect_meta) {  // ... and outside its rectangle
            const unsigned rc = (unsigned)v.colrect[(size_t)env * v.rank_cap + k];
            if (!rect_has(rc, ri, ci) || !rect_has(rc, rj, cj)) continue;
        }
        acc -= (double)U[(size_t)k * v.Npad + i] * (double)U[(size_t)k * v.Npad + j];
    }
    out[(size_t)i * v.N + j] = (float)acc;
}

// diag <- diag(P) after a dense injection; also clears the row padding.
__global__ void k_dense_fixup(View v, int env) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.N) return;
    float* P = v.cov + (size_t)env * v.cov_slot;
    v.diag[(size_t)env * v.Npad + i] = P[(size_t)i * v.Npad + i];
    for (int j = v.N; j < v.Npad; ++j) P[(size_t)i * v.Npad + j] = 0.f;
}

// planning/evaluation_metrics.py:4-58 fused into one pass pair per env (mask = gt >= value_threshold,
// planning/missions.py:179).  out[item][8] = rmse, masked rmse, wrmse, mll, wmll, trace, masked trace, diff.
__global__ __launch_bounds__(256) void k_metrics(View v, const int* __restrict__ env_ids, int n_items,
                                                 float* __restrict__ out) {
    __shared__ double red[4][8];
    const int item = blockIdx.x;
    const int env = env_ids ? env_ids[item] : item;
    if (env < 0 || env >= v.cap) return;
    const float* gt = gt_plane(v, env);
    const float* est = v.mean + (size_t)env * v.Npad;
    const float* dg = v.diag + (size_t)env * v.Npad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // pass 1: extrema and the weight normaliser
    float gmin = INFINITY, gmax = -INFINITY, emin = INFINITY;
    double gsum = 0.0;
    for (int i = tid; i < v.N; i += blockDim.x) {
        gmin = fminf(gmin, gt[i]); gmax = fmaxf(gmax, gt[i]); emin = fminf(emin, est[i]);
        gsum += (double)gt[i];
    }
    gmin = wave_min(gmin); gmax = wave_max(gmax); emin = wave_min(emin); gsum = wave_sum(gsum);
    if (lane == 0) { red[wave][0] = gmin; red[wave][1] = gmax; red[wave][2] = emin; red[wave][3] = gsum; }
    __syncthreads();
    const double g_lo = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
    const double g_hi = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
    const double e_lo = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    const double g_sum = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    __syncthreads();
    const double range = g_hi - g_lo;
    const double wsum = (g_sum - v.N * e_lo) / range;  // sum of (gt - min(est)) / range
    // pass 2
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // se, se_mask, n_mask, w*se, ll, w*ll, tr, tr_mask
    for (int i = tid; i < v.N; i += blockDim.x) {
        const double g = gt[i], e = est[i], p = dg[i];
        const double se = (g - e) * (g - e);
        const double w = ((g - e_lo) / range) / wsum;
        const double ll = 0.5 * log(2.0 * M_PI * p) + se / 2.0 * p;  // precedence as in evaluation_metrics.py:44
        const bool mk = (double)gt[i] >= v.thr;
        s[0] += se; s[3] += w * se; s[4] += ll; s[5] += w * ll; s[6] += p;
        if (mk) { s[1] += se; s[2] += 1.0; s[7] += p; }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = wave_sum(s[q]);
    if (lane == 0)
        for (int q = 0; q < 8; ++q) red[wave][q] = s[q];
    __syncthreads();
    if (tid == 0) {
        double t[8];
        for (int q = 0; q < 8; ++q) t[q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
        const double n = v.N, nm = t[2], nu = n - nm;
        float* o = out + (size_t)item * 8;
        o[0] = (float)sqrt(t[0] / n);
        o[1] = (float)sqrt(t[1] / nm);
        o[2] = (float)sqrt(t[3] / n);
        o[3] = (float)(t[4] / n);
        o[4] = (float)(t[5] / n);
        o[5] = (float)t[6];
        o[6] = (float)t[7];
        const double mu_u = (t[6] - t[7]) / nu, mu_i = t[7] / nm;
        o[7] = (float)((mu_u - mu_i) / mu_u);
    }
}

__global__ void k_fill_normal(float* __restrict__ out, uint64_t count, uint64_t seed, uint64_t subseq) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= count) return;
    float nrm[4];
    philox_normal4(q, subseq, seed, nrm);
    for (int e = 0; e < 4; ++e)
        if (q * 4 + e < count) out[q * 4 + e] = nrm[e];
}

// Row-keyed variant: out[p][j][c] (planes x rows x row_len) = normal(seed, subsequence subseq0 + p, counter =
// (row id of j) * ceil(row_len / 4) + c / 4, element c % 4), row id = (row_ids ? row_ids[j] : j) + row_offset.
// A row is an env (its ground-truth white noise, its measurement noise of one step): keyed on the GLOBAL env id the
// value does not depend on which rows share a launch, i.e. on how the envs are sharded over GPUs.
__global__ void k_fill_normal_rows(float* __restrict__ out, int planes, int rows, int row_len, const int* __restrict__ row_ids,
                                   long long row_offset, uint64_t seed, uint64_t subseq0) {
    const int qpr = (row_len + 3) >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)rows * qpr) return;
    const int j = (int)(idx / qpr), qc = (int)(idx - (long long)j * qpr);
    const int p = blockIdx.y;
    const uint64_t rid = (uint64_t)((row_ids ? (long long)row_ids[j] : (long long)j) + row_offset);
    const uint64_t q = rid * (uint64_t)qpr + (uint64_t)qc;
    const uint64_t subseq = subseq0 + (uint64_t)p;
    float nrm[4];
    philox_normal4(q, subseq, seed, nrm);
    float* o = out + ((size_t)p * rows + j) * row_len + 4 * qc;
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (4 * qc + h < row_len) o[h] = nrm[h];
}

// Occupies the device for `ticks` of the 100 MHz wall clock (ipp_probe_stream_pair: dependent launches on two queues).
__global__ void k_spin(unsigned long long ticks, int* sink) {
    const unsigned long long t0 = wall_clock64();
    int n = 0;
    while (wall_clock64() - t0 < ticks) { __builtin_amdgcn_s_sleep(8); ++n; }
    if (sink && n < 0) *sink = n;
}

}  // namespace ipp
