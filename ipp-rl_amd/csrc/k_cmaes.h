// Batched CMA-ES for the trajectory planner (the reference's planning/ipp_masha.py: cma.CMAEvolutionStrategy driven by ask / tell at
// :160-178 around simulate_trajectory, :102-140).  The strategy is Hansen's (mu/mu_w, lambda)-CMA-ES ("The CMA Evolution Strategy: A
// Tutorial", default parameters, positive recombination weights only), one independent search per env, each with its OWN dimension
// N_e <= nmax <= kCmaMaxDim.  Everything is fp64 with contraction off and every sum runs in a fixed order: two runs agree bit for bit.
// Kernels:
//   k_cma_init       the start state of every env: m = m0, sigma = 1, C = B = I, D = 1, paths 0, best-ever (m0, +inf)
//   k_cma_ask        one wave per env: X[k] = m + sigma s (.) (B (D (.) z_k)) for the lam normals of the env
//   k_cma_plan       one thread per candidate: bounds test, per-step costs, path cost and live-step count of simulate_trajectory, and the
//                    action / previous-action rows of the covariance-only step launches (NaN action = nothing applied)
//   k_cma_objective  one thread per candidate: the trajectory objective from the step rewards and statuses
//   k_cma_tell       one wave per env: stable ranking, recombination, both evolution paths, the covariance and step-size update, then
//                    a cyclic Jacobi eigendecomposition of the new C in LDS (round-robin pair order: the pairs of a round are
//                    disjoint and rotate together; sweeps until one rotates no pair, at most kJacobiSweeps) and the best-ever
// These are latency-bound kernels like k_mcts_select: the evaluation between ask and tell (lam x horizon env steps) is the work.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cma {

constexpr int kCmaMaxDim = 48;  // 16 waypoints: C and B as [48][49] doubles are 2 x 18.4 KB of LDS
constexpr int kCmaMaxLam = 64;  // one lane per candidate in the ranking
constexpr int kLd = kCmaMaxDim + 1;  // LDS row stride: lane i reading row i at a fixed column hits 32 distinct banks per half wave
constexpr int kJacobiSweeps = 30;
constexpr double kJacobiTol = 0x1p-53;  // a pair rotates while |a_pq| > kJacobiTol sqrt(|a_pp a_qq|)

// Layout of one env's state in 8-byte words (doubles, the last three int64): a function of nmax alone
struct Layout {
    int nmax, m, sigma, C, B, D, ps, pc, bx, bf, gen, status, dim, words;
};
__host__ __device__ inline Layout layout(int nmax) {
    Layout L;
    L.nmax = nmax;
    L.m = 0;
    L.sigma = nmax;
    L.C = L.sigma + 1;
    L.B = L.C + nmax * nmax;
    L.D = L.B + nmax * nmax;
    L.ps = L.D + nmax;
    L.pc = L.ps + nmax;
    L.bx = L.pc + nmax;
    L.bf = L.bx + nmax;
    L.gen = L.bf + 1;
    L.status = L.gen + 1;
    L.dim = L.status + 1;
    L.words = L.dim + 1;
    return L;
}

__device__ __forceinline__ double lane_bcast(double x, int src) {  // src wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// Wave-wide sum without LDS permutes (the DPP reductions of k_mcts.h): quads, half rows and rows through DPP moves, the four row
// results through v_readlane.  Every lane returns the result; the order of the additions is fixed.
__device__ __forceinline__ double wave_sum(double x) {
#pragma clang fp contract(off)
    x += dpp_f64<0xB1>(x);
    x += dpp_f64<0x4E>(x);
    x += dpp_f64<0x141>(x);
    x += dpp_f64<0x140>(x);
    return (lane_bcast(x, 0) + lane_bcast(x, 16)) + (lane_bcast(x, 32) + lane_bcast(x, 48));
}
// the env's dimension as the kernels use it: anything outside [0, nmax] counts as 0 (the env is skipped)
__device__ __forceinline__ int env_dim(const double* st, const Layout& L) {
    const long long d = reinterpret_cast<const long long*>(st)[L.dim];
    return (d < 0 || d > L.nmax) ? 0 : (int)d;
}

__global__ __launch_bounds__(64) void k_cma_init(double* __restrict__ state, int nmax, const int32_t* __restrict__ dims,
                                                 const double* __restrict__ m0) {
    const Layout L = layout(nmax);
    double* st = state + (size_t)blockIdx.x * L.words;
    const int lane = threadIdx.x;
    for (int t = lane; t < nmax * nmax; t += 64) {
        const double id = (t / nmax == t % nmax) ? 1.0 : 0.0;
        st[L.C + t] = id;
        st[L.B + t] = id;
    }
    for (int i = lane; i < nmax; i += 64) {
        const double mi = m0[(size_t)blockIdx.x * nmax + i];
        st[L.m + i] = mi;
        st[L.bx + i] = mi;
        st[L.D + i] = 1.0;
        st[L.ps + i] = 0.0;
        st[L.pc + i] = 0.0;
    }
    if (lane == 0) {
        const int d = dims[blockIdx.x];
        st[L.sigma] = 1.0;
        st[L.bf] = INFINITY;
        long long* w = reinterpret_cast<long long*>(st);
        w[L.gen] = 0;
        w[L.status] = (d < 0 || d > nmax) ? 2 : 0;  // 2: a dimension the state cannot hold (the env is skipped)
        w[L.dim] = (d < 0 || d > nmax) ? 0 : d;
    }
}

// y_i = sum_j B[i][j] v[j] for lane i < N (B in LDS at stride kLd, v in LDS: broadcast reads), j ascending
__device__ __forceinline__ double mat_vec(const double* sB, const double* sv, int i, int N) {
#pragma clang fp contract(off)
    double y = 0.0;
    for (int j = 0; j < N; ++j) y += sB[i * kLd + j] * sv[j];
    return y;
}

__global__ __launch_bounds__(64) void k_cma_ask(const double* __restrict__ state, int nmax, int lam, const float* __restrict__ Z,
                                                const double* __restrict__ scale, double* __restrict__ X) {
#pragma clang fp contract(off)
    __shared__ double sB[kCmaMaxDim * kLd];
    __shared__ double sv[kCmaMaxDim];
    const Layout L = layout(nmax);
    const double* st = state + (size_t)blockIdx.x * L.words;
    const int N = env_dim(st, L);
    if (N == 0 || reinterpret_cast<const long long*>(st)[L.status] != 0) return;  // (wave-uniform)
    const int lane = threadIdx.x;
    for (int t = lane; t < N * N; t += 64) {
        const int i = t / N, j = t - i * N;
        sB[i * kLd + j] = st[L.B + i * nmax + j];
    }
    const int i = lane < N ? lane : 0;
    const double Di = st[L.D + i], mi = st[L.m + i], si = scale[i], sigma = st[L.sigma];
    const float* z = Z + (size_t)blockIdx.x * lam * nmax;
    double* x = X + (size_t)blockIdx.x * lam * nmax;
    for (int k = 0; k < lam; ++k) {
        __syncthreads();
        if (lane < N) sv[lane] = Di * (double)z[(size_t)k * nmax + lane];
        __syncthreads();
        const double y = mat_vec(sB, sv, i, N);
        if (lane < nmax) x[(size_t)k * nmax + lane] = lane < N ? mi + sigma * si * y : 0.0;
    }
}

struct PlanArgs {
    int n, per_env, nmax, horizon, use_flight_time;
    double x_hi, y_hi, z_lo, z_hi, vmax, amax;  // x_hi = y_dim * resolution bounds waypoint[0], y_hi = x_dim * resolution waypoint[1]
    const int32_t* dims;   // [n] 3 x waypoints of the env's candidates
    const double* X;       // [n][per_env][nmax]
    const double* prev;    // [n][3] the env's current waypoint
    const double* budget;  // [n] remaining budget
    double* action;        // [horizon][n * per_env][3]
    double* prev_action;   // [horizon][n * per_env][3]
    double* cost;          // [horizon][n * per_env]
    double* path;          // [n * per_env]
    int32_t* live;         // [n * per_env] live steps, -1 out of bounds, -2 path cost <= 0
};

// actions.py:8-41 in the operand order of mc_cost (k_mcts.h)
__device__ __forceinline__ double step_cost(const PlanArgs& a, const double* w, const double* p) {
#pragma clang fp contract(off)
    const double d0 = w[0] - p[0], d1 = w[1] - p[1], d2 = w[2] - p[2];
    const double dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    if (!a.use_flight_time) return dist;
    const double ramp = fmin(0.5 * dist, (a.vmax * a.vmax) / (2 * a.amax));
    return (dist - 2 * ramp) / a.vmax + 2 * sqrt(2 * ramp / a.amax);
}

__global__ __launch_bounds__(256) void k_cma_plan(PlanArgs a) {
#pragma clang fp contract(off)
    const int nc = a.n * a.per_env;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const int e = c / a.per_env;
    int W = a.dims[e];
    W = (W < 0 || W > a.nmax) ? 0 : W / 3;
    if (W > a.horizon) W = a.horizon;
    const double* x = a.X + (size_t)c * a.nmax;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double p0[3] = {a.prev[3 * e], a.prev[3 * e + 1], a.prev[3 * e + 2]};
    bool oob = false;  // out_of_bounds (actions.py:102-106): inclusive on both ends; a NaN coordinate fails every comparison
    for (int t = 0; t < W; ++t) {
        const double w0 = x[3 * t], w1 = x[3 * t + 1], w2 = x[3 * t + 2];
        const bool in = (0.0 <= w1 && w1 <= a.y_hi) && (0.0 <= w0 && w0 <= a.x_hi) && (a.z_lo <= w2 && w2 <= a.z_hi);
        oob = oob || !in;
    }
    double path = 0.0;
    int live = 0;
    if (!oob) {
        double p[3] = {p0[0], p0[1], p0[2]};
        double left = a.budget[e];
        bool stopped = false;
        for (int t = 0; t < W; ++t) {
            const double w[3] = {x[3 * t], x[3 * t + 1], x[3 * t + 2]};
            const double ct = step_cost(a, w, p);
            a.cost[(size_t)t * nc + c] = ct;
            path += ct;
            if (!stopped && ct > left) stopped = true;  // ipp_masha.py:124-125
            if (!stopped) {
                left -= ct;
                ++live;
            }
            p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
        }
    }
    const bool run = !oob && path > 0.0;  // ipp_masha.py:104-106, :114-115
    if (!run) live = 0;
    double p[3] = {p0[0], p0[1], p0[2]};
    for (int t = 0; t < a.horizon; ++t) {
        double* act = a.action + ((size_t)t * nc + c) * 3;
        double* pa = a.prev_action + ((size_t)t * nc + c) * 3;
        pa[0] = p[0]; pa[1] = p[1]; pa[2] = p[2];
        if (t < live) {
            act[0] = p[0] = x[3 * t]; act[1] = p[1] = x[3 * t + 1]; act[2] = p[2] = x[3 * t + 2];
        } else {
            act[0] = act[1] = act[2] = nan;
            if (oob || t >= W) a.cost[(size_t)t * nc + c] = 0.0;
        }
    }
    a.path[c] = path;
    a.live[c] = oob ? -1 : (path > 0.0 ? live : -2);
}

__global__ __launch_bounds__(256) void k_cma_objective(int nc, int horizon, const float* __restrict__ reward, const int32_t* __restrict__ status,
                                                       const double* __restrict__ cost, const double* __restrict__ path,
                                                       const int32_t* __restrict__ live, double* __restrict__ f) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const int lv = live[c];
    if (lv < 0) {
        f[c] = 100.0;
        return;
    }
    double total = 0.0;
    bool bad = false;
    for (int t = 0; t < lv && t < horizon; ++t) {
        const int s = status[(size_t)t * nc + c];
        bad = bad || (s != 0 && s != 1);  // (1: the Cholesky fallback, a valid step)
        total += (double)reward[(size_t)t * nc + c] * (cost[(size_t)t * nc + c] + 1.0);  // ipp_masha.py:135
    }
    f[c] = bad ? 100.0 : -total / path[c];
}

// The pair (p, q), p < q, that slot k of round r of the round-robin schedule over n2 (even) indices rotates
__device__ __forceinline__ void jacobi_pair(int r, int k, int n2, int& p, int& q) {
    const int m = n2 - 1;
    int a, b;
    if (k == 0) {
        a = m;
        b = r;
    } else {
        a = (r + k) % m;
        b = (r - k + m) % m;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__global__ __launch_bounds__(64) void k_cma_tell(double* __restrict__ state, int nmax, int lam, const float* __restrict__ Z,
                                                 const double* __restrict__ X, const double* __restrict__ fit,
                                                 const double* __restrict__ scale) {
#pragma clang fp contract(off)
    __shared__ double sC[kCmaMaxDim * kLd];
    __shared__ double sB[kCmaMaxDim * kLd];
    __shared__ double sY[(kCmaMaxLam / 2) * kCmaMaxDim];
    __shared__ double sv[kCmaMaxDim], syw[kCmaMaxDim], spc[kCmaMaxDim], sw[kCmaMaxLam / 2];
    __shared__ double s_c[kCmaMaxDim / 2], s_s[kCmaMaxDim / 2];
    __shared__ int s_p[kCmaMaxDim / 2], s_q[kCmaMaxDim / 2], s_idx[kCmaMaxLam];
    const Layout L = layout(nmax);
    double* st = state + (size_t)blockIdx.x * L.words;
    long long* stw = reinterpret_cast<long long*>(st);
    const int N = env_dim(st, L);
    if (N == 0 || stw[L.status] != 0) return;  // (wave-uniform)
    const int lane = threadIdx.x;
    const float* z = Z + (size_t)blockIdx.x * lam * nmax;
    const double* x = X + (size_t)blockIdx.x * lam * nmax;

    // ---- ranking: ascending, ties to the lower index; a NaN fitness ranks as +inf
    double fk = lane < lam ? fit[(size_t)blockIdx.x * lam + lane] : INFINITY;
    if (!(fk == fk)) fk = INFINITY;
    int rank = 0;
    for (int j = 0; j < lam; ++j) {
        const double fj = lane_bcast(fk, j);
        rank += (fj < fk || (fj == fk && j < lane)) ? 1 : 0;
    }
    if (lane < lam) s_idx[rank] = lane;

    // ---- constants of (N, lam)
    const int mu = lam / 2;
    const double dN = (double)N;
    const double wraw = lane < mu ? log(((double)lam + 1.0) / 2.0) - log((double)(lane + 1)) : 0.0;
    const double wsum = wave_sum(wraw);
    const double wl = wraw / wsum;
    const double mu_eff = 1.0 / wave_sum(wl * wl);
    if (lane < mu) sw[lane] = wl;
    const double c_sigma = (mu_eff + 2.0) / (dN + mu_eff + 5.0);
    const double d_sigma = 1.0 + 2.0 * fmax(0.0, sqrt((mu_eff - 1.0) / (dN + 1.0)) - 1.0) + c_sigma;
    const double c_c = (4.0 + mu_eff / dN) / (dN + 4.0 + 2.0 * mu_eff / dN);
    const double c_1 = 2.0 / ((dN + 1.3) * (dN + 1.3) + mu_eff);
    const double c_mu = fmin(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((dN + 2.0) * (dN + 2.0) + mu_eff));
    const double chi_N = sqrt(dN) * (1.0 - 1.0 / (4.0 * dN) + 1.0 / (21.0 * dN * dN));

    for (int t = lane; t < N * N; t += 64) {
        const int i = t / N, j = t - i * N;
        sB[i * kLd + j] = st[L.B + i * nmax + j];
        sC[i * kLd + j] = st[L.C + i * nmax + j];
    }
    const int i = lane < N ? lane : 0;
    const bool on = lane < N;
    const double Di = st[L.D + i], mi = st[L.m + i], si = scale[i], sigma = st[L.sigma];
    const double psi = st[L.ps + i], pci = st[L.pc + i];
    const long long gen = stw[L.gen];
    __syncthreads();

    // ---- best-ever: the first candidate of the smallest fitness, only when strictly smaller
    {
        const int kb = __builtin_amdgcn_readfirstlane(s_idx[0]);
        const double fb = lane_bcast(fk, kb);
        if (fb < st[L.bf]) {
            if (on) st[L.bx + lane] = x[(size_t)kb * nmax + lane];
            if (lane == 0) st[L.bf] = fb;
        }
    }

    // ---- y_{r:lam} = B (D (.) z) of the mu best, y_w = sum w_r y_r (r ascending)
    double yw = 0.0;
    for (int r = 0; r < mu; ++r) {
        const int k = s_idx[r];
        __syncthreads();
        if (on) sv[lane] = Di * (double)z[(size_t)k * nmax + lane];
        __syncthreads();
        const double y = mat_vec(sB, sv, i, N);
        if (on) sY[r * kCmaMaxDim + lane] = y;
        yw += sw[r] * y;
    }
    const double m_new = mi + sigma * si * yw;
    __syncthreads();
    if (on) syw[lane] = yw;
    __syncthreads();
    // ---- p_sigma: C^-1/2 y_w = B ((B^T y_w) / D)
    double tj = 0.0;
    for (int r = 0; r < N; ++r) tj += sB[r * kLd + i] * syw[r];
    __syncthreads();
    if (on) sv[lane] = tj / Di;
    __syncthreads();
    const double v = mat_vec(sB, sv, i, N);
    const double ps_new = (1.0 - c_sigma) * psi + sqrt(c_sigma * (2.0 - c_sigma) * mu_eff) * v;
    const double ps_norm = sqrt(wave_sum(on ? ps_new * ps_new : 0.0));
    const double h_sigma = (ps_norm / sqrt(1.0 - pow(1.0 - c_sigma, 2.0 * (double)(gen + 1))) < (1.4 + 2.0 / (dN + 1.0)) * chi_N) ? 1.0 : 0.0;
    const double pc_new = (1.0 - c_c) * pci + h_sigma * sqrt(c_c * (2.0 - c_c) * mu_eff) * yw;
    if (on) spc[lane] = pc_new;
    __syncthreads();
    // ---- C, then (C + C^T) / 2
    const double keep = 1.0 - c_1 - c_mu, old_w = (1.0 - h_sigma) * c_c * (2.0 - c_c);
    for (int t = lane; t < N * N; t += 64) {
        const int a = t / N, b = t - a * N;
        double rk = 0.0;
        for (int r = 0; r < mu; ++r) rk += sw[r] * sY[r * kCmaMaxDim + a] * sY[r * kCmaMaxDim + b];
        const double cab = sC[a * kLd + b];
        sC[a * kLd + b] = keep * cab + c_1 * (spc[a] * spc[b] + old_w * cab) + c_mu * rk;
    }
    __syncthreads();
    for (int t = lane; t < N * N; t += 64) {
        const int a = t / N, b = t - a * N;
        if (a < b) {
            const double s2 = 0.5 * (sC[a * kLd + b] + sC[b * kLd + a]);
            sC[a * kLd + b] = s2;
            sC[b * kLd + a] = s2;
        }
    }
    const double sigma_new = sigma * exp((c_sigma / d_sigma) * (ps_norm / chi_N - 1.0));
    __syncthreads();
    for (int t = lane; t < N * N; t += 64) {
        const int a = t / N, b = t - a * N;
        st[L.C + a * nmax + b] = sC[a * kLd + b];
        sB[a * kLd + b] = a == b ? 1.0 : 0.0;  // V of the Jacobi sweeps (the old B is not needed any more)
    }
    if (on) {
        st[L.ps + lane] = ps_new;
        st[L.pc + lane] = pc_new;
    }
    if (lane == 0) st[L.sigma] = sigma_new;
    __syncthreads();

    // ---- cyclic Jacobi on sC, V in sB: C = V diag(eig) V^T
    const int n2 = N + (N & 1), npairs = n2 / 2;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < n2 - 1; ++r) {
            if (lane < npairs) {
                int p, q;
                jacobi_pair(r, lane, n2, p, q);
                double cs = 1.0, sn = 0.0;
                if (q < N) {
                    const double apq = sC[p * kLd + q];
                    const double app = sC[p * kLd + p], aqq = sC[q * kLd + q];
                    if (fabs(apq) > kJacobiTol * sqrt(fabs(app * aqq))) {  // (false for a NaN)
                        rotated = 1;
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        cs = 1.0 / sqrt(tt * tt + 1.0);
                        sn = tt * cs;
                    }
                } else {
                    q = p;  // the idle slot of an odd dimension: identity on (p, p)
                }
                s_p[lane] = p; s_q[lane] = q; s_c[lane] = cs; s_s[lane] = sn;
            }
            __syncthreads();
            // columns: A <- A J, V <- V J (item = (row, pair))
            for (int t = lane; t < N * npairs; t += 64) {
                const int row = t / npairs, k = t - row * npairs;
                const int p = s_p[k], q = s_q[k];
                if (p == q) continue;
                const double cs = s_c[k], sn = s_s[k];
                const double ap = sC[row * kLd + p], aq = sC[row * kLd + q];
                sC[row * kLd + p] = cs * ap - sn * aq;
                sC[row * kLd + q] = sn * ap + cs * aq;
                const double vp = sB[row * kLd + p], vq = sB[row * kLd + q];
                sB[row * kLd + p] = cs * vp - sn * vq;
                sB[row * kLd + q] = sn * vp + cs * vq;
            }
            __syncthreads();
            // rows: A <- J^T A (item = (pair, column))
            for (int t = lane; t < npairs * N; t += 64) {
                const int k = t / N, col = t - k * N;
                const int p = s_p[k], q = s_q[k];
                if (p == q) continue;
                const double cs = s_c[k], sn = s_s[k];
                const double ap = sC[p * kLd + col], aq = sC[q * kLd + col];
                sC[p * kLd + col] = cs * ap - sn * aq;
                sC[q * kLd + col] = sn * ap + cs * aq;
            }
            __syncthreads();
            if (lane < npairs && s_p[lane] != s_q[lane] && s_s[lane] != 0.0) {
                sC[s_p[lane] * kLd + s_q[lane]] = 0.0;
                sC[s_q[lane] * kLd + s_p[lane]] = 0.0;
            }
            __syncthreads();
        }
        if (!__any(rotated)) break;  // (wave-uniform) a whole sweep without a rotation: every |a_pq| <= kJacobiTol sqrt(|a_pp a_qq|)
    }
    const double eig = sC[i * kLd + i];
    const bool eig_ok = eig > 0.0 && eig < INFINITY;  // (false for a NaN)
    const bool sig_ok = sigma_new == sigma_new && fabs(sigma_new) < INFINITY;
    const bool ok = __all((!on || eig_ok) && sig_ok);
    if (!ok) {  // breakdown: m, B and D stay what they were; later calls for this env do nothing
        if (lane == 0) stw[L.status] = 1;
        return;
    }
    for (int t = lane; t < N * N; t += 64) {
        const int a = t / N, b = t - a * N;
        st[L.B + a * nmax + b] = sB[a * kLd + b];
    }
    if (on) {
        st[L.D + lane] = sqrt(eig);
        st[L.m + lane] = m_new;
    }
    if (lane == 0) stw[L.gen] = gen + 1;
}

}  // namespace cma
