// NN input feature planes of a batch of histories (planning/common/features.py:83-151, generate_input_feature_planes), one
// launch for the whole batch.  Request i has H entries (newest first); entry h is a state given as an env slot, a column
// prefix of it (rank) and an optional tree path below it, so that no history needs a covariance of its own: within an
// episode the factor columns of a slot are only ever appended, the state k steps ago is the first r_{t-k} of them.
//
// One workgroup per (request, entry) and, with the cost plane, one more per request:
//   state plane  densify P = s^2 P0 - U U^T (the column readers of k_score_densify: exact, band-tile, patch, tree chain) in
//                64 x 64 tiles, zero the rows / columns outside the adaptive mask (mean of the request + k * the entry's own
//                diagonal >= thr), take min / max with a workgroup reduction, write (x - min) / (max - min).  Planes of
//                N^2 * 4 <= kPlaneCacheBytes stay in LDS between the two passes (one densify); larger ones are densified
//                again in the writing pass (no scratch, no second launch).
//   constant     position [x, y, z] / FoV outer(sel, sel) and budget planes of the entry: pure 16-byte stores.
//   cost plane   row c = action cost from (p0.x, p0.y, min_alt) to cell c's centre at min_alt (features.py:64-71), fp64,
//                min-max normalised over the N costs.
// Padding entries (valid = 0) write zero planes.  An entry the engine cannot evaluate (slot, node id or rank out of range,
// a path on a dense engine, a prefix below a path) writes NaN planes: it is never clamped to some other state.
#pragma once
#include "ipp_common.h"
#include "k_tree.h"

namespace ipp {

constexpr int kPlaneLdsBytes = 64 * 1024;  // whole LDS of a workgroup, static tiles included (10 x 10 grid: 57 KB; 2 workgroups per CU)
constexpr int kPlaneStaticLds = 2 * 32 * 65 * 4 + 8 * 4 + 8 * 8;  // ui, uj, red, dred of k_feature_planes

struct PlaneArgs {
    const ipp_plane_entry* entries;  // [n][H]
    const int* mask_env;             // [n] slot whose current mean masks request i (mask_mean == NULL)
    const float* mask_mean;          // [n][N] or NULL
    float* out;                      // [n][C][N][N]
    int n, H, C, cpe;                // cpe: channels per entry (5 position mode, 3 FoV mode)
    int fov, costs, adaptive, flight, cache, dense;
    double min_alt, max_alt;
};

// The columns of one entry's state: the root slot's first r_root columns, then the column blocks of the path's nodes.
struct PlaneSrc {
    const float* U;
    const int* span;
    const int* rect;
    int root, r_root, depth, total;
    int ids[kTreeDepth], off[kTreeDepth];
};

// Value of column k of the state at cell c (0 where the column stores nothing), like k_score_densify's loader.
__device__ __forceinline__ float plane_col(const View& v, const TreeView& tv, const PlaneSrc& s, int k, int c) {
    int d = -1;
#pragma unroll
    for (int j = 0; j < kTreeDepth; ++j)
        if (j < s.depth && k >= s.off[j]) d = j;
    const int row = c / v.W, col = c - row * v.W;
    if (v.patch) {
        unsigned rc;
        const float* pk;
        if (d < 0) {
            rc = (unsigned)s.rect[k];
            pk = s.U + (size_t)k * v.pstride;
        } else {
            const int id = s.ids[d];
            rc = (unsigned)tv.node_meta[kNodeMeta * id + 4];
            pk = tv.node_cov + ((size_t)id * v.meas_cap + (k - s.off[d])) * v.pstride;
        }
        if (!rect_has(rc, row, col)) return 0.f;
        return pk[(row - (int)(rc & 0xff)) * v.pw + (col - (int)((rc >> 16) & 0xff))];
    }
    int sp;
    unsigned rc = kRectFull;
    const float* p;
    if (d < 0) {
        sp = s.span[k];
        if (v.rect_meta) rc = (unsigned)s.rect[k];
        p = s.U + (size_t)k * v.Npad + c;
    } else {
        const int id = s.ids[d];
        sp = tv.node_meta[kNodeMeta * id + 1];
        if (v.rect_meta) rc = (unsigned)tv.node_meta[kNodeMeta * id + 4];
        p = tv.node_cov + (size_t)id * v.meas_cap * tv.win_cells + (size_t)(k - s.off[d]) * tv.win_cells + (c - (sp & 0xffff) * v.tile_cells);
    }
    const int tile = c / v.tile_cells;
    if (tile < (sp & 0xffff) || tile > (sp >> 16) || !rect_has(rc, row, col)) return 0.f;
    return *p;
}

// Diagonal of the entry's state at cell c: stored diag of the slot (its current state) or of the deepest path node that holds
// c (k_tree_read_diag), else the densified diagonal of the prefix (the same fp32 sum as the densified plane's (c, c)).
__device__ __forceinline__ float plane_diag(const View& v, const TreeView& tv, const PlaneSrc& s, int c, int cur_rank) {
    if (s.depth > 0) {
        const int row = c / v.W, col = c - row * v.W, tile = c / v.tile_cells;
        for (int j = s.depth - 1; j >= 0; --j) {
            const int id = s.ids[j];
            const unsigned rc = (unsigned)tv.node_meta[kNodeMeta * id + 4];
            if (v.patch) {
                if (rect_has(rc, row, col))
                    return tv.node_diag[(size_t)id * v.pstride + (row - (int)(rc & 0xff)) * v.pw + (col - (int)((rc >> 16) & 0xff))];
            } else {
                const int sp = tv.node_meta[kNodeMeta * id + 1], lo = sp & 0xffff, hi = sp >> 16;
                if (tile >= lo && tile <= hi && rect_has(rc, row, col)) return tv.node_diag[(size_t)id * tv.win_cells + (c - lo * v.tile_cells)];
            }
        }
    }
    if (s.depth > 0 || s.r_root == cur_rank) return v.diag[(size_t)s.root * v.Npad + c];
    float acc = 0.f;
    for (int k = 0; k < s.r_root; ++k) {
        const float u = plane_col(v, tv, s, k, c);
        acc = fmaf(u, u, acc);
    }
    const double p00 = prior_d(v.prior_kind, 0, 0, v.res, v.prior[2 * s.root + 0], v.prior[2 * s.root + 1]);
    return (float)(p00 - (double)acc);
}

__device__ __forceinline__ void plane_fill(float* __restrict__ dst, float val, size_t nn, bool vec) {
    if (vec) {
        const float4 q = make_float4(val, val, val, val);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (size_t i = threadIdx.x; i < nn / 4; i += blockDim.x) d4[i] = q;
    } else {
        for (size_t i = threadIdx.x; i < nn; i += blockDim.x) dst[i] = val;
    }
}

// min / max of the whole workgroup (256 threads); every thread gets the result
__device__ __forceinline__ void plane_reduce(float& lo, float& hi, float* red) {
    lo = wave_min(lo);
    hi = wave_max(hi);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lo; red[4 + (threadIdx.x >> 6)] = hi; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

__device__ __forceinline__ double plane_cost(const View& v, const PlaneArgs& a, double px, double py, int c) {
    const int x = c / v.W, y = c - x * v.W;  // actions[x_dim * x + y] = cell (x, y) (actions.py:76-88; square grids)
    const double dx = ((double)x * v.res + 0.5 * v.res) - px, dy = ((double)y * v.res + 0.5 * v.res) - py, dz = 0.0;
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    if (!a.flight) return dist;
    const double d_acc = fmin(dist * 0.5, v.vmax * v.vmax / (2 * v.amax));  // actions.py:32-41
    return (dist - 2 * d_acc) / v.vmax + 2 * sqrt(2 * d_acc / v.amax);
}

__global__ __launch_bounds__(256) void k_feature_planes(View v, TreeView tv, PlaneArgs a) {
    constexpr int TB = 64, KC = 32;
    __shared__ float ui[KC][TB + 1], uj[KC][TB + 1];
    __shared__ float red[8];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_plane[];
    const int per = a.H + a.costs;
    const int req = blockIdx.x / per, h = blockIdx.x - req * per;
    const int N = v.N;
    const size_t NN = (size_t)N * N;
    const bool vec = (NN % 4 == 0);
    float* req_out = a.out + (size_t)req * a.C * NN;

    if (h == a.H) {  // ---------------------------------------------------------------- cost plane of the request
        float* dst = req_out + (size_t)(a.C - 1) * NN;
        const ipp_plane_entry e0 = a.entries[(size_t)req * a.H];
        if (!e0.valid) { plane_fill(dst, 0.f, NN, vec); return; }
        const double px = e0.position[0], py = e0.position[1];
        double lo = INFINITY, hi = -INFINITY;
        for (int c = threadIdx.x; c < N; c += blockDim.x) {
            const double x = plane_cost(v, a, px, py, c);
            lo = fmin(lo, x);
            hi = fmax(hi, x);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off, kWave)); hi = fmax(hi, __shfl_xor(hi, off, kWave)); }
        __shared__ double dred[8];
        if ((threadIdx.x & 63) == 0) { dred[threadIdx.x >> 6] = lo; dred[4 + (threadIdx.x >> 6)] = hi; }
        __syncthreads();
        lo = fmin(fmin(dred[0], dred[1]), fmin(dred[2], dred[3]));
        hi = fmax(fmax(dred[4], dred[5]), fmax(dred[6], dred[7]));
        const bool flat = (lo == hi);
        for (size_t idx = threadIdx.x; idx < NN; idx += blockDim.x) {
            const double x = plane_cost(v, a, px, py, (int)(idx / N));
            dst[idx] = (float)(flat ? x / hi : (x - lo) / (hi - lo));
        }
        return;
    }

    const ipp_plane_entry e = a.entries[(size_t)req * a.H + h];
    float* base = req_out + (size_t)h * a.cpe * NN;
    if (!e.valid) {
        for (int ch = 0; ch < a.cpe; ++ch) plane_fill(base + ch * NN, 0.f, NN, vec);
        return;
    }
    // ---------------------------------------------------------------- resolve the state (every thread the same)
    PlaneSrc s;
    bool bad = (e.root_env < 0 || e.root_env >= v.cap);
    s.root = bad ? 0 : e.root_env;
    const int cur = a.dense ? 0 : v.rank[s.root];
    s.U = v.cov + (size_t)s.root * v.cov_slot;
    s.span = v.colspan + (size_t)s.root * v.rank_cap;
    s.rect = v.colrect + (size_t)s.root * v.rank_cap;
    s.r_root = (e.rank < 0 || a.dense) ? cur : e.rank;
    if (s.r_root > cur) bad = true;
    s.depth = 0;
    int total = s.r_root;
#pragma unroll
    for (int j = 0; j < kTreeDepth; ++j) { s.ids[j] = 0; s.off[j] = 0x7fffffff; }
    for (int j = 0; j < kTreeDepth; ++j) {
        const int id = e.path[j];
        if (id < 0) continue;
        if (a.dense || id >= tv.node_cap || s.r_root != cur) { bad = true; break; }
        s.ids[s.depth] = id;
        s.off[s.depth] = total;
        total += tv.node_meta[kNodeMeta * id];
        ++s.depth;
    }
    s.total = total;
    int menv = 0;
    if (!a.mask_mean && a.adaptive) {
        menv = a.mask_env[req];
        if (menv < 0 || menv >= v.cap) bad = true;
    }
    if (bad) {
        for (int ch = 0; ch < a.cpe; ++ch) plane_fill(base + ch * NN, NAN, NN, vec);
        return;
    }

    // ---------------------------------------------------------------- constant planes of the entry
    if (a.fov) {  // outer(sel, sel), sel = get_field_of_view_indices (features.py:153-167): x in [xl, xr), y in [yu, yd), cell x_dim x + y
        const double az = e.position[2];
        const double ext_x = 2 * az * v.tanx, ext_y = 2 * az * v.tany;
        const double cells_x = floor(ext_x / v.res), cells_y = floor(ext_y / v.res);
        const double gx = floor(e.position[0] / v.res), gy = floor(e.position[1] / v.res);
        const double rad_x = floor(0.5 * cells_x), rad_y = floor(0.5 * cells_y);
        const int xl = (int)fmin(fmax(gx - rad_x, 0.0), (double)(v.W - 1)), xr = (int)fmin(fmax(gx + rad_x, 0.0), (double)(v.W - 1));
        const int yu = (int)fmin(fmax(gy - rad_y, 0.0), (double)(v.H - 1)), yd = (int)fmin(fmax(gy + rad_y, 0.0), (double)(v.H - 1));
        float* dst = base + NN;
        for (size_t idx = threadIdx.x; idx < NN; idx += blockDim.x) {
            const int r = (int)(idx / N), c = (int)(idx - (size_t)r * N);
            const int xr_ = r / v.W, yr_ = r - xr_ * v.W, xc_ = c / v.W, yc_ = c - xc_ * v.W;
            const bool in = xr_ >= xl && xr_ < xr && yr_ >= yu && yr_ < yd && xc_ >= xl && xc_ < xr && yc_ >= yu && yc_ < yd;
            dst[idx] = in ? 1.f : 0.f;
        }
        plane_fill(base + 2 * NN, (float)e.budget, NN, vec);
    } else {  // features.py:46-57: x and y both over x_dim * resolution
        const double span_xy = (double)v.W * v.res;
        plane_fill(base + NN, (float)(e.position[0] / span_xy), NN, vec);
        plane_fill(base + 2 * NN, (float)(e.position[1] / span_xy), NN, vec);
        plane_fill(base + 3 * NN, (float)((e.position[2] - a.min_alt) / (a.max_alt - a.min_alt)), NN, vec);
        plane_fill(base + 4 * NN, (float)e.budget, NN, vec);
    }

    // ---------------------------------------------------------------- adaptive mask (features.py:91-97, rewards.py:8-12)
    unsigned char* mask = smem_plane;
    float* cache = reinterpret_cast<float*>(smem_plane + ((N + 15) & ~15));
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
        bool mk = true;
        if (a.adaptive) {
            const double mu = a.mask_mean ? (double)a.mask_mean[(size_t)req * N + c] : (double)v.mean[(size_t)menv * v.Npad + c];
            mk = mu + v.kf * (double)plane_diag(v, tv, s, c, cur) >= v.thr;
        }
        mask[c] = mk ? 1 : 0;
    }
    __syncthreads();

    // ---------------------------------------------------------------- densify, masked extrema (and the LDS copy)
    const float* Pd = v.cov + (size_t)s.root * v.cov_slot;  // dense slot, read in place
    const double svv = v.prior[2 * s.root + 0], ls = v.prior[2 * s.root + 1];
    const int tid = threadIdx.x, ti = tid / 16, tj = tid % 16;
    const int nt = (N + TB - 1) / TB;
    const int r = a.dense ? 0 : s.total;
    float* dst = base;
    float lo = INFINITY, hi = -INFINITY;
    double dlo = 0, dhi = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && a.cache) break;
        for (int t = 0; t < nt * nt; ++t) {
            const int i0 = (t / nt) * TB, j0 = (t % nt) * TB;
            float acc[4][4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = 0.f;
            for (int k0 = 0; k0 < r; k0 += KC) {
                __syncthreads();
                for (int idx = tid; idx < KC * TB; idx += 256) {
                    const int kk = idx / TB, c = idx - kk * TB, k = k0 + kk;
                    float x = 0.f, y = 0.f;
                    if (k < r) {
                        if (i0 + c < N) x = plane_col(v, tv, s, k, i0 + c);
                        if (j0 + c < N) y = plane_col(v, tv, s, k, j0 + c);
                    }
                    ui[kk][c] = x;
                    uj[kk][c] = y;
                }
                __syncthreads();
#pragma unroll 8
                for (int kk = 0; kk < KC; ++kk) {
                    float av[4], bv[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) av[p] = ui[kk][ti * 4 + p];
#pragma unroll
                    for (int q = 0; q < 4; ++q) bv[q] = uj[kk][tj * 4 + q];
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(av[p], bv[q], acc[p][q]);
                }
            }
            with_prior_kind(v.prior_kind, [&](auto kind) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int i = i0 + ti * 4 + p;
                    if (i >= N) continue;
                    const int ri = i / v.W, ci = i - ri * v.W;
                    const bool mi = mask[i] != 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = j0 + tj * 4 + q;
                        if (j >= N) continue;
                        float x = 0.f;
                        if (mi && mask[j]) {
                            if (a.dense) {
                                x = Pd[(size_t)i * v.Npad + j];
                            } else {
                                const int rj = j / v.W, cj = j - rj * v.W;
                                x = (float)(prior_d<decltype(kind)::value>(ri - rj, ci - cj, v.res, svv, ls) - (double)acc[p][q]);
                            }
                        }
                        if (pass == 0) {
                            lo = fminf(lo, x);
                            hi = fmaxf(hi, x);
                            if (a.cache) cache[(size_t)i * N + j] = x;
                        } else {
                            const double xd = (double)x;
                            dst[(size_t)i * N + j] = (float)(dlo == dhi ? xd / dhi : (xd - dlo) / (dhi - dlo));
                        }
                    }
                }
            });
        }
        if (pass == 0) {
            plane_reduce(lo, hi, red);
            dlo = (double)lo;
            dhi = (double)hi;
        }
    }
    if (a.cache) {  // normalising pass from LDS, 16-byte stores (plane_reduce ended on a barrier: the cache is complete)
        const bool flat = (dlo == dhi);
        if (vec) {
            float4* d4 = reinterpret_cast<float4*>(dst);
            const float4* c4 = reinterpret_cast<const float4*>(cache);
            for (size_t q = threadIdx.x; q < NN / 4; q += blockDim.x) {
                const float4 x = c4[q];
                float4 y;
                y.x = (float)(flat ? (double)x.x / dhi : ((double)x.x - dlo) / (dhi - dlo));
                y.y = (float)(flat ? (double)x.y / dhi : ((double)x.y - dlo) / (dhi - dlo));
                y.z = (float)(flat ? (double)x.z / dhi : ((double)x.z - dlo) / (dhi - dlo));
                y.w = (float)(flat ? (double)x.w / dhi : ((double)x.w - dlo) / (dhi - dlo));
                d4[q] = y;
            }
        } else {
            for (size_t q = threadIdx.x; q < NN; q += blockDim.x) {
                const double x = (double)cache[q];
                dst[q] = (float)(flat ? x / dhi : (x - dlo) / (dhi - dlo));
            }
        }
    }
}

}  // namespace ipp
