// Hotspot and split ground truths (reference simulations/simulations.py:50-123): two values and at most two rectangles per field.
// The record of a field is computed once per workgroup (from Philox uniforms, or taken from the caller), then the plane is a pure
// store stream: H W floats per field against a few dozen instructions of set-up.
#pragma once
#include "ipp_common.h"
#include "k_grf_fft.h"
#include "k_misc.h"

namespace ipp {

// Uniform k of a field: Philox4x32-10 of (counter row * 8 + k, subsequence) under `seed`, word 0 as (c + 0.5) / 2^32 in fp64 (the host
// copy is philox_uniform in vec_env.py; budget_start draws the same way).
__device__ __forceinline__ double field_uniform(uint64_t row, int k, uint64_t subseq, uint64_t seed) {
    const uint64_t q = row * 8ull + (uint64_t)k;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)subseq, (uint32_t)(subseq >> 32)};
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int r = 0; r < 10; ++r) philox_round(c, key);
    return ((double)c[0] + 0.5) * (1.0 / 4294967296.0);
}

// a + (b - a) u with the product rounded before the sum (numpy.random.uniform; no contraction into an fma)
__device__ __forceinline__ double field_value(double a, double b, double u) { return __dadd_rn(a, __dmul_rn(b - a, u)); }

// randint(lo, hi) from one uniform: lo + min(floor(u (hi - lo)), hi - lo - 1)
__device__ __forceinline__ int field_randint(int lo, int hi, double u) {
    const int span = hi - lo;
    return lo + min((int)floor(__dmul_rn(u, (double)span)), span - 1);
}

// Cluster bounds of the reference (:63-66): int(max(c - r, 0)) .. int(min(c + r, dim)), fp64, truncated.
__device__ __forceinline__ void field_cluster(int c, double r, int dim, int& lo, int& hi) {
    lo = (int)fmax((double)c - r, 0.0);
    hi = (int)fmin((double)c + r, (double)dim);
}

// Second centre on one axis: uniform over {c in [lo, dim) : |c - c0| > r} (the rejection loop of :71-86 accepts exactly these, both axes
// independently).  The set is the integers below c0 - r and those above c0 + r; the host rejects (dim, r) where it can be empty.
__device__ __forceinline__ int field_second_centre(int c0, double r, int lo, int dim, double u) {
    const int left_end = (int)ceil((double)c0 - r) - 1;   // largest integer < c0 - r
    const int right_beg = (int)floor((double)c0 + r) + 1; // smallest integer > c0 + r
    const int nl = max(0, left_end - lo + 1), nr = max(0, dim - max(right_beg, lo));
    const int j = field_randint(0, nl + nr, u);
    return j < nl ? lo + j : max(right_beg, lo) + (j - nl);
}

__device__ __forceinline__ ipp_field_record field_draw(int kind, double r, int H, int W, uint64_t row, uint64_t subseq, uint64_t seed) {
    ipp_field_record f;
    f.rect[1][0] = f.rect[1][1] = f.rect[1][2] = f.rect[1][3] = 0;
    if (kind == IPP_FIELD_HOTSPOT) {
        const double high = field_value(0.7, 1.0, field_uniform(row, 0, subseq, seed));
        const double low = field_value(0.0, 0.3, field_uniform(row, 1, subseq, seed));
        const int lo = (int)r;  // (numpy's randint truncates a float low)
        const int yc = field_randint(lo, H, field_uniform(row, 2, subseq, seed));
        const int xc = field_randint(lo, W, field_uniform(row, 3, subseq, seed));
        const int yc2 = field_second_centre(yc, r, lo, H, field_uniform(row, 4, subseq, seed));
        const int xc2 = field_second_centre(xc, r, lo, W, field_uniform(row, 5, subseq, seed));
        f.inside = high;
        f.outside = low;
        field_cluster(yc, r, H, f.rect[0][0], f.rect[0][1]);
        field_cluster(xc, r, W, f.rect[0][2], f.rect[0][3]);
        field_cluster(yc2, r, H, f.rect[1][0], f.rect[1][1]);
        field_cluster(xc2, r, W, f.rect[1][2], f.rect[1][3]);
    } else {  // IPP_FIELD_SPLIT
        const double high = field_value(0.65, 1.0, field_uniform(row, 0, subseq, seed));
        const double low = field_value(0.0, 0.35, field_uniform(row, 1, subseq, seed));
        const bool swap = field_uniform(row, 2, subseq, seed) > 0.5;
        const bool ysplit = field_uniform(row, 3, subseq, seed) > 0.5;
        const double u = field_uniform(row, 4, subseq, seed);
        f.inside = swap ? low : high;
        f.outside = swap ? high : low;
        f.rect[0][0] = 0; f.rect[0][2] = 0;
        if (ysplit) {
            const int s = field_randint((int)ceil((double)H * 0.33), (int)ceil((double)H * 0.66) + 1, u);
            f.rect[0][1] = s; f.rect[0][3] = W;
        } else {
            const int s = field_randint((int)floor((double)W * 0.33), (int)ceil((double)W * 0.66) + 1, u);
            f.rect[0][1] = H; f.rect[0][3] = s;
        }
    }
    return f;
}

__device__ __forceinline__ bool field_in(const ipp_field_record& f, int y, int x) {
    return (y >= f.rect[0][0] && y < f.rect[0][1] && x >= f.rect[0][2] && x < f.rect[0][3]) ||
           (y >= f.rect[1][0] && y < f.rect[1][1] && x >= f.rect[1][2] && x < f.rect[1][3]);
}

constexpr int kFieldThreads = 256;

// One workgroup per field.  rec != nullptr: field i = rec[i]; else drawn (kind, r) from the GrfNoise keying of the GRF generator
// (row id, group subsequences, REFILL: subseq + episode[env] + 1).  Destination: gt_out [n][N], else the ALTERNATE plane of env
// row_ids[i] (its [N, Npad) tail zeroed, staged flag set).  vec4: the destination rows start 16-byte aligned and hold a multiple of
// 4 floats -- float4 stores.
template <bool REFILL>
__global__ __launch_bounds__(kFieldThreads) void k_fields(View v, int n_items, int kind, double r, const ipp_field_record* __restrict__ rec,
                                                         float* __restrict__ gt_out, GrfNoise gn, int vec4) {
    const int item = blockIdx.x;
    if (item >= n_items) return;
    const int rid = gn.row_ids ? gn.row_ids[item] : item;
    if (gn.row_ids && rid < 0) return;  // (skipped field: padding row of a staged block, or no reset at this position)
    const int env = gt_out ? 0 : rid;
    if (!gt_out && env >= v.cap) return;
    ipp_field_record f;
    if (rec) {
        f = rec[item];
    } else {
        const uint64_t row = (uint64_t)((long long)rid + gn.row_offset);
        const uint64_t subseq = REFILL ? gn.subseq + (uint64_t)(gn.episode[env] + 1)
                                       : gn.subseq + (gn.group_rows > 0 ? (uint64_t)gn.group_subseq[min(item / gn.group_rows, 15)] : 0ull);
        f = field_draw(kind, r, v.H, v.W, row, subseq, gn.seed);
    }
    const float fin = (float)f.inside, fout = (float)f.outside;
    const int W = v.W, N = v.N;
    float* gt = gt_out ? gt_out + (size_t)item * N : v.gt + (size_t)gt_alt_slot(v, env) * v.Npad;
    const int len = gt_out ? N : v.Npad;  // (an env plane's padding tail is written as zeros)
    const int tid = threadIdx.x;
    if (vec4) {
        float4* gt4 = reinterpret_cast<float4*>(gt);
        for (int c = tid; c < len / 4; c += kFieldThreads) {
            const int i0 = 4 * c;
            int y = i0 / W, x = i0 - y * W;
            float o[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                o[h] = (i0 + h < N) ? (field_in(f, y, x) ? fin : fout) : 0.f;
                if (++x == W) { x = 0; ++y; }
            }
            gt4[c] = make_float4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int i = tid; i < len; i += kFieldThreads) {
            const int y = i / W, x = i - y * W;
            gt[i] = (i < N) ? (field_in(f, y, x) ? fin : fout) : 0.f;
        }
    }
    if (!gt_out && tid == 0) v.gt_slot[v.cap + env] = 1;  // the env's next folded reset may flip (stream order: the reset's launch waits for this one)
}

}  // namespace ipp
