// The white noise a Gaussian-random-field generator draws for itself, and where such a field goes: ONE definition for every family
// (k_grf_fft.h, k_grf_hartley.h, k_grf_dft.h).
//
// Noise (white == nullptr): the numbers ipp_fill_normal_rows would have written for row id r = (row_ids ? row_ids[item] : item) +
// row_offset of a row_len = N fill -- element e of the field is normal e & 3 of Philox counter r * ceil(N / 4) + (e >> 2) -- so the fill
// kernel's 4 N bytes per field written and read back do not exist (160 MB per step of BASELINE configs[2], 13 % of its GPU time), and a
// budget step's refill list, which lives on the device, needs no host read to turn into fields.
#pragma once
#include "ipp_common.h"

namespace ipp {

struct GrfNoise {
    const int* row_ids;
    long long row_offset;
    uint64_t seed, subseq;
    // fields of several episodes in one launch (ipp_generate_grf_groups): field i belongs to group i / group_rows and draws from
    // subseq + group_subseq[group] (by value: no upload in front of the launch); group_rows == 0: one group.  A NEGATIVE row id skips the field.
    int group_rows;
    long long group_subseq[16];
    int to_alt;  // gt_out == NULL: field i goes to the ALTERNATE ground-truth plane of env row_ids[i] (staged for its next episode; the reset flips)
    const long long* episode;  // REFILL (ipp_generate_grf_refill): [capacity] current episode of every env; field i draws from subseq + episode[env] + 1
};

// field `item` of a drawn launch is skipped (padding row of a staged block, no reset at this position of a refill list)
__device__ __forceinline__ bool grf_noise_skip(const float* white, const GrfNoise& gn, int item) {
    return !white && gn.row_ids && gn.row_ids[item] < 0;
}

// env slot of field `item` (0 with a caller's destination, which has no env)
__device__ __forceinline__ int grf_item_env(const float* gt_out, const int* env_ids, const GrfNoise& gn, int item) {
    return gt_out ? 0 : (gn.to_alt ? gn.row_ids[item] : (env_ids ? env_ids[item] : item));
}

// Philox row id and subsequence of field `item`: plain rows, groups, or (refill) the episode after the env's current one
__device__ __forceinline__ uint64_t grf_noise_row(const GrfNoise& gn, int item) {
    return (uint64_t)((gn.row_ids ? (long long)gn.row_ids[item] : (long long)item) + gn.row_offset);
}
__device__ __forceinline__ uint64_t grf_noise_subseq(const GrfNoise& gn, int item, int env, bool refill) {
    return refill ? gn.subseq + (uint64_t)(gn.episode[env] + 1)
                  : gn.subseq + (gn.group_rows > 0 ? (uint64_t)gn.group_subseq[min(item / gn.group_rows, 15)] : 0ull);
}

// The N normals of one field, four per counter, spread over the NT threads of its workgroup: put(e, x) receives element e < N.
template <int NT, typename Put>
__device__ __forceinline__ void grf_noise_draw(const GrfNoise& gn, int item, int env, bool refill, int N, int tid, Put put) {
    const uint64_t rid = grf_noise_row(gn, item);
    const uint64_t subseq = grf_noise_subseq(gn, item, env, refill);
    const int qpr = (N + 3) / 4;  // counters per row
    for (int qc = tid; qc < qpr; qc += NT) {
        float nrm[4];
        philox_normal4(rid * (uint64_t)qpr + (uint64_t)qc, subseq, gn.seed, nrm);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int e = 4 * qc + h;
            if (e < N) put(e, nrm[h]);
        }
    }
}

// ... the same normals as 16-byte vector stores into a field's own destination (4 | N, dst 16-byte aligned): the generators whose
// noise does not fit their LDS keep it there until the field overwrites it.
template <int NT>
__device__ __forceinline__ void grf_noise_store(const GrfNoise& gn, int item, int env, bool refill, int N, int tid, float* dst) {
    const uint64_t rid = grf_noise_row(gn, item);
    const uint64_t subseq = grf_noise_subseq(gn, item, env, refill);
    const int qpr = N / 4;
    for (int qc = tid; qc < qpr; qc += NT) {
        float nrm[4];
        philox_normal4(rid * (uint64_t)qpr + (uint64_t)qc, subseq, gn.seed, nrm);
        reinterpret_cast<float4*>(dst)[qc] = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
    }
}

// Destination of field `item`: the caller's row, the env's alternate plane (to_alt), or its current plane
__device__ __forceinline__ float* grf_dest(const View& v, float* gt_out, const GrfNoise& gn, int item, int env, int N) {
    return gt_out ? gt_out + (size_t)item * N : (gn.to_alt ? v.gt + (size_t)gt_alt_slot(v, env) * v.Npad : gt_plane(v, env));
}

// Behind the field's cells in an env plane: the pad cells zeroed, and -- alternate plane -- the staged flag, written last: the env's
// next folded reset may flip (stream order: the reset's launch waits for this one)
template <int NT>
__device__ __forceinline__ void grf_dest_finish(const View& v, const float* gt_out, const GrfNoise& gn, float* gt, int env, int N, int tid) {
    if (!gt_out)
        for (int i = N + tid; i < v.Npad; i += NT) gt[i] = 0.f;
    if (!gt_out && gn.to_alt && tid == 0) v.gt_slot[v.cap + env] = 1;
}

}  // namespace ipp
