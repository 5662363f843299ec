// Slot export and import (include/ipp_engine.h, "Slot export and import"): the state of env slots of a patch-layout factor engine as
// packed records in caller memory and back.  The record format is the table in the header; slot_record_bytes and the slot_off_*
// functions below are its arithmetic (restated in NumPy by ipp-rl_amd/slots.py, the CPU-testable definition).  The kernels:
//   k_slots_plan     one workgroup: the exclusive scan of the named slots' record sizes (a function of each slot's rank, read here) and
//                    the per-slot status
//   k_slots_export   grid (chunks, n): the columns of slot blockIdx.y in float4 strides over the chunks; chunk 0 also the header, the
//                    prior pair, spans and rectangles, and the three maps
//   k_slots_import   the inverse.  Every workgroup of a slot derives the slot's status from the record's header alone (the blob is
//                    read-only here), so no workgroup writes anything of a refused slot and none reads a rank another one replaces
// Bandwidth kernels: 16 bytes per lane and access on the blob side and on the column storage, vector stores only.  Workgroups are
// indexed by the slot's rank, not rank_cap: a chunk behind the last column costs an exit.
#pragma once
#include "ipp_common.h"
#include "ipp_host.h"

namespace ipp {

__host__ __device__ __forceinline__ unsigned long long slot_pad16(unsigned long long b) { return (b + 15ull) & ~15ull; }
// byte offsets of a record's parts from its start (what, rank r, N cells, pstride floats per column)
__host__ __device__ __forceinline__ unsigned long long slot_off_prior(unsigned what) { return IPP_SLOT_HEADER_BYTES; }
__host__ __device__ __forceinline__ unsigned long long slot_off_colspan(unsigned what) { return slot_off_prior(what) + 16; }
__host__ __device__ __forceinline__ unsigned long long slot_off_colrect(unsigned what, int r) { return slot_off_colspan(what) + slot_pad16(4ull * r); }
__host__ __device__ __forceinline__ unsigned long long slot_off_columns(unsigned what, int r) { return slot_off_colrect(what, r) + slot_pad16(4ull * r); }
__host__ __device__ __forceinline__ unsigned long long slot_off_maps(unsigned what, int r, int pstride) {
    return (what & IPP_SLOT_COLUMNS) ? slot_off_columns(what, r) + 4ull * (unsigned long long)r * (unsigned long long)pstride
                                     : (unsigned long long)IPP_SLOT_HEADER_BYTES;
}
__host__ __device__ __forceinline__ unsigned long long slot_record_bytes(unsigned what, int r, int N, int pstride) {
    return slot_off_maps(what, r, pstride) + ((what & IPP_SLOT_MAPS) ? 3ull * slot_pad16(4ull * N) : 0ull);
}

__device__ __forceinline__ int slot_rank(const SlotStore& st, int e) {
    const int r = st.rank[e];
    return r < 0 ? 0 : (r > st.rank_cap ? st.rank_cap : r);
}

__global__ __launch_bounds__(256) void k_slots_plan(SlotStore st, const int* __restrict__ ids, int n, unsigned what,
                                                    unsigned long long* __restrict__ offsets, int* __restrict__ status) {
    __shared__ unsigned long long wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long carry = 0;  // (every thread keeps the same running total)
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        unsigned long long sz = 0;
        if (i < n) {
            const int e = ids[i];
            const bool ok = e >= 0 && e < st.cap;
            sz = ok ? slot_record_bytes(what, (what & IPP_SLOT_COLUMNS) ? slot_rank(st, e) : 0, st.N, st.pstride)
                    : (unsigned long long)IPP_SLOT_HEADER_BYTES;
            status[i] = ok ? IPP_SLOT_OK : IPP_SLOT_BAD_ID;
        }
        unsigned long long x = sz;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        unsigned long long pre = carry;
        for (int j = 0; j < w; ++j) pre += wsum[j];
        if (i < n) offsets[i] = pre + x - sz;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();  // (the sums are read before the next round replaces them)
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

// one map [N] of the engine (a slab row: 16-byte aligned, Npad >= N rounded up to 4) -> its padded part of the record
__device__ __forceinline__ void slot_map_out(const float* __restrict__ src, unsigned char* dst, int N) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int g = threadIdx.x; 4 * g < N; g += blockDim.x) {
        float4 x = s4[g];
        if (4 * g + 1 >= N) x.y = 0.f;  // (the padding of a record is zero)
        if (4 * g + 2 >= N) x.z = 0.f;
        if (4 * g + 3 >= N) x.w = 0.f;
        d4[g] = x;
    }
}
// ... and back, the whole slab row: the cells [N, Npad) become zero, as a reset leaves them (wave_reset_env: ipp_common.h); the
// record's own padding is zero, so a last partial group is one float4 as well
__device__ __forceinline__ void slot_map_in(const unsigned char* src, float* __restrict__ dst, int N, int Npad) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int g = threadIdx.x; 4 * g < Npad; g += blockDim.x) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * g < N) {
            x = s4[g];
            if (4 * g + 1 >= N) x.y = 0.f;
            if (4 * g + 2 >= N) x.z = 0.f;
            if (4 * g + 3 >= N) x.w = 0.f;
        }
        d4[g] = x;
    }
}

__global__ __launch_bounds__(256) void k_slots_export(SlotStore st, const int* __restrict__ ids, int n, unsigned what,
                                                      const unsigned long long* __restrict__ offsets, unsigned char* __restrict__ blob) {
    const int item = blockIdx.y;
    if (item >= n) return;
    const unsigned long long off = offsets[item];
    if (off & 15ull) return;  // (not an ipp_slots_plan offset)
    const int e = ids[item];
    const bool ok = e >= 0 && e < st.cap;
    const bool cols = ok && (what & IPP_SLOT_COLUMNS);
    const int r = cols ? slot_rank(st, e) : 0;
    unsigned char* rec = blob + off;
    if (cols) {
        const size_t n4 = (size_t)r * st.pstride / 4;  // (a stored column is pstride floats, a multiple of 16)
        const float4* cs = reinterpret_cast<const float4*>(st.cov + (size_t)e * st.cov_slot);
        float4* cd = reinterpret_cast<float4*>(rec + slot_off_columns(what, r));
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) cd[i] = cs[i];
    }
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        const unsigned w = ok ? what : 0u;
        const unsigned long long bytes = ok ? slot_record_bytes(what, r, st.N, st.pstride) : (unsigned long long)IPP_SLOT_HEADER_BYTES;
        uint4* h = reinterpret_cast<uint4*>(rec);
        h[0] = make_uint4(IPP_SLOT_MAGIC, (unsigned)IPP_SLOT_FORMAT, w, (unsigned)r);
        h[1] = make_uint4((unsigned)(bytes & 0xffffffffull), (unsigned)(bytes >> 32), (unsigned)st.N, (unsigned)st.pstride);
        if (cols) *reinterpret_cast<double2*>(rec + slot_off_prior(what)) = *reinterpret_cast<const double2*>(st.prior + 2 * (size_t)e);
    }
    if (!ok) return;
    if (cols) {
        const int* span = st.colspan + (size_t)e * st.rank_cap;  // (rank_cap ints per slot: no 16-byte alignment on this side)
        const int* rect = st.colrect + (size_t)e * st.rank_cap;
        int4* ds = reinterpret_cast<int4*>(rec + slot_off_colspan(what));
        int4* dr = reinterpret_cast<int4*>(rec + slot_off_colrect(what, r));
        for (int g = threadIdx.x; 4 * g < r; g += blockDim.x) {
            const int k = 4 * g;
            ds[g] = make_int4(span[k], k + 1 < r ? span[k + 1] : 0, k + 2 < r ? span[k + 2] : 0, k + 3 < r ? span[k + 3] : 0);
            dr[g] = make_int4(rect[k], k + 1 < r ? rect[k + 1] : 0, k + 2 < r ? rect[k + 2] : 0, k + 3 < r ? rect[k + 3] : 0);
        }
    }
    if (what & IPP_SLOT_MAPS) {
        const unsigned long long m0 = slot_off_maps(what, r, st.pstride), ms = slot_pad16(4ull * st.N);
        slot_map_out(st.mean + (size_t)e * st.Npad, rec + m0, st.N);
        slot_map_out(st.diag + (size_t)e * st.Npad, rec + m0 + ms, st.N);
        int p = st.gt_slot[e];  // the plane the slot reads now: e or cap + e
        if (p != e && p != st.cap + e) p = e;
        slot_map_out(st.gt + (size_t)p * st.Npad, rec + m0 + 2 * ms, st.N);
    }
}

__global__ __launch_bounds__(256) void k_slots_import(SlotStore st, const int* __restrict__ ids, int n, unsigned what,
                                                      const unsigned long long* __restrict__ offsets, const unsigned char* __restrict__ blob,
                                                      int* __restrict__ status) {
    const int item = blockIdx.y;
    if (item >= n) return;
    const int e = ids[item];
    const unsigned long long off = offsets[item], end = offsets[item + 1];
    int s = IPP_SLOT_OK, r = 0;
    if (e < 0 || e >= st.cap) {
        s = IPP_SLOT_BAD_ID;
    } else if ((off & 15ull) || end < off + IPP_SLOT_HEADER_BYTES) {
        s = IPP_SLOT_BAD_RECORD;
    } else {
        const uint4* h = reinterpret_cast<const uint4*>(blob + off);
        const uint4 h0 = h[0], h1 = h[1];
        const unsigned long long bytes = (unsigned long long)h1.x | ((unsigned long long)h1.y << 32);
        r = (int)h0.w;
        if (h0.x != IPP_SLOT_MAGIC || h0.y != (unsigned)IPP_SLOT_FORMAT || h0.z != what || r < 0 || r > (1 << 24) || (int)h1.z != st.N ||
            (int)h1.w != st.pstride || bytes != end - off || bytes != slot_record_bytes(what, r, st.N, st.pstride))
            s = IPP_SLOT_BAD_RECORD;
        else if ((what & IPP_SLOT_COLUMNS) && r > st.rank_cap)
            s = IPP_SLOT_RANK;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) status[item] = s;
    if (s != IPP_SLOT_OK) return;  // (the slot stays bit for bit as it was)
    const unsigned char* rec = blob + off;
    const bool cols = (what & IPP_SLOT_COLUMNS) != 0;
    if (cols) {
        const size_t n4 = (size_t)r * st.pstride / 4;
        const float4* cs = reinterpret_cast<const float4*>(rec + slot_off_columns(what, r));
        float4* cd = reinterpret_cast<float4*>(st.cov + (size_t)e * st.cov_slot);
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) cd[i] = cs[i];
    }
    if (blockIdx.x != 0) return;
    if (cols) {
        int* span = st.colspan + (size_t)e * st.rank_cap;
        int* rect = st.colrect + (size_t)e * st.rank_cap;
        const int4* ss = reinterpret_cast<const int4*>(rec + slot_off_colspan(what));
        const int4* sr = reinterpret_cast<const int4*>(rec + slot_off_colrect(what, r));
        for (int g = threadIdx.x; 4 * g < r; g += blockDim.x) {
            const int k = 4 * g;
            const int4 a = ss[g], b = sr[g];
            span[k] = a.x; rect[k] = b.x;
            if (k + 1 < r) { span[k + 1] = a.y; rect[k + 1] = b.y; }
            if (k + 2 < r) { span[k + 2] = a.z; rect[k + 2] = b.z; }
            if (k + 3 < r) { span[k + 3] = a.w; rect[k + 3] = b.w; }
        }
        if (threadIdx.x == 0) {
            *reinterpret_cast<double2*>(st.prior + 2 * (size_t)e) = *reinterpret_cast<const double2*>(rec + slot_off_prior(what));
            st.rank[e] = r;
        }
    }
    if (what & IPP_SLOT_MAPS) {
        const unsigned long long m0 = slot_off_maps(what, r, st.pstride), ms = slot_pad16(4ull * st.N);
        slot_map_in(rec + m0, st.mean + (size_t)e * st.Npad, st.N, st.Npad);
        slot_map_in(rec + m0 + ms, st.diag + (size_t)e * st.Npad, st.N, st.Npad);
        slot_map_in(rec + m0 + 2 * ms, st.gt + (size_t)e * st.Npad, st.N, st.Npad);  // plane e becomes the slot's plane, nothing staged
        if (threadIdx.x == 0) {
            st.gt_slot[e] = e;
            st.gt_slot[st.cap + e] = 0;
        }
    }
}

}  // namespace ipp
