// The slot export / import calls of the C-ABI (include/ipp_engine.h, "Slot export and import").  A translation unit of its own: it sees
// an engine through ipp_host.h (SlotStore), not through the step kernels, and is the only one that includes k_slots.h.
#include <algorithm>

#include "ipp_common.h"
#include "ipp_host.h"
#include "k_slots.h"

using namespace ipp;

namespace {
constexpr int kSlotItemsPerLaunch = 65535;  // (gridDim.y)

int slots_check(void* engine, const char* call, const void* a, const void* b, const void* c, int32_t n, uint32_t what, SlotStore* st) {
    if (!engine) return fail(-1, "%s: null engine", call);
    if (int err = slot_store(engine, st)) return err;
    if (!a || !b || !c) return fail(-1, "%s: null argument", call);
    if (n < 0) return fail(-1, "%s: n = %d < 0", call, n);
    if (what == 0 || (what & ~(IPP_SLOT_COLUMNS | IPP_SLOT_MAPS))) return fail(-1, "%s: what = 0x%x selects no section or an unknown one", call, what);
    if (st->mode != IPP_FACTOR)
        return fail(-1, "%s: a dense engine has no factor slots to pack (ipp_read_cov_dense / ipp_write_cov_dense move its P)", call);
    if (!st->patch) return fail(-1, "%s needs the patch-layout windowed factor engine (ipp_info.patch_layout == 1)", call);
    if ((st->Npad & 3) || (st->pstride & 15) || st->Npad < ((st->N + 3) & ~3))
        return fail(-1, "%s: Npad = %d, pstride = %d: not the patch layout's multiples", call, st->Npad, st->pstride);
    return 0;
}

int slot_chunks(const SlotStore& st) {  // 1024 float4 per workgroup and pass, at most 64 workgroups per slot (as ipp_fork's and the archive's)
    const uint64_t n4 = (uint64_t)st.rank_cap * (uint64_t)st.pstride / 4;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(64, (n4 + 1023) / 1024));
}
}  // namespace

extern "C" {

int ipp_slots_layout(void* engine, ipp_slot_layout* out) {
    if (!engine || !out) return fail(-1, "ipp_slots_layout: null argument");
    SlotStore st;
    if (int err = slot_store(engine, &st)) return err;
    if (st.mode != IPP_FACTOR) return fail(-1, "ipp_slots_layout: a dense engine has no factor slots to pack");
    if (!st.patch) return fail(-1, "ipp_slots_layout needs the patch-layout windowed factor engine (ipp_info.patch_layout == 1)");
    *out = ipp_slot_layout{IPP_SLOT_FORMAT, st.W, st.H, st.N, st.Npad, st.pw, st.ph, st.pstride, st.window_rows, st.tile_cells, st.prior_kind, 0};
    return 0;
}

int ipp_slots_plan(void* engine, const int32_t* slot_ids, int32_t n, uint32_t what, uint64_t* offsets, int32_t* status, void* stream) {
    SlotStore st;
    if (int err = slots_check(engine, "ipp_slots_plan", slot_ids, offsets, status, n, what, &st)) return err;
    HIP_TRY(hipSetDevice(st.device));
    hipLaunchKernelGGL(k_slots_plan, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), st, slot_ids, (int)n, what,
                       reinterpret_cast<unsigned long long*>(offsets), status);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_slots_export(void* engine, const int32_t* slot_ids, int32_t n, uint32_t what, const uint64_t* offsets, void* blob, void* stream) {
    SlotStore st;
    if (int err = slots_check(engine, "ipp_slots_export", slot_ids, offsets, blob, n, what, &st)) return err;
    if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(-1, "ipp_slots_export: blob is not 16-byte aligned");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(st.device));
    const int chunks = slot_chunks(st);
    for (int o = 0; o < n; o += kSlotItemsPerLaunch) {
        const int cnt = std::min(kSlotItemsPerLaunch, n - o);
        hipLaunchKernelGGL(k_slots_export, dim3(chunks, cnt), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), st, slot_ids + o, cnt, what,
                           reinterpret_cast<const unsigned long long*>(offsets) + o, reinterpret_cast<unsigned char*>(blob));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_slots_import(void* engine, const int32_t* slot_ids, int32_t n, uint32_t what, const uint64_t* offsets, const void* blob,
                     int32_t* status, void* stream) {
    SlotStore st;
    if (int err = slots_check(engine, "ipp_slots_import", slot_ids, offsets, blob, n, what, &st)) return err;
    if (!status) return fail(-1, "ipp_slots_import: null argument");
    if (reinterpret_cast<uintptr_t>(blob) & 15) return fail(-1, "ipp_slots_import: blob is not 16-byte aligned");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(st.device));
    const int chunks = slot_chunks(st);
    for (int o = 0; o < n; o += kSlotItemsPerLaunch) {
        const int cnt = std::min(kSlotItemsPerLaunch, n - o);
        hipLaunchKernelGGL(k_slots_import, dim3(chunks, cnt), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), st, slot_ids + o, cnt, what,
                           reinterpret_cast<const unsigned long long*>(offsets) + o, reinterpret_cast<const unsigned char*>(blob), status + o);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
