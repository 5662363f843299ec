// Host-side internals shared by the library's seven translation units: the one error slot behind ipp_last_error, and the narrow views
// of an engine that the search calls (ipp_search.hip) and the slot calls (ipp_slots.hip) need.  No kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ipp {
int fail(int code, const char* fmt, ...);  // formats the calling thread's ipp_last_error message, returns `code` (ipp_engine.hip)

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return ipp::fail(-2, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct TreeEngine {  // read at every call (ipp_set_uav changes vmax / amax)
    int device, max_batch, node_cap;
    bool tree_ok, patch;  // ipp_tree_step available; tree nodes as patches (k_tree_patch.h)
    double vmax, amax;
};
int tree_engine(void* engine, TreeEngine* out);  // (null engine: "null engine")

// The factor storage of an engine's env slots as the compact replay ring's calls see it (k_replay_compact.h): the slabs of View
struct FactorSlots {
    int device, cap, rank_cap, N, Npad, pstride;
    bool patch;
    uint64_t cov_slot;  // floats per slot
    float* cov; int* colspan; int* colrect; int* rank; double* prior; const float* mean;
    // per-episode priors of the budget ledger (ipp_set_budget_prior; prior_shuffle == 0: off, the rest unused): what prior_start needs
    // to name the prior of an episode again, and the ledger's depth / episode arrays [capacity]
    int prior_shuffle;
    double sv0, ls0;
    uint64_t prior_seed;
    long long prior_row_offset;
    const int* led_depth; const long long* led_episode;
};
int factor_slots(void* engine, FactorSlots* out);  // (null engine: "null engine")

// Everything of an engine's env slots that a packed slot record holds (k_slots.h, ipp_slots.hip): the geometry the record's layout
// depends on and the slabs of View.  A struct of its own, passed to the slot kernels by value: View and FactorSlots stay as they are.
struct SlotStore {
    int device, mode, cap, rank_cap;
    int W, H, N, Npad, pw, ph, pstride, window_rows, tile_cells, prior_kind;
    bool patch;
    uint64_t cov_slot;  // floats per slot
    float* cov; int* colspan; int* colrect; int* rank; double* prior;
    float* mean; float* diag; float* gt; int* gt_slot;
};
int slot_store(void* engine, SlotStore* out);  // (null engine: "null engine")

// ipp_tree_step + the search driver's extras: the item count on the device (n_dev), the edge numerators written by the patch kernel
// itself (edge_out: ipp_common.h); either may be NULL
struct TreeEdgeOut;
int tree_step(void* engine, const int32_t* root_ids, const int32_t* path_ids, const int32_t* new_ids, int32_t n, const double* action,
              const double* prev_action, uint32_t flags, float* reward, int32_t* status, void* stream, const int32_t* n_dev,
              const TreeEdgeOut* edge_out);
}  // namespace ipp
