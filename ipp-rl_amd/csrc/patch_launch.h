// Host side of the patch kernels (k_step_patch.h, k_tree_patch.h): the A/B switches an engine is created under, and
// the LAUNCH PLAN they and the configuration give -- which instantiation a launch of n items runs, the record capacity it stages
// (View::pcap) and its LDS.  No kernels here: ipp_engine.hip maps a PatchVariant to its kernel through its list of instantiations.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <optional>

#include "k_step_patch.h"

#ifndef IPP_PATCH_BIGKP
#define IPP_PATCH_BIGKP 4  // rows per request group of the six-waves-per-SIMD instantiation of k_step_patch
#endif

namespace ipp {

// Every IPP_* switch that plan() and engine creation consult (A/B experiments and tests).  Constructing a Switches parses them, here and
// nowhere else; an empty optional is an unset variable, a value is atoi() of its text.
inline std::optional<int> env_int(const char* name) { const char* s = getenv(name); return s ? std::optional<int>(atoi(s)) : std::nullopt; }
inline int env_int_in(const char* name, int lo, int hi, int otherwise) { const int x = env_int(name).value_or(otherwise); return x >= lo && x <= hi ? x : otherwise; }
struct Switches {
    std::optional<int> patch = env_int("IPP_PATCH");                               // 0 selects the band-tile kernels
    std::optional<int> patch_cap = env_int("IPP_PATCH_CAP");                       // records staged in LDS, at least 8 (A/B, overflow tests): no launch-size tiers then
    int two_min_items = std::max(0, env_int("IPP_PATCH_TWO_MIN").value_or(6144));  // smallest launch that runs two waves per item (0: never)
    int big_min_items = env_int("IPP_PATCH_BIG").value_or(16384);                  // smallest launch that takes the six-waves-per-SIMD form (0: never)
    // the A/B switches of the band-tile kernels: the presence of any of these four selects those kernels (no patch layout)
    std::optional<int> rect = env_int("IPP_RECT");                // rectangle tiles: 0 off, 1 predict-only, 2 always
    std::optional<int> rect_meta = env_int("IPP_RECT_META");      // 0: no rectangle metadata
    std::optional<int> fused = env_int("IPP_FUSED");              // 0: prologue and gain kernel as two launches
    std::optional<int> step_chunks = env_int("IPP_STEP_CHUNKS");  // chunks of a step (0: auto)
    std::optional<int> rect_tree = env_int("IPP_RECT_TREE");      // tree steps on rectangle tiles
    std::optional<int> tree_split = env_int("IPP_TREE_SPLIT");    // smallest tree launch that runs k_tree_prepare + k_tree_gain (0: never)
    std::optional<int> grf_fft = env_int("IPP_GRF_FFT");          // 0: the GEMM form of the Hartley ground truths
    std::optional<int> grf_hartley = env_int("IPP_GRF_HARTLEY");  // 0: no Hartley form at all: even n <= 128 run k_grf_dft
};

// One instantiation of k_step_patch<NW, KPN, MINW, RJN, BUD> (k_tree_patch<NW, RJN>) and what a launch of it is given.
struct PatchVariant {
    int min_items;             // the plan runs it on launches of at least this many items
    int waves, kpn, minw;      // NW waves per item (workgroups of 64 * waves threads), KPN stored rows per request group, MINW waves per SIMD of the launch bound
    int rjn;                   // RJN: form of the rounds over the columns' rectangles (k_step_patch.h)
    int pcap;                  // records staged in LDS: View::pcap of the launch
    size_t lds;                // dynamic LDS bytes
};
struct PatchPlan {
    // Env steps by launch size: tier[0] from 0 items; a later tier takes the launches that reach the one before it and have at least its
    // min_items (the default engine: three waves from 0, two waves from 6144, two waves / four rows / six per SIMD from 16384)
    PatchVariant tier[3];
    int n_tiers = 0, two_wave_tier = 0, big_tier = 0;  // (index of the tier of that form; 0: none -- ipp_info)
    PatchVariant tree;   // k_tree_patch, every launch size
};

// The variant a launch of n items runs: the only place a launch size meets a threshold.
inline const PatchVariant& pick(const PatchPlan& p, int n) {
    int t = 0;
    while (t + 1 < p.n_tiers && n >= p.tier[t + 1].min_items) ++t;
    return p.tier[t];
}

// LDS of a patch kernel with `cap` records staged
inline size_t patch_lds_bytes(const View& v, int cap, int waves) {
    return PatchLds::bytes(cap, v.plw * v.plw, waves, v.punits, v.rank_cap);
}
inline PatchVariant patch_variant(const View& v, int min_items, int waves, int kpn, int minw, int rjn, int pcap) {
    return {min_items, waves, kpn, minw, rjn, pcap, patch_lds_bytes(v, pcap, waves)};
}

// Column records a workgroup stages in LDS: what fits its share when wgs_per_cu workgroups of the kernel are resident per CU.
// (The LDS of a workgroup is allocated in granules of 1280 bytes on gfx950: 16 KB would take 13 of the 128.)
//   min_records  fewest records that justify the tier; when they do not fit, the capacity is `fallback`
//   prev_cap     a tier for larger launches stages no more than the tier before it
// A staging capacity below the rank is a multiple of 8: the m x m algebra sums the records in groups of eight, so S does not depend
// on where a record is staged (solve_wave_fast).
inline int staged_records(int records, int rank_cap) { return records >= rank_cap ? rank_cap : (records & ~7); }
inline int lds_share_records(const View& v, int wgs_per_cu, int waves, int min_records, int fallback, int prev_cap = INT_MAX) {
    const size_t rec = kPatchRec * 4;
    size_t budget = (size_t)160 * 1024 / wgs_per_cu / 1280 * 1280;
    // (at most 13 granules: 170 records are more than the two register pages of the unit loop hold, and the 8
    // workgroups of the default configuration then leave 30 KB of the CU's LDS to the ground-truth kernel that runs beside the steps)
    budget = std::min(budget, (size_t)13 * 1280);
    const size_t fixed = patch_lds_bytes(v, 0, waves);
    if (fixed + min_records * rec > budget) return std::min(staged_records(fallback, v.rank_cap), prev_cap);
    const int fit = (int)((budget - fixed) / rec);
    // (one record of the share stays free)
    return std::min(staged_records(fit - 1, v.rank_cap), prev_cap);
}

// The plan of a patch engine: v carries the geometry (plw, punits) and rank_cap.  tier[0].pcap is the engine's View::pcap.
inline PatchPlan make_patch_plan(const View& v, const Switches& sw) {
    PatchPlan p = {};
    static_assert(kPatchWavesDefault == 3, "the first tier's RJN counts rounds of 192 threads");
    // kPatchWavesPerCu waves of the kernel resident per CU; three waves: rounds of 192 threads over the columns' rectangles (k_step_patch.h, RJN)
    const int pcap = sw.patch_cap ? staged_records(std::max(8, *sw.patch_cap), v.rank_cap)
                                  : lds_share_records(v, kPatchWavesPerCu / kPatchWavesDefault, kPatchWavesDefault, 17, 16);
    p.tier[p.n_tiers++] = patch_variant(v, 0, kPatchWavesDefault, kPatchKP, kPatchMinW, v.rank_cap <= 192 ? 1 : v.rank_cap <= 384 ? 2 : 0, pcap);
    if (!sw.patch_cap && sw.two_min_items > 0) {
        // Launch-size rule of the default engine (round 6).  Three waves per item shorten the chains of the heaviest items, which end
        // a launch of one or two rounds of workgroup slots (2048 items: 55 M env-steps/s against 37 M with two waves); a launch of
        // many rounds has no tail to shorten and is paid in items in flight: two waves per item are 12 items per CU instead of 8
        // (3072 slots).  Same box, two groups of launches: 8192 envs of 50x50 (4096 items per launch) 64.9 M with three waves against
        // 54.5 M with two; 16384 envs 62.9 against 66.5 M; 32768 envs (configs[3] share) 61.8-64.3 against 66.1 M; configs[2]
        // 66.1-67.0 against 70.1-71.6 M (profiles/r06_experiments.txt 3).  Same arithmetic per cell, same order: bit-identical results
        // (tests/test_hip_two_waves.py).  IPP_PATCH_TWO_MIN=<items> (0: never) for A/B.
        p.two_wave_tier = p.n_tiers;
        p.tier[p.n_tiers++] = patch_variant(v, sw.two_min_items, 2, kPatchKP, kPatchMinW, 0, lds_share_records(v, 12, 2, 17, 16, pcap));
    }
    if (p.two_wave_tier && sw.big_min_items > 0) {
        // second configuration for large launches of two waves per item, LDS share of 12 workgroups per CU (10 granules of 1280 bytes) as
        // well: six waves per SIMD pay once a launch is many rounds of workgroups (k_step_patch.h).  Only where 32 records and one to spare fit.
        const int pc = lds_share_records(v, 12, 2, 33, 0, p.tier[p.n_tiers - 1].pcap);
        if (pc > 0) p.big_tier = p.n_tiers;
        if (pc > 0) p.tier[p.n_tiers++] = patch_variant(v, sw.big_min_items, 2, IPP_PATCH_BIGKP, 6, 0, pc);
    }
    // tree nodes on patches: the first tier's waves and staging; its reduced rounds exist for rank_cap <= 192 only
    p.tree = patch_variant(v, 0, kPatchWavesDefault, kPatchKP, kPatchMinW, v.rank_cap <= 192 ? 1 : 0, pcap);
    return p;
}

}  // namespace ipp
