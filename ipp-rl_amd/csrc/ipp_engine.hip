// C-ABI of the MI355X-native batched IPP environment-step engine (see include/ipp_engine.h).
// One of the five translation units of libipp_hip.so (csrc/Makefile); the search and self-play calls are in ipp_search.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ipp_common.h"
#include "ipp_host.h"
#include "k_gain.h"
#include "k_gain_factor.h"
#include "k_step_factor.h"
#include "k_step_patch.h"
#include "k_gain_wave.h"
#include "k_misc.h"
#include "k_grf_dft.h"
#include "k_grf_hartley.h"
#include "k_grf_fft.h"
#include "k_fields.h"
#include "k_score.h"
#include "k_score_batch.h"
#include "k_plane.h"
#include "k_feature_planes.h"
#include "k_tree.h"
#include "k_tree_patch.h"
#include "k_prepare.h"
#include "patch_launch.h"

using namespace ipp;

static thread_local std::string g_err;
int ipp::fail(int code, const char* fmt, ...) {  // (ipp_host.h: every translation unit of the library reports through this slot)
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

constexpr uint64_t kAlign = 256;
constexpr int kMaxChunks = 8;
inline uint64_t up(uint64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct ProfEvent { hipEvent_t a, b; int kind; };
constexpr int kProfKinds = 4;  // 0 streaming kernel, 1 dense downdate, 2 prologue kernel; 3: every launch of a step (busy time only)
struct ProfSlot {
    double total_ms = 0.0;
    int64_t launches = 0;
    double busy_ms = 0.0;       // union of the dispatches' [start, stop] intervals (launches of different streams overlap)
    int64_t busy_launches = 0;
};

struct Engine {
    ipp_config cfg;
    int device;
    View v;
    int n_bands;
    uint64_t used_bytes;
    size_t prep_lds;
    size_t gain_lds;
    int q_chunk;
    TreeView tv = {};      // node pool of ipp_tree_step (node_cap == 0: none)
    float* node_diag_scratch = nullptr;  // [Npad] assembled diagonal of a node state (ipp_tree_score_actions)
    bool scoring = false;  // arena holds the ipp_score_actions scratch
    ScoreView sv = {};
    bool grf_dft = false;  // even square grids up to 256: k_grf_dft instead of k_grf_conv + k_grf_norm
    int grf_tt = 0;        // > 0: even square grids up to 128: k_grf_hartley<grf_tt> (fp64 MFMA GEMMs)
    bool grf_fft = false;  // ... and n = 50 / 100: k_grf_fft (fast Hartley transforms) on the same amplitude table
    bool grf_rows_all = false;  // ipp_set_grf_rows: every family above draws its own noise (rows / groups / refill calls on every even square grid <= 256)
    int grf_kc = 1;        // spectrum rows per LDS chunk
    int lut_cap;
    int lut_rows = 0;  // workgroup-per-item factor kernels: rows |drow| of the prior table kept in LDS
    bool profile = false;
    int step_chunks = 0;  // 0 = auto
    bool fused = false;   // k_step_factor instead of k_prepare + k_gain_factor
    bool tree_ok = false; // ipp_tree_step available (fused engines; MC = 25: the fused tree kernel beside two-launch env steps)
    size_t tree_fused_lds = 0;
    bool patch = false;   // k_step_patch on compact column patches (View::patch)
    PatchPlan pp;         // ... which instantiation a launch runs, its record capacity and LDS (patch_launch.h)
    const double* reset_prior = nullptr;  // ipp_set_reset_prior: priors of the episodes started by ipp_step_autoreset
    Ledger led = {};                      // ipp_set_budget: the budget ledger of IPP_BUDGET steps (budget == NULL: none installed)
    bool rect_ok = false;      // rectangle tiles (k_gain_factor.h) possible: clipped windows, 128-cell tiles, even grid width
    bool rect_commit = false;  // ... used for committed steps too (else for predict-only calls only)
    bool rect_tree = false;    // tree steps on rectangle tiles (same width rule; either tile size)
    int tree_split_min = 0;   // ipp_tree_step: launches of at least this many items run k_tree_prepare + k_tree_gain (0: never)
    int tree_T = kStepThreads;  // workgroup size of k_tree_gain
    size_t tree_step_lds = 0;   // k_tree_step: the fused kernel's LDS + the column-pointer table
    size_t tree_gain_lds = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t ev_prep[8] = {};
    ProfSlot prof[kProfKinds];
    std::vector<ProfEvent> prof_pending;
    int last_n = 0;
    uint64_t last_needed_bytes = 0;  // of the last ipp_streamed_bytes(_detail) read
};

struct Layout {
    int N, Npad, T, n_tiles, win_tiles, MC, FC, QS, q_rows, VEC;
    bool patch;
    PatchGeo pg;
    uint64_t off_mean, off_diag, off_gt, off_gtslot, off_prior, off_rank, off_span, off_cnt, off_icnt, off_cov, off_hdr, off_linv, off_yv, off_q, off_wc,
        off_partial, off_dbg, off_grfh, off_grfcs, off_grfg, off_grfhp, off_grfamp, off_grfraw, off_grfraw2, off_sc_hdr, off_sc_ext, off_sc_mask, off_sc_G, off_sc_P, off_tr_cov, off_tr_diag, off_tr_meta, off_sc_ndiag, total, cov_slot_floats;
};

uint64_t q_item_floats(const Layout& L) {
    const uint64_t lq = ((uint64_t)L.MC * L.MC + L.MC + 3) & ~(uint64_t)3;
    // multiple of 16 floats: item blocks start on 64-byte lines (no scalar-cache line shared between two items)
    uint64_t q = lq + (uint64_t)(L.q_rows + 8) * L.QS;
    if (L.patch) q = std::max<uint64_t>(q, (uint64_t)L.q_rows * kPatchRec);  // column records that overflow the LDS staging
    return (q + 15) & ~(uint64_t)15;
}

// Compact column patches + k_step_patch / k_tree_patch (k_step_patch.h, k_tree_patch.h): windowed factor engines on grids wide enough for two-dimensional windows, MC = 9.  Any of the A/B
// switches of the band-tile kernels selects those kernels instead; IPP_PATCH=0 does so explicitly.
bool patch_layout(const ipp_config& c, int MC, const Switches& sw) {
    if (c.state_repr != IPP_FACTOR || c.window_rows <= 0 || MC != 9) return false;
    if (c.tile_threads != 0) return false;
    if (c.x_dim % 2 != 0 || c.x_dim > 256 || c.y_dim > 256) return false;
    if (!(c.x_dim > 2 * c.window_rows + 13)) return false;
    if (c.rank_cap > kPatchMaxRank) return false;
    if (c.window_rows > 25) return false;  // (prior table of (R + 7)^2 floats and patches of (2 R + 6) x (2 R + 7) cells: small windows only)
    {   // the units map a cell index to (row, column) of a rectangle through a reciprocal: exact for every width and index this geometry has
        const PatchGeo g = patch_geometry(c.x_dim, c.y_dim, c.window_rows);
        if (!patch_units_exact(g.pw, g.ph)) return false;
    }
    if (sw.rect_meta || sw.rect || sw.fused || sw.step_chunks) return false;
    return !sw.patch || *sw.patch != 0;
}

// Windowed factor columns: the largest length scale a reset may install and the prior covariance dropped at the
// window edge for it (the prior of `kind` at R rows; every kind decays monotonically in the distance).  The RBF prior
// takes the Matern 3/2 rule: its own tail is below 1e-6 at 5 rows (example prior, 4 m cells), but the columns a step
// appends are P H^T L^-1, and for this smoothest kernel L^-1 of a footprint of neighbouring cells is large -- cut at 5
// rows, the 40-step episode_rf1_50_s0 drifts 1.2e-3 from exact columns in the mean, at 7 rows 1.3e-5, at 10 rows 6e-8
// (dense NumPy model of the window), while Matern 1/2 at its own window stays below 3e-6.  Matern 5/2 takes the Matern 3/2 rule
// for the same reason: at its own 8 rows the mean and the variances stay within 3e-6, but the off-diagonal covariances of an
// 8-step walk on 40x40 drift 5.0e-5 from the dense fp64 chain (dropped column tails times entries of order 1; the feature
// planes of the state, bar 1e-5, showed it), at 10 rows 1.3e-6 (same model).
constexpr double kWindowBound = 1e-6;
bool prior_kind_ok(int kind) { return kind >= IPP_PRIOR_MATERN32 && kind <= IPP_PRIOR_RBF; }
const char* prior_kind_name(int kind) {
    switch (kind) {
    case IPP_PRIOR_MATERN12: return "Matern nu=0.5";
    case IPP_PRIOR_MATERN52: return "Matern nu=2.5";
    case IPP_PRIOR_RBF: return "RBF (Matern nu=inf)";
    default: return "Matern nu=1.5";
    }
}
double max_length_scale(const ipp_config& c) { return (c.fixed_prior ? 1.0 : 1.2) * c.length_scale; }
double window_bound(const ipp_config& c, int kind, int rows) {
    if (kind != IPP_PRIOR_MATERN12) {  // Matern 3/2, and 5/2 and RBF by its rule
        const double a = std::sqrt(3.0) * (double)rows * c.resolution / max_length_scale(c);
        return c.signal_variance * (1.0 + a) * std::exp(-a);
    }
    const double u = (double)rows * c.resolution / max_length_scale(c);
    return c.signal_variance * std::exp(-u);  // IPP_PRIOR_MATERN12
}
int min_window_rows(const ipp_config& c, int kind) {
    int r = 1;
    while (r < (1 << 20) && window_bound(c, kind, r) > kWindowBound) ++r;
    return r;
}

int plan(const ipp_config& c, int kind, const Switches& sw, Layout& L, bool allow_patch = true) {
    if (!prior_kind_ok(kind)) return fail(-1, "unknown prior kind %d (IPP_PRIOR_MATERN32 / MATERN12 / MATERN52 / RBF)", kind);
    if (c.x_dim <= 0 || c.y_dim <= 0) return fail(-1, "x_dim/y_dim must be positive");
    if (!(c.resolution > 0)) return fail(-1, "resolution must be positive");
    if (c.state_repr != IPP_DENSE && c.state_repr != IPP_FACTOR) return fail(-1, "state_repr must be IPP_DENSE or IPP_FACTOR");
    if (c.capacity <= 0 || c.max_batch <= 0) return fail(-1, "capacity and max_batch must be positive");
    if (c.state_repr == IPP_FACTOR && c.rank_cap <= 0) return fail(-1, "rank_cap must be positive for IPP_FACTOR");
    if (!(c.signal_variance > 0) || !(c.length_scale > 0)) return fail(-1, "signal_variance and length_scale must be positive");
    if (!(c.max_v > 0) || !(c.max_a > 0)) return fail(-1, "max_v and max_a must be positive");
    L.MC = (c.max_measurements <= 0 || c.max_measurements <= 9) ? 9 : 25;
    if (c.max_measurements > IPP_MAX_MEAS) return fail(-1, "max_measurements above %d is not compiled in", IPP_MAX_MEAS);
    L.FC = 4 * L.MC;
    L.QS = (L.MC + 3) & ~3;
    // cells per thread of the streaming kernels (register budget).  Windowed factor columns are stored and streamed on
    // whole tiles of 64 VEC cells: 128-cell tiles round a step's window up by half as much as 256-cell tiles do, and the
    // step moves 15 % fewer bytes (4096 envs of 50x50: 12.5 -> 13.8 M env-steps/s; every config gained 5-11 %)
    // Only while a window is a few tiles: at 200x200 (20 tiles of 256 cells per step) the rounding is 2.5 % of the bytes and
    // twice as many tiles cost more than that in per-tile work (configs[4] tree wave: 13.4 M steps/s with 256-cell tiles,
    // 12.1 M with 128).
    const bool windowed = c.state_repr == IPP_FACTOR && c.window_rows > 0;
    const long window_cells = std::min<long>(c.y_dim, 2L * c.window_rows + 5) * c.x_dim;
    L.VEC = (L.MC == 9 && !(windowed && window_cells < 16 * 256)) ? 4 : 2;
    L.patch = allow_patch && patch_layout(c, L.MC, sw);
    if (L.patch) {
        L.VEC = 2;
        L.pg = patch_geometry(c.x_dim, c.y_dim, c.window_rows);
    }
    L.N = c.x_dim * c.y_dim;
    const int n4 = (L.N + L.VEC - 1) / L.VEC;
    if (c.tile_threads > 0) {
        if (c.tile_threads % 64 != 0 || c.tile_threads > kMaxTileThreads) return fail(-1, "tile_threads must be a multiple of 64 and <= %d", kMaxTileThreads);
        L.T = c.tile_threads;
    } else {
        // least padding first; among equals 128 threads (2 waves) measured best on MI355X (many small
        // workgroups per CU hide each other's prologue / epilogue), else the largest <= 320
        int best_t = 64;
        long best_pad = -1;
        for (int t = 64; t <= 320; t += 64) {
            const long tiles = (n4 + t - 1) / t, padded = tiles * t;
            const bool better = best_pad < 0 || padded < best_pad ||
                                (padded == best_pad && (t == 128 || (best_t != 128 && t > best_t)));
            if (better) { best_pad = padded; best_t = t; }
        }
        L.T = best_t;
    }
    L.n_tiles = (n4 + L.T - 1) / L.T;
    L.Npad = L.n_tiles * L.T * L.VEC;
    if (c.state_repr == IPP_FACTOR && c.window_rows > 0) {
        // the columns are cut where the prior covariance to the footprint has decayed: refuse windows that are too
        // narrow for this prior (length scale up to 1.2 x nominal under shuffle_prior_cov, mappings.py:238-240)
        const double bound = window_bound(c, kind, c.window_rows);
        if (c.window_rows < std::max(c.x_dim, c.y_dim) && bound > kWindowBound)
            return fail(-1, "window_rows = %d drops prior covariances up to %.1e (> 1e-6) for length scales up to %.3g m at %.3g m cells "
                            "(%s prior): use window_rows >= %d, or 0 for exact columns", c.window_rows, bound, max_length_scale(c),
                        c.resolution, prior_kind_name(kind), min_window_rows(c, kind));
        // windowed factor state: one workgroup per item, wave-granular tiles of 64 * VEC cells (k_gain_factor.h);
        // tile_threads is the workgroup size (waves share the item's Q block and prior table in LDS)
        L.T = (c.tile_threads > 0) ? c.tile_threads : 256;  // 256: fused workgroup kernel (k_step_factor.h), 64: one wave per item (k_gain_wave.h)
        // Large batches of short items on large grids (BASELINE configs[2]: 32768 envs of 100x100, ranks <= 144, ~10 tiles
        // of ~20 rows per item): the per-item latency chain of the fused kernel and its workgroup-granular dispatch leave
        // the stream at 32 % of peak; the prologue as its own kernel + a 128-thread gain kernel streams at 50 % and is 15 %
        // faster per step with the two pipelined over 4 chunks.  Tree steps need the fused layout.
        // With two-dimensional windows the stream of an item is short enough for that to hold at 50x50 too (32768 envs:
        // fused 22.4 M env-steps/s, split 24.7 M, split in 2 chunks 25.6 M; at 4096 envs the fused kernel stays ahead).
        // (Since the rectangle metadata the fused kernel is ahead up to 16384 envs of 50x50 -- 8192: 24.7 vs 23.4 M, 16384:
        // 26.0 vs 23.7 M env-steps/s -- and the split path from 32768: 28.3 vs 26.9 M; on 100x100 the split path stays 23 % ahead.)
        if (c.tile_threads <= 0 && c.node_capacity <= 0 && c.capacity >= ((int64_t)c.x_dim * c.y_dim >= 6000 ? 8192 : 24576)) L.T = 128;
        if (L.patch) L.T = 64 * kPatchWavesDefault;  // one fused kernel for every batch size
        if (L.T > 512) return fail(-1, "tile_threads must be <= 512 for IPP_FACTOR");
        L.n_tiles = (n4 + 63) / 64;
        L.Npad = L.n_tiles * 64 * L.VEC;
    }
    L.win_tiles = L.n_tiles;
    if (c.state_repr == IPP_FACTOR && c.window_rows > 0) {
        // rows a step can touch: the footprint (ny <= m <= MC blocks of rf <= 2 rows) + window_rows on both sides
        const long rows = std::min<long>(c.y_dim, 2L * c.window_rows + 2L * L.MC);
        L.win_tiles = (int)std::min<long>(L.n_tiles, (rows * c.x_dim + 64 * L.VEC - 1) / (64 * L.VEC) + 1);
    }
    L.q_rows = (c.state_repr == IPP_FACTOR) ? c.rank_cap : L.FC;
    L.cov_slot_floats = (c.state_repr == IPP_FACTOR) ? (uint64_t)c.rank_cap * L.Npad : (uint64_t)L.N * L.Npad;
    if (L.patch) L.cov_slot_floats = (uint64_t)c.rank_cap * L.pg.pstride;
    uint64_t o = 0;
    const uint64_t cap = c.capacity, mb = c.max_batch, np = L.Npad;
    L.off_mean = o; o += up(cap * np * 4);
    L.off_diag = o; o += up(cap * np * 4);
    L.off_gt = o; o += up(2 * cap * np * 4);  // two ground-truth planes per env: the current one and the one staged for its next episode
    L.off_gtslot = o; o += up(2 * cap * 4);  // [cap] current plane of every env + [cap] "alternate plane staged" flags
    L.off_prior = o; o += up(cap * 2 * 8);
    L.off_rank = o; o += up(cap * 4);
    L.off_span = o; o += (c.state_repr == IPP_FACTOR) ? up(2 * cap * (uint64_t)c.rank_cap * 4) : 0;  // tile spans, then rectangles
    L.off_cnt = o; o += up((uint64_t)kCountSlots * 128);
    L.off_icnt = o; o += up((uint64_t)c.max_batch * 16);
    L.off_cov = o; o += up(cap * L.cov_slot_floats * 4);
    L.off_hdr = o; o += up(mb * sizeof(ItemHdr));
    L.off_linv = o; o += up(mb * L.MC * L.MC * 4);
    L.off_yv = o; o += up(mb * L.MC * 4);
    L.off_q = o; o += up(mb * q_item_floats(L) * 4 + 4096);  // [L^-1|y] head + Q rows + pad rows, + DMA over-read slack
    L.off_wc = o; o += (c.state_repr == IPP_DENSE) ? up(mb * L.MC * np * 4) : 0;
    L.off_partial = o; o += up(mb * L.n_tiles * 8);
    L.off_dbg = o; o += up(mb * (2 * L.MC * L.MC + 2 * L.MC) * 8);
    L.off_grfh = o; o += up((uint64_t)L.N * 8);
    L.off_grfcs = o; o += up((uint64_t)c.x_dim * 16);                       // (cos, sin)(2 pi j / n)
    L.off_grfg = o; o += up((uint64_t)(c.y_dim / 2 + 1) * c.x_dim * 8);    // g_k[d], k = 0 .. n/2 (k_grf_dft.h)
    {
        const uint64_t npad = 16 * (uint64_t)((std::max(c.x_dim, c.y_dim) + 15) / 16);
        const uint64_t tab = (c.x_dim == c.y_dim && c.x_dim % 2 == 0 && c.x_dim <= 128) ? npad * npad * 8 : 8;
        L.off_grfhp = o; o += up(tab);
        L.off_grfamp = o; o += up(tab);
    }
    {   // un-normalised fields of the convolution path (k_grf_conv + k_grf_norm): even square grids up to 256 run the Hartley /
        // DFT kernels, which normalise in place (2 x 1.3 GB of the configs[2] arena)
        const bool conv = !(c.x_dim == c.y_dim && c.x_dim % 2 == 0 && c.x_dim >= 4 && c.x_dim <= 256);
        L.off_grfraw = o; o += conv ? up(mb * np * 4) : 0;
        L.off_grfraw2 = o; o += conv ? up(mb * np * 4) : 0;
    }
    L.off_sc_hdr = L.off_sc_ext = L.off_sc_mask = L.off_sc_G = L.off_sc_P = o;
    if (c.score_scratch) {  // ipp_score_actions (k_score.h)
        L.off_sc_hdr = o; o += up(mb * sizeof(ScoreHdr));
        L.off_sc_ext = o; o += up(64);
        L.off_sc_mask = o; o += up(np * 4);
        L.off_sc_G = o; o += up((uint64_t)kScoreSplit * L.N * kScoreBandCap * 8);
        L.off_sc_P = o; o += (c.state_repr == IPP_FACTOR) ? up((uint64_t)L.N * np * 4) : 0;
    }
    L.off_tr_cov = L.off_tr_diag = L.off_tr_meta = L.off_sc_ndiag = o;
    if (c.node_capacity > 0) {  // ipp_tree_step (k_tree.h)
        if (c.state_repr != IPP_FACTOR) return fail(-1, "node_capacity needs IPP_FACTOR");
        const uint64_t nc = c.node_capacity, wc = L.patch ? (uint64_t)L.pg.pstride : (uint64_t)L.win_tiles * 64 * L.VEC;  // a node lives on its step's tile span / patch
        L.off_tr_cov = o; o += up(nc * L.MC * wc * 4 + 4096);
        L.off_tr_diag = o; o += up(nc * wc * 4 + 4096);
        L.off_tr_meta = o; o += up(nc * kNodeMeta * 4);
        L.off_sc_ndiag = o; o += c.score_scratch ? up(np * 4) : 0;
        // tree nodes on patches (k_tree_patch.h): a record addresses its column patch by a 32-bit offset in 8-byte units from
        // View::cov - kTreePatchGuard, so root slots AND node blocks have to lie within 2^35 bytes (32 GB) of it -- decided on the finished
        // layout (the score scratch sits between the two regions: 6.5 GB at 200x200, 17 GB at 256x256); beyond that the band-tile
        // tree kernels take over
        if (L.patch && allow_patch) {
            const uint64_t reach = (L.off_tr_diag - L.off_cov) + (uint64_t)kTreePatchGuard + (1ull << 20);  // (+ the largest shift of a patch)
            if (reach >= (1ull << 35)) return plan(c, kind, sw, L, false);
        }
    }
    L.total = o;
    return 0;
}

size_t prep_lds_bytes(const Layout& L, const ipp_config& c) {
    const size_t MC = L.MC, FC = L.FC;
    const size_t small = (L.MC == 9) ? prep_small_bytes<9>() : prep_small_bytes<25>();
    size_t b = (small + 15) & ~(size_t)15;
    if (c.state_repr == IPP_FACTOR)
        b += MC * (size_t)((c.rank_cap + 3) & ~3) * sizeof(float);
    else
        b += FC * (FC + 1) * sizeof(float);
    return (b + 15) & ~(size_t)15;
}

// h = Re ifft2(amp) with the reference's amplitude table (simulations/ground_truths.py:7-29), on the host.
void grf_kernel_host(int H, int W, double c, std::vector<double>& h) {
    auto idx_list = [](int n) {
        std::vector<int> a;
        const int half = n / 2;
        for (int i = 0; i <= half; ++i) a.push_back(i);
        for (int i = half - 1; i >= 1; --i) a.push_back(-i);
        return a;  // one entry short for odd n, like the reference
    };
    const std::vector<int> ky = idx_list(H), kx = idx_list(W);
    std::vector<double> amp((size_t)H * W, 0.0);
    for (size_t i = 0; i < ky.size(); ++i)
        for (size_t j = 0; j < kx.size(); ++j) {
            if (ky[i] == 0 && kx[j] == 0) continue;
            const double k = std::sqrt((double)ky[i] * ky[i] + (double)kx[j] * kx[j]);
            amp[i * W + j] = std::sqrt(std::pow(k, -c));
        }
    // separable inverse DFT, real part only (amp is real; imaginary parts cancel for even amp)
    std::vector<double> are((size_t)H * W), aim((size_t)H * W);
    for (int u = 0; u < H; ++u)
        for (int x = 0; x < W; ++x) {
            double re = 0, im = 0;
            for (int q = 0; q < W; ++q) {
                const double ang = 2.0 * M_PI * (double)((long)q * x % W) / W;
                re += amp[(size_t)u * W + q] * std::cos(ang);
                im += amp[(size_t)u * W + q] * std::sin(ang);
            }
            are[(size_t)u * W + x] = re;
            aim[(size_t)u * W + x] = im;
        }
    h.assign((size_t)H * W, 0.0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            double re = 0;
            for (int u = 0; u < H; ++u) {
                const double ang = 2.0 * M_PI * (double)((long)u * y % H) / H;
                re += are[(size_t)u * W + x] * std::cos(ang) - aim[(size_t)u * W + x] * std::sin(ang);
            }
            h[(size_t)y * W + x] = re / ((double)H * W);
        }
}

// Kernel launch; with profiling on (bench.py's roofline leg) the start / stop events are attached to the dispatch
// itself (hipExtLaunchKernelGGL), so their difference is the kernel's own duration as rocprofv3 reports it, not the
// interval between two event packets around it (which adds the dispatch latency, 20-25 us on this pool).
template <typename... P, typename... A>
void timed_launch(Engine* e, int kind, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    if (!e->profile) {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
        return;
    }
    hipEvent_t a = nullptr, b = nullptr;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, a, b, 0, static_cast<P>(args)...);
    e->prof_pending.push_back({a, b, kind});
}

void prof_drain(Engine* e) {
    // per kind: sum of the dispatches' durations + the union of their [start, stop] intervals (launches of different streams
    // overlap); slot 3: the union over EVERY launch (a two-kernel step is a prologue launch and a gain launch: both are the step)
    auto& pend = e->prof_pending;
    if (pend.empty()) return;
    std::vector<std::pair<float, float>> iv[kProfKinds];  // ms behind the first start of this batch
    for (auto& pr : pend) (void)hipEventSynchronize(pr.b);
    for (auto& pr : pend) {
        float ms = 0.f, t0 = 0.f;
        if (hipEventElapsedTime(&ms, pr.a, pr.b) == hipSuccess) {
            e->prof[pr.kind].total_ms += ms;
            e->prof[pr.kind].launches += 1;
            if (hipEventElapsedTime(&t0, pend.front().a, pr.a) == hipSuccess) { iv[pr.kind].emplace_back(t0, t0 + ms); iv[3].emplace_back(t0, t0 + ms); }
        }
    }
    if (const char* dump = getenv("IPP_PROFILE_DUMP")) {  // tools/region_timeline.py: every dispatch's [start, stop] of this batch
        if (FILE* f = fopen(dump, "a")) {
            fprintf(f, "# batch of %zu dispatches: kind start_us stop_us\n", pend.size());
            for (int k = 0; k < 3; ++k)
                for (auto& x : iv[k]) fprintf(f, "%d %.2f %.2f\n", k, 1e3 * x.first, 1e3 * x.second);
            fclose(f);
        }
    }
    for (auto& pr : pend) {
        (void)hipEventDestroy(pr.a);
        (void)hipEventDestroy(pr.b);
    }
    pend.clear();
    for (int k = 0; k < kProfKinds; ++k) {
        std::sort(iv[k].begin(), iv[k].end());
        float end = -1e30f;
        ProfSlot& p = e->prof[k];
        for (auto& x : iv[k]) {
            if (x.first > end) { p.busy_ms += x.second - x.first; end = x.second; }
            else if (x.second > end) { p.busy_ms += x.second - end; end = x.second; }
        }
        p.busy_launches += (int64_t)iv[k].size();
    }
}

size_t gain_lds_bytes(const View& v, int q_chunk, int lut_cap) {
    const size_t MC = v.meas_cap, QS = v.q_stride;
    size_t b = std::max((size_t)(q_chunk + 2 * kPipe) * QS, (size_t)((lut_cap + 3) & ~3)) * 4 + ((MC * MC + 3) & ~(size_t)3) * 4 + ((MC + 3) & ~(size_t)3) * 4 + 16 * 8;
    b += (size_t)std::max(q_chunk, v.q_rows) * 4;  // rowidx: streaming index -> row of the covariance slab
    return (b + 15) & ~(size_t)15;
}

// The instantiations of k_step_patch -- X(NW, KPN, MINW, RJN), each in its plain and its IPP_BUDGET form -- and of k_tree_patch --
// X(NW, RJN): the launches and the LDS opt-in of engine creation both go through these lists.
#define IPP_STEP_PATCH_KERNELS(X)      \
    X(2, kPatchKP, kPatchMinW, 0)      \
    X(3, kPatchKP, kPatchMinW, 0)      \
    X(3, kPatchKP, kPatchMinW, 1)      \
    X(3, kPatchKP, kPatchMinW, 2)      \
    X(2, IPP_PATCH_BIGKP, 6, 0)
#define IPP_TREE_PATCH_KERNELS(X) X(3, 0) X(3, 1)

using StepPatchKernel = decltype(&k_step_patch<3>);
using TreePatchKernel = decltype(&k_tree_patch<3>);
template <bool BUD>
StepPatchKernel patch_kernel(const PatchVariant& pv) {  // nullptr: not instantiated
#define X(NW, KPN, MINW, RJN) \
    if (pv.waves == NW && pv.kpn == KPN && pv.minw == MINW && pv.rjn == RJN) return k_step_patch<NW, KPN, MINW, RJN, BUD>;
    IPP_STEP_PATCH_KERNELS(X)
#undef X
    return nullptr;
}
TreePatchKernel tree_patch_kernel(const PatchVariant& pv) {
#define X(NW, RJN) if (pv.waves == NW && pv.rjn == RJN) return k_tree_patch<NW, RJN>;
    IPP_TREE_PATCH_KERNELS(X)
#undef X
    return nullptr;
}

// One chunk of items: prologue -> streaming gain (-> reward finalize) (-> dense downdate) on stream `s`.
// `v` carries scratch pointers already offset to the chunk's first item.
template <int MC, int VEC>
void launch_chunk(Engine* e, const View& v, const int32_t* env_ids, const int32_t* dst_ids, int n, const double* action,
                  const double* prev, const float* noise, unsigned flags, float* reward, int32_t* status, hipStream_t s,
                  hipEvent_t prep_done, const AutoReset& ar) {
    if (e->patch) {  // compact column patches: one fused kernel, one small workgroup per item (k_step_patch.h)
        if constexpr (MC == 9 && VEC == 2) {
            // (the budget ledger: the IPP_BUDGET instantiation of the kernel the launch would run otherwise)
            const PatchVariant& pv = pick(e->pp, n);
            View vp = v;
            vp.pcap = pv.pcap;
            timed_launch(e, 0, (flags & IPP_BUDGET) ? patch_kernel<true>(pv) : patch_kernel<false>(pv), dim3(n), dim3(64 * pv.waves), pv.lds, s, vp,
                         env_ids, n, action, prev, noise, flags, status, reward, ar);
        }
        if (prep_done) (void)hipEventRecord(prep_done, s);
        return;
    }
    if constexpr (MC == 9) {  // (MC = 25: the fused kernel would spill 431 VGPRs -- those engines run the prologue and the gain kernel as two launches)
    if (e->fused) {  // windowed factor state: prologue + gain in one kernel, one workgroup per item
        if (VEC == 2 && e->rect_ok && (e->rect_commit || (flags & IPP_PREDICT_ONLY)))
            timed_launch(e, 0, k_step_factor<MC, VEC, (MC == 9 && VEC == 2)>, dim3(n), dim3(kStepThreads), e->gain_lds, s, v, env_ids, n, action, prev, noise,
                     flags, e->lut_rows, status, reward, ar);
        else
            timed_launch(e, 0, k_step_factor<MC, VEC>, dim3(n), dim3(kStepThreads), e->gain_lds, s, v, env_ids, n, action, prev, noise,
                     flags, e->lut_rows, status, reward, ar);
        if (prep_done) (void)hipEventRecord(prep_done, s);
        return;
    }
    }
    if (v.mode == IPP_FACTOR)
        timed_launch(e, 2, k_prepare<MC, IPP_FACTOR>, dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, dst_ids, n, action, prev,
                     noise, flags, status, (float*)nullptr, (int*)nullptr, (int*)nullptr);
    else
        timed_launch(e, 2, k_prepare<MC, IPP_DENSE>, dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, dst_ids, n, action, prev,
                     noise, flags, status, (float*)nullptr, (int*)nullptr, (int*)nullptr);
    if (prep_done) (void)hipEventRecord(prep_done, s);
    {
        const int grid = grid_for(n, v.n_tiles);
        if (v.mode == IPP_FACTOR && v.window_rows > 0 && v.T == kWave)
            timed_launch(e, 0, k_gain_wave<MC, VEC>, dim3(n), dim3(kWave), e->gain_lds, s, v, v.q, n, flags, reward);
        else if (v.mode == IPP_FACTOR && v.window_rows > 0)
            if (MC == 9 && VEC == 2 && e->rect_ok && (e->rect_commit || (flags & IPP_PREDICT_ONLY)))
                timed_launch(e, 0, k_gain_factor<MC, VEC, (MC == 9 && VEC == 2)>, dim3(n), dim3(v.T), e->gain_lds, s, v, v.q, n, flags, e->lut_rows, reward);
            else
                timed_launch(e, 0, k_gain_factor<MC, VEC>, dim3(n), dim3(v.T), e->gain_lds, s, v, v.q, n, flags, e->lut_rows, reward);
        else if (v.mode == IPP_FACTOR)
            timed_launch(e, 0, k_gain<MC, VEC, IPP_FACTOR>, dim3(grid), dim3(v.T), e->gain_lds, s, v, n, flags, e->q_chunk, e->lut_cap, reward);
        else
            timed_launch(e, 0, k_gain<MC, VEC, IPP_DENSE>, dim3(grid), dim3(v.T), e->gain_lds, s, v, n, flags, e->q_chunk, e->lut_cap, reward);
    }
    if (v.n_tiles > 1 && !(v.mode == IPP_FACTOR && v.window_rows > 0)) hipLaunchKernelGGL(k_reward_finalize, dim3((n + 255) / 256), dim3(256), 0, s, v, n, reward);
    if (v.mode == IPP_DENSE && !(flags & IPP_PREDICT_ONLY)) {
        const int grid = grid_for(n, e->n_bands * v.n_tiles);
        timed_launch(e, 1, k_downdate<MC, VEC>, dim3(grid), dim3(v.T), 0, s, v, n, e->n_bands);
    }
}

// The prologue is latency-bound (dependent loads, a 9x9 fp64 factorisation per item) and the gain kernel is
// HBM-bound, so a large batch is cut into chunks that alternate between the caller's stream and an engine-owned
// side stream: chunk c's prologue waits for chunk c-1's prologue and therefore runs under chunk c-1's gain
// kernel.  Chunks touch disjoint items and (for committed steps) disjoint env slots.
template <int MC, int VEC>
int launch_step(Engine* e, const int32_t* env_ids, const int32_t* dst_ids, int n, const double* action,
                const double* prev, const float* noise, unsigned flags, float* reward, int32_t* status, hipStream_t s,
                const AutoReset& ar) {
    int chunks = e->step_chunks;
    // measured on MI355X: at 4096 items of 50x50 no gain from 2 chunks, slower from 4; at 32768 items of 100x100 on the
    // split path 4 chunks hide most of the prologue kernel under the previous chunk's gain kernel
    if (chunks <= 0) chunks = (!e->fused && e->v.mode == IPP_FACTOR && e->v.window_rows > 0 && e->v.T == 128 && n >= 16384) ? (e->v.N >= 6000 ? 4 : 2) : 1;
    if (e->profile) chunks = 1;  // kernels are timed alone (bench.py roofline leg)
    chunks = std::min(chunks, kMaxChunks);
    if (chunks <= 1 || !e->side) {
        launch_chunk<MC, VEC>(e, e->v, env_ids, dst_ids, n, action, prev, noise, flags, reward, status, s, nullptr, ar);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    HIP_TRY(hipEventRecord(e->ev_begin, s));
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_begin, 0));
    const int per = ((n + chunks - 1) / chunks + 7) / 8 * 8;
    const bool ordered = e->v.item_order && e->v.item_order_n == n && e->v.mode == IPP_FACTOR && e->v.window_rows > 0 && e->v.T != kWave;  // (k_gain_wave keeps its own item map)
    for (int c = 0, off = 0; off < n; ++c, off += per) {
        const int nc = std::min(per, n - off);
        hipStream_t st = (c % 2 == 0) ? s : e->side;
        View v = e->v;
        if (c > 0) HIP_TRY(hipStreamWaitEvent(st, e->ev_prep[c - 1], 0));
        if (ordered) {
            // a dispatch order is set for this launch size: chunk c takes positions [off, off + nc) of it -- any items, so the
            // per-item arrays keep their global indexing (heaviest chunk first, the last chunk ends the step on the lightest)
            v.item_order = e->v.item_order + off;
            v.item_order_n = nc;
            launch_chunk<MC, VEC>(e, v, env_ids, dst_ids, nc, action, prev, noise, flags, reward, status, st, e->ev_prep[c], ar);
            continue;
        }
        v.item_order = nullptr;
        v.env_base = off;
        v.hdr += off;
        v.linv += (size_t)off * v.meas_cap * v.meas_cap;
        v.yv += (size_t)off * v.meas_cap;
        v.q += (size_t)off * v.q_item;
        if (v.wc) v.wc += (size_t)off * v.meas_cap * v.Npad;
        v.partial += (size_t)off * v.n_tiles;
        v.dbg += (size_t)off * (2 * v.meas_cap * v.meas_cap + 2 * v.meas_cap);
        AutoReset arc = ar;
        if (arc.src) arc.src += off;
        launch_chunk<MC, VEC>(e, v, env_ids ? env_ids + off : nullptr, dst_ids ? dst_ids + off : nullptr, nc,
                              action + 3 * (size_t)off, prev + 3 * (size_t)off, noise ? noise + (size_t)off * MC : nullptr,
                              flags, reward + off, status ? status + off : nullptr, st, e->ev_prep[c], arc);
    }
    HIP_TRY(hipEventRecord(e->ev_end, e->side));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_end, 0));
    HIP_TRY(hipGetLastError());
    return 0;
}

// white [n][N] -> normalised field, either into the env slots (gt_out == nullptr) or into gt_out [n][N]
// Tables of k_grf_dft.h: cs[j] = (cos, sin)(2 pi j / n); g[k][d] = c_k / n * sum_l amp[k][l] cos(2 pi l d / n).
void grf_dft_tables_host(int n, double c, std::vector<double>& cs, std::vector<double>& g) {
    std::vector<int> kidx;
    for (int i = 0; i <= n / 2; ++i) kidx.push_back(i);
    for (int i = n / 2 - 1; i >= 1; --i) kidx.push_back(-i);  // ground_truths.py:7-11 (n entries for even n)
    cs.resize((size_t)2 * n);
    for (int j = 0; j < n; ++j) {
        cs[2 * j] = std::cos(2.0 * M_PI * j / n);
        cs[2 * j + 1] = std::sin(2.0 * M_PI * j / n);
    }
    const int n_k = n / 2 + 1;
    g.assign((size_t)n_k * n, 0.0);
    std::vector<double> amp(n);
    for (int k = 0; k < n_k; ++k) {
        for (int l = 0; l < n; ++l) {
            const double kk = std::sqrt((double)kidx[k] * kidx[k] + (double)kidx[l] * kidx[l]);
            amp[l] = (kidx[k] == 0 && kidx[l] == 0) ? 0.0 : std::sqrt(std::pow(kk, -c));
        }
        const double ck = (k == 0 || k == n / 2) ? 1.0 : 2.0;
        for (int d = 0; d < n; ++d) {
            double acc = 0.0;
            for (int l = 0; l < n; ++l) acc += amp[l] * cs[2 * (int)((long)l * d % n)];
            g[(size_t)k * n + d] = ck * acc / n;
        }
    }
}

// Tables of k_grf_hartley.h, zero padded to np x np: H[j][k] = cos + sin of 2 pi j k / n; amp as ground_truths.py:20-27.
// Returns false when the amplitude is not even in each index (then the Hartley form does not apply).
bool grf_hartley_tables_host(int n, int np, double c, std::vector<double>& hp, std::vector<double>& amp) {
    std::vector<int> kidx;
    for (int i = 0; i <= n / 2; ++i) kidx.push_back(i);
    for (int i = n / 2 - 1; i >= 1; --i) kidx.push_back(-i);  // ground_truths.py:7-11 (n entries for even n)
    hp.assign((size_t)np * np, 0.0);
    amp.assign((size_t)np * np, 0.0);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) {
            const double a = 2.0 * M_PI * (double)(((long)j * k) % n) / n;
            hp[(size_t)j * np + k] = std::cos(a) + std::sin(a);
            const double kk = std::sqrt((double)kidx[j] * kidx[j] + (double)kidx[k] * kidx[k]);
            amp[(size_t)j * np + k] = (kidx[j] == 0 && kidx[k] == 0) ? 0.0 : std::sqrt(std::pow(kk, -c));
        }
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) {
            const int jm = (n - j) % n, km = (n - k) % n;
            if (amp[(size_t)j * np + k] != amp[(size_t)jm * np + k] || amp[(size_t)j * np + k] != amp[(size_t)j * np + km]) return false;
        }
    return true;
}

// 8 waves (one owned 16-row tile each) from TT = 5: half the registers per wave of the 4-wave form, so that waves of the
// streaming kernels still fit beside a field's workgroup on every SIMD
template <int TT>
void launch_grf_hartley(const View& v, int n, const float* white, const int32_t* env_ids, float* gt_out, hipStream_t s, const GrfNoise& gn) {
    constexpr int NW = (TT > 4 && TT < 8) ? 8 : 4;  // (TT = 8 with one tile per wave spills 112 registers at the 168 it may use)
    // the grid sizes of BASELINE.json contract over ceil(n / 4) steps instead of the padded 4 TT (k_grf_hartley.h, KS)
    if (TT == 4 && v.W == 50)
        hipLaunchKernelGGL((k_grf_hartley<4, 4, 13>), dim3(n), dim3(256), grf_hartley_lds_bytes(4), s, v, env_ids, n, white,
                           (const double*)v.grf_hp, (const double*)v.grf_amp, gt_out, gn);
    else if (TT == 7 && v.W == 100)
        hipLaunchKernelGGL((k_grf_hartley<7, 8, 25>), dim3(n), dim3(512), grf_hartley_lds_bytes(7), s, v, env_ids, n, white,
                           (const double*)v.grf_hp, (const double*)v.grf_amp, gt_out, gn);
    else
        hipLaunchKernelGGL((k_grf_hartley<TT, NW>), dim3(n), dim3(64 * NW), grf_hartley_lds_bytes(TT), s, v, env_ids, n, white,
                           (const double*)v.grf_hp, (const double*)v.grf_amp, gt_out, gn);
}

// the engine's generator draws a field's white noise itself (GrfNoise): k_grf_fft always, the GEMM-Hartley and DFT families once
// ipp_set_grf_rows has switched them on (grf_dft: every even square grid of 4 .. 256 cells a side)
bool grf_draws_noise(const Engine* e) { return (e->grf_tt > 0 && e->grf_fft) || (e->grf_rows_all && e->grf_dft); }

int launch_grf(Engine* e, int n, const float* white, float* raw, const int32_t* env_ids, float* gt_out, hipStream_t s,
               const GrfNoise* noise = nullptr) {
    const View& v = e->v;
    if (!white && !(noise && grf_draws_noise(e)))
        return fail(-1, "in-kernel ground-truth noise needs the fast Hartley path (50x50 / 100x100 grids), or ipp_set_grf_rows(engine, 1) on an even square grid of 4 .. 256 cells a side");
    const GrfNoise gn = noise ? *noise : GrfNoise{nullptr, 0, 0, 0, 0, {0}, 0};
    if (v.W != v.H) return fail(-1, "device GRF needs a square grid (the reference transposes its dims, simulations/simulations.py:45-47)");
    if (e->grf_tt > 0 && e->grf_fft) {  // n = 50 / 100: fast Hartley transforms in LDS (k_grf_fft.h), same amplitude table
        const int np = 16 * e->grf_tt;
        const double* ampt = (const double*)v.grf_amp;
        const double2* twt = (const double2*)v.grf_cs;
        if (gn.episode) {  // ipp_generate_grf_refill
            if (v.W == 100) hipLaunchKernelGGL((k_grf_fft<10, float, true>), dim3(n), dim3(512), grf_fft_lds_bytes(100, 4), s, v, env_ids, n, white, ampt, np, gt_out, gn, twt);
            else hipLaunchKernelGGL((k_grf_fft<5, float, true>), dim3(n), dim3(256), grf_fft_lds_bytes(50, 4), s, v, env_ids, n, white, ampt, np, gt_out, gn, twt);
        } else if (v.W == 100) hipLaunchKernelGGL((k_grf_fft<10, float>), dim3(n), dim3(512), grf_fft_lds_bytes(100, 4), s, v, env_ids, n, white, ampt, np, gt_out, gn, twt);
        else hipLaunchKernelGGL((k_grf_fft<5, float>), dim3(n), dim3(256), grf_fft_lds_bytes(50, 4), s, v, env_ids, n, white, ampt, np, gt_out, gn, twt);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (e->grf_tt > 0) {  // even n <= 128: four fp64 GEMMs on the matrix cores, normalisation fused (k_grf_hartley.h)
        switch (e->grf_tt) {
            case 1: launch_grf_hartley<1>(v, n, white, env_ids, gt_out, s, gn); break;
            case 2: launch_grf_hartley<2>(v, n, white, env_ids, gt_out, s, gn); break;
            case 3: launch_grf_hartley<3>(v, n, white, env_ids, gt_out, s, gn); break;
            case 4: launch_grf_hartley<4>(v, n, white, env_ids, gt_out, s, gn); break;
            case 5: launch_grf_hartley<5>(v, n, white, env_ids, gt_out, s, gn); break;
            case 6: launch_grf_hartley<6>(v, n, white, env_ids, gt_out, s, gn); break;
            case 7: launch_grf_hartley<7>(v, n, white, env_ids, gt_out, s, gn); break;
            default: launch_grf_hartley<8>(v, n, white, env_ids, gt_out, s, gn); break;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (e->grf_dft) {  // even n <= 256: half-spectrum DFT, normalisation fused (k_grf_dft.h)
        const bool small = v.W <= 100;
        const int nt = small ? 256 : 1024;
        const int xb = (v.W % 4 == 0) ? 4 : 2;                 // columns per thread in the row-inverse stage
        const int rgroups = std::max(1, nt / (v.W / xb));      // row groups
        const int rows = (v.W + rgroups - 1) / rgroups;        // rows per thread
        const size_t lds = grf_dft_lds_bytes(v.W, e->grf_kc, small);
#define IPP_GRF_LAUNCH(OPT, XB, NT, WLDS) \
    hipLaunchKernelGGL((k_grf_dft<OPT, XB, NT, WLDS>), dim3(n), dim3(NT), lds, s, v, env_ids, n, white, v.grf_cs, v.grf_g, e->grf_kc, gt_out, gn)
        if (small && xb == 4) IPP_GRF_LAUNCH(10, 4, 256, true);        // rows <= 10 for every n <= 100
        else if (small && rows <= 10) IPP_GRF_LAUNCH(10, 2, 256, true);
        else if (small) IPP_GRF_LAUNCH(20, 2, 256, true);              // n = 54 .. 98, n = 2 mod 4
        else if (xb == 4 && rows <= 10) IPP_GRF_LAUNCH(10, 4, 1024, false);   // n <= 200
        else if (xb == 4) IPP_GRF_LAUNCH(16, 4, 1024, false);                 // n <= 256
        else if (rows <= 20) IPP_GRF_LAUNCH(20, 2, 1024, false);              // n <= 202
        else IPP_GRF_LAUNCH(32, 2, 1024, false);                              // n <= 256
#undef IPP_GRF_LAUNCH
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const size_t lds = (size_t)v.N * (sizeof(double) + sizeof(float));
    const bool use_lds = lds <= 120 * 1024;
    const int ot = (v.W <= 64) ? 5 : 8;
    const int tpr = (v.W + ot - 1) / ot;
    const int groups = v.H * tpr;
    if (use_lds) {  // one workgroup per env, tables in LDS
        if (ot == 5) hipLaunchKernelGGL((k_grf_conv<5, true>), dim3(1, n), dim3(256), lds, s, v, n, white, tpr, raw);
        else         hipLaunchKernelGGL((k_grf_conv<8, true>), dim3(1, n), dim3(256), lds, s, v, n, white, tpr, raw);
    } else {
        if (ot == 5) hipLaunchKernelGGL((k_grf_conv<5, false>), dim3((groups + 255) / 256, n), dim3(256), 0, s, v, n, white, tpr, raw);
        else         hipLaunchKernelGGL((k_grf_conv<8, false>), dim3((groups + 255) / 256, n), dim3(256), 0, s, v, n, white, tpr, raw);
    }
    hipLaunchKernelGGL(k_grf_norm, dim3(n), dim3(256), 0, s, v, env_ids, n, raw, gt_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

Engine* as_engine(void* p) { return reinterpret_cast<Engine*>(p); }

int check_env(Engine* e, int env) {
    if (env < 0 || env >= e->v.cap) return fail(-1, "env_id %d outside [0, %d)", env, e->v.cap);
    return 0;
}

}  // namespace

extern "C" {

int ipp_abi_version(void) { return IPP_ABI_VERSION; }
const char* ipp_last_error(void) { return g_err.c_str(); }

int ipp_min_window_rows_prior(const ipp_config* cfg, int32_t kind, int32_t* rows) {
    if (!cfg || !rows) return fail(-1, "null argument");
    if (!prior_kind_ok(kind)) return fail(-1, "unknown prior kind %d (IPP_PRIOR_MATERN32 / MATERN12 / MATERN52 / RBF)", kind);
    if (!(cfg->resolution > 0) || !(cfg->length_scale > 0) || !(cfg->signal_variance > 0)) return fail(-1, "resolution, length_scale and signal_variance must be positive");
    *rows = min_window_rows(*cfg, kind);
    return 0;
}
int ipp_min_window_rows(const ipp_config* cfg, int32_t* rows) { return ipp_min_window_rows_prior(cfg, IPP_PRIOR_MATERN32, rows); }

int ipp_engine_arena_bytes_prior(const ipp_config* cfg, int32_t kind, uint64_t* bytes) {
    if (!cfg || !bytes) return fail(-1, "null argument");
    Layout L;
    if (int rc = plan(*cfg, kind, Switches(), L)) return rc;  // (the switches ipp_engine_create_prior will read: the two agree)
    *bytes = L.total;
    return 0;
}
int ipp_engine_arena_bytes(const ipp_config* cfg, uint64_t* bytes) { return ipp_engine_arena_bytes_prior(cfg, IPP_PRIOR_MATERN32, bytes); }

int ipp_engine_create(const ipp_config* cfg, int device, void* arena, uint64_t arena_bytes, void** engine) {
    return ipp_engine_create_prior(cfg, IPP_PRIOR_MATERN32, device, arena, arena_bytes, engine);
}
int ipp_engine_create_prior(const ipp_config* cfg, int32_t kind, int device, void* arena, uint64_t arena_bytes, void** engine) {
    if (!cfg || !arena || !engine) return fail(-1, "null argument");
    const Switches sw;  // (parsed here, once: plan() and everything below see the same values)
    Layout L;
    if (int rc = plan(*cfg, kind, sw, L)) return rc;
    if (arena_bytes < L.total) return fail(-1, "arena too small: %llu < %llu", (unsigned long long)arena_bytes, (unsigned long long)L.total);
    if ((reinterpret_cast<uintptr_t>(arena) & (kAlign - 1)) != 0) return fail(-1, "arena must be %llu-byte aligned", (unsigned long long)kAlign);
    HIP_TRY(hipSetDevice(device));
    Engine* e = new (std::nothrow) Engine();
    if (!e) return fail(-3, "out of host memory");
    e->cfg = *cfg;
    e->device = device;
    e->used_bytes = L.total;
    View& v = e->v;
    v.W = cfg->x_dim; v.H = cfg->y_dim; v.N = L.N; v.Npad = L.Npad; v.T = L.T; v.n_tiles = L.n_tiles; v.vec = L.VEC; v.env_base = 0;
    v.mode = cfg->state_repr; v.cap = cfg->capacity; v.rank_cap = cfg->rank_cap; v.max_batch = cfg->max_batch;
    v.meas_cap = L.MC; v.fp_cap = L.FC; v.q_stride = L.QS; v.q_rows = L.q_rows; v.q_item = q_item_floats(L);
    v.res = cfg->resolution; v.tanx = cfg->tan_half_fov_x; v.tany = cfg->tan_half_fov_y; v.rf_alt = cfg->rf_altitude;
    v.coeff_a = cfg->coeff_a; v.coeff_b = cfg->coeff_b; v.sv0 = cfg->signal_variance; v.ls0 = cfg->length_scale;
    v.ls_max = (cfg->state_repr == IPP_FACTOR && cfg->window_rows > 0 && cfg->window_rows < std::max(cfg->x_dim, cfg->y_dim)) ? max_length_scale(*cfg) : 0.0;
    v.vmax = cfg->max_v; v.amax = cfg->max_a; v.thr = cfg->value_threshold; v.kf = cfg->interval_factor;
    v.prior_kind = kind;
    char* base = reinterpret_cast<char*>(arena);
    v.mean = reinterpret_cast<float*>(base + L.off_mean);
    v.diag = reinterpret_cast<float*>(base + L.off_diag);
    v.gt = reinterpret_cast<float*>(base + L.off_gt);
    v.gt_slot = reinterpret_cast<int*>(base + L.off_gtslot);
    v.prior = reinterpret_cast<double*>(base + L.off_prior);
    v.rank = reinterpret_cast<int*>(base + L.off_rank);
    v.colspan = reinterpret_cast<int*>(base + L.off_span);
    v.colrect = v.colspan + (size_t)cfg->capacity * cfg->rank_cap;
    v.dbg_capture = 0;
    v.counters = reinterpret_cast<unsigned long long*>(base + L.off_cnt);
    v.item_counts = reinterpret_cast<unsigned long long*>(base + L.off_icnt);
    v.window_rows = (cfg->state_repr == IPP_FACTOR) ? std::max(0, cfg->window_rows) : 0;
    v.tile_cells = (cfg->state_repr == IPP_FACTOR && cfg->window_rows > 0) ? 64 * L.VEC : L.T * L.VEC;
    v.tile_shift = -1;
    for (int sh = 0; sh < 20; ++sh) if ((1 << sh) == v.tile_cells) v.tile_shift = sh;
    // two-dimensional windows (k_gain_factor.h): every kernel that appends columns of a windowed state clips them (the
    // one-wave-per-item kernel of tile_threads = 64 and the pipelined kernel do not: off for those engines)
    v.clip_cols = (cfg->state_repr == IPP_FACTOR && cfg->window_rows > 0 && L.T != 64 && cfg->x_dim > 2 * cfg->window_rows + 13) ? 1 : 0;
    // rectangle tiles for committed steps where a rectangle (<= 2 R + 5 + 2 cells of alignment wide) is at most 0.4 grid rows
    // (the rectangle-tile kernels carry no sqrt / exp form of the prior term: the table P0(|drow|, |dcol|) must be complete,
    // i.e. not cut at 48 KiB -- same arithmetic as for lut_rows below)
    const int lut_tile_rows = (v.tile_cells + cfg->x_dim - 1) / cfg->x_dim + 1;
    const bool lut_complete = (size_t)std::min(cfg->y_dim, std::max(0, cfg->window_rows) + lut_tile_rows + 6) * cfg->x_dim <= 12288;
    e->rect_ok = v.clip_cols && L.MC == 9 && L.VEC == 2 && cfg->x_dim % 2 == 0 && lut_complete;
    e->rect_commit = e->rect_ok && 5 * (2 * cfg->window_rows + 7) <= 2 * cfg->x_dim;
    e->rect_tree = v.clip_cols && L.MC == 9 && cfg->x_dim % L.VEC == 0 && lut_complete && 5 * (2 * cfg->window_rows + 5 + 2 * (L.VEC - 1)) <= 2 * cfg->x_dim;
    if (sw.rect_tree) e->rect_tree = v.clip_cols && L.MC == 9 && cfg->x_dim % L.VEC == 0 && lut_complete && *sw.rect_tree != 0;  // A/B experiments
    if (sw.rect) { e->rect_commit = e->rect_ok && *sw.rect == 2; e->rect_ok = e->rect_ok && *sw.rect != 0; }  // A/B: 0 off, 1 predict-only, 2 always
    // Rectangle metadata (View::rect_meta, ipp_common.h): steps on rectangle tiles store the new columns on the rectangle
    // only and record it per column; every reader of stored columns masks with it.  Without it the band cells outside the
    // rectangle received zeros from a store-only pass: 75 % of the gain kernel's HBM writes at 100x100, more at 200x200.
    v.rect_meta = (v.clip_cols && L.MC == 9 && cfg->x_dim % L.VEC == 0 && cfg->x_dim <= 256 && cfg->y_dim <= 256 && (e->rect_ok || e->rect_tree)) ? 1 : 0;
    if (sw.rect_meta) v.rect_meta = v.rect_meta && *sw.rect_meta != 0;  // A/B experiments
    // Only the rectangle-tile variants of the streaming kernels mask (k_gain_factor.h), so with the metadata on every
    // stream over columns that may carry a true rectangle runs on rectangle tiles: env steps where they exist (VEC = 2;
    // else the env columns are written on band tiles and carry full rectangles), tree steps always.
    if (v.rect_meta) { e->rect_commit = e->rect_ok; e->rect_tree = true; }
    v.patch = L.patch ? 1 : 0;
    v.pw = v.ph = v.pstride = v.plw = v.pcap = v.punits = 0;
    v.pos0 = 0;
    e->patch = L.patch;
    if (L.patch) {
        v.clip_cols = 1;
        v.rect_meta = 1;
        v.pw = L.pg.pw; v.ph = L.pg.ph; v.pstride = L.pg.pstride; v.plw = L.pg.plw; v.punits = L.pg.punits;
        e->pp = make_patch_plan(v, sw);
        v.pcap = e->pp.tier[0].pcap;
        // every variant of the plan is an instantiated kernel, in its plain and its IPP_BUDGET form
        bool have = tree_patch_kernel(e->pp.tree) != nullptr;
        for (int i = 0; i < e->pp.n_tiers; ++i) have = have && patch_kernel<false>(e->pp.tier[i]) && patch_kernel<true>(e->pp.tier[i]);
        if (!have) { delete e; return fail(-3, "the patch launch plan names a kernel that is not instantiated"); }
    }
    v.win_tiles = L.win_tiles;
    v.cov = reinterpret_cast<float*>(base + L.off_cov);
    v.cov_slot = L.cov_slot_floats;
    v.hdr = reinterpret_cast<ItemHdr*>(base + L.off_hdr);
    v.linv = reinterpret_cast<float*>(base + L.off_linv);
    v.yv = reinterpret_cast<float*>(base + L.off_yv);
    v.q = reinterpret_cast<float*>(base + L.off_q);
    v.wc = reinterpret_cast<float*>(base + L.off_wc);
    v.partial = reinterpret_cast<double*>(base + L.off_partial);
    v.dbg = reinterpret_cast<double*>(base + L.off_dbg);
    v.grf_h = reinterpret_cast<double*>(base + L.off_grfh);
    v.grf_cs = reinterpret_cast<double2*>(base + L.off_grfcs);
    v.grf_g = reinterpret_cast<double*>(base + L.off_grfg);
    v.grf_hp = reinterpret_cast<double*>(base + L.off_grfhp);
    v.grf_amp = reinterpret_cast<double*>(base + L.off_grfamp);
    v.grf_raw = reinterpret_cast<float*>(base + L.off_grfraw);
    v.grf_raw2 = reinterpret_cast<float*>(base + L.off_grfraw2);
    e->tv.node_cap = std::max(0, cfg->node_capacity);
    if (e->tv.node_cap > 0) {
        e->tv.node_cov = reinterpret_cast<float*>(base + L.off_tr_cov);
        e->tv.node_diag = reinterpret_cast<float*>(base + L.off_tr_diag);
        e->tv.node_meta = reinterpret_cast<int*>(base + L.off_tr_meta);
        e->tv.win_cells = L.patch ? L.pg.pstride : L.win_tiles * 64 * L.VEC;
        e->node_diag_scratch = cfg->score_scratch ? reinterpret_cast<float*>(base + L.off_sc_ndiag) : nullptr;
    }
    e->scoring = cfg->score_scratch != 0;
    if (e->scoring) {
        e->sv.hdr = reinterpret_cast<ScoreHdr*>(base + L.off_sc_hdr);
        e->sv.extent = reinterpret_cast<int*>(base + L.off_sc_ext);
        e->sv.mask = reinterpret_cast<float*>(base + L.off_sc_mask);
        e->sv.G = reinterpret_cast<double*>(base + L.off_sc_G);
        e->sv.P = (cfg->state_repr == IPP_FACTOR) ? reinterpret_cast<float*>(base + L.off_sc_P) : nullptr;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score_band), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    }
    e->n_bands = (L.N + kBandRows - 1) / kBandRows;
    e->prep_lds = prep_lds_bytes(L, *cfg);
    e->q_chunk = 2 * kPipe;  // (k_gain reads Q through the scalar cache: the LDS area only holds the prior table)
    // prior table of the factor base term lives in LDS when the grid is small enough (<= 48 KiB)
    e->lut_cap = (v.mode == IPP_FACTOR && L.N <= 12288) ? L.N : 0;
    e->gain_lds = gain_lds_bytes(v, e->q_chunk, e->lut_cap);
    if (v.mode == IPP_FACTOR && v.window_rows > 0) {
        const size_t MCs = v.meas_cap, LQ = (MCs * MCs + MCs + 3) & ~(size_t)3;
        e->fused = ((v.T == kStepThreads) && v.meas_cap == 9) || e->patch;  // (MC = 25: two launches, see launch_chunk)
        if (sw.fused) e->fused = e->fused && *sw.fused != 0;  // A/B experiments
        const int waves = v.T / 64;
        // prior table rows: a tile that holds new columns lies within window_rows of the footprint, so
        // |drow| <= window_rows + rows a tile spans + footprint height; farther rows (tall footprints) use sqrt / exp
        const int tile_rows = (v.tile_cells + v.W - 1) / v.W + 1;
        e->lut_rows = std::min(v.H, v.window_rows + tile_rows + 6);
        while (e->lut_rows > 0 && (size_t)e->lut_rows * v.W > 12288) --e->lut_rows;  // <= 48 KiB
        const int lutf = e->lut_rows * v.W;
        if (v.meas_cap == 9)
            e->gain_lds = e->fused ? std::max(GainLds<9>::bytes(v.rank_cap, step_work_floats<9>(v.rank_cap), lutf, step_small_floats<9>(), waves, v.win_tiles, v.win_tiles * kWave),
                                              GainLds<9>::bytes(v.rank_cap, step_work_floats<9>(v.rank_cap), lutf, step_small_floats<9>(), waves, v.win_tiles, 0, 0, v.vec))
                                   : GainLds<9>::bytes(v.rank_cap, 0, lutf, 0, waves, v.win_tiles, 0, 0, v.vec);
        else {
            // MC = 25: env steps are two launches (gain_lds = the gain kernel's), tree steps stay the fused tree kernel (its LDS below)
            e->gain_lds = GainLds<25>::bytes(v.rank_cap, 0, lutf, 0, waves, v.win_tiles, 0, 0, v.vec);
            e->tree_ok = v.T == kStepThreads;
            e->tree_fused_lds = std::max(GainLds<25>::bytes(v.rank_cap, step_work_floats<25>(v.rank_cap), lutf, step_small_floats<25>(), waves, v.win_tiles, v.win_tiles * kWave),
                                         GainLds<25>::bytes(v.rank_cap, step_work_floats<25>(v.rank_cap), lutf, step_small_floats<25>(), waves, v.win_tiles, 0, 0, v.vec));
        }
        if (e->patch) e->gain_lds = e->pp.tier[0].lds;
        if (v.T == kWave && !e->patch)
            e->gain_lds = (LQ + kTileLut) * 4 + (size_t)v.rank_cap * 4 + (8 * MCs) * 4 +
                          (size_t)(v.rank_cap + 8) * 2;
        e->gain_lds = (e->gain_lds + 15) & ~(size_t)15;
        if (e->gain_lds > 160 * 1024) {
            const size_t need = e->gain_lds;
            delete e;
            return fail(-1, "gain kernel needs %zu B of LDS (> 160 KiB): lower rank_cap", need);
        }
    }
    if (e->prep_lds > 160 * 1024) {
        delete e;
        return fail(-1, "prologue needs %zu B of LDS (> 160 KiB): lower rank_cap or max_measurements", e->prep_lds);
    }
    // opt in to > 64 KiB dynamic LDS for the prologue instantiations
    const int lds = (int)e->prep_lds;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_prepare<9, IPP_FACTOR>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_prepare<9, IPP_DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_prepare<25, IPP_FACTOR>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_prepare<25, IPP_DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    {  // patch kernels: opt in to more than the default 64 KB of dynamic LDS
        auto opt_in = [](auto* kernel) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); };
        // (the plain form and the IPP_BUDGET form)
#define X(NW, KPN, MINW, RJN) opt_in(k_step_patch<NW, KPN, MINW, RJN, false>); opt_in(k_step_patch<NW, KPN, MINW, RJN, true>);
        IPP_STEP_PATCH_KERNELS(X)
#undef X
#define X(NW, RJN) opt_in(k_tree_patch<NW, RJN>);
        IPP_TREE_PATCH_KERNELS(X)
#undef X
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_grf_conv<5, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_grf_conv<8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    const int glds = (int)e->gain_lds;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain<9, 4, IPP_FACTOR>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain<25, 2, IPP_FACTOR>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain_factor<9, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step_factor<9, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain_factor<9, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step_factor<9, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step_factor<9, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain_factor<9, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    if (e->fused) e->tree_ok = true;
    e->tree_step_lds = ((e->tree_fused_lds ? e->tree_fused_lds : e->gain_lds) + (size_t)v.rank_cap * 8 + 15) & ~(size_t)15;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_step<9, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_step_lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_step<9, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_step_lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_step<9, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_step_lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_step<9, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_step_lds);
    if (e->fused && e->tv.node_cap > 0 && v.meas_cap == 9) {
        // Split tree steps: worth it once the launch fills the device several times over (below that the second launch
        // and the scratch round trip of L^-1 | Q cost more than the occupancy gains); IPP_TREE_SPLIT=<min items> / 0
        e->tree_gain_lds = (GainLds<9>::bytes(v.rank_cap, 0, e->lut_rows * v.W, 0, e->tree_T / kWave, v.win_tiles, 0, v.rank_cap, v.vec) + 15) & ~(size_t)15;
        e->tree_split_min = 2048;
        if (sw.tree_split) e->tree_split_min = *sw.tree_split;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_prepare<9>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_gain<9, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_gain_lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_gain<9, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_gain_lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_gain<9, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_gain_lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_gain<9, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_gain_lds);
    }
    if (e->tv.node_cap > 0 && v.meas_cap == 25) {
        // MC = 25 tree steps: ALWAYS the two launches (prologue + gain kernel), like the env steps of these engines -- the fused
        // k_tree_step<25, 2> spilled 381 VGPRs (1412 bytes of scratch per lane) and is no longer instantiated
        e->tree_gain_lds = (GainLds<25>::bytes(v.rank_cap, 0, e->lut_rows * v.W, 0, e->tree_T / kWave, v.win_tiles, 0, v.rank_cap, v.vec) + 15) & ~(size_t)15;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_prepare<25>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tree_gain<25, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tree_gain_lds);
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain_factor<25, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain<9, 4, IPP_DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gain<25, 2, IPP_DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, glds);
    (void)hipGetLastError();
    // state starts zeroed (rank 0, padding 0); envs must still be ipp_reset before use
    HIP_TRY(hipMemset(base, 0, L.off_cov));
    hipLaunchKernelGGL(k_init_gt_slots, dim3((cfg->capacity + 255) / 256), dim3(256), 0, nullptr, v);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(base + L.off_hdr, 0, L.total - L.off_hdr));
    if (cfg->x_dim == cfg->y_dim) {
        std::vector<double> h;
        grf_kernel_host(cfg->y_dim, cfg->x_dim, cfg->cluster_radius, h);
        HIP_TRY(hipMemcpy(v.grf_h, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        const int n = cfg->x_dim;
        e->grf_dft = (n % 2 == 0) && n >= 4 && n <= 256;  // odd n: the reference's amp is not even (ground_truths.py:8-11)
        const bool hartley = !(sw.grf_hartley && *sw.grf_hartley == 0);  // A/B and tests: k_grf_dft as before the GEMM form existed
        if (e->grf_dft && n <= 128 && hartley) {
            const int tt = (n + 15) / 16;
            std::vector<double> hp, amp;
            bool ok = grf_hartley_tables_host(n, 16 * tt, cfg->cluster_radius, hp, amp);
            if (ok) {
                HIP_TRY(hipMemcpy(v.grf_hp, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(v.grf_amp, amp.data(), amp.size() * sizeof(double), hipMemcpyHostToDevice));
                e->grf_tt = tt;
                const int hl = (int)grf_hartley_lds_bytes(tt);
                const void* fn[] = {(const void*)&k_grf_hartley<1, 4>, (const void*)&k_grf_hartley<2, 4>, (const void*)&k_grf_hartley<3, 4>, (const void*)&k_grf_hartley<4, 4>,
                                    (const void*)&k_grf_hartley<5, 8>, (const void*)&k_grf_hartley<6, 8>, (const void*)&k_grf_hartley<7, 8>, (const void*)&k_grf_hartley<8, 4>};
                (void)hipFuncSetAttribute(fn[tt - 1], hipFuncAttributeMaxDynamicSharedMemorySize, hl);
                if (n == 50) (void)hipFuncSetAttribute((const void*)&k_grf_hartley<4, 4, 13>, hipFuncAttributeMaxDynamicSharedMemorySize, hl);
                if (n == 100) (void)hipFuncSetAttribute((const void*)&k_grf_hartley<7, 8, 25>, hipFuncAttributeMaxDynamicSharedMemorySize, hl);
                e->grf_fft = (n == 50 || n == 100);
                if (sw.grf_fft) e->grf_fft = e->grf_fft && *sw.grf_fft != 0;  // A/B: the GEMM form
            }
        }
        if (e->grf_dft) {
            std::vector<double> cs, g;
            grf_dft_tables_host(n, cfg->cluster_radius, cs, g);
            HIP_TRY(hipMemcpy(v.grf_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(v.grf_g, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
            const long budget = (n <= 64) ? 32768 : 65536;
            const long fixed = (n <= 100 ? (long)n * n * 4 : 0) + (long)n * 16 + 256;
            e->grf_kc = (int)std::max(1L, std::min((long)(n / 2 + 1), (budget - fixed) / ((long)n * 40)));
        }
    }
    if (sw.step_chunks) e->step_chunks = *sw.step_chunks;
    if (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) == hipSuccess) {
        (void)hipEventCreateWithFlags(&e->ev_begin, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&e->ev_end, hipEventDisableTiming);
        for (auto& ev : e->ev_prep) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    } else {
        e->side = nullptr;
        (void)hipGetLastError();
    }
    *engine = e;
    return 0;
}

int ipp_engine_destroy(void* engine) {
#if IPP_MCTS_CLOCKS
    {
        unsigned long long c[16];
        if (hipMemcpyFromSymbol(c, HIP_SYMBOL(g_mclk), sizeof c) == hipSuccess && c[8]) {
            const double lv = (double)c[8], ds = (double)c[9];
            fprintf(stderr, "[k_mcts_select, us per level (lane 0, sections serialised)] rows + min/max %.2f  PUCT + argmax %.2f  edge fields + cost %.2f  "
                            "hash lookup %.2f  child record %.2f  bookkeeping %.2f | per descent: start %.2f  leaf + fence %.2f | levels %.0f descents %.0f (%.2f levels each)\n",
                    c[1] / lv / 100, c[2] / lv / 100, c[3] / lv / 100, c[4] / lv / 100, c[5] / lv / 100, c[6] / lv / 100, c[0] / ds / 100, c[7] / ds / 100, lv, ds, lv / ds);
            memset(c, 0, sizeof c);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mclk), c, sizeof c);
        }
    }
#endif
    Engine* e = as_engine(engine);
    if (!e) return 0;
    prof_drain(e);
    if (e->side) {
        (void)hipStreamSynchronize(e->side);
        (void)hipStreamDestroy(e->side);
        (void)hipEventDestroy(e->ev_begin);
        (void)hipEventDestroy(e->ev_end);
        for (auto& ev : e->ev_prep) (void)hipEventDestroy(ev);
    }
    delete e;
    return 0;
}

int ipp_grf_generator(void* engine, int32_t* kind, int32_t* param) {  // (the order of launch_grf)
    Engine* e = as_engine(engine);
    if (!e || !kind || !param) return fail(-1, "null argument");
    if (e->grf_tt > 0) { *kind = e->grf_fft ? IPP_GRF_GEN_FFT : IPP_GRF_GEN_HARTLEY; *param = e->grf_tt; }
    else if (e->grf_dft) { *kind = IPP_GRF_GEN_DFT; *param = e->grf_kc; }
    else { *kind = IPP_GRF_GEN_CONV; *param = 0; }
    return 0;
}

int ipp_set_grf_rows(void* engine, int32_t all_grids) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (all_grids != 0 && all_grids != 1) return fail(-1, "ipp_set_grf_rows: all_grids = %d, 0 or 1", all_grids);
    if (all_grids && !e->grf_dft)
        return fail(-1, "ipp_set_grf_rows: %d x %d (x_dim x y_dim) grid: generators that draw their own noise exist on even square grids of 4 .. 256 cells a side",
                    e->v.W, e->v.H);
    e->grf_rows_all = all_grids != 0;
    return 0;
}

int ipp_engine_info(void* engine, ipp_info* out) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    out->abi_version = IPP_ABI_VERSION;
    out->n_cells = e->v.N;
    out->n_pad = e->v.Npad;
    out->tile_threads = e->v.T;
    out->n_tiles = e->v.n_tiles;
    out->meas_cap = e->v.meas_cap;
    out->fp_cap = e->v.fp_cap;
    out->window_rows = e->v.window_rows;
    out->arena_bytes = e->used_bytes;
    out->cov_slot_bytes = e->v.cov_slot * 4;
    out->step_lds_bytes = e->gain_lds;
    out->fused_step = e->fused ? 1 : 0;
    out->patch_layout = e->patch ? 1 : 0;
    out->patch_waves = e->patch ? e->pp.tier[0].waves : 0;
    out->patch_big_min_items = e->patch ? e->pp.tier[e->pp.big_tier].min_items : 0;  // (tier[0].min_items = 0: no such tier)
    out->patch_two_wave_min_items = e->patch ? e->pp.tier[e->pp.two_wave_tier].min_items : 0;
    out->patch_split_min_items = 0;  // (always: the field only keeps the struct's layout)
    return 0;
}

int ipp_reset_episode(void* engine, const int32_t* env_ids, int32_t n, const double* prior_scale, const float* gt,
                      const float* white_noise, double* prev_action, const double* init_action, void* stream) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (!env_ids && n > e->v.cap) return fail(-1, "n exceeds capacity");
    if (prev_action && !init_action) return fail(-1, "prev_action needs init_action");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const View& v = e->v;
    HIP_TRY(hipSetDevice(e->device));
    InitAction ia = {{0.0, 0.0, 0.0}};
    if (init_action) for (int k = 0; k < 3; ++k) ia.p[k] = init_action[k];
    hipLaunchKernelGGL(k_reset_small, dim3((v.Npad + 255) / 256, n), dim3(256), 0, s, v, env_ids, n, prior_scale, gt, prev_action, ia);
    if (!gt && white_noise) {
        if (v.W != v.H) return fail(-1, "device GRF needs a square grid (the reference transposes its dims, simulations/simulations.py:45-47)");
        if (int rc = launch_grf(e, n, white_noise, v.grf_raw, env_ids, nullptr, s)) return rc;
    }
    if (v.mode == IPP_DENSE) {
        const int n_ctiles = (v.Npad + 1023) / 1024;
        const int grid = grid_for(n, e->n_bands * n_ctiles);
        hipLaunchKernelGGL(k_reset_dense, dim3(grid), dim3(256), 0, s, v, env_ids, n, e->n_bands, n_ctiles);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_reset(void* engine, const int32_t* env_ids, int32_t n, const double* prior_scale, const float* gt,
              const float* white_noise, void* stream) {
    return ipp_reset_episode(engine, env_ids, n, prior_scale, gt, white_noise, nullptr, nullptr, stream);
}

static int step_impl(void* engine, const int32_t* env_ids, const int32_t* dst_ids, int32_t n, const double* action,
                     const double* prev_action, const float* meas_noise, uint32_t flags, float* reward, int32_t* status,
                     void* stream, const AutoReset& ar) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!action || !prev_action || !reward) return fail(-1, "action, prev_action and reward are required");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (!env_ids && n > e->v.cap) return fail(-1, "n exceeds capacity");
    if (flags & ~(IPP_COV_ONLY | IPP_PREDICT_ONLY | IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME | IPP_GIVEN_OBSERVATION | IPP_UPDATE_PREV | IPP_BUDGET | IPP_RESET_ON_DONE)) return fail(-1, "unknown flag bits 0x%x", flags);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    e->last_n = n;
    if (e->v.mode == IPP_FACTOR && dst_ids && !(flags & IPP_PREDICT_ONLY)) {
        // factor state: an out-of-place step is a slot copy followed by an in-place step on the copy
        // (the dense downdate kernel writes P_dst = P_src - Wc Wc^T directly instead)
        if (!env_ids) return fail(-1, "dst_ids needs explicit env_ids");
        if (int rc = ipp_fork(engine, env_ids, dst_ids, n, stream)) return rc;
        env_ids = dst_ids;
        dst_ids = nullptr;
    }
    // the fused kernel resets the flagged envs itself; every other path gets a separate launch behind the step
    const bool in_kernel = e->fused;
    const AutoReset none = {nullptr, nullptr, nullptr, nullptr, {0.0, 0.0, 0.0}};
    int rc;
    if (e->v.meas_cap == 9)
        rc = (e->v.vec == 2) ? launch_step<9, 2>(e, env_ids, dst_ids, n, action, prev_action, meas_noise, flags, reward, status, s, in_kernel ? ar : none)
                             : launch_step<9, 4>(e, env_ids, dst_ids, n, action, prev_action, meas_noise, flags, reward, status, s, in_kernel ? ar : none);
    else
        rc = launch_step<25, 2>(e, env_ids, dst_ids, n, action, prev_action, meas_noise, flags, reward, status, s, in_kernel ? ar : none);
    if (rc == 0 && ar.src && !in_kernel) {
        hipLaunchKernelGGL(k_reset_flagged, dim3((e->v.Npad + 255) / 256, n), dim3(256), 0, s, e->v, env_ids, n, ar);
        HIP_TRY(hipGetLastError());
    }
    return rc;
}

int ipp_step(void* engine, const int32_t* env_ids, const int32_t* dst_ids, int32_t n, const double* action,
             const double* prev_action, const float* meas_noise, uint32_t flags, float* reward, int32_t* status,
             void* stream) {
    if (flags & (IPP_BUDGET | IPP_RESET_ON_DONE)) return fail(-1, "ipp_step: IPP_BUDGET / IPP_RESET_ON_DONE are flags of ipp_step_autoreset and ipp_step_parts");
    const AutoReset none = {nullptr, nullptr, nullptr, nullptr, {0.0, 0.0, 0.0}};
    return step_impl(engine, env_ids, dst_ids, n, action, prev_action, meas_noise, flags, reward, status, stream, none);
}

// Why a budget step (IPP_BUDGET / IPP_RESET_ON_DONE) cannot run on this engine with these arguments, or nullptr.  The ledger lives in
// the fused patch-step kernels only: no silent fallback to a path without it.  n: items of one launch (a part's, for ipp_step_parts).
static const char* budget_launch_error(const Engine* e, uint32_t flags, int n, const int32_t* env_ids, const int32_t* reset_src,
                                       const float* reset_gt, const double* init_action) {
    if (!(flags & (IPP_BUDGET | IPP_RESET_ON_DONE))) return nullptr;
    if (!(flags & IPP_BUDGET)) return "IPP_RESET_ON_DONE needs IPP_BUDGET";
    if (!e->led.budget) return "IPP_BUDGET: no ledger installed (ipp_set_budget)";
    if (e->v.mode != IPP_FACTOR || !e->patch || !e->fused) return "IPP_BUDGET: patch-layout factor engines only (ipp_info.patch_layout == 1)";
    if (flags & IPP_PREDICT_ONLY) return "IPP_BUDGET: not with IPP_PREDICT_ONLY (the ledger charges committed steps)";
    if (env_ids) return "IPP_BUDGET: full-batch in-place steps only (env_ids == NULL)";
    if (n > e->v.cap) return "IPP_BUDGET: more items than env slots";
    if (e->step_chunks > 1) return "IPP_BUDGET: not with a chunked step (IPP_STEP_CHUNKS)";
    if (flags & IPP_RESET_ON_DONE) {
        if (reset_src || reset_gt) return "IPP_RESET_ON_DONE: the resets come from the ledger (reset_src and reset_gt must be NULL)";
        if (!init_action) return "IPP_RESET_ON_DONE needs init_action";
        if (e->reset_prior) return "IPP_RESET_ON_DONE: no per-episode reset priors (ipp_set_reset_prior)";
    }
    return nullptr;
}

int ipp_set_budget(void* engine, double* budget, int32_t* depth, int64_t* episode, uint8_t* done, int32_t* refill,
                   double initial_budget, int32_t max_steps, int32_t shuffle_budget, uint64_t seed, int64_t row_offset) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!budget) { e->led = Ledger{}; return 0; }
    if (!depth || !episode || !done || !refill) return fail(-1, "ipp_set_budget: budget, depth, episode, done and refill are required");
    if (!e->patch) return fail(-1, "ipp_set_budget: patch-layout factor engines only (ipp_info.patch_layout == 1)");
    if (!(initial_budget >= e->v.res)) return fail(-1, "ipp_set_budget: initial_budget %g below the resolution %g", initial_budget, e->v.res);
    if (shuffle_budget && !(initial_budget >= 10.0)) return fail(-1, "ipp_set_budget: shuffle_budget needs initial_budget >= 10");
    if (max_steps < 1) return fail(-1, "ipp_set_budget: max_steps < 1");
    Ledger L = {};
    L.budget = budget; L.depth = depth; L.episode = reinterpret_cast<long long*>(episode); L.done = done; L.refill = refill;
    L.b0 = initial_budget; L.res = e->v.res; L.max_steps = max_steps; L.shuffle = shuffle_budget ? kLedgerShuffleBudget : 0; L.seed = seed;
    L.row_offset = (long long)row_offset;
    e->led = L;
    return 0;
}

int ipp_set_budget_prior(void* engine, int32_t shuffle_prior) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!e->led.budget) return fail(-1, "ipp_set_budget_prior: no ledger installed (ipp_set_budget)");
    if (!e->patch || e->v.mode != IPP_FACTOR) return fail(-1, "ipp_set_budget_prior: patch-layout factor engines only (ipp_info.patch_layout == 1)");
    if (shuffle_prior && e->v.ls_max > 0.0 && e->cfg.fixed_prior)
        return fail(-1, "ipp_set_budget_prior: the column window (%d rows) was sized for the nominal length scale (ipp_config.fixed_prior = 1): "
                        "a drawn length scale of up to 1.2 x %g m would poison envs; create the engine with fixed_prior = 0",
                    e->v.window_rows, e->cfg.length_scale);
    if (shuffle_prior) e->led.shuffle |= kLedgerShufflePrior;
    else e->led.shuffle &= ~kLedgerShufflePrior;
    return 0;
}

int ipp_read_prior(void* engine, const int32_t* env_ids, int32_t n, double* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (n < 0 || (!env_ids && n > e->v.cap)) return fail(-1, "ipp_read_prior: n = %d outside [0, capacity = %d]", n, e->v.cap);
    if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(-1, "ipp_read_prior: out must be 16-byte aligned");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_read_prior, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, env_ids, n,
                       reinterpret_cast<double2*>(out));
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_step_autoreset(void* engine, const int32_t* env_ids, int32_t n, const double* action, double* prev_action,
                       const float* meas_noise, uint32_t flags, float* reward, int32_t* status, const int32_t* reset_src,
                       const float* reset_gt, const double* init_action, void* stream) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (e->v.mode != IPP_FACTOR) return fail(-1, "ipp_step_autoreset: factor state only (dense engines: ipp_step + ipp_reset_episode)");
    if (flags & IPP_PREDICT_ONLY) return fail(-1, "ipp_step_autoreset: not with IPP_PREDICT_ONLY");
    if (reset_src && !init_action) return fail(-1, "reset_src needs init_action");  // (reset_gt == NULL: the ground truths were staged into the alternate planes)
    if (const char* why = budget_launch_error(e, flags, n, env_ids, reset_src, reset_gt, init_action)) return fail(-1, "ipp_step_autoreset: %s", why);
    AutoReset ar = {reset_src, reset_gt, reset_src ? e->reset_prior : nullptr, reset_src ? prev_action : nullptr, {0.0, 0.0, 0.0}};
    if (init_action) for (int k = 0; k < 3; ++k) ar.init[k] = init_action[k];
    if (flags & IPP_BUDGET) {
        ar.led = e->led;
        if (flags & IPP_RESET_ON_DONE) ar.prev = prev_action;
    }
    return step_impl(engine, env_ids, nullptr, n, action, prev_action, meas_noise, flags, reward, status, stream, ar);
}

int ipp_step_parts(void* engine, int32_t n, const double* action, double* prev_action, const float* meas_noise,
                   uint32_t flags, float* reward, int32_t* status, const int32_t* reset_src, const float* reset_gt,
                   const double* init_action, int32_t n_parts, const int32_t* part_begin, void* const* streams) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!action || !prev_action || !reward || !part_begin || !streams) return fail(-1, "null argument");
    if (e->v.mode != IPP_FACTOR || !(e->fused || e->patch) || e->v.meas_cap != 9 || e->v.vec != 2)
        return fail(-1, "ipp_step_parts: engines whose step is one fused kernel only (ipp_info.fused_step)");
    // (predict-only parts: reward / status of every item, no state write -- consecutive calls do not depend on each other at all)
    if ((flags & IPP_PREDICT_ONLY) && (reset_src || (flags & IPP_UPDATE_PREV))) return fail(-1, "ipp_step_parts: IPP_PREDICT_ONLY with resets or IPP_UPDATE_PREV");
    if (flags & ~(IPP_COV_ONLY | IPP_PREDICT_ONLY | IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME | IPP_GIVEN_OBSERVATION | IPP_UPDATE_PREV | IPP_BUDGET | IPP_RESET_ON_DONE)) return fail(-1, "unknown flag bits 0x%x", flags);
    if (n <= 0 || n > e->v.max_batch || n > e->v.cap) return fail(-1, "n = %d outside [1, min(max_batch, capacity)]", n);
    if (!e->v.item_order || e->v.item_order_n != n) return fail(-1, "ipp_step_parts: needs the dispatch order of all n items (ipp_set_item_order)");
    if (n_parts < 1 || n_parts > kMaxChunks) return fail(-1, "n_parts = %d outside [1, %d]", n_parts, kMaxChunks);
    if (part_begin[0] != 0 || part_begin[n_parts] != n) return fail(-1, "part_begin has to run from 0 to n");
    for (int p = 0; p < n_parts; ++p)
        if (part_begin[p + 1] <= part_begin[p]) return fail(-1, "part %d is empty", p);
    if (reset_src && !init_action) return fail(-1, "reset_src needs init_action");
    for (int p = 0; p < n_parts; ++p)
        if (const char* why = budget_launch_error(e, flags, part_begin[p + 1] - part_begin[p], nullptr, reset_src, reset_gt, init_action))
            return fail(-1, "ipp_step_parts: %s", why);
    AutoReset ar = {reset_src, reset_gt, reset_src ? e->reset_prior : nullptr, reset_src ? prev_action : nullptr, {0.0, 0.0, 0.0}};
    if (init_action) for (int k = 0; k < 3; ++k) ar.init[k] = init_action[k];
    if (flags & IPP_BUDGET) {
        ar.led = e->led;
        if (flags & IPP_RESET_ON_DONE) ar.prev = prev_action;
    }
    HIP_TRY(hipSetDevice(e->device));
    e->last_n = n;
    for (int p = 0; p < n_parts; ++p) {
        View v = e->v;  // (the per-item arrays keep their batch indexing: a part is a range of positions of the order)
        v.pos0 = part_begin[p];  // (the budget ledger's refill list is indexed by the dispatch position)
        v.item_order = e->v.item_order + part_begin[p];
        v.item_order_n = part_begin[p + 1] - part_begin[p];
        launch_chunk<9, 2>(e, v, nullptr, nullptr, v.item_order_n, action, prev_action, meas_noise, flags, reward, status,
                           reinterpret_cast<hipStream_t>(streams[p]), nullptr, ar);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_generate_grf(void* engine, int32_t n, const float* white_noise, float* gt_out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !white_noise || !gt_out) return fail(-1, "null argument");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    return launch_grf(e, n, white_noise, e->v.grf_raw2, nullptr, gt_out, reinterpret_cast<hipStream_t>(stream));
}

int ipp_generate_grf_rows(void* engine, int32_t n, const int32_t* row_ids, int64_t row_offset, uint64_t seed, uint64_t subsequence,
                          float* gt_out, void* stream) {
    return ipp_generate_grf_groups(engine, n, 0, nullptr, row_ids, row_offset, seed, subsequence, gt_out, stream);
}

int ipp_generate_grf_groups(void* engine, int32_t n, int32_t group_rows, const int64_t* group_subsequence, const int32_t* row_ids,
                            int64_t row_offset, uint64_t seed, uint64_t subsequence, float* gt_out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!gt_out && !row_ids) return fail(-1, "ipp_generate_grf_groups: gt_out == NULL writes the alternate plane of env row_ids[i]: row_ids needed");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (group_rows < 0 || (group_rows > 0 && (!group_subsequence || (n + group_rows - 1) / group_rows > 16)))
        return fail(-1, "ipp_generate_grf_groups: at most 16 groups of group_rows fields, with their subsequence offsets");
    if (!grf_draws_noise(e)) return fail(-3, "ipp_generate_grf_rows: this grid has no generator that draws its own noise (ipp_fill_normal_rows + ipp_generate_grf; ipp_set_grf_rows)");
    HIP_TRY(hipSetDevice(e->device));
    GrfNoise gn = {row_ids, (long long)row_offset, seed, subsequence, group_rows, {0}, gt_out ? 0 : 1};
    for (int g = 0; group_rows > 0 && g < (n + group_rows - 1) / group_rows; ++g) gn.group_subseq[g] = (long long)group_subsequence[g];
    return launch_grf(e, n, nullptr, e->v.grf_raw2, nullptr, gt_out, reinterpret_cast<hipStream_t>(stream), &gn);
}

int ipp_generate_grf_refill(void* engine, int32_t n, const int32_t* refill, const int64_t* episode, int64_t row_offset, uint64_t seed,
                            uint64_t subsequence, void* stream) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!refill || !episode) return fail(-1, "ipp_generate_grf_refill: refill and episode are required");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (!grf_draws_noise(e)) return fail(-3, "ipp_generate_grf_refill: this grid has no generator that draws its own noise (50x50 / 100x100 grids; ipp_set_grf_rows)");
    HIP_TRY(hipSetDevice(e->device));
    GrfNoise gn = {refill, (long long)row_offset, seed, subsequence, 0, {0}, 1, reinterpret_cast<const long long*>(episode)};
    return launch_grf(e, n, nullptr, e->v.grf_raw2, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream), &gn);
}

}  // extern "C"

namespace {

// Hotspot draws need a non-empty set of admissible second centres for every first centre on both axes (the reference's rejection
// loop, simulations/simulations.py:71-86, never ends otherwise) and trunc(r) < dim (its randint raises).
bool hotspot_axis_ok(int dim, double r) {
    if (!(r >= 0.0) || (double)(int)std::min(r, 1e9) >= (double)dim) return false;
    const int lo = (int)r;
    for (int c = lo; c < dim; ++c) {
        const int left_end = (int)std::ceil((double)c - r) - 1, right_beg = (int)std::floor((double)c + r) + 1;
        if (std::max(0, left_end - lo + 1) + std::max(0, dim - std::max(right_beg, lo)) == 0) return false;
    }
    return true;
}

int field_kind_check(const Engine* e, int kind, const char* fn) {
    if (kind == IPP_FIELD_HOTSPOT) {
        const double r = e->cfg.cluster_radius;
        if (!hotspot_axis_ok(e->v.H, r) || !hotspot_axis_ok(e->v.W, r))
            return fail(-1, "%s: hotspot fields on %d x %d with cluster_radius %g: a first centre can leave no second one more than r away "
                            "on an axis (the reference loops forever), or trunc(r) >= the grid", fn, e->v.H, e->v.W, r);
        return 0;
    }
    if (kind == IPP_FIELD_SPLIT) return 0;
    return fail(-1, "%s: unknown field kind %d", fn, kind);
}

int launch_fields(Engine* e, int n, int kind, const ipp_field_record* rec, float* gt_out, const GrfNoise& gn, hipStream_t s) {
    const View& v = e->v;
    const bool vec4 = gt_out ? ((v.N & 3) == 0 && (reinterpret_cast<uintptr_t>(gt_out) & 15) == 0)
                             : ((v.Npad & 3) == 0 && (reinterpret_cast<uintptr_t>(v.gt) & 15) == 0);
    if (gn.episode)
        hipLaunchKernelGGL((k_fields<true>), dim3(n), dim3(kFieldThreads), 0, s, v, n, kind, e->cfg.cluster_radius, rec, gt_out, gn, (int)vec4);
    else
        hipLaunchKernelGGL((k_fields<false>), dim3(n), dim3(kFieldThreads), 0, s, v, n, kind, e->cfg.cluster_radius, rec, gt_out, gn, (int)vec4);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int ipp_generate_field_groups(void* engine, int32_t kind, int32_t n, int32_t group_rows, const int64_t* group_subsequence, const int32_t* row_ids,
                              int64_t row_offset, uint64_t seed, uint64_t subsequence, float* gt_out, void* stream) {
    if (kind == IPP_FIELD_GRF)
        return ipp_generate_grf_groups(engine, n, group_rows, group_subsequence, row_ids, row_offset, seed, subsequence, gt_out, stream);
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (int rc = field_kind_check(e, kind, "ipp_generate_field_groups")) return rc;
    if (!gt_out && !row_ids) return fail(-1, "ipp_generate_field_groups: gt_out == NULL writes the alternate plane of env row_ids[i]: row_ids needed");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (group_rows < 0 || (group_rows > 0 && (!group_subsequence || (n + group_rows - 1) / group_rows > 16)))
        return fail(-1, "ipp_generate_field_groups: at most 16 groups of group_rows fields, with their subsequence offsets");
    HIP_TRY(hipSetDevice(e->device));
    GrfNoise gn = {row_ids, (long long)row_offset, seed, subsequence, group_rows, {0}, gt_out ? 0 : 1};
    for (int g = 0; group_rows > 0 && g < (n + group_rows - 1) / group_rows; ++g) gn.group_subseq[g] = (long long)group_subsequence[g];
    return launch_fields(e, n, kind, nullptr, gt_out, gn, reinterpret_cast<hipStream_t>(stream));
}

int ipp_generate_field_refill(void* engine, int32_t kind, int32_t n, const int32_t* refill, const int64_t* episode, int64_t row_offset,
                              uint64_t seed, uint64_t subsequence, void* stream) {
    if (kind == IPP_FIELD_GRF) return ipp_generate_grf_refill(engine, n, refill, episode, row_offset, seed, subsequence, stream);
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (int rc = field_kind_check(e, kind, "ipp_generate_field_refill")) return rc;
    if (!refill || !episode) return fail(-1, "ipp_generate_field_refill: refill and episode are required");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    GrfNoise gn = {refill, (long long)row_offset, seed, subsequence, 0, {0}, 1, reinterpret_cast<const long long*>(episode)};
    return launch_fields(e, n, kind, nullptr, nullptr, gn, reinterpret_cast<hipStream_t>(stream));
}

int ipp_fill_fields(void* engine, int32_t n, const ipp_field_record* records, const int32_t* row_ids, float* gt_out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!records) return fail(-1, "ipp_fill_fields: records are required");
    if (!gt_out && !row_ids) return fail(-1, "ipp_fill_fields: gt_out == NULL writes the alternate plane of env row_ids[i]: row_ids needed");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    GrfNoise gn = {gt_out ? nullptr : row_ids, 0, 0, 0, 0, {0}, gt_out ? 0 : 1};
    return launch_fields(e, n, IPP_FIELD_HOTSPOT, records, gt_out, gn, reinterpret_cast<hipStream_t>(stream));
}

int ipp_observe(void* engine, const int32_t* env_ids, int32_t n, const double* action, const float* meas_noise,
                float* z_out, int32_t* m_out, int32_t* shape_out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !action || !z_out || !m_out) return fail(-1, "null argument");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const View& v = e->v;
    // the prologue kernel in observation-only mode (prev_action is unused there: pass action)
    if (v.meas_cap == 9) {
        if (v.mode == IPP_FACTOR)
            hipLaunchKernelGGL((k_prepare<9, IPP_FACTOR>), dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, (const int*)nullptr, n, action, action, meas_noise, 0u, (int*)nullptr, z_out, m_out, shape_out);
        else
            hipLaunchKernelGGL((k_prepare<9, IPP_DENSE>), dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, (const int*)nullptr, n, action, action, meas_noise, 0u, (int*)nullptr, z_out, m_out, shape_out);
    } else {
        if (v.mode == IPP_FACTOR)
            hipLaunchKernelGGL((k_prepare<25, IPP_FACTOR>), dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, (const int*)nullptr, n, action, action, meas_noise, 0u, (int*)nullptr, z_out, m_out, shape_out);
        else
            hipLaunchKernelGGL((k_prepare<25, IPP_DENSE>), dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, env_ids, (const int*)nullptr, n, action, action, meas_noise, 0u, (int*)nullptr, z_out, m_out, shape_out);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_set_uav(void* engine, double max_v, double max_a) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (!(max_v > 0) || !(max_a > 0)) return fail(-1, "max_v and max_a must be positive");
    e->v.vmax = max_v;
    e->v.amax = max_a;
    return 0;
}

int ipp_set_item_order(void* engine, const int32_t* order, int32_t n) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    if (order && (n <= 0 || n > e->v.max_batch)) return fail(-1, "n = %d outside [1, max_batch = %d]", n, e->v.max_batch);
    e->v.item_order = order;
    e->v.item_order_n = order ? n : 0;
    return 0;
}

int ipp_set_reset_prior(void* engine, const double* prior) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    e->reset_prior = prior;
    return 0;
}

int ipp_set_adaptive(void* engine, double value_threshold, double interval_factor) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    e->v.thr = value_threshold;
    e->v.kf = interval_factor;
    return 0;
}

static int score_actions_impl(void* engine, int32_t env_id, const ScorePath& path, const float* node_diag, const double* actions,
                              int32_t n, const double* prev_action, uint32_t flags, float* reward, int32_t* status, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !actions || !prev_action || !reward) return fail(-1, "null argument");
    if (!e->scoring) return fail(-1, "ipp_score_actions needs ipp_config.score_scratch = 1");
    if (int rc = check_env(e, env_id)) return rc;
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (flags & ~(IPP_COV_ONLY | IPP_PREDICT_ONLY | IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) return fail(-1, "unsupported flag bits 0x%x", flags);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const View& v = e->v;
    int band_kc = 64;  // columns k per LDS tile: 2 row blocks of W cells in fp64
    while (band_kc > 8 && (size_t)2 * v.W * (band_kc + 1) * sizeof(double) > 64 * 1024) band_kc /= 2;
    const size_t band_lds = (size_t)2 * v.W * (band_kc + 1) * sizeof(double);
    if (band_lds > 150 * 1024) return fail(-1, "grid rows of %d cells exceed the band kernel's LDS tiles", v.W);
    ScoreView sv = e->sv;
    if (v.mode == IPP_DENSE) sv.P = v.cov + (size_t)env_id * v.cov_slot;
    PrevAction pa = {{prev_action[0], prev_action[1], prev_action[2]}};
    HIP_TRY(hipMemsetAsync(sv.extent, 0, 8, s));
    const int hdr_blocks = std::max((n + 255) / 256, std::min(64, (v.Npad + 255) / 256));
    if (v.meas_cap == 9) hipLaunchKernelGGL((k_score_hdr<9>), dim3(hdr_blocks), dim3(256), 0, s, v, sv, env_id, actions, n, pa, flags, reward, status, node_diag);
    else                 hipLaunchKernelGGL((k_score_hdr<25>), dim3(hdr_blocks), dim3(256), 0, s, v, sv, env_id, actions, n, pa, flags, reward, status, node_diag);
    if (v.mode == IPP_FACTOR && path.depth > 0)
        hipLaunchKernelGGL(k_score_densify<true>, dim3(v.Npad / 64, (v.N + 63) / 64), dim3(256), 0, s, v, sv, env_id, path, e->tv.node_cov, e->tv.node_meta, e->tv.win_cells);
    else if (v.mode == IPP_FACTOR)
        hipLaunchKernelGGL(k_score_densify<false>, dim3(v.Npad / 64, (v.N + 63) / 64), dim3(256), 0, s, v, sv, env_id, path, nullptr, nullptr, 0);
    hipLaunchKernelGGL(k_score_band, dim3(v.H, kScoreDCap + 1, kScoreSplit), dim3(256), band_lds, s, v, sv, band_kc);
    if (v.meas_cap == 9) hipLaunchKernelGGL((k_score_eval<9>), dim3((n + 3) / 4), dim3(256), 0, s, v, sv, n, reward);
    else                 hipLaunchKernelGGL((k_score_eval<25>), dim3((n + 3) / 4), dim3(256), 0, s, v, sv, n, reward);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// the search calls' side of the engine (ipp_host.h)
int ipp::tree_engine(void* engine, TreeEngine* out) {
    const Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    *out = TreeEngine{e->device, e->v.max_batch, e->tv.node_cap, e->tree_ok, e->patch, e->v.vmax, e->v.amax};
    return 0;
}

int ipp::factor_slots(void* engine, FactorSlots* out) {
    const Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    const View& v = e->v;
    *out = FactorSlots{e->device, v.cap, v.rank_cap, v.N, v.Npad, v.pstride, e->patch && v.mode == IPP_FACTOR, v.cov_slot,
                       v.cov, v.colspan, v.colrect, v.rank, v.prior, v.mean,
                       (e->led.budget && (e->led.shuffle & kLedgerShufflePrior)) ? 1 : 0, v.sv0, v.ls0, e->led.seed, e->led.row_offset,
                       e->led.depth, e->led.episode};
    return 0;
}

int ipp::slot_store(void* engine, SlotStore* out) {
    const Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    const View& v = e->v;
    *out = SlotStore{e->device, v.mode, v.cap, v.rank_cap, v.W, v.H, v.N, v.Npad, v.pw, v.ph, v.pstride, v.window_rows, v.tile_cells,
                     v.prior_kind, e->patch && v.mode == IPP_FACTOR, v.cov_slot, v.cov, v.colspan, v.colrect, v.rank, v.prior,
                     v.mean, v.diag, v.gt, v.gt_slot};
    return 0;
}

int ipp::tree_step(void* engine, const int32_t* root_ids, const int32_t* path_ids, const int32_t* new_ids, int32_t n, const double* action,
                   const double* prev_action, uint32_t flags, float* reward, int32_t* status, void* stream, const int32_t* n_dev,
                   const TreeEdgeOut* edge_out) {
    Engine* e = as_engine(engine);
    if (!e || !root_ids || !path_ids || !action || !prev_action || !reward) return fail(-1, "null argument");
    if (e->tv.node_cap <= 0) return fail(-1, "ipp_tree_step needs ipp_config.node_capacity > 0");
    if (!e->tree_ok) return fail(-1, "ipp_tree_step needs IPP_FACTOR with window_rows > 0 and the default tile_threads");
    if (n < 0 || n > e->v.max_batch) return fail(-1, "n = %d outside [0, max_batch = %d]", n, e->v.max_batch);
    if (n == 0) return 0;
    if (flags & ~(IPP_COV_ONLY | IPP_PREDICT_ONLY | IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) return fail(-1, "unsupported flag bits 0x%x", flags);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    e->last_n = n;
    const View& v = e->v;
    if (e->patch) {  // tree nodes as patches: one fused kernel for every launch size (k_tree_patch.h)
        const PatchVariant& pv = e->pp.tree;
        const TreeEdgeOut eo = edge_out ? *edge_out : TreeEdgeOut{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
        timed_launch(e, 0, tree_patch_kernel(pv), dim3(n), dim3(64 * pv.waves), pv.lds, s, v, e->tv, root_ids, path_ids, new_ids, n, action, prev_action, flags, status,
                     reward, n_dev, eo);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (n_dev) return fail(-1, "device-side item counts need the patch layout (ipp_info.patch_layout)");
    if (v.meas_cap == 9 && e->tree_split_min > 0 && n >= e->tree_split_min) {
        timed_launch(e, 2, k_tree_prepare<9>, dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, e->tv, root_ids, path_ids, new_ids, n, action,
                     prev_action, flags, status);
#define IPP_TREE_GAIN(V, R) timed_launch(e, 0, k_tree_gain<9, V, R>, dim3(n), dim3(e->tree_T), e->tree_gain_lds, s, v, e->tv, (const float*)v.q, \
                                         root_ids, path_ids, new_ids, n, flags, e->lut_rows, reward)
        if (v.vec == 2) { if (e->rect_tree) IPP_TREE_GAIN(2, true); else IPP_TREE_GAIN(2, false); }
        else            { if (e->rect_tree) IPP_TREE_GAIN(4, true); else IPP_TREE_GAIN(4, false); }
#undef IPP_TREE_GAIN
    } else if (v.meas_cap == 9) {
#define IPP_TREE_STEP(V, R) timed_launch(e, 0, k_tree_step<9, V, R>, dim3(n), dim3(kStepThreads), e->tree_step_lds, s, v, e->tv, root_ids, path_ids, \
                                         new_ids, n, action, prev_action, flags, e->lut_rows, status, reward)
        if (v.vec == 2) { if (e->rect_tree) IPP_TREE_STEP(2, true); else IPP_TREE_STEP(2, false); }
        else            { if (e->rect_tree) IPP_TREE_STEP(4, true); else IPP_TREE_STEP(4, false); }
#undef IPP_TREE_STEP
    }
    else {
        if (v.vec != 2) return fail(-1, "tree steps with max_measurements = 25 need two cells per lane");
        timed_launch(e, 2, k_tree_prepare<25>, dim3(n), dim3(kPrepThreads), e->prep_lds, s, v, e->tv, root_ids, path_ids, new_ids, n, action,
                     prev_action, flags, status);
        timed_launch(e, 0, k_tree_gain<25, 2>, dim3(n), dim3(e->tree_T), e->tree_gain_lds, s, v, e->tv, (const float*)v.q, root_ids, path_ids,
                     new_ids, n, flags, e->lut_rows, reward);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int ipp_tree_step(void* engine, const int32_t* root_ids, const int32_t* path_ids, const int32_t* new_ids, int32_t n,
                  const double* action, const double* prev_action, uint32_t flags, float* reward, int32_t* status,
                  void* stream) {
    return tree_step(engine, root_ids, path_ids, new_ids, n, action, prev_action, flags, reward, status, stream, nullptr, nullptr);
}

int ipp_tree_read_diag(void* engine, int32_t node_id, float* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (node_id < 0 || node_id >= e->tv.node_cap) return fail(-1, "node_id %d outside [0, %d)", node_id, e->tv.node_cap);
    HIP_TRY(hipSetDevice(e->device));
    if (e->patch)
        hipLaunchKernelGGL(k_tree_read_diag_patch, dim3((e->v.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, e->tv, node_id, out);
    else
        hipLaunchKernelGGL(k_tree_read_diag, dim3((e->v.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, e->tv,
                           node_id, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_state_plane(void* engine, int32_t env_id, const float* mean_for_mask, uint32_t flags, float* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (int rc = check_env(e, env_id)) return rc;
    if (flags & ~IPP_ADAPTIVE) return fail(-1, "unsupported flag bits 0x%x", flags);
    if (!e->scoring) return fail(-1, "ipp_state_plane needs ipp_config.score_scratch = 1");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const View& v = e->v;
    ScoreView sv = e->sv;
    if (v.mode == IPP_DENSE) sv.P = v.cov + (size_t)env_id * v.cov_slot;
    hipLaunchKernelGGL(k_plane_mask, dim3((v.Npad + 255) / 256), dim3(256), 0, s, v, env_id, mean_for_mask, flags, sv.mask, sv.extent);
    if (v.mode == IPP_FACTOR)
        hipLaunchKernelGGL(k_score_densify<false>, dim3(v.Npad / 64, (v.N + 63) / 64), dim3(256), 0, s, v, sv, env_id, ScorePath{}, nullptr, nullptr, 0);
    const int blocks = std::min(v.N, 1024);
    hipLaunchKernelGGL(k_plane_minmax, dim3(blocks), dim3(256), 0, s, v, sv.P, sv.mask, sv.extent);
    hipLaunchKernelGGL(k_plane_write, dim3(blocks), dim3(256), 0, s, v, sv.P, sv.mask, sv.extent, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_feature_planes(void* engine, const ipp_plane_spec* spec, const ipp_plane_entry* entries, int32_t n, const int32_t* mask_env,
                       const float* mask_mean, float* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !spec) return fail(-1, "null argument");
    if (n < 0 || n > (1 << 20)) return fail(-1, "n = %d outside [0, 2^20]", n);
    if (spec->history < 1 || spec->history > 64) return fail(-1, "history = %d outside [1, 64]", spec->history);
    if ((spec->use_fov | spec->use_costs | spec->adaptive | spec->use_flight_time) & ~1) return fail(-1, "spec flags must be 0 or 1");
    if (!spec->use_fov && !(std::isfinite(spec->min_altitude) && std::isfinite(spec->max_altitude) && spec->max_altitude != spec->min_altitude))
        return fail(-1, "position mode needs finite min_altitude != max_altitude");
    const View& v = e->v;
    const bool costs = spec->use_costs && !spec->use_fov;
    if ((spec->use_fov || costs) && v.W != v.H) return fail(-1, "FoV and cost planes need a square grid (cell x_dim * x + y), got %d x %d", v.W, v.H);
    if (costs && spec->use_flight_time && !(v.vmax > 0 && v.amax > 0)) return fail(-1, "flight-time costs need max_v, max_a > 0");
    if (spec->adaptive && !mask_env && !mask_mean) return fail(-1, "adaptive planes need mask_env or mask_mean");
    if (n == 0) return 0;
    if (!entries || !out) return fail(-1, "null argument");
    const size_t mask_bytes = ((size_t)v.N + 15) & ~(size_t)15;
    if (mask_bytes > 64 * 1024) return fail(-1, "grids over 65536 cells are not supported");
    PlaneArgs a{};
    a.entries = entries; a.mask_env = mask_env; a.mask_mean = mask_mean; a.out = out;
    a.n = n; a.H = spec->history; a.cpe = spec->use_fov ? 3 : 5; a.C = a.cpe * a.H + (costs ? 1 : 0);
    a.fov = spec->use_fov; a.costs = costs ? 1 : 0; a.adaptive = spec->adaptive; a.flight = spec->use_flight_time;
    a.dense = v.mode == IPP_DENSE ? 1 : 0;
    a.cache = (size_t)v.N * v.N * 4 + mask_bytes + kPlaneStaticLds <= (size_t)kPlaneLdsBytes ? 1 : 0;  // (no opt-in above 64 KB)
    a.min_alt = spec->min_altitude; a.max_alt = spec->max_altitude;
    const size_t lds = mask_bytes + (a.cache ? (size_t)v.N * v.N * 4 : 0);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_feature_planes, dim3((unsigned)n * (a.H + a.costs)), dim3(256), lds, s, v, e->tv, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_score_actions(void* engine, int32_t env_id, const double* actions, int32_t n, const double* prev_action,
                      uint32_t flags, float* reward, int32_t* status, void* stream) {
    return score_actions_impl(engine, env_id, ScorePath{}, nullptr, actions, n, prev_action, flags, reward, status, stream);
}

// ipp_score_actions_envs (k_score_batch.h): the item lists of the predict-only step launches live in the caller's scratch
int ipp_score_actions_envs_scratch_bytes(void* engine, int32_t n, int32_t k, uint64_t* bytes) {
    Engine* e = as_engine(engine);
    if (!e || !bytes) return fail(-1, "null argument");
    if (n < 0 || k < 0) return fail(-1, "n = %d, k = %d: negative", n, k);
    if (!e->patch) return fail(-1, "ipp_score_actions_envs needs the patch-layout windowed factor engine (ipp_info.patch_layout == 1)");
    *bytes = score_batch_scratch_bytes((uint64_t)n * (uint64_t)k);
    return 0;
}

int ipp_score_actions_envs(void* engine, const int32_t* env_ids, int32_t n, int32_t k, const double* actions,
                           const double* prev_action, uint32_t flags, float* reward, double* cost, int32_t* status,
                           void* scratch, uint64_t scratch_bytes, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !actions || !prev_action || !reward) return fail(-1, "null argument");
    if (!e->patch) return fail(-1, "ipp_score_actions_envs needs the patch-layout windowed factor engine (ipp_info.patch_layout == 1)");
    if (n < 0 || k < 0) return fail(-1, "n = %d, k = %d: negative", n, k);
    if (flags & ~(IPP_COV_ONLY | IPP_PREDICT_ONLY | IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) return fail(-1, "unsupported flag bits 0x%x", flags);
    const uint64_t items = (uint64_t)n * (uint64_t)k;
    const uint64_t need = score_batch_scratch_bytes(items);
    if (items == 0) return 0;
    if (scratch_bytes < need || !scratch)
        return fail(-1, "scratch of %llu bytes, ipp_score_actions_envs needs %llu for n = %d, k = %d", (unsigned long long)scratch_bytes,
                    (unsigned long long)need, n, k);
    if ((items + 255) / 256 > 0x7fffffffull) return fail(-1, "n x k = %llu candidates exceed one call", (unsigned long long)items);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    int* ids = reinterpret_cast<int*>(scratch);
    double* prevx = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(scratch) + score_batch_ids_bytes(items));
    hipLaunchKernelGGL(k_score_expand, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, e->v, env_ids, n, k, actions, prev_action, flags,
                       ids, prevx, cost);
    HIP_TRY(hipGetLastError());
    // one predict-only covariance-only item per candidate, in launches of at most max_batch items: the candidates of an env are
    // consecutive items, so its columns stay in the caches between them
    const uint32_t step_flags = (flags & (IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) | IPP_COV_ONLY | IPP_PREDICT_ONLY;
    const uint64_t mb = (uint64_t)e->v.max_batch;
    for (uint64_t o = 0; o < items; o += mb) {
        const int cnt = (int)std::min<uint64_t>(mb, items - o);
        if (int rc = ipp_step(engine, ids + o, nullptr, cnt, actions + 3 * o, prevx + 3 * o, nullptr, step_flags, reward + o,
                              status ? status + o : nullptr, stream))
            return rc;
    }
    return 0;
}

int ipp_tree_score_actions(void* engine, int32_t root_id, const int32_t* path_ids, const double* actions, int32_t n,
                           const double* prev_action, uint32_t flags, float* reward, int32_t* status, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !path_ids) return fail(-1, "null argument");
    if (e->tv.node_cap <= 0 || e->v.mode != IPP_FACTOR) return fail(-1, "ipp_tree_score_actions needs IPP_FACTOR and node_capacity > 0");
    ScorePath path{};
    for (int j = 0; j < kTreeDepth; ++j) {
        const int id = path_ids[j];
        if (id < 0) continue;
        if (id >= e->tv.node_cap) return fail(-1, "node id %d outside [0, %d)", id, e->tv.node_cap);
        path.ids[path.depth++] = id;
    }
    const float* node_diag = nullptr;
    if (path.depth) {  // the node's diagonal lives on its span only: assemble the whole one along the parent chain
        if (!e->node_diag_scratch) return fail(-1, "ipp_tree_score_actions needs ipp_config.score_scratch = 1");
        HIP_TRY(hipSetDevice(e->device));
        if (e->patch)
            hipLaunchKernelGGL(k_tree_read_diag_patch, dim3((e->v.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, e->tv,
                               path.ids[path.depth - 1], e->node_diag_scratch);
        else
            hipLaunchKernelGGL(k_tree_read_diag, dim3((e->v.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, e->tv,
                               path.ids[path.depth - 1], e->node_diag_scratch);
        node_diag = e->node_diag_scratch;
    }
    return score_actions_impl(engine, root_id, path, node_diag, actions, n, prev_action, flags, reward, status, stream);
}

int ipp_fork(void* engine, const int32_t* src_ids, const int32_t* dst_ids, int32_t n, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !src_ids || !dst_ids) return fail(-1, "null argument");
    if (n <= 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t n4 = e->v.cov_slot / 4;
    int chunks = (int)std::min<uint64_t>(512, (n4 + 1023) / 1024);
    if (chunks < 1) chunks = 1;
    hipLaunchKernelGGL(k_fork, dim3(chunks, n), dim3(256), 0, s, e->v, src_ids, dst_ids, n);
    hipLaunchKernelGGL(k_fork_rank, dim3((n + 255) / 256), dim3(256), 0, s, e->v, src_ids, dst_ids, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int read_row(Engine* e, const float* slab, int env, float* out, void* stream) {
    if (!e || !out) return fail(-1, "null argument");
    if (int rc = check_env(e, env)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, slab + (size_t)env * e->v.Npad, (size_t)e->v.N * 4, hipMemcpyDeviceToDevice,
                           reinterpret_cast<hipStream_t>(stream)));
    return 0;
}
int ipp_read_mean(void* engine, int32_t env_id, float* out, void* stream) { Engine* e = as_engine(engine); return read_row(e, e ? e->v.mean : nullptr, env_id, out, stream); }
int ipp_read_diag(void* engine, int32_t env_id, float* out, void* stream) { Engine* e = as_engine(engine); return read_row(e, e ? e->v.diag : nullptr, env_id, out, stream); }
static int copy_gt(Engine* e, int env, float* out, const float* in, void* stream) {
    if (!e || (!out && !in)) return fail(-1, "null argument");
    if (int rc = check_env(e, env)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_copy_gt, dim3((e->v.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, env, out, in);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ipp_read_gt(void* engine, int32_t env_id, float* out, void* stream) { return copy_gt(as_engine(engine), env_id, out, nullptr, stream); }

int ipp_read_cov_dense(void* engine, int32_t env_id, float* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (int rc = check_env(e, env_id)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const View& v = e->v;
    if (v.mode == IPP_DENSE) {
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)v.N * 4, v.cov + (size_t)env_id * v.cov_slot, (size_t)v.Npad * 4,
                                 (size_t)v.N * 4, v.N, hipMemcpyDeviceToDevice, s));
    } else {
        if (v.patch) hipLaunchKernelGGL(k_read_cov_patch, dim3((v.N + 255) / 256, v.N), dim3(256), 0, s, v, env_id, out);
        else hipLaunchKernelGGL(k_read_cov_factor, dim3((v.N + 255) / 256, v.N), dim3(256), 0, s, v, env_id, out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int ipp_read_rank(void* engine, int32_t env_id, int32_t* rank, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !rank) return fail(-1, "null argument");
    if (int rc = check_env(e, env_id)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(rank, e->v.rank + env_id, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ipp_read_ranks(void* engine, int32_t* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, e->v.rank, (size_t)e->v.cap * 4, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

static int write_row(Engine* e, float* slab, int env, const float* in, void* stream) {
    if (!e || !in) return fail(-1, "null argument");
    if (int rc = check_env(e, env)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(slab + (size_t)env * e->v.Npad, in, (size_t)e->v.N * 4, hipMemcpyDeviceToDevice,
                           reinterpret_cast<hipStream_t>(stream)));
    return 0;
}
int ipp_write_mean(void* engine, int32_t env_id, const float* mean, void* stream) { Engine* e = as_engine(engine); return write_row(e, e ? e->v.mean : nullptr, env_id, mean, stream); }
int ipp_write_gt(void* engine, int32_t env_id, const float* gt, void* stream) { return copy_gt(as_engine(engine), env_id, nullptr, gt, stream); }

int ipp_write_cov_dense(void* engine, int32_t env_id, const float* P, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !P) return fail(-1, "null argument");
    if (int rc = check_env(e, env_id)) return rc;
    const View& v = e->v;
    if (v.mode != IPP_DENSE) return fail(-1, "ipp_write_cov_dense needs an IPP_DENSE engine (a factor state cannot hold an arbitrary P)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy2DAsync(v.cov + (size_t)env_id * v.cov_slot, (size_t)v.Npad * 4, P, (size_t)v.N * 4, (size_t)v.N * 4,
                             v.N, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_dense_fixup, dim3((v.N + 255) / 256), dim3(256), 0, s, v, env_id);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_metrics(void* engine, const int32_t* env_ids, int32_t n, float* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (n <= 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_metrics, dim3(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), e->v, env_ids, n, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_fill_normal(void* engine, float* out, uint64_t count, uint64_t seed, uint64_t subsequence, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t quads = (count + 3) / 4;
    hipLaunchKernelGGL(k_fill_normal, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), out, count, seed, subsequence);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_fill_normal_rows(void* engine, float* out, int32_t planes, int32_t rows, int32_t row_len, const int32_t* row_ids,
                         int64_t row_offset, uint64_t seed, uint64_t subsequence, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (planes < 0 || rows < 0 || row_len <= 0 || planes > 65535) return fail(-1, "bad shape %d x %d x %d", planes, rows, row_len);
    if (planes == 0 || rows == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const long long quads = (long long)rows * ((row_len + 3) / 4);
    hipLaunchKernelGGL(k_fill_normal_rows, dim3((unsigned)((quads + 255) / 256), (unsigned)planes), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), out, planes, rows, row_len, row_ids, (long long)row_offset, seed, subsequence);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_debug_step_item(void* engine, int32_t idx, ipp_step_item* out, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !out) return fail(-1, "null argument");
    if (idx < 0 || idx >= e->last_n) return fail(-1, "item %d outside the last step's batch of %d", idx, e->last_n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    const int MC = e->v.meas_cap;
    ItemHdr h;
    std::vector<double> d((size_t)2 * MC * MC + 2 * MC);
    HIP_TRY(hipMemcpyAsync(&h, e->v.hdr + idx, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(d.data(), e->v.dbg + (size_t)idx * d.size(), d.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->env = h.env; out->dst = h.dst; out->rank_before = h.rank; out->status = h.status;
    out->xl = h.xl; out->xr = h.xr; out->yu = h.yu; out->yd = h.yd;
    out->rf = h.rf; out->m = h.m; out->f = h.f;
    out->cost = h.cost_d;
    out->noise_var = h.nv_d;
    for (int i = 0; i < h.m; ++i)
        for (int j = 0; j < h.m; ++j) {
            out->S[i * h.m + j] = d[(size_t)i * MC + j];
            out->Linv[i * h.m + j] = d[(size_t)MC * MC + i * MC + j];
        }
    for (int i = 0; i < h.m; ++i) {
        out->z[i] = d[(size_t)2 * MC * MC + i];
        out->y[i] = d[(size_t)2 * MC * MC + MC + i];
    }
    return 0;
}

int ipp_streamed_bytes(void* engine, uint64_t* bytes, int32_t reset, void* stream) {
    return ipp_streamed_bytes_detail(engine, bytes, nullptr, reset, stream);
}

int ipp_streamed_bytes_detail(void* engine, uint64_t* bytes, uint64_t* mask_reread_bytes, int32_t reset, void* stream) {
    Engine* e = as_engine(engine);
    if (!e || !bytes) return fail(-1, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    static_assert(kCountSlots * 16 <= 1024, "counter slots");
    unsigned long long cnt[kCountSlots * 16] = {};
    HIP_TRY(hipMemcpyAsync(cnt, e->v.counters, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t units = 0, extra = 0;
    for (int k = 0; k < kCountSlots; ++k) { units += cnt[16 * k]; extra += cnt[16 * k + 8]; }
    {  // patch kernels: per-item totals
        std::vector<unsigned long long> ic((size_t)2 * e->v.max_batch);
        HIP_TRY(hipMemcpyAsync(ic.data(), e->v.item_counts, ic.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t needed = 0;
        for (size_t i = 0; i < ic.size(); i += 2) { units += ic[i]; needed += ic[i + 1]; }
        e->last_needed_bytes = needed * 4;
    }
    *bytes = units * 4;
    if (mask_reread_bytes) *mask_reread_bytes = extra * 4;
#if IPP_PHASE_TIMING
    {
        unsigned long long c[8];
        HIP_TRY(hipMemcpy(c, e->v.counters, 64, hipMemcpyDeviceToHost));
        fprintf(stderr, "[phase timing, 10 ns ticks summed over workgroups] c1 hdr %llu c2 obs %llu c3 gather %llu c4 %llu c5 %llu c6 %llu c7 %llu\n", c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
    }
#endif
#if IPP_TIMELINE
    if (const char* path = getenv("IPP_TIMELINE_FILE")) {
        const size_t n = (size_t)8 * std::min((int)e->v.max_batch, kTimelineItems);
        std::vector<unsigned long long> tl(n);
        HIP_TRY(hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_timeline), n * 8));
        if (FILE* f = fopen(path, "wb")) { fwrite(tl.data(), 8, n, f); fclose(f); }
        std::vector<unsigned long long> ut((size_t)kUnitTraceItems * 2 * 8 * 4);
        HIP_TRY(hipMemcpyFromSymbol(ut.data(), HIP_SYMBOL(g_unit_trace), ut.size() * 8));
        const std::string upath = std::string(path) + ".units";
        if (FILE* f = fopen(upath.c_str(), "wb")) { fwrite(ut.data(), 8, ut.size(), f); fclose(f); }
        std::fill(ut.begin(), ut.end(), 0ull);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_unit_trace), ut.data(), ut.size() * 8));
    }
    {
        unsigned long long wp[16];
        HIP_TRY(hipMemcpyFromSymbol(wp, HIP_SYMBOL(g_wphase), sizeof wp));
        if (wp[10]) {
            const double u = (double)wp[10], w = (double)std::max<unsigned long long>(wp[11], 1);
            fprintf(stderr, "[k_step_patch wave phases, shader clocks] per unit: setup+compaction %.0f  prior term %.0f  stream %.0f  solve wait %.0f  "
                            "epilogue %.0f  stores %.0f | per wave: prologue %.0f  algebra/observation %.0f  results %.0f | units %.0f waves %.0f groups/unit %.2f\n",
                    wp[0] / u, wp[1] / u, wp[2] / u, wp[3] / u, wp[4] / u, wp[5] / u, wp[6] / w, wp[7] / w, wp[8] / w, u, w, wp[9] / u);
        }
        memset(wp, 0, sizeof wp);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wphase), wp, sizeof wp));
    }
#endif
    if (reset) {
        HIP_TRY(hipMemsetAsync(e->v.counters, 0, (size_t)kCountSlots * 128, s));
        HIP_TRY(hipMemsetAsync(e->v.item_counts, 0, (size_t)e->v.max_batch * 16, s));
    }
    return 0;
}

int ipp_probe_stream_pair(void* engine, void* stream_a, void* stream_b, int32_t launches, double* ms) {
    Engine* e = as_engine(engine);
    if (!e || !ms || launches < 1 || launches > 256) return fail(-1, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t a = reinterpret_cast<hipStream_t>(stream_a), b = reinterpret_cast<hipStream_t>(stream_b);
    hipEvent_t e0, ea, eb;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&ea)); HIP_TRY(hipEventCreate(&eb));
    HIP_TRY(hipStreamSynchronize(a)); HIP_TRY(hipStreamSynchronize(b));
    // warm both queues, then a chain of dependent launches on each, issued alternately like the parts of a batched step
    hipLaunchKernelGGL(k_spin, dim3(64), dim3(64), 0, a, 100ull, (int*)nullptr);
    hipLaunchKernelGGL(k_spin, dim3(64), dim3(64), 0, b, 100ull, (int*)nullptr);
    HIP_TRY(hipStreamSynchronize(a)); HIP_TRY(hipStreamSynchronize(b));
    HIP_TRY(hipEventRecord(e0, a));
    HIP_TRY(hipStreamWaitEvent(b, e0, 0));
    for (int i = 0; i < launches; ++i) {
        hipLaunchKernelGGL(k_spin, dim3(256), dim3(64), 0, a, 3000ull, (int*)nullptr);  // 30 us each
        hipLaunchKernelGGL(k_spin, dim3(256), dim3(64), 0, b, 3000ull, (int*)nullptr);
    }
    HIP_TRY(hipEventRecord(ea, a)); HIP_TRY(hipEventRecord(eb, b));
    HIP_TRY(hipEventSynchronize(ea)); HIP_TRY(hipEventSynchronize(eb));
    float ta = 0.f, tb = 0.f;
    HIP_TRY(hipEventElapsedTime(&ta, e0, ea)); HIP_TRY(hipEventElapsedTime(&tb, e0, eb));
    *ms = (double)std::max(ta, tb);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_debug_capture(void* engine, int32_t enable) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
#if IPP_EXIT_POINTS || defined(IPP_ISSUE_TEST)
    e->v.dbg_capture = enable;  // (instruction-count build: enable = 1 + exit point, k_step_patch.h)
#else
    e->v.dbg_capture = enable != 0;
#endif
    return 0;
}

int ipp_streamed_bytes_needed(void* engine, uint64_t* bytes) {
    Engine* e = as_engine(engine);
    if (!e || !bytes) return fail(-1, "null argument");
    *bytes = e->last_needed_bytes;
    return 0;
}

int ipp_profile_enable(void* engine, int32_t enable) {
    Engine* e = as_engine(engine);
    if (!e) return fail(-1, "null engine");
    e->profile = enable != 0;
    return 0;
}

int ipp_profile_read(void* engine, int32_t kind, double* avg_ms, int64_t* launches, int32_t reset) {
    Engine* e = as_engine(engine);
    if (!e || kind < 0 || kind > 2) return fail(-1, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    ProfSlot& p = e->prof[kind];
    prof_drain(e);
    if (avg_ms) *avg_ms = p.launches ? p.total_ms / (double)p.launches : 0.0;
    if (launches) *launches = p.launches;
    if (reset) { p.total_ms = 0.0; p.launches = 0; }
    return 0;
}

int ipp_profile_read_busy(void* engine, int32_t kind, double* busy_ms, int64_t* launches, int32_t reset) {
    Engine* e = as_engine(engine);
    if (!e || kind < 0 || kind > 3) return fail(-1, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    ProfSlot& p = e->prof[kind];
    prof_drain(e);
    if (busy_ms) *busy_ms = p.busy_ms;
    if (launches) *launches = p.busy_launches;
    if (reset) { p.busy_ms = 0.0; p.busy_launches = 0; }
    return 0;
}

}  // extern "C"
