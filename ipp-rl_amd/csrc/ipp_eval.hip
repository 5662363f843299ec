// The baseline missions' decisions and the planner-comparison curves (include/ipp_engine.h "Baselines and comparison curves"; kernels:
// csrc/k_baselines.h, csrc/k_curves.h).  A translation unit of its own: the calls take bare device buffers; only ipp_curve_record may
// be given an engine, whose ipp_metrics it then runs in front of its own kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/ipp_engine.h"
#include "ipp_host.h"
#include "k_baselines.h"
#include "k_curves.h"

using ipp::fail;

namespace {

int bad(const char* fn, const char* why) { return fail(-1, "%s: %s", fn, why); }

const char* check_baseline(const ipp_baseline* b) {
    if (!b) return "null descriptor";
    if (b->n < 0) return "n < 0";
    if (b->kind < IPP_BASELINE_LAWNMOWER || b->kind > IPP_BASELINE_RANDOM_CONTINUOUS) return "unknown kind";
    if (!b->prev || !b->budget || !b->episode || !b->cursor || !b->seen_episode || !b->decision || !b->start_budget || !b->action || !b->has)
        return "null argument";
    const bool flight = b->kind == IPP_BASELINE_RANDOM_DISCRETE ? b->adaptive != 0 : b->use_flight_time != 0;
    if (flight && !(b->max_v > 0 && b->max_a > 0)) return "flight time needs max_v > 0 and max_a > 0";
    switch (b->kind) {
        case IPP_BASELINE_LAWNMOWER:
        case IPP_BASELINE_SPIRAL:
            if (b->table_len < 0 || b->table_len > INT32_MAX / 3) return "table_len out of range";
            if (b->table_len > 0 && !b->table) return "null table";
            if (b->kind == IPP_BASELINE_LAWNMOWER && !(b->step_size >= 0)) return "step_size must not be negative";
            break;
        case IPP_BASELINE_RANDOM_DISCRETE:
            if (b->grid_w < 1 || b->grid_w != b->grid_h || b->grid_w > 256) return "square grids of 1 .. 256 cells a side only";
            if (b->n_levels < 1 || b->n_levels > 1024 || !b->levels) return "n_levels outside [1, 1024] or null levels";
            if (!(b->resolution > 0)) return "resolution must be positive";
            break;
        default:
            for (int c = 0; c < 3; ++c)
                if (!(b->high[c] >= b->low[c])) return "box: high < low";
            break;
    }
    return nullptr;
}

}  // namespace

extern "C" {

int ipp_baseline_act(const ipp_baseline* bl, void* stream) {
    if (const char* why = check_baseline(bl)) return bad("ipp_baseline_act", why);
    if (bl->n == 0) return 0;
    HIP_TRY(hipSetDevice(bl->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned n = (unsigned)bl->n;
    if (bl->kind == IPP_BASELINE_RANDOM_DISCRETE)
        hipLaunchKernelGGL(ipp::bl::k_baseline_discrete, dim3(n), dim3(ipp::bl::kDiscreteThreads), 0, st, *bl);
    else if (bl->kind == IPP_BASELINE_RANDOM_CONTINUOUS)
        hipLaunchKernelGGL(ipp::bl::k_baseline_continuous, dim3(n), dim3(64), 0, st, *bl);
    else
        hipLaunchKernelGGL(ipp::bl::k_baseline_table, dim3((n + 255) / 256), dim3(256), 0, st, *bl);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_curve_record(void* engine, float* metrics, const double* action, const double* prev_before, const uint8_t* executed, int32_t n,
                     int32_t first, double max_v, double max_a, double* log, int32_t* count, uint8_t* overflow, int32_t t_cap, int32_t device,
                     void* stream) {
    if (n < 0) return bad("ipp_curve_record", "n < 0");
    if (t_cap < 1 || (int64_t)n * t_cap > INT32_MAX / IPP_CURVE_POINT) return bad("ipp_curve_record", "t_cap < 1 or n * t_cap too large");
    if (!metrics || !log || !count || !overflow) return bad("ipp_curve_record", "null argument");
    if (!first && (!action || !prev_before || !executed)) return bad("ipp_curve_record", "action, prev_before and executed are required unless first");
    if (!first && !(max_v > 0 && max_a > 0)) return bad("ipp_curve_record", "flight time needs max_v > 0 and max_a > 0");
    if (n == 0) return 0;
    if (engine) {
        ipp::TreeEngine te;
        if (int rc = ipp::tree_engine(engine, &te)) return rc;
        if (te.device != device) return bad("ipp_curve_record", "the engine lives on another device");
        if (int rc = ipp_metrics(engine, nullptr, n, metrics, stream)) return rc;
    }
    HIP_TRY(hipSetDevice(device));
    ipp::cv::RecordArgs a;
    a.n = n; a.first = first ? 1 : 0; a.t_cap = t_cap; a.vmax = max_v; a.amax = max_a;
    a.metrics = metrics; a.action = action; a.prev_before = prev_before; a.executed = executed;
    a.log = log; a.count = count; a.overflow = overflow;
    hipLaunchKernelGGL(ipp::cv::k_curve_record, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_curve_extent(const double* log, const int32_t* count, int32_t n, int32_t t_cap, double* max_x_all, int32_t device, void* stream) {
    if (n < 0 || t_cap < 1) return bad("ipp_curve_extent", "n < 0 or t_cap < 1");
    if (!log || !count || !max_x_all) return bad("ipp_curve_extent", "null argument");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(ipp::cv::k_curve_extent, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n, t_cap, log, count, max_x_all);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_curve_resample(const double* log, const int32_t* count, int32_t n, int32_t t_cap, double max_x, int32_t grid, double* out,
                       int32_t device, void* stream) {
    if (n < 0 || t_cap < 1) return bad("ipp_curve_resample", "n < 0 or t_cap < 1");
    if (grid < 1 || (int64_t)n * grid > INT32_MAX / IPP_CURVE_VALUES) return bad("ipp_curve_resample", "grid < 1 or n * grid too large");
    if (!(max_x >= 0) || !std::isfinite(max_x)) return bad("ipp_curve_resample", "max_x must be finite and not negative");
    if (!log || !count || !out) return bad("ipp_curve_resample", "null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    const double step = grid > 1 ? max_x / (double)(grid - 1) : 0.0;  // (np.linspace's step, rounded once on the host)
    hipLaunchKernelGGL(ipp::cv::k_curve_resample, dim3((unsigned)n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t_cap, grid, step,
                       max_x, log, count, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_curve_reduce(const double* per_env, int32_t n, int32_t grid, double* mean, double* sd, int32_t device, void* stream) {
    if (n < 1) return bad("ipp_curve_reduce", "n < 1");
    if (grid < 1 || (int64_t)n * grid > INT32_MAX / IPP_CURVE_VALUES) return bad("ipp_curve_reduce", "grid < 1 or n * grid too large");
    if (!per_env || !mean || !sd) return bad("ipp_curve_reduce", "null argument");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(ipp::cv::k_curve_reduce, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n, grid, per_env,
                       mean, sd);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
