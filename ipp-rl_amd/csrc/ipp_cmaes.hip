// The batched CMA-ES planner's calls (include/ipp_engine.h "Batched CMA-ES"; kernels: csrc/k_cmaes.h).  A translation unit of its own:
// the calls take bare device buffers and need no engine handle; the evaluation between ipp_cma_plan and ipp_cma_objective is the
// caller's ipp_fork and covariance-only ipp_step launches.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/ipp_engine.h"
#include "ipp_host.h"
#include "k_cmaes.h"

using ipp::fail;

namespace {

int bad(const char* fn, const char* why) { return fail(-1, "%s: %s", fn, why); }

static_assert(cma::kCmaMaxDim == IPP_CMA_MAX_DIM && cma::kCmaMaxLam == IPP_CMA_MAX_LAMBDA, "header and kernel limits");

const char* check_shape(int32_t n, int32_t nmax) {
    if (n < 0) return "n < 0";
    if (nmax < 1 || nmax > IPP_CMA_MAX_DIM) return "nmax outside [1, IPP_CMA_MAX_DIM]";
    return nullptr;
}
const char* check_lambda(int32_t lam) { return (lam < 4 || lam > IPP_CMA_MAX_LAMBDA) ? "lam outside [4, IPP_CMA_MAX_LAMBDA]" : nullptr; }

}  // namespace

extern "C" {

int ipp_cma_state_bytes(int32_t nmax, uint64_t* bytes) {
    if (!bytes) return bad("ipp_cma_state_bytes", "null argument");
    if (const char* why = check_shape(0, nmax)) return bad("ipp_cma_state_bytes", why);
    *bytes = (uint64_t)cma::layout(nmax).words * 8;
    return 0;
}

int ipp_cma_init(void* state, int32_t n, int32_t nmax, const int32_t* dims, const double* m0, int32_t device, void* stream) {
    if (const char* why = check_shape(n, nmax)) return bad("ipp_cma_init", why);
    if (!state || !dims || !m0) return bad("ipp_cma_init", "null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(cma::k_cma_init, dim3((unsigned)n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), static_cast<double*>(state), nmax,
                       dims, m0);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_cma_ask(const void* state, int32_t n, int32_t nmax, int32_t lam, const float* normals, const double* scale, double* x, int32_t device,
                void* stream) {
    if (const char* why = check_shape(n, nmax)) return bad("ipp_cma_ask", why);
    if (const char* why = check_lambda(lam)) return bad("ipp_cma_ask", why);
    if (!state || !normals || !scale || !x) return bad("ipp_cma_ask", "null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(cma::k_cma_ask, dim3((unsigned)n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), static_cast<const double*>(state),
                       nmax, lam, normals, scale, x);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_cma_plan(const int32_t* dims, const double* x, const double* prev, const double* budget, int32_t n, int32_t per_env, int32_t nmax,
                 int32_t horizon, double x_hi, double y_hi, double z_lo, double z_hi, int32_t use_flight_time, double max_v, double max_a,
                 double* action, double* prev_action, double* cost, double* path, int32_t* live, int32_t device, void* stream) {
    if (const char* why = check_shape(n, nmax)) return bad("ipp_cma_plan", why);
    if (per_env < 1) return bad("ipp_cma_plan", "per_env < 1");
    if (horizon < 1 || 3 * horizon > nmax) return bad("ipp_cma_plan", "horizon outside [1, nmax / 3]");
    if ((int64_t)n * per_env > INT32_MAX / 4) return bad("ipp_cma_plan", "n * per_env too large");
    if (use_flight_time && !(max_v > 0 && max_a > 0)) return bad("ipp_cma_plan", "flight time needs max_v > 0 and max_a > 0");
    if (!dims || !x || !prev || !budget || !action || !prev_action || !cost || !path || !live) return bad("ipp_cma_plan", "null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    cma::PlanArgs a;
    a.n = n; a.per_env = per_env; a.nmax = nmax; a.horizon = horizon; a.use_flight_time = use_flight_time ? 1 : 0;
    a.x_hi = x_hi; a.y_hi = y_hi; a.z_lo = z_lo; a.z_hi = z_hi; a.vmax = max_v; a.amax = max_a;
    a.dims = dims; a.X = x; a.prev = prev; a.budget = budget;
    a.action = action; a.prev_action = prev_action; a.cost = cost; a.path = path; a.live = live;
    const int nc = n * per_env;
    hipLaunchKernelGGL(cma::k_cma_plan, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_cma_objective(const float* reward, const int32_t* status, const double* cost, const double* path, const int32_t* live,
                      int32_t candidates, int32_t horizon, double* f, int32_t device, void* stream) {
    if (candidates < 0) return bad("ipp_cma_objective", "candidates < 0");
    if (horizon < 1 || 3 * horizon > IPP_CMA_MAX_DIM) return bad("ipp_cma_objective", "horizon outside [1, IPP_CMA_MAX_DIM / 3]");
    if (candidates > INT32_MAX / 4) return bad("ipp_cma_objective", "candidates too large");
    if (!reward || !status || !cost || !path || !live || !f) return bad("ipp_cma_objective", "null argument");
    if (candidates == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(cma::k_cma_objective, dim3((unsigned)((candidates + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       candidates, horizon, reward, status, cost, path, live, f);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_cma_tell(void* state, int32_t n, int32_t nmax, int32_t lam, const float* normals, const double* x, const double* f, const double* scale,
                 int32_t device, void* stream) {
    if (const char* why = check_shape(n, nmax)) return bad("ipp_cma_tell", why);
    if (const char* why = check_lambda(lam)) return bad("ipp_cma_tell", why);
    if (!state || !normals || !x || !f || !scale) return bad("ipp_cma_tell", "null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(cma::k_cma_tell, dim3((unsigned)n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), static_cast<double*>(state), nmax,
                       lam, normals, x, f, scale);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
