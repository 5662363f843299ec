// The search and self-play calls of the C-ABI (include/ipp_engine.h): device tree search, self-play records and replay ring, deployment
// games, classic MCTS for a batch.  A translation unit of its own, and the only one that includes these kernel headers: most calls take
// bare device tables; the few that take an engine see it through ipp_host.h (TreeEngine, tree_step), not through the step kernels.
#include <algorithm>

#include "ipp_common.h"
#include "ipp_host.h"
#include "k_mcts.h"
#include "k_selfplay.h"
#include "k_replay_per.h"
#include "k_replay_compact.h"
#include "k_learn.h"
#include "k_play.h"
#include "k_rollout.h"
#include "k_ctree.h"

using namespace ipp;

extern "C" {

// ---- device-side tree search (k_mcts.h)
static int mcts_check(const ipp_mcts_tables* t) {
    if (!t) return fail(-1, "null tables");
    if (t->roots <= 0 || t->kmax <= 0 || t->nodes_per_root <= 1 || t->dev_per_root <= 0 || t->wave <= 0 || t->max_depth <= 0)
        return fail(-1, "ipp_mcts_tables: roots, kmax, nodes_per_root, dev_per_root, wave and max_depth must be positive");
    if (t->table_size < 2 * t->nodes_per_root || (t->table_size & (t->table_size - 1)))
        return fail(-1, "ipp_mcts_tables.table_size = %d must be a power of two >= 2 nodes_per_root", t->table_size);
    if (t->max_depth > 8 || t->horizon + 1 > kMctsPath) return fail(-1, "ipp_mcts_tables: horizon %d exceeds the path length %d", t->horizon, kMctsPath - 1);
    if (!t->actions || !t->cell_action || !t->off_x || !t->off_y || !t->zkey || !t->uniform_ps || !t->t_idx || !t->t_ps || !t->t_nsa ||
        !t->t_qsa || !t->t_num || !t->t_child || !t->n_k || !t->n_ns || !t->n_flags || !t->n_hash || !t->n_value || !t->n_devpath ||
        !t->root_count || !t->dev_count || !t->h_keys || !t->h_vals || !t->p_node || !t->p_k || !t->p_cost || !t->p_len || !t->leaf ||
        !t->pend_node || !t->pend_depth || !t->pend_sim || !t->pend_prev || !t->pend_budget || !t->pend_count || !t->rq_root ||
        !t->rq_parent || !t->rq_k || !t->rq_child || !t->rq_newdev || !t->rq_cost || !t->rq_prev || !t->rq_action || !t->rq_count ||
        !t->ts_paths || !t->ts_reward || !t->ts_status || !t->err)
        return fail(-1, "ipp_mcts_tables: null buffer");
    if (t->root_base < 0 || t->dev_base < 0 || t->scratch_base < 0) return fail(-1, "ipp_mcts_tables: root_base, dev_base and scratch_base must be >= 0");
    return 0;
}

int ipp_mcts_select(const ipp_mcts_tables* t, const int32_t* root_env, const double* prev0, const double* budget0, int32_t depth,
                    int32_t sim0, int32_t wave, uint64_t seed, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    if (!root_env || !prev0 || !budget0) return fail(-1, "null argument");
    if (wave <= 0 || wave > t->wave) return fail(-1, "wave = %d outside [1, %d]", wave, t->wave);
    if (depth < 0 || t->horizon + 1 - depth > t->max_depth) return fail(-1, "depth %d: the descents need %d steps, max_depth = %d", depth, t->horizon + 1 - depth, t->max_depth);
    HIP_TRY(hipSetDevice(t->device));
    const int blocks = (t->roots * kWave + 255) / 256;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ne = (t->kmax + 63) / 64;  // edge rows in registers up to 256 valid actions per node
    if (ne == 1)      hipLaunchKernelGGL(k_mcts_select<1>, dim3(blocks), dim3(256), 0, s, *t, root_env, prev0, budget0, (int)depth, (int)sim0, (int)wave, seed);
    else if (ne == 2) hipLaunchKernelGGL(k_mcts_select<2>, dim3(blocks), dim3(256), 0, s, *t, root_env, prev0, budget0, (int)depth, (int)sim0, (int)wave, seed);
    else if (ne == 3) hipLaunchKernelGGL(k_mcts_select<3>, dim3(blocks), dim3(256), 0, s, *t, root_env, prev0, budget0, (int)depth, (int)sim0, (int)wave, seed);
    else if (ne == 4) hipLaunchKernelGGL(k_mcts_select<4>, dim3(blocks), dim3(256), 0, s, *t, root_env, prev0, budget0, (int)depth, (int)sim0, (int)wave, seed);
    else              hipLaunchKernelGGL(k_mcts_select<0>, dim3(blocks), dim3(256), 0, s, *t, root_env, prev0, budget0, (int)depth, (int)sim0, (int)wave, seed);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_mcts_steps(void* engine, const ipp_mcts_tables* t, int32_t first, int32_t n, uint32_t flags, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    TreeEngine e;
    if (int rc = tree_engine(engine, &e)) return rc;
    const int64_t cap = (int64_t)t->max_depth * t->roots * t->wave;
    // n < 0: the request count stays on the device (t->rq_count[0]); the launch is sized for roots x wave items (patch engines:
    // k_tree_patch reads the count) -- a search wave needs no read-back between select and the steps
    const bool dev_count = n < 0;
    if (dev_count && !e.patch) return fail(-1, "n < 0 (device-side count) needs the patch layout");
    if (dev_count && first != 0) return fail(-1, "n < 0 (device-side count) goes with first = 0");
    if (first < 0 || (!dev_count && (int64_t)first + n > cap)) return fail(-1, "requests [%d, %d) outside the list of %lld", first, first + n, (long long)cap);
    if (n == 0) return 0;
    const int n_grid = dev_count ? (int)std::min<int64_t>(e.max_batch, (int64_t)t->roots * t->wave) : n;
    if ((int64_t)t->dev_base + (int64_t)t->roots * t->dev_per_root > e.node_cap)
        return fail(-1, "dev_base + roots x dev_per_root = %lld device nodes exceed ipp_config.node_capacity = %d",
                    (long long)t->dev_base + (long long)t->roots * t->dev_per_root, e.node_cap);
    if (t->scratch_base > 0 && !e.patch) return fail(-1, "ipp_mcts_tables.scratch_base needs the patch layout");
    if ((int64_t)t->scratch_base + n_grid > e.max_batch)
        return fail(-1, "scratch_base + items = %lld exceed ipp_config.max_batch = %d", (long long)t->scratch_base + n_grid, e.max_batch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e.device));
    const size_t o = (size_t)first;
    // (the path arguments ts_paths were written by ipp_mcts_select; the patch kernel writes the edge numerators itself)
    const TreeEdgeOut eo{t->rq_parent + o, t->rq_k + o, t->rq_cost + o, t->t_num, t->err, t->kmax, (int)t->scratch_base};
    if (int rc = tree_step(engine, t->rq_root + o, t->ts_paths + kMctsPath * o, t->rq_newdev + o, n_grid, t->rq_action + 3 * o, t->rq_prev + 3 * o,
                           flags, t->ts_reward + o, t->ts_status + o, stream, dev_count ? t->rq_count : nullptr, e.patch ? &eo : nullptr))
        return rc;
    if (!e.patch) hipLaunchKernelGGL(k_mcts_apply, dim3((n_grid + 255) / 256), dim3(256), 0, s, *t, (int)first, (int)n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_mcts_expand(const ipp_mcts_tables* t, const double* prior, const double* value, double value_const, int32_t sets_only,
                    double alpha, double eps, uint64_t seed, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    if (!(alpha > 0.0) || eps < 0.0 || eps > 1.0) return fail(-1, "Dirichlet alpha must be > 0 and eps in [0, 1]");
    HIP_TRY(hipSetDevice(t->device));
    const int waves = t->roots * t->wave;
    hipLaunchKernelGGL(k_mcts_expand, dim3((waves * kWave + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *t, prior, value,
                       value_const, (int)sets_only, alpha, eps, seed);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_mcts_backup(const ipp_mcts_tables* t, int32_t wave, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    if (wave <= 0 || wave > t->wave) return fail(-1, "wave = %d outside [1, %d]", wave, t->wave);
    HIP_TRY(hipSetDevice(t->device));
    if (t->wave * t->max_depth <= kWave)  // one wave per root, one lane per recorded step
        hipLaunchKernelGGL(k_mcts_backup, dim3(t->roots), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *t, (int)wave);
    else
        hipLaunchKernelGGL(k_mcts_backup_serial, dim3((std::max(t->roots, t->max_depth) + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), *t, (int)wave);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_mcts_policy(const ipp_mcts_tables* t, const double* tie_uniform, double temperature, int32_t deploy_time, double* policy,
                    int32_t* valid_idx, int32_t* ok, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    if (!policy || !ok) return fail(-1, "null argument");
    if (!(temperature > 0)) return fail(-1, "temperature = %g: the read-out on the device is the one for temperature > 0 (mcts.py:133-143)", temperature);
    HIP_TRY(hipSetDevice(t->device));
    hipLaunchKernelGGL(k_mcts_policy, dim3((t->roots * kWave + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *t, tie_uniform,
                       1.0 / temperature, (int)(deploy_time != 0), policy, valid_idx, ok);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_mcts_plane_entries(const ipp_mcts_tables* t, const int32_t* root_env, const double* prev0, const double* budget0,
                           const ipp_plane_entry* root_history, int32_t history, double initial_budget, int32_t sim0, ipp_plane_entry* out,
                           int32_t* mask_env, void* stream) {
    if (int rc = mcts_check(t)) return rc;
    if (!root_env || !prev0 || !budget0 || !out) return fail(-1, "null argument");
    if (history < 1 || history > 64) return fail(-1, "history = %d outside [1, 64]", history);
    if (!(initial_budget > 0.0)) return fail(-1, "initial_budget must be > 0");
    HIP_TRY(hipSetDevice(t->device));
    const int n = t->roots * t->wave;
    hipLaunchKernelGGL(k_mcts_plane_entries, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *t, root_env, prev0,
                       budget0, root_history, (int)history, initial_budget, (int)sim0, out, mask_env);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int selfplay_check(const ipp_selfplay* sp) {
    if (!sp) return fail(-1, "null argument");
    if (sp->num_envs <= 0 || sp->slots <= 0 || (long long)sp->num_envs * sp->slots > INT32_MAX)
        return fail(-1, "num_envs = %d, slots = %d: need both > 0 and a ring of < 2^31 rows", sp->num_envs, sp->slots);
    if (sp->kmax <= 0 || sp->kmax > kSpMaxK) return fail(-1, "kmax = %d outside [1, %d]", sp->kmax, kSpMaxK);
    if (sp->num_actions <= 0 || sp->horizon < 0) return fail(-1, "num_actions = %d, horizon = %d", sp->num_actions, sp->horizon);
    if (!sp->actions || !sp->budget || !sp->depth || !sp->episode || !sp->done || !sp->prev || !sp->reward || !sp->ep_len || !sp->forced ||
        !sp->tie_u || !sp->episode_value || !sp->action || !sp->action_idx || !sp->r_policy || !sp->r_idx || !sp->r_value || !sp->r_reward ||
        !sp->r_flags)
        return fail(-1, "ipp_selfplay: null device pointer");
    return 0;
}

int ipp_selfplay_record(const ipp_selfplay* sp, int64_t step, const double* policy_t, const double* policy_1, const int32_t* valid_idx,
                        const int32_t* ok, void* stream) {
    if (int rc = selfplay_check(sp)) return rc;
    if (step < 0) return fail(-1, "step = %lld < 0", (long long)step);
    if (!policy_t || !policy_1 || !valid_idx || !ok) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    const size_t lds = (size_t)sp->kmax * (sizeof(double) + sizeof(int32_t));
    hipLaunchKernelGGL(k_sp_record, dim3(sp->num_envs), dim3(kWave), lds, reinterpret_cast<hipStream_t>(stream), *sp, (long long)step, policy_t,
                       policy_1, valid_idx, ok);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_selfplay_commit(const ipp_selfplay* sp, int64_t step, void* stream) {
    if (int rc = selfplay_check(sp)) return rc;
    if (step < 0) return fail(-1, "step = %lld < 0", (long long)step);
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_sp_commit, dim3(sp->num_envs), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *sp, (long long)step);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_gather(const ipp_selfplay* sp, int32_t n, int32_t copies, int32_t channels, int32_t side, const float* planes,
                      const int32_t* committed_cum, uint64_t seed, uint64_t subsequence, float* states, float* policy, uint8_t* mask,
                      double* value, double* reward, int64_t* index, int32_t* offsets, void* stream) {
    if (int rc = selfplay_check(sp)) return rc;
    if (n < 1 || copies < 1 || channels < 0) return fail(-1, "n = %d, copies = %d, channels = %d", n, copies, channels);
    if (channels > 0 && (side < 1 || !planes || !states)) return fail(-1, "planes need side >= 1 and the planes / states buffers");
    if (!committed_cum || !policy || !mask || !value || !reward || !index || !offsets) return fail(-1, "null argument");
    const long long blocks = (long long)n * copies * (channels + 1);
    if (blocks > INT32_MAX) return fail(-1, "%lld blocks: minibatch too large", blocks);
    SpGather g{};
    g.n = n; g.copies = copies; g.C = channels; g.side = side; g.A = sp->num_actions; g.kmax = sp->kmax;
    g.cap = (long long)sp->num_envs * sp->slots;
    g.cum = committed_cum; g.planes = planes; g.seed = seed; g.subseq = subsequence;
    g.states = states; g.policy = policy; g.mask = mask; g.value = value; g.reward = reward; g.index = index; g.offsets = offsets;
    HIP_TRY(hipSetDevice(sp->device));
    const size_t lds = (size_t)sp->kmax * (sizeof(float) + sizeof(int32_t));
    hipLaunchKernelGGL(k_sp_gather, dim3((unsigned)blocks), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), *sp, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the prioritised sampler's calls read the ring's size and flags only
static int replay_ring_check(const ipp_selfplay* sp) {
    if (!sp) return fail(-1, "null argument");
    if (sp->num_envs <= 0 || sp->slots <= 0 || (long long)sp->num_envs * sp->slots > INT32_MAX)
        return fail(-1, "num_envs = %d, slots = %d: need both > 0 and a ring of < 2^31 rows", sp->num_envs, sp->slots);
    if (!sp->r_flags) return fail(-1, "ipp_selfplay: null r_flags");
    return 0;
}

int ipp_replay_priority_reset(const ipp_selfplay* sp, double* priority, uint64_t* count, void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (!priority || !count) return fail(-1, "null argument");
    const long long cap = (long long)sp->num_envs * sp->slots;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint64_t), s));
    const unsigned blocks = (unsigned)((cap + kPerThreads - 1) / kPerThreads);
    hipLaunchKernelGGL(k_per_count, dim3(blocks), dim3(kPerThreads), 0, s, sp->r_flags, cap, reinterpret_cast<unsigned long long*>(count));
    hipLaunchKernelGGL(k_per_reset, dim3(blocks), dim3(kPerThreads), 0, s, sp->r_flags, cap,
                       reinterpret_cast<const unsigned long long*>(count), priority);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_mass(const ipp_selfplay* sp, const double* priority, double alpha, double* cum, double* scratch, uint64_t scratch_doubles,
                    void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (!priority || !cum || !scratch) return fail(-1, "null argument");
    if (!(alpha >= 0.0) || !(alpha < INFINITY)) return fail(-1, "alpha = %g outside [0, inf)", alpha);
    const long long cap = (long long)sp->num_envs * sp->slots;
    const long long tiles = (cap + IPP_REPLAY_SCAN_TILE - 1) / IPP_REPLAY_SCAN_TILE;
    if (scratch_doubles < (uint64_t)tiles)
        return fail(-1, "scratch of %llu doubles, ipp_replay_mass needs %lld for %lld rows", (unsigned long long)scratch_doubles, tiles, cap);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_per_mass_tile, dim3((unsigned)tiles), dim3(kPerThreads), 0, s, sp->r_flags, priority, cap, alpha, cum, scratch);
    hipLaunchKernelGGL(k_per_scan_tiles, dim3(1), dim3(kPerThreads), 0, s, scratch, tiles);
    hipLaunchKernelGGL(k_per_scan_rows, dim3((unsigned)tiles), dim3(kPerThreads), 0, s, cap, scratch, cum);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_draw_per(const ipp_selfplay* sp, const double* priority, const double* cum, double alpha, double beta,
                        int64_t committed_count, int32_t n, uint64_t seed, uint64_t subsequence, int64_t* index, float* weight, void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (!priority || !cum || !index || !weight) return fail(-1, "null argument");
    if (n < 1 || committed_count < 1) return fail(-1, "n = %d, committed_count = %lld: need both >= 1", n, (long long)committed_count);
    if (!(alpha >= 0.0) || !(alpha < INFINITY) || !(beta >= 0.0) || !(beta < INFINITY))
        return fail(-1, "alpha = %g, beta = %g outside [0, inf)", alpha, beta);
    PerDraw d{};
    d.n = n; d.cap = (long long)sp->num_envs * sp->slots; d.priority = priority; d.cum = cum;
    d.alpha = alpha; d.beta = beta; d.L = (double)committed_count; d.seed = seed; d.subseq = subsequence;
    d.index = index; d.weight = weight;
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_per_draw, dim3(1), dim3(kPerThreads), 0, reinterpret_cast<hipStream_t>(stream), *sp, d);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_gather_rows(const ipp_selfplay* sp, int32_t n, int32_t channels, int32_t side, const float* planes, const int64_t* rows,
                           float* states, float* policy, uint8_t* mask, double* value, double* reward, void* stream) {
    if (int rc = selfplay_check(sp)) return rc;
    if (n < 1 || channels < 0) return fail(-1, "n = %d, channels = %d", n, channels);
    if (channels > 0 && (side < 1 || !planes || !states)) return fail(-1, "planes need side >= 1 and the planes / states buffers");
    if (!rows || !policy || !mask || !value || !reward) return fail(-1, "null argument");
    const long long blocks = (long long)n * (channels + 1);
    if (blocks > INT32_MAX) return fail(-1, "%lld blocks: minibatch too large", blocks);
    SpGather g{};
    g.n = n; g.copies = 1; g.C = channels; g.side = side; g.A = sp->num_actions; g.kmax = sp->kmax;
    g.cap = (long long)sp->num_envs * sp->slots;
    g.planes = planes; g.states = states; g.policy = policy; g.mask = mask; g.value = value; g.reward = reward;
    HIP_TRY(hipSetDevice(sp->device));
    const size_t lds = (size_t)sp->kmax * (sizeof(float) + sizeof(int32_t));
    hipLaunchKernelGGL(k_sp_gather_rows, dim3((unsigned)blocks), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), *sp, g, rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_priority_update(const ipp_selfplay* sp, double* priority, const int64_t* index, const double* value, int32_t n,
                               void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (n < 0) return fail(-1, "n = %d < 0", n);
    if (n == 0) return 0;
    if (!priority || !index || !value) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_per_update, dim3((unsigned)((n + kPerThreads - 1) / kPerThreads)), dim3(kPerThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), (long long)sp->num_envs * sp->slots, (int)n, index, value, priority);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- self-play iterations and the off-policy window (k_sp_commit_iter in k_selfplay.h, k_learn.h)
static int selfplay_iter_check(const ipp_selfplay_iter* it) {
    if (!it) return fail(-1, "null argument");
    if (it->episode_cap < 1) return fail(-1, "ipp_selfplay_iter: episode_cap = %d < 1", it->episode_cap);
    if (!it->iter_episodes || !it->r_iter || !it->examples || !it->value_sum) return fail(-1, "ipp_selfplay_iter: null device pointer");
    return 0;
}

int ipp_selfplay_commit_iter(const ipp_selfplay* sp, int64_t step, const ipp_selfplay_iter* it, void* stream) {
    if (int rc = selfplay_check(sp)) return rc;
    if (int rc = selfplay_iter_check(it)) return rc;
    if (step < 0) return fail(-1, "step = %lld < 0", (long long)step);
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_sp_commit_iter, dim3(sp->num_envs), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *sp, (long long)step, *it);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_selfplay_iter_totals(const ipp_selfplay* sp, const ipp_selfplay_iter* it, void* out, void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (int rc = selfplay_iter_check(it)) return rc;
    if (!out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_sp_iter_totals, dim3(1), dim3(kPerThreads), 0, reinterpret_cast<hipStream_t>(stream), (int)sp->num_envs, *it,
                       reinterpret_cast<IterTotals*>(out));
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_priority_reset_window(const ipp_selfplay* sp, const int32_t* r_iter, int32_t lo, int32_t hi, double* priority,
                                     uint64_t* count, void* stream) {
    if (int rc = replay_ring_check(sp)) return rc;
    if (!r_iter || !priority || !count) return fail(-1, "null argument");
    if (lo > hi) return fail(-1, "window [%d, %d]: lo > hi", lo, hi);
    const long long cap = (long long)sp->num_envs * sp->slots;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint64_t), s));
    const unsigned blocks = (unsigned)((cap + kPerThreads - 1) / kPerThreads);
    hipLaunchKernelGGL(k_per_count_win, dim3(blocks), dim3(kPerThreads), 0, s, sp->r_flags, r_iter, (int)lo, (int)hi, cap,
                       reinterpret_cast<unsigned long long*>(count));
    hipLaunchKernelGGL(k_per_reset_win, dim3(blocks), dim3(kPerThreads), 0, s, sp->r_flags, r_iter, (int)lo, (int)hi, cap,
                       reinterpret_cast<const unsigned long long*>(count), priority);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the compact replay ring (k_replay_compact.h)
static int replay_compact_check(void* engine, const ipp_selfplay* sp, const ipp_replay_compact* rc, FactorSlots* fs) {
    if (int err = selfplay_check(sp)) return err;
    if (!rc) return fail(-1, "null argument");
    if (rc->history < 1 || rc->history > 64) return fail(-1, "ipp_replay_compact: history = %d outside [1, 64]", rc->history);
    if (rc->archive_episodes < 1) return fail(-1, "ipp_replay_compact: archive_episodes = %d < 1", rc->archive_episodes);
    if (!rc->r_entries || !rc->r_mean || !rc->r_episode || !rc->episodes || !rc->last_rank || !rc->evicted)
        return fail(-1, "ipp_replay_compact: null device pointer");
    if (int err = factor_slots(engine, fs)) return err;
    if (!fs->patch) return fail(-1, "the compact replay ring needs the patch-layout windowed factor engine (ipp_info.patch_layout == 1)");
    const long long need = (long long)sp->num_envs * (1 + (long long)rc->archive_episodes);
    if (need > fs->cap)
        return fail(-1, "the compact replay ring needs num_envs (1 + archive_episodes) = %lld engine slots, the engine has %d", need, fs->cap);
    if (fs->device != sp->device) return fail(-1, "engine on device %d, ipp_selfplay on device %d", fs->device, sp->device);
    return 0;
}

int ipp_replay_record_compact(void* engine, const ipp_selfplay* sp, const ipp_replay_compact* rc, int64_t step,
                              const ipp_plane_entry* entries, void* stream) {
    FactorSlots fs;
    if (int err = replay_compact_check(engine, sp, rc, &fs)) return err;
    if (step < 0) return fail(-1, "step = %lld < 0", (long long)step);
    if (!entries) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_rc_record, dim3(sp->num_envs), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *sp, *rc, fs, (long long)step,
                       entries);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_selfplay_archive(void* engine, const ipp_selfplay* sp, const ipp_replay_compact* rc, void* stream) {
    FactorSlots fs;
    if (int err = replay_compact_check(engine, sp, rc, &fs)) return err;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(sp->device));
    // (chunks of a slot's columns as in ipp_fork: 1024 float4 per workgroup and pass, at most 64 workgroups per env)
    const uint64_t n4 = (uint64_t)fs.rank_cap * (uint64_t)fs.pstride / 4;
    const int chunks = (int)std::max<uint64_t>(1, std::min<uint64_t>(64, (n4 + 1023) / 1024));
    hipLaunchKernelGGL(k_rc_archive, dim3(chunks, sp->num_envs), dim3(256), 0, s, *sp, *rc, fs);
    hipLaunchKernelGGL(k_rc_evict, dim3(sp->num_envs), dim3(kWave), 0, s, *sp, *rc);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_replay_compact_planes(void* engine, const ipp_selfplay* sp, const ipp_replay_compact* rc, const ipp_plane_spec* spec, int32_t n,
                              int32_t copies, const int64_t* index, const int32_t* offsets, ipp_plane_entry* ent_scratch,
                              float* mean_scratch, float* states, void* stream) {
    FactorSlots fs;
    if (int err = replay_compact_check(engine, sp, rc, &fs)) return err;
    if (!spec || !index || !ent_scratch || !mean_scratch || !states) return fail(-1, "null argument");
    if (spec->history != rc->history) return fail(-1, "spec.history = %d, ipp_replay_compact.history = %d", spec->history, rc->history);
    if (n < 1 || copies < 1) return fail(-1, "n = %d, copies = %d: need both >= 1", n, copies);
    if (copies > 1 && !offsets) return fail(-1, "augmented copies need ipp_replay_gather's offsets");
    const int C = (spec->use_fov ? 3 : 5) * spec->history + ((spec->use_costs && !spec->use_fov) ? 1 : 0);
    const long long blocks = (long long)n * (copies - 1) * C;
    if (blocks > INT32_MAX) return fail(-1, "%lld blocks: minibatch too large", blocks);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(sp->device));
    hipLaunchKernelGGL(k_rc_entries, dim3(n), dim3(256), 0, s, *rc, (long long)sp->num_envs * sp->slots, fs.N, (int)n, index, ent_scratch,
                       mean_scratch);
    HIP_TRY(hipGetLastError());
    if (int err = ipp_feature_planes(engine, spec, ent_scratch, n, nullptr, mean_scratch, states, stream)) return err;
    if (copies > 1) {
        SpGather g{};
        g.n = n; g.copies = copies; g.C = C; g.side = fs.N; g.planes = states; g.states = states;
        hipLaunchKernelGGL(k_rc_crop, dim3((unsigned)blocks), dim3(256), 0, s, g, offsets);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

static int play_check(const ipp_play* pl) {
    if (!pl) return fail(-1, "null argument");
    if (pl->num_envs <= 0) return fail(-1, "ipp_play: num_envs = %d, need > 0", pl->num_envs);
    if (pl->workers < 1 || (long long)pl->num_envs * pl->workers > INT32_MAX)
        return fail(-1, "ipp_play: workers = %d, need >= 1 and num_envs x workers < 2^31", pl->workers);
    if (pl->kmax < 1 || pl->kmax > kSpMaxK) return fail(-1, "ipp_play: kmax = %d outside [1, %d]", pl->kmax, kSpMaxK);
    if (pl->num_actions <= 0) return fail(-1, "ipp_play: num_actions = %d", pl->num_actions);
    if (pl->games_per_env < 1 || (long long)pl->num_envs * pl->games_per_env > INT32_MAX)
        return fail(-1, "ipp_play: games_per_env = %d, need >= 1 and num_envs x games_per_env < 2^31", pl->games_per_env);
    if (pl->tie_rule != 0 && pl->tie_rule != 1) return fail(-1, "ipp_play: tie_rule = %d, need 0 (deploy) or 1 (arena)", pl->tie_rule);
    if (!pl->actions || !pl->budget || !pl->depth || !pl->episode || !pl->done || !pl->prev || !pl->reward || !pl->ret || !pl->steps ||
        !pl->games || !pl->forced || !pl->tie_u || !pl->action || !pl->action_idx || !pl->game_value || !pl->game_steps)
        return fail(-1, "ipp_play: null device pointer");
    return 0;
}

int ipp_play_pick(const ipp_play* pl, const double* policy, const int32_t* valid_idx, const int32_t* ok, void* stream) {
    if (int rc = play_check(pl)) return rc;
    if (!policy || !valid_idx || !ok) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(pl->device));
    const size_t lds = (size_t)pl->kmax * (sizeof(double) + sizeof(int32_t));
    hipLaunchKernelGGL(k_play_pick, dim3(pl->num_envs), dim3(kWave), lds, reinterpret_cast<hipStream_t>(stream), *pl, policy, valid_idx, ok);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_play_tally(const ipp_play* pl, void* stream) {
    if (int rc = play_check(pl)) return rc;
    HIP_TRY(hipSetDevice(pl->device));
    hipLaunchKernelGGL(k_play_tally, dim3(pl->num_envs), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *pl);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_play_totals(const ipp_play* pl, double* out, void* stream) {
    if (int rc = play_check(pl)) return rc;
    if (!out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(pl->device));
    hipLaunchKernelGGL(k_play_totals, dim3(1), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *pl, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- classic MCTS for a batch (k_rollout.h): candidate scoring from many tree nodes, the rollout policy on the device
static int nodes_engine(void* engine, TreeEngine* e) {  // the engine these calls step tree nodes on
    if (int rc = tree_engine(engine, e)) return rc;
    if (e->tree_ok && e->node_cap > 0) return 0;
    return fail(-1, "ipp_tree_score_nodes and ipp_rollout_run need an engine ipp_tree_step runs on: IPP_FACTOR with window_rows > 0, the default tile_threads and node_capacity > 0");
}

// one tree step per item (predict-only, or recorded as node new_ids[i]) in launches of at most max_batch items; new_ids and status may be NULL
static int tree_step_chunks(void* engine, uint64_t max_batch, const int32_t* root_ids, const int32_t* path_ids, const int32_t* new_ids,
                            uint64_t n, const double* action, const double* prev_action, uint32_t flags, float* reward, int32_t* status,
                            void* stream) {
    for (uint64_t o = 0; o < n; o += max_batch) {
        const int cnt = (int)std::min<uint64_t>(max_batch, n - o);
        if (int rc = tree_step(engine, root_ids + o, path_ids + kTreeDepth * o, new_ids ? new_ids + o : nullptr, cnt, action + 3 * o,
                               prev_action + 3 * o, flags, reward + o, status ? status + o : nullptr, stream, nullptr, nullptr))
            return rc;
    }
    return 0;
}

int ipp_tree_score_nodes_scratch_bytes(void* engine, int32_t n, int32_t k, uint64_t* bytes) {
    if (!engine || !bytes) return fail(-1, "null argument");
    if (n < 0 || k < 0) return fail(-1, "n = %d, k = %d: negative", n, k);
    TreeEngine e;
    if (int rc = nodes_engine(engine, &e)) return rc;
    *bytes = nodes_scratch_bytes((uint64_t)n * (uint64_t)k);
    return 0;
}

int ipp_tree_score_nodes(void* engine, const int32_t* root_ids, const int32_t* path_ids, int32_t n, int32_t k, const double* actions,
                         const double* prev_action, uint32_t flags, float* reward, double* cost, int32_t* status, void* scratch,
                         uint64_t scratch_bytes, void* stream) {
    if (!engine || !root_ids || !path_ids || !actions || !prev_action || !reward) return fail(-1, "null argument");
    TreeEngine e;
    if (int rc = nodes_engine(engine, &e)) return rc;
    if (n < 0 || k < 0) return fail(-1, "n = %d, k = %d: negative", n, k);
    if (flags & ~(IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) return fail(-1, "unsupported flag bits 0x%x", flags);
    const uint64_t items = (uint64_t)n * (uint64_t)k;
    const uint64_t need = nodes_scratch_bytes(items);
    if (items == 0) return 0;
    if (scratch_bytes < need || !scratch)
        return fail(-1, "scratch of %llu bytes, ipp_tree_score_nodes needs %llu for n = %d, k = %d", (unsigned long long)scratch_bytes,
                    (unsigned long long)need, n, k);
    if ((items + 255) / 256 > 0x7fffffffull) return fail(-1, "n x k = %llu candidates exceed one call", (unsigned long long)items);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e.device));
    unsigned char* base = reinterpret_cast<unsigned char*>(scratch);
    int* roots = reinterpret_cast<int*>(base);
    int* paths = reinterpret_cast<int*>(base + nodes_scratch_align(items * 4));
    double* prevx = reinterpret_cast<double*>(base + nodes_scratch_align(items * 4) + nodes_scratch_align(items * 4 * kTreeDepth));
    hipLaunchKernelGGL(k_nodes_expand, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, n, k, root_ids, path_ids, actions, prev_action,
                       flags, e.vmax, e.amax, roots, paths, prevx, cost);
    HIP_TRY(hipGetLastError());
    // one predict-only item per candidate, in launches of at most max_batch items: the candidates of a node are consecutive items
    const uint32_t step_flags = (flags & (IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) | IPP_PREDICT_ONLY;
    return tree_step_chunks(engine, e.max_batch, roots, paths, nullptr, items, actions, prevx, step_flags, reward, status, stream);
}

static int rollout_check(const ipp_rollout* ro) {
    if (!ro) return fail(-1, "null rollout");
    if (ro->n <= 0 || ro->kmax <= 0 || ro->max_depth <= 0 || ro->n_levels <= 0 || ro->half < 0 || ro->grid_w <= 0 || ro->grid_h <= 0)
        return fail(-1, "ipp_rollout: n, kmax, max_depth, n_levels, grid_w and grid_h must be positive, half >= 0");
    if ((int64_t)(2 * ro->half + 1) * (2 * ro->half + 1) * ro->n_levels != (int64_t)ro->kmax)
        return fail(-1, "ipp_rollout.kmax = %d is not (2 half + 1)^2 n_levels = (2 x %d + 1)^2 x %d", ro->kmax, ro->half, ro->n_levels);
    if (ro->max_depth > kTreeDepth) return fail(-1, "ipp_rollout.max_depth = %d exceeds IPP_TREE_DEPTH", ro->max_depth);
    if ((int64_t)ro->n * ro->max_depth > 0x7fffffffll - (int64_t)std::max(ro->node_base, 0) || ro->node_base < 0)
        return fail(-1, "ipp_rollout.node_base = %d with n max_depth = %lld node ids", ro->node_base, (long long)ro->n * ro->max_depth);
    if (ro->gcb != 0 && ro->gcb != 1) return fail(-1, "ipp_rollout.gcb = %d is neither 0 nor 1", ro->gcb);
    if ((size_t)ro->kmax * sizeof(double) > 48 * 1024) return fail(-1, "ipp_rollout.kmax = %d exceeds the pick kernel's LDS row", ro->kmax);
    if (!ro->levels || !ro->u || !ro->root || !ro->path || !ro->plen || !ro->cur || !ro->charge_from || !ro->budget || !ro->depth_left ||
        !ro->value || !ro->disc || !ro->live || !ro->flag || !ro->cand || !ro->reward || !ro->cost || !ro->status || !ro->action ||
        !ro->new_id || !ro->step_reward || !ro->step_status || !ro->pick_idx)
        return fail(-1, "ipp_rollout: null buffer");
    return 0;
}

int ipp_rollout_candidates(const ipp_rollout* ro, void* stream) {
    if (int rc = rollout_check(ro)) return rc;
    HIP_TRY(hipSetDevice(ro->device));
    const uint64_t items = (uint64_t)ro->n * (uint64_t)ro->kmax;
    hipLaunchKernelGGL(k_rollout_candidates, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *ro);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_rollout_pick(const ipp_rollout* ro, int32_t level, void* stream) {
    if (int rc = rollout_check(ro)) return rc;
    if (level < 0 || level >= ro->max_depth) return fail(-1, "level = %d outside [0, max_depth = %d)", level, ro->max_depth);
    HIP_TRY(hipSetDevice(ro->device));
    hipLaunchKernelGGL(k_rollout_pick, dim3(ro->n), dim3(kWave), (size_t)ro->kmax * sizeof(double), reinterpret_cast<hipStream_t>(stream), *ro,
                       level);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_rollout_advance(const ipp_rollout* ro, void* stream) {
    if (int rc = rollout_check(ro)) return rc;
    HIP_TRY(hipSetDevice(ro->device));
    hipLaunchKernelGGL(k_rollout_advance, dim3((ro->n + kWave - 1) / kWave), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *ro);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_rollout_run(void* engine, const ipp_rollout* ro, void* scratch, uint64_t scratch_bytes, void* stream) {
    if (!engine) return fail(-1, "null engine");
    if (int rc = rollout_check(ro)) return rc;
    TreeEngine e;
    if (int rc = nodes_engine(engine, &e)) return rc;
    if ((int64_t)ro->node_base + (int64_t)ro->n * ro->max_depth > (int64_t)e.node_cap)
        return fail(-1, "rollout nodes [%d, %lld) exceed node_capacity = %d", ro->node_base, (long long)ro->node_base + (long long)ro->n * ro->max_depth,
                    e.node_cap);
    if (ro->device != e.device) return fail(-1, "ipp_rollout.device = %d, the engine runs on %d", ro->device, e.device);
    if (ro->flags & ~(uint32_t)(IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME)) return fail(-1, "unsupported flag bits 0x%x", ro->flags);
    for (int l = 0; l < ro->max_depth; ++l) {
        if (int rc = ipp_rollout_candidates(ro, stream)) return rc;
        if (int rc = ipp_tree_score_nodes(engine, ro->root, ro->path, ro->n, ro->kmax, ro->cand, ro->cur, ro->flags, ro->reward, ro->cost, ro->status,
                                          scratch, scratch_bytes, stream))
            return rc;
        if (int rc = ipp_rollout_pick(ro, l, stream)) return rc;
        if (int rc = tree_step_chunks(engine, e.max_batch, ro->root, ro->path, ro->new_id, ro->n, ro->action, ro->cur, ro->flags, ro->step_reward,
                                      ro->step_status, stream))  // the recorded step of every rollout (a NaN action: nothing is applied)
            return rc;
        if (int rc = ipp_rollout_advance(ro, stream)) return rc;
    }
    return 0;
}

// ---- classic MCTS for a batch, the tree on the device (k_ctree.h)
static int ctree_check(const ipp_ctree* ct) {
    if (!ct) return fail(-1, "null ipp_ctree");
    if (ct->roots <= 0 || ct->cap <= 0 || ct->thr_len <= 0) return fail(-1, "ipp_ctree: roots, cap and thr_len must be positive");
    if (ct->horizon < 1 || ct->horizon > kTreeDepth) return fail(-1, "ipp_ctree.horizon = %d outside [1, IPP_TREE_DEPTH]", ct->horizon);
    if ((int64_t)ct->roots * ct->cap > 0x7fffffffll) return fail(-1, "ipp_ctree: roots x cap = %lld slots exceed one table", (long long)ct->roots * ct->cap);
    if (ct->tree_node_base < 0) return fail(-1, "ipp_ctree.tree_node_base = %d", ct->tree_node_base);
    if (!ct->thr || !ct->root_slot || !ct->root_wp || !ct->root_budget || !ct->tie_u || !ct->parent || !ct->dev || !ct->plen || !ct->path ||
        !ct->action || !ct->visits || !ct->value_sum || !ct->edge_reward || !ct->count || !ct->err || !ct->t_len || !ct->t_slot ||
        !ct->leaf_kind || !ct->leaf_budget || !ct->leaf_depth)
        return fail(-1, "ipp_ctree: null buffer");
    return 0;
}

// a state that travels with the tables: one row per root on the tables' device
static int ctree_state_check(const ipp_ctree* ct, const ipp_rollout* st, const char* name) {
    if (int rc = rollout_check(st)) return rc;
    if (st->n != ct->roots) return fail(-1, "ipp_ctree: %s.n = %d, the tables hold %d roots", name, st->n, ct->roots);
    if (st->device != ct->device) return fail(-1, "ipp_ctree: %s.device = %d, the tables' is %d", name, st->device, ct->device);
    return 0;
}

static int ctree_states_check(const ipp_ctree* ct, const ipp_rollout* expand, const ipp_rollout* rollout) {
    if (int rc = ctree_check(ct)) return rc;
    if (int rc = ctree_state_check(ct, expand, "expand")) return rc;
    if (int rc = ctree_state_check(ct, rollout, "rollout")) return rc;
    if (expand->max_depth != 1 || expand->gcb != 0) return fail(-1, "ipp_ctree: the expansion state needs max_depth = 1 and gcb = 0");
    if (rollout->max_depth != ct->horizon) return fail(-1, "ipp_ctree: rollout.max_depth = %d, horizon = %d", rollout->max_depth, ct->horizon);
    if (expand->kmax != rollout->kmax || expand->half != rollout->half || expand->n_levels != rollout->n_levels)
        return fail(-1, "ipp_ctree: the two states differ in their candidate square");
    return 0;
}

int ipp_ctree_descend(const ipp_ctree* ct, const ipp_rollout* expand, const ipp_rollout* rollout, void* stream) {
    if (int rc = ctree_states_check(ct, expand, rollout)) return rc;
    HIP_TRY(hipSetDevice(ct->device));
    hipLaunchKernelGGL(k_ctree_descend, dim3(ct->roots), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *ct, *expand, *rollout);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_ctree_attach(const ipp_ctree* ct, const ipp_rollout* expand, const ipp_rollout* rollout, void* stream) {
    if (int rc = ctree_states_check(ct, expand, rollout)) return rc;
    HIP_TRY(hipSetDevice(ct->device));
    hipLaunchKernelGGL(k_ctree_attach, dim3((ct->roots + kWave - 1) / kWave), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *ct, *expand,
                       *rollout);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_ctree_backup(const ipp_ctree* ct, const ipp_rollout* rollout, void* stream) {
    if (int rc = ctree_check(ct)) return rc;
    if (int rc = ctree_state_check(ct, rollout, "rollout")) return rc;
    HIP_TRY(hipSetDevice(ct->device));
    hipLaunchKernelGGL(k_ctree_backup, dim3((ct->roots + kWave - 1) / kWave), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *ct, *rollout);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_ctree_best(const ipp_ctree* ct, double* action, int32_t* has, void* stream) {
    if (int rc = ctree_check(ct)) return rc;
    if (!action || !has) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(ct->device));
    hipLaunchKernelGGL(k_ctree_best, dim3(ct->roots), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), *ct, action, has);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_ctree_search(void* engine, const ipp_ctree* ct, const ipp_rollout* expand, const ipp_rollout* rollout, void* scratch,
                     uint64_t scratch_bytes, int32_t first_sim, int32_t n_sims, void* stream) {
    if (!engine) return fail(-1, "null engine");
    if (int rc = ctree_states_check(ct, expand, rollout)) return rc;
    TreeEngine e;
    if (int rc = nodes_engine(engine, &e)) return rc;
    if (ct->device != e.device) return fail(-1, "ipp_ctree.device = %d, the engine runs on %d", ct->device, e.device);
    if ((expand->flags | rollout->flags) & ~(uint32_t)(IPP_ADAPTIVE | IPP_USE_FLIGHT_TIME))
        return fail(-1, "unsupported flag bits 0x%x", expand->flags | rollout->flags);
    if (first_sim < 0 || n_sims < 0 || (int64_t)first_sim + n_sims > (int64_t)ct->cap - 1)
        return fail(-1, "simulations [%d, %lld) do not fit cap = %d node slots per root", first_sim, (long long)first_sim + n_sims, ct->cap);
    const int R = ct->roots;
    const int64_t tree_lo = ct->tree_node_base, tree_hi = tree_lo + (int64_t)(ct->cap - 1) * R;
    const int64_t ro_lo = rollout->node_base, ro_hi = ro_lo + (int64_t)R * rollout->max_depth;
    if (tree_hi > (int64_t)e.node_cap || ro_hi > (int64_t)e.node_cap)
        return fail(-1, "tree nodes [%lld, %lld) and rollout nodes [%lld, %lld) exceed node_capacity = %d", (long long)tree_lo, (long long)tree_hi,
                    (long long)ro_lo, (long long)ro_hi, e.node_cap);
    if (ro_lo < tree_hi && tree_lo < ro_hi)
        return fail(-1, "tree nodes [%lld, %lld) and rollout nodes [%lld, %lld) overlap", (long long)tree_lo, (long long)tree_hi, (long long)ro_lo,
                    (long long)ro_hi);
    for (int s = first_sim; s < first_sim + n_sims; ++s) {
        ipp_ctree c = *ct;
        ipp_rollout ex = *expand, ro = *rollout;
        c.tie_u = ct->tie_u + (size_t)s * R * ct->horizon;
        ex.u = expand->u + (size_t)s * R * 2;
        ro.u = rollout->u + (size_t)s * R * ct->horizon * 2;
        ex.node_base = ct->tree_node_base + s * R;
        if (int rc = ipp_ctree_descend(&c, &ex, &ro, stream)) return rc;
        if (int rc = ipp_rollout_candidates(&ex, stream)) return rc;
        if (int rc = ipp_tree_score_nodes(engine, ex.root, ex.path, R, ex.kmax, ex.cand, ex.cur, ex.flags, ex.reward, ex.cost, ex.status, scratch,
                                          scratch_bytes, stream))
            return rc;
        if (int rc = ipp_rollout_pick(&ex, 0, stream)) return rc;
        if (int rc = tree_step_chunks(engine, e.max_batch, ex.root, ex.path, ex.new_id, R, ex.action, ex.cur, ex.flags, ex.step_reward, ex.step_status,
                                      stream))  // the recorded step of every expansion (a NaN action: nothing is applied)
            return rc;
        if (int rc = ipp_ctree_attach(&c, &ex, &ro, stream)) return rc;
        if (int rc = ipp_rollout_run(engine, &ro, scratch, scratch_bytes, stream)) return rc;
        if (int rc = ipp_ctree_backup(&c, &ro, stream)) return rc;
    }
    return 0;
}

}  // extern "C"
