// cstr_per.hip -- prioritized experience replay (Schaul et al. 2016, the proportional variant) over the HBM replay ring, gfx950.
//
// THE SUM STRUCTURE IS A RADIX-64 TREE, because a wave is 64 lanes: a node's 64 children are one coalesced 512-byte load, their
// inclusive prefix is a six-step lane scan and "the first child whose prefix exceeds the mass" is one ballot. A sample costs one
// dependent load per level -- four at 2^20 leaves, where the textbook binary tree costs twenty. Level 0 holds the leaves
// (p^alpha, 0 for a slot never written), level l + 1 one node per 64 nodes of level l, up to a single root; every level is float64
// and padded with zeros to a multiple of 64, so a node's load never needs a bound.
//
// A NODE IS ALWAYS THE SUM OF ITS 64 CHILDREN IN ONE FIXED ORDER (node_sum: the xor butterfly 32, 16, .. 1, whose two partners form the
// same commutative sum at every step). Nothing is adjusted incrementally and there are no float atomics: at rest the tree is a pure
// function of its leaves, two waves that recompute the same node store the same bits, and a rebuild gives back what the add and update
// launches left. Levels that depend on each other are separated by a __syncthreads() inside ONE workgroup (add, update) or by a launch
// boundary (rebuild); no workgroup ever waits for a word another one writes.
//
// The launches:
//   rebuild  one launch per level, a wave per node;
//   add      one workgroup: the ring row the launch in front wrote gets max_priority^alpha, its ancestors (one contiguous range per
//            level) are recomputed;
//   sample   a wave per sample: stratified mass, the descent, the gather of the slot's five fields; the launch's last workgroup turns
//            the B probabilities into importance weights and advances the Philox offset;
//   update   one workgroup: new leaves for the sampled slots (of equal indices the largest position wins), max_priority, ancestors.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t PER_STREAM_TAG = 0x9E7A11EDu;  // counter word 3: never shares counters with the other streams
constexpr int WG = 1024;                          // add / update: one workgroup of 16 waves
constexpr int WG_WAVES = WG / 64;
constexpr int CTL_MAX = 0, CTL_SEED = 1, CTL_OFFSET = 2, CTL_TICKET = 3;  // per_ctl words (include/cstr_rl_hip.h)

// the sum of a node's 64 children, one per lane; every lane gets the same bits
__device__ __forceinline__ double node_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// inclusive prefix over the wave, lanes ascending (Hillis-Steele: offsets 1, 2, .. 32)
__device__ __forceinline__ double lane_prefix(double v, const int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ double ctl_f64(const uint64_t *per_ctl, int w) { return __longlong_as_double((long long)per_ctl[w]); }

// nodes lo .. hi (inclusive) of level l from their children, a wave per node, the workgroup's waves in turn
__device__ __forceinline__ void recompute_nodes(const cstr_per_tree_t &t, const int l, const int64_t lo, const int64_t hi)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const double *__restrict__ child = t.node + t.offset[l - 1];
    double *__restrict__ parent = t.node + t.offset[l];
    for (int64_t n = lo + wave; n <= hi; n += waves) {
        const double s = node_sum(child[n * 64 + lane]);
        if (lane == 0) parent[n] = s;
    }
}

__global__ __launch_bounds__(256) void per_level_kernel(const double *__restrict__ child, double *__restrict__ parent, const int64_t n_parent)
{
    const int lane = threadIdx.x & 63;
    for (int64_t n = blockIdx.x * 4ll + (threadIdx.x >> 6); n < n_parent; n += (int64_t)gridDim.x * 4ll) {
        const double s = node_sum(child[n * 64 + lane]);
        if (lane == 0) parent[n] = s;
    }
}

__global__ __launch_bounds__(WG) void per_add_kernel(const cstr_per_tree_t t, const int64_t *__restrict__ ring_ctl, const int64_t rows,
                                                     const int64_t n_envs, const uint64_t *__restrict__ per_ctl, const double alpha)
{
    int64_t row = ring_ctl[0] - 1;  // the launch in front advanced pos past the row it wrote
    if (row < 0) row += rows;
    row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);  // a broken control word must not leave the tree
    const double v = pow(ctl_f64(per_ctl, CTL_MAX), alpha);
    int64_t lo = row * n_envs, hi = lo + n_envs - 1;
    for (int64_t i = lo + threadIdx.x; i <= hi; i += WG) t.node[i] = v;
    for (int l = 1; l < t.n_levels; ++l) {
        __syncthreads();  // level l - 1 is complete
        lo >>= 6;
        hi >>= 6;
        recompute_nodes(t, l, lo, hi);
    }
}

__global__ __launch_bounds__(WG) void per_update_kernel(const cstr_per_tree_t t, uint64_t *__restrict__ per_ctl,
                                                        const int64_t *__restrict__ leaf_idx, const float *__restrict__ td_abs,
                                                        const int batch, const double alpha, const double min_priority)
{
    __shared__ int32_t s_leaf[CSTR_PER_MAX_BATCH];
    __shared__ double s_max[WG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double max_p = ctl_f64(per_ctl, CTL_MAX);
    int32_t leaf = -1;  // an index outside the tree is skipped
    double v = max_p, seen = 0.0;
    if (tid < batch) {
        const int64_t i = leaf_idx[tid];
        if (i >= 0 && i < t.capacity) leaf = (int32_t)i;
        const double a = (double)fabsf(td_abs[tid]);
        if (a < (double)INFINITY) {  // false for a NaN: a non-finite error takes the current max_priority and does not raise it
            v = a + min_priority;
            if (leaf >= 0) seen = v;
        }
    }
    s_leaf[tid] = leaf;
    seen = wave_max(seen);
    if (lane == 0) s_max[wave] = seen;
    __syncthreads();
    bool wins = leaf >= 0;  // of several positions with one leaf the largest wins (the sequential loop's last write)
    for (int j = tid + 1; j < batch && wins; ++j) wins = s_leaf[j] != leaf;
    if (wins) t.node[leaf] = pow(v, alpha);
    if (tid == 0) {
        double m = max_p;
        for (int w = 0; w < WG_WAVES; ++w) m = fmax(m, s_max[w]);
        per_ctl[CTL_MAX] = (uint64_t)__double_as_longlong(m);
    }
    for (int l = 1; l < t.n_levels; ++l) {
        __syncthreads();  // level l - 1 is complete
        const int sh = 6 * l;
        for (int j = wave; j < batch; j += WG_WAVES) {  // wave-uniform: position j's ancestor; equal neighbours leave it to the last
            const int32_t a = s_leaf[j], b = j + 1 < batch ? s_leaf[j + 1] : -1;
            if (a < 0 || (b >= 0 && (b >> sh) == (a >> sh))) continue;
            const int64_t n = a >> sh;
            const double s = node_sum(t.node[t.offset[l - 1] + n * 64 + lane]);
            if (lane == 0) t.node[t.offset[l] + n] = s;  // another wave on the same node stores the same bits
        }
    }
}

struct SampleOut {
    float *obs, *act, *next_obs, *done, *rew, *weight;
    int64_t *leaf;
    unsigned long long *prob;  // double [B]: P_j, handed to the last workgroup through agent-scope stores
};

// One wave per sample and per workgroup: the launch is a chain of dependent loads, so it is spread over as many CUs as there are samples.
__global__ __launch_bounds__(64) void per_sample_kernel(const cstr_ring_t ring, const int64_t *__restrict__ ring_ctl, const cstr_per_tree_t t,
                                                        uint64_t *__restrict__ per_ctl, const double *__restrict__ beta,
                                                        const float *__restrict__ u_in, const int batch, const SampleOut out)
{
    const int lane = threadIdx.x, j = blockIdx.x;
    const bool draw = u_in == nullptr;  // teacher-forced uniforms are read, otherwise PER's own Philox stream is drawn from
    const uint64_t seed = draw ? per_ctl[CTL_SEED] : 0ull, base = draw ? per_ctl[CTL_OFFSET] : 0ull;
    float u;
    if (draw) {
        const uint64_t ctr = base + (uint64_t)j;
        uint32_t x[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, PER_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        u = philox_uniform(x[0]);
    } else {
        u = u_in[j];
    }
    const double total = t.node[t.offset[t.n_levels - 1]];
    double mass = ((double)j + (double)u) * total / (double)batch;  // the j-th of B equal strata
    int64_t node = 0;
    double p = total;
    for (int l = t.n_levels - 1; l >= 1; --l) {
        const double c = t.node[t.offset[l - 1] + node * 64 + lane];
        const double pre = lane_prefix(c, lane);
        const unsigned long long over = __ballot(pre > mass);
        int pick;
        if (over) {
            pick = __ffsll(over) - 1;  // pre[pick - 1] <= mass < pre[pick]: the child is non-zero
        } else {  // rounding left the mass at or beyond the node's sum: the last non-zero child
            const unsigned long long nz = __ballot(c > 0.0);
            pick = nz ? 63 - __clzll(nz) : 0;
        }
        const double below = __shfl(pre, pick > 0 ? pick - 1 : 0);
        mass -= pick > 0 ? below : 0.0;
        p = __shfl(c, pick);
        node = node * 64 + pick;
    }
    // the slot's five fields, as replay_sample_kernel writes them (core/common/buffers.py:316-323), lanes sharing the words
    const int D = ring.obs_dim, A = ring.act_dim;
    if (lane < D) out.obs[(int64_t)j * D + lane] = ring.obs[node * D + lane];
    else if (lane >= 8 && lane < 8 + D) out.next_obs[(int64_t)j * D + lane - 8] = ring.next_obs[node * D + lane - 8];
    else if (lane >= 16 && lane < 16 + A) out.act[(int64_t)j * A + lane - 16] = ring.act[node * A + lane - 16];
    else if (lane == 24) out.done[j] = ring.done[node] * (1.0f - ring.timeout[node]);
    else if (lane == 25) out.rew[j] = ring.rew[node];
    else if (lane == 26) out.leaf[j] = node;
    else if (lane == 27) publish_f64(out.prob + j, p / total);
    __threadfence();  // release: P_j is visible chip-wide before this workgroup's ticket is
    if (!last_block_ticket(reinterpret_cast<unsigned long long *>(per_ctl + CTL_TICKET))) return;
    __threadfence();  // acquire
    // w_j = (N P_j)^-beta / max_j (N P_j)^-beta, N the filled slots; float64 throughout, one rounding to float32
    const double n_filled = (double)((ring_ctl[1] ? ring.rows : ring_ctl[0]) * ring.n_envs), nb = -beta[0];
    double best = 0.0;
    for (int k = lane; k < batch; k += 64) best = fmax(best, pow(n_filled * consume_f64(out.prob + k), nb));
    best = wave_max(best);
    for (int k = lane; k < batch; k += 64) out.weight[k] = (float)(pow(n_filled * consume_f64(out.prob + k), nb) / best);
    if (draw && lane == 0) per_ctl[CTL_OFFSET] = base + (uint64_t)batch;
}

// the levels of a tree over `capacity` leaves; false: the capacity is out of range
inline bool layout_of(const int64_t capacity, cstr_per_tree_t &t)
{
    if (capacity < 1 || capacity > CSTR_PER_MAX_CAPACITY) return false;
    t.capacity = capacity;
    t.reserved = 0;
    int l = 0;
    int64_t n = capacity, off = 0;
    for (;;) {
        t.count[l] = n;
        t.offset[l] = off;
        off += (n + 63) / 64 * 64;
        ++l;
        if (l > 1 && n == 1) break;
        n = (n + 63) / 64;
    }
    t.n_levels = l;
    t.words = off;
    for (; l < CSTR_PER_MAX_LEVELS; ++l) t.count[l] = t.offset[l] = 0;
    return true;
}

// a tree struct is taken only if it is exactly the layout of its capacity: no offset of the caller's reaches a kernel unchecked
inline int tree_check(const cstr_per_tree_t *t)
{
    if (!t || !t->node || !aligned8(t->node)) return CSTR_E_BADARG;
    cstr_per_tree_t want;
    if (!layout_of(t->capacity, want)) return t->capacity < 1 ? CSTR_E_BADARG : CSTR_E_UNSUPPORTED;
    if (t->n_levels != want.n_levels || t->words != want.words) return CSTR_E_BADARG;
    for (int l = 0; l < CSTR_PER_MAX_LEVELS; ++l)
        if (t->offset[l] != want.offset[l] || t->count[l] != want.count[l]) return CSTR_E_BADARG;
    return CSTR_OK;
}

inline bool alpha_ok(double alpha) { return alpha >= 0.0 && alpha < (double)INFINITY; }

}  // namespace

extern "C" int cstr_per_tree_layout(int64_t capacity, cstr_per_tree_t *tree)
{
    if (!tree || capacity < 1) return CSTR_E_BADARG;
    double *keep = tree->node;
    if (!layout_of(capacity, *tree)) return CSTR_E_UNSUPPORTED;
    tree->node = keep;
    return CSTR_OK;
}

extern "C" int cstr_per_rebuild_f64(const cstr_per_tree_t *tree, cstr_stream_t stream)
{
    const int rc = tree_check(tree);
    if (rc) return rc;
    for (int l = 1; l < tree->n_levels; ++l) {
        const int64_t n = tree->count[l];
        per_level_kernel<<<lane_grid(n, 4, 65536), 256, 0, (hipStream_t)stream>>>(tree->node + tree->offset[l - 1], tree->node + tree->offset[l], n);
        const int err = (int)hipGetLastError();
        if (err) return err;
    }
    return CSTR_OK;
}

extern "C" int cstr_per_add_f64(const cstr_per_tree_t *tree, const int64_t *ring_ctl, int64_t rows, int64_t n_envs, const uint64_t *per_ctl,
                                double alpha, cstr_stream_t stream)
{
    const int rc = tree_check(tree);
    if (rc) return rc;
    if (!ring_ctl || !per_ctl || rows < 1 || n_envs < 1 || !alpha_ok(alpha)) return CSTR_E_BADARG;
    if (rows > tree->capacity || n_envs > tree->capacity || rows * n_envs != tree->capacity) return CSTR_E_BADARG;
    if (!aligned8(ring_ctl) || !aligned8(per_ctl)) return CSTR_E_BADARG;
    {
        const Buf ins[2] = {{ring_ctl, 2 * CSTR_RING_CTL_WORDS}, {per_ctl, 2 * CSTR_PER_CTL_WORDS}};
        const Buf outs[1] = {{tree->node, 2 * tree->words}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    per_add_kernel<<<1, WG, 0, (hipStream_t)stream>>>(*tree, ring_ctl, rows, n_envs, per_ctl, alpha);
    return (int)hipGetLastError();
}

extern "C" int cstr_per_update_f64(const cstr_per_tree_t *tree, uint64_t *per_ctl, const int64_t *leaf_idx, const float *td_abs, int64_t batch,
                                   double alpha, double min_priority, cstr_stream_t stream)
{
    const int rc = tree_check(tree);
    if (rc) return rc;
    if (!per_ctl || !leaf_idx || !td_abs || batch < 1 || !alpha_ok(alpha) || !(min_priority > 0.0) || !(min_priority < (double)INFINITY))
        return CSTR_E_BADARG;
    if (batch > CSTR_PER_MAX_BATCH) return CSTR_E_UNSUPPORTED;
    if (!aligned8(per_ctl) || !aligned8(leaf_idx) || !aligned4(td_abs)) return CSTR_E_BADARG;
    {
        const Buf ins[2] = {{leaf_idx, 2 * batch}, {td_abs, batch}};
        const Buf outs[2] = {{tree->node, 2 * tree->words}, {per_ctl, 2 * CSTR_PER_CTL_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    per_update_kernel<<<1, WG, 0, (hipStream_t)stream>>>(*tree, per_ctl, leaf_idx, td_abs, (int)batch, alpha, min_priority);
    return (int)hipGetLastError();
}

extern "C" int cstr_per_sample_f32(const cstr_ring_t *ring, const int64_t *ring_ctl, const cstr_per_tree_t *tree, uint64_t *per_ctl,
                                   const double *beta, const float *u_in, int64_t batch, float *out_obs, float *out_act,
                                   float *out_next_obs, float *out_done, float *out_rew, int64_t *leaf_out, double *prob_out, float *weight_out,
                                   cstr_stream_t stream)
{
    if (!ring || !ring->obs || !ring->next_obs || !ring->act || !ring->rew || !ring->done || !ring->timeout) return CSTR_E_BADARG;
    const int rc = tree_check(tree);
    if (rc) return rc;
    if (!ring_ctl || !per_ctl || !beta || !out_obs || !out_act || !out_next_obs || !out_done || !out_rew || !leaf_out || !prob_out ||
        !weight_out || batch < 1)
        return CSTR_E_BADARG;
    const bool lay_ok = (ring->obs_dim == 4 && ring->act_dim == 2) || (ring->obs_dim == 8 && (ring->act_dim == 2 || ring->act_dim == 4));
    if (!lay_ok) return CSTR_E_UNSUPPORTED;
    if (batch > CSTR_PER_MAX_BATCH) return CSTR_E_UNSUPPORTED;
    if (ring->rows < 1 || ring->n_envs < 1 || ring->rows > tree->capacity || ring->n_envs > tree->capacity ||
        ring->rows * ring->n_envs != tree->capacity)
        return CSTR_E_BADARG;
    if (!aligned4(ring->obs) || !aligned4(ring->next_obs) || !aligned4(ring->act) || !aligned4(ring->rew) || !aligned4(ring->done) ||
        !aligned4(ring->timeout) || !aligned8(ring_ctl) || !aligned8(per_ctl) || !aligned8(beta) || (u_in && !aligned4(u_in)) ||
        !aligned4(out_obs) || !aligned4(out_act) || !aligned4(out_next_obs) || !aligned4(out_done) || !aligned4(out_rew) ||
        !aligned8(leaf_out) || !aligned8(prob_out) || !aligned4(weight_out))
        return CSTR_E_BADARG;
    {
        const int64_t B = batch, C = tree->capacity, D = ring->obs_dim, A = ring->act_dim;
        const Buf ins[10] = {{ring->obs, C * D}, {ring->next_obs, C * D}, {ring->act, C * A}, {ring->rew, C}, {ring->done, C},
                             {ring->timeout, C}, {ring_ctl, 2 * CSTR_RING_CTL_WORDS}, {tree->node, 2 * tree->words}, {beta, 2}, {u_in, B}};
        const Buf outs[9] = {{out_obs, B * D}, {out_act, B * A}, {out_next_obs, B * D}, {out_done, B}, {out_rew, B},
                             {leaf_out, 2 * B}, {prob_out, 2 * B}, {weight_out, B}, {per_ctl, 2 * CSTR_PER_CTL_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    const SampleOut out = {out_obs, out_act, out_next_obs, out_done, out_rew, weight_out, leaf_out, reinterpret_cast<unsigned long long *>(prob_out)};
    per_sample_kernel<<<(unsigned)batch, 64, 0, (hipStream_t)stream>>>(*ring, ring_ctl, *tree, per_ctl, beta, u_in, (int)batch, out);
    return (int)hipGetLastError();
}
