// cstr_goal_device.h -- device functions of the goal-conditioned face of the CSTR env (internal, included by cstr_her.hip and by the
// goal instantiations of the evaluation kernel in cstr_eval.hip): the desired goal of a raw target, the goal reward, the flat
// [achieved | desired | observation] row and the counter-based target redraw. One statement of each, so that the step-by-step launch
// and the whole-episode launch cannot drift apart. Every TU that includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t HER_GOAL_TAG = 0x90A17A67u;  // counter word 3 of the target redraw: shares no counters with the other streams

// desired_goal of a raw target: the observation's own affine map of C2 (twoseriescstr.py:131), f32
__device__ __forceinline__ float goal_of_target(const cstr_coef_t &k, const float target) { return 2.0f * (target - k.s_lo[2]) / k.s_span[2] - 1.0f; }

// GoalEnv reward = the reference's concentration term (twoseriescstr.py:288-291) on (achieved, desired), both normalised
__device__ __forceinline__ float goal_reward(const float s_lo2, const float s_span2, const float conc_span, const float ag, const float dg)
{
    const float C2 = s_lo2 + (ag + 1.0f) * s_span2 / 2.0f;
    const float T = s_lo2 + (dg + 1.0f) * s_span2 / 2.0f;
    const float ne = fabsf(C2 - T) / conc_span;
    return -5.0f * (ne * ne) - 2.0f * ne;
}

// flat row [achieved_goal | desired_goal | observation]: six floats, 8-byte aligned
__device__ __forceinline__ void store_row6(float *p, const int64_t i, const float dg, const float o[4])
{
    float2 *q = reinterpret_cast<float2 *>(p + 6 * i);
    q[0] = make_float2(o[2], dg);
    q[1] = make_float2(o[0], o[1]);
    q[2] = make_float2(o[2], o[3]);
}

struct GoalDraw { uint64_t seed; int64_t index_offset; float lo, hi; int32_t *episode; };

// raw target of env i's episode of ordinal e: counter (env index [64 bit], episode ordinal, tag), key = goal seed
__device__ __forceinline__ float goal_draw_target(const GoalDraw &gd, const int64_t i, const int32_t e)
{
    const uint64_t idx = (uint64_t)(gd.index_offset + i);
    uint32_t x[4];
    philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)e, HER_GOAL_TAG, (uint32_t)gd.seed, (uint32_t)(gd.seed >> 32), x);
    const float u = (float)(x[0] >> 8) * (1.0f / 16777216.0f);
    return gd.lo + (gd.hi - gd.lo) * u;
}

}  // namespace
