// dropout_hash.hpp -- the dropout mask of the fused MlpWorld training step (world_mlp_train.hip), for the host
// (mcn_dropout_mask) and the device alike.  The definition is the comment above mcn_dropout_mask in include/mcn.h: a
// stateless counter hash of (seed, step, layer, slot, unit), so a mask does not depend on how the scenes of a mini-batch
// are dealt to workgroups, and a test can restate it from plain integers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr uint64_t DROPOUT_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int DROPOUT_MAX_WIDTH = 256;      // units of a layer: a slot's units never reach the next slot's counters

__host__ __device__ inline uint64_t dropout_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the key of one mask: one (seed, training step, dropout layer)
__host__ __device__ inline uint64_t dropout_key(uint64_t seed, uint64_t step, int layer)
{
    return dropout_mix(seed + DROPOUT_GOLDEN * (2 * step + (uint64_t)layer + 1));
}

// 24 bits for one unit of one slot (a scene's position in the mini-batch); it is kept where they are below the threshold
__host__ __device__ inline uint32_t dropout_bits(uint64_t key, int slot, int unit)
{
    return (uint32_t)(dropout_mix(key + DROPOUT_GOLDEN * (256 * (uint64_t)slot + (uint64_t)unit + 1)) >> 40);
}

// T = llrint((1 - p) 2^24) for the p that was written (launch.hpp: written_as), 0 <= p < 1
inline uint32_t dropout_threshold(double p) { return (uint32_t)llrint((1.0 - p) * 16777216.0); }

}  // namespace
