/*
 * nfc_tap_reduce.hip - device kernels of nfcgpu_signal_tap_reduce: the tap's planes reduced over sample ranges. What a unit is,
 * how a lane walks it and how partials merge is nfc_tap_reduce.hpp; this file adds the grid and the butterfly.
 *
 * nfc_tap_reduce_kernel: a wave per unit - (range, segment of 16 384 samples, channel) - grid-stride over the units of the pass,
 * four waves to a workgroup that share nothing. A lane reads its quads with 16-byte loads (the last, short quad of a range
 * sample by sample), keeps (value, index) for min and max, a double sum and a count in registers, the wave combines them in a
 * butterfly and lane 0 writes the unit's partial. nfc_tap_reduce_finish_kernel: a thread per record merges the range's partials
 * in segment order. No LDS, no atomics: the order of every sum is fixed by a sample's offset within its range.
 */
#include <hip/hip_runtime.h>

#include "nfc_tap_reduce.hpp"

namespace {

__device__ __forceinline__ NfcTapPartial nfc_tap_reduce_wave(NfcTapPartial acc)
{
   for (int off = 1; off < 64; off <<= 1)
   {
      NfcTapPartial other;
      other.sum = __shfl_xor(acc.sum, off);
      other.minV = __shfl_xor(acc.minV, off);
      other.maxV = __shfl_xor(acc.maxV, off);
      other.minI = __shfl_xor(acc.minI, off);
      other.maxI = __shfl_xor(acc.maxI, off);
      other.valid = __shfl_xor(acc.valid, off);
      other.pad = 0;
      acc = nfc_tap_partial_merge(acc, other);
   }
   return acc;
}

}

__global__ __launch_bounds__(64 * NfcTapReduceShape::kWaves) void nfc_tap_reduce_kernel(NfcTapReduceArgs A)
{
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t waves = (uint64_t)gridDim.x * NfcTapReduceShape::kWaves;

   for (uint64_t j = (uint64_t)blockIdx.x * NfcTapReduceShape::kWaves + (threadIdx.x >> 6); j < A.units; j += waves)
   {
      const NfcTapPartial acc = nfc_tap_reduce_wave(nfc_tap_reduce_lane(A, j, lane));

      if (lane == 0)
         A.partials[j] = acc;
   }
}

__global__ __launch_bounds__(256) void nfc_tap_reduce_finish_kernel(NfcTapReduceArgs A)
{
   const uint64_t records = A.items * A.channels;

   for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < records; t += (uint64_t)gridDim.x * blockDim.x)
      nfc_tap_reduce_finish(A, t);
}
